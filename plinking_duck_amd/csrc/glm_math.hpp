// glm_math.hpp -- the small dense arithmetic of plink_glm, shared by the host and the device (glm.hip, api_glm.cpp):
// two-sided p-values of a t or z statistic, an in-place Cholesky factor of a symmetric p x p matrix and the exact
// CONST_ALLELE test.
// Written from the textbook definitions; every value is FP64.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace pgh {

#define PGH_GLM_HD __host__ __device__ inline

// Lentz's continued fraction of the regularised incomplete beta I_x(a, b) (valid for x < (a+1)/(a+b+2)):
// returns the fraction; the caller multiplies by x^a (1-x)^b / (a B(a, b)).
PGH_GLM_HD double GlmBetaCf(double a, double b, double x) {
	const double tiny = 1e-300, eps = 1e-16;
	double c = 1.0, d = 1.0 - (a + b) * x / (a + 1.0);
	if (fabs(d) < tiny) {
		d = tiny;
	}
	d = 1.0 / d;
	double f = d;
	for (int m = 1; m <= 200000; m++) {
		const double m2 = 2.0 * m;
		double num = m * (b - m) * x / ((a + m2 - 1.0) * (a + m2));
		d = 1.0 + num * d;
		d = fabs(d) < tiny ? tiny : d;
		c = 1.0 + num / c;
		c = fabs(c) < tiny ? tiny : c;
		d = 1.0 / d;
		f *= d * c;
		num = -(a + m) * (a + b + m) * x / ((a + m2) * (a + m2 + 1.0));
		d = 1.0 + num * d;
		d = fabs(d) < tiny ? tiny : d;
		c = 1.0 + num / c;
		c = fabs(c) < tiny ? tiny : c;
		d = 1.0 / d;
		const double del = d * c;
		f *= del;
		if (fabs(del - 1.0) < eps) {
			break;
		}
	}
	return f;
}

// I_x(a, b) with y = 1 - x given separately (so that x close to 1 keeps its precision)
PGH_GLM_HD double GlmBetaInc(double a, double b, double x, double y) {
	if (x <= 0.0) {
		return 0.0;
	}
	if (y <= 0.0) {
		return 1.0;
	}
	const double lbeta = lgamma(a + b) - lgamma(a) - lgamma(b);
	const double front = exp(lbeta + a * log1p(-y) + b * log(y));
	if (x < (a + 1.0) / (a + b + 2.0)) {
		return front * GlmBetaCf(a, b, x) / a;
	}
	return 1.0 - front * GlmBetaCf(b, a, y) / b;
}

// two-sided p of Student's t with df degrees of freedom: I_{df/(df+t^2)}(df/2, 1/2)
PGH_GLM_HD double GlmPFromT(double t, double df) {
	if (t != t || !(df > 0.0)) {
		return NAN;
	}
	const double tt = t * t;
	if (tt == INFINITY) {
		return 0.0;
	}
	const double den = df + tt;
	return GlmBetaInc(0.5 * df, 0.5, df / den, tt / den);
}

// two-sided p of a standard normal z
PGH_GLM_HD double GlmPFromZ(double z) {
	if (z != z) {
		return NAN;
	}
	return erfc(fabs(z) * 0.70710678118654752440);
}

// In-place lower Cholesky factor of the leading n x n block of the symmetric matrix a (row-major, stride ld; the
// lower triangle is read and overwritten).  Returns false when a pivot is not positive or falls below rel_tol times
// its original diagonal entry (the matrix is treated as singular).  log_det (may be null) receives ln det.
PGH_GLM_HD bool GlmCholesky(double *a, int n, int ld, double rel_tol, double *log_det) {
	double ld_sum = 0.0;
	for (int j = 0; j < n; j++) {
		const double orig = a[j * ld + j];
		double d = orig;
		for (int k = 0; k < j; k++) {
			d -= a[j * ld + k] * a[j * ld + k];
		}
		if (!(d > 0.0) || d <= rel_tol * fabs(orig)) {
			return false;
		}
		const double l = sqrt(d);
		a[j * ld + j] = l;
		ld_sum += 2.0 * log(l);
		const double inv = 1.0 / l;
		for (int i = j + 1; i < n; i++) {
			double s = a[i * ld + j];
			for (int k = 0; k < j; k++) {
				s -= a[i * ld + k] * a[j * ld + k];
			}
			a[i * ld + j] = s * inv;
		}
	}
	if (log_det) {
		*log_det = ld_sum;
	}
	return true;
}

// Solve L L^T x = b in place (l: lower factor from GlmCholesky)
PGH_GLM_HD void GlmCholSolve(const double *l, int n, int ld, double *b) {
	for (int i = 0; i < n; i++) {
		double s = b[i];
		for (int k = 0; k < i; k++) {
			s -= l[i * ld + k] * b[k];
		}
		b[i] = s / l[i * ld + i];
	}
	for (int i = n - 1; i >= 0; i--) {
		double s = b[i];
		for (int k = i + 1; k < n; k++) {
			s -= l[k * ld + i] * b[k];
		}
		b[i] = s / l[i * ld + i];
	}
}

// Full symmetric inverse from the lower factor: inv (n x n, stride ld) = (L L^T)^-1.  col: n doubles of workspace.
PGH_GLM_HD void GlmCholInverse(const double *l, int n, int ld, double *inv, double *col) {
	for (int c = 0; c < n; c++) {
		for (int i = 0; i < n; i++) {
			col[i] = i == c ? 1.0 : 0.0;
		}
		GlmCholSolve(l, n, ld, col);
		for (int i = 0; i < n; i++) {
			inv[i * ld + c] = col[i];
		}
	}
}

// CONST_ALLELE where the reference uses its two-pass variance sum (x - mean)^2 < 1e-20 (the multivariate linear and
// the logistic fits).  Calls and dosages (value / 16384) lie on the 2^-14 grid in [0, 2], so n, sum x and sum x^2
// are exact sums (sum x^2 while n < 2^23; for calls always), and a used set that is not constant has a variance sum
// of at least 2^-28 (1 - 1/n) > 1e-20.  The rule is therefore "every used x is equal", which is n sum x^2 == (sum x)^2
// (Cauchy-Schwarz: > otherwise).  Both products are compared exactly, each as an fma two-product (hi + lo).  The
// one-pass sum x^2 - (sum x)^2 / n is not enough: for a constant dosage it can round to a positive number (2.3e-13 for
// 20,001 samples at 4915 / 16384).
PGH_GLM_HD bool GlmConstant(double n, double sx, double sxx) {
	const double a = n * sxx, a_lo = fma(n, sxx, -a);
	const double b = sx * sx, b_lo = fma(sx, sx, -b);
	return a < b || (a == b && a_lo <= b_lo);
}

#undef PGH_GLM_HD

} // namespace pgh
