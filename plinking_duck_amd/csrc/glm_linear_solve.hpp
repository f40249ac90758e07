// glm_linear_solve.hpp -- the OLS of one variant from its sums: the decisions and the arithmetic of the linear fit,
// shared by GlmLinearSolveKernel (glm.hip) and GlmSparseMultiSolveKernel (glm_sparse_multi.hip).  Device code only.
#pragma once

#include "../../include/pgenhip.h"
#include "glm_math.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace pgh {

constexpr int kGlmSolveMaxP = 22; // intercept + genotype + PGH_GLM_MAX_COVAR

__device__ inline int PackIdx(int a, int b, int q) { // a <= b < q
	return a * q - a * (a - 1) / 2 + (b - a);
}

__device__ inline void SetRowNull(pgh_glm_row &r) {
	r.beta = r.se = r.stat = r.p = r.a1_freq = NAN;
	r.obs_ct = 0;
	r.errcode = PGH_GLM_OK;
	r.firth = 0;
	r.pad[0] = r.pad[1] = 0;
}

// The row of one variant.  s = {n, sum x, sum x^2, sum x y, sum x z_j (j < k)} over the variant's samples N (raw x);
// gm(e): entry e of the packed upper Gram of u = [1, z_1..z_k, y] over N.  FLAGGED: CONST_ALLELE is the caller's
// x_const, otherwise GlmConstant's (k == 0: the closed form's own test).  In order: TOO_FEW_SAMPLES, CONST_ALLELE,
// SINGULAR_MATRIX (the 1e-10 pivot rule; no rule at k == 0), ZERO_VARIANCE with beta filled, or the fitted row.
template <bool FLAGGED, class GramAt>
__device__ inline pgh_glm_row GlmLinearSolveRow(const double *s, uint32_t k, GramAt gm, bool x_const) {
	const uint32_t q = k + 2;
	pgh_glm_row r;
	SetRowNull(r);
	const double n = s[0];
	const int p = static_cast<int>(k) + 2;
	r.obs_ct = static_cast<uint32_t>(n);
	if (n < p + 1) {
		r.errcode = PGH_GLM_TOO_FEW_SAMPLES;
		return r;
	}
	r.a1_freq = s[1] / (2.0 * n);
	// with no covariates the reference takes its one-pass closed form, and its test with it
	bool constant;
	if constexpr (FLAGGED) {
		constant = x_const;
	} else {
		constant = k ? GlmConstant(n, s[1], s[2]) : s[2] - s[1] * s[1] / n < 1e-20;
	}
	if (constant) {
		r.errcode = PGH_GLM_CONST_ALLELE;
		return r;
	}
	// augmented matrix, order [1, z_1..z_k, x, y]; u = [1, z, y] is the Gram's order
	constexpr int M = kGlmSolveMaxP + 1;
	double a[M * M];
	const int xi = p - 1, yi = p;
	auto uidx = [&](int j) { return j <= static_cast<int>(k) ? j : yi; }; // u index -> matrix index
	for (int ua = 0; ua < static_cast<int>(q); ua++) {
		for (int ub = ua; ub < static_cast<int>(q); ub++) {
			const int e = PackIdx(ua, ub, q);
			const double val = gm(e);
			const int ia = uidx(ua), ib = uidx(ub);
			a[ib * M + ia] = val; // lower triangle: ib >= ia
		}
	}
	a[xi * M + 0] = s[1];
	for (int j = 0; j < static_cast<int>(k); j++) {
		a[xi * M + 1 + j] = s[4 + j];
	}
	a[xi * M + xi] = s[2];
	a[yi * M + xi] = s[3];
	if (!GlmCholesky(a, p, M, k ? 1e-10 : 0.0, nullptr)) {
		r.errcode = PGH_GLM_SINGULAR_MATRIX;
		return r;
	}
	double rss = a[yi * M + yi];
	for (int j = 0; j < p; j++) {
		double l = a[yi * M + j];
		for (int t = 0; t < j; t++) {
			l -= a[yi * M + t] * a[j * M + t];
		}
		l /= a[j * M + j];
		a[yi * M + j] = l;
		rss -= l * l;
	}
	rss = rss < 0.0 ? 0.0 : rss;
	const double lxx = a[xi * M + xi];
	const double df = n - p;
	const double se2 = rss / df / (lxx * lxx);
	const double beta = a[yi * M + xi] / lxx;
	r.beta = beta;
	if (se2 < 1e-30) {
		r.errcode = PGH_GLM_ZERO_VARIANCE;
		return r;
	}
	r.se = sqrt(se2);
	r.stat = beta / r.se;
	r.p = GlmPFromT(r.stat, df);
	return r;
}

} // namespace pgh
