// skat_math.hpp -- pgh_skat_p_from_lambda: the survival function of Q = sum_k lambda_k chi^2_1 at q, by the saddlepoint
// approximation of Kuonen (1999) in the Barndorff-Nielsen form (the definition is in include/pgenhip.h).  Plain host
// C++ that includes nothing of the project; every value is FP64.
#pragma once

#include <cmath>
#include <cstdint>

namespace pgh {

enum : uint8_t { kSkatPNone = 0, kSkatPExact = 1, kSkatPSaddle = 2, kSkatPNearMean = 3, kSkatPFailed = 4 };

// The upper tail of the standard normal.
inline double SkatPhibar(double x) {
	return 0.5 * std::erfc(x * 0.70710678118654752440);
}

// K'(s) and K''(s) of Q's cumulant generating function K(s) = -1/2 sum ln(1 - 2 s lambda_k).
inline void SkatCgfDerivs(const double *lambda, uint32_t n, double s, double *k1, double *k2) {
	double a = 0.0, b = 0.0;
	for (uint32_t i = 0; i < n; i++) {
		const double t = lambda[i] / (1.0 - 2.0 * s * lambda[i]);
		a += t;
		b += 2.0 * t * t;
	}
	*k1 = a;
	*k2 = b;
}

// lambda: the n used eigenvalues (all positive).  *state (may be null): kSkatP*.
inline double SkatPFromLambda(double q, const double *lambda, uint32_t n, uint8_t *state) {
	uint8_t st_local;
	uint8_t &st = state ? *state : st_local;
	st = kSkatPFailed;
	if (!lambda || n == 0 || !std::isfinite(q)) {
		return NAN;
	}
	double mu = 0.0, s2 = 0.0, s3 = 0.0, lmax = 0.0;
	for (uint32_t i = 0; i < n; i++) {
		const double l = lambda[i];
		if (!std::isfinite(l) || !(l > 0.0)) {
			return NAN;
		}
		mu += l;
		s2 += l * l;
		s3 += l * l * l;
		lmax = l > lmax ? l : lmax;
	}
	if (q <= 0.0) {
		return q == 0.0 ? 1.0 : NAN;
	}
	if (n == 1) {
		st = kSkatPExact;
		return std::erfc(std::fabs(std::sqrt(q / lambda[0])) * 0.70710678118654752440); // GlmPFromZ (glm_math.hpp), to the bit
	}
	const double k2 = 2.0 * s2, k3 = 8.0 * s3;
	if (!std::isfinite(mu) || !std::isfinite(k2) || !std::isfinite(k3)) {
		return NAN;
	}
	if (std::fabs(q - mu) <= 1e-3 * std::sqrt(k2)) {
		const double p = SkatPhibar(k3 / (6.0 * k2 * std::sqrt(k2)));
		if (std::isfinite(p)) {
			st = kSkatPNearMean;
			return p;
		}
		return NAN;
	}
	// the root of K'(s) = q: K' increases, the root has the sign of q - mu
	const bool up = q > mu;
	double lo = up ? 0.0 : -INFINITY, hi = up ? 0.5 / lmax : 0.0; // hi is never reached when up
	double limit = 1.0 / std::sqrt(k2);
	double s = (q - mu) / k2; // the Newton step from 0
	if (up) {
		if (s >= hi) {
			s = 0.5 * hi;
		}
	} else if (-s > limit) {
		s = -limit;
		limit *= 2.0;
	}
	bool found = false;
	double kd1 = 0.0, kd2 = 0.0;
	for (int eval = 0; eval < 100; eval++) {
		SkatCgfDerivs(lambda, n, s, &kd1, &kd2);
		const double f = kd1 - q;
		if (!std::isfinite(f) || !std::isfinite(kd2) || !(kd2 > 0.0)) {
			return NAN;
		}
		if (f > 0.0) {
			hi = s;
		} else {
			lo = s;
		}
		double next = s - f / kd2;
		if (lo == -INFINITY) { // (then f > 0 and next < s)
			if (s - next > limit) {
				next = s - limit;
				limit *= 2.0;
			}
		} else if (next <= lo) {
			next = 0.5 * (s + lo);
		} else if (next >= hi) {
			next = 0.5 * (s + hi);
		}
		const double step = std::fabs(next - s);
		s = next;
		if (step <= 1e-12 * std::fabs(s)) {
			found = true;
			break;
		}
	}
	if (!found || !std::isfinite(s) || s == 0.0) {
		return NAN;
	}
	double cgf = 0.0;
	for (uint32_t i = 0; i < n; i++) {
		cgf += std::log1p(-2.0 * s * lambda[i]);
	}
	cgf *= -0.5;
	SkatCgfDerivs(lambda, n, s, &kd1, &kd2);
	const double w2 = 2.0 * (s * q - cgf);
	if (!std::isfinite(w2) || !(w2 > 0.0) || !std::isfinite(kd2) || !(kd2 > 0.0)) {
		return NAN;
	}
	const double omega = s > 0.0 ? std::sqrt(w2) : -std::sqrt(w2);
	const double nu = s * std::sqrt(kd2);
	const double ratio = nu / omega;
	if (!std::isfinite(ratio) || !(ratio > 0.0)) {
		return NAN;
	}
	const double p = SkatPhibar(omega + std::log(ratio) / omega);
	if (!std::isfinite(p)) {
		return NAN;
	}
	st = kSkatPSaddle;
	return p;
}

} // namespace pgh
