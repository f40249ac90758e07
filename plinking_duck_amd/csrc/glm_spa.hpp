// glm_spa.hpp -- the saddlepoint arithmetic that GlmScoreSpaKernel (glm_score_spa.hip) and GlmScoreDenseSpaKernel
// (glm_score_dense_spa.hip) share: pi, K, the safeguarded Newton step, a tail, and phase B, the iteration of one team
// over its stash of (g, mu) pairs (the contract is pgh_glm_score_sparse_spa's in include/pgenhip.h).
#pragma once

#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kSpaMaxEval = 64;        // evaluations of K', K'' per row (both tails in one)
constexpr double kSpaStop = 1e-12;     // |delta s| sqrt(V) at which a root is taken
constexpr double kSpaUlps = 0x1p-50;   // ... or |delta s| / |s|

// pi = mu e^x / (1 - mu + mu e^x) and 1 - pi from one exp of a non-positive argument.
__device__ __forceinline__ void SpaPi(double x, double mu, double *pi, double *qi) {
	const double a = exp(-fabs(x)), nu = 1.0 - mu;
	const double np = x > 0.0 ? mu : mu * a, nq = x > 0.0 ? nu * a : nu;
	const double inv = 1.0 / (np + nq);
	*pi = np * inv;
	*qi = nq * inv;
}

// ln(1 - mu + mu e^x) - mu x
__device__ __forceinline__ double SpaK(double x, double mu) {
	const double m = x > 0.0 ? 1.0 - mu : mu;
	return (x > 0.0 ? x : 0.0) + log1p(m * expm1(-fabs(x))) - mu * x;
}

// One tail's iteration for the root u > 0 of F(u) = |U|, F increasing, F(0) = 0.
struct SpaRoot {
	double u, lo, hi, grow;
	bool done;
};

// F and F' at r->u are known: the bracket, then the next u.  Returns false when a value is not finite.
__device__ __forceinline__ bool SpaStep(SpaRoot *r, double f, double fp, double q, double tol) {
	if (r->done) {
		return true;
	}
	if (!(fabs(f) < INFINITY) || !(fabs(fp) < INFINITY)) {
		return false;
	}
	if (f < q) {
		r->lo = r->u;
	} else {
		r->hi = r->u;
	}
	double un = r->u + (q - f) / fp;
	if (r->hi == INFINITY) {
		if (!(un <= r->u + r->grow)) { // (a NaN step too)
			un = r->u + r->grow;
			r->grow *= 2.0;
		}
	} else if (!(un >= r->lo && un <= r->hi)) {
		un = 0.5 * (r->lo + r->hi);
	}
	// (far out, where a step of kSpaStop / sqrt(V) is below the spacing of s, a step of a few ulps is as good)
	r->done = fabs(un - r->u) <= fmax(tol, kSpaUlps * r->u) || r->hi - r->lo <= tol;
	r->u = un;
	return true;
}

// Phi-bar(|omega + ln(nu / omega) / omega|) of one tail; NaN when the formula cannot be evaluated.
__device__ __forceinline__ double SpaTail(double u, double q, double kk, double k2) {
	const double rad = 2.0 * (u * q - kk);
	if (!(rad > 0.0) || !(k2 > 0.0)) {
		return NAN;
	}
	const double om = sqrt(rad), ratio = u * sqrt(k2) / om;
	if (!(ratio > 0.0) || !(ratio < INFINITY)) {
		return NAN;
	}
	return 0.5 * erfc(fabs(om + log(ratio) / om) * 0.70710678118654752440);
}

// Phase B of one row by one team, after phase A has left the row's `count` pairs in st[0 .. count - 1] (and a barrier
// behind them): u+ and u- (the roots are s = +u+ and s = -u-, both u > 0) by the safeguarded Newton iteration of the
// contract.  One evaluation is one pass of the team over the stash, both tails in the same pass: an exp per pair and
// tail, four fma chains per lane, TeamSums.  Every thread then holds the same four sums and takes the same step, so the
// control flow is team-uniform.  A last pass gives K and K'' at the two roots.  q = |U|; ok: false when the stash does
// not hold the row.  Returns whether the saddlepoint p was found (state 1, *p_out) or not (state 2), on every thread.
template <int TEAM, class Stash>
__device__ __forceinline__ bool SpaSolveStash(Stash st, uint32_t count, bool ok, double q, double v, double v_rest,
                                              int tid, int lane, int wave, double *p_out) {
	double sums[4];
	long long none[4] = {0, 0, 0, 0};
	const double tol = kSpaStop / sqrt(v);
	SpaRoot ra = {q / v, 0.0, INFINITY, 1.0 / sqrt(v), false}, rb = ra;
	asm volatile("" : "+v"(ra.lo), "+v"(ra.hi), "+v"(rb.lo), "+v"(rb.hi));
	for (int ev = 0; ok && ev < kSpaMaxEval && !(ra.done && rb.done); ev++) {
		sums[0] = sums[1] = sums[2] = sums[3] = 0.0;
		for (uint32_t j = tid; j < count; j += TEAM) {
			const double2 e = st[j];
			const double gg = e.x * e.x;
			double pi, qi;
			SpaPi(e.x * ra.u, e.y, &pi, &qi);
			sums[0] = fma(e.x, pi - e.y, sums[0]);
			sums[1] = fma(gg, pi * qi, sums[1]);
			SpaPi(-e.x * rb.u, e.y, &pi, &qi);
			sums[2] = fma(e.x, pi - e.y, sums[2]);
			sums[3] = fma(gg, pi * qi, sums[3]);
		}
		TeamSums<TEAM>(sums, none, lane, wave);
		TeamSync<TEAM>();
		ok = SpaStep(&ra, fma(v_rest, ra.u, sums[0]), sums[1] + v_rest, q, tol) &&
		     SpaStep(&rb, fma(v_rest, rb.u, -sums[2]), sums[3] + v_rest, q, tol);
	}
	ok = ok && ra.done && rb.done;
	double p = NAN;
	if (ok) { // (the whole team agrees)
		// K and K'' at the two roots, a tail at a time (one copy of the code; this pass runs once per row)
		p = 0.0;
#pragma nounroll
		for (int h = 0; h < 2; h++) {
			const double u = h ? rb.u : ra.u, su = h ? -u : u;
			sums[0] = sums[1] = sums[2] = sums[3] = 0.0;
			for (uint32_t j = tid; j < count; j += TEAM) {
				const double2 e = st[j];
				double pi, qi;
				SpaPi(e.x * su, e.y, &pi, &qi);
				sums[0] += SpaK(e.x * su, e.y);
				sums[1] = fma(e.x * e.x, pi * qi, sums[1]);
			}
			TeamSums<TEAM>(sums, none, lane, wave);
			TeamSync<TEAM>();
			p += SpaTail(u, q, fma(0.5 * v_rest * u, u, sums[0]), sums[1] + v_rest);
		}
		ok = fabs(p) < INFINITY;
	}
	*p_out = p;
	return ok;
}

} // namespace

} // namespace pgh
