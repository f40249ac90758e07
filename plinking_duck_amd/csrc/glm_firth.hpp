// glm_firth.hpp -- phase B of GlmScoreDenseFirthKernel (glm_score_dense_firth.hip) and GlmScoreSparseFirthKernel
// (glm_score_sparse_firth.hip): the approximate Firth estimate of a row's own coefficient from one team's stash of
// (x, mu) pairs, with glm_spa.hpp's pi and K (the contract is pgh_glm_score_multi_firth's in include/pgenhip.h;
// pgh_glm_score_sparse_firth's pairs hold d = x - b in x's place).
#pragma once

#include "glm_spa.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kFirthMaxEval = 64;     // evaluations of l*, F, H per row, the one at 0 included
constexpr double kFirthStop = 1e-10;  // |delta beta| sqrt(K''(0)) at which the evaluated point is taken

struct FirthFit {
	double beta, se, p;
};

// After phase A has left the row's `count` pairs in st[0 .. count - 1] (and a barrier behind them) and g = sum_E x r:
// the root of Firth's modified score F by the safeguarded Newton iteration of the contract, SpaStep's scheme on
// u = sgn beta >= 0 with sgn = sign F(0): the near end of the bracket is the last point with sgn F > 0, the far end is
// open until a point has sgn F < 0.  One evaluation is one pass of the team over the stash: an exp, an expm1 and a log1p
// per pair, five chains per lane, TeamSums.  Every thread then holds the same five sums and takes the same step, so the
// control flow is team-uniform.  The point that ends the iteration has been evaluated, so there is no pass after it.
// ok: false when the stash does not hold the row.  Returns whether the estimate was found (state 1, *fit) or not
// (state 2), on every thread.
template <int TEAM, class Stash>
__device__ __forceinline__ bool FirthSolveStash(Stash st, uint32_t count, bool ok, double g, int tid, int lane, int wave,
                                                FirthFit *fit) {
	double sums[5];
	long long none[4] = {0, 0, 0, 0};
	double sgn = 0.0, u = 0.0, lo = 0.0, hi = INFINITY, grow = 0.0, tol = 0.0, l0 = 0.0;
	asm volatile("" : "+v"(sgn), "+v"(u), "+v"(lo), "+v"(hi), "+v"(grow), "+v"(tol), "+v"(l0));
	bool done = false;
	for (int ev = 0; ok && !done && ev < kFirthMaxEval; ev++) {
		const double beta = sgn * u;
		sums[0] = sums[1] = sums[2] = sums[3] = sums[4] = 0.0;
		for (uint32_t j = tid; j < count; j += TEAM) {
			const double2 e = st[j];
			const double xb = e.x * beta, xx = e.x * e.x;
			double pi, qi;
			SpaPi(xb, e.y, &pi, &qi);
			const double v = pi * qi;
			sums[0] += SpaK(xb, e.y);
			sums[1] = fma(e.x, pi - e.y, sums[1]);
			sums[2] = fma(xx, v, sums[2]);
			sums[3] = fma(xx * e.x, v * (qi - pi), sums[3]);
			sums[4] = fma(xx * xx, v * (1.0 - 6.0 * v), sums[4]);
		}
		TeamSums<TEAM>(sums, none, lane, wave);
		TeamSync<TEAM>();
		const double k2 = sums[2], r3 = sums[3] / k2;
		const double ls = beta * g - sums[0] + 0.5 * log(k2);
		const double f = g - sums[1] + 0.5 * r3;
		double h = k2 - 0.5 * (sums[4] / k2 - r3 * r3);
		h = h > 0.0 ? h : k2;
		ok = k2 > 0.0 && fabs(ls) < INFINITY && fabs(f) < INFINITY && fabs(h) < INFINITY;
		if (!ok) { // (the whole team agrees)
			break;
		}
		if (ev == 0) {
			sgn = f > 0.0 ? 1.0 : -1.0;
			l0 = ls;
			grow = 1.0 / sqrt(k2);
			tol = kFirthStop * grow;
		}
		const double fs = sgn * f;
		double un = u;
		done = fs == 0.0;
		if (!done) {
			if (fs > 0.0) {
				lo = u;
			} else {
				hi = u;
			}
			un = u + fs / h;
			if (hi == INFINITY) {
				if (!(un <= u + grow)) {
					un = u + grow;
					grow *= 2.0;
				}
			} else if (!(un >= lo && un <= hi)) {
				un = 0.5 * (lo + hi);
			}
			const double d = fabs(un - u);
			done = d <= tol || hi - lo <= tol || d <= kSpaUlps * u;
		}
		if (done) {
			fit->beta = beta;
			fit->se = 1.0 / sqrt(k2);
			fit->p = erfc(sqrt(fmax(2.0 * (ls - l0), 0.0)) * 0.70710678118654752440); // GlmPFromZ (glm_math.hpp)
		}
		u = un;
	}
	return ok && done;
}

} // namespace

} // namespace pgh
