// glm_firth.hpp -- phase B of GlmScoreDenseFirthKernel (glm_score_dense_firth.hip), GlmScoreSparseFirthKernel
// (glm_score_sparse_firth.hip) and GlmScoreSparseMultiFirthKernel (glm_score_sparse_multi_firth.hip): the approximate
// Firth estimate of a row's own coefficient from one team's stash of (x, mu) pairs, with glm_spa.hpp's pi and K (the
// contract is pgh_glm_score_multi_firth's in include/pgenhip.h; pgh_glm_score_sparse_firth's pairs hold d = x - b in
// x's place).  And SparseFirthRow, the sparse kernels' row: the walk of a sparse-resident row's entries into the stash,
// then phase B.
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

// One sparse-resident row by one team: phase A, the walk of the row's entries into the team's stash, and phase B, for
// GlmScoreSparseFirthKernel (glm_score_sparse_firth.hip) and GlmScoreSparseMultiFirthKernel
// (glm_score_sparse_multi_firth.hip).  i: the chunk variant; at: where the row stands in out and firth.  st: the team's
// stash of at least `cap` pairs (LDS or global).  r_of(s): the staged r of raw sample s, NaN where s is outside S.
// The team returns from a row of the other form (a wave takes the sparse rows of at most kGlmSparseLong entries, the
// workgroup the longer ones and the dense-form rows); of every other row it writes firth[at]: the score row's beta, se
// and p with state 0 where the row is not fitted or |stat| <= cutoff.
template <int TEAM, class R, class Stash>
__device__ __forceinline__ void SparseFirthRow(const SparseRows &rows, uint32_t i, uint32_t at, const R &r_of,
                                               const pgh_glm_row *__restrict__ out, double cutoff, Stash st,
                                               uint32_t cap, pgh_glm_firth_row *__restrict__ firth) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int tid = TEAM == kTeamBlock ? static_cast<int>(threadIdx.x) : lane;
	const uint32_t r = rows.v_first + i;
	const int32_t ro = rows.row_of[r];
	const bool dense = ro >= 0;
	uint64_t e0 = 0, e1 = rows.sample_ct;
	if (dense) {
		if (TEAM != kTeamBlock) {
			return; // the workgroup launch's row
		}
	} else {
		e0 = rows.off[r];
		e1 = rows.off[r + 1];
		if ((e1 - e0 > kGlmSparseLong) != (TEAM == kTeamBlock)) {
			return; // the other launch's row
		}
	}
	const bool fitted = out[at].errcode == PGH_GLM_OK;
	pgh_glm_firth_row res {};
	res.beta = fitted ? out[at].beta : NAN;
	res.se = fitted ? out[at].se : NAN;
	res.p = fitted ? out[at].p : NAN;
	if (fitted && fabs(out[at].stat) > cutoff) { // (the whole team)
		const uint8_t *prow = dense ? rows.pool + static_cast<uint64_t>(ro) * rows.pitch : nullptr;
		const int bx = (dense || ro == -4) ? 0 : -1 - ro;

		// phase A
		uint32_t count = 0;
		double sums[1] = {0.0};
		long long none[4] = {0, 0, 0, 0};
		for (uint64_t p0 = e0; p0 < e1; p0 += TEAM) {
			const uint64_t p = p0 + tid;
			bool take = false;
			double d = 0.0, mu = 0.0;
			if (p < e1) {
				uint32_t code, s;
				bool entry;
				if (dense) {
					s = static_cast<uint32_t>(p);
					code = (prow[s >> 2] >> (2 * (s & 3u))) & 3u;
					entry = code != 0u;
				} else {
					const uint32_t x = rows.entries[p];
					s = x >> 2;
					code = x & 3u;
					entry = s < rows.sample_ct;
				}
				// (a base-3 row holds its hom-ref calls as entries: d = 0, a constant of l*, not in E)
				if (entry && code != 3u && static_cast<int>(code) != bx) {
					const double ri = r_of(s);
					if (ri == ri) {
						take = true;
						d = static_cast<double>(static_cast<int>(code) - bx);
						mu = ri > 0.0 ? 1.0 - ri : -ri;
						sums[0] = fma(d, ri, sums[0]);
					}
				}
			}
			uint32_t total;
			const uint32_t pos = count + TeamRank<TEAM>(take, lane, wave, &total);
			if (take && pos < cap) {
				st[pos] = make_double2(d, mu);
			}
			count += total;
			TeamSync<TEAM>(); // TeamRank's counts are rewritten by the next step
		}
		TeamSums<TEAM>(sums, none, lane, wave);
		TeamSync<TEAM>(); // the pairs before their readers, and TeamSums' LDS before it is written again
		// (the row is the same for the whole workgroup, which would make G and the state of the iteration scalar
		// registers: keep them in vector registers, as GlmScoreDenseFirthKernel does)
		double g = sums[0];
		asm volatile("" : "+v"(g));

		// phase B
		FirthFit fit;
		const bool ok = FirthSolveStash<TEAM>(st, count, count <= cap, g, tid, lane, wave, &fit);
		if (ok) {
			res.beta = fit.beta;
			res.se = fit.se;
			res.p = fit.p;
		}
		res.state = ok ? 1 : 2;
	}
	if (tid == 0) {
		firth[at] = res;
	}
}

} // namespace

} // namespace pgh
