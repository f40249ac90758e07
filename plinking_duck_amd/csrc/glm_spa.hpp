// glm_spa.hpp -- the saddlepoint arithmetic that GlmScoreSpaKernel (glm_score_spa.hip), GlmScoreDenseSpaKernel
// (glm_score_dense_spa.hip), GlmScoreDenseDosageSpaKernel (glm_score_dense_dosage_spa.hip) and
// GlmScoreSparseMultiSpaKernel (glm_score_sparse_multi_spa.hip) share: pi, K, the
// safeguarded Newton step, a tail, and phase B, the iteration of one team over its stash of (g, mu) pairs (the contract
// is pgh_glm_score_sparse_spa's in include/pgenhip.h); and SpaSparseRow, the walk of one sparse-resident row into the
// stash that the first and the last instantiate with how they read a sample.
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

// One sparse-resident row by one team: phase A, the walk of the row's entries into the team's stash, and phase B,
// for GlmScoreSpaKernel (glm_score_spa.hip) and GlmScoreSparseMultiSpaKernel (glm_score_sparse_multi_spa.hip).
// i: the chunk variant; at: where the row's values stand in out, tv (rows of KP + 3: t, U, V), p_spa and state.
// st: the team's stash of at least `cap` pairs (LDS or global).  A Src is how a kernel reads a sample:
//   Sample, Load(s, &v): what the staged r of sample s needs (false: s is outside S);  R(v), W(s, v);
//   Z(s, j): covariate j of sample s, centred.
// The team returns from a row of the other form (a wave takes the sparse rows of at most kGlmSparseLong entries, the
// workgroup the longer ones and the dense-form rows) and from one that is not fitted with |stat| > cutoff.
template <int KP, int TEAM, class Src, class Stash>
__device__ __forceinline__ void SpaSparseRow(const SparseRows &rows, uint32_t i, uint32_t at, const Src &src,
                                             const pgh_glm_row *__restrict__ out, const double *__restrict__ tv,
                                             double cutoff, Stash st, uint32_t cap, double *__restrict__ p_spa,
                                             uint8_t *__restrict__ state) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int tid = TEAM == kTeamBlock ? static_cast<int>(threadIdx.x) : lane;
	const uint32_t r = rows.v_first + i;
	const int32_t ro = rows.row_of[r];
	const bool dense = ro >= 0;
	uint64_t e0 = 0, e1 = rows.sample_ct;
	if (dense) {
		if (TEAM != kTeamBlock) {
			return;
		}
	} else {
		e0 = rows.off[r];
		e1 = rows.off[r + 1];
		if ((e1 - e0 > kGlmSparseLong) != (TEAM == kTeamBlock)) {
			return;
		}
	}
	if (out[at].errcode != PGH_GLM_OK || !(fabs(out[at].stat) > cutoff)) {
		return;
	}
	const uint8_t *prow = dense ? rows.pool + static_cast<uint64_t>(ro) * rows.pitch : nullptr;
	const bool base3 = ro == -4;
	const int bx = (dense || base3) ? 0 : -1 - ro;
	double t[KP + 1];
#pragma unroll
	for (int j = 0; j <= KP; j++) {
		t[j] = tv[static_cast<uint64_t>(at) * (KP + 3) + j];
		// the row is the same for the whole workgroup, which would make t, and below U, V and the state of the
		// iteration, scalar registers, more than there are: keep them in vector registers
		asm volatile("" : "+v"(t[j]));
	}
	double q = fabs(tv[static_cast<uint64_t>(at) * (KP + 3) + KP + 1]), v = tv[static_cast<uint64_t>(at) * (KP + 3) + KP + 2];
	asm volatile("" : "+v"(q), "+v"(v));

	// phase A
	uint32_t count = 0;
	double sums[4] = {0.0, 0.0, 0.0, 0.0};
	long long none[4] = {0, 0, 0, 0};
	for (uint64_t p0 = e0; p0 < e1; p0 += TEAM) {
		const uint64_t p = p0 + tid;
		bool take = false;
		double g = 0.0, mu = 0.0;
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
			if (entry && code != 3u) {
				typename Src::Sample sv;
				if (src.Load(s, &sv)) {
					const double ri = src.R(sv);
					take = true;
					g = static_cast<double>(static_cast<int>(code) - bx) - t[0];
#pragma unroll
					for (int j = 0; j < KP; j++) {
						g = fma(-src.Z(s, j), t[1 + j], g);
					}
					mu = ri > 0.0 ? 1.0 - ri : -ri;
					sums[0] = fma(src.W(s, sv) * g, g, sums[0]);
				}
			}
		}
		uint32_t total;
		const uint32_t pos = count + TeamRank<TEAM>(take, lane, wave, &total);
		if (take && pos < cap) {
			st[pos] = make_double2(g, mu);
		}
		count += total;
		TeamSync<TEAM>(); // TeamRank's counts are rewritten by the next step
	}
	TeamSums<TEAM>(sums, none, lane, wave);
	TeamSync<TEAM>(); // the pairs before their readers, and TeamSums' LDS before it is written again
	bool ok = count <= cap;
	const double v_rest = base3 ? 0.0 : fmax(v - sums[0], 0.0);

	// phase B
	double p;
	ok = SpaSolveStash<TEAM>(st, count, ok, q, v, v_rest, tid, lane, wave, &p);
	if (tid == 0) {
		if (ok) {
			p_spa[at] = p;
		}
		state[at] = ok ? 1 : 2;
	}
}

} // namespace

} // namespace pgh
