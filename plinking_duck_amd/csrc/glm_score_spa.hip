// glm_score_spa.hip -- pgh_glm_score_sparse_spa: the saddlepoint p-value of the logistic score test of a sparse row,
// from the row's entries (the launch wrapper is in glm.hpp, the contract in include/pgenhip.h).
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per variant its row, [t = H_N^-1 c, U, V], and p_spa = p with
// state 0.  A team (a wave, or the workgroup for rows of more than kGlmSparseLong entries and for dense-form rows, the
// split of the entry kernel) takes a row that is fitted with |stat| > cutoff:
//   phase A  one walk of the row's entries.  A used called entry (the set E) gathers r, w and its z row and becomes
//            the pair (g, mu): g = d - Zt t, mu = r > 0 ? 1 - r : -r.  The pairs go to the team's stash in entry order
//            (TeamRank), V_E = sum_E w g^2 is a lane chain and TeamSums.
//   phase B  SpaSolveStash (glm_spa.hpp, shared with glm_score_dense_spa.hip): u+ and u- by the safeguarded Newton
//            iteration of the contract, one evaluation being one pass of the team over the stash, then K and K'' at
//            the two roots.  All control flow is team-uniform.
// The stash of a wave is 1,024 pairs of LDS; a workgroup's is sample_ct pairs of global scratch of its own, and the
// workgroup form runs as a bounded grid of workgroups that stride over the rows.  No atomics; nothing depends on which
// workgroup takes a row, on the grid, on the chunk or on where the range starts.
#include "glm.hpp"
#include "glm_spa.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;
constexpr uint32_t kSpaWaveStash = kGlmSparseLong; // pairs per wave

// One row by one team.  st: the team's stash of at least `cap` pairs (LDS or global).
template <int KP, int TEAM, class Stash>
__device__ __forceinline__ void SpaRow(const SparseRows &rows, uint32_t i, const double *__restrict__ rr,
                                       const double *__restrict__ ww, const double *__restrict__ z,
                                       const pgh_glm_row *__restrict__ out, const double *__restrict__ tv,
                                       double cutoff, Stash st, uint32_t cap,
                                       double *__restrict__ p_spa, uint8_t *__restrict__ state) {
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
	if (out[i].errcode != PGH_GLM_OK || !(fabs(out[i].stat) > cutoff)) {
		return;
	}
	const uint8_t *prow = dense ? rows.pool + static_cast<uint64_t>(ro) * rows.pitch : nullptr;
	const bool base3 = ro == -4;
	const int bx = (dense || base3) ? 0 : -1 - ro;
	double t[KP + 1];
#pragma unroll
	for (int j = 0; j <= KP; j++) {
		t[j] = tv[static_cast<uint64_t>(i) * (KP + 3) + j];
		// the row is the same for the whole workgroup, which would make t, and below U, V and the state of the
		// iteration, scalar registers, more than there are: keep them in vector registers
		asm volatile("" : "+v"(t[j]));
	}
	double q = fabs(tv[static_cast<uint64_t>(i) * (KP + 3) + KP + 1]), v = tv[static_cast<uint64_t>(i) * (KP + 3) + KP + 2];
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
				const double ri = rr[s];
				if (ri == ri) {
					take = true;
					g = static_cast<double>(static_cast<int>(code) - bx) - t[0];
#pragma unroll
					for (int j = 0; j < KP; j++) {
						g = fma(-z[static_cast<uint64_t>(s) * KP + j], t[1 + j], g);
					}
					mu = ri > 0.0 ? 1.0 - ri : -ri;
					sums[0] = fma(ww[s] * g, g, sums[0]);
				}
			}
		}
		uint32_t total;
		const uint32_t at = count + TeamRank<TEAM>(take, lane, wave, &total);
		if (take && at < cap) {
			st[at] = make_double2(g, mu);
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
			p_spa[i] = p;
		}
		state[i] = ok ? 1 : 2;
	}
}

template <int KP, int TEAM>
__global__ void __launch_bounds__(kBlock) GlmScoreSpaKernel(const int32_t *__restrict__ row_of,
                                                            const uint64_t *__restrict__ off,
                                                            const uint32_t *__restrict__ entries,
                                                            const uint8_t *__restrict__ pool, uint64_t pitch,
                                                            uint32_t sample_ct, uint32_t v_first, uint32_t nv,
                                                            const double *__restrict__ rr,
                                                            const double *__restrict__ ww,
                                                            const double *__restrict__ z,
                                                            const pgh_glm_row *__restrict__ out,
                                                            const double *__restrict__ tv, double cutoff,
                                                            double2 *__restrict__ stash, double *__restrict__ p_spa,
                                                            uint8_t *__restrict__ state) {
	const SparseRows rows = {row_of, off, entries, pool, pitch, sample_ct, v_first, nv};
	if constexpr (TEAM == kTeamBlock) {
		// TeamGridRows: a workgroup has its own sample_ct pairs of `stash`
		double2 *st = stash + static_cast<uint64_t>(blockIdx.x) * sample_ct;
		// (only thread 0's stores use them: held in vector registers, the loop's scalar registers all fit)
		asm volatile("" : "+v"(p_spa), "+v"(state));
		TeamGridRows(nv, [&](uint32_t i) {
			SpaRow<KP, TEAM>(rows, i, rr, ww, z, out, tv, cutoff, st, sample_ct, p_spa, state);
		});
	} else {
		__shared__ double2 lds[kTeamWaves * kSpaWaveStash];
		const uint32_t i = blockIdx.x * kTeamWaves + (threadIdx.x >> 6);
		if (i < nv) {
			SpaRow<KP, TEAM>(rows, i, rr, ww, z, out, tv, cutoff, lds + (threadIdx.x >> 6) * kSpaWaveStash,
			                 kSpaWaveStash, p_spa, state);
		}
	}
}

} // namespace

hipError_t LaunchGlmScoreSpa(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *r, const double *w,
                             const double *z, uint32_t kp, const pgh_glm_row *rows, const double *t,
                             double cutoff, uint32_t n_groups, void *stash, double *p_spa, uint8_t *state,
                             hipStream_t stream) {
	if (nv == 0) {
		return hipSuccess;
	}
	if (n_groups == 0) {
		return hipErrorInvalidValue;
	}
	return GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value;
		GlmScoreSpaKernel<KP, 64><<<(nv + kTeamWaves - 1) / kTeamWaves, kBlock, 0, stream>>>(
		    sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, nv, r, w, z, rows, t, cutoff,
		    nullptr, p_spa, state);
		GlmScoreSpaKernel<KP, kBlock><<<n_groups < nv ? n_groups : nv, kBlock, 0, stream>>>(
		    sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, nv, r, w, z, rows, t, cutoff,
		    static_cast<double2 *>(stash), p_spa, state);
	});
}

} // namespace pgh
