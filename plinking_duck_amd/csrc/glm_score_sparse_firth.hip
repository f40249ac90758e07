// glm_score_sparse_firth.hip -- pgh_glm_score_sparse_firth: the approximate Firth estimate of a sparse row's own
// coefficient, from the row's entries (the launch wrapper is in glm.hpp, the contract in include/pgenhip.h, the
// iteration in glm_firth.hpp).
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per chunk variant its row.  A team (a wave, or the workgroup for
// rows of more than kGlmSparseLong entries and for dense-form rows, the split of the entry kernel and of
// GlmScoreSpaKernel) takes a row and writes its pgh_glm_firth_row: the score row's beta, se and p with state 0 where the
// row is not fitted or |stat| <= cutoff, otherwise
//   phase A  one walk of the row's entries.  A used called entry with d = x - b != 0 (the set E) gathers r alone and
//            becomes the pair (d, mu), mu = r > 0 ? 1 - r : -r.  The pairs go to the team's stash in entry order
//            (TeamRank), G = sum_E d r is a lane chain and TeamSums.
//   phase B  FirthSolveStash (glm_firth.hpp, shared with glm_score_dense_firth.hip) over the stash.
// The stash of a wave is 1,024 pairs of LDS; a workgroup's is sample_ct pairs of global scratch of its own, and the
// workgroup form runs as a bounded grid of workgroups that stride over the rows.  Every row is written once, by thread 0
// of the one team that takes it.  No atomics; nothing depends on which workgroup takes a row, on the grid, on the chunk
// or on where the range starts.  The kernel reads no covariates, so it has no width in it.
#include "glm.hpp"
#include "glm_firth.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;
constexpr uint32_t kFirthWaveStash = kGlmSparseLong; // pairs per wave

// One row by one team.  st: the team's stash of at least `cap` pairs (LDS or global).
template <int TEAM, class Stash>
__device__ __forceinline__ void SparseFirthRow(const SparseRows &rows, uint32_t i, const double *__restrict__ rr,
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
	const bool fitted = out[i].errcode == PGH_GLM_OK;
	pgh_glm_firth_row res {};
	res.beta = fitted ? out[i].beta : NAN;
	res.se = fitted ? out[i].se : NAN;
	res.p = fitted ? out[i].p : NAN;
	if (fitted && fabs(out[i].stat) > cutoff) { // (the whole team)
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
					const double ri = rr[s];
					if (ri == ri) {
						take = true;
						d = static_cast<double>(static_cast<int>(code) - bx);
						mu = ri > 0.0 ? 1.0 - ri : -ri;
						sums[0] = fma(d, ri, sums[0]);
					}
				}
			}
			uint32_t total;
			const uint32_t at = count + TeamRank<TEAM>(take, lane, wave, &total);
			if (take && at < cap) {
				st[at] = make_double2(d, mu);
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
		firth[i] = res;
	}
}

template <int TEAM>
__global__ void __launch_bounds__(kBlock) GlmScoreSparseFirthKernel(const SparseRows rows,
                                                                    const double *__restrict__ rr,
                                                                    const pgh_glm_row *__restrict__ out, double cutoff,
                                                                    double2 *__restrict__ stash,
                                                                    pgh_glm_firth_row *__restrict__ firth) {
	if constexpr (TEAM == kTeamBlock) {
		// TeamGridRows: a workgroup has its own sample_ct pairs of `stash`
		double2 *st = stash + static_cast<uint64_t>(blockIdx.x) * rows.sample_ct;
		TeamGridRows(rows.nv, [&](uint32_t i) { SparseFirthRow<TEAM>(rows, i, rr, out, cutoff, st, rows.sample_ct, firth); });
	} else {
		__shared__ double2 lds[kTeamWaves * kFirthWaveStash];
		const uint32_t i = blockIdx.x * kTeamWaves + (threadIdx.x >> 6);
		if (i < rows.nv) {
			SparseFirthRow<TEAM>(rows, i, rr, out, cutoff, lds + (threadIdx.x >> 6) * kFirthWaveStash, kFirthWaveStash,
			                     firth);
		}
	}
}

} // namespace

hipError_t LaunchGlmScoreSparseFirth(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *r,
                                     const pgh_glm_row *rows, double cutoff, uint32_t n_groups, void *stash,
                                     pgh_glm_firth_row *firth, hipStream_t stream) {
	if (nv == 0) {
		return hipSuccess;
	}
	if (n_groups == 0) {
		return hipErrorInvalidValue;
	}
	const SparseRows sr = {sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, nv};
	GlmScoreSparseFirthKernel<64><<<(nv + kTeamWaves - 1) / kTeamWaves, kBlock, 0, stream>>>(sr, r, rows, cutoff, nullptr,
	                                                                                          firth);
	GlmScoreSparseFirthKernel<kBlock><<<n_groups < nv ? n_groups : nv, kBlock, 0, stream>>>(
	    sr, r, rows, cutoff, static_cast<double2 *>(stash), firth);
	return hipGetLastError();
}

} // namespace pgh
