// glm_score_sparse_firth.hip -- pgh_glm_score_sparse_firth: the approximate Firth estimate of a sparse row's own
// coefficient, from the row's entries (the launch wrapper is in glm.hpp, the contract in include/pgenhip.h, the
// iteration in glm_firth.hpp).
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per chunk variant its row.  A team (a wave, or the workgroup for
// rows of more than kGlmSparseLong entries and for dense-form rows, the split of the entry kernel and of
// GlmScoreSpaKernel) takes a row and writes its pgh_glm_firth_row (SparseFirthRow, glm_firth.hpp, shared with
// glm_score_sparse_multi_firth.hip): the score row's beta, se and p with state 0 where the row is not fitted or
// |stat| <= cutoff, otherwise
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

// How SparseFirthRow reads a sample's r: the staged residuals in raw-sample order, NaN outside S.
struct RawR {
	const double *__restrict__ rr;
	__device__ __forceinline__ double operator()(uint32_t s) const {
		return rr[s];
	}
};

template <int TEAM>
__global__ void __launch_bounds__(kBlock) GlmScoreSparseFirthKernel(const SparseRows rows,
                                                                    const double *__restrict__ rr,
                                                                    const pgh_glm_row *__restrict__ out, double cutoff,
                                                                    double2 *__restrict__ stash,
                                                                    pgh_glm_firth_row *__restrict__ firth) {
	if constexpr (TEAM == kTeamBlock) {
		// TeamGridRows: a workgroup has its own sample_ct pairs of `stash`
		double2 *st = stash + static_cast<uint64_t>(blockIdx.x) * rows.sample_ct;
		TeamGridRows(rows.nv, [&](uint32_t i) { SparseFirthRow<TEAM>(rows, i, i, RawR {rr}, out, cutoff, st, rows.sample_ct, firth); });
	} else {
		__shared__ double2 lds[kTeamWaves * kFirthWaveStash];
		const uint32_t i = blockIdx.x * kTeamWaves + (threadIdx.x >> 6);
		if (i < rows.nv) {
			SparseFirthRow<TEAM>(rows, i, i, RawR {rr}, out, cutoff, lds + (threadIdx.x >> 6) * kFirthWaveStash,
			                     kFirthWaveStash, firth);
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
