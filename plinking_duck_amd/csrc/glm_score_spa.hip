// glm_score_spa.hip -- pgh_glm_score_sparse_spa: the saddlepoint p-value of the logistic score test of a sparse row,
// from the row's entries (the launch wrapper is in glm.hpp, the contract in include/pgenhip.h).
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per variant its row, [t = H_N^-1 c, U, V], and p_spa = p with
// state 0.  A team (a wave, or the workgroup for rows of more than kGlmSparseLong entries and for dense-form rows, the
// split of the entry kernel) takes a row that is fitted with |stat| > cutoff (SpaSparseRow in glm_spa.hpp, which
// GlmScoreSparseMultiSpaKernel instantiates too, reading a sample through VectorSrc here):
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

// How SpaSparseRow (glm_spa.hpp) reads a sample here: r and w in raw-sample order, the centred covariates.
template <int KP>
struct VectorSrc {
	const double *__restrict__ rr, *__restrict__ ww, *__restrict__ z;
	using Sample = double;
	__device__ __forceinline__ bool Load(uint32_t s, Sample *v) const {
		*v = rr[s];
		return *v == *v;
	}
	__device__ __forceinline__ double R(const Sample &v) const {
		return v;
	}
	__device__ __forceinline__ double W(uint32_t s, const Sample &) const {
		return ww[s];
	}
	__device__ __forceinline__ double Z(uint32_t s, int j) const {
		return z[static_cast<uint64_t>(s) * KP + j];
	}
};

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
	const VectorSrc<KP> src = {rr, ww, z};
	if constexpr (TEAM == kTeamBlock) {
		// TeamGridRows: a workgroup has its own sample_ct pairs of `stash`
		double2 *st = stash + static_cast<uint64_t>(blockIdx.x) * sample_ct;
		// (only thread 0's stores use them: held in vector registers, the loop's scalar registers all fit)
		asm volatile("" : "+v"(p_spa), "+v"(state));
		TeamGridRows(nv, [&](uint32_t i) {
			SpaSparseRow<KP, TEAM>(rows, i, i, src, out, tv, cutoff, st, sample_ct, p_spa, state);
		});
	} else {
		__shared__ double2 lds[kTeamWaves * kSpaWaveStash];
		const uint32_t i = blockIdx.x * kTeamWaves + (threadIdx.x >> 6);
		if (i < nv) {
			SpaSparseRow<KP, TEAM>(rows, i, i, src, out, tv, cutoff, lds + (threadIdx.x >> 6) * kSpaWaveStash,
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
