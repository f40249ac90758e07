// glm_score_sparse_multi_spa.hip -- pgh_glm_score_sparse_multi_spa: the saddlepoint p-value of the logistic score test
// of a (variant, phenotype) row of the sparse many-phenotype route, from the variant's entries (the launch wrapper is
// in glm.hpp, the contract in include/pgenhip.h, the arithmetic in glm_spa.hpp).
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per (block phenotype j, chunk variant i), at j * nv + i, its row,
// [t = H_N^-1 c, U, V], and p_spa = p with state 0.
//
// The work lists (glm_score_sparse_lists.hpp, shared with glm_score_sparse_multi_firth.hip).  The rows that are applied
// (fitted with |stat| > cutoff) are few, so no team is launched per possible row: three small kernels list them first,
// in [variant][phenotype] order (element e = i * pb + j), one list per team form, without atomics.  The phenotypes
// applied for one variant then run next to each other in time and find the variant's entry words and covariate rows in
// L2.
//
// One row by one team: SpaSparseRow (glm_spa.hpp), GlmScoreSpaKernel's walk and iteration, reading a sample through
// PairSrc: (r, w) is one double2 of the pair block at s * pb + j, and the covariate row is the raw-order one with
// phenotype j's means subtracted in the chain of g, the subtraction the entry kernel applies.  The stash of a wave is
// kGlmSparseLong pairs of LDS; a workgroup's is sample_ct pairs of global scratch of its own.  Both forms run as a
// bounded grid whose teams stride over their list, whose length they read from the device.  Nothing depends on which
// team takes a row, on the grids, on the chunk, on the phenotype block or on where the range starts.
#include "glm.hpp"
#include "glm_score_sparse_lists.hpp"
#include "glm_spa.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;
constexpr uint32_t kSpaWaveStash = kGlmSparseLong; // pairs per wave

struct SparseMultiSpaArgs {
	SparseRows rows;
	const double2 *pair; // [sample][pb]
	uint32_t pb;
	const double *z0, *mz;  // the uncentred covariates in raw-sample order, the block's means [pb][kp]
	const pgh_glm_row *out; // [pb][nv]
	const double *tv;       // [pb][nv][kp + 3]
	double cutoff;
	uint32_t *list_wave, *list_group; // the two forms' elements, nv * pb words each
	uint32_t *tile_ct;      // [tiles][2], then the two lengths
	uint32_t n_tiles;
	double2 *stash;
	double *p_spa;  // [pb][nv]
	uint8_t *state; // [pb][nv]
};

// ---------------------------------------------------------------------------
// the rows
// ---------------------------------------------------------------------------

// How SpaSparseRow reads a sample for block phenotype j: its pair of the block, and the raw-order covariate row minus
// the phenotype's means.
template <int KP>
struct PairSrc {
	const double2 *pair; // the block at phenotype j: sample s at pair[s * pb]
	uint32_t pb;
	const double *z0, *mzj;
	using Sample = double2;
	__device__ __forceinline__ bool Load(uint32_t s, Sample *v) const {
		*v = pair[static_cast<uint64_t>(s) * pb];
		return v->x == v->x;
	}
	__device__ __forceinline__ double R(const Sample &v) const {
		return v.x;
	}
	__device__ __forceinline__ double W(uint32_t, const Sample &v) const {
		return v.y;
	}
	__device__ __forceinline__ double Z(uint32_t s, int t) const {
		return z0[static_cast<uint64_t>(s) * KP + t] - mzj[t];
	}
};

// Element e = i * pb + j of a list by one team.
template <int KP, int TEAM, class Stash>
__device__ __forceinline__ void ListedRow(const SparseMultiSpaArgs &a, uint32_t e, Stash st, uint32_t cap,
                                          const pgh_glm_row *__restrict__ out, const double *__restrict__ tv,
                                          double *__restrict__ p_spa, uint8_t *__restrict__ state) {
	const uint32_t i = e / a.pb, j = e - i * a.pb;
	const PairSrc<KP> src = {a.pair + j, a.pb, a.z0, a.mz + static_cast<uint64_t>(j) * KP};
	SpaSparseRow<KP, TEAM>(a.rows, i, j * a.rows.nv + i, src, out, tv, a.cutoff, st, cap, p_spa, state);
}

// TEAM == 64: a wave strides over the wave-form list.  TEAM == 256: TeamGridRows over the workgroup-form list.
template <int KP, int TEAM>
__global__ void __launch_bounds__(kBlock) GlmScoreSparseMultiSpaKernel(const SparseMultiSpaArgs a) {
	double *p_spa = a.p_spa;
	uint8_t *state = a.state;
	const pgh_glm_row *out = a.out;
	const double *tv = a.tv;
	// (thread 0's stores and a few loads per row use them: held in vector registers, the loop's scalar registers all fit)
	asm volatile("" : "+v"(p_spa), "+v"(state), "+v"(out), "+v"(tv));
	if constexpr (TEAM == kTeamBlock) {
		const uint32_t n = a.tile_ct[2 * a.n_tiles + 1];
		double2 *st = a.stash + static_cast<uint64_t>(blockIdx.x) * a.rows.sample_ct;
		TeamGridRows(n, [&](uint32_t at) {
			ListedRow<KP, TEAM>(a, a.list_group[at], st, a.rows.sample_ct, out, tv, p_spa, state);
		});
	} else {
		__shared__ double2 lds[kTeamWaves * kSpaWaveStash];
		const uint32_t n = a.tile_ct[2 * a.n_tiles];
		double2 *st = lds + (threadIdx.x >> 6) * kSpaWaveStash;
		for (uint32_t at = blockIdx.x * kTeamWaves + (threadIdx.x >> 6); at < n; at += gridDim.x * kTeamWaves) {
			ListedRow<KP, TEAM>(a, a.list_wave[at], st, kSpaWaveStash, out, tv, p_spa, state);
			TeamSync<TEAM>(); // the next row rewrites the stash
		}
	}
}

} // namespace

hipError_t LaunchGlmScoreSparseMultiSpa(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *pair,
                                        uint32_t pb, const double *z0, const double *mz, uint32_t kp,
                                        const pgh_glm_row *rows, const double *t, double cutoff, uint32_t *list_wave,
                                        uint32_t *list_group, uint32_t *tile_ct, uint32_t n_wave_groups,
                                        uint32_t n_groups, void *stash, double *p_spa, uint8_t *state,
                                        hipStream_t stream) {
	if (pb == 0 || pb > kGlmScoreSparsePb) {
		return hipErrorInvalidValue;
	}
	if (nv == 0) {
		return hipSuccess;
	}
	const uint64_t n_rows = static_cast<uint64_t>(nv) * pb;
	if (n_groups == 0 || n_wave_groups == 0 || n_rows > UINT32_MAX) {
		return hipErrorInvalidValue;
	}
	SparseMultiSpaArgs a {};
	a.rows = {sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, nv};
	a.pair = reinterpret_cast<const double2 *>(pair);
	a.pb = pb;
	a.z0 = z0;
	a.mz = mz;
	a.out = rows;
	a.tv = t;
	a.cutoff = cutoff;
	a.list_wave = list_wave;
	a.list_group = list_group;
	a.tile_ct = tile_ct;
	a.n_tiles = static_cast<uint32_t>(GlmScoreSparseListTiles(n_rows));
	a.stash = static_cast<double2 *>(stash);
	a.p_spa = p_spa;
	a.state = state;
	LaunchGlmScoreSparseMultiLists(a, stream);
	const uint64_t wave_most = (n_rows + kTeamWaves - 1) / kTeamWaves;
	return GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value;
		GlmScoreSparseMultiSpaKernel<KP, 64><<<static_cast<uint32_t>(n_wave_groups < wave_most ? n_wave_groups : wave_most),
		                                       kBlock, 0, stream>>>(a);
		GlmScoreSparseMultiSpaKernel<KP, kBlock><<<static_cast<uint32_t>(n_groups < n_rows ? n_groups : n_rows), kBlock, 0,
		                                           stream>>>(a);
	});
}

} // namespace pgh
