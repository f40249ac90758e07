// glm_score_sparse_multi_firth.hip -- pgh_glm_score_sparse_multi_firth: the approximate Firth estimate of the own
// coefficient of a (variant, phenotype) row of the sparse many-phenotype route, from the variant's entries (the launch
// wrapper is in glm.hpp, the contract in include/pgenhip.h, the row and the iteration in glm_firth.hpp).
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per (block phenotype j, chunk variant i), at j * nv + i, its row.
//
// The default rows.  GlmScoreSparseMultiFirthFillKernel, one thread per element, writes every pgh_glm_firth_row of the
// chunk first: NaN where the row is not fitted, otherwise the score row's beta, se and p; state 0, pad 0.  The teams
// below then overwrite the applied rows, later on the same stream.
//
// The work lists (glm_score_sparse_lists.hpp, shared with glm_score_sparse_multi_spa.hip).  The rows that are applied
// (fitted with |stat| > cutoff) are few, so no team is launched per possible row: three small kernels list them first,
// in [variant][phenotype] order (element e = i * pb + j), one list per team form, without atomics.
//
// One row by one team: SparseFirthRow (glm_firth.hpp), GlmScoreSparseFirthKernel's walk and iteration, reading a
// sample's r as the x of one double2 of the pair block at s * pb + j, which is NaN where the sample is not in that
// phenotype's S.  The stash of a wave is kGlmSparseLong pairs of LDS; a workgroup's is sample_ct pairs of global scratch
// of its own.  Both forms run as a bounded grid whose teams stride over their list, whose length they read from the
// device.  An applied row is written once more, by thread 0 of the one team that takes it.  No atomics; nothing
// depends on which team takes a row, on the grids, on the chunk, on the phenotype block or on where the range starts.
// The kernels read no covariates and no w, so they have no width in them.
#include "glm.hpp"
#include "glm_firth.hpp"
#include "glm_score_sparse_lists.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;
constexpr uint32_t kFirthWaveStash = kGlmSparseLong; // pairs per wave

struct SparseMultiFirthArgs {
	SparseRows rows;
	const double2 *pair; // [sample][pb]
	uint32_t pb;
	const pgh_glm_row *out; // [pb][nv]
	double cutoff;
	uint32_t *list_wave, *list_group; // the two forms' elements, nv * pb words each
	uint32_t *tile_ct;      // [tiles][2], then the two lengths
	uint32_t n_tiles;
	double2 *stash;
	pgh_glm_firth_row *firth; // [pb][nv]
};

// Row `at` = j * nv + i as it stands when the Firth step is not applied.
__global__ void __launch_bounds__(kBlock) GlmScoreSparseMultiFirthFillKernel(const pgh_glm_row *__restrict__ out,
                                                                             uint32_t n_rows,
                                                                             pgh_glm_firth_row *__restrict__ firth) {
	const uint32_t at = blockIdx.x * kBlock + threadIdx.x;
	if (at < n_rows) {
		const bool fitted = out[at].errcode == PGH_GLM_OK;
		pgh_glm_firth_row res {};
		res.beta = fitted ? out[at].beta : NAN;
		res.se = fitted ? out[at].se : NAN;
		res.p = fitted ? out[at].p : NAN;
		firth[at] = res;
	}
}

// How SparseFirthRow reads a sample's r for block phenotype j: the x of its pair of the block.
struct PairR {
	const double2 *pair; // the block at phenotype j: sample s at pair[s * pb]
	uint32_t pb;
	__device__ __forceinline__ double operator()(uint32_t s) const {
		return pair[static_cast<uint64_t>(s) * pb].x;
	}
};

// Element e = i * pb + j of a list by one team.
template <int TEAM, class Stash>
__device__ __forceinline__ void ListedRow(const SparseMultiFirthArgs &a, uint32_t e, Stash st, uint32_t cap) {
	const uint32_t i = e / a.pb, j = e - i * a.pb;
	SparseFirthRow<TEAM>(a.rows, i, j * a.rows.nv + i, PairR {a.pair + j, a.pb}, a.out, a.cutoff, st, cap, a.firth);
}

// TEAM == 64: a wave strides over the wave-form list.  TEAM == 256: TeamGridRows over the workgroup-form list.
template <int TEAM>
__global__ void __launch_bounds__(kBlock) GlmScoreSparseMultiFirthKernel(const SparseMultiFirthArgs a) {
	if constexpr (TEAM == kTeamBlock) {
		const uint32_t n = a.tile_ct[2 * a.n_tiles + 1];
		double2 *st = a.stash + static_cast<uint64_t>(blockIdx.x) * a.rows.sample_ct;
		TeamGridRows(n, [&](uint32_t at) { ListedRow<TEAM>(a, a.list_group[at], st, a.rows.sample_ct); });
	} else {
		__shared__ double2 lds[kTeamWaves * kFirthWaveStash];
		const uint32_t n = a.tile_ct[2 * a.n_tiles];
		double2 *st = lds + (threadIdx.x >> 6) * kFirthWaveStash;
		for (uint32_t at = blockIdx.x * kTeamWaves + (threadIdx.x >> 6); at < n; at += gridDim.x * kTeamWaves) {
			ListedRow<TEAM>(a, a.list_wave[at], st, kFirthWaveStash);
			TeamSync<TEAM>(); // the next row rewrites the stash
		}
	}
}

} // namespace

hipError_t LaunchGlmScoreSparseMultiFirth(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *pair,
                                          uint32_t pb, const pgh_glm_row *rows, double cutoff, uint32_t *list_wave,
                                          uint32_t *list_group, uint32_t *tile_ct, uint32_t n_wave_groups,
                                          uint32_t n_groups, void *stash, pgh_glm_firth_row *firth,
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
	SparseMultiFirthArgs a {};
	a.rows = {sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, nv};
	a.pair = reinterpret_cast<const double2 *>(pair);
	a.pb = pb;
	a.out = rows;
	a.cutoff = cutoff;
	a.list_wave = list_wave;
	a.list_group = list_group;
	a.tile_ct = tile_ct;
	a.n_tiles = static_cast<uint32_t>(GlmScoreSparseListTiles(n_rows));
	a.stash = static_cast<double2 *>(stash);
	a.firth = firth;
	GlmScoreSparseMultiFirthFillKernel<<<static_cast<uint32_t>((n_rows + kBlock - 1) / kBlock), kBlock, 0, stream>>>(
	    rows, static_cast<uint32_t>(n_rows), firth);
	LaunchGlmScoreSparseMultiLists(a, stream);
	const uint64_t wave_most = (n_rows + kTeamWaves - 1) / kTeamWaves;
	GlmScoreSparseMultiFirthKernel<64><<<static_cast<uint32_t>(n_wave_groups < wave_most ? n_wave_groups : wave_most),
	                                     kBlock, 0, stream>>>(a);
	GlmScoreSparseMultiFirthKernel<kBlock><<<static_cast<uint32_t>(n_groups < n_rows ? n_groups : n_rows), kBlock, 0,
	                                         stream>>>(a);
	return hipGetLastError();
}

} // namespace pgh
