// glm_score_sparse_lists.hpp -- the work lists of the follow-ups of the sparse many-phenotype score route:
// GlmScoreSparseMultiSpaKernel (glm_score_sparse_multi_spa.hip) and GlmScoreSparseMultiFirthKernel
// (glm_score_sparse_multi_firth.hip) instantiate the three kernels below with their own argument structs.
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per (block phenotype j, chunk variant i), at j * nv + i, its row.
// The rows that are applied (fitted with |stat| > cutoff) are few, so no team is launched per possible row: three small
// kernels list them first, in [variant][phenotype] order (element e = i * pb + j), so that the phenotypes applied for
// one variant run next to each other in time and find the variant's entry words in L2.  The wave-form list holds the
// sparse rows of at most kGlmSparseLong entries, the workgroup-form list the longer ones and the dense-form rows: the
// entry kernel's split.  A workgroup of the count kernel takes kListTile consecutive elements, a thread kListOwn
// consecutive ones of them, and leaves the tile's two counts; one workgroup turns the tiles' counts into their offsets
// and the lists' lengths; the write kernel ranks its tile again in thread order (TeamRankCounts) and writes the elements
// at offset + rank.  No atomics: a list is the applied elements of its form in ascending order, whatever the grid.  No
// result depends on that order either: a row is computed from its own inputs alone.
//
// Args is the including kernel file's argument struct.  The list kernels read of it
//   SparseRows rows;  uint32_t pb;  const pgh_glm_row *out ([pb][nv]);  double cutoff;
//   uint32_t *list_wave, *list_group (nv * pb words each);  uint32_t *tile_ct ([tiles][2], then the two lengths);
//   uint32_t n_tiles
// and nothing else, so a kernel's instructions do not depend on what else the struct holds beyond the fields' offsets.
#pragma once

#include "glm.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr uint32_t kListOwn = 8;                      // consecutive elements of a thread of the list kernels
constexpr uint32_t kListTile = kTeamBlock * kListOwn; // elements of a workgroup of the list kernels
static_assert(kListTile == kGlmScoreSparseListTile, "GlmScoreSparseMultiTileWords counts these tiles");

// A thread's kListOwn elements: bit u of *mw / *mg set where element e0 + u is applied and of the wave / workgroup form.
template <class Args>
__device__ __forceinline__ void ListFlags(const Args &a, uint32_t e0, uint32_t *mw, uint32_t *mg) {
	const uint32_t n = a.rows.nv * a.pb;
	*mw = *mg = 0;
#pragma unroll
	for (uint32_t u = 0; u < kListOwn; u++) {
		const uint32_t e = e0 + u;
		if (e < n) {
			const uint32_t i = e / a.pb, j = e - i * a.pb;
			const pgh_glm_row &row = a.out[static_cast<uint64_t>(j) * a.rows.nv + i];
			if (row.errcode == PGH_GLM_OK && fabs(row.stat) > a.cutoff) {
				const uint32_t r = a.rows.v_first + i;
				const bool wide = a.rows.row_of[r] >= 0 || a.rows.off[r + 1] - a.rows.off[r] > kGlmSparseLong;
				*mw |= wide ? 0u : 1u << u;
				*mg |= wide ? 1u << u : 0u;
			}
		}
	}
}

template <class Args>
__global__ void __launch_bounds__(kTeamBlock) GlmScoreSparseMultiCountKernel(const Args a) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t mw, mg, tw, tg;
	ListFlags(a, blockIdx.x * kListTile + threadIdx.x * kListOwn, &mw, &mg);
	TeamRankCounts(static_cast<uint32_t>(__popc(mw)), 0, lane, wave, &tw);
	TeamRankCounts(static_cast<uint32_t>(__popc(mg)), 1, lane, wave, &tg);
	if (threadIdx.x == 0) {
		a.tile_ct[2 * blockIdx.x] = tw;
		a.tile_ct[2 * blockIdx.x + 1] = tg;
	}
}

// One workgroup: tile_ct[tile][f] becomes the number of list f's elements before the tile, tile_ct[n_tiles][f] the
// list's length.  A thread takes consecutive tiles, so the offsets are those of the ascending order.
template <class Args>
__global__ void __launch_bounds__(kTeamBlock) GlmScoreSparseMultiOffsetKernel(const Args a) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t per = (a.n_tiles + kTeamBlock - 1) / kTeamBlock;
	const uint32_t t0 = threadIdx.x * per, t1 = t0 + per < a.n_tiles ? t0 + per : a.n_tiles;
	for (uint32_t f = 0; f < 2u; f++) {
		uint32_t mine = 0;
		for (uint32_t t = t0; t < t1; t++) {
			mine += a.tile_ct[2 * t + f];
		}
		uint32_t total;
		uint32_t before = TeamRankCounts(mine, f, lane, wave, &total);
		for (uint32_t t = t0; t < t1; t++) {
			const uint32_t c = a.tile_ct[2 * t + f];
			a.tile_ct[2 * t + f] = before;
			before += c;
		}
		if (threadIdx.x == 0) {
			a.tile_ct[2 * a.n_tiles + f] = total;
		}
	}
}

// The elements of the set bits of a thread's mask m, the first of them at list[pos]; n: the list's room.
__device__ __forceinline__ void ListWrite(uint32_t m, uint32_t e0, uint32_t pos, uint32_t n, uint32_t *__restrict__ list) {
	while (m) {
		const uint32_t u = static_cast<uint32_t>(__ffs(static_cast<int>(m)) - 1);
		m &= m - 1u;
		if (pos < n) { // (it is: a list holds no more than the chunk's elements)
			list[pos] = e0 + u;
		}
		pos++;
	}
}

template <class Args>
__global__ void __launch_bounds__(kTeamBlock) GlmScoreSparseMultiListKernel(const Args a) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t e0 = blockIdx.x * kListTile + threadIdx.x * kListOwn, n = a.rows.nv * a.pb;
	uint32_t mw, mg, total;
	ListFlags(a, e0, &mw, &mg);
	const uint32_t pw = TeamRankCounts(static_cast<uint32_t>(__popc(mw)), 0, lane, wave, &total);
	const uint32_t pg = TeamRankCounts(static_cast<uint32_t>(__popc(mg)), 1, lane, wave, &total);
	ListWrite(mw, e0, a.tile_ct[2 * blockIdx.x] + pw, n, a.list_wave);
	ListWrite(mg, e0, a.tile_ct[2 * blockIdx.x + 1] + pg, n, a.list_group);
}

// The three launches for a chunk of a.rows.nv * a.pb rows; a.n_tiles is GlmScoreSparseListTiles of that count.
template <class Args>
inline void LaunchGlmScoreSparseMultiLists(const Args &a, hipStream_t stream) {
	GlmScoreSparseMultiCountKernel<Args><<<a.n_tiles, kTeamBlock, 0, stream>>>(a);
	GlmScoreSparseMultiOffsetKernel<Args><<<1, kTeamBlock, 0, stream>>>(a);
	GlmScoreSparseMultiListKernel<Args><<<a.n_tiles, kTeamBlock, 0, stream>>>(a);
}

} // namespace

} // namespace pgh
