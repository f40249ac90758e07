// king.hpp -- launch wrappers of the KING-robust pair-count contraction (king.hip).
// All pointers are device pointers; every wrapper only enqueues work on `stream`.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pgh {

constexpr uint32_t kKingTile = 128;  // sample pairs per workgroup: kKingTile x kKingTile
constexpr uint32_t kKingPlanes = 5;  // NSNP, HETHET, IBS0, HET1HOM2, HET2HOM1 (PGH_KING_*)

// pgh_king_pair's layout (include/pgenhip.h; api_king.cpp asserts that the two agree)
struct KingPair {
	uint32_t i, j;
	uint32_t nsnp, hethet, ibs0, het1hom2, het2hom1;
	uint32_t pad;
	double kinship;
};

// The sample-major 2-bit matrix of the call's variants (LaunchTranspose2bit): row s at xt + s * pitch holds n_var
// codes, zero padded to whole 64-byte pieces.  sel: raw row of each output sample (NULL: output sample = raw sample).
struct KingOperand {
	const uint8_t *xt;
	uint64_t pitch;
	const uint32_t *sel;
	uint32_t n_var;
};

// out[p][i - i_begin][j - j_begin] (uint32, plane-major) for the output samples [i_begin, i_end) x [j_begin, j_end)
hipError_t LaunchKingCounts(const KingOperand &op, uint32_t i_begin, uint32_t i_end, uint32_t j_begin, uint32_t j_end,
                            uint32_t *out, hipStream_t stream);

// The pairs i < j < n_samples of the tile rows [tile_row_begin, tile_row_end) (i / kKingTile) that pass the filter
// (no_filter, or kinship >= min_kinship): *count += their number (the caller zeroes it), and the pairs that find a
// slot below `capacity` are written to out in no particular order -- every pair when *count <= capacity afterwards.
hipError_t LaunchKingTable(const KingOperand &op, uint32_t n_samples, uint32_t tile_row_begin, uint32_t tile_row_end,
                           double min_kinship, bool no_filter, KingPair *out, uint64_t capacity,
                           unsigned long long *count, hipStream_t stream);

} // namespace pgh
