// ldband.hpp -- launch wrappers of the banded variant-pair contraction (ldband.hip).
// All pointers are device pointers; every wrapper only enqueues work on `stream`.
#pragma once

#include "kernels.hpp"

namespace pgh {

constexpr uint32_t kLdTileA = 96;   // anchor variants per workgroup tile
constexpr uint32_t kLdTileB = 128;  // partner variants per workgroup tile
constexpr uint32_t kLdPlanes = 6;   // n, sum_a, sum_b, sum_ab, sum_a2, sum_b2 (pgh_ld_pairs' order)
constexpr uint32_t kLdTileBitWords = kLdTileA * (kLdTileB / 32); // uint32 words of one tile of the band bit matrix
constexpr uint32_t kLdTileScoreSlots = kLdTileA + kLdTileB;     // row sums, then column sums, of one tile's r2 terms

// The call's variants: variant k of the call is row list[k] of view (a local row index), k < n_var.
// mask2: the subset's row of 01 slots (NULL: every sample).
struct LdBandOperand {
	RowView view;
	const uint32_t *list;
	uint32_t n_var;
	const uint8_t *mask2;
};

// First anchor and first partner (indices into the call's variants) of one kLdTileA x kLdTileB tile.
struct LdTile {
	uint32_t a0, b0;
};

// The six sums of the pairs (a, b), a in [a_begin, a_end), b in [b_begin, b_end) that the n_tiles tiles cover:
// out[p * plane_stride + (a - a_begin) * (b_end - b_begin) + (b - b_begin)], plane_stride = (a_end - a_begin) *
// (b_end - b_begin).  A tile's pairs outside the rectangle are not written.
hipError_t LaunchLdBandSums(const LdBandOperand &op, const LdTile *tiles, uint32_t n_tiles, uint32_t a_begin,
                            uint32_t a_end, uint32_t b_begin, uint32_t b_end, uint32_t *out, hipStream_t stream);

// One bit per pair of the n_tiles tiles: bits[(t * kLdTileA + r) * 4 + w] bit c is the pair (tiles[t].a0 + r,
// tiles[t].b0 + 32 w + c), set iff k < u < win_end[k] (k the anchor, u the partner) and LdExceeds(sums, threshold).
// Every word of every tile is written; the sums stay in registers.
hipError_t LaunchLdBandBits(const LdBandOperand &op, const LdTile *tiles, uint32_t n_tiles, const uint32_t *win_end,
                            double threshold, uint32_t *bits, hipStream_t stream);

// The LD-score partial sums of the n_tiles tiles.  A pair (k, u) of a tile counts iff k < u < win_end[k] and
// LdR2Term(sums, flags, &term) says it is defined; every other pair of the tile has term 0 and count 0.  For tile t:
// part[t * kLdTileScoreSlots + r] is the sum of the terms of anchor row r (r < kLdTileA) over the tile's 128 partners,
// part[t * kLdTileScoreSlots + kLdTileA + c] the sum of partner column c over the tile's 96 anchors, and cnt[...] the
// number of counting pairs of the same row or column.  The additions are in a fixed order that depends only on the
// position inside the tile (ldband.hip).  Every slot of every tile is written; the sums and the terms
// stay in registers and LDS.
hipError_t LaunchLdBandScores(const LdBandOperand &op, const LdTile *tiles, uint32_t n_tiles, const uint32_t *win_end,
                              uint32_t flags, double *part, uint32_t *cnt, hipStream_t stream);

} // namespace pgh
