// grm.hpp -- launch wrapper of the variance-standardised relationship matrix (grm.hip).
// All pointers are device pointers; the wrapper only enqueues work on `stream`.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pgh {

constexpr uint32_t kGrmTile = 128;  // sample pairs per workgroup: kGrmTile x kGrmTile
constexpr uint32_t kGrmKStep = 64;  // variants per K-step: the table array is padded to a whole number of them

// The sample-major 2-bit matrix of the USED variants (LaunchTranspose2bitRange): raw sample r of the row side sits
// at xt_i + (r - raw_i0) * pitch, of the column side at xt_j + (r - raw_j0) * pitch.  sel: raw sample of each output
// sample (NULL: output sample = raw sample).  table: double[4] per used variant (z of the codes 0, 1, 2 and 0 for a
// missing call), zero padded to a multiple of kGrmKStep variants.
struct GrmOperand {
	const uint8_t *xt_i, *xt_j;
	uint32_t raw_i0, raw_j0;
	uint64_t pitch;
	const uint32_t *sel;
	const double *table;
	uint32_t n_used;
};

struct GrmOutput {
	// rows [i_begin, i_end) of the rectangle: entry (i, j) at (i - i_begin) * ld + (j - j_begin)
	double *rel;
	uint32_t *nobs; // may be NULL
	uint64_t ld;
	// triangle launches only: entry (j, i) of a tile right of the diagonal goes to row j of `rel` when j < i_end, and
	// to (j - i_end) * ld_m + (i - i_begin) of the mirror strip otherwise
	double *rel_m;
	uint32_t *nobs_m;
	uint64_t ld_m;
};

// rel = (sum over used variants of z_i z_j) / nobs, nobs = variants at which both are called (meanimpute: / n_used),
// for the output samples [i_begin, i_end) x [j_begin, j_end).  triangle: the rectangle is a band of tile rows of the
// square [j_begin, j_end)^2 (i_begin - j_begin a multiple of kGrmTile); only the tiles on and right of the diagonal
// are computed and each is written twice.
hipError_t LaunchGrm(const GrmOperand &op, uint32_t i_begin, uint32_t i_end, uint32_t j_begin, uint32_t j_end,
                     bool triangle, bool meanimpute, const GrmOutput &out, hipStream_t stream);

} // namespace pgh
