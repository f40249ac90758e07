// sparse.hpp -- launch wrappers of the sparse-resident kernels (sparse.hip): the second resident form of a dataset
// (pgh_open_sparse, api_sparse.cpp).  Per variant ONE of two forms:
//   sparse  a base code (the row's majority class, any of 0..3) and the samples whose call differs from it,
//           ascending, one uint32 entry each: sample << 2 | code;
//   dense   the plain 2-bit row, in a compact pool of rows `pitch` bytes apart.
// row_of[r] >= 0: row r is dense, pool row row_of[r]; row_of[r] < 0: row r is sparse with base code -1 - row_of[r].
// off[r] .. off[r + 1]: row r's entries (empty for a dense row).
// All pointers are device pointers; every wrapper only enqueues work on `stream`.
#pragma once

#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace pgh {

struct SparseView {
	const int32_t *row_of;
	const uint64_t *off;
	const uint32_t *entries;
	const uint8_t *pool;
	uint64_t pitch;
	uint32_t sample_ct;
	uint32_t record_bytes;
};

// Samples of one LDS tile of k_sparse_sample_classes: 8192 x 3 uint32 = 96 KB of the 160 KiB.
constexpr uint32_t kSparseTile = 8192;

// First index in [lo, hi) whose entry's sample is >= s0 (hi if none), by the whole wave: 64 probes per step.
__device__ __forceinline__ uint64_t WaveLowerBound(const uint32_t *entries, uint64_t lo, uint64_t hi, uint32_t s0,
                                                   uint32_t lane) {
	while (hi - lo > 64) {
		const uint64_t step = (hi - lo + 63) / 64;
		const uint64_t p = lo + lane * step;
		const bool below = p < hi && (entries[p] >> 2) < s0;
		const uint32_t k = static_cast<uint32_t>(__popcll(__ballot(below))); // probes below s0: a prefix of the lanes
		if (k == 0) {
			return lo;
		}
		const uint64_t nlo = lo + (k - 1) * step + 1;
		hi = std::min<uint64_t>(hi, lo + k * step);
		lo = nlo;
	}
	const uint64_t p = lo + lane;
	const bool below = p < hi && (entries[p] >> 2) < s0;
	return lo + static_cast<uint64_t>(__popcll(__ballot(below)));
}

// out[2 * i] = majority code of row i of `view` (ties: the lower code), out[2 * i + 1] = samples not in it.
hipError_t LaunchSparseClassify(const RowView &view, uint32_t v_count, uint32_t *out, hipStream_t stream);

// Rows 0 .. v_count-1 of `view` into the sparse form: row_of / off as above (window-local), entries written at
// off[r] (at most off[r + 1]), dense rows copied to pool row row_of[r].
hipError_t LaunchSparseEmit(const RowView &view, uint32_t v_count, const int32_t *row_of, const uint64_t *off,
                            uint32_t *entries, uint8_t *pool, hipStream_t stream);

// out[i] = {hom_ref, het, hom_alt, missing} of row v_first + i over the samples `include` keeps (NULL = all;
// n_out = how many it keeps).  Dense rows copy dense_counts[row_of - dense_first] (LaunchCounts over the pool).
hipError_t LaunchSparseCounts(const SparseView &sv, uint32_t v_first, uint32_t v_count, const uint64_t *include,
                              uint32_t n_out, const uint32_t *dense_counts, uint32_t dense_first, uint32_t *out,
                              hipStream_t stream);

// out[c * out_stride + s] += het / hom-alt / missing tallies of sample s over the SPARSE rows among
// (vlist ? vlist[i] : v_first + i), i < v_count; dense rows are skipped (LaunchClassCounts3 over the pool).
// entries_hint: about how many entries those rows hold (sizes the row slices).
hipError_t LaunchSparseSampleClasses(const SparseView &sv, uint32_t v_first, const uint32_t *vlist, uint32_t v_count,
                                     uint64_t entries_hint, uint32_t *out, uint32_t out_stride, hipStream_t stream);

// Rows v_first .. v_first + v_count - 1 back to 2-bit rows, dst_pitch bytes apart (a multiple of 4, >= sv.pitch is
// not needed: ceil(record_bytes / 4) words per row are written, pad slots zero).
hipError_t LaunchSparseExpand(const SparseView &sv, uint32_t v_first, uint32_t v_count, uint8_t *dst, uint64_t dst_pitch,
                              hipStream_t stream);

// ---- pgh_score_sparse (score_sparse.hip): plink_score's per-sample sums from the listed rows' entries ----
// The listed variant i is row vlist[i] of `sv`, with base code b_i (0 for a row held in the dense form, whose entries
// are then its samples with a code other than 0) and the tables ts / td / ac of LaunchScoreTables.  All sums are
// int64 fixed point: column c's terms are llrint(weights[i][c] (ts_i[g] - ts_i[b_i]) 2^kexp[c]), the dosage sum's
// (column index n_cols) llrint((td_i[g] - td_i[b_i]) 2^kexp[n_cols]).
constexpr uint32_t kScoreSparseChunk = 8;         // weight columns of one walk of the entries
constexpr uint32_t kScoreSparseAccBytes = 131072; // LDS of a sample tile's accumulators (of the 160 KiB)
constexpr uint32_t kScoreSparseParts = 32;        // partial sums per column of LaunchScoreSparseStats (a fixed shape)

// Samples of one LDS tile when n_acc int64 accumulators (weight columns, plus one for the dosage sum) and one uint32
// (the allele count) are kept per sample: the most that fit, a multiple of 64.
constexpr uint32_t ScoreSparseTile(uint32_t n_acc) {
	return kScoreSparseAccBytes / (8u * n_acc + 4u) / 64u * 64u;
}

// counts[i] = range_counts[vlist[i] - l_min] (uint32[4] each): the listed rows' counts out of a range's.
hipError_t LaunchScoreSparseGather(const uint32_t *range_counts, const uint32_t *vlist, uint32_t l_min,
                                   uint32_t n_scored, uint32_t *counts, hipStream_t stream);

// Per column c < n_cols, and for the dosage sum (c == n_cols, unit weights, td in the place of ts):
//   k0[c]   = sum_i weights[i][c] ts_i[b_i]: kScoreSparseParts partial sums over fixed runs of the list, each by a
//             fixed tree, added in order -- a function of column c alone;
//   kexp[c] = 62 - ceil(log2 n_scored) - e, with 2^e the power of two above the column's largest |term| (0 when every
//             term is 0): n_scored terms cannot carry an int64 sum past 2^62.
// alc0[0] = sum_i (the allele-count increment of ac[i] at code b_i).  part: (n_cols + 1) x kScoreSparseParts x 2
// doubles of scratch.
hipError_t LaunchScoreSparseStats(const SparseView &sv, const uint32_t *vlist, uint32_t n_scored, const double *weights,
                                  uint32_t n_cols, const double *ts, const double *td, const uint32_t *ac, double *part,
                                  double *k0, int32_t *kexp, uint32_t *alc0, hipStream_t stream);

// One walk of the listed rows for the columns [c0, c0 + n_chunk), n_chunk <= kScoreSparseChunk: adds the terms of
// the entries whose sample `include` keeps (NULL = all) into acc_score[s * n_cols + c] and, when acc_dos / acc_alc are
// not null, the dosage-sum terms into acc_dos[s] and the allele-count corrections into acc_alc[s] (raw samples; all
// zeroed by the caller before the first walk).  slices: row slices per sample tile, 0 = chosen from entries_hint
// (about how many entries the listed rows hold); integer adds, so the sums do not depend on it.
hipError_t LaunchScoreSparse(const SparseView &sv, const uint64_t *include, const uint32_t *vlist, uint32_t n_scored,
                             const double *weights, uint32_t n_cols, uint32_t c0, uint32_t n_chunk, const double *ts,
                             const double *td, const uint32_t *ac, const int32_t *kexp, uint64_t entries_hint,
                             uint32_t slices, unsigned long long *acc_score, unsigned long long *acc_dos,
                             uint32_t *acc_alc, hipStream_t stream);

// In place: acc_score[s * n_cols + c] becomes the double k0[c] + acc 2^-kexp[c], acc_dos[s] (may be null) the double
// k0[n_cols] + acc 2^-kexp[n_cols], acc_alc[s] += alc0[0].
hipError_t LaunchScoreSparseFlush(uint32_t sample_ct, uint32_t n_cols, const double *k0, const int32_t *kexp,
                                  const uint32_t *alc0, unsigned long long *acc_score, unsigned long long *acc_dos,
                                  uint32_t *acc_alc, hipStream_t stream);

} // namespace pgh
