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

} // namespace pgh
