// het.hpp -- launch wrapper of pgh_het's kernel (het.hip).
// All pointers are device pointers; the wrapper only enqueues work on `stream`.
#pragma once

#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pgh {

constexpr uint32_t kHetTile = 4096;       // samples per workgroup tile: 1 KiB of a row, 32 KiB of int64 sums in LDS
constexpr uint32_t kHetMaxSlices = 65535; // grid.y

// The variant slices a launch over n_rows rows of sample_ct samples takes by default on a device of `cus` compute
// units: enough workgroups to fill it four times over, never less than 64 rows to a slice.
uint32_t HetDefaultSlices(uint32_t sample_ct, uint32_t n_rows, int cus);

// msum[s] = sum of q[i] over the rows i < n_rows (row vlist[i] of the view) at which raw sample s is missing, in
// wrapping 64-bit integer arithmetic, for s < view.sample_ct.  msum is zeroed on the stream first.  slices: variant
// slices of the grid, 1 .. kHetMaxSlices (clamped); the result does not depend on it.
hipError_t LaunchHetMissingSum(const RowView &view, const uint32_t *vlist, uint32_t n_rows, const unsigned long long *q,
                               uint32_t slices, unsigned long long *msum, hipStream_t stream);

} // namespace pgh
