// set_walk.hpp -- the member walk of the workgroup-per-set kernels (burden_sparse.hip, skat_sparse.hip): one resident
// row of a sparse-resident dataset (sparse.hpp), walked by a whole workgroup of kSetBlock threads.
#pragma once

#include "sparse.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pgh {

constexpr int kSetBlock = 256;

// The value base of a resident row from its row_of word: val(b) of a sparse row's base code b, 0 for a row held in the
// dense form (val(0, 1, 2, 3) = (0, 1, 2, 0)).
__device__ __forceinline__ int SetMemberBase(int32_t ro) {
	return ro < 0 && ro != -4 ? -1 - ro : 0;
}

// The entries of row v that count, at stride over the workgroup: f(sample, val(code) - val(base), y[sample]).  An
// entry counts when y[sample] is not NaN.  A dense-form row (ro >= 0) is read from its pool row as base 0 with one
// entry per sample whose code is 1 or 2, 16 samples per word per lane.
template <class F>
__device__ inline void WalkMember(const SparseView &sv, uint32_t v, int32_t ro, int vb, const double *__restrict__ y,
                                  int tid, F &&f) {
	if (ro < 0) {
		const uint64_t e0 = sv.off[v], e1 = sv.off[v + 1];
		for (uint64_t p = e0 + tid; p < e1; p += kSetBlock) {
			const uint32_t x = sv.entries[p];
			const uint32_t smp = x >> 2, code = x & 3u;
			if (smp < sv.sample_ct) {
				const double yi = y[smp];
				if (yi == yi) {
					f(smp, (code == 3u ? 0 : static_cast<int>(code)) - vb, yi);
				}
			}
		}
	} else {
		const uint32_t *row = reinterpret_cast<const uint32_t *>(sv.pool + static_cast<uint64_t>(ro) * sv.pitch);
		const uint32_t words = (sv.sample_ct + 15u) / 16u;
		for (uint32_t wi = tid; wi < words; wi += kSetBlock) {
			const uint32_t word = row[wi];
			uint32_t hit = (word ^ (word >> 1)) & 0x55555555u; // the low bit of every slot that holds 1 or 2
			while (hit) {
				const int bit = __ffs(static_cast<int>(hit)) - 1;
				hit &= hit - 1u;
				const uint32_t smp = wi * 16u + static_cast<uint32_t>(bit >> 1);
				if (smp < sv.sample_ct) {
					const double yi = y[smp];
					if (yi == yi) {
						f(smp, static_cast<int>((word >> bit) & 3u), yi);
					}
				}
			}
		}
	}
}

} // namespace pgh
