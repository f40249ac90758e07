// het.hip -- k_het_missing_sum: per raw sample, the sum of a per-variant 64-bit weight over the variants at which the
// sample is MISSING (pgh_het, api_het.cpp).
//
// Grid: (sample tiles of kHetTile samples) x (variant slices).  A workgroup keeps its tile's int64 sums in LDS; its
// waves take the slice's rows in turn, a lane loads 16 bytes (64 samples) of a row, forms the missing mask
// w & (w >> 1) & 0x5555.. and adds the row's weight to the LDS sum of every sample whose bit is set.  At the end the
// tile goes into msum with 64-bit global atomic adds.  Everything added is an integer, so neither the order of the
// adds nor the grid changes a bit of the result.
#include "het.hpp"

#include <algorithm>

namespace pgh {

namespace {

constexpr uint32_t kHetWaves = 8; // waves per workgroup
constexpr uint32_t kHetDepth = 4; // rows a wave has in flight

static_assert(kHetTile == 64 * 64, "a lane's 16 bytes hold 64 samples, a wave's load the whole tile");

// A lane's 64 samples as one 64-bit mask: the even bits of dwords 0 and 1 of its 16 bytes interleaved in the low
// word, those of dwords 2 and 3 in the high word -- bit 32 h + 2 j + c is sample j of dword 2 h + c, sample
// 16 (2 h + c) + j of the lane.
__device__ __forceinline__ uint32_t HetBitOf(uint32_t sample_in_lane) {
	const uint32_t dword = sample_in_lane >> 4;
	return (dword >> 1) * 32u + 2u * (sample_in_lane & 15u) + (dword & 1u);
}

// LDS slot of bit b of lane's mask: the bit index itself picks the row of 64 slots, so the loop over the set bits
// decodes nothing, and lanes that add at the same bit land on consecutive 8-byte words (the natural order
// 64 lane + sample would put all 64 lanes of an add on one bank).  Measured against decoding the sample in the loop:
// 22.9 against 23.5 ms at 2 % missing calls, 87 against 134 ms at 50 %.
__device__ __forceinline__ uint32_t HetSlot(uint32_t lane, uint32_t b) {
	return b * 64u + lane;
}

__global__ __launch_bounds__(64 * kHetWaves) void k_het_missing_sum(const uint8_t *__restrict__ rows, uint64_t pitch,
                                                                   uint32_t sample_ct,
                                                                   const uint32_t *__restrict__ vlist, uint32_t n_rows,
                                                                   const unsigned long long *__restrict__ q,
                                                                   uint32_t slice_len,
                                                                   unsigned long long *__restrict__ msum) {
	__shared__ unsigned long long acc[kHetTile];
	for (uint32_t j = threadIdx.x; j < kHetTile; j += 64 * kHetWaves) {
		acc[j] = 0;
	}
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	// the lane's 16 bytes of every row; pitch is a multiple of 16, so a chunk that starts inside a row ends inside it.
	// Bits past sample_ct and the bytes up to pitch are zero in the resident rows: they never count.
	const uint64_t off = static_cast<uint64_t>(blockIdx.x) * (kHetTile / 4) + lane * 16u;
	const bool inside = off < pitch;
	const uint64_t i0 = static_cast<uint64_t>(blockIdx.y) * slice_len;
	const uint64_t i1 = std::min<uint64_t>(n_rows, i0 + slice_len);
	for (uint64_t i = i0 + wave; i < i1; i += kHetWaves * kHetDepth) {
		uint4 w[kHetDepth];
		unsigned long long qv[kHetDepth];
#pragma unroll
		for (uint32_t d = 0; d < kHetDepth; d++) {
			const uint64_t idx = i + d * kHetWaves; // the same for the whole wave
			w[d] = make_uint4(0, 0, 0, 0);
			qv[d] = 0;
			if (idx < i1) {
				qv[d] = q[idx];
				if (inside) {
					w[d] = *reinterpret_cast<const uint4 *>(rows + static_cast<uint64_t>(vlist[idx]) * pitch + off);
				}
			}
		}
#pragma unroll
		for (uint32_t d = 0; d < kHetDepth; d++) {
			const uint32_t m0 = w[d].x & (w[d].x >> 1) & 0x55555555u, m1 = w[d].y & (w[d].y >> 1) & 0x55555555u;
			const uint32_t m2 = w[d].z & (w[d].z >> 1) & 0x55555555u, m3 = w[d].w & (w[d].w >> 1) & 0x55555555u;
			unsigned long long m = static_cast<unsigned long long>(m0 | (m1 << 1)) |
			                       (static_cast<unsigned long long>(m2 | (m3 << 1)) << 32);
			while (m) {
				const uint32_t b = static_cast<uint32_t>(__ffsll(static_cast<long long>(m))) - 1u;
				atomicAdd(&acc[HetSlot(lane, b)], qv[d]);
				m &= m - 1ull;
			}
		}
	}
	__syncthreads();
	const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kHetTile;
	for (uint32_t j = threadIdx.x; j < kHetTile; j += 64 * kHetWaves) {
		const unsigned long long v = acc[HetSlot(j >> 6, HetBitOf(j & 63u))];
		if (v != 0 && t0 + j < sample_ct) {
			atomicAdd(&msum[t0 + j], v);
		}
	}
}

} // namespace

uint32_t HetDefaultSlices(uint32_t sample_ct, uint32_t n_rows, int cus) {
	const uint64_t tiles = std::max<uint64_t>(1, (static_cast<uint64_t>(sample_ct) + kHetTile - 1) / kHetTile);
	// four workgroups fit a compute unit; four rounds of them even out the tiles' unequal shares of missing calls
	// (measured at 1M x 500k with the kernel's first version: 34 slices, this rule's choice, 73 ms a call against 76 ms
	// with 17 at 2 % missing calls and 176 against 192 ms at 50 %)
	const uint64_t target = 16ull * static_cast<uint32_t>(std::max(cus, 1));
	const uint64_t want = (target + tiles - 1) / tiles;
	const uint64_t most = std::max<uint64_t>(1, n_rows / 64);
	return static_cast<uint32_t>(std::min<uint64_t>(std::min(want, most), kHetMaxSlices));
}

hipError_t LaunchHetMissingSum(const RowView &view, const uint32_t *vlist, uint32_t n_rows, const unsigned long long *q,
                               uint32_t slices, unsigned long long *msum, hipStream_t stream) {
	hipError_t e = hipMemsetAsync(msum, 0, sizeof(unsigned long long) * static_cast<size_t>(view.sample_ct), stream);
	if (e != hipSuccess || n_rows == 0 || view.sample_ct == 0) {
		return e;
	}
	slices = std::min(std::max(slices, 1u), std::min(n_rows, kHetMaxSlices));
	const uint32_t slice_len = (n_rows + slices - 1) / slices;
	slices = (n_rows + slice_len - 1) / slice_len; // no empty slice
	const uint32_t tiles = static_cast<uint32_t>((static_cast<uint64_t>(view.sample_ct) + kHetTile - 1) / kHetTile);
	hipLaunchKernelGGL(k_het_missing_sum, dim3(tiles, slices), dim3(64 * kHetWaves), 0, stream, view.rows, view.pitch,
	                   view.sample_ct, vlist, n_rows, q, slice_len, msum);
	return hipGetLastError();
}

} // namespace pgh
