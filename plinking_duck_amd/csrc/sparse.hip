// sparse.hip -- gfx950 kernels of the sparse-resident form (sparse.hpp): classify and compact the rows of a decoded
// window, per-variant class counts, per-sample class tallies and the expansion back to 2-bit rows.
#include "device_utils.hpp"
#include "sparse.hpp"

#include <algorithm>

namespace pgh {

namespace {

constexpr uint64_t kLo = 0x5555555555555555ull;

// mask of the 2-bit slots of word wi (32 samples per uint64) that hold a sample
__device__ __forceinline__ uint64_t SlotMask(uint64_t wi, uint32_t sample_ct) {
	const uint64_t first = wi * 32;
	if (first + 32 <= sample_ct) {
		return ~0ull;
	}
	return first >= sample_ct ? 0ull : (1ull << (2 * (sample_ct - first))) - 1ull;
}

// One workgroup per row: the het / hom-alt / missing popcounts of the two bit-planes; hom-ref = N - the three, so
// whatever the pad slots hold cancels against N (they are masked off as well).
__global__ void __launch_bounds__(256) k_sparse_classify(const uint8_t *rows, uint64_t pitch, uint32_t sample_ct,
                                                         uint32_t v_count, uint32_t *out) {
	__shared__ uint32_t part[3][4];
	const uint64_t words = (static_cast<uint64_t>(sample_ct) + 31) / 32;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t r = blockIdx.x; r < v_count; r += gridDim.x) {
		const uint64_t *row = reinterpret_cast<const uint64_t *>(rows + static_cast<uint64_t>(r) * pitch);
		uint32_t het = 0, alt = 0, miss = 0;
		for (uint64_t w = threadIdx.x; w < words; w += blockDim.x) {
			const uint64_t x = row[w] & SlotMask(w, sample_ct);
			const uint64_t lo = x & kLo, hi = (x >> 1) & kLo;
			het += static_cast<uint32_t>(__popcll(lo & ~hi));
			alt += static_cast<uint32_t>(__popcll(hi & ~lo));
			miss += static_cast<uint32_t>(__popcll(lo & hi));
		}
		het = WaveSum(het);
		alt = WaveSum(alt);
		miss = WaveSum(miss);
		if (lane == 0) {
			part[0][wave] = het;
			part[1][wave] = alt;
			part[2][wave] = miss;
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t c[4];
			c[1] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
			c[2] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
			c[3] = part[2][0] + part[2][1] + part[2][2] + part[2][3];
			c[0] = sample_ct - c[1] - c[2] - c[3];
			uint32_t major = 0;
			for (uint32_t k = 1; k < 4; k++) {
				major = c[k] > c[major] ? k : major;
			}
			out[2ull * r] = major;
			out[2ull * r + 1] = sample_ct - c[major];
		}
		__syncthreads();
	}
}

// One workgroup per row.  Dense rows: a copy into the pool.  Sparse rows: 8192 samples per step, a uint64 word of
// 32 slots per lane; a lane's non-base slots are counted, a wave scan plus the four wave totals in LDS give each lane
// its first output slot, and the lane writes its entries in slot order -- ascending samples, no atomics, the same
// order every run.
__global__ void __launch_bounds__(256) k_sparse_emit(const uint8_t *rows, uint64_t pitch, uint32_t sample_ct,
                                                     uint32_t v_count, const int32_t *row_of, const uint64_t *off,
                                                     uint32_t *entries, uint8_t *pool) {
	__shared__ uint32_t wave_tot[4];
	const uint64_t words = (static_cast<uint64_t>(sample_ct) + 31) / 32;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t r = blockIdx.x; r < v_count; r += gridDim.x) {
		const uint8_t *src = rows + static_cast<uint64_t>(r) * pitch;
		const int32_t ro = row_of[r];
		if (ro >= 0) {
			const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
			uint4 *d4 = reinterpret_cast<uint4 *>(pool + static_cast<uint64_t>(ro) * pitch);
			for (uint64_t i = threadIdx.x; i < pitch / 16; i += blockDim.x) {
				d4[i] = s4[i];
			}
			continue; // (uniform across the block)
		}
		const uint64_t pattern = static_cast<uint64_t>(-1 - ro) * kLo;
		const uint64_t *row = reinterpret_cast<const uint64_t *>(src);
		uint64_t at = off[r];
		const uint64_t stop = off[r + 1];
		for (uint64_t w0 = 0; w0 < words; w0 += blockDim.x) {
			const uint64_t w = w0 + threadIdx.x;
			uint64_t x = 0, nz = 0;
			if (w < words) {
				x = row[w];
				const uint64_t d = x ^ pattern;
				nz = (d | (d >> 1)) & kLo & SlotMask(w, sample_ct);
			}
			const uint32_t cnt = static_cast<uint32_t>(__popcll(nz));
			uint32_t incl = cnt;
			for (int d = 1; d < 64; d <<= 1) {
				const uint32_t up = __shfl_up(incl, d, 64);
				incl += lane >= static_cast<uint32_t>(d) ? up : 0u;
			}
			if (lane == 63) {
				wave_tot[wave] = incl;
			}
			__syncthreads();
			uint32_t before = 0, total = 0;
			for (uint32_t k = 0; k < 4; k++) {
				before += k < wave ? wave_tot[k] : 0u;
				total += wave_tot[k];
			}
			uint64_t pos = at + before + incl - cnt;
			while (nz) {
				const uint32_t b = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(nz)) - 1);
				if (pos < stop) {
					entries[pos] = static_cast<uint32_t>((w * 32 + b / 2) << 2) | static_cast<uint32_t>((x >> b) & 3u);
				}
				pos++;
				nz &= nz - 1;
			}
			at += total;
			__syncthreads(); // wave_tot is rewritten by the next step
		}
	}
}

// One wave per row, four rows per workgroup.  Sparse rows: the entries' classes over the kept samples; the base
// class gets what is left of n_out.
__global__ void __launch_bounds__(256) k_sparse_counts(const int32_t *row_of, const uint64_t *off, const uint32_t *entries,
                                                       uint32_t v_first, uint32_t v_count, const uint64_t *include,
                                                       uint32_t n_out, const uint4 *dense_counts, uint32_t dense_first,
                                                       uint4 *out) {
	const uint32_t lane = threadIdx.x & 63u;
	for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < v_count; i += gridDim.x * 4) {
		const uint32_t r = v_first + i;
		const int32_t ro = row_of[r];
		if (ro >= 0) {
			if (lane == 0) {
				out[i] = dense_counts[static_cast<uint32_t>(ro) - dense_first];
			}
			continue;
		}
		uint32_t c[4] = {0, 0, 0, 0};
		const uint64_t e1 = off[r + 1];
		for (uint64_t e = off[r] + lane; e < e1; e += 64) {
			const uint32_t x = entries[e], s = x >> 2;
			if (!include || ((include[s >> 6] >> (s & 63u)) & 1ull)) {
				const uint32_t code = x & 3u;
				c[0] += code == 0;
				c[1] += code == 1;
				c[2] += code == 2;
				c[3] += code == 3;
			}
		}
		for (int k = 0; k < 4; k++) {
			c[k] = WaveSum(c[k]);
		}
		if (lane == 0) {
			const uint32_t base = static_cast<uint32_t>(-1 - ro);
			c[base] = n_out - (c[0] + c[1] + c[2] + c[3]); // entries never carry the base code
			out[i] = make_uint4(c[0], c[1], c[2], c[3]);
		}
	}
}

// Per-sample het / hom-alt / missing over the sparse rows.  A workgroup owns one tile of kSparseTile samples
// (privatised in LDS) and a slice of the rows; each wave takes a row, finds the tile's first entry by a 64-way
// search (the entries are sorted) and walks the tile's entries: +1 to the entry's class, -1 to the base class when
// the base is not hom-ref.  A per-base count of rows is added to every sample of the tile at the flush, one
// coalesced add per sample and class.  uint32 arithmetic is modular, so the -1s may wrap below zero on the way:
// every final tally is a true count in [0, rows], and sums mod 2^32 of such values are exact.
constexpr uint32_t kClassWaves = 16; // one 96 KB workgroup per CU: 16 waves keep enough searches in flight

__global__ void __launch_bounds__(64 * kClassWaves) k_sparse_sample_classes(const int32_t *row_of, const uint64_t *off,
                                                               const uint32_t *entries, uint32_t sample_ct,
                                                               uint32_t v_first, const uint32_t *vlist,
                                                               uint32_t v_count, uint32_t slice_len, uint32_t *out,
                                                               uint32_t out_stride) {
	__shared__ uint32_t cls[3][kSparseTile];
	__shared__ uint32_t base_rows[4];
	const uint32_t t0 = blockIdx.x * kSparseTile;
	const uint32_t t1 = std::min<uint32_t>(sample_ct, t0 + kSparseTile);
	for (uint32_t j = threadIdx.x; j < 3 * kSparseTile; j += blockDim.x) {
		(&cls[0][0])[j] = 0;
	}
	if (threadIdx.x < 4) {
		base_rows[threadIdx.x] = 0;
	}
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t i0 = blockIdx.y * slice_len;
	const uint32_t i1 = std::min<uint32_t>(v_count, i0 + slice_len);
	for (uint32_t i = i0 + wave; i < i1; i += kClassWaves) {
		const uint32_t r = vlist ? vlist[i] : v_first + i;
		const int32_t ro = row_of[r];
		if (ro >= 0) {
			continue; // dense: tallied over the pool
		}
		const uint32_t base = static_cast<uint32_t>(-1 - ro);
		if (lane == 0) {
			atomicAdd(&base_rows[base], 1u);
		}
		const uint64_t e1 = off[r + 1];
		for (uint64_t e = WaveLowerBound(entries, off[r], e1, t0, lane);; e += 64) {
			const uint64_t p = e + lane;
			const uint32_t x = p < e1 ? entries[p] : 0xffffffffu;
			const uint32_t s = x >> 2;
			if (p < e1 && s < t1) {
				const uint32_t code = x & 3u;
				if (code != 0) {
					atomicAdd(&cls[code - 1][s - t0], 1u);
				}
				if (base != 0) {
					atomicAdd(&cls[base - 1][s - t0], 0xffffffffu); // -1
				}
			}
			// the last lane's entry lies beyond the tile (or the row): nothing of the tile is left
			if (__shfl(static_cast<int>(p < e1 && s < t1), 63, 64) == 0) {
				break;
			}
		}
	}
	__syncthreads();
	for (uint32_t j = threadIdx.x; t0 + j < t1; j += blockDim.x) {
		for (uint32_t c = 0; c < 3; c++) {
			const uint32_t v = cls[c][j] + base_rows[c + 1];
			if (v) {
				atomicAdd(&out[static_cast<uint64_t>(c) * out_stride + t0 + j], v);
			}
		}
	}
}

// One uint32 output word (16 samples) per lane: dense rows copy the pool's word, sparse rows start from the base
// pattern and patch the word's entries (found by binary search).
__global__ void __launch_bounds__(256) k_sparse_expand(const int32_t *row_of, const uint64_t *off, const uint32_t *entries,
                                                       const uint8_t *pool, uint64_t pitch, uint32_t sample_ct,
                                                       uint32_t v_first, uint32_t v_count, uint32_t *dst,
                                                       uint64_t dst_words) {
	const uint32_t words = (sample_ct + 15) / 16;
	for (uint32_t i = blockIdx.y; i < v_count; i += gridDim.y) {
		const uint32_t r = v_first + i;
		const int32_t ro = row_of[r];
		for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < words; w += gridDim.x * blockDim.x) {
			uint32_t x;
			if (ro >= 0) {
				x = reinterpret_cast<const uint32_t *>(pool + static_cast<uint64_t>(ro) * pitch)[w];
			} else {
				x = static_cast<uint32_t>(-1 - ro) * 0x55555555u;
				uint64_t lo = off[r], hi = off[r + 1];
				const uint32_t s0 = w * 16;
				while (lo < hi) {
					const uint64_t mid = (lo + hi) / 2;
					if ((entries[mid] >> 2) < s0) {
						lo = mid + 1;
					} else {
						hi = mid;
					}
				}
				for (uint64_t e = lo; e < off[r + 1]; e++) {
					const uint32_t y = entries[e], s = y >> 2;
					if (s >= s0 + 16) {
						break;
					}
					const uint32_t sh = 2 * (s - s0);
					x = (x & ~(3u << sh)) | ((y & 3u) << sh);
				}
				if (s0 + 16 > sample_ct) {
					x &= (1u << (2 * (sample_ct - s0))) - 1u;
				}
			}
			dst[static_cast<uint64_t>(i) * dst_words + w] = x;
		}
	}
}

uint32_t GridOf(uint64_t blocks) {
	return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(blocks, 1u << 20)));
}

} // namespace

hipError_t LaunchSparseClassify(const RowView &view, uint32_t v_count, uint32_t *out, hipStream_t stream) {
	if (v_count == 0) {
		return hipSuccess;
	}
	hipLaunchKernelGGL(k_sparse_classify, dim3(GridOf(v_count)), dim3(256), 0, stream, view.rows, view.pitch,
	                   view.sample_ct, v_count, out);
	return hipGetLastError();
}

hipError_t LaunchSparseEmit(const RowView &view, uint32_t v_count, const int32_t *row_of, const uint64_t *off,
                            uint32_t *entries, uint8_t *pool, hipStream_t stream) {
	if (v_count == 0) {
		return hipSuccess;
	}
	hipLaunchKernelGGL(k_sparse_emit, dim3(GridOf(v_count)), dim3(256), 0, stream, view.rows, view.pitch,
	                   view.sample_ct, v_count, row_of, off, entries, pool);
	return hipGetLastError();
}

hipError_t LaunchSparseCounts(const SparseView &sv, uint32_t v_first, uint32_t v_count, const uint64_t *include,
                              uint32_t n_out, const uint32_t *dense_counts, uint32_t dense_first, uint32_t *out,
                              hipStream_t stream) {
	if (v_count == 0) {
		return hipSuccess;
	}
	hipLaunchKernelGGL(k_sparse_counts, dim3(GridOf((v_count + 3) / 4)), dim3(256), 0, stream, sv.row_of, sv.off,
	                   sv.entries, v_first, v_count, include, n_out, reinterpret_cast<const uint4 *>(dense_counts),
	                   dense_first, reinterpret_cast<uint4 *>(out));
	return hipGetLastError();
}

hipError_t LaunchSparseSampleClasses(const SparseView &sv, uint32_t v_first, const uint32_t *vlist, uint32_t v_count,
                                     uint64_t entries_hint, uint32_t *out, uint32_t out_stride, hipStream_t stream) {
	if (v_count == 0 || sv.sample_ct == 0) {
		return hipSuccess;
	}
	const uint32_t tiles = (sv.sample_ct + kSparseTile - 1) / kSparseTile;
	// ~512 workgroups (two rounds of one per CU), but few enough slices that the flush (3 adds per sample and slice)
	// stays below a sixth of the entries' LDS adds, and at least 4 rows per wave
	uint32_t slices = std::max<uint32_t>(1, (512 + tiles - 1) / tiles);
	slices = std::min<uint64_t>(slices, std::max<uint64_t>(1, entries_hint / (18ull * sv.sample_ct)));
	slices = std::min<uint32_t>(slices, std::max<uint32_t>(1, v_count / (4 * kClassWaves)));
	slices = std::min<uint32_t>(slices, 65535);
	const uint32_t slice_len = (v_count + slices - 1) / slices;
	slices = (v_count + slice_len - 1) / slice_len;
	hipLaunchKernelGGL(k_sparse_sample_classes, dim3(tiles, slices), dim3(64 * kClassWaves), 0, stream, sv.row_of, sv.off, sv.entries,
	                   sv.sample_ct, v_first, vlist, v_count, slice_len, out, out_stride);
	return hipGetLastError();
}

hipError_t LaunchSparseExpand(const SparseView &sv, uint32_t v_first, uint32_t v_count, uint8_t *dst, uint64_t dst_pitch,
                              hipStream_t stream) {
	if (v_count == 0) {
		return hipSuccess;
	}
	const uint32_t words = (sv.sample_ct + 15) / 16;
	const uint32_t gx = std::min<uint32_t>((words + 255) / 256, 1024);
	const uint32_t gy = std::min<uint32_t>(v_count, 65535);
	hipLaunchKernelGGL(k_sparse_expand, dim3(std::max<uint32_t>(1, gx), gy), dim3(256), 0, stream, sv.row_of, sv.off,
	                   sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, v_count, reinterpret_cast<uint32_t *>(dst),
	                   dst_pitch / 4);
	return hipGetLastError();
}

} // namespace pgh
