// score_sparse.hip -- pgh_score_sparse: plink_score's per-sample sums (src/plink_score.cpp:598-652, hardcalls) from
// the entries of a sparse-resident dataset (launch wrappers in sparse.hpp).
//
// For the listed variant i with base code b_i (0 for a row held in the dense form, whose entries are then its samples
// with a code other than 0) and the tables ts_i / td_i / ac_i of LaunchScoreTables over the subset's counts:
//   score[s][c] = K_c + sum over the entries (i, g) of sample s of W[i][c] (ts_i[g] - ts_i[b_i]),
//   K_c         = sum_i W[i][c] ts_i[b_i],
// the dosage sum likewise with td and unit weights, and the allele count with the integer increments of ac_i.
// A skipped variant (no call in the subset; sd == 0 under CENTER) has all-zero tables and adds nothing.
//
// Every per-sample sum is int64 FIXED POINT: column c has one scale 2^kexp[c], chosen from the column's largest |term|
// and n_scored so that no sample's sum can pass 2^62, each term is llrint(term 2^kexp[c]), and the flush writes
// K_c + (double)sum 2^-kexp[c].  Integer adds commute: LDS atomics, global atomics across the row slices and any grid
// give the same bytes, and a column is a function of its own weights alone.
//
// k_score_sparse has k_sparse_sample_classes' shape (sparse.hip): a workgroup owns one tile of samples, privatised in
// LDS, and a slice of the listed rows; a wave takes a row, finds the tile's first entry by a 64-way search and walks
// the tile's entries; of a dense-form row it reads the tile's words from the pool.  The weight columns go through in
// chunks of kScoreSparseChunk, one walk each; the first walk also carries the dosage sum and the allele count.
#include "sparse.hpp"

#include <algorithm>

namespace pgh {

namespace {

constexpr uint32_t kWaves = 16; // one workgroup per CU (its LDS): 16 waves keep enough searches in flight
constexpr uint32_t kStatBlock = 256;

__device__ __forceinline__ uint32_t BaseOf(int32_t ro) {
	return ro < 0 ? static_cast<uint32_t>(-1 - ro) : 0u;
}

// the allele-count increment of a call with `code` at a variant whose increments are `ac` (LaunchScoreTables)
__device__ __forceinline__ uint32_t AlleleInc(uint32_t ac, uint32_t code) {
	return code == 3u ? (ac >> 8) & 0xffu : ac & 0xffu;
}

__global__ __launch_bounds__(256) void k_score_sparse_gather(const uint4 *__restrict__ range_counts,
                                                             const uint32_t *__restrict__ vlist, uint32_t l_min,
                                                             uint32_t n_scored, uint4 *__restrict__ counts) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n_scored) {
		counts[i] = range_counts[vlist[i] - l_min];
	}
}

// Workgroup (c, p): run p of the list for column c.  A thread adds its variants in list order, the threads are folded
// by a fixed tree: the partial sum depends on (c, p, n_scored) alone.  The largest |term| is a maximum, exact in any
// order.  Column n_cols is the dosage sum; its workgroups also total the allele-count increments at the base codes
// (integers: any order).
__global__ __launch_bounds__(kStatBlock) void k_score_sparse_stats(const int32_t *__restrict__ row_of,
                                                                   const uint32_t *__restrict__ vlist, uint32_t n_scored,
                                                                   const double *__restrict__ weights, uint32_t n_cols,
                                                                   const double *__restrict__ ts,
                                                                   const double *__restrict__ td,
                                                                   const uint32_t *__restrict__ ac, uint32_t run,
                                                                   double *__restrict__ part, uint32_t *__restrict__ alc0) {
	__shared__ double sum_s[kStatBlock], max_s[kStatBlock];
	__shared__ uint32_t alc_s[kStatBlock];
	const uint32_t c = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
	const bool dos = c == n_cols;
	const double *tab = dos ? td : ts;
	const uint64_t i0 = static_cast<uint64_t>(p) * run;
	const uint64_t i1 = std::min<uint64_t>(n_scored, i0 + run);
	double sum = 0.0, mx = 0.0;
	uint32_t alc = 0;
	for (uint64_t i = i0 + tid; i < i1; i += kStatBlock) {
		const uint32_t b = BaseOf(row_of[vlist[i]]);
		const double w = dos ? 1.0 : weights[i * n_cols + c];
		const double *t = tab + 4 * i;
		const double tb = t[b];
		sum += w * tb;
		for (uint32_t g = 0; g < 4; g++) {
			mx = fmax(mx, fabs(w * (t[g] - tb)));
		}
		alc += dos ? AlleleInc(ac[i], b) : 0u;
	}
	sum_s[tid] = sum;
	max_s[tid] = mx;
	alc_s[tid] = alc;
	__syncthreads();
	for (uint32_t h = kStatBlock / 2; h > 0; h >>= 1) {
		if (tid < h) {
			sum_s[tid] += sum_s[tid + h];
			max_s[tid] = fmax(max_s[tid], max_s[tid + h]);
			alc_s[tid] += alc_s[tid + h];
		}
		__syncthreads();
	}
	if (tid == 0) {
		double *o = part + 2ull * (static_cast<uint64_t>(c) * kScoreSparseParts + p);
		o[0] = sum_s[0];
		o[1] = max_s[0];
		if (dos && alc_s[0]) {
			atomicAdd(alc0, alc_s[0]);
		}
	}
}

// One thread per column: the partial sums in order, and the scale.
__global__ __launch_bounds__(256) void k_score_sparse_scales(const double *__restrict__ part, uint32_t n_total,
                                                             uint32_t n_scored, double *__restrict__ k0,
                                                             int32_t *__restrict__ kexp) {
	const uint32_t c = blockIdx.x * 256u + threadIdx.x;
	if (c >= n_total) {
		return;
	}
	const double *o = part + 2ull * c * kScoreSparseParts;
	double sum = 0.0, mx = 0.0;
	for (uint32_t p = 0; p < kScoreSparseParts; p++) {
		sum += o[2 * p];
		mx = fmax(mx, o[2 * p + 1]);
	}
	k0[c] = sum;
	int32_t k = 0;
	if (mx > 0.0) {
		int e = 0;
		(void)frexp(mx, &e); // mx < 2^e
		const int32_t lg = n_scored > 1 ? 32 - __clz(static_cast<int>(n_scored - 1)) : 0; // n_scored <= 2^lg
		k = 62 - lg - e;
	}
	kexp[c] = k;
}

__global__ __launch_bounds__(64 * kWaves) void k_score_sparse(const SparseView sv, const uint64_t *__restrict__ include,
                                                               const uint32_t *__restrict__ vlist, uint32_t n_scored,
                                                               const double *__restrict__ weights, uint32_t n_cols,
                                                               uint32_t c0, uint32_t n_chunk,
                                                               const double *__restrict__ ts,
                                                               const double *__restrict__ td,
                                                               const uint32_t *__restrict__ ac,
                                                               const int32_t *__restrict__ kexp, uint32_t tile,
                                                               uint32_t slice_len, unsigned long long *__restrict__ acc_score,
                                                               unsigned long long *__restrict__ acc_dos,
                                                               uint32_t *__restrict__ acc_alc) {
	// sample-major: n_acc int64 sums per sample of the tile, then one uint32 per sample (ScoreSparseTile)
	__shared__ unsigned long long lds[kScoreSparseAccBytes / 8];
	const uint32_t n_acc = n_chunk + (acc_dos ? 1u : 0u);
	unsigned long long *acc = lds;
	uint32_t *alc = reinterpret_cast<uint32_t *>(lds + static_cast<uint64_t>(tile) * n_acc);
	const uint32_t t0 = blockIdx.x * tile;
	const uint32_t t1 = std::min<uint32_t>(sv.sample_ct, t0 + tile);
	for (uint32_t j = threadIdx.x; j < tile * n_acc; j += blockDim.x) {
		acc[j] = 0;
	}
	for (uint32_t j = threadIdx.x; j < tile; j += blockDim.x) {
		alc[j] = 0;
	}
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t i0 = blockIdx.y * slice_len;
	const uint32_t i1 = std::min<uint32_t>(n_scored, i0 + slice_len);
	for (uint32_t i = i0 + wave; i < i1; i += kWaves) {
		const uint32_t r = vlist[i];
		const int32_t ro = sv.row_of[r];
		const uint32_t base = BaseOf(ro);
		uint64_t e = 0, e1 = 0;
		if (ro < 0) {
			e1 = sv.off[r + 1];
			e = WaveLowerBound(sv.entries, sv.off[r], e1, t0, lane);
			if (e >= e1 || (sv.entries[e] >> 2) >= t1) {
				continue; // nothing of this row in the tile (the whole wave)
			}
		}
		// lane 4 c + g holds the fixed-point term of accumulator c for a call g at this variant
		long long term = 0;
		if (lane < 4 * n_acc) {
			const uint32_t c = lane >> 2, g = lane & 3u;
			double d;
			int32_t k;
			if (c < n_chunk) {
				const double *t = ts + 4ull * i;
				d = weights[static_cast<uint64_t>(i) * n_cols + c0 + c] * (t[g] - t[base]);
				k = kexp[c0 + c];
			} else {
				const double *t = td + 4ull * i;
				d = t[g] - t[base];
				k = kexp[n_cols];
			}
			term = llrint(scalbn(d, k));
		}
		const uint32_t inc = acc_alc ? ac[i] : 0u;
		const uint32_t inc_base = AlleleInc(inc, base);
		// every lane takes part in the shuffles; `hit` says whether its call counts
		auto add = [&](bool hit, uint32_t s, uint32_t code) {
			for (uint32_t c = 0; c < n_acc; c++) {
				const long long v = __shfl(term, static_cast<int>(4 * c + code), 64);
				if (hit && v != 0) {
					atomicAdd(&acc[static_cast<uint64_t>(s - t0) * n_acc + c], static_cast<unsigned long long>(v));
				}
			}
			const uint32_t dv = AlleleInc(inc, code) - inc_base; // (modular: the corrections may be negative)
			if (hit && dv != 0) {
				atomicAdd(&alc[s - t0], dv);
			}
		};
		if (ro < 0) {
			for (;; e += 64) {
				const uint64_t p = e + lane;
				const uint32_t x = p < e1 ? sv.entries[p] : 0xffffffffu;
				const uint32_t s = x >> 2;
				const bool in = p < e1 && s < t1;
				const bool hit = in && (!include || ((include[s >> 6] >> (s & 63u)) & 1ull));
				add(hit, s, in ? (x & 3u) : 0u);
				// the last lane's entry lies beyond the tile (or the row): nothing of the tile is left
				if (__shfl(static_cast<int>(in), 63, 64) == 0) {
					break;
				}
			}
		} else {
			// the tile's part of the pool row, 16 samples per word per lane, slot by slot (t0 is a multiple of 64)
			const uint32_t *row = reinterpret_cast<const uint32_t *>(sv.pool + static_cast<uint64_t>(ro) * sv.pitch);
			for (uint32_t w0 = t0 / 16; w0 * 16 < t1; w0 += 64) {
				const uint32_t w = w0 + lane;
				const uint32_t word = w * 16 < t1 ? row[w] : 0u;
				for (uint32_t slot = 0; slot < 16; slot++) {
					const uint32_t code = (word >> (2 * slot)) & 3u;
					const uint32_t s = w * 16 + slot;
					const bool in = code != 0 && s < t1;
					if (__ballot(in) == 0) {
						continue; // (the whole wave)
					}
					const bool hit = in && (!include || ((include[s >> 6] >> (s & 63u)) & 1ull));
					add(hit, s, code);
				}
			}
		}
	}
	__syncthreads();
	const uint32_t n_tile = t1 > t0 ? t1 - t0 : 0u;
	for (uint32_t idx = threadIdx.x; idx < n_tile * n_acc; idx += blockDim.x) {
		const unsigned long long v = acc[idx];
		if (v != 0) {
			const uint32_t j = idx / n_acc, c = idx - j * n_acc;
			const uint64_t s = t0 + j;
			atomicAdd(c < n_chunk ? &acc_score[s * n_cols + c0 + c] : &acc_dos[s], v);
		}
	}
	if (acc_alc) {
		for (uint32_t j = threadIdx.x; j < n_tile; j += blockDim.x) {
			const uint32_t v = alc[j];
			if (v != 0) {
				atomicAdd(&acc_alc[t0 + j], v);
			}
		}
	}
}

__global__ __launch_bounds__(256) void k_score_sparse_flush(uint64_t n, uint32_t n_cols, uint32_t col_first,
                                                            const double *__restrict__ k0,
                                                            const int32_t *__restrict__ kexp,
                                                            unsigned long long *__restrict__ acc) {
	for (uint64_t idx = blockIdx.x * 256ull + threadIdx.x; idx < n; idx += gridDim.x * 256ull) {
		const uint32_t c = col_first + static_cast<uint32_t>(idx % n_cols);
		const double sum = static_cast<double>(static_cast<long long>(acc[idx]));
		acc[idx] = static_cast<unsigned long long>(__double_as_longlong(k0[c] + scalbn(sum, -kexp[c])));
	}
}

__global__ __launch_bounds__(256) void k_score_sparse_flush_alc(uint32_t sample_ct, const uint32_t *__restrict__ alc0,
                                                                uint32_t *__restrict__ acc_alc) {
	const uint32_t add = alc0[0];
	for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < sample_ct; s += gridDim.x * 256u) {
		acc_alc[s] += add;
	}
}

uint32_t FlushGrid(uint64_t n) {
	return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 4096)));
}

} // namespace

hipError_t LaunchScoreSparseGather(const uint32_t *range_counts, const uint32_t *vlist, uint32_t l_min,
                                   uint32_t n_scored, uint32_t *counts, hipStream_t stream) {
	if (n_scored == 0) {
		return hipSuccess;
	}
	hipLaunchKernelGGL(k_score_sparse_gather, dim3((n_scored + 255) / 256), dim3(256), 0, stream,
	                   reinterpret_cast<const uint4 *>(range_counts), vlist, l_min, n_scored,
	                   reinterpret_cast<uint4 *>(counts));
	return hipGetLastError();
}

hipError_t LaunchScoreSparseStats(const SparseView &sv, const uint32_t *vlist, uint32_t n_scored, const double *weights,
                                  uint32_t n_cols, const double *ts, const double *td, const uint32_t *ac, double *part,
                                  double *k0, int32_t *kexp, uint32_t *alc0, hipStream_t stream) {
	if (n_scored == 0 || n_cols == 0 || n_cols >= 65535) {
		return hipErrorInvalidValue;
	}
	hipError_t e = hipMemsetAsync(alc0, 0, sizeof(uint32_t), stream);
	if (e != hipSuccess) {
		return e;
	}
	const uint32_t run = (n_scored + kScoreSparseParts - 1) / kScoreSparseParts;
	hipLaunchKernelGGL(k_score_sparse_stats, dim3(n_cols + 1, kScoreSparseParts), dim3(kStatBlock), 0, stream, sv.row_of,
	                   vlist, n_scored, weights, n_cols, ts, td, ac, run, part, alc0);
	hipLaunchKernelGGL(k_score_sparse_scales, dim3((n_cols + 1 + 255) / 256), dim3(256), 0, stream, part, n_cols + 1,
	                   n_scored, k0, kexp);
	return hipGetLastError();
}

hipError_t LaunchScoreSparse(const SparseView &sv, const uint64_t *include, const uint32_t *vlist, uint32_t n_scored,
                             const double *weights, uint32_t n_cols, uint32_t c0, uint32_t n_chunk, const double *ts,
                             const double *td, const uint32_t *ac, const int32_t *kexp, uint64_t entries_hint,
                             uint32_t slices, unsigned long long *acc_score, unsigned long long *acc_dos,
                             uint32_t *acc_alc, hipStream_t stream) {
	if (n_chunk == 0 || n_chunk > kScoreSparseChunk || c0 + n_chunk > n_cols) {
		return hipErrorInvalidValue;
	}
	if (n_scored == 0 || sv.sample_ct == 0) {
		return hipSuccess;
	}
	const uint32_t tile = ScoreSparseTile(n_chunk + (acc_dos ? 1u : 0u));
	const uint32_t tiles = (sv.sample_ct + tile - 1) / tile;
	if (slices == 0) {
		// ~512 workgroups (two rounds of one per CU), but few enough slices that the flush (one global add per
		// sample, accumulator and slice) stays below a sixth of the entries' LDS adds, and at least 4 rows per wave
		slices = std::max<uint32_t>(1, (512 + tiles - 1) / tiles);
		slices = std::min<uint64_t>(slices, std::max<uint64_t>(1, entries_hint / (6ull * sv.sample_ct)));
		slices = std::min<uint32_t>(slices, std::max<uint32_t>(1, n_scored / (4 * kWaves)));
	}
	slices = std::max<uint32_t>(1, std::min<uint32_t>(std::min<uint32_t>(slices, n_scored), 65535));
	const uint32_t slice_len = (n_scored + slices - 1) / slices;
	slices = (n_scored + slice_len - 1) / slice_len;
	hipLaunchKernelGGL(k_score_sparse, dim3(tiles, slices), dim3(64 * kWaves), 0, stream, sv, include, vlist, n_scored,
	                   weights, n_cols, c0, n_chunk, ts, acc_dos ? td : nullptr, ac, kexp, tile, slice_len, acc_score,
	                   acc_dos, acc_alc);
	return hipGetLastError();
}

hipError_t LaunchScoreSparseFlush(uint32_t sample_ct, uint32_t n_cols, const double *k0, const int32_t *kexp,
                                  const uint32_t *alc0, unsigned long long *acc_score, unsigned long long *acc_dos,
                                  uint32_t *acc_alc, hipStream_t stream) {
	if (sample_ct == 0) {
		return hipSuccess;
	}
	const uint64_t n = static_cast<uint64_t>(sample_ct) * n_cols;
	hipLaunchKernelGGL(k_score_sparse_flush, dim3(FlushGrid(n)), dim3(256), 0, stream, n, n_cols, 0u, k0, kexp, acc_score);
	if (acc_dos) {
		hipLaunchKernelGGL(k_score_sparse_flush, dim3(FlushGrid(sample_ct)), dim3(256), 0, stream,
		                   static_cast<uint64_t>(sample_ct), 1u, n_cols, k0, kexp, acc_dos);
	}
	hipLaunchKernelGGL(k_score_sparse_flush_alc, dim3(FlushGrid(sample_ct)), dim3(256), 0, stream, sample_ct, alc0,
	                   acc_alc);
	return hipGetLastError();
}

} // namespace pgh
