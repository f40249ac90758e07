// grm.hip -- variance-standardised relationship matrix on the FP64 matrix cores (pgh_grm).
//
//   rel_ij = (sum over used variants v of z_iv z_jv) / nobs_ij        z_iv = table[v][code of sample i at v]
//   nobs_ij = number of used variants at which both i and j are called
//
// The numerator is a real Gram product, so it runs on v_mfma_f64_16x16x4_f64; the denominator is KING's MM, one
// v_mfma_i32_16x16x64_i8 product of the "called" planes.  Neither operand matrix exists in memory: a lane builds its
// FP64 operand for the four variants of an instruction from the 2-bit code it holds and the variant's table of four
// doubles (z of hom-ref, het, hom-alt, and 0 for a missing call), which sits in LDS.
//
// Shape: a workgroup of eight waves owns 128 x 128 pairs and walks the used variants 64 at a time, in list order.
// Wave (wr, wc) of the 4 x 2 grid owns row blocks 2 wr .. 2 wr + 1 and column blocks 4 wc .. 4 wc + 3: 2 x 4 tiles of
// 16 x 16 pairs, so the six operand values a lane looks up per four variants feed eight matrix instructions.
// The operand is the sample-major 2-bit matrix of the used variants, where 64 variants of a sample are 16 contiguous
// bytes.  Lane l of a 16-sample block serves sample l & 15 and k index kq = l >> 4 of every instruction: it loads the
// sample's 16 bytes of the K-step (the four lanes of a sample load the same bytes), and for the instruction over the
// variants 4 s .. 4 s + 3 its code is bits 2 kq .. 2 kq + 1 of byte s.  The lookup is one ds_read_b64 at
// tab + ((4 s + kq) * 4 + code) * 8: the four variants of an instruction cover all 32 banks once and lanes with the
// same code read the same address, so there is no bank conflict.  For the int8 product the lane's 16 variants are
// word kq of the same 16 bytes, expanded to the "called" plane as king.hip does.
// The 64 x 4 table entries of a K-step are staged in LDS once per workgroup, double buffered: one barrier per
// K-step (128 FP64 matrix instructions per wave).
//
// Order of the sum: one workgroup owns a pair's whole sum, and every pair's accumulator sees the K-steps in list
// order and the instruction's own order inside a step, wherever the pair sits in the tile or the rectangle.  A
// product z_i z_j does not depend on which factor is the A operand, so rel_ij and rel_ji are the same bits.
//
// The C/D maps differ: FP64 has row = (lane >> 4) + 4 reg, int8 has row = 4 (lane >> 4) + reg (col = lane & 15 in
// both).  The int8 A operand is therefore fed with its rows permuted (row 4 a + g carries sample a + 4 g, one
// cross-lane read per block and K-step), so that both accumulators of a lane belong to the same pairs.
// Padding: the codes at and past n_used, and every code of a tile row past the last sample, are forced to 3: z = 0
// and not called.  The table array is zero padded to whole K-steps, so the staging reads no further.
#include "device_utils.hpp"
#include "grm.hpp"

namespace pgh {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef double v4d __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 512;
constexpr uint32_t kTabDoubles = kGrmKStep * 4u; // one K-step's tables

struct GrmArgs {
	GrmOperand op;
	uint32_t i_begin, i_end, j_begin, j_end;
	GrmOutput out;
	int meanimpute;
};

// 16 codes (one 4-byte word) -> 16 int8 of the "called" plane
__device__ __forceinline__ v4i ExpandCalled(uint32_t w) {
	v4i M;
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const uint32_t b = (w >> (8 * q)) & 0xffu;
		const uint32_t v = b | (b << 12);
		const uint32_t c = (v | (v << 6)) & 0x03030303u; // one code per byte
		M[q] = static_cast<int>(__builtin_amdgcn_perm(0x00010101u, 0x00010101u, c));
	}
	return M;
}

// the codes at and past n become 3; first = variant of the word's lowest code
__device__ __forceinline__ uint32_t MaskTail(uint32_t w, uint32_t first, uint32_t n) {
	if (first >= n) {
		return 0xffffffffu;
	}
	const uint32_t left = n - first;
	return left >= 16u ? w : (w | (0xffffffffu << (2u * left)));
}

struct Row {
	const uint8_t *p;  // always readable: a tile row past the last sample points at the first row
	uint32_t fill;     // all ones for such a row
};

__device__ __forceinline__ Row MakeRow(const uint8_t *xt, uint32_t raw0, uint64_t pitch, const uint32_t *sel, uint32_t s,
                                       uint32_t end) {
	Row r {xt, 0xffffffffu};
	if (s < end) {
		const uint32_t raw = sel ? sel[s] : s;
		r.p = xt + static_cast<uint64_t>(raw - raw0) * pitch;
		r.fill = 0;
	}
	return r;
}

__device__ __forceinline__ uint4 LoadStep(const Row &r, uint32_t ks) {
	uint4 w = *reinterpret_cast<const uint4 *>(r.p + 16ull * ks);
	w.x |= r.fill;
	w.y |= r.fill;
	w.z |= r.fill;
	w.w |= r.fill;
	return w;
}

__device__ __forceinline__ uint4 MaskStep(uint4 w, uint32_t ks, uint32_t n) {
	w.x = MaskTail(w.x, ks * 64u, n);
	w.y = MaskTail(w.y, ks * 64u + 16u, n);
	w.z = MaskTail(w.z, ks * 64u + 32u, n);
	w.w = MaskTail(w.w, ks * 64u + 48u, n);
	return w;
}

__device__ __forceinline__ uint32_t Word(const uint4 &w, uint32_t q) {
	return q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w;
}

// z of the lane's variant of instruction S (variants 4 S .. 4 S + 3 of the K-step): w is already shifted right by
// 2 kq, tab points at the lane's kq inside the staged tables
template <int S>
__device__ __forceinline__ double Lookup(const uint4 &w, const uint8_t *tab) {
	const uint32_t word = (S >> 2) == 0 ? w.x : (S >> 2) == 1 ? w.y : (S >> 2) == 2 ? w.z : w.w;
	constexpr int kShift = 8 * (S & 3);
	const uint32_t off = kShift >= 3 ? (word >> (kShift >= 3 ? kShift - 3 : 0)) & 0x18u : (word << 3) & 0x18u;
	return *reinterpret_cast<const double *>(tab + S * 128 + off);
}

template <int S>
__device__ __forceinline__ void KSub(const uint4 (&wa)[2], const uint4 (&wb)[4], const uint8_t *tab, v4d (&acc)[2][4]) {
	double bv[4];
#pragma unroll
	for (int y = 0; y < 4; y++) {
		bv[y] = Lookup<S>(wb[y], tab);
	}
#pragma unroll
	for (int x = 0; x < 2; x++) {
		const double av = Lookup<S>(wa[x], tab);
#pragma unroll
		for (int y = 0; y < 4; y++) {
			acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[y], acc[x][y], 0, 0, 0);
		}
	}
}

template <bool TRI>
__global__ __launch_bounds__(kThreads) void k_grm(const GrmArgs a) {
	__shared__ __attribute__((aligned(16))) double s_tab[2][kTabDoubles];
	// triangle: the grid starts at the band's first tile column, nothing left of it is launched
	const uint32_t i0 = a.i_begin + blockIdx.y * kGrmTile;
	const uint32_t j0 = (TRI ? a.i_begin : a.j_begin) + blockIdx.x * kGrmTile;
	if (TRI && j0 < i0) {
		return; // left of the diagonal: the tile on the other side writes these pairs
	}
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const uint32_t wr = wave >> 1, wc = wave & 1u;
	const uint32_t li = lane & 15u, kq = lane >> 4;
	const uint32_t n = a.op.n_used;
	const uint32_t n_steps = (n + 63u) / 64u; // 16 bytes a step: within the padded pitch

	Row ra[2], rb[4];
#pragma unroll
	for (int x = 0; x < 2; x++) {
		ra[x] = MakeRow(a.op.xt_i, a.op.raw_i0, a.op.pitch, a.op.sel, i0 + wr * 32u + x * 16u + li, a.i_end);
	}
#pragma unroll
	for (int y = 0; y < 4; y++) {
		rb[y] = MakeRow(a.op.xt_j, a.op.raw_j0, a.op.pitch, a.op.sel, j0 + wc * 64u + y * 16u + li, a.j_end);
	}
	// the int8 A operand's row R = li carries sample (R >> 2) + 4 (R & 3) of the block
	const int a_src = static_cast<int>((kq << 4) | ((li >> 2) + 4u * (li & 3u)));

	v4d acc[2][4];
	v4i cnt[2][4];
#pragma unroll
	for (int x = 0; x < 2; x++) {
#pragma unroll
		for (int y = 0; y < 4; y++) {
			acc[x][y] = v4d {0.0, 0.0, 0.0, 0.0};
			cnt[x][y] = v4i {0, 0, 0, 0};
		}
	}

	uint4 wa[2], wb[4];
#pragma unroll
	for (int x = 0; x < 2; x++) {
		wa[x] = LoadStep(ra[x], 0);
	}
#pragma unroll
	for (int y = 0; y < 4; y++) {
		wb[y] = LoadStep(rb[y], 0);
	}
	if (t < kTabDoubles) {
		s_tab[0][t] = a.op.table[t];
	}
	__syncthreads();

	for (uint32_t ks = 0; ks < n_steps; ks++) {
		const bool more = ks + 1 < n_steps;
		uint4 na[2], nb[4];
		double ntab = 0.0;
		if (more) {
#pragma unroll
			for (int x = 0; x < 2; x++) {
				na[x] = LoadStep(ra[x], ks + 1);
			}
#pragma unroll
			for (int y = 0; y < 4; y++) {
				nb[y] = LoadStep(rb[y], ks + 1);
			}
			if (t < kTabDoubles) {
				ntab = a.op.table[static_cast<uint64_t>(ks + 1) * kTabDoubles + t];
			}
		} else {
#pragma unroll
			for (int x = 0; x < 2; x++) {
				wa[x] = MaskStep(wa[x], ks, n);
			}
#pragma unroll
			for (int y = 0; y < 4; y++) {
				wb[y] = MaskStep(wb[y], ks, n);
			}
		}

		// ---- denominator: both called, 64 variants per instruction ----
		{
			v4i mb[4];
#pragma unroll
			for (int y = 0; y < 4; y++) {
				mb[y] = ExpandCalled(Word(wb[y], kq));
			}
#pragma unroll
			for (int x = 0; x < 2; x++) {
				const uint32_t own = Word(wa[x], kq);
				const v4i ma = ExpandCalled(static_cast<uint32_t>(__shfl(static_cast<int>(own), a_src)));
#pragma unroll
				for (int y = 0; y < 4; y++) {
					cnt[x][y] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ma, mb[y], cnt[x][y], 0, 0, 0);
				}
			}
		}

		// ---- numerator: four variants per instruction, in list order ----
#pragma unroll
		for (int x = 0; x < 2; x++) {
			wa[x].x >>= 2u * kq;
			wa[x].y >>= 2u * kq;
			wa[x].z >>= 2u * kq;
			wa[x].w >>= 2u * kq;
		}
#pragma unroll
		for (int y = 0; y < 4; y++) {
			wb[y].x >>= 2u * kq;
			wb[y].y >>= 2u * kq;
			wb[y].z >>= 2u * kq;
			wb[y].w >>= 2u * kq;
		}
		const uint8_t *tab = reinterpret_cast<const uint8_t *>(&s_tab[ks & 1u][kq * 4u]);
		KSub<0>(wa, wb, tab, acc);
		KSub<1>(wa, wb, tab, acc);
		KSub<2>(wa, wb, tab, acc);
		KSub<3>(wa, wb, tab, acc);
		KSub<4>(wa, wb, tab, acc);
		KSub<5>(wa, wb, tab, acc);
		KSub<6>(wa, wb, tab, acc);
		KSub<7>(wa, wb, tab, acc);
		KSub<8>(wa, wb, tab, acc);
		KSub<9>(wa, wb, tab, acc);
		KSub<10>(wa, wb, tab, acc);
		KSub<11>(wa, wb, tab, acc);
		KSub<12>(wa, wb, tab, acc);
		KSub<13>(wa, wb, tab, acc);
		KSub<14>(wa, wb, tab, acc);
		KSub<15>(wa, wb, tab, acc);

		if (more) {
#pragma unroll
			for (int x = 0; x < 2; x++) {
				wa[x] = na[x];
			}
#pragma unroll
			for (int y = 0; y < 4; y++) {
				wb[y] = nb[y];
			}
			if (t < kTabDoubles) {
				s_tab[(ks + 1u) & 1u][t] = ntab;
			}
		}
		__syncthreads();
	}

	// ---- epilogue: lane holds column li, rows kq + 4 reg of each 16 x 16 block, in both accumulators ----
	const double all = static_cast<double>(n);
	const bool mirror = TRI && j0 > i0;
#pragma unroll
	for (int x = 0; x < 2; x++) {
#pragma unroll
		for (int y = 0; y < 4; y++) {
			const uint32_t j = j0 + wc * 64u + y * 16u + li;
#pragma unroll
			for (int reg = 0; reg < 4; reg++) {
				const uint32_t i = i0 + wr * 32u + x * 16u + kq + 4u * reg;
				if (i >= a.i_end || j >= a.j_end) {
					continue;
				}
				const uint32_t nobs = static_cast<uint32_t>(cnt[x][y][reg]);
				const double div = a.meanimpute ? all : static_cast<double>(nobs);
				const double rel = div == 0.0 ? __builtin_nan("") : acc[x][y][reg] / div;
				const uint64_t at = static_cast<uint64_t>(i - a.i_begin) * a.out.ld + (j - a.j_begin);
				a.out.rel[at] = rel;
				if (a.out.nobs) {
					a.out.nobs[at] = nobs;
				}
				if (mirror) {
					if (j < a.i_end) {
						const uint64_t m = static_cast<uint64_t>(j - a.i_begin) * a.out.ld + (i - a.j_begin);
						a.out.rel[m] = rel;
						if (a.out.nobs) {
							a.out.nobs[m] = nobs;
						}
					} else {
						const uint64_t m = static_cast<uint64_t>(j - a.i_end) * a.out.ld_m + (i - a.i_begin);
						a.out.rel_m[m] = rel;
						if (a.out.nobs_m) {
							a.out.nobs_m[m] = nobs;
						}
					}
				}
			}
		}
	}
}

} // namespace

hipError_t LaunchGrm(const GrmOperand &op, uint32_t i_begin, uint32_t i_end, uint32_t j_begin, uint32_t j_end,
                     bool triangle, bool meanimpute, const GrmOutput &out, hipStream_t stream) {
	if (i_begin >= i_end || j_begin >= j_end || op.n_used == 0) {
		return hipErrorInvalidValue;
	}
	if (triangle && (i_begin < j_begin || (i_begin - j_begin) % kGrmTile != 0 || i_end > j_end)) {
		return hipErrorInvalidValue;
	}
	const uint32_t col_begin = triangle ? i_begin : j_begin;
	const dim3 grid((j_end - col_begin + kGrmTile - 1) / kGrmTile, (i_end - i_begin + kGrmTile - 1) / kGrmTile);
	if (grid.y > 65535u) {
		return hipErrorInvalidValue;
	}
	GrmArgs a {};
	a.op = op;
	a.i_begin = i_begin;
	a.i_end = i_end;
	a.j_begin = j_begin;
	a.j_end = j_end;
	a.out = out;
	a.meanimpute = meanimpute ? 1 : 0;
	if (triangle) {
		hipLaunchKernelGGL(k_grm<true>, grid, dim3(kThreads), 0, stream, a);
	} else {
		hipLaunchKernelGGL(k_grm<false>, grid, dim3(kThreads), 0, stream, a);
	}
	return hipGetLastError();
}

} // namespace pgh
