// king.hip -- KING-robust pair counts on the int8 matrix cores (pgh_king_counts / pgh_king_table).
//
// For two samples i and j the five counts over the variants at which both have a call are sums over variants of
// products of per-sample indicators, so a tile of sample pairs is a Gram-like product of indicator matrices.  Three
// int8 planes are expanded from every 2-bit code (0 hom-ref, 1 het, 2 hom-alt, 3 missing):
//
//   H = [het]    M = [called]    D = [hom-ref] - [hom-alt]  in {-1, 0, 1}
//
// and five v_mfma_i32_16x16x64_i8 products per 16 x 16 block of pairs and 64 variants give everything:
//
//   HH = H_i.H_j = HETHET                 HM = H_i.M_j = HETHET + HET1HOM2       MH = M_i.H_j = HETHET + HET2HOM1
//   MM = M_i.M_j = NSNP                   DD = D_i.D_j = (both hom, same) - (both hom, opposite)
//   Hom.Hom = MM - HM - MH + HH  (Hom = M - H)        IBS0 = (Hom.Hom - DD) / 2
//
// Every term of every product is 0 or +-1, so an int32 accumulator never exceeds the number of variants in magnitude:
// with n_var <= 2^31 - 1 nothing wraps and every count is the true count.  The sum over a K-step of 64 variants does
// not depend on the order of its terms, and both operands of a product are expanded by the same code, so the
// instruction's k order inside a lane's 16 bytes needs no care; only the C/D map (col = lane & 15,
// row = (lane >> 4) * 4 + reg) is relied on.
//
// Shape: a workgroup of eight waves owns 128 x 128 pairs and walks all variants 64 at a time.  The operand is the
// sample-major 2-bit matrix (k_transpose_2bit), where 64 variants of one sample are 16 contiguous bytes: each of the
// 512 threads loads one 4-byte word (16 variants) of a row sample and one of a column sample, expands both to the
// three planes (a shift-or spread to one code per byte, then one byte permute per plane and four codes) and parks
// them in LDS in MFMA operand order (lane l of a 16-row block reads 16 bytes at l * 16: no bank conflicts).  Wave
// (wr, wc) of the 4 x 2 grid multiplies row blocks 2 wr .. 2 wr + 1 by column blocks 4 wc .. 4 wc + 3: 40 matrix
// instructions per K-step into 2 x 4 x 5 accumulator tiles (160 registers).  Two LDS buffers, one barrier per K-step:
// step k + 1 is loaded before, and expanded after, step k's products.
// Padding: a row of the transposed matrix is zero padded and code 0 is hom-ref, so the codes past n_var, and every
// code of a tile row past the last sample, are forced to 3 (not called) before the expansion.
#include "device_utils.hpp"
#include "king.hpp"
#include "king_math.hpp"

namespace pgh {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 512;
constexpr uint32_t kBlocksPerSide = kKingTile / 16;                       // 16-row MFMA blocks of one operand side
constexpr uint32_t kPlaneBytes = kBlocksPerSide * 64u * 16u;              // one plane of one side, one K-step
constexpr uint32_t kBufBytes = 2u * 3u * kPlaneBytes;                     // both sides, three planes
constexpr uint32_t kLdsBytes = 2u * kBufBytes;                            // double buffered: 96 KiB

struct KingArgs {
	const uint8_t *xt;
	uint64_t pitch;
	const uint32_t *sel;
	uint32_t n_var;
	uint32_t i_begin, i_end, j_begin, j_end; // output-sample rectangle (table: [0, n) x [0, n))
	uint32_t tile_row0;                      // table: first tile row of this launch
	// counts
	uint32_t *out;
	uint64_t plane_stride; // (i_end - i_begin) * (j_end - j_begin)
	// table
	double min_kinship;
	int no_filter;
	KingPair *pairs;
	uint64_t capacity;
	unsigned long long *count;
};

// 16 codes (one 4-byte word) -> 16 int8 of each plane
__device__ __forceinline__ void Expand(uint32_t w, v4i &H, v4i &M, v4i &D) {
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const uint32_t b = (w >> (8 * q)) & 0xffu;
		const uint32_t v = b | (b << 12);
		const uint32_t c = (v | (v << 6)) & 0x03030303u; // one code per byte
		// byte lookups by code; the table sits in both sources, so selectors 0..3 find it in either
		H[q] = static_cast<int>(__builtin_amdgcn_perm(0x00000100u, 0x00000100u, c));
		M[q] = static_cast<int>(__builtin_amdgcn_perm(0x00010101u, 0x00010101u, c));
		D[q] = static_cast<int>(__builtin_amdgcn_perm(0x00ff0001u, 0x00ff0001u, c));
	}
}

// the codes at and past n_var become 3; first = variant of the word's lowest code
__device__ __forceinline__ uint32_t MaskTail(uint32_t w, uint32_t first, uint32_t n_var) {
	if (first >= n_var) {
		return 0xffffffffu;
	}
	const uint32_t left = n_var - first;
	return left >= 16u ? w : (w | (0xffffffffu << (2u * left)));
}

template <bool TABLE>
__global__ __launch_bounds__(kThreads) void k_king(const KingArgs a) {
	extern __shared__ __attribute__((aligned(16))) uint8_t s_ops[];
	const uint32_t ti = blockIdx.y + a.tile_row0, tj = blockIdx.x;
	if (TABLE && tj < ti) {
		return; // one triangle: the pairs i < j
	}
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const uint32_t wr = wave >> 1, wc = wave & 1u;
	const uint32_t i0 = a.i_begin + ti * kKingTile, j0 = a.j_begin + tj * kKingTile;

	// loader role: word g (16 variants) of the K-step, of tile row r on both sides
	const uint32_t r = t >> 2, g = t & 3u;
	const uint8_t *pa = nullptr, *pb = nullptr;
	if (i0 + r < a.i_end) {
		const uint32_t raw = a.sel ? a.sel[i0 + r] : i0 + r;
		pa = a.xt + static_cast<uint64_t>(raw) * a.pitch + 4u * g;
	}
	if (j0 + r < a.j_end) {
		const uint32_t raw = a.sel ? a.sel[j0 + r] : j0 + r;
		pb = a.xt + static_cast<uint64_t>(raw) * a.pitch + 4u * g;
	}
	const uint32_t slot = ((r >> 4) * 64u + g * 16u + (r & 15u)) * 16u; // block, then operand lane
	const uint32_t n_steps = (a.n_var + 63u) / 64u;                     // 16 bytes a step: within the padded pitch

	auto load = [&](const uint8_t *p, uint32_t ks) -> uint32_t {
		const uint32_t w = p ? *reinterpret_cast<const uint32_t *>(p + 16ull * ks) : 0xffffffffu;
		return MaskTail(w, ks * 64u + g * 16u, a.n_var);
	};
	auto park = [&](uint32_t buf, uint32_t wa, uint32_t wb) {
		uint8_t *base = s_ops + buf * kBufBytes + slot;
		v4i H, M, D;
		Expand(wa, H, M, D);
		*reinterpret_cast<v4i *>(base) = H;
		*reinterpret_cast<v4i *>(base + kPlaneBytes) = M;
		*reinterpret_cast<v4i *>(base + 2u * kPlaneBytes) = D;
		Expand(wb, H, M, D);
		*reinterpret_cast<v4i *>(base + 3u * kPlaneBytes) = H;
		*reinterpret_cast<v4i *>(base + 4u * kPlaneBytes) = M;
		*reinterpret_cast<v4i *>(base + 5u * kPlaneBytes) = D;
	};

	v4i acc[2][4][5];
#pragma unroll
	for (int x = 0; x < 2; x++) {
#pragma unroll
		for (int y = 0; y < 4; y++) {
#pragma unroll
			for (int p = 0; p < 5; p++) {
				acc[x][y][p] = v4i {0, 0, 0, 0};
			}
		}
	}

	park(0, load(pa, 0), load(pb, 0));
	__syncthreads();
	for (uint32_t ks = 0; ks < n_steps; ks++) {
		const bool more = ks + 1 < n_steps;
		uint32_t na = 0, nb = 0;
		if (more) {
			na = load(pa, ks + 1);
			nb = load(pb, ks + 1);
		}
		const uint8_t *buf = s_ops + (ks & 1u) * kBufBytes + lane * 16u;
		v4i bH[4], bM[4], bD[4];
#pragma unroll
		for (int y = 0; y < 4; y++) {
			const uint8_t *p = buf + 3u * kPlaneBytes + (wc * 4u + y) * 1024u;
			bH[y] = *reinterpret_cast<const v4i *>(p);
			bM[y] = *reinterpret_cast<const v4i *>(p + kPlaneBytes);
			bD[y] = *reinterpret_cast<const v4i *>(p + 2u * kPlaneBytes);
		}
#pragma unroll
		for (int x = 0; x < 2; x++) {
			const uint8_t *p = buf + (wr * 2u + x) * 1024u;
			const v4i aH = *reinterpret_cast<const v4i *>(p);
			const v4i aM = *reinterpret_cast<const v4i *>(p + kPlaneBytes);
			const v4i aD = *reinterpret_cast<const v4i *>(p + 2u * kPlaneBytes);
#pragma unroll
			for (int y = 0; y < 4; y++) {
				acc[x][y][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aH, bH[y], acc[x][y][0], 0, 0, 0);
				acc[x][y][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aH, bM[y], acc[x][y][1], 0, 0, 0);
				acc[x][y][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aM, bH[y], acc[x][y][2], 0, 0, 0);
				acc[x][y][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aM, bM[y], acc[x][y][3], 0, 0, 0);
				acc[x][y][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aD, bD[y], acc[x][y][4], 0, 0, 0);
			}
		}
		if (more) {
			park((ks + 1u) & 1u, na, nb);
		}
		__syncthreads();
	}

	// ---- epilogue: lane holds column (lane & 15), rows 4 (lane >> 4) + reg of each 16 x 16 block ----
	const uint32_t nj = a.j_end - a.j_begin;
#pragma unroll
	for (int x = 0; x < 2; x++) {
#pragma unroll
		for (int y = 0; y < 4; y++) {
			const uint32_t j = j0 + wc * 64u + y * 16u + (lane & 15u);
#pragma unroll
			for (int reg = 0; reg < 4; reg++) {
				const uint32_t i = i0 + wr * 32u + x * 16u + (lane >> 4) * 4u + reg;
				const int hh = acc[x][y][0][reg], hm = acc[x][y][1][reg], mh = acc[x][y][2][reg];
				const int mm = acc[x][y][3][reg], dd = acc[x][y][4][reg];
				const uint32_t nsnp = static_cast<uint32_t>(mm), hethet = static_cast<uint32_t>(hh);
				const uint32_t h1 = static_cast<uint32_t>(hm - hh), h2 = static_cast<uint32_t>(mh - hh);
				const uint32_t ibs0 = static_cast<uint32_t>((mm - hm - mh + hh) - dd) >> 1;
				if (!TABLE) {
					if (i < a.i_end && j < a.j_end) {
						uint32_t *o = a.out + static_cast<uint64_t>(i - a.i_begin) * nj + (j - a.j_begin);
						o[0] = nsnp;
						o[a.plane_stride] = hethet;
						o[2 * a.plane_stride] = ibs0;
						o[3 * a.plane_stride] = h1;
						o[4 * a.plane_stride] = h2;
					}
				} else {
					const double kin = KingKinship(hethet, ibs0, h1, h2);
					const bool pass = i < j && j < a.j_end && (a.no_filter || kin >= a.min_kinship);
					// one counter add per wave; the slots inside it by lane order (the host sorts by (i, j) anyway)
					const unsigned long long votes = __ballot(pass);
					if (votes) {
						unsigned long long base = 0;
						if (lane == 0) {
							base = atomicAdd(a.count, static_cast<unsigned long long>(__popcll(votes)));
						}
						base = __shfl(base, 0);
						const unsigned long long at = base + __popcll(votes & ((1ull << lane) - 1ull));
						if (pass && at < a.capacity) {
							KingPair rec;
							rec.i = i;
							rec.j = j;
							rec.nsnp = nsnp;
							rec.hethet = hethet;
							rec.ibs0 = ibs0;
							rec.het1hom2 = h1;
							rec.het2hom1 = h2;
							rec.pad = 0;
							rec.kinship = kin;
							a.pairs[at] = rec;
						}
					}
				}
			}
		}
	}
}

template <bool TABLE>
hipError_t Launch(const KingArgs &a, dim3 grid, hipStream_t stream) {
	if (grid.x == 0 || grid.y == 0) {
		return hipSuccess;
	}
	if (grid.y > 65535u) {
		return hipErrorInvalidValue;
	}
	hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_king<TABLE>),
	                                   hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBytes));
	if (e != hipSuccess) {
		return e;
	}
	hipLaunchKernelGGL(k_king<TABLE>, grid, dim3(kThreads), kLdsBytes, stream, a);
	return hipGetLastError();
}

} // namespace

hipError_t LaunchKingCounts(const KingOperand &op, uint32_t i_begin, uint32_t i_end, uint32_t j_begin, uint32_t j_end,
                            uint32_t *out, hipStream_t stream) {
	if (i_begin >= i_end || j_begin >= j_end || op.n_var == 0) {
		return hipErrorInvalidValue;
	}
	KingArgs a {};
	a.xt = op.xt;
	a.pitch = op.pitch;
	a.sel = op.sel;
	a.n_var = op.n_var;
	a.i_begin = i_begin;
	a.i_end = i_end;
	a.j_begin = j_begin;
	a.j_end = j_end;
	a.out = out;
	a.plane_stride = static_cast<uint64_t>(i_end - i_begin) * (j_end - j_begin);
	return Launch<false>(a, dim3((j_end - j_begin + kKingTile - 1) / kKingTile, (i_end - i_begin + kKingTile - 1) / kKingTile),
	                     stream);
}

hipError_t LaunchKingTable(const KingOperand &op, uint32_t n_samples, uint32_t tile_row_begin, uint32_t tile_row_end,
                           double min_kinship, bool no_filter, KingPair *out, uint64_t capacity,
                           unsigned long long *count, hipStream_t stream) {
	const uint32_t tiles = (n_samples + kKingTile - 1) / kKingTile;
	if (tile_row_begin > tile_row_end || tile_row_end > tiles || op.n_var == 0) {
		return hipErrorInvalidValue;
	}
	KingArgs a {};
	a.xt = op.xt;
	a.pitch = op.pitch;
	a.sel = op.sel;
	a.n_var = op.n_var;
	a.i_end = n_samples;
	a.j_end = n_samples;
	a.tile_row0 = tile_row_begin;
	a.min_kinship = min_kinship;
	a.no_filter = no_filter ? 1 : 0;
	a.pairs = out;
	a.capacity = capacity;
	a.count = count;
	return Launch<true>(a, dim3(tiles, tile_row_end - tile_row_begin), stream);
}

} // namespace pgh
