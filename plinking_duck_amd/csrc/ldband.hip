// ldband.hip -- the six r2 sums of variant pairs on the int8 matrix cores (pgh_ld_window_sums / pgh_ld_prune /
// pgh_ld_scores).
//
// For two variants a and b the sums over the samples at which both are called are sums over samples of products of
// per-variant planes, so a tile of variant pairs is a Gram-like product of plane matrices.  Three int8 planes are
// expanded from every 2-bit code (0 hom-ref, 1 het, 2 hom-alt, 3 missing):
//
//   C = [called] 1,1,1,0      G = genotype, missing as 0: 0,1,2,0      Q = G^2: 0,1,4,0
//
// and six v_mfma_i32_16x16x64_i8 products per 16 x 16 block of pairs and 64 samples give pgh_ld_pairs' six numbers:
//
//   n = C_a.C_b    sum_a = G_a.C_b    sum_b = C_a.G_b    sum_ab = G_a.G_b    sum_a2 = Q_a.C_b    sum_b2 = C_a.Q_b
//
// Every term is at most 4, so with at most 2^29 - 1 samples an int32 accumulator stays below 2^31: nothing wraps and
// every sum is the true sum.  A K-step's sum does not depend on the order of its 64 terms and both operands are
// expanded by the same code, so the instruction's k order inside a lane's 16 bytes needs no care; only the C/D map
// (col = lane & 15, row = (lane >> 4) * 4 + reg) is relied on.
//
// Shape: a workgroup of eight waves owns kLdTileA x kLdTileB = 96 anchors x 128 partners and walks all samples 64 at
// a time.  The operand is the resident variant-major 2-bit matrix as it lies in HBM: 64 samples of one variant are 16
// contiguous bytes of its row, so nothing is transposed.  Each of the 512 threads loads one 4-byte word (16 samples)
// of a partner row and (the first 384) one of an anchor row, forces the samples the subset leaves out and the padding
// past the last sample to code 3, expands to the three planes (a shift-or spread to one code per byte, then one byte
// permute per plane and four codes) and parks them in LDS in MFMA operand order (lane l of a 16-row block reads 16
// bytes at l * 16: no bank conflicts).  Wave (wr, wc) of the 2 x 4 grid multiplies anchor blocks 3 wr .. 3 wr + 2 by
// partner blocks 2 wc, 2 wc + 1: 36 matrix instructions per K-step into 3 x 2 x 6 accumulator tiles (144 registers;
// a 128 x 128 tile would need 192 of the 256 a wave has at two waves per SIMD).  Two LDS buffers, one barrier per
// K-step: step k + 1 is loaded before, and expanded after, step k's products.
// The tiles of a launch come from a list, so only the tiles that meet the band k < u < win_end[k] are run.
//
// Three epilogues on the one main loop (template MODE): the six sums of a rectangle (kSums), one "exceeds" bit per
// band pair (kBits), and the per-row and per-column sums of the band pairs' r2 terms (kScores).  The last adds in a
// fixed order, a function of the position in the tile alone -- rows: a lane's two partner blocks, a butterfly over the
// 16 lanes of its row group (xor 1, 2, 4, 8), then the four wc waves in wc order through LDS; columns: a lane's 12
// rows (block, then register), xor 16, xor 32, then the two wr waves -- so a tile's 224 sums are the same bits on
// every run.  s_ops is free for this after the loop's last barrier.
#include "device_utils.hpp"
#include "ld_math.hpp"
#include "ldband.hpp"

namespace pgh {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 512;
constexpr uint32_t kBlocksA = kLdTileA / 16, kBlocksB = kLdTileB / 16;
constexpr uint32_t kPlaneA = kBlocksA * 64u * 16u;            // one plane of the anchor side, one K-step
constexpr uint32_t kPlaneB = kBlocksB * 64u * 16u;            // one plane of the partner side
constexpr uint32_t kSideB = 3u * kPlaneA;                     // the partner planes follow the anchor planes
constexpr uint32_t kBufBytes = 3u * (kPlaneA + kPlaneB);      // both sides, three planes: 42 KiB
constexpr uint32_t kLdsBytes = 2u * kBufBytes;                // double buffered: 84 KiB
constexpr uint32_t kWaveA = 3, kWaveB = 2;                    // 16-row blocks of a wave's tile
static_assert(2u * kWaveA == kBlocksA && 4u * kWaveB == kBlocksB, "2 x 4 waves cover the tile");
static_assert(kWaveB * 16u == 32u, "one bit word per wave and anchor row");
static_assert(kLdTileScoreSlots <= kThreads, "one thread per slot writes a tile's score partials");

enum LdMode : int { kSums = 0, kBits = 1, kScores = 2 };

struct LdBandArgs {
	const uint8_t *rows;
	uint64_t pitch;
	const uint32_t *list;
	const uint8_t *mask2;
	const LdTile *tiles;
	uint32_t sample_ct, n_var;
	uint32_t a_begin, a_end, b_begin, b_end; // the pairs that are wanted (bits: [0, n_var) x [0, n_var))
	// sums
	uint32_t *out;
	uint64_t plane_stride;
	// bits
	const uint32_t *win_end;
	double threshold;
	uint32_t *bits;
	// scores (win_end as for bits)
	double *part;
	uint32_t *cnt;
	uint32_t flags;
};

// 16 codes (one 4-byte word) -> 16 int8 of each plane
__device__ __forceinline__ void Expand(uint32_t w, v4i &C, v4i &G, v4i &Q) {
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const uint32_t b = (w >> (8 * q)) & 0xffu;
		const uint32_t v = b | (b << 12);
		const uint32_t c = (v | (v << 6)) & 0x03030303u; // one code per byte
		// byte lookups by code; the table sits in both sources, so selectors 0..3 find it in either
		C[q] = static_cast<int>(__builtin_amdgcn_perm(0x00010101u, 0x00010101u, c));
		G[q] = static_cast<int>(__builtin_amdgcn_perm(0x00020100u, 0x00020100u, c));
		Q[q] = static_cast<int>(__builtin_amdgcn_perm(0x00040100u, 0x00040100u, c));
	}
}

// the codes of the samples at and past sample_ct become 3; first = sample of the word's lowest code
__device__ __forceinline__ uint32_t MaskTail(uint32_t w, uint32_t first, uint32_t sample_ct) {
	if (first >= sample_ct) {
		return 0xffffffffu;
	}
	const uint32_t left = sample_ct - first;
	return left >= 16u ? w : (w | (0xffffffffu << (2u * left)));
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_ld_band(const LdBandArgs a) {
	constexpr bool BITS = MODE == kBits, SCORES = MODE == kScores;
	extern __shared__ __attribute__((aligned(16))) uint8_t s_ops[];
	const LdTile tile = a.tiles[blockIdx.x];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const uint32_t wr = wave >> 2, wc = wave & 3u;

	// loader role: word g (16 samples) of the K-step, of tile row r on the partner side and, r < kLdTileA, the anchor side
	const uint32_t r = t >> 2, g = t & 3u;
	const uint8_t *pa = nullptr, *pb = nullptr;
	if (r < kLdTileA && tile.a0 + r < a.a_end) {
		pa = a.rows + static_cast<uint64_t>(a.list[tile.a0 + r]) * a.pitch + 4u * g;
	}
	if (tile.b0 + r < a.b_end) {
		pb = a.rows + static_cast<uint64_t>(a.list[tile.b0 + r]) * a.pitch + 4u * g;
	}
	const uint8_t *pm = a.mask2 ? a.mask2 + 4u * g : nullptr;
	const uint32_t slot = ((r >> 4) * 64u + g * 16u + (r & 15u)) * 16u; // block, then operand lane
	const uint32_t n_steps = (a.sample_ct + 63u) / 64u;                 // 16 bytes a step: within the padded pitch

	// excluded samples and the row's padding become code 3 (not called)
	auto load = [&](const uint8_t *p, uint32_t ks, uint32_t drop) -> uint32_t {
		const uint32_t w = p ? *reinterpret_cast<const uint32_t *>(p + 16ull * ks) : 0xffffffffu;
		return MaskTail(w | drop, ks * 64u + g * 16u, a.sample_ct);
	};
	auto dropped = [&](uint32_t ks) -> uint32_t {
		if (!pm) {
			return 0u;
		}
		const uint32_t m = *reinterpret_cast<const uint32_t *>(pm + 16ull * ks) & 0x55555555u;
		return ~(m | (m << 1));
	};
	auto park = [&](uint32_t buf, uint32_t wa, uint32_t wb) {
		uint8_t *base = s_ops + buf * kBufBytes + slot;
		v4i C, G, Q;
		if (r < kLdTileA) {
			Expand(wa, C, G, Q);
			*reinterpret_cast<v4i *>(base) = C;
			*reinterpret_cast<v4i *>(base + kPlaneA) = G;
			*reinterpret_cast<v4i *>(base + 2u * kPlaneA) = Q;
		}
		Expand(wb, C, G, Q);
		*reinterpret_cast<v4i *>(base + kSideB) = C;
		*reinterpret_cast<v4i *>(base + kSideB + kPlaneB) = G;
		*reinterpret_cast<v4i *>(base + kSideB + 2u * kPlaneB) = Q;
	};

	v4i acc[kWaveA][kWaveB][6];
#pragma unroll
	for (uint32_t x = 0; x < kWaveA; x++) {
#pragma unroll
		for (uint32_t y = 0; y < kWaveB; y++) {
#pragma unroll
			for (int p = 0; p < 6; p++) {
				acc[x][y][p] = v4i {0, 0, 0, 0};
			}
		}
	}

	{
		const uint32_t drop = dropped(0);
		park(0, load(pa, 0, drop), load(pb, 0, drop));
	}
	__syncthreads();
	for (uint32_t ks = 0; ks < n_steps; ks++) {
		const bool more = ks + 1 < n_steps;
		uint32_t na = 0, nb = 0;
		if (more) {
			const uint32_t drop = dropped(ks + 1);
			na = load(pa, ks + 1, drop);
			nb = load(pb, ks + 1, drop);
		}
		const uint8_t *buf = s_ops + (ks & 1u) * kBufBytes + lane * 16u;
		v4i bC[kWaveB], bG[kWaveB], bQ[kWaveB];
#pragma unroll
		for (uint32_t y = 0; y < kWaveB; y++) {
			const uint8_t *p = buf + kSideB + (wc * kWaveB + y) * 1024u;
			bC[y] = *reinterpret_cast<const v4i *>(p);
			bG[y] = *reinterpret_cast<const v4i *>(p + kPlaneB);
			bQ[y] = *reinterpret_cast<const v4i *>(p + 2u * kPlaneB);
		}
#pragma unroll
		for (uint32_t x = 0; x < kWaveA; x++) {
			const uint8_t *p = buf + (wr * kWaveA + x) * 1024u;
			const v4i aC = *reinterpret_cast<const v4i *>(p);
			const v4i aG = *reinterpret_cast<const v4i *>(p + kPlaneA);
			const v4i aQ = *reinterpret_cast<const v4i *>(p + 2u * kPlaneA);
#pragma unroll
			for (uint32_t y = 0; y < kWaveB; y++) {
				acc[x][y][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aC, bC[y], acc[x][y][0], 0, 0, 0);
				acc[x][y][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aG, bC[y], acc[x][y][1], 0, 0, 0);
				acc[x][y][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aC, bG[y], acc[x][y][2], 0, 0, 0);
				acc[x][y][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aG, bG[y], acc[x][y][3], 0, 0, 0);
				acc[x][y][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aQ, bC[y], acc[x][y][4], 0, 0, 0);
				acc[x][y][5] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aC, bQ[y], acc[x][y][5], 0, 0, 0);
			}
		}
		if (more) {
			park((ks + 1u) & 1u, na, nb);
		}
		__syncthreads();
	}

	// ---- epilogue: lane holds column (lane & 15), rows 4 (lane >> 4) + reg of each 16 x 16 block ----
	const uint32_t nb_out = a.b_end - a.b_begin;
	// scores: the waves' row and column partials meet in LDS (the operands are done with: the loop ends on a barrier)
	double *s_row = reinterpret_cast<double *>(s_ops);                          // [4 wc][kLdTileA]
	double *s_col = s_row + 4u * kLdTileA;                                      // [2 wr][kLdTileB]
	uint32_t *s_rown = reinterpret_cast<uint32_t *>(s_col + 2u * kLdTileB);     // [4 wc][kLdTileA]
	uint32_t *s_coln = s_rown + 4u * kLdTileA;                                  // [2 wr][kLdTileB]
	double col[kWaveB];
	uint32_t coln[kWaveB];
#pragma unroll
	for (uint32_t y = 0; y < kWaveB; y++) {
		col[y] = 0.0;
		coln[y] = 0u;
	}
#pragma unroll
	for (uint32_t x = 0; x < kWaveA; x++) {
#pragma unroll
		for (int reg = 0; reg < 4; reg++) {
			const uint32_t row = wr * (kWaveA * 16u) + x * 16u + (lane >> 4) * 4u + reg; // of the tile
			const uint32_t k = tile.a0 + row;
			uint32_t k_end = 0; // partners of k: (k, k_end)
			if ((BITS || SCORES) && k < a.n_var) {
				k_end = a.win_end[k];
			}
			unsigned long long votes[kWaveB];
			double terms[kWaveB];
#pragma unroll
			for (uint32_t y = 0; y < kWaveB; y++) {
				const uint32_t u = tile.b0 + wc * (kWaveB * 16u) + y * 16u + (lane & 15u);
				const uint32_t n = static_cast<uint32_t>(acc[x][y][0][reg]), sa = static_cast<uint32_t>(acc[x][y][1][reg]);
				const uint32_t sb = static_cast<uint32_t>(acc[x][y][2][reg]), sab = static_cast<uint32_t>(acc[x][y][3][reg]);
				const uint32_t sa2 = static_cast<uint32_t>(acc[x][y][4][reg]), sb2 = static_cast<uint32_t>(acc[x][y][5][reg]);
				if (MODE == kSums) {
					if (k >= a.a_begin && k < a.a_end && u >= a.b_begin && u < a.b_end) {
						uint32_t *o = a.out + static_cast<uint64_t>(k - a.a_begin) * nb_out + (u - a.b_begin);
						o[0] = n;
						o[a.plane_stride] = sa;
						o[2 * a.plane_stride] = sb;
						o[3 * a.plane_stride] = sab;
						o[4 * a.plane_stride] = sa2;
						o[5 * a.plane_stride] = sb2;
					}
				} else if (BITS) {
					const bool pass = u > k && u < k_end && LdExceeds(n, sa, sb, sab, sa2, sb2, a.threshold);
					votes[y] = __ballot(pass);
				} else {
					double term = 0.0;
					const bool counts = u > k && u < k_end && LdR2Term(n, sa, sb, sab, sa2, sb2, a.flags, &term);
					terms[y] = counts ? term : 0.0;
					votes[y] = __ballot(counts);
					col[y] += terms[y];
					coln[y] += counts ? 1u : 0u;
				}
			}
			if (BITS && lane < 4u) {
				// lane q writes the word of tile row 4 q + reg (of this block): 16 columns from each of the two votes
				const uint32_t lo = static_cast<uint32_t>(votes[0] >> (16u * lane)) & 0xffffu;
				const uint32_t hi = static_cast<uint32_t>(votes[1] >> (16u * lane)) & 0xffffu;
				const uint32_t my_row = wr * (kWaveA * 16u) + x * 16u + lane * 4u + reg;
				a.bits[(static_cast<uint64_t>(blockIdx.x) * kLdTileA + my_row) * (kLdTileB / 32u) + wc] = lo | (hi << 16);
			}
			if (SCORES) {
				// this wave's 32 partners of the lane's row: the two blocks, then the 16 lanes of the row group
				double rs = terms[0] + terms[1];
#pragma unroll
				for (int m = 1; m < 16; m <<= 1) {
					rs += __shfl_xor(rs, m);
				}
				if ((lane & 15u) == 0u) {
					const uint32_t sh = 16u * (lane >> 4);
					s_row[wc * kLdTileA + row] = rs;
					s_rown[wc * kLdTileA + row] = __popc(static_cast<uint32_t>(votes[0] >> sh) & 0xffffu) +
					                              __popc(static_cast<uint32_t>(votes[1] >> sh) & 0xffffu);
				}
			}
		}
	}
	if (SCORES) {
		// this wave's 48 anchors of the lane's columns: the 12 of the lane are in col[], then the four row groups
#pragma unroll
		for (uint32_t y = 0; y < kWaveB; y++) {
			double cs = col[y];
			uint32_t cn = coln[y];
			cs += __shfl_xor(cs, 16);
			cn += __shfl_xor(cn, 16);
			cs += __shfl_xor(cs, 32);
			cn += __shfl_xor(cn, 32);
			if (lane < 16u) {
				const uint32_t c = wc * (kWaveB * 16u) + y * 16u + lane;
				s_col[wr * kLdTileB + c] = cs;
				s_coln[wr * kLdTileB + c] = cn;
			}
		}
		__syncthreads();
		const uint64_t slot0 = static_cast<uint64_t>(blockIdx.x) * kLdTileScoreSlots;
		if (t < kLdTileA) {
			double v = s_row[t];
			uint32_t c = s_rown[t];
#pragma unroll
			for (uint32_t w = 1; w < 4u; w++) {
				v += s_row[w * kLdTileA + t];
				c += s_rown[w * kLdTileA + t];
			}
			a.part[slot0 + t] = v;
			a.cnt[slot0 + t] = c;
		} else if (t < kLdTileScoreSlots) {
			const uint32_t c = t - kLdTileA;
			a.part[slot0 + t] = s_col[c] + s_col[kLdTileB + c];
			a.cnt[slot0 + t] = s_coln[c] + s_coln[kLdTileB + c];
		}
	}
}

template <int MODE>
hipError_t Launch(const LdBandArgs &a, uint32_t n_tiles, hipStream_t stream) {
	if (n_tiles == 0) {
		return hipSuccess;
	}
	hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_ld_band<MODE>),
	                                   hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBytes));
	if (e != hipSuccess) {
		return e;
	}
	hipLaunchKernelGGL(k_ld_band<MODE>, dim3(n_tiles), dim3(kThreads), kLdsBytes, stream, a);
	return hipGetLastError();
}

LdBandArgs Common(const LdBandOperand &op, const LdTile *tiles) {
	LdBandArgs a {};
	a.rows = op.view.rows;
	a.pitch = op.view.pitch;
	a.list = op.list;
	a.mask2 = op.mask2;
	a.tiles = tiles;
	a.sample_ct = op.view.sample_ct;
	a.n_var = op.n_var;
	return a;
}

} // namespace

hipError_t LaunchLdBandSums(const LdBandOperand &op, const LdTile *tiles, uint32_t n_tiles, uint32_t a_begin,
                            uint32_t a_end, uint32_t b_begin, uint32_t b_end, uint32_t *out, hipStream_t stream) {
	if (a_begin >= a_end || b_begin >= b_end || a_end > op.n_var || b_end > op.n_var ||
	    op.view.sample_ct > kLdBandMaxSamples) {
		return hipErrorInvalidValue;
	}
	LdBandArgs a = Common(op, tiles);
	a.a_begin = a_begin;
	a.a_end = a_end;
	a.b_begin = b_begin;
	a.b_end = b_end;
	a.out = out;
	a.plane_stride = static_cast<uint64_t>(a_end - a_begin) * (b_end - b_begin);
	return Launch<kSums>(a, n_tiles, stream);
}

hipError_t LaunchLdBandBits(const LdBandOperand &op, const LdTile *tiles, uint32_t n_tiles, const uint32_t *win_end,
                            double threshold, uint32_t *bits, hipStream_t stream) {
	if (op.n_var == 0 || op.view.sample_ct > kLdBandMaxSamples) {
		return hipErrorInvalidValue;
	}
	LdBandArgs a = Common(op, tiles);
	a.a_end = op.n_var;
	a.b_end = op.n_var;
	a.win_end = win_end;
	a.threshold = threshold;
	a.bits = bits;
	return Launch<kBits>(a, n_tiles, stream);
}

hipError_t LaunchLdBandScores(const LdBandOperand &op, const LdTile *tiles, uint32_t n_tiles, const uint32_t *win_end,
                              uint32_t flags, double *part, uint32_t *cnt, hipStream_t stream) {
	if (op.n_var == 0 || op.view.sample_ct > kLdBandMaxSamples) {
		return hipErrorInvalidValue;
	}
	LdBandArgs a = Common(op, tiles);
	a.a_end = op.n_var;
	a.b_end = op.n_var;
	a.win_end = win_end;
	a.flags = flags;
	a.part = part;
	a.cnt = cnt;
	return Launch<kScores>(a, n_tiles, stream);
}

} // namespace pgh
