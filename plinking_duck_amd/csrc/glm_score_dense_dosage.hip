// glm_score_dense_dosage.hip -- pgh_glm_score_multi_dosage: glm_score_dense.hip's score test for the variants of a
// dense-resident dataset that carry a dosage track (the launch wrapper is in glm.hpp).
//
// The row of (variant, phenotype) is glm_score_dense.hip's with x_i = value / 16384 where sample i has an explicit
// dosage and its call's ALT count otherwise; M = the samples of S with neither.  Three kernels stand in for that file's
// counts and contraction, and its correction kernel runs unchanged over a 2-bit row that says who is missing:
//
// Expansion (GlmScoreDosageExpandKernel).  Per listed variant, a thread per 16 samples writes
//   the u16 row: 64 ceil(N / 64) values in raw-sample order on the 2^-14 grid -- the explicit value where the presence
//     bit is set (values[val_off + rank[word] + popcount(bits below)]), else 0 / 16384 / 32768 for the calls 0 / 1 / 2,
//     0xFFFF for neither, 0 past the last sample;
//   the effective 2-bit row: the resident codes with code 3 replaced by code 0 where a dosage is present, so that its
//     code 3 is exactly M.
//
// Counts (GlmScoreDosageCountsKernel).  A wave per (variant, phenotype) sums v and v^2 of the u16 row under the
// phenotype's sample mask in 64-bit integers and counts the 0xFFFF: n = |S| - |M|, sum x = sum v * 2^-14 and
// sum x^2 = sum v^2 * 2^-28 are exact in FP64 while sum v^2 < 2^53, which sample_ct < 2^23 guarantees, and do not
// depend on the order.  For a track that restates its calls they are GlmScoreDenseCountsKernel's doubles.
//
// Contraction (GlmScoreDosageMfmaKernel).  GlmScoreDenseMfmaKernel's geometry, lane map, LDS tile of B and order of
// sums: a workgroup owns 128 variants x 64 columns, walks the samples 32 a step from sample 0, one accumulator chain per
// (variant, column) over the samples 4 j .. 4 j + 3 in ascending j; no split of the sample axis, no atomics.  Only the A
// operand differs: a step of a row is 64 bytes of the u16 row, of which lane (row, kq) loads the eight 4-byte pairs that
// hold its values (the four kq lanes of a row share the lines) and takes value 4 S + kq for instruction S:
// a = double(v) * 2^-14, 0.0 for 0xFFFF, or a * a for an x^2 column block.  Both are exact, and for the values
// 0 / 16384 / 32768 they are the 0 / 1 / 2 and 0 / 1 / 4 of the 2-bit kernel, so a track that restates its calls gives
// that kernel's sums bit for bit.
#include "dosage.hpp"
#include "glm.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

namespace pgh {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int kBlock = kTeamBlock;
constexpr uint32_t kTileV = kGlmScoreDenseTileV, kTileC = kGlmScoreDenseTileC, kStep = 32;
constexpr uint32_t kLdsLd = kTileC + 16; // doubles a row of the LDS tile
constexpr uint32_t kNone = 0xffffu;      // neither a dosage nor a call
static_assert(kTileV == 128 && kTileC == 64 && kBlock == 256, "the wave grid below is 4 waves x (32 variants, 64 columns)");

uint32_t Blocks(uint64_t n, uint32_t per) {
	return static_cast<uint32_t>((n + per - 1) / per);
}

// Workgroup (t, y): the 16-sample words 256 y .. 256 y + 255 of listed variant t, a word per thread.
// u16: nt rows of 64 words16 values; eff: nt rows of 16 words16 bytes.
__global__ void __launch_bounds__(kBlock) GlmScoreDosageExpandKernel(const uint8_t *__restrict__ rows, uint64_t pitch,
                                                                     uint32_t sample_ct, DosageView dos,
                                                                     const uint32_t *__restrict__ vlist,
                                                                     uint32_t words16, uint16_t *__restrict__ u16,
                                                                     uint32_t *__restrict__ eff) {
	const uint32_t t = blockIdx.x, wi = blockIdx.y * kBlock + threadIdx.x;
	if (wi >= 4u * words16) {
		return;
	}
	const uint32_t lv = vlist[t];
	const uint32_t r = static_cast<uint32_t>(dos.row_of[lv]); // the host lists variants with a track only
	const uint32_t c = reinterpret_cast<const uint32_t *>(rows + static_cast<uint64_t>(lv) * pitch)[wi];
	const uint32_t w = wi >> 2, shift = 16u * (wi & 3u);
	const uint64_t bits = dos.present[static_cast<uint64_t>(r) * dos.words + w];
	const uint32_t have = static_cast<uint32_t>(bits >> shift) & 0xffffu;
	const uint16_t *val = dos.values + dos.val_off[r] + dos.rank[static_cast<uint64_t>(r) * dos.words + w] +
	                      static_cast<uint32_t>(__popcll(bits & ((1ull << shift) - 1ull)));
	uint32_t out[8], e = c, at = 0;
#pragma unroll
	for (uint32_t i = 0; i < 16u; i++) {
		const uint32_t code = (c >> (2u * i)) & 3u;
		uint32_t v = code == 3u ? kNone : code << 14;
		if ((have >> i) & 1u) {
			v = val[at++];
			if (code == 3u) {
				e &= ~(3u << (2u * i));
			}
		}
		if (16u * wi + i >= sample_ct) {
			v = 0;
		}
		out[i >> 1] = (i & 1u) ? out[i >> 1] | (v << 16) : v;
	}
	uint4 *dst = reinterpret_cast<uint4 *>(u16 + (static_cast<uint64_t>(t) * words16 * 4u + wi) * 16u);
	dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
	dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
	eff[static_cast<uint64_t>(t) * words16 * 4u + wi] = e;
}

__device__ __forceinline__ void CountPair(uint32_t pair, uint32_t m2, uint64_t *sv, uint64_t *sq, uint32_t *nm) {
#pragma unroll
	for (uint32_t h = 0; h < 2u; h++) {
		const uint32_t v = (pair >> (16u * h)) & 0xffffu;
		if ((m2 >> (2u * h)) & 1u) {
			if (v == kNone) {
				*nm += 1u;
			} else {
				*sv += v;
				*sq += static_cast<uint64_t>(v) * v;
			}
		}
	}
}

// A wave per (listed variant, block phenotype): sums[p][t][0..2] = {n, sum x, sum x^2} and nmiss[p][t] = |M|.
// mask: GlmScoreDenseCountsKernel's.
__global__ void __launch_bounds__(kBlock) GlmScoreDosageCountsKernel(const uint16_t *__restrict__ u16, uint32_t nt,
                                                                     uint32_t words16,
                                                                     const uint32_t *__restrict__ mask, uint32_t pb,
                                                                     const uint32_t *__restrict__ n_y, uint32_t kp,
                                                                     double *__restrict__ sums,
                                                                     uint32_t *__restrict__ nmiss) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * kTeamWaves + (threadIdx.x >> 6);
	if (gw >= static_cast<uint64_t>(nt) * pb) {
		return;
	}
	const uint32_t t = static_cast<uint32_t>(gw / pb), p = static_cast<uint32_t>(gw % pb);
	const uint32_t n_words = 4u * words16; // 16-sample words: 32 bytes of the u16 row, one word of the mask
	const uint4 *row = reinterpret_cast<const uint4 *>(u16 + static_cast<uint64_t>(t) * n_words * 16u);
	const uint32_t *m = mask + static_cast<uint64_t>(p) * n_words;
	uint64_t sv = 0, sq = 0;
	uint32_t nm = 0;
	for (uint32_t i = lane; i < n_words; i += 64u) {
		const uint32_t mm = m[i];
		if (mm == 0u) {
			continue;
		}
		const uint4 a = row[2u * i], b = row[2u * i + 1u];
		CountPair(a.x, mm, &sv, &sq, &nm);
		CountPair(a.y, mm >> 4, &sv, &sq, &nm);
		CountPair(a.z, mm >> 8, &sv, &sq, &nm);
		CountPair(a.w, mm >> 12, &sv, &sq, &nm);
		CountPair(b.x, mm >> 16, &sv, &sq, &nm);
		CountPair(b.y, mm >> 20, &sv, &sq, &nm);
		CountPair(b.z, mm >> 24, &sv, &sq, &nm);
		CountPair(b.w, mm >> 28, &sv, &sq, &nm);
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		sv += __shfl_xor(sv, off, 64);
		sq += __shfl_xor(sq, off, 64);
	}
	nm = WaveSum(nm);
	if (lane == 0) {
		const uint64_t at = static_cast<uint64_t>(p) * nt + t;
		double *s = sums + at * (kp + 6);
		s[0] = static_cast<double>(n_y[p] - nm);
		s[1] = static_cast<double>(sv) * 0x1p-14;
		s[2] = static_cast<double>(sq) * 0x1p-28;
		nmiss[at] = nm;
	}
}

struct DosageArgs {
	const uint16_t *u16; // the expanded rows, 32 n_steps values each
	uint32_t nt;         // listed variants
	uint32_t n_steps;    // 32-sample steps: B holds 32 n_steps rows
	const double *b;
	uint32_t ld, n_xblocks, pb, k, kp;
	double *sums; // [pb][nt][kp + 6]: slots 3 (U0), 4 (A), 5 .. 5 + k (c) are written
};

// what a lane takes of a row's 32 values of step ks: per instruction S the pair of values 4 S + 2 (kq >> 1) and the next
struct StepValues {
	uint32_t d[8];
};

// row: the lane's row of the u16 block, advanced by 2 (kq >> 1) values
__device__ __forceinline__ StepValues LoadValues(const uint16_t *row, uint32_t ks) {
	const uint32_t *src = reinterpret_cast<const uint32_t *>(row + 32ull * ks);
	StepValues s;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		s.d[i] = src[2 * i];
	}
	return s;
}

// instruction S of a step: the samples 4 S .. 4 S + 3, the lane's is 4 S + kq
template <int S>
__device__ __forceinline__ void KSub(const StepValues (&w)[2], uint32_t kq, const double *tile, const bool (&sq)[4],
                                     v4d (&acc)[2][4]) {
	double bv[4];
#pragma unroll
	for (int y = 0; y < 4; y++) {
		bv[y] = tile[S * 4 * kLdsLd + y * 16];
	}
#pragma unroll
	for (int x = 0; x < 2; x++) {
		const uint32_t v = (w[x].d[S] >> (16u * (kq & 1u))) & 0xffffu;
		const double a1 = v == kNone ? 0.0 : static_cast<double>(v) * 0x1p-14, a2 = a1 * a1;
#pragma unroll
		for (int y = 0; y < 4; y++) {
			acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(sq[y] ? a2 : a1, bv[y], acc[x][y], 0, 0, 0);
		}
	}
}

__global__ void __launch_bounds__(kBlock) GlmScoreDosageMfmaKernel(const DosageArgs a) {
	__shared__ __attribute__((aligned(16))) double s_b[2][kStep * kLdsLd];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const uint32_t li = lane & 15u, kq = lane >> 4;
	const uint32_t vt0 = blockIdx.x * kTileV, cb0 = blockIdx.y * (kTileC / 16u);

	const uint16_t *ra[2];
#pragma unroll
	for (int x = 0; x < 2; x++) {
		const uint32_t v = min(vt0 + wave * 32u + x * 16u + li, a.nt - 1u);
		ra[x] = a.u16 + static_cast<uint64_t>(v) * a.n_steps * kStep + 2u * (kq >> 1);
	}
	bool sq[4];
#pragma unroll
	for (int y = 0; y < 4; y++) {
		sq[y] = cb0 + y >= a.n_xblocks;
	}
	// staging: thread t moves the eight doubles (t & 7) * 8 .. of row t >> 3 of a step's 32 x 64 tile
	const uint32_t sr = t >> 3, sc = (t & 7u) * 8u;
	const double *src = a.b + static_cast<uint64_t>(sr) * a.ld + cb0 * 16u + sc;
	const uint64_t src_step = static_cast<uint64_t>(kStep) * a.ld;
	const uint32_t dst = sr * kLdsLd + sc;

	v4d acc[2][4];
#pragma unroll
	for (int x = 0; x < 2; x++) {
#pragma unroll
		for (int y = 0; y < 4; y++) {
			acc[x][y] = v4d {0.0, 0.0, 0.0, 0.0};
		}
	}

	StepValues wa[2];
#pragma unroll
	for (int x = 0; x < 2; x++) {
		wa[x] = LoadValues(ra[x], 0);
	}
#pragma unroll
	for (int q = 0; q < 4; q++) {
		*reinterpret_cast<v2d *>(&s_b[0][dst + 2 * q]) = *reinterpret_cast<const v2d *>(src + 2 * q);
	}
	__syncthreads();

	for (uint32_t ks = 0; ks < a.n_steps; ks++) {
		const bool more = ks + 1 < a.n_steps;
		StepValues na[2];
		v2d nb[4];
		if (more) {
			const double *nsrc = src + (ks + 1ull) * src_step;
#pragma unroll
			for (int q = 0; q < 4; q++) {
				nb[q] = *reinterpret_cast<const v2d *>(nsrc + 2 * q);
			}
#pragma unroll
			for (int x = 0; x < 2; x++) {
				na[x] = LoadValues(ra[x], ks + 1);
			}
		}
		const double *tile = &s_b[ks & 1u][kq * kLdsLd + li];
		KSub<0>(wa, kq, tile, sq, acc);
		KSub<1>(wa, kq, tile, sq, acc);
		KSub<2>(wa, kq, tile, sq, acc);
		KSub<3>(wa, kq, tile, sq, acc);
		KSub<4>(wa, kq, tile, sq, acc);
		KSub<5>(wa, kq, tile, sq, acc);
		KSub<6>(wa, kq, tile, sq, acc);
		KSub<7>(wa, kq, tile, sq, acc);
		if (more) {
#pragma unroll
			for (int q = 0; q < 4; q++) {
				*reinterpret_cast<v2d *>(&s_b[(ks + 1u) & 1u][dst + 2 * q]) = nb[q];
			}
#pragma unroll
			for (int x = 0; x < 2; x++) {
				wa[x] = na[x];
			}
		}
		__syncthreads();
	}

	// ---- epilogue (GlmScoreDenseMfmaKernel's): the lane holds column li, rows kq + 4 reg of each 16 x 16 block ----
	const uint32_t q2 = a.k + 2u, ns = a.kp + 6u;
#pragma unroll
	for (int y = 0; y < 4; y++) {
		const uint32_t cb = cb0 + y;
		uint32_t p, slot;
		if (cb < a.n_xblocks) {
			const uint32_t col = cb * 16u + li;
			p = col / q2;
			const uint32_t j = col - p * q2;
			slot = j == 0u ? 3u : 4u + j; // r -> U0; w, w Zt_1 .. -> c_0, c_1 ..
		} else {
			p = (cb - a.n_xblocks) * 16u + li;
			slot = 4u; // A
		}
		if (p >= a.pb) {
			continue;
		}
#pragma unroll
		for (int x = 0; x < 2; x++) {
#pragma unroll
			for (int reg = 0; reg < 4; reg++) {
				const uint32_t v = vt0 + wave * 32u + x * 16u + kq + 4u * reg;
				if (v < a.nt) {
					a.sums[(static_cast<uint64_t>(p) * a.nt + v) * ns + slot] = acc[x][y][reg];
				}
			}
		}
	}
}

} // namespace

uint64_t GlmScoreDosageRowBytes(uint32_t sample_ct) {
	const uint64_t words16 = (static_cast<uint64_t>(sample_ct) + 63u) / 64u;
	return 128ull * words16 + 16ull * words16;
}

hipError_t LaunchGlmScoreDenseDosage(const RowView &view, const DosageView &dos, const uint32_t *vlist, uint32_t nt,
                                     const uint32_t *mask, const uint32_t *n_y, uint32_t pb, const double *b,
                                     const double *z0, const double *mz, uint32_t kp, uint32_t k, const double *hg,
                                     uint16_t *u16, uint8_t *eff, double *sums, uint32_t *nmiss, double *hgn,
                                     hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp || pb == 0 || pb > kGlmScoreDensePb) {
		return hipErrorInvalidValue;
	}
	if (nt == 0) {
		return hipSuccess;
	}
	const uint32_t words16 = (view.sample_ct + 63u) / 64u;
	if (16ull * words16 > view.pitch || dos.words != words16 || !dos.row_of) {
		return hipErrorInvalidValue; // the expansion reads whole 16-byte lanes of a resident row
	}
	const GlmScoreDenseCols c = GlmScoreDenseLayout(pb, k);
	GlmScoreDosageExpandKernel<<<dim3(nt, Blocks(4u * words16, kBlock)), kBlock, 0, stream>>>(
	    view.rows, view.pitch, view.sample_ct, dos, vlist, words16, u16, reinterpret_cast<uint32_t *>(eff));
	GlmScoreDosageCountsKernel<<<Blocks(static_cast<uint64_t>(nt) * pb, kTeamWaves), kBlock, 0, stream>>>(
	    u16, nt, words16, mask, pb, n_y, kp, sums, nmiss);
	DosageArgs a {};
	a.u16 = u16;
	a.nt = nt;
	a.n_steps = words16 * 2u;
	a.b = b;
	a.ld = c.ld;
	a.n_xblocks = c.n_xblocks;
	a.pb = pb;
	a.k = k;
	a.kp = kp;
	a.sums = sums;
	GlmScoreDosageMfmaKernel<<<dim3(Blocks(nt, kTileV), c.ld / kTileC), kBlock, 0, stream>>>(a);
	if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
		return e;
	}
	// the missing-call corrections over the effective rows, whose code 3 is M
	const RowView eff_view {eff, 16ull * words16, view.sample_ct, view.record_bytes};
	return LaunchGlmScoreDenseCorr(eff_view, 0, nt, mask, nmiss, pb, b, z0, mz, kp, k, hg, hgn, stream);
}

} // namespace pgh
