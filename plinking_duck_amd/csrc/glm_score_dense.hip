// glm_score_dense.hip -- pgh_glm_score_multi: the logistic score test of every variant of a dense-resident dataset for
// many phenotypes at once, on the FP64 matrix cores (the launch wrappers are in glm.hpp).
//
// The row of (variant, phenotype) is the row of glm_score_sparse.hip's header comment with d = x.  With x in {0, 1, 2,
// missing} every x sum of that row is a product of the 2-bit matrix with a real column of the phenotype:
//   U0 = sum x r     c_0 = sum x w     c_j = sum x (w Zt_j)     A = sum x^2 w
// so a phenotype owns k + 2 columns taken against x (r, w, w Zt_1 .. w Zt_k) and one taken against x^2 (w again), all
// 0.0 at a sample outside S_p or outside the subset.  A missing call has x = x^2 = 0, so these sums run over N alone.
//
// Column block (GlmScoreDenseColumnsKernel).  B is sample-major in RAW sample order, ld doubles a row, rows zero padded
// to a whole number of 64-sample steps: the x columns of the block's phenotypes first (phenotype j at j (k + 2)),
// padded to whole 16-column blocks, then the x^2 columns (phenotype j at 16 n_xblocks + j), padded likewise, and ld
// padded to whole column tiles.  A 16-column block is therefore of one kind.  The block is cleared before the
// phenotypes write it, so a subset costs a scatter here and nothing in the contraction.
//
// Contraction (GlmScoreDenseMfmaKernel).  A workgroup of four waves owns 128 variants x 64 columns and walks the
// samples 32 at a time from sample 0, one accumulator chain per (variant, column): v_mfma_f64_16x16x4_f64 with the
// FP64 lane map of grm.hip's header (A: row = lane & 15, k = lane >> 4; B: k = lane >> 4, col = lane & 15; C/D: row =
// (lane >> 4) + 4 reg, col = lane & 15).  Wave w owns the variants 32 w .. 32 w + 31 as two 16-row blocks and all four
// column blocks: eight matrix instructions per two operand values.  The A operand never exists in memory: the four
// samples of an instruction's K are the four codes of one byte of the variant-major row, lane (row, kq) takes code kq
// of byte s of its row's eight bytes of the step and turns it into x (codes {0, 1, 2, 3} -> {0, 1, 2, 0}) or x^2
// ({0, 1, 4, 0}) by the kind of the column block.  B passes through LDS, double buffered, one barrier a step; a row of
// the LDS tile is 80 doubles, so the four k rows of an instruction start 128 bytes apart in the banks.
// Sample tails: the rows of B past the last sample are 0.0 and the resident rows hold code 0 there, so the tail adds
// 0.0 * 0.0, as a code-3 pad would.  A tile row past the chunk's last variant reads the last variant and is not stored.
//
// Order of the sums, and why a row does not depend on its tile.  One workgroup owns the whole sum of an output
// element; the element's accumulator sees the steps in sample order and the instruction's own order inside a step,
// whichever tile row, column block, phenotype block or chunk it sits in, and no other column enters it.  The sample
// axis is not split, and there are no atomics.
//
// Counts (GlmScoreDenseCountsKernel).  n, sum x and sum x^2 over N are integers: a wave counts the het, hom-alt and
// missing codes of the row under the phenotype's sample mask (one bit per 2-bit code, raw-sample order) with popcounts,
// so they are pgh_glm's bit for bit.  It also leaves |M| for the correction kernel.
//
// Missing-call corrections (GlmScoreDenseCorrKernel).  H_N = H - sum_M w Zt Zt', g_N = g_S - sum_M Zt r.  A workgroup
// owns (variant, phenotype): it walks the row 4,096 samples a step (a 16-code word per thread), ranks the missing calls
// of S in sample order (TeamRankCounts over the words' counts), writes their list rows [1, Zt, w, r], 256 at a time, and
// every entry's one owner adds its term in list order: the arithmetic and the order of GlmScoreSparseKernel's owners.
// A variant with M empty copies H and g_S.
// The rows come from GlmScoreSolveKernel (LaunchGlmScoreSolve), unchanged, once per phenotype.
#include "glm.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int kBlock = kTeamBlock;
constexpr uint32_t kTileV = kGlmScoreDenseTileV, kTileC = kGlmScoreDenseTileC, kStep = 32;
constexpr uint32_t kLdsLd = kTileC + 16; // doubles a row of the LDS tile
static_assert(kTileV == 128 && kTileC == 64 && kBlock == 256, "the wave grid below is 4 waves x (32 variants, 64 columns)");

uint32_t Blocks(uint64_t n, uint32_t per) {
	return static_cast<uint32_t>((n + per - 1) / per);
}

// z[i][j] = z0[i][j] - mz[j]: the covariates centred on a missing-value pattern's samples (GlmStage's subtraction)
__global__ void __launch_bounds__(kBlock) GlmScoreDenseCentreKernel(uint64_t total, uint32_t kp,
                                                                    const double *__restrict__ z0,
                                                                    const double *__restrict__ mz,
                                                                    double *__restrict__ z) {
	const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
	if (i < total) {
		z[i] = z0[i] - mz[i % kp];
	}
}

// One phenotype's columns of B, from the null fit's r and w (raw-sample order, NaN r = no phenotype) and the centred
// covariates (output-sample order).  A thread per output sample; the samples outside the subset keep the block's 0.0.
__global__ void __launch_bounds__(kBlock) GlmScoreDenseColumnsKernel(uint32_t n_out, const uint32_t *__restrict__ sel,
                                                                     const double *__restrict__ r_raw,
                                                                     const double *__restrict__ w_raw,
                                                                     const double *__restrict__ z, uint32_t kp, uint32_t k,
                                                                     double *__restrict__ b, uint32_t ld, uint32_t col_x,
                                                                     uint32_t col_sq) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n_out) {
		return;
	}
	const uint32_t s = sel ? sel[i] : i;
	const double r = r_raw[s];
	const bool in = r == r;
	const double w = in ? w_raw[s] : 0.0;
	double *row = b + static_cast<uint64_t>(s) * ld;
	row[col_x] = in ? r : 0.0;
	row[col_x + 1] = w;
	for (uint32_t j = 0; j < k; j++) {
		row[col_x + 2 + j] = w * z[static_cast<uint64_t>(i) * kp + j];
	}
	row[col_sq] = w;
}

// 16 codes of a word under 16 mask bits (bit 2 i of m: sample i counts) -> het, hom-alt, missing
__device__ __forceinline__ void CountWord(uint32_t c, uint32_t m, uint32_t *n1, uint32_t *n2, uint32_t *nm) {
	const uint32_t lo = c & 0x55555555u, hi = (c >> 1) & 0x55555555u;
	*n1 += static_cast<uint32_t>(__popc(lo & ~hi & m));
	*n2 += static_cast<uint32_t>(__popc(hi & ~lo & m));
	*nm += static_cast<uint32_t>(__popc(lo & hi & m));
}

// A wave per (chunk variant, block phenotype): sums[p][v][0..2] = {n, sum x, sum x^2} and nmiss[p][v] = |M|.
// mask: per phenotype 4 * words16 words, zero past the last sample.
__global__ void __launch_bounds__(kBlock) GlmScoreDenseCountsKernel(const uint8_t *__restrict__ rows, uint64_t pitch,
                                                                    uint32_t v0, uint32_t nv, uint32_t words16,
                                                                    const uint32_t *__restrict__ mask, uint32_t pb,
                                                                    const uint32_t *__restrict__ n_y, uint32_t kp,
                                                                    double *__restrict__ sums,
                                                                    uint32_t *__restrict__ nmiss) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * kTeamWaves + (threadIdx.x >> 6);
	if (gw >= static_cast<uint64_t>(nv) * pb) {
		return;
	}
	const uint32_t v = static_cast<uint32_t>(gw / pb), p = static_cast<uint32_t>(gw % pb);
	const uint4 *row = reinterpret_cast<const uint4 *>(rows + static_cast<uint64_t>(v0 + v) * pitch);
	const uint4 *m = reinterpret_cast<const uint4 *>(mask + static_cast<uint64_t>(p) * 4u * words16);
	uint32_t n1 = 0, n2 = 0, nm = 0;
	for (uint32_t i = lane; i < words16; i += 64u) {
		const uint4 c = row[i], mm = m[i];
		CountWord(c.x, mm.x, &n1, &n2, &nm);
		CountWord(c.y, mm.y, &n1, &n2, &nm);
		CountWord(c.z, mm.z, &n1, &n2, &nm);
		CountWord(c.w, mm.w, &n1, &n2, &nm);
	}
	n1 = WaveSum(n1);
	n2 = WaveSum(n2);
	nm = WaveSum(nm);
	if (lane == 0) {
		const uint64_t at = static_cast<uint64_t>(p) * nv + v;
		double *s = sums + at * (kp + 6);
		s[0] = static_cast<double>(n_y[p] - nm);
		s[1] = static_cast<double>(n1 + 2u * n2);
		s[2] = static_cast<double>(n1 + 4u * n2);
		nmiss[at] = nm;
	}
}

struct DenseArgs {
	const uint8_t *rows; // the resident rows
	uint64_t pitch;
	uint32_t v0, nv;  // the chunk: local rows v0 .. v0 + nv - 1
	uint32_t n_steps; // 32-sample steps: B holds 32 n_steps rows
	const double *b;
	uint32_t ld, n_xblocks, pb, k, kp;
	double *sums; // [pb][nv][kp + 6]: slots 3 (U0), 4 (A), 5 .. 5 + k (c) are written
};

__device__ __forceinline__ uint2 LoadCodes(const uint8_t *row, uint32_t ks, uint32_t kq) {
	uint2 w = *reinterpret_cast<const uint2 *>(row + 8ull * ks);
	w.x >>= 2u * kq;
	w.y >>= 2u * kq;
	return w;
}

// instruction S of a step: the samples 4 S .. 4 S + 3; w is already shifted to the lane's k index
template <int S>
__device__ __forceinline__ void KSub(const uint2 (&w)[2], const double *tile, const bool (&sq)[4], v4d (&acc)[2][4]) {
	double bv[4];
#pragma unroll
	for (int y = 0; y < 4; y++) {
		bv[y] = tile[S * 4 * kLdsLd + y * 16];
	}
#pragma unroll
	for (int x = 0; x < 2; x++) {
		const uint32_t word = S < 4 ? w[x].x : w[x].y;
		const uint32_t code = (word >> (8 * (S & 3))) & 3u;
		const uint32_t xv = code == 3u ? 0u : code;
		const double a1 = static_cast<double>(xv), a2 = static_cast<double>(xv * xv);
#pragma unroll
		for (int y = 0; y < 4; y++) {
			acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(sq[y] ? a2 : a1, bv[y], acc[x][y], 0, 0, 0);
		}
	}
}

__global__ void __launch_bounds__(kBlock) GlmScoreDenseMfmaKernel(const DenseArgs a) {
	__shared__ __attribute__((aligned(16))) double s_b[2][kStep * kLdsLd];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const uint32_t li = lane & 15u, kq = lane >> 4;
	const uint32_t vt0 = blockIdx.x * kTileV, cb0 = blockIdx.y * (kTileC / 16u);

	const uint8_t *ra[2];
#pragma unroll
	for (int x = 0; x < 2; x++) {
		const uint32_t v = min(vt0 + wave * 32u + x * 16u + li, a.nv - 1u);
		ra[x] = a.rows + static_cast<uint64_t>(a.v0 + v) * a.pitch;
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

	uint2 wa[2];
#pragma unroll
	for (int x = 0; x < 2; x++) {
		wa[x] = LoadCodes(ra[x], 0, kq);
	}
#pragma unroll
	for (int q = 0; q < 4; q++) {
		*reinterpret_cast<v2d *>(&s_b[0][dst + 2 * q]) = *reinterpret_cast<const v2d *>(src + 2 * q);
	}
	__syncthreads();

	for (uint32_t ks = 0; ks < a.n_steps; ks++) {
		const bool more = ks + 1 < a.n_steps;
		uint2 na[2];
		v2d nb[4];
		if (more) {
			const double *nsrc = src + (ks + 1ull) * src_step;
#pragma unroll
			for (int q = 0; q < 4; q++) {
				nb[q] = *reinterpret_cast<const v2d *>(nsrc + 2 * q);
			}
#pragma unroll
			for (int x = 0; x < 2; x++) {
				na[x] = LoadCodes(ra[x], ks + 1, kq);
			}
		}
		const double *tile = &s_b[ks & 1u][kq * kLdsLd + li];
		KSub<0>(wa, tile, sq, acc);
		KSub<1>(wa, tile, sq, acc);
		KSub<2>(wa, tile, sq, acc);
		KSub<3>(wa, tile, sq, acc);
		KSub<4>(wa, tile, sq, acc);
		KSub<5>(wa, tile, sq, acc);
		KSub<6>(wa, tile, sq, acc);
		KSub<7>(wa, tile, sq, acc);
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

	// ---- epilogue: the lane holds column li, rows kq + 4 reg of each 16 x 16 block ----
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
				if (v < a.nv) {
					a.sums[(static_cast<uint64_t>(p) * a.nv + v) * ns + slot] = acc[x][y][reg];
				}
			}
		}
	}
}

// Workgroup (v, p): hgn[p][v] = hg[p] - the sums over the variant's missing calls in S_p (the file's header comment).
// z0: the uncentred covariates in raw-sample order, mz[p]: the means that centre them for p (kp doubles each).
__global__ void __launch_bounds__(kBlock) GlmScoreDenseCorrKernel(const uint8_t *__restrict__ rows, uint64_t pitch,
                                                                  uint32_t v0, uint32_t nv, uint32_t n_raw,
                                                                  const uint32_t *__restrict__ mask, uint32_t mask_words,
                                                                  const uint32_t *__restrict__ nmiss,
                                                                  const double *__restrict__ b, uint32_t ld,
                                                                  const double *__restrict__ z0, uint32_t kp, uint32_t k,
                                                                  const double *__restrict__ mz,
                                                                  const double *__restrict__ hg,
                                                                  double *__restrict__ hgn) {
	extern __shared__ double list[]; // kBlock rows of k + 3 doubles (sized at launch)
	const uint32_t v = blockIdx.x, p = blockIdx.y;
	const uint32_t q = k + 3, ne = (k + 1) * (k + 2) / 2 + k + 1;
	const uint64_t at = static_cast<uint64_t>(p) * nv + v;
	const double *hgp = hg + static_cast<uint64_t>(p) * ne;
	double *out = hgn + at * ne;
	if (nmiss[at] == 0) {
		if (threadIdx.x < ne) {
			out[threadIdx.x] = hgp[threadIdx.x];
		}
		return;
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int ea, eb, ew;
	ScoreOwnedEntry(threadIdx.x, k, &ea, &eb, &ew);
	const uint32_t *row = reinterpret_cast<const uint32_t *>(rows + static_cast<uint64_t>(v0 + v) * pitch);
	const uint32_t *m = mask + static_cast<uint64_t>(p) * mask_words;
	const double *mzp = mz + static_cast<uint64_t>(p) * kp;
	const uint32_t col_x = p * (k + 2);
	double acc = 0.0;
	// A step is 256 words of 16 codes, a word per thread: the missing calls of S are ranked in thread order and, inside
	// a word, in bit order, which is sample order; they enter the list at most 256 rows at a time.
	for (uint32_t w0 = 0, step = 0; w0 < mask_words; w0 += kBlock, step++) {
		const uint32_t wi = w0 + threadIdx.x;
		uint32_t mm = 0; // bit 2 i: sample 16 wi + i is a missing call of S (the mask is zero past the last sample)
		if (wi < mask_words) {
			const uint32_t c = row[wi];
			mm = c & (c >> 1) & 0x55555555u & m[wi];
		}
		uint32_t total;
		const uint32_t pos = TeamRankCounts(static_cast<uint32_t>(__popc(mm)), step, lane, wave, &total);
		for (uint32_t base = 0; base < total; base += kBlock) { // total is the same on every thread
			uint32_t bits = mm, at = pos;
			while (bits) {
				const uint32_t i = static_cast<uint32_t>(__ffs(static_cast<int>(bits)) - 1) >> 1;
				bits &= bits - 1u;
				if (at >= base && at < base + kBlock) {
					const uint32_t s = 16u * wi + i;
					double *lr = list + (at - base) * q;
					const double *br = b + static_cast<uint64_t>(s) * ld + col_x;
					lr[0] = 1.0;
					for (uint32_t j = 0; j < k; j++) {
						lr[1 + j] = z0[static_cast<uint64_t>(s) * kp + j] - mzp[j];
					}
					lr[k + 1] = br[1];
					lr[k + 2] = br[0];
				}
				at++;
			}
			__syncthreads();
			const uint32_t rows_now = min(static_cast<uint32_t>(kBlock), total - base);
			if (ea >= 0) {
				for (uint32_t i = 0; i < rows_now; i++) {
					acc += list[i * q + ew] * list[i * q + ea] * list[i * q + eb];
				}
			}
			__syncthreads();
		}
	}
	if (threadIdx.x < ne) {
		out[threadIdx.x] = hgp[threadIdx.x] - acc;
	}
}

} // namespace

GlmScoreDenseCols GlmScoreDenseLayout(uint32_t pb, uint32_t k) {
	GlmScoreDenseCols c;
	c.n_xblocks = (pb * (k + 2) + 15u) / 16u;
	const uint32_t n_sqblocks = (pb + 15u) / 16u;
	c.ld = (16u * (c.n_xblocks + n_sqblocks) + kGlmScoreDenseTileC - 1u) / kGlmScoreDenseTileC * kGlmScoreDenseTileC;
	return c;
}

hipError_t LaunchGlmScoreDenseCentre(uint32_t n_out, uint32_t kp, const double *z0, const double *mz, double *z,
                                     hipStream_t stream) {
	const uint64_t total = static_cast<uint64_t>(n_out) * kp;
	if (total == 0) {
		return hipSuccess;
	}
	GlmScoreDenseCentreKernel<<<Blocks(total, kBlock), kBlock, 0, stream>>>(total, kp, z0, mz, z);
	return hipGetLastError();
}

hipError_t LaunchGlmScoreDenseColumns(uint32_t n_out, const uint32_t *sel, const double *r_raw, const double *w_raw,
                                      const double *z, uint32_t kp, uint32_t k, uint32_t pb, uint32_t j, double *b,
                                      hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp || j >= pb || pb > kGlmScoreDensePb) {
		return hipErrorInvalidValue;
	}
	if (n_out == 0) {
		return hipSuccess;
	}
	const GlmScoreDenseCols c = GlmScoreDenseLayout(pb, k);
	GlmScoreDenseColumnsKernel<<<Blocks(n_out, kBlock), kBlock, 0, stream>>>(n_out, sel, r_raw, w_raw, z, kp, k, b, c.ld,
	                                                                         j * (k + 2), 16u * c.n_xblocks + j);
	return hipGetLastError();
}

hipError_t LaunchGlmScoreDense(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask, const uint32_t *n_y,
                               uint32_t pb, const double *b, const double *z0, const double *mz, uint32_t kp,
                               uint32_t k, const double *hg, double *sums, uint32_t *nmiss, double *hgn,
                               hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp || pb == 0 || pb > kGlmScoreDensePb) {
		return hipErrorInvalidValue;
	}
	if (nv == 0) {
		return hipSuccess;
	}
	const uint32_t words16 = (view.sample_ct + 63u) / 64u;
	if (16ull * words16 > view.pitch) {
		return hipErrorInvalidValue; // the kernels read whole 16-byte lanes of a row
	}
	const GlmScoreDenseCols c = GlmScoreDenseLayout(pb, k);
	GlmScoreDenseCountsKernel<<<Blocks(static_cast<uint64_t>(nv) * pb, kTeamWaves), kBlock, 0, stream>>>(
	    view.rows, view.pitch, v0, nv, words16, mask, pb, n_y, kp, sums, nmiss);
	DenseArgs a {};
	a.rows = view.rows;
	a.pitch = view.pitch;
	a.v0 = v0;
	a.nv = nv;
	a.n_steps = words16 * 2u;
	a.b = b;
	a.ld = c.ld;
	a.n_xblocks = c.n_xblocks;
	a.pb = pb;
	a.k = k;
	a.kp = kp;
	a.sums = sums;
	GlmScoreDenseMfmaKernel<<<dim3(Blocks(nv, kTileV), c.ld / kTileC), kBlock, 0, stream>>>(a);
	return LaunchGlmScoreDenseCorr(view, v0, nv, mask, nmiss, pb, b, z0, mz, kp, k, hg, hgn, stream);
}

hipError_t LaunchGlmScoreDenseCorr(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask,
                                   const uint32_t *nmiss, uint32_t pb, const double *b, const double *z0,
                                   const double *mz, uint32_t kp, uint32_t k, const double *hg, double *hgn,
                                   hipStream_t stream) {
	const uint32_t words16 = (view.sample_ct + 63u) / 64u;
	if (k > PGH_GLM_MAX_COVAR || k > kp || pb == 0 || pb > kGlmScoreDensePb || 16ull * words16 > view.pitch) {
		return hipErrorInvalidValue;
	}
	if (nv == 0) {
		return hipSuccess;
	}
	GlmScoreDenseCorrKernel<<<dim3(nv, pb), kBlock, sizeof(double) * kBlock * (k + 3), stream>>>(
	    view.rows, view.pitch, v0, nv, view.sample_ct, mask, 4u * words16, nmiss, b, GlmScoreDenseLayout(pb, k).ld, z0, kp,
	    k, mz, hg, hgn);
	return hipGetLastError();
}

} // namespace pgh
