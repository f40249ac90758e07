// glm_sparse_multi.hip -- pgh_glm_sparse_multi: the linear fit of every variant of a sparse-resident dataset
// (sparse.hpp) for a block of phenotypes in one walk of the entries (the launch wrappers are in glm.hpp).  The sums are
// those of glm_sparse.hip's header comment, per (row, phenotype j), with S_j the samples that have a value of j.
//
// The value block.  yv[s][j] is one double per (raw sample s, block phenotype j < pb), the phenotype centred on its own
// mean over S_j; NaN: s is outside S_j or outside the subset.  The pb values of a sample are contiguous.  The block is
// cleared to NaN and then written from the uploaded phenotypes in the subset's raw-sample order.
//
// The whole-call Grams.  G_j is the packed upper Gram of u = [1, z - mz_j, yv_j] over S_j, mz_j the covariates' means
// over S_j: kGlmSparseMultiParts workgroups per phenotype each sum a fixed slice of the raw samples in sample order, one
// thread per entry, and a second kernel adds the parts in ascending order.
//
// The entry kernel, lanes across phenotypes: the walk of glm_score_sparse_multi.hip with the linear model's weights.  A
// group of PBW lanes (pb rounded up to a power of two) walks a row, lane j for phenotype j: per entry the group reads
// the entry word and the covariate row once and the lanes read the pb contiguous values of the sample.  A lane keeps
// sum_C d y_j, sum_C d (z_t - mz_j,t) (d = x - b) and its integer counts, gated by yv == yv.  The order of the sums is a
// function of the row alone: consecutive segments of kGlmSparseLong entries (samples, for a dense-form row, which is
// walked from its pool row as a base-0 row), each (segment, phenotype, sum) one fma chain in entry order, the segments'
// chains added in ascending order; a sparse row of at most one segment in the group form, the longer rows and the
// dense-form rows in the workgroup form through LDS.  No floating-point atomics.
//
// The missing-call corrections corr_j (GlmSparseMultiCorrKernel): the Gram of u over the row's list set (its code-3
// entries, or every entry of a base-3 row, where corr_j = G_j - that Gram) intersected with S_j, by the owners' rule
// with a phenotype axis.  A row without list entries is not written: the solve reads G_j for it (nlist[i] == 0).
//
// The solve (GlmSparseMultiSolveKernel): one thread per (row, block phenotype).  It puts the sums back into pgh_glm's
// parameterisation, sum_N x u = b (G_j - corr_j)(1, u) + sum_C d u, and runs GlmLinearSolveRow (glm_linear_solve.hpp),
// the device function of GlmLinearSolveKernel.  The rows are written variant-major, rows[i][j].
#include "glm.hpp"
#include "glm_linear_solve.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;
constexpr uint32_t kSeg = kGlmSparseLong;
constexpr int kCorrOwn = 8;   // (entry, phenotype) pairs a thread of the correction kernel owns
constexpr int kCorrStep = 32; // list rows of one LDS step of the correction kernel
constexpr uint32_t kCorrGroups = 2048; // workgroups of the correction kernel's grid per tile of entries, at most

uint32_t Blocks(uint64_t n, uint32_t per) {
	return static_cast<uint32_t>((n + per - 1) / per);
}

// ---------------------------------------------------------------------------
// the value block
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock) GlmSparseMultiClearKernel(uint64_t n, double *__restrict__ yv) {
	const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
	if (i < n) {
		yv[i] = NAN;
	}
}

// yb: pb x n_out, phenotype-major, NaN = missing; my: the pb means.
__global__ void __launch_bounds__(kBlock) GlmSparseMultiValuesKernel(uint32_t n_out, const uint32_t *__restrict__ sel,
                                                                     const double *__restrict__ yb,
                                                                     const double *__restrict__ my, uint32_t pb,
                                                                     double *__restrict__ yv) {
	const uint64_t at = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
	if (at < static_cast<uint64_t>(n_out) * pb) {
		const uint32_t i = static_cast<uint32_t>(at / pb), j = static_cast<uint32_t>(at - static_cast<uint64_t>(i) * pb);
		const uint32_t s = sel ? sel[i] : i;
		yv[static_cast<uint64_t>(s) * pb + j] = yb[static_cast<uint64_t>(j) * n_out + i] - my[j]; // (NaN stays NaN)
	}
}

// ---------------------------------------------------------------------------
// the whole-call Grams
// ---------------------------------------------------------------------------

// Workgroup (part, j): the samples [part * per, (part + 1) * per) of phenotype j, thread e the entry e.
__global__ void __launch_bounds__(kBlock) GlmSparseMultiGramPartKernel(uint32_t sample_ct, uint32_t per,
                                                                       const double *__restrict__ yv, uint32_t pb,
                                                                       const double *__restrict__ z, uint32_t kp,
                                                                       uint32_t k, const double *__restrict__ mz,
                                                                       double *__restrict__ part) {
	const uint32_t q = k + 2, ne = q * (q + 1) / 2;
	const uint32_t e = threadIdx.x, j = blockIdx.y;
	if (e >= ne) {
		return;
	}
	int a, b;
	PackedUpper(static_cast<int>(e), static_cast<int>(q), &a, &b);
	const bool a_one = a == 0, a_y = a == static_cast<int>(q) - 1, b_y = b == static_cast<int>(q) - 1;
	const bool b_one = b == 0;
	const double ma = (!a_one && !a_y) ? mz[static_cast<uint64_t>(j) * kp + a - 1] : 0.0;
	const double mb = (!b_one && !b_y) ? mz[static_cast<uint64_t>(j) * kp + b - 1] : 0.0;
	const uint64_t s0 = static_cast<uint64_t>(blockIdx.x) * per;
	const uint64_t s1 = s0 + per < sample_ct ? s0 + per : sample_ct;
	double acc = 0.0;
	for (uint64_t s = s0; s < s1; s++) {
		const double v = yv[s * pb + j];
		if (v == v) {
			const double ua = a_one ? 1.0 : a_y ? v : z[s * kp + a - 1] - ma;
			const double ub = b_one ? 1.0 : b_y ? v : z[s * kp + b - 1] - mb;
			acc = fma(ua, ub, acc);
		}
	}
	part[(static_cast<uint64_t>(j) * kGlmSparseMultiParts + blockIdx.x) * ne + e] = acc;
}

__global__ void __launch_bounds__(kBlock) GlmSparseMultiGramSumKernel(uint32_t n, uint32_t ne,
                                                                      const double *__restrict__ part,
                                                                      double *__restrict__ gram) {
	const uint32_t at = blockIdx.x * kBlock + threadIdx.x;
	if (at < n) {
		const uint32_t j = at / ne, e = at - j * ne;
		double sum = 0.0;
		for (uint32_t t = 0; t < kGlmSparseMultiParts; t++) {
			sum += part[(static_cast<uint64_t>(j) * kGlmSparseMultiParts + t) * ne + e];
		}
		gram[at] = sum;
	}
}

// ---------------------------------------------------------------------------
// the entry kernel
// ---------------------------------------------------------------------------

// One lane's sums of one phenotype: ls = {sum_C d y, sum_C d (z_t - mz_t)} and |M|, |C|, sum_C (x - b),
// sum_C (x^2 - b^2).
template <int KP>
struct LaneSums {
	double ls[KP + 1];
	long long cm, cc, sx, sxx;
	__device__ __forceinline__ void Clear() {
#pragma unroll
		for (int t = 0; t < KP + 1; t++) {
			ls[t] = 0.0;
		}
		cm = cc = sx = sxx = 0;
	}
};

// An entry (code, its covariate row zi) of a sample whose value is y joins the lane's sums.
template <int KP>
__device__ __forceinline__ void AddEntry(const double y, uint32_t code, int bx, const double *zi,
                                         const double (&mzr)[KP > 0 ? KP : 1], LaneSums<KP> *a) {
	if (y == y) {
		if (code != 3u) {
			const int d = static_cast<int>(code) - bx;
			a->cc++;
			a->sx += d;
			a->sxx += static_cast<int>(code * code) - bx * bx;
			const double dd = static_cast<double>(d);
			a->ls[0] = fma(dd, y, a->ls[0]);
#pragma unroll
			for (int t = 0; t < KP; t++) {
				a->ls[1 + t] = fma(dd, zi[t] - mzr[t], a->ls[1 + t]);
			}
		} else {
			a->cm++;
		}
	}
}

// The entries [p0, p1) of a sparse row, in order; returns how many belong to the list set.
template <int KP, int PBW, bool LONG>
__device__ __forceinline__ uint32_t WalkEntries(const uint32_t *__restrict__ entries, uint64_t p0, uint64_t p1,
                                                uint32_t sample_ct, const double *__restrict__ yv, uint32_t pb, int j,
                                                const double *__restrict__ z, int bx, bool base3,
                                                const double (&mzr)[KP > 0 ? KP : 1], LaneSums<KP> *a) {
	// entries whose loads are in flight together; with PBW == 64 the covariate rows are held in scalar registers, 2 KP U
	// of them, which must leave the kernel's other scalars their room (the table of DESIGN.md section 3.10)
	constexpr int U = PBW == 64 ? (KP <= 4 ? 4 : KP <= 12 ? 2 : 1) : (KP <= 8 ? 4 : LONG && KP >= 16 ? 1 : 2);
	uint32_t n_list = 0;
	for (uint64_t p = p0; p < p1; p += U) {
		uint32_t x[U];
		double y[U];
		double zi[U][KP > 0 ? KP : 1];
#pragma unroll
		for (int u = 0; u < U; u++) {
			x[u] = p + u < p1 ? entries[p + u] : 0xFFFFFFFFu;
			if constexpr (PBW == 64) {
				x[u] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x[u])));
			}
		}
#pragma unroll
		for (int u = 0; u < U; u++) {
			const uint32_t s = x[u] >> 2;
			y[u] = NAN;
			if (s < sample_ct) {
				y[u] = yv[static_cast<uint64_t>(s) * pb + j];
#pragma unroll
				for (int t = 0; t < KP; t++) {
					zi[u][t] = z[static_cast<uint64_t>(s) * KP + t];
				}
			}
		}
#pragma unroll
		for (int u = 0; u < U; u++) {
			const uint32_t s = x[u] >> 2, code = x[u] & 3u;
			if (s < sample_ct) {
				n_list += (base3 || code == 3u) ? 1u : 0u;
				AddEntry<KP>(y[u], code, bx, zi[u], mzr, a);
			}
		}
	}
	return n_list;
}

// The samples [s0, s1) of a dense-form row (s0 a multiple of 4), in order, as a base-0 row.
template <int KP>
__device__ __forceinline__ uint32_t WalkSamples(const uint8_t *__restrict__ prow, uint32_t s0, uint32_t s1,
                                                const double *__restrict__ yv, uint32_t pb, int j,
                                                const double *__restrict__ z, const double (&mzr)[KP > 0 ? KP : 1],
                                                LaneSums<KP> *a) {
	uint32_t n_list = 0;
	for (uint32_t sb = s0; sb < s1; sb += 4) {
		const uint32_t byte = prow[sb >> 2];
		if (byte == 0u) {
			continue;
		}
		for (uint32_t q = 0; q < 4u && sb + q < s1; q++) {
			const uint32_t code = (byte >> (2u * q)) & 3u, s = sb + q;
			if (code != 0u) {
				n_list += code == 3u ? 1u : 0u;
				double zi[KP > 0 ? KP : 1];
#pragma unroll
				for (int t = 0; t < KP; t++) {
					zi[t] = z[static_cast<uint64_t>(s) * KP + t];
				}
				AddEntry<KP>(yv[static_cast<uint64_t>(s) * pb + j], code, 0, zi, mzr, a);
			}
		}
	}
	return n_list;
}

// sums[i][j][KP + 4] = {n, sum x, sum x^2, sum_C d y, sum_C d zc_t}: the first three final, the others the entry sums
// that the solve puts back into the raw parameterisation.
template <int KP>
__device__ __forceinline__ void StoreSums(const LaneSums<KP> &a, uint32_t i, uint32_t pb, int j, uint32_t n_y, int bx,
                                          bool base3, double *__restrict__ sums) {
	double *so = sums + (static_cast<uint64_t>(i) * pb + j) * (KP + 4);
	const long long n = base3 ? a.cc : static_cast<long long>(n_y) - a.cm;
	so[0] = static_cast<double>(n);
	so[1] = static_cast<double>(bx * n + a.sx);
	so[2] = static_cast<double>(bx * bx * n + a.sxx);
#pragma unroll
	for (int t = 0; t < KP + 1; t++) {
		so[3 + t] = a.ls[t];
	}
}

// LONG == false, the group form: a group of PBW lanes per row, kBlock / PBW rows per workgroup, the sparse rows of at
// most kSeg entries.  LONG == true, the workgroup form: a workgroup per row, the longer sparse rows and the dense-form
// rows.  The two launches cover the same rows and each returns from the other's.
template <int KP, int PBW, bool LONG>
__global__ void __launch_bounds__(kBlock) GlmSparseMultiKernel(SparseRows rows, const double *__restrict__ yv,
                                                               const double *__restrict__ z,
                                                               const double *__restrict__ mz,
                                                               const uint32_t *__restrict__ ny, uint32_t pb,
                                                               double *__restrict__ sums,
                                                               uint32_t *__restrict__ nlist) {
	constexpr int G = kBlock / PBW; // lane groups of a workgroup
	constexpr int NL = KP + 1;
	const int j = static_cast<int>(threadIdx.x) & (PBW - 1), g = static_cast<int>(threadIdx.x) / PBW;
	uint32_t i = LONG ? blockIdx.x : blockIdx.x * G + static_cast<uint32_t>(g);
	if constexpr (PBW == 64) {
		i = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(i)));
	}
	if (i >= rows.nv) {
		return; // (LONG: the whole workgroup)
	}
	const uint32_t r = rows.v_first + i;
	const int32_t ro = rows.row_of[r];
	const bool dense = ro >= 0;
	uint64_t e0 = 0, e1 = rows.sample_ct;
	if (!dense) {
		e0 = rows.off[r];
		e1 = rows.off[r + 1];
	}
	if ((dense || e1 - e0 > kSeg) != LONG) {
		return; // the other launch's row (LONG: the whole workgroup)
	}
	const bool live = static_cast<uint32_t>(j) < pb;
	if (!LONG && !live) {
		return;
	}
	const bool base3 = ro == -4;
	const int bx = (dense || base3) ? 0 : -1 - ro;
	const int jj = live ? j : 0; // (an idle lane of the workgroup form reads phenotype 0's values and stores nothing)
	double mzr[KP > 0 ? KP : 1];
#pragma unroll
	for (int t = 0; t < KP; t++) {
		mzr[t] = mz[static_cast<uint64_t>(jj) * KP + t];
	}
	LaneSums<KP> a;
	a.Clear();
	uint32_t n_list = 0;
	if constexpr (!LONG) {
		n_list = WalkEntries<KP, PBW, false>(rows.entries, e0, e1, rows.sample_ct, yv, pb, jj, z, bx, base3, mzr, &a);
	} else {
		// the groups' chains of a round, G x max(NL, 5) x PBW doubles, then the row's totals, NL x PBW doubles: group 0's
		// lanes alone read and write the totals, each its own, so they cost no registers and need no barrier
		extern __shared__ double part[];
		double *tot = part + kBlock * (NL > 5 ? NL : 5);
		const uint8_t *prow = dense ? rows.pool + static_cast<uint64_t>(ro) * rows.pitch : nullptr;
		const uint64_t n_seg = (e1 - e0 + kSeg - 1) / kSeg;
		if (g == 0) {
#pragma unroll
			for (int t = 0; t < NL; t++) {
				tot[t * PBW + j] = 0.0;
			}
		}
		long long cm = 0, cc = 0, sx = 0, sxx = 0;
		for (uint64_t seg0 = 0; seg0 < n_seg; seg0 += G) {
			const uint64_t seg = seg0 + static_cast<uint64_t>(g);
			a.Clear();
			if (seg < n_seg) {
				const uint64_t p0 = e0 + seg * kSeg, p1 = p0 + kSeg < e1 ? p0 + kSeg : e1;
				if (dense) {
					n_list += WalkSamples<KP>(prow, static_cast<uint32_t>(p0), static_cast<uint32_t>(p1), yv, pb, jj, z, mzr, &a);
				} else {
					n_list += WalkEntries<KP, PBW, true>(rows.entries, p0, p1, rows.sample_ct, yv, pb, jj, z, bx, base3, mzr, &a);
				}
			}
			cm += a.cm;
			cc += a.cc;
			sx += a.sx;
			sxx += a.sxx;
#pragma unroll
			for (int t = 0; t < NL; t++) {
				part[(g * NL + t) * PBW + j] = a.ls[t];
			}
			__syncthreads();
			if (g == 0) {
				const uint64_t left = n_seg - seg0;
				const int n_here = left < static_cast<uint64_t>(G) ? static_cast<int>(left) : G;
#pragma unroll
				for (int t = 0; t < NL; t++) {
					double sum = tot[t * PBW + j];
					for (int gg = 0; gg < n_here; gg++) {
						sum += part[(gg * NL + t) * PBW + j];
					}
					tot[t * PBW + j] = sum;
				}
			}
			__syncthreads();
		}
		// the integer counts of the groups: any order gives the same number
		long long *ipart = reinterpret_cast<long long *>(part);
		ipart[(g * 5 + 0) * PBW + j] = cm;
		ipart[(g * 5 + 1) * PBW + j] = cc;
		ipart[(g * 5 + 2) * PBW + j] = sx;
		ipart[(g * 5 + 3) * PBW + j] = sxx;
		ipart[(g * 5 + 4) * PBW + j] = static_cast<long long>(n_list);
		__syncthreads();
		if (g != 0 || !live) {
			return;
		}
		a.cm = a.cc = a.sx = a.sxx = 0;
		long long nl = 0;
		for (int gg = 0; gg < G; gg++) {
			a.cm += ipart[(gg * 5 + 0) * PBW + j];
			a.cc += ipart[(gg * 5 + 1) * PBW + j];
			a.sx += ipart[(gg * 5 + 2) * PBW + j];
			a.sxx += ipart[(gg * 5 + 3) * PBW + j];
			nl += ipart[(gg * 5 + 4) * PBW + j];
		}
		n_list = static_cast<uint32_t>(nl);
#pragma unroll
		for (int t = 0; t < NL; t++) {
			a.ls[t] = tot[t * PBW + j];
		}
	}
	StoreSums<KP>(a, i, pb, j, ny[j], bx, base3, sums);
	if (j == 0) {
		nlist[i] = n_list;
	}
}

// ---------------------------------------------------------------------------
// the missing-call corrections
// ---------------------------------------------------------------------------

// Workgroup (x, tile): the rows x, x + gridDim.x, .. that have list entries, and of each the entries tile * ET .. of the
// packed Gram, ET = kBlock * kCorrOwn / PBW.  Most rows of a rare-variant file have no list entry, and a workgroup per
// row that only finds that out costs more than the rows that have one: the grid is kCorrGroups wide instead.
// lds: the list rows zl[kCorrStep][k + 1] = [1, z], their values val[kCorrStep][PBW], the transposed sums
// stage[kBlock * kCorrOwn], and the list rows' samples.
template <int PBW>
__global__ void __launch_bounds__(kBlock) GlmSparseMultiCorrKernel(SparseRows rows, const double *__restrict__ yv,
                                                                   const double *__restrict__ z, uint32_t kp,
                                                                   uint32_t k, const double *__restrict__ mz,
                                                                   uint32_t pb, const double *__restrict__ gram,
                                                                   const uint32_t *__restrict__ nlist,
                                                                   double *__restrict__ corr) {
	extern __shared__ __attribute__((aligned(16))) double lds[];
	constexpr int GR = kBlock / PBW;  // entries of one pass of the workgroup's threads
	constexpr int ET = GR * kCorrOwn; // entries of a tile
	const uint32_t q1 = k + 1, q = k + 2, ne = q * (q + 1) / 2;
	const uint32_t tile = blockIdx.y;
	const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
	for (uint32_t i = blockIdx.x; i < rows.nv; i += gridDim.x) {
	if (nlist[i] == 0u) {
		continue; // no list entry: the solve reads G_j (the whole workgroup)
	}
	const uint32_t r = rows.v_first + i;
	const int32_t ro = rows.row_of[r];
	const bool dense = ro >= 0, base3 = ro == -4;
	const uint32_t e_first = tile * ET;
	const uint32_t e_ct = ne - e_first < static_cast<uint32_t>(ET) ? ne - e_first : ET; // (the grid has e_first < ne)

	double *zl = lds;
	double *val = lds + kCorrStep * q1;
	double *stage = val + kCorrStep * PBW;
	uint32_t *sl = reinterpret_cast<uint32_t *>(stage + kBlock * kCorrOwn);

	const int p = tid & (PBW - 1), el0 = tid / PBW;
	const bool live = static_cast<uint32_t>(p) < pb;
	int ea[kCorrOwn], eb[kCorrOwn];
	double ma[kCorrOwn], mb[kCorrOwn], acc[kCorrOwn];
#pragma unroll
	for (int t = 0; t < kCorrOwn; t++) {
		const uint32_t el = static_cast<uint32_t>(el0 + t * GR);
		ea[t] = eb[t] = -1;
		if (live && el < e_ct) {
			PackedUpper(static_cast<int>(e_first + el), static_cast<int>(q), &ea[t], &eb[t]);
		}
		ma[t] = mb[t] = 0.0; // (u_0 = 1 and y are not centred here)
		if (ea[t] > 0 && ea[t] <= static_cast<int>(k)) {
			ma[t] = mz[static_cast<uint64_t>(p) * kp + ea[t] - 1];
		}
		if (eb[t] > 0 && eb[t] <= static_cast<int>(k)) {
			mb[t] = mz[static_cast<uint64_t>(p) * kp + eb[t] - 1];
		}
		acc[t] = 0.0;
	}

	uint64_t e0 = 0, e1 = rows.sample_ct;
	if (!dense) {
		e0 = rows.off[r];
		e1 = rows.off[r + 1];
	}
	const uint8_t *prow = dense ? rows.pool + static_cast<uint64_t>(ro) * rows.pitch : nullptr;
	for (uint64_t p0 = e0; p0 < e1; p0 += kBlock) {
		const uint64_t at = p0 + static_cast<uint64_t>(tid);
		bool take = false;
		uint32_t s = 0;
		if (at < e1) {
			if (dense) {
				s = static_cast<uint32_t>(at);
				take = ((prow[s >> 2] >> (2u * (s & 3u))) & 3u) == 3u;
			} else {
				const uint32_t x = rows.entries[at];
				s = x >> 2;
				take = s < rows.sample_ct && (base3 || (x & 3u) == 3u);
			}
		}
		uint32_t total;
		const uint32_t rank = TeamRank<kBlock>(take, lane, wave, &total);
		for (uint32_t sub = 0; sub < total; sub += kCorrStep) {
			if (take && rank >= sub && rank < sub + kCorrStep) {
				const uint32_t l = rank - sub;
				sl[l] = s;
				zl[l * q1] = 1.0;
				for (uint32_t t = 0; t < k; t++) {
					zl[l * q1 + 1 + t] = z[static_cast<uint64_t>(s) * kp + t];
				}
			}
			__syncthreads();
			const uint32_t nl = total - sub < static_cast<uint32_t>(kCorrStep) ? total - sub : kCorrStep;
			for (uint32_t c = static_cast<uint32_t>(tid); c < nl * PBW; c += kBlock) {
				const uint32_t l = c / PBW, pp = c & (PBW - 1);
				val[c] = pp < pb ? yv[static_cast<uint64_t>(sl[l]) * pb + pp] : NAN;
			}
			__syncthreads();
#pragma unroll
			for (int t = 0; t < kCorrOwn; t++) {
				if (ea[t] >= 0) {
					const bool a_y = ea[t] == static_cast<int>(q1), b_y = eb[t] == static_cast<int>(q1);
					for (uint32_t l = 0; l < nl; l++) {
						const double v = val[l * PBW + p];
						if (v == v) { // in S_p
							const double ua = a_y ? v : zl[l * q1 + ea[t]] - ma[t];
							const double ub = b_y ? v : zl[l * q1 + eb[t]] - mb[t];
							acc[t] = fma(ua, ub, acc[t]);
						}
					}
				}
			}
			__syncthreads();
		}
		__syncthreads(); // TeamRank's counts are rewritten by the next step
	}

	// the tile's sums, transposed through LDS so that a phenotype's entries are stored side by side
#pragma unroll
	for (int t = 0; t < kCorrOwn; t++) {
		stage[(el0 + t * GR) * PBW + p] = acc[t];
	}
	__syncthreads();
	for (uint32_t c = static_cast<uint32_t>(tid); c < pb * e_ct; c += kBlock) {
		const uint32_t pp = c / e_ct, el = c - pp * e_ct, e = e_first + el;
		const double v = stage[el * PBW + pp];
		corr[(static_cast<uint64_t>(i) * pb + pp) * ne + e] = base3 ? gram[static_cast<uint64_t>(pp) * ne + e] - v : v;
	}
	__syncthreads(); // the next row rewrites the stage and the list
	}
}

// ---------------------------------------------------------------------------
// the solve: one thread per (row, block phenotype)
// ---------------------------------------------------------------------------

__global__ void GlmSparseMultiSolveKernel(const int32_t *__restrict__ row_of, uint32_t v_first, uint32_t nv, uint32_t pb,
                                          const double *__restrict__ sums, uint32_t kp, uint32_t k,
                                          const double *__restrict__ gram, const double *__restrict__ corr,
                                          const uint32_t *__restrict__ nlist, pgh_glm_row *__restrict__ rows) {
	const uint64_t at = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (at >= static_cast<uint64_t>(nv) * pb) {
		return;
	}
	const uint32_t i = static_cast<uint32_t>(at / pb), j = static_cast<uint32_t>(at - static_cast<uint64_t>(i) * pb);
	const uint32_t ns = kp + 4, q = k + 2, ne = q * (q + 1) / 2;
	const int32_t ro = row_of[v_first + i];
	const bool base3 = ro == -4;
	const int bx = (ro >= 0 || base3) ? 0 : -1 - ro;
	const bool listed = nlist[i] != 0u;
	const double *sr = sums + at * ns;
	const double *g = gram + static_cast<uint64_t>(j) * ne;
	const double *c = corr + at * ne;
	// corr_j: the stored one; without list entries zero, or G_j itself under base 3 (no entry: no sample)
	const auto corr_at = [&](int e) { return listed ? c[e] : base3 ? g[e] : 0.0; };
	double s[4 + PGH_GLM_MAX_COVAR];
	s[0] = sr[0];
	s[1] = sr[1];
	s[2] = sr[2];
	// entry (1, u_e) of the Gram is entry e: u_e = z_e (1 <= e <= k), y at e == q - 1
	for (uint32_t e = 1; e < q; e++) {
		const double sc = sr[e == q - 1 ? 3 : 3 + e];
		s[e == q - 1 ? 3 : 3 + e] = bx ? static_cast<double>(bx) * (g[e] - corr_at(static_cast<int>(e))) + sc : sc;
	}
	rows[at] = GlmLinearSolveRow<false>(s, k, [&](int e) { return g[e] - corr_at(e); }, false);
}

template <int KP, int PBW>
void LaunchEntryForms(const SparseRows &rows, const double *yv, const double *z, const double *mz, const uint32_t *ny,
                      uint32_t pb, double *sums, uint32_t *nlist, hipStream_t stream) {
	// a block of one phenotype takes the workgroup form of two lanes per group, with one lane idle, as
	// glm_score_sparse_multi.hip's does
	constexpr int G = kBlock / PBW, NL = KP + 1, PBL = PBW == 1 ? 2 : PBW;
	const size_t lds = sizeof(double) * (kBlock * (NL > 5 ? NL : 5) + NL * PBL);
	GlmSparseMultiKernel<KP, PBW, false><<<Blocks(rows.nv, G), kBlock, 0, stream>>>(rows, yv, z, mz, ny, pb, sums, nlist);
	GlmSparseMultiKernel<KP, PBL, true><<<rows.nv, kBlock, lds, stream>>>(rows, yv, z, mz, ny, pb, sums, nlist);
}

template <int PBW>
void LaunchCorr(const SparseRows &rows, const double *yv, const double *z, uint32_t kp, uint32_t k, const double *mz,
                uint32_t pb, const double *gram, const uint32_t *nlist, double *corr, hipStream_t stream) {
	const uint32_t q1 = k + 1, q = k + 2, ne = q * (q + 1) / 2, et = kBlock * kCorrOwn / PBW;
	const size_t lds = sizeof(double) * (kCorrStep * q1 + kCorrStep * PBW + kBlock * kCorrOwn) + 4 * kCorrStep;
	const uint32_t groups = rows.nv < kCorrGroups ? rows.nv : kCorrGroups;
	GlmSparseMultiCorrKernel<PBW><<<dim3(groups, (ne + et - 1) / et), kBlock, lds, stream>>>(rows, yv, z, kp, k, mz, pb,
	                                                                                          gram, nlist, corr);
}

// Calls launch(std::integral_constant<int, PBW>()) with PBW = pb rounded up to a power of two (pb <= 64).
template <class Launch>
void ForGroupWidth(uint32_t pb, Launch &&launch) {
	if (pb <= 1) {
		launch(std::integral_constant<int, 1>());
	} else if (pb <= 2) {
		launch(std::integral_constant<int, 2>());
	} else if (pb <= 4) {
		launch(std::integral_constant<int, 4>());
	} else if (pb <= 8) {
		launch(std::integral_constant<int, 8>());
	} else if (pb <= 16) {
		launch(std::integral_constant<int, 16>());
	} else if (pb <= 32) {
		launch(std::integral_constant<int, 32>());
	} else {
		launch(std::integral_constant<int, 64>());
	}
}

} // namespace

hipError_t LaunchGlmSparseMultiValues(uint32_t sample_ct, uint32_t n_out, const uint32_t *sel, const double *yb,
                                      const double *my, uint32_t pb, double *yv, hipStream_t stream) {
	const uint64_t n = static_cast<uint64_t>(sample_ct) * pb, m = static_cast<uint64_t>(n_out) * pb;
	if (pb == 0 || pb > kGlmSparseMultiPb || n_out > sample_ct) {
		return hipErrorInvalidValue;
	}
	if (n == 0) {
		return hipSuccess;
	}
	GlmSparseMultiClearKernel<<<Blocks(n, kBlock), kBlock, 0, stream>>>(n, yv);
	if (m) {
		GlmSparseMultiValuesKernel<<<Blocks(m, kBlock), kBlock, 0, stream>>>(n_out, sel, yb, my, pb, yv);
	}
	return hipGetLastError();
}

hipError_t LaunchGlmSparseMultiGram(uint32_t sample_ct, const double *yv, uint32_t pb, const double *z, const double *mz,
                                    uint32_t kp, uint32_t k, double *part, double *gram, hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp || pb == 0 || pb > kGlmSparseMultiPb) {
		return hipErrorInvalidValue;
	}
	const uint32_t q = k + 2, ne = q * (q + 1) / 2; // <= kTeamMaxOwned <= kBlock: a thread per entry
	const uint32_t per = (sample_ct + kGlmSparseMultiParts - 1) / kGlmSparseMultiParts;
	GlmSparseMultiGramPartKernel<<<dim3(kGlmSparseMultiParts, pb), kBlock, 0, stream>>>(sample_ct, per, yv, pb, z, kp, k, mz,
	                                                                                    part);
	GlmSparseMultiGramSumKernel<<<Blocks(static_cast<uint64_t>(pb) * ne, kBlock), kBlock, 0, stream>>>(pb * ne, ne, part, gram);
	return hipGetLastError();
}

hipError_t LaunchGlmSparseMulti(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *yv,
                                const uint32_t *n_y, uint32_t pb, const double *z, const double *mz, uint32_t kp,
                                uint32_t k, const double *gram, double *sums, uint32_t *nlist, double *corr,
                                pgh_glm_row *out, hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp || pb == 0 || pb > kGlmSparseMultiPb) {
		return hipErrorInvalidValue;
	}
	if (nv == 0) {
		return hipSuccess;
	}
	const SparseRows rows = {sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, nv};
	const hipError_t err = GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value;
		ForGroupWidth(pb, [&](auto group) {
			constexpr int PBW = decltype(group)::value;
			LaunchEntryForms<KP, PBW>(rows, yv, z, mz, n_y, pb, sums, nlist, stream);
			LaunchCorr<PBW>(rows, yv, z, kp, k, mz, pb, gram, nlist, corr, stream);
		});
	});
	if (err != hipSuccess) {
		return err;
	}
	GlmSparseMultiSolveKernel<<<Blocks(static_cast<uint64_t>(nv) * pb, 64), 64, 0, stream>>>(sv.row_of, v_first, nv, pb, sums,
	                                                                                         kp, k, gram, corr, nlist, out);
	return hipGetLastError();
}

} // namespace pgh
