// glm_score_sparse_multi.hip -- pgh_glm_score_sparse_multi: the logistic score test of every variant of a
// sparse-resident dataset (sparse.hpp) for a block of phenotypes in one walk of the entries (the launch wrappers are in
// glm.hpp).  The sums are those of glm_score_sparse.hip's header comment, per (row, phenotype).
//
// The pair block.  The null fits (LaunchGlmScoreNull, one per phenotype) leave r and w in raw-sample order; the scatter
// kernel writes them to pair[s][j] = (r, w), one double2 per (raw sample s, block phenotype j < pb), so that the pb
// pairs of a sample are contiguous.  r = NaN (w = 0): s is outside S_j or outside the subset; the block is cleared to
// that before its phenotypes write it.
//
// The entry kernel, lanes across phenotypes.  A group of PBW lanes (pb rounded up to a power of two) walks a row, lane j
// for phenotype j: per entry the group reads the entry word and the covariate row once (the same address on every
// lane; with PBW == 64 they are scalar loads) and the lanes read the pb contiguous pairs of the sample.  A lane keeps
// U0, A, c_0 .. c_KP and its integer counts, gated by r == r.  A wave holds 64 / PBW rows.  The entry words, pairs and
// covariate rows of several entries are loaded before their FMAs.
//
// The order of the sums, a function of the row alone.  A sparse row's entries are cut into consecutive segments of
// kGlmSparseLong entries, a dense-form row's samples (it is walked from its pool row as a base-0 row) into consecutive
// segments of kGlmSparseLong samples.  Each (segment, phenotype, sum) is one fma chain in entry order, and the
// segments' chains are added in ascending order.  A sparse row of at most kGlmSparseLong entries is one segment, one
// chain (the group form); the longer rows and the dense-form rows go to a workgroup whose lane groups take the
// segments round robin and add them in order through LDS, where the row's totals live too (the workgroup form).  Neither depends on pb, on which rows
// share a wave, on the chunk or on where the range starts, and there are no floating-point atomics.
//
// Centring.  Phenotype j's covariates are centred on the means over its own missing-value pattern: a lane subtracts its
// means mz[j] from the covariate row per entry, the same subtraction that centred the null fit's covariates.
//
// The missing-call corrections H_N and g_N (GlmScoreSparseMultiCorrKernel): a workgroup per (row, tile of the packed
// {H, g} entries).  The list set (the code-3 entries, or every entry of a base-3 row) does not depend on the phenotype;
// its rows [1, z] and their [entries][pb] tile of (w, r), zero outside S_j, are staged in LDS kCorrStep at a time, and a
// thread owns kCorrOwn (entry, phenotype) pairs, phenotype fastest across lanes, each summed over the list in entry
// order (the owners' rule of glm_team.hpp with a phenotype axis).  A row without list entries copies hg.
#include "glm.hpp"
#include "glm_math.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;
constexpr uint32_t kSeg = kGlmSparseLong;
constexpr int kCorrOwn = 8;   // (entry, phenotype) pairs a thread of the correction kernel owns
constexpr int kCorrStep = 32; // list rows of one LDS step of the correction kernel

// ---------------------------------------------------------------------------
// the pair block
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock) GlmScoreSparsePairClearKernel(uint64_t n, double2 *__restrict__ pair) {
	const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
	if (i < n) {
		pair[i] = make_double2(NAN, 0.0);
	}
}

__global__ void __launch_bounds__(kBlock) GlmScoreSparsePairKernel(uint32_t n_out, const uint32_t *__restrict__ sel,
                                                                   const double *__restrict__ r_raw,
                                                                   const double *__restrict__ w_raw, uint32_t pb,
                                                                   uint32_t j, double2 *__restrict__ pair) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i < n_out) {
		const uint32_t s = sel ? sel[i] : i;
		pair[static_cast<uint64_t>(s) * pb + j] = make_double2(r_raw[s], w_raw[s]);
	}
}

// ---------------------------------------------------------------------------
// the entry kernel
// ---------------------------------------------------------------------------

// One lane's sums of one phenotype: ls = {U0, A, c_0, c_1 .. c_KP} and |M|, |C|, sum_C (x - b), sum_C (x^2 - b^2).
template <int KP>
struct LaneSums {
	double ls[KP + 3];
	long long cm, cc, sx, sxx;
	__device__ __forceinline__ void Clear() {
#pragma unroll
		for (int t = 0; t < KP + 3; t++) {
			ls[t] = 0.0;
		}
		cm = cc = sx = sxx = 0;
	}
};

// An entry (code, its covariate row zi) of a sample whose pair is pr joins the lane's sums.
template <int KP>
__device__ __forceinline__ void AddEntry(const double2 pr, uint32_t code, int bx, const double *zi,
                                         const double (&mzr)[KP > 0 ? KP : 1], LaneSums<KP> *a) {
	if (pr.x == pr.x) {
		if (code != 3u) {
			const int d = static_cast<int>(code) - bx;
			a->cc++;
			a->sx += d;
			a->sxx += static_cast<int>(code * code) - bx * bx;
			const double dd = static_cast<double>(d);
			const double wd = pr.y * dd;
			a->ls[0] = fma(dd, pr.x, a->ls[0]);
			a->ls[1] = fma(wd, dd, a->ls[1]);
			a->ls[2] += wd;
#pragma unroll
			for (int t = 0; t < KP; t++) {
				a->ls[3 + t] = fma(wd, zi[t] - mzr[t], a->ls[3 + t]);
			}
		} else {
			a->cm++;
		}
	}
}

// The entries [p0, p1) of a sparse row, in order; returns how many belong to the list set.
template <int KP, int PBW, bool LONG>
__device__ __forceinline__ uint32_t WalkEntries(const uint32_t *__restrict__ entries, uint64_t p0, uint64_t p1,
                                                uint32_t sample_ct, const double2 *__restrict__ pair, uint32_t pb, int j,
                                                const double *__restrict__ z, int bx, bool base3,
                                                const double (&mzr)[KP > 0 ? KP : 1], LaneSums<KP> *a) {
	// entries whose loads are in flight together; with PBW == 64 the covariate rows are held in scalar registers, 2 KP U
	// of them, which must leave the kernel's other scalars their room; the workgroup form at the two widest widths takes
	// one entry at a time, which keeps it within the vector registers
	constexpr int U = PBW == 64 ? (KP <= 4 ? 4 : KP <= 12 ? 2 : 1) : (KP <= 8 ? 4 : LONG && KP >= 16 ? 1 : 2);
	uint32_t n_list = 0;
	for (uint64_t p = p0; p < p1; p += U) {
		uint32_t x[U];
		double2 pr[U];
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
			pr[u] = make_double2(NAN, 0.0);
			if (s < sample_ct) {
				pr[u] = pair[static_cast<uint64_t>(s) * pb + j];
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
				AddEntry<KP>(pr[u], code, bx, zi[u], mzr, a);
			}
		}
	}
	return n_list;
}

// The samples [s0, s1) of a dense-form row (s0 a multiple of 4), in order, as a base-0 row.
template <int KP>
__device__ __forceinline__ uint32_t WalkSamples(const uint8_t *__restrict__ prow, uint32_t s0, uint32_t s1,
                                                const double2 *__restrict__ pair, uint32_t pb, int j,
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
				AddEntry<KP>(pair[static_cast<uint64_t>(s) * pb + j], code, 0, zi, mzr, a);
			}
		}
	}
	return n_list;
}

// sums[j][i][KP + 6] of the row i for the block phenotype j, and the row's list-set count.
template <int KP>
__device__ __forceinline__ void StoreSums(const LaneSums<KP> &a, uint32_t i, uint32_t nv, int j, uint32_t n_y, int bx,
                                          bool base3, double *__restrict__ sums) {
	double *so = sums + (static_cast<uint64_t>(j) * nv + i) * (KP + 6);
	const long long n = base3 ? a.cc : static_cast<long long>(n_y) - a.cm;
	so[0] = static_cast<double>(n);
	so[1] = static_cast<double>(bx * n + a.sx);
	so[2] = static_cast<double>(bx * bx * n + a.sxx);
#pragma unroll
	for (int t = 0; t < KP + 3; t++) {
		so[3 + t] = a.ls[t];
	}
}

// LONG == false, the group form: a group of PBW lanes per row, kBlock / PBW rows per workgroup, the sparse rows of at
// most kSeg entries.  LONG == true, the workgroup form: a workgroup per row, the longer sparse rows and the dense-form
// rows.  The two launches cover the same rows and each returns from the other's.
template <int KP, int PBW, bool LONG>
__global__ void __launch_bounds__(kBlock) GlmScoreSparseMultiKernel(SparseRows rows, const double2 *__restrict__ pair,
                                                                    const double *__restrict__ z,
                                                                    const double *__restrict__ mz,
                                                                    const uint32_t *__restrict__ ny, uint32_t pb,
                                                                    double *__restrict__ sums,
                                                                    uint32_t *__restrict__ nlist) {
	constexpr int G = kBlock / PBW; // lane groups of a workgroup
	constexpr int NL = KP + 3;
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
		n_list = WalkEntries<KP, PBW, false>(rows.entries, e0, e1, rows.sample_ct, pair, pb, jj, z, bx, base3, mzr, &a);
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
					n_list += WalkSamples<KP>(prow, static_cast<uint32_t>(p0), static_cast<uint32_t>(p1), pair, pb, jj, z, mzr,
					                          &a);
				} else {
					n_list += WalkEntries<KP, PBW, true>(rows.entries, p0, p1, rows.sample_ct, pair, pb, jj, z, bx, base3, mzr, &a);
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
	StoreSums<KP>(a, i, rows.nv, j, ny[j], bx, base3, sums);
	if (j == 0) {
		nlist[i] = n_list;
	}
}

// ---------------------------------------------------------------------------
// the missing-call corrections
// ---------------------------------------------------------------------------

// Workgroup (i, tile): the row i and the entries tile * ET .. of the packed {H, g} set, ET = kBlock * kCorrOwn / PBW.
// lds: the list rows zl[kCorrStep][k + 1], their pairs wr[kCorrStep][PBW] (double2), the transposed sums
// stage[kBlock * kCorrOwn], and the list rows' samples.
template <int PBW>
__global__ void __launch_bounds__(kBlock) GlmScoreSparseMultiCorrKernel(SparseRows rows, const double2 *__restrict__ pair,
                                                                        const double *__restrict__ z, uint32_t kp,
                                                                        uint32_t k, const double *__restrict__ mz,
                                                                        uint32_t pb, const double *__restrict__ hg,
                                                                        const uint32_t *__restrict__ nlist,
                                                                        double *__restrict__ hgn) {
	extern __shared__ __attribute__((aligned(16))) double lds[];
	constexpr int GR = kBlock / PBW;    // entries of one pass of the workgroup's threads
	constexpr int ET = GR * kCorrOwn;   // entries of a tile
	const uint32_t q1 = k + 1, ne = q1 * (q1 + 1) / 2 + q1;
	const uint32_t i = blockIdx.x, tile = blockIdx.y;
	const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
	const uint32_t r = rows.v_first + i;
	const int32_t ro = rows.row_of[r];
	const bool dense = ro >= 0, base3 = ro == -4;
	const uint32_t e_first = tile * ET;
	const uint32_t e_ct = ne - e_first < static_cast<uint32_t>(ET) ? ne - e_first : ET; // (the grid has e_first < ne)

	if (nlist[i] == 0u) {
		// no list entry: H_N = H and g_N = g_S (zeros under base 3); the first tile's workgroup writes the whole row
		if (tile == 0u) {
			for (uint32_t at = static_cast<uint32_t>(tid); at < pb * ne; at += kBlock) {
				const uint32_t p = at / ne, e = at - p * ne;
				hgn[(static_cast<uint64_t>(p) * rows.nv + i) * ne + e] = base3 ? 0.0 : hg[at];
			}
		}
		return;
	}

	double *zl = lds;
	double2 *wr = reinterpret_cast<double2 *>(lds + kCorrStep * q1);
	double *stage = lds + kCorrStep * q1 + 2 * kCorrStep * PBW;
	uint32_t *sl = reinterpret_cast<uint32_t *>(stage + kBlock * kCorrOwn);

	const int p = tid & (PBW - 1), el0 = tid / PBW;
	const bool live = static_cast<uint32_t>(p) < pb;
	int ea[kCorrOwn], eb[kCorrOwn];
	bool is_h[kCorrOwn];
	double ma[kCorrOwn], mb[kCorrOwn], acc[kCorrOwn];
#pragma unroll
	for (int t = 0; t < kCorrOwn; t++) {
		const uint32_t el = static_cast<uint32_t>(el0 + t * GR);
		int ew;
		ScoreOwnedEntry(static_cast<int>(e_first + el), static_cast<int>(k), &ea[t], &eb[t], &ew);
		if (!live || el >= e_ct) {
			ea[t] = -1;
		}
		is_h[t] = ew == static_cast<int>(k) + 1;
		ma[t] = mb[t] = 0.0; // (Zt_0 = 1 is not centred)
		if (ea[t] > 0) {
			ma[t] = mz[static_cast<uint64_t>(p) * kp + ea[t] - 1];
		}
		if (ea[t] >= 0 && eb[t] > 0) {
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
				double2 v = make_double2(0.0, 0.0);
				if (pp < pb) {
					v = pair[static_cast<uint64_t>(sl[l]) * pb + pp];
					if (v.x != v.x) {
						v = make_double2(0.0, 0.0); // outside S_pp: exact zeros join its sums
					}
				}
				wr[c] = v;
			}
			__syncthreads();
#pragma unroll
			for (int t = 0; t < kCorrOwn; t++) {
				if (ea[t] >= 0) {
					for (uint32_t l = 0; l < nl; l++) {
						const double2 v = wr[l * PBW + p];
						const double za = zl[l * q1 + ea[t]] - ma[t], zb = zl[l * q1 + eb[t]] - mb[t];
						acc[t] = fma((is_h[t] ? v.y : v.x) * za, zb, acc[t]);
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
		hgn[(static_cast<uint64_t>(pp) * rows.nv + i) * ne + e] = base3 ? v : hg[static_cast<uint64_t>(pp) * ne + e] - v;
	}
}

uint32_t Blocks(uint64_t n, uint32_t per) {
	return static_cast<uint32_t>((n + per - 1) / per);
}

template <int KP, int PBW>
void LaunchEntryForms(const SparseRows &rows, const double2 *pair, const double *z, const double *mz, const uint32_t *ny,
                      uint32_t pb, double *sums, uint32_t *nlist, hipStream_t stream) {
	// the workgroup form of one lane per group holds the means in scalar registers and spilled some of them: a block of
	// one phenotype takes the form of two lanes per group there, with one lane idle
	constexpr int G = kBlock / PBW, NL = KP + 3, PBL = PBW == 1 ? 2 : PBW;
	const size_t lds = sizeof(double) * (kBlock * (NL > 5 ? NL : 5) + NL * PBL);
	GlmScoreSparseMultiKernel<KP, PBW, false><<<Blocks(rows.nv, G), kBlock, 0, stream>>>(rows, pair, z, mz, ny, pb, sums,
	                                                                                     nlist);
	GlmScoreSparseMultiKernel<KP, PBL, true><<<rows.nv, kBlock, lds, stream>>>(rows, pair, z, mz, ny, pb, sums, nlist);
}

template <int PBW>
void LaunchCorr(const SparseRows &rows, const double2 *pair, const double *z, uint32_t kp, uint32_t k, const double *mz,
                uint32_t pb, const double *hg, const uint32_t *nlist, double *hgn, hipStream_t stream) {
	const uint32_t q1 = k + 1, ne = q1 * (q1 + 1) / 2 + q1, et = kBlock * kCorrOwn / PBW;
	const size_t lds = sizeof(double) * (kCorrStep * q1 + 2 * kCorrStep * PBW + kBlock * kCorrOwn) + 4 * kCorrStep;
	GlmScoreSparseMultiCorrKernel<PBW><<<dim3(rows.nv, (ne + et - 1) / et), kBlock, lds, stream>>>(rows, pair, z, kp, k, mz,
	                                                                                               pb, hg, nlist, hgn);
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

hipError_t LaunchGlmScoreSparsePairClear(uint32_t sample_ct, uint32_t pb, double *pair, hipStream_t stream) {
	const uint64_t n = static_cast<uint64_t>(sample_ct) * pb;
	if (pb == 0 || pb > kGlmScoreSparsePb) {
		return hipErrorInvalidValue;
	}
	if (n == 0) {
		return hipSuccess;
	}
	GlmScoreSparsePairClearKernel<<<Blocks(n, kBlock), kBlock, 0, stream>>>(n, reinterpret_cast<double2 *>(pair));
	return hipGetLastError();
}

hipError_t LaunchGlmScoreSparsePairs(uint32_t n_out, const uint32_t *sel, const double *r_raw, const double *w_raw,
                                     uint32_t pb, uint32_t j, double *pair, hipStream_t stream) {
	if (pb == 0 || pb > kGlmScoreSparsePb || j >= pb) {
		return hipErrorInvalidValue;
	}
	if (n_out == 0) {
		return hipSuccess;
	}
	GlmScoreSparsePairKernel<<<Blocks(n_out, kBlock), kBlock, 0, stream>>>(n_out, sel, r_raw, w_raw, pb, j,
	                                                                       reinterpret_cast<double2 *>(pair));
	return hipGetLastError();
}

hipError_t LaunchGlmScoreSparseMulti(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *pair,
                                     const uint32_t *n_y, uint32_t pb, const double *z0, const double *mz, uint32_t kp,
                                     uint32_t k, const double *hg, double *sums, uint32_t *nlist, double *hgn,
                                     hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp || pb == 0 || pb > kGlmScoreSparsePb) {
		return hipErrorInvalidValue;
	}
	if (nv == 0) {
		return hipSuccess;
	}
	const SparseRows rows = {sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, nv};
	const double2 *pr = reinterpret_cast<const double2 *>(pair);
	return GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value;
		ForGroupWidth(pb, [&](auto group) {
			constexpr int PBW = decltype(group)::value;
			LaunchEntryForms<KP, PBW>(rows, pr, z0, mz, n_y, pb, sums, nlist, stream);
			LaunchCorr<PBW>(rows, pr, z0, kp, k, mz, pb, hg, nlist, hgn, stream);
		});
	});
}

} // namespace pgh
