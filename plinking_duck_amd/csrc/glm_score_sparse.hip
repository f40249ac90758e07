// glm_score_sparse.hip -- pgh_glm_score_sparse: the logistic score test of every variant of a sparse-resident dataset
// (sparse.hpp) from the variant's entries alone (the launch wrappers are in glm.hpp).
//
// The covariates-only logistic model y ~ Zt = [1, z] is fitted once per call (GlmScoreNullKernel: one Newton
// evaluation, the Cholesky step itself runs on the host).  It leaves, in raw-sample order, r = y - mu (NaN: no
// phenotype or outside the subset), w = mu (1 - mu), and the packed H = sum_S w Zt Zt' and g_S = sum_S Zt r.
//
// A row is a base code b and the entries that differ from it.  Of the entries whose sample is in S, M are those with
// code 3 and C the others.  The score of x given Zt is unchanged when a multiple of the intercept is added to x, so
// with d = x - b (d = x under b == 3) every x sum runs over C alone:
//   U0 = sum_C d r,   A = sum_C w d^2,   c_j = sum_C w d Zt_j;
//   b in {0, 1, 2}: H_N = H - sum_M w Zt Zt',  g_N = g_S - sum_M Zt r,  n = n_y - |M|;
//   b == 3:         H_N = sum_C w Zt Zt',      g_N = sum_C Zt r,        n = |C|.
// n, sum x and sum x^2 are integers until they are stored, so they equal pgh_glm's sums bit for bit.
//
// The skeleton is GlmSparseKernel's (glm_sparse.hip): a team (one wave, or the whole workgroup for a row of more than
// kGlmSparseLong entries) walks a row's entries at stride; the sums over C are one fma chain per lane, then a
// butterfly (and waves 0..3 in turn); the entries of the H_N / g_N set are compacted in entry order into an LDS list of
// rows [1, z, w, r], and every entry of H_N and g_N belongs to one thread that walks the list in order.  A row held in
// the dense form is walked by the workgroup form from its pool row, one sample per lane per step, as a base-0 row
// whose entries are the samples with a code other than 0.  Nothing depends on which rows share a workgroup, on the
// chunk or on where the range starts, and there are no floating-point atomics.
#include "device_utils.hpp"
#include "glm.hpp"
#include "glm_math.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxNe = 253; // bounds (k + 1)(k + 2) / 2 + k + 1 = 252 at k = PGH_GLM_MAX_COVAR
constexpr int kMaxQ = PGH_GLM_MAX_COVAR + 2; // intercept + covariates + genotype

// Orders a team's LDS writes before its LDS reads.  A wave's LDS instructions complete in issue order, so a team of
// one wave only has to keep the compiler from moving them.
template <int TEAM>
__device__ inline void TeamSync() {
	if constexpr (TEAM == kBlock) {
		__syncthreads();
	} else {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
}

// Entry e of the packed set {H: sum w Zt_a Zt_b (a <= b <= k, row-major upper), then g: sum r Zt_a (a <= k)} as
// columns of a list row [Zt_0..Zt_k, w, r]: its term is row[ew] * row[ea] * row[eb] (eb = 0, the 1.0, for g).
// ea < 0: there is no such entry.
__device__ inline void ScoreOwnedEntry(int e, int k, int *ea, int *eb, int *ew) {
	const int q1 = k + 1, nh = q1 * (q1 + 1) / 2;
	*ea = *eb = *ew = -1;
	if (e < nh) {
		int a = 0;
		while (e >= q1 - a) {
			e -= q1 - a;
			a++;
		}
		*ea = a;
		*eb = a + e;
		*ew = k + 1;
	} else if (e < nh + q1) {
		*ea = e - nh;
		*eb = 0;
		*ew = k + 2;
	}
}

// ---------------------------------------------------------------------------
// the null model: one Newton evaluation at beta
// ---------------------------------------------------------------------------

// Workgroup b takes the 256-sample steps b, b + kGlmScoreNullParts, ... of the output samples: mu, w and r of every
// sample (stored at its raw index), and its partial of H and g over its samples with a phenotype, each entry summed by
// one thread in sample order.  GlmScoreNullReduceKernel adds the partials in workgroup order.
__global__ void __launch_bounds__(kBlock) GlmScoreNullKernel(uint32_t n_out, const double *__restrict__ y,
                                                             const double *__restrict__ z, uint32_t kp, uint32_t k,
                                                             GlmScoreBeta beta, const uint32_t *__restrict__ sel,
                                                             double *__restrict__ r_raw, double *__restrict__ w_raw,
                                                             double *__restrict__ part) {
	extern __shared__ double list[]; // kBlock rows of q doubles (sized at launch)
	__shared__ uint32_t wave_ct[kWaves];
	const uint32_t q = k + 3, ne = (k + 1) * (k + 2) / 2 + k + 1;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int ea, eb, ew;
	ScoreOwnedEntry(threadIdx.x, k, &ea, &eb, &ew);
	double acc = 0.0;
	for (uint32_t c0 = blockIdx.x * kBlock; c0 < n_out; c0 += kGlmScoreNullParts * kBlock) {
		const uint32_t i = c0 + threadIdx.x;
		bool take = false;
		double ri = 0.0, wi = 0.0;
		if (i < n_out) {
			const double yi = y[i];
			take = yi == yi;
			double eta = beta.b[0];
			for (uint32_t j = 0; j < k; j++) {
				eta = fma(beta.b[1 + j], z[static_cast<uint64_t>(i) * kp + j], eta);
			}
			// (a NaN eta cannot come from a finite beta short of an overflow; r must stay a number on S)
			const double mu = eta == eta ? 1.0 / (1.0 + exp(-eta)) : 0.5;
			wi = take ? mu * (1.0 - mu) : 0.0;
			ri = take ? yi - mu : NAN;
			const uint32_t s = sel ? sel[i] : i;
			r_raw[s] = ri;
			w_raw[s] = wi;
		}
		const uint64_t bal = __ballot(take);
		if (lane == 0) {
			wave_ct[wave] = static_cast<uint32_t>(__popcll(bal));
		}
		__syncthreads();
		uint32_t before = 0, total = 0;
		for (int w = 0; w < kWaves; w++) {
			before += w < wave ? wave_ct[w] : 0u;
			total += wave_ct[w];
		}
		if (take) {
			double *row = list + (before + static_cast<uint32_t>(__popcll(bal & ((1ull << lane) - 1ull)))) * q;
			row[0] = 1.0;
			for (uint32_t j = 0; j < k; j++) {
				row[1 + j] = z[static_cast<uint64_t>(i) * kp + j];
			}
			row[k + 1] = wi;
			row[k + 2] = ri;
		}
		__syncthreads();
		if (ea >= 0) {
			for (uint32_t m = 0; m < total; m++) {
				acc += list[m * q + ew] * list[m * q + ea] * list[m * q + eb];
			}
		}
		__syncthreads(); // the list and wave_ct are rewritten by the next step
	}
	if (threadIdx.x < ne) {
		part[static_cast<uint64_t>(blockIdx.x) * ne + threadIdx.x] = acc;
	}
}

__global__ void __launch_bounds__(kBlock) GlmScoreNullReduceKernel(const double *__restrict__ part, uint32_t ne,
                                                                   double *__restrict__ hg) {
	if (threadIdx.x < ne) {
		double s = part[threadIdx.x];
		for (uint32_t b = 1; b < kGlmScoreNullParts; b++) {
			s += part[static_cast<uint64_t>(b) * ne + threadIdx.x];
		}
		hg[threadIdx.x] = s;
	}
}

// ---------------------------------------------------------------------------
// the entry kernel
// ---------------------------------------------------------------------------

// TEAM == 64: a wave per row, four rows per workgroup, the sparse rows of at most kGlmSparseLong entries.
// TEAM == 256: a workgroup per row, the longer sparse rows and the rows held in the dense form.
// sums[i][KP + 6] = {n, sum x, sum x^2, U0, A, c_0, c_1 .. c_KP}; hgn[i] = H_N then g_N, packed as hg.
template <int KP, int TEAM>
__global__ void __launch_bounds__(kBlock) GlmScoreSparseKernel(const int32_t *__restrict__ row_of,
                                                               const uint64_t *__restrict__ off,
                                                               const uint32_t *__restrict__ entries,
                                                               const uint8_t *__restrict__ pool, uint64_t pitch,
                                                               uint32_t sample_ct, uint32_t v_first, uint32_t nv,
                                                               const double *__restrict__ rr,
                                                               const double *__restrict__ ww,
                                                               const double *__restrict__ z, uint32_t k, uint32_t n_y,
                                                               const double *__restrict__ hg,
                                                               double *__restrict__ sums, double *__restrict__ hgn) {
	constexpr int NS = KP + 6;
	constexpr int NL = KP + 3;                       // the lane sums: U0, A, c_0, c_1 .. c_KP
	constexpr int NOWN = (kMaxNe + TEAM - 1) / TEAM; // entries of H_N and g_N a thread owns
	constexpr int TEAMS = kBlock / TEAM;
	extern __shared__ double lds[]; // kBlock list rows of q doubles (sized at launch)
	const uint32_t q = k + 3, ne = (k + 1) * (k + 2) / 2 + k + 1;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int tid = TEAM == kBlock ? static_cast<int>(threadIdx.x) : lane;
	const uint32_t i = blockIdx.x * TEAMS + (TEAM == kBlock ? 0 : wave);
	if (i >= nv) {
		return; // (the whole team)
	}
	const uint32_t r = v_first + i;
	const int32_t ro = row_of[r];
	const bool dense = ro >= 0;
	uint64_t e0 = 0, e1 = sample_ct; // a dense-form row: its samples
	if (dense) {
		if (TEAM != kBlock) {
			return; // the workgroup launch's row
		}
	} else {
		e0 = off[r];
		e1 = off[r + 1];
		if ((e1 - e0 > kGlmSparseLong) != (TEAM == kBlock)) {
			return; // the other launch's row
		}
	}
	const uint8_t *prow = pool + (dense ? static_cast<uint64_t>(ro) * pitch : 0);
	const bool base3 = ro == -4;
	const int bx = (dense || base3) ? 0 : -1 - ro;
	double *s_out = sums + static_cast<uint64_t>(i) * NS;
	double *h_out = hgn + static_cast<uint64_t>(i) * ne;
	double *list = lds + (TEAM == kBlock ? 0 : static_cast<uint32_t>(wave) * 64u * q);

	int ea[NOWN], eb[NOWN], ew[NOWN];
	double acc[NOWN];
#pragma unroll
	for (int t = 0; t < NOWN; t++) {
		ScoreOwnedEntry(tid + t * TEAM, k, &ea[t], &eb[t], &ew[t]);
		acc[t] = 0.0;
	}

	double ls[NL];
#pragma unroll
	for (int j = 0; j < NL; j++) {
		ls[j] = 0.0;
	}
	long long c_miss = 0, c_called = 0, sx = 0, sxx = 0;
	for (uint64_t p0 = e0; p0 < e1; p0 += TEAM) {
		const uint64_t p = p0 + tid;
		bool used = false;
		uint32_t code = 0, s = 0;
		double ri = 0.0, wi = 0.0;
		if (p < e1) {
			bool entry;
			if (dense) {
				s = static_cast<uint32_t>(p);
				code = (prow[s >> 2] >> (2 * (s & 3u))) & 3u;
				entry = code != 0u;
			} else {
				const uint32_t x = entries[p];
				s = x >> 2;
				code = x & 3u;
				entry = s < sample_ct;
			}
			if (entry) {
				ri = rr[s];
				used = ri == ri;
			}
		}
		double zi[KP > 0 ? KP : 1];
		if (used) {
			wi = ww[s];
#pragma unroll
			for (int j = 0; j < KP; j++) {
				zi[j] = z[static_cast<uint64_t>(s) * KP + j];
			}
			if (code != 3u) {
				const int d = static_cast<int>(code) - bx;
				c_called++;
				sx += d;
				sxx += static_cast<int>(code * code) - bx * bx;
				const double dd = static_cast<double>(d), wd = wi * dd;
				ls[0] = fma(dd, ri, ls[0]);
				ls[1] = fma(wd, dd, ls[1]);
				ls[2] += wd;
#pragma unroll
				for (int j = 0; j < KP; j++) {
					ls[3 + j] = fma(wd, zi[j], ls[3 + j]);
				}
			} else {
				c_miss++;
			}
		}
		// the H_N / g_N set of this step, in entry order (base 3: the called entries, which are all of them)
		const bool take = used && (base3 || code == 3u);
		const uint64_t bal = __ballot(take);
		uint32_t before = 0, total = static_cast<uint32_t>(__popcll(bal));
		if constexpr (TEAM == kBlock) {
			__shared__ uint32_t wave_ct[kWaves];
			if (lane == 0) {
				wave_ct[wave] = total;
			}
			__syncthreads();
			total = 0;
			for (int w = 0; w < kWaves; w++) {
				before += w < wave ? wave_ct[w] : 0u;
				total += wave_ct[w];
			}
		}
		if (total) { // (the whole team agrees)
			if (take) {
				double *row = list + (before + static_cast<uint32_t>(__popcll(bal & ((1ull << lane) - 1ull)))) * q;
				row[0] = 1.0;
#pragma unroll
				for (int j = 0; j < KP; j++) {
					if (j < static_cast<int>(k)) {
						row[1 + j] = zi[j];
					}
				}
				row[k + 1] = wi;
				row[k + 2] = ri;
			}
			TeamSync<TEAM>();
#pragma unroll
			for (int t = 0; t < NOWN; t++) {
				if (ea[t] >= 0) {
					for (uint32_t m = 0; m < total; m++) {
						acc[t] += list[m * q + ew[t]] * list[m * q + ea[t]] * list[m * q + eb[t]];
					}
				}
			}
		}
		TeamSync<TEAM>(); // the list and wave_ct are rewritten by the next step
	}

	// team totals, on every thread
#pragma unroll
	for (int j = 0; j < NL; j++) {
		ls[j] = WaveSum(ls[j]);
	}
	c_miss = WaveSum(c_miss);
	c_called = WaveSum(c_called);
	sx = WaveSum(sx);
	sxx = WaveSum(sxx);
	if constexpr (TEAM == kBlock) {
		__shared__ double part[kWaves][NL];
		__shared__ long long ipart[kWaves][4];
		if (lane == 0) {
#pragma unroll
			for (int j = 0; j < NL; j++) {
				part[wave][j] = ls[j];
			}
			ipart[wave][0] = c_miss;
			ipart[wave][1] = c_called;
			ipart[wave][2] = sx;
			ipart[wave][3] = sxx;
		}
		__syncthreads();
		c_miss = ipart[0][0];
		c_called = ipart[0][1];
		sx = ipart[0][2];
		sxx = ipart[0][3];
#pragma unroll
		for (int j = 0; j < NL; j++) {
			ls[j] = part[0][j];
		}
		for (int w = 1; w < kWaves; w++) {
#pragma unroll
			for (int j = 0; j < NL; j++) {
				ls[j] += part[w][j];
			}
			c_miss += ipart[w][0];
			c_called += ipart[w][1];
			sx += ipart[w][2];
			sxx += ipart[w][3];
		}
	}

	const long long n = base3 ? c_called : static_cast<long long>(n_y) - c_miss;
	if (tid == 0) {
		s_out[0] = static_cast<double>(n);
		s_out[1] = static_cast<double>(bx * n + sx);
		s_out[2] = static_cast<double>(bx * bx * n + sxx);
#pragma unroll
		for (int j = 0; j < NL; j++) {
			s_out[3 + j] = ls[j];
		}
	}
#pragma unroll
	for (int t = 0; t < NOWN; t++) {
		if (ea[t] >= 0) {
			const uint32_t e = static_cast<uint32_t>(tid + t * TEAM);
			h_out[e] = base3 ? acc[t] : hg[e] - acc[t];
		}
	}
}

// ---------------------------------------------------------------------------
// the row of a variant: one thread per variant
// ---------------------------------------------------------------------------

__global__ void GlmScoreSolveKernel(uint32_t nv, const double *__restrict__ sums, uint32_t kp, uint32_t k,
                                    const double *__restrict__ hgn, int null_status, pgh_glm_row *__restrict__ rows) {
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= nv) {
		return;
	}
	const int q1 = static_cast<int>(k) + 1, nh = q1 * (q1 + 1) / 2;
	const double *s = sums + static_cast<uint64_t>(v) * (kp + 6);
	const double *h = hgn + static_cast<uint64_t>(v) * (nh + q1);
	pgh_glm_row r;
	r.beta = r.se = r.stat = r.p = r.a1_freq = NAN;
	r.errcode = PGH_GLM_OK;
	r.firth = 0;
	r.pad[0] = r.pad[1] = 0;
	const double n = s[0];
	r.obs_ct = static_cast<uint32_t>(n);
	if (n < static_cast<double>(k) + 3.0) {
		r.errcode = PGH_GLM_TOO_FEW_SAMPLES;
		rows[v] = r;
		return;
	}
	r.a1_freq = s[1] / (2.0 * n);
	if (GlmConstant(n, s[1], s[2])) {
		r.errcode = PGH_GLM_CONST_ALLELE;
		rows[v] = r;
		return;
	}
	if (null_status != PGH_GLM_OK) {
		r.errcode = static_cast<uint8_t>(null_status);
		rows[v] = r;
		return;
	}
	// the augmented matrix [[H_N, c], [c', A]], lower triangle; its last pivot is V
	double a[kMaxQ * kMaxQ];
	for (int ia = 0, e = 0; ia < q1; ia++) {
		for (int ib = ia; ib < q1; ib++, e++) {
			a[ib * kMaxQ + ia] = h[e];
		}
	}
	const int xi = q1;
	for (int j = 0; j < q1; j++) {
		a[xi * kMaxQ + j] = s[5 + j];
	}
	a[xi * kMaxQ + xi] = s[4];
	if (!GlmCholesky(a, q1 + 1, kMaxQ, 1e-10, nullptr)) {
		r.errcode = PGH_GLM_SINGULAR_MATRIX;
		rows[v] = r;
		return;
	}
	// U = U0 - c' H_N^-1 g_N = U0 - (L^-1 c) . (L^-1 g_N); row xi of the factor is L^-1 c
	double u = s[3];
	double f[kMaxQ];
	for (int j = 0; j < q1; j++) {
		double t = h[nh + j];
		for (int m = 0; m < j; m++) {
			t -= a[j * kMaxQ + m] * f[m];
		}
		f[j] = t / a[j * kMaxQ + j];
		u -= a[xi * kMaxQ + j] * f[j];
	}
	const double lxx = a[xi * kMaxQ + xi]; // sqrt(V)
	r.beta = u / (lxx * lxx);
	r.se = 1.0 / lxx;
	r.stat = u / lxx;
	r.p = GlmPFromZ(r.stat);
	rows[v] = r;
}

uint32_t Blocks(uint32_t n, uint32_t per) {
	return (n + per - 1) / per;
}

template <int KP>
void LaunchBoth(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *r, const double *w, const double *z,
                uint32_t k, uint32_t n_y, const double *hg, double *sums, double *hgn, hipStream_t stream) {
	const size_t lds = sizeof(double) * kBlock * (k + 3);
	GlmScoreSparseKernel<KP, 64><<<Blocks(nv, kWaves), kBlock, lds, stream>>>(
	    sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, nv, r, w, z, k, n_y, hg, sums, hgn);
	GlmScoreSparseKernel<KP, kBlock><<<nv, kBlock, lds, stream>>>(sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch,
	                                                              sv.sample_ct, v_first, nv, r, w, z, k, n_y, hg, sums,
	                                                              hgn);
}

} // namespace

hipError_t LaunchGlmScoreNull(uint32_t n_out, const double *y, const double *z, uint32_t kp, uint32_t k,
                              const GlmScoreBeta &beta, const uint32_t *sel, double *r_raw, double *w_raw, double *part,
                              double *hg, hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp) {
		return hipErrorInvalidValue;
	}
	const uint32_t ne = (k + 1) * (k + 2) / 2 + k + 1;
	GlmScoreNullKernel<<<kGlmScoreNullParts, kBlock, sizeof(double) * kBlock * (k + 3), stream>>>(
	    n_out, y, z, kp, k, beta, sel, r_raw, w_raw, part);
	GlmScoreNullReduceKernel<<<1, kBlock, 0, stream>>>(part, ne, hg);
	return hipGetLastError();
}

hipError_t LaunchGlmScoreSparse(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *r, const double *w,
                                const double *z, uint32_t kp, uint32_t k, uint32_t n_y, const double *hg, double *sums,
                                double *hgn, hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp) {
		return hipErrorInvalidValue;
	}
	if (nv == 0) {
		return hipSuccess;
	}
#define PGH_SCORE_SPARSE(KP_)                                                                                          \
	case KP_:                                                                                                          \
		LaunchBoth<KP_>(sv, v_first, nv, r, w, z, k, n_y, hg, sums, hgn, stream);                                      \
		break;
	switch (kp) {
		PGH_SCORE_SPARSE(0)
		PGH_SCORE_SPARSE(1)
		PGH_SCORE_SPARSE(2)
		PGH_SCORE_SPARSE(4)
		PGH_SCORE_SPARSE(8)
		PGH_SCORE_SPARSE(12)
		PGH_SCORE_SPARSE(16)
		PGH_SCORE_SPARSE(20)
	default:
		return hipErrorInvalidValue;
	}
#undef PGH_SCORE_SPARSE
	return hipGetLastError();
}

hipError_t LaunchGlmScoreSolve(uint32_t nv, const double *sums, uint32_t kp, uint32_t k, const double *hgn,
                               int null_status, pgh_glm_row *rows, hipStream_t stream) {
	if (nv == 0) {
		return hipSuccess;
	}
	GlmScoreSolveKernel<<<Blocks(nv, 64), 64, 0, stream>>>(nv, sums, kp, k, hgn, null_status, rows);
	return hipGetLastError();
}

} // namespace pgh
