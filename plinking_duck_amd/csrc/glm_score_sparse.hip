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
// The walk of a row, its teams, its ordered list and its reductions are TeamWalkSparseRow's (glm_team.hpp), shared with
// GlmSparseKernel; this file holds the score model's arithmetic: list rows [1, z, w, r], and every entry of H_N and g_N
// belongs to one thread that walks the list in order.  A row held in the dense form is walked by the workgroup form
// from its pool row.  Nothing depends on which rows share a workgroup, on the chunk or on where the range starts, and
// there are no floating-point atomics.
#include "glm.hpp"
#include "glm_math.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;
constexpr int kMaxQ = PGH_GLM_MAX_COVAR + 2; // intercept + covariates + genotype

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
		// the ordered-list step (TeamRank in glm_team.hpp)
		uint32_t total;
		const uint32_t pos = TeamRank<kBlock>(take, lane, wave, &total);
		if (take) {
			double *row = list + pos * q;
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
		__syncthreads();
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

// The list rows are [Zt_0..Zt_k, w, r]; the lane sums are U0, A, c_0, c_1 .. c_KP; an owner's entry of the packed
// {H, g} set (ScoreOwnedEntry) adds row[w] * row[a] * row[b].
// sums[i][KP + 6] = {n, sum x, sum x^2, U0, A, c_0, c_1 .. c_KP}; hgn[i] = H_N then g_N, packed as hg.
template <int KP>
struct ScoreModel {
	static constexpr int kNS = KP + 6;
	static constexpr int kNL = KP + 3;
	static constexpr int kTail = 2;
	static constexpr bool kWalksDense = true;
	const double *rr, *ww, *hg;
	double *sums, *hgn;

	struct Sample {
		double r, w;
	};
	struct Own {
		int a, b, w;
	};
	__device__ __forceinline__ bool Load(uint32_t s, Sample *v) const {
		v->r = rr[s];
		if (v->r != v->r) {
			return false;
		}
		v->w = ww[s];
		return true;
	}
	__device__ __forceinline__ void Add(double dd, const Sample &v, const double *zi, double (&ls)[kNL]) const {
		const double wd = v.w * dd;
		ls[0] = fma(dd, v.r, ls[0]);
		ls[1] = fma(wd, dd, ls[1]);
		ls[2] += wd;
#pragma unroll
		for (int j = 0; j < KP; j++) {
			ls[3 + j] = fma(wd, zi[j], ls[3 + j]);
		}
	}
	__device__ __forceinline__ void Tail(const Sample &v, double *tail) const {
		tail[0] = v.w;
		tail[1] = v.r;
	}
	__device__ __forceinline__ Own OwnedEntry(int e, int k) const {
		Own o;
		ScoreOwnedEntry(e, k, &o.a, &o.b, &o.w);
		return o;
	}
	__device__ __forceinline__ double Term(const double *list, uint32_t row, const Own &o) const {
		return list[row + o.w] * list[row + o.a] * list[row + o.b];
	}
	template <int TEAM, int NOWN>
	__device__ __forceinline__ void Epilogue(uint32_t i, int tid, uint32_t k, bool base3, int bx,
	                                         const double (&ls)[kNL], const Own (&own)[NOWN],
	                                         const double (&acc)[NOWN]) const {
		double *h_out = hgn + static_cast<uint64_t>(i) * ((k + 1) * (k + 2) / 2 + k + 1);
		if (tid == 0) {
#pragma unroll
			for (int j = 0; j < kNL; j++) {
				sums[static_cast<uint64_t>(i) * kNS + 3 + j] = ls[j];
			}
		}
#pragma unroll
		for (int t = 0; t < NOWN; t++) {
			if (own[t].a >= 0) {
				const uint32_t e = static_cast<uint32_t>(tid + t * TEAM);
				h_out[e] = base3 ? acc[t] : hg[e] - acc[t];
			}
		}
	}
};

// TEAM == 64 covers the sparse rows of at most kGlmSparseLong entries, TEAM == 256 the longer ones and the rows held in
// the dense form.
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
	extern __shared__ double lds[]; // kBlock list rows of k + 3 doubles (sized at launch)
	const SparseRows rows = {row_of, off, entries, pool, pitch, sample_ct, v_first, nv};
	const ScoreModel<KP> m = {rr, ww, hg, sums, hgn};
	TeamWalkSparseRow<ScoreModel<KP>, KP, TEAM>(rows, z, k, n_y, m, lds);
}

// ---------------------------------------------------------------------------
// the row of a variant: one thread per variant
// ---------------------------------------------------------------------------

// spa.t != null (pgh_glm_score_sparse_spa): a fitted row also leaves t = H_N^-1 c (kp + 1 doubles, zero past k), U and
// V (kp + 3 doubles in all), and every row p_spa = its p (NaN when it is not fitted) and state 0, for GlmScoreSpaKernel to replace.
__global__ void GlmScoreSolveKernel(uint32_t nv, const double *__restrict__ sums, uint32_t kp, uint32_t k,
                                    const double *__restrict__ hgn, int null_status, pgh_glm_row *__restrict__ rows,
                                    GlmScoreSpaOut spa) {
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= nv) {
		return;
	}
	if (spa.t) {
		spa.p_spa[v] = NAN;
		spa.state[v] = 0;
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
	if (spa.t) {
		// t = L^-T (L^-1 c): one back substitution with the factor
		double *t = spa.t + static_cast<uint64_t>(v) * (kp + 3);
		for (int j = static_cast<int>(kp); j >= q1; j--) {
			t[j] = 0.0;
		}
		for (int j = q1 - 1; j >= 0; j--) {
			double x = a[xi * kMaxQ + j];
			for (int m = j + 1; m < q1; m++) {
				x -= a[m * kMaxQ + j] * t[m];
			}
			t[j] = x / a[j * kMaxQ + j];
		}
		t[kp + 1] = u;
		t[kp + 2] = lxx * lxx;
		spa.p_spa[v] = r.p;
	}
}

uint32_t Blocks(uint32_t n, uint32_t per) {
	return (n + per - 1) / per;
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
	const size_t lds = sizeof(double) * kBlock * (k + 3);
	return GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value;
		GlmScoreSparseKernel<KP, 64><<<Blocks(nv, kTeamWaves), kBlock, lds, stream>>>(
		    sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch, sv.sample_ct, v_first, nv, r, w, z, k, n_y, hg, sums, hgn);
		GlmScoreSparseKernel<KP, kBlock><<<nv, kBlock, lds, stream>>>(sv.row_of, sv.off, sv.entries, sv.pool, sv.pitch,
		                                                              sv.sample_ct, v_first, nv, r, w, z, k, n_y, hg, sums,
		                                                              hgn);
	});
}

hipError_t LaunchGlmScoreSolve(uint32_t nv, const double *sums, uint32_t kp, uint32_t k, const double *hgn,
                               int null_status, pgh_glm_row *rows, hipStream_t stream, const GlmScoreSpaOut &spa) {
	if (nv == 0) {
		return hipSuccess;
	}
	GlmScoreSolveKernel<<<Blocks(nv, 64), 64, 0, stream>>>(nv, sums, kp, k, hgn, null_status, rows, spa);
	return hipGetLastError();
}

} // namespace pgh
