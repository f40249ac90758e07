// glm.hip -- plink_glm's per-variant regressions in FP64 (glm.hpp).
//
// Linear: one pass over the rows.  Only the genotype terms change between variants, so a workgroup accumulates
// {n, sum x, sum x^2, sum x y, sum x z_j} for a tile of T variants (each sample's y and z are loaded once for the
// tile); the covariate block [1, z, y]' [1, z, y] is one Gram per call, and a variant with missing calls subtracts
// the Gram of those samples (a compacted list per sample chunk: sparse when calls are rarely missing, any count
// works; the ranking of the list and the barriers around its walk are TeamRank's, glm_team.hpp).  The solve is a
// Cholesky of the augmented [1, z, x, y] matrix per variant.
// Logistic / Firth: rounds of an accumulation launch (one workgroup per variant still in play) and a per-variant
// update launch (one thread per variant).
//
// Determinism: a thread always owns the same samples (stride 256) and reductions run in one fixed order, so a
// variant's sums do not depend on its place in a tile, chunk or shard.
#include "device_utils.hpp"
#include "glm.hpp"
#include "glm_linear_solve.hpp"
#include "glm_math.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxP = kGlmSolveMaxP;

__device__ inline double GlmValue(const GlmX &g, uint32_t v, uint32_t i) {
	const int32_t s = g.slot ? g.slot[v] : -1;
	if (s >= 0) {
		return g.dos[static_cast<uint64_t>(s) * g.n_out + i];
	}
	const uint32_t raw = g.sel ? g.sel[i] : i;
	const uint8_t *row = g.view.rows + static_cast<uint64_t>(g.v0 + v) * g.view.pitch;
	const uint32_t c = (row[raw >> 2] >> (2 * (raw & 3))) & 3u;
	return c == 3u ? -9.0 : static_cast<double>(c);
}

// Block sum of NE per-thread values in a fixed order: butterfly within each wave, then waves 0..3 in turn.
template <int NE>
__device__ inline void BlockSums(const double (&acc)[NE], double *lds, double *out) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int e = 0; e < NE; e++) {
		const double s = WaveSum(acc[e]);
		if (lane == 0) {
			lds[wave * NE + e] = s;
		}
	}
	__syncthreads();
	for (int e = threadIdx.x; e < NE; e += kBlock) {
		double s = lds[e];
		for (int w = 1; w < kWaves; w++) {
			s += lds[w * NE + e];
		}
		out[e] = s;
	}
}

// ---------------------------------------------------------------------------
// linear sums
// ---------------------------------------------------------------------------

template <int KP, int T>
__global__ void __launch_bounds__(kBlock) GlmSumsKernel(GlmX g, uint32_t nv, const double *__restrict__ y,
                                                        const double *__restrict__ z, double *__restrict__ sums) {
	constexpr int NS = KP + 4;
	__shared__ double lds[kWaves * NS * T];
	const uint32_t v0 = blockIdx.x * T;
	double acc[NS * T];
#pragma unroll
	for (int e = 0; e < NS * T; e++) {
		acc[e] = 0.0;
	}
	for (uint32_t i = threadIdx.x; i < g.n_out; i += kBlock) {
		const double yi = y[i];
		if (yi != yi) {
			continue;
		}
		double zi[KP > 0 ? KP : 1];
#pragma unroll
		for (int j = 0; j < KP; j++) {
			zi[j] = z[static_cast<uint64_t>(i) * KP + j];
		}
#pragma unroll
		for (int t = 0; t < T; t++) {
			if (v0 + t < nv) {
				const double x = GlmValue(g, v0 + t, i);
				if (x != -9.0) {
					double *a = acc + t * NS;
					a[0] += 1.0;
					a[1] += x;
					a[2] += x * x;
					a[3] += x * yi;
#pragma unroll
					for (int j = 0; j < KP; j++) {
						a[4 + j] += x * zi[j];
					}
				}
			}
		}
	}
	__shared__ double tile[NS * T];
	BlockSums<NS * T>(acc, lds, tile);
	__syncthreads();
	for (int e = threadIdx.x; e < NS * T; e += kBlock) {
		if (v0 + e / NS < nv) {
			sums[static_cast<uint64_t>(v0) * NS + e] = tile[e];
		}
	}
}

// ---------------------------------------------------------------------------
// Gram of [1, z, y] over a compacted sample list
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock) GlmGramKernel(GlmX g, int per_variant, const double *__restrict__ sums,
                                                        uint32_t sums_stride, uint32_t n_y, uint32_t n_out,
                                                        const double *__restrict__ y, const double *__restrict__ z,
                                                        uint32_t kp, uint32_t k, double *__restrict__ out) {
	const uint32_t q = k + 2, ne = q * (q + 1) / 2;
	const uint32_t v = blockIdx.x;
	double *dst = out + static_cast<uint64_t>(v) * ne;
	if (per_variant && sums[static_cast<uint64_t>(v) * sums_stride] == static_cast<double>(n_y)) {
		for (uint32_t e = threadIdx.x; e < ne; e += kBlock) {
			dst[e] = 0.0;
		}
		return;
	}
	extern __shared__ double list[]; // kBlock rows of q doubles (sized at launch)
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	// entry owned by this thread
	int ea = -1, eb = -1;
	if (threadIdx.x < ne) {
		PackedUpper(threadIdx.x, q, &ea, &eb);
	}
	double acc = 0.0;
	for (uint32_t c0 = 0; c0 < n_out; c0 += kBlock) {
		const uint32_t i = c0 + threadIdx.x;
		bool take = false;
		double yi = 0.0;
		if (i < n_out) {
			yi = y[i];
			take = yi == yi && (!per_variant || GlmValue(g, v, i) == -9.0);
		}
		// the ordered-list step (TeamRank in glm_team.hpp)
		uint32_t total;
		const uint32_t pos = TeamRank<kBlock>(take, lane, wave, &total);
		if (take) {
			double *r = list + pos * q;
			r[0] = 1.0;
			for (uint32_t j = 0; j < k; j++) {
				r[1 + j] = z[static_cast<uint64_t>(i) * kp + j];
			}
			r[q - 1] = yi;
		}
		__syncthreads();
		if (ea >= 0) {
			for (uint32_t s = 0; s < total; s++) {
				acc += list[s * q + ea] * list[s * q + eb];
			}
		}
		__syncthreads();
	}
	if (ea >= 0) {
		dst[threadIdx.x] = acc;
	}
}

// ---------------------------------------------------------------------------
// linear solve: one thread per variant
// ---------------------------------------------------------------------------

// FLAGGED (pgh_burden_sparse): x is not on the dosage grid, so CONST_ALLELE is decided by the caller (x_const[v] != 0)
// and the correction Gram is zero (corr is not read).  FLAGGED == false is the kernel of pgh_glm and pgh_glm_sparse.
template <bool FLAGGED>
__global__ void GlmLinearSolveKernel(uint32_t nv, const double *__restrict__ sums, uint32_t kp, uint32_t k,
                                     const double *__restrict__ gram, const double *__restrict__ corr,
                                     const uint8_t *__restrict__ x_const, pgh_glm_row *__restrict__ rows) {
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= nv) {
		return;
	}
	const uint32_t ns = kp + 4, q = k + 2, ne = q * (q + 1) / 2;
	const double *s = sums + static_cast<uint64_t>(v) * ns;
	if constexpr (FLAGGED) {
		rows[v] = GlmLinearSolveRow<true>(s, k, [&](int e) { return gram[e]; }, x_const[v] != 0);
	} else {
		const double *c = corr + static_cast<uint64_t>(v) * ne;
		rows[v] = GlmLinearSolveRow<false>(s, k, [&](int e) { return gram[e] - c[e]; }, false);
	}
}

// ---------------------------------------------------------------------------
// logistic / Firth
// ---------------------------------------------------------------------------

__global__ void GlmLogisticInitKernel(uint32_t nv, const double *__restrict__ sums, uint32_t kp_sums, uint32_t kp,
                                      uint32_t k, GlmState *__restrict__ st, double *__restrict__ beta,
                                      pgh_glm_row *__restrict__ rows) {
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= nv) {
		return;
	}
	const double *s = sums + static_cast<uint64_t>(v) * (kp_sums + 4);
	pgh_glm_row r;
	SetRowNull(r);
	GlmState g;
	g.status = kGlmActive;
	g.iter = 0;
	g.firth = 0;
	g.pad = 0;
	g.min_delta = 1e9;
	g.delta_max = 0.0;
	g.loglik = g.loglik_old = 0.0;
	const double n = s[0];
	r.obs_ct = static_cast<uint32_t>(n);
	if (n < static_cast<double>(k) + 3.0) {
		r.errcode = PGH_GLM_TOO_FEW_SAMPLES;
		g.status = kGlmDecided + PGH_GLM_TOO_FEW_SAMPLES;
	} else {
		r.a1_freq = s[1] / (2.0 * n);
		if (GlmConstant(n, s[1], s[2])) {
			r.errcode = PGH_GLM_CONST_ALLELE;
			g.status = kGlmDecided + PGH_GLM_CONST_ALLELE;
		}
	}
	for (uint32_t j = 0; j < kp + 2; j++) {
		beta[static_cast<uint64_t>(v) * (kp + 2) + j] = 0.0;
	}
	st[v] = g;
	rows[v] = r;
}

template <int KP, int MODE>
__global__ void __launch_bounds__(kBlock) GlmIrlsAccKernel(GlmX g, const uint32_t *__restrict__ list,
                                                           const double *__restrict__ y, const double *__restrict__ z,
                                                           const GlmState *__restrict__ st,
                                                           const double *__restrict__ beta,
                                                           const double *__restrict__ hinv0, double *__restrict__ acc_out) {
	constexpr int PP = KP + 2;
	constexpr int NH = PP * (PP + 1) / 2;
	constexpr int NE = NH + PP + 2;
	const uint32_t v = list ? list[blockIdx.x] : blockIdx.x;
	if (st[v].status != kGlmActive) {
		return;
	}
	__shared__ double lds[kWaves * NE];
	__shared__ double hin[MODE == 2 ? PP * PP : 1];
	double b[PP];
#pragma unroll
	for (int j = 0; j < PP; j++) {
		b[j] = beta[static_cast<uint64_t>(v) * PP + j];
	}
	if (MODE == 2) {
		for (int e = threadIdx.x; e < PP * PP; e += kBlock) {
			hin[e] = hinv0[static_cast<uint64_t>(v) * PP * PP + e];
		}
		__syncthreads();
	}
	double acc[NE];
#pragma unroll
	for (int e = 0; e < NE; e++) {
		acc[e] = 0.0;
	}
	for (uint32_t i = threadIdx.x; i < g.n_out; i += kBlock) {
		const double yi = y[i];
		if (yi != yi) {
			continue;
		}
		const double x = GlmValue(g, v, i);
		if (x == -9.0) {
			continue;
		}
		double xr[PP];
		xr[0] = 1.0;
		xr[1] = x;
#pragma unroll
		for (int j = 0; j < KP; j++) {
			xr[2 + j] = z[static_cast<uint64_t>(i) * KP + j];
		}
		double eta = 0.0;
#pragma unroll
		for (int j = 0; j < PP; j++) {
			eta += b[j] * xr[j];
		}
		const double mu = 1.0 / (1.0 + exp(-eta));
		const double var = mu * (1.0 - mu);
		double w = var, r = mu - yi;
		if (MODE == 1) {
			if (mu == 0.0 || mu == 1.0) {
				acc[NE - 1] += 1.0;
			}
			acc[NH + PP] += yi != 0.0 ? log(mu) : log1p(-mu);
		} else if (MODE == 2) {
			double h = 0.0;
#pragma unroll
			for (int a = 0; a < PP; a++) {
				double t = 0.0;
#pragma unroll
				for (int c = 0; c < PP; c++) {
					t += hin[a * PP + c] * xr[c];
				}
				h += xr[a] * t;
			}
			h *= var;
			r = (yi - mu) + h * (0.5 - mu);
			w = (1.0 + h) * var;
		}
		int e = 0;
#pragma unroll
		for (int a = 0; a < PP; a++) {
			const double wa = w * xr[a];
#pragma unroll
			for (int c = a; c < PP; c++) {
				acc[e++] += wa * xr[c];
			}
		}
		if (MODE != 1) {
#pragma unroll
			for (int a = 0; a < PP; a++) {
				acc[NH + a] += r * xr[a];
			}
		}
	}
	BlockSums<NE>(acc, lds, acc_out + static_cast<uint64_t>(v) * NE);
}

// unpack the real p x p block of a packed upper matrix of order pp into a full row-major matrix of stride kMaxP
__device__ inline void UnpackSym(const double *packed, int pp, int p, double *m) {
	for (int a = 0; a < p; a++) {
		for (int c = a; c < p; c++) {
			const double val = packed[PackIdx(a, c, pp)];
			m[a * kMaxP + c] = val;
			m[c * kMaxP + a] = val;
		}
	}
}

__global__ void GlmNewtonUpdateKernel(uint32_t nv, uint32_t kp, uint32_t k, const double *__restrict__ acc,
                                      GlmState *__restrict__ st, double *__restrict__ beta, double *__restrict__ hmat) {
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= nv || st[v].status != kGlmActive) {
		return;
	}
	const int pp = kp + 2, p = k + 2;
	const int nh = pp * (pp + 1) / 2, ne = nh + pp + 2;
	const double *a = acc + static_cast<uint64_t>(v) * ne;
	double h[kMaxP * kMaxP], l[kMaxP * kMaxP], d[kMaxP];
	UnpackSym(a, pp, p, h);
	double *hs = hmat + static_cast<uint64_t>(v) * kMaxP * kMaxP;
	for (int e = 0; e < p * kMaxP; e++) {
		hs[e] = h[e];
	}
	// the reference's Cholesky: a negative pivot is replaced by 1e-6 rather than failing the fit
	for (int j = 0; j < p; j++) {
		double dd = h[j * kMaxP + j];
		for (int t = 0; t < j; t++) {
			dd -= l[j * kMaxP + t] * l[j * kMaxP + t];
		}
		const double lj = dd >= 0.0 ? sqrt(dd) : 1e-6;
		l[j * kMaxP + j] = lj;
		const double inv = 1.0 / lj;
		for (int i = j + 1; i < p; i++) {
			double s = h[i * kMaxP + j];
			for (int t = 0; t < j; t++) {
				s -= l[i * kMaxP + t] * l[j * kMaxP + t];
			}
			l[i * kMaxP + j] = s * inv;
		}
	}
	for (int j = 0; j < p; j++) {
		d[j] = a[nh + j];
	}
	GlmCholSolve(l, p, kMaxP, d);
	GlmState s = st[v];
	double *b = beta + static_cast<uint64_t>(v) * pp;
	double delta = 0.0;
	for (int j = 0; j < p; j++) {
		delta += fabs(d[j]);
		b[j] -= d[j];
	}
	const int it = s.iter++;
	s.min_delta = delta < s.min_delta ? delta : s.min_delta;
	if (delta != delta) {
		s.status = kGlmFailed;
	} else {
		bool done = false;
		if (it > 3) {
			if ((delta > 20.0 && delta > 2 * s.min_delta) || (it > 6 && fabs(1.0 - delta) < 1e-3)) {
				s.status = kGlmFailed;
				done = true;
			} else if (it > 13) {
				s.status = kGlmUnfinished;
				for (int j = 0; j < p; j++) {
					if (fabs(b[j]) > 8e3) {
						s.status = kGlmFailed;
					}
				}
				done = true;
			}
		}
		if (!done && delta < 1e-4) {
			s.status = kGlmConverged;
			for (int j = 0; j < p; j++) {
				if (fabs(b[j]) > 6e4) {
					s.status = kGlmFailed;
				}
			}
		}
	}
	st[v] = s;
}

__global__ void GlmFirthStartKernel(const uint32_t *__restrict__ list, uint32_t n, uint32_t kp,
                                    GlmState *__restrict__ st, double *__restrict__ beta) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) {
		return;
	}
	const uint32_t v = list[t];
	GlmState s = st[v];
	s.status = kGlmActive;
	s.iter = 0;
	s.firth = 1;
	s.delta_max = 0.0;
	s.loglik = s.loglik_old = 0.0;
	st[v] = s;
	for (uint32_t j = 0; j < kp + 2; j++) {
		beta[static_cast<uint64_t>(v) * (kp + 2) + j] = 0.0;
	}
}

// half 0: after the first pass (I(beta), log-likelihood): penalised log-likelihood and I(beta)^-1.
// half 1: after the second pass (U*, second-weight Hessian): the convergence tests, then the capped step.
__global__ void GlmFirthUpdateKernel(int half, const uint32_t *__restrict__ list, uint32_t n, uint32_t kp, uint32_t k,
                                     const double *__restrict__ acc, GlmState *__restrict__ st,
                                     double *__restrict__ beta, double *__restrict__ hinv0, double *__restrict__ hmat) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) {
		return;
	}
	const uint32_t v = list[t];
	GlmState s = st[v];
	if (s.status != kGlmActive) {
		return;
	}
	const int pp = kp + 2, p = k + 2;
	const int nh = pp * (pp + 1) / 2, ne = nh + pp + 2;
	const double *a = acc + static_cast<uint64_t>(v) * ne;
	double h[kMaxP * kMaxP], col[kMaxP];
	UnpackSym(a, pp, p, h);
	if (half == 0) {
		double logdet = 0.0;
		if (a[ne - 1] != 0.0 || !GlmCholesky(h, p, kMaxP, 1e-13, &logdet)) {
			s.status = kGlmFailed;
			st[v] = s;
			return;
		}
		s.loglik = a[nh + pp] + 0.5 * logdet;
		double *dst = hinv0 + static_cast<uint64_t>(v) * pp * pp;
		double inv[kMaxP * kMaxP];
		GlmCholInverse(h, p, kMaxP, inv, col);
		for (int i = 0; i < pp; i++) {
			for (int c = 0; c < pp; c++) {
				dst[i * pp + c] = (i < p && c < p) ? inv[i * kMaxP + c] : 0.0;
			}
		}
		st[v] = s;
		return;
	}
	double ustar_max = 0.0;
	for (int j = 0; j < p; j++) {
		ustar_max = fmax(ustar_max, fabs(a[nh + j]));
	}
	if (s.iter > 0) {
		if (s.delta_max <= 1e-4 && ustar_max < 1e-4 && s.loglik - s.loglik_old < 1e-4) {
			s.status = kGlmConverged;
			st[v] = s;
			return;
		}
		if (s.iter > 25) {
			s.status = kGlmUnfinished;
			st[v] = s;
			return;
		}
	}
	s.loglik_old = s.loglik;
	if (!GlmCholesky(h, p, kMaxP, 1e-13, nullptr)) {
		s.status = kGlmFailed;
		st[v] = s;
		return;
	}
	double inv[kMaxP * kMaxP];
	GlmCholInverse(h, p, kMaxP, inv, col);
	double *hs = hmat + static_cast<uint64_t>(v) * kMaxP * kMaxP;
	for (int e = 0; e < p * kMaxP; e++) {
		hs[e] = inv[e];
	}
	double dl[kMaxP];
	double dmax = 0.0;
	for (int i = 0; i < p; i++) {
		double sdot = 0.0;
		for (int c = 0; c < p; c++) {
			sdot += inv[i * kMaxP + c] * a[nh + c];
		}
		dl[i] = sdot;
		dmax = fmax(dmax, fabs(sdot));
	}
	if (dmax > 5.0) {
		const double sc = 5.0 / dmax;
		for (int i = 0; i < p; i++) {
			dl[i] *= sc;
		}
		dmax = 5.0;
	}
	s.delta_max = dmax;
	double *b = beta + static_cast<uint64_t>(v) * pp;
	for (int i = 0; i < p; i++) {
		b[i] += dl[i];
	}
	s.iter++;
	st[v] = s;
}

__global__ void GlmLogisticFinishKernel(uint32_t nv, uint32_t kp, uint32_t k, const GlmState *__restrict__ st, const double *__restrict__ beta,
                                        const double *__restrict__ hmat, pgh_glm_row *__restrict__ rows) {
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= nv) {
		return;
	}
	const GlmState s = st[v];
	if (s.status >= kGlmDecided) {
		return; // row written by the init kernel
	}
	pgh_glm_row r = rows[v];
	const int pp = kp + 2, p = k + 2;
	const double *hs = hmat + static_cast<uint64_t>(v) * kMaxP * kMaxP;
	double se2;
	if (s.firth) {
		if (s.status == kGlmFailed) {
			r.errcode = PGH_GLM_NO_CONVERGENCE;
			rows[v] = r;
			return;
		}
		r.firth = 1;
		se2 = hs[1 * kMaxP + 1];
	} else {
		if (s.status != kGlmConverged) {
			r.errcode = s.status == kGlmFailed ? PGH_GLM_SEPARATION : PGH_GLM_NO_CONVERGENCE;
			rows[v] = r;
			return;
		}
		double l[kMaxP * kMaxP], col[kMaxP];
		for (int e = 0; e < p * kMaxP; e++) {
			l[e] = hs[e];
		}
		if (!GlmCholesky(l, p, kMaxP, 1e-13, nullptr)) {
			r.errcode = PGH_GLM_SINGULAR_MATRIX;
			rows[v] = r;
			return;
		}
		for (int i = 0; i < p; i++) {
			col[i] = i == 1 ? 1.0 : 0.0;
		}
		GlmCholSolve(l, p, kMaxP, col);
		se2 = col[1];
	}
	r.beta = beta[static_cast<uint64_t>(v) * pp + 1];
	if (se2 < 1e-30) {
		r.errcode = PGH_GLM_ZERO_VARIANCE;
		rows[v] = r;
		return;
	}
	r.se = sqrt(se2);
	r.stat = r.beta / r.se;
	r.p = GlmPFromZ(r.stat);
	rows[v] = r;
}

// ---------------------------------------------------------------------------
// many phenotypes (pgh_glm_multi, linear): the phenotypes of one missing-value pattern share n, sum x, sum x^2,
// sum x z_j, the (1, z) Gram and its corrections; each adds sum x y_p and the (1, y_p), (z_j, y_p), (y_p, y_p) entries.
// Every per-phenotype number of a variant is one thread's sequential FMA chain over the samples in order, so it does
// not depend on the phenotype tile, the other phenotypes or the variant chunk.
// ---------------------------------------------------------------------------

// sxy[v][p] = sum_i x_v(i) y_p(i): a GEMM of the chunk's genotype rows (nv x n_out) and the phenotype block
// (pb x n_out, phenotype-major, 0 where missing).  A workgroup owns TV variants x TP phenotypes and each thread an
// MV x MP register tile; both operands pass through LDS kXyS samples at a time (missing calls staged as 0).
constexpr int kXyS = 32;

template <int MV, int MP, int NTP>
__global__ void __launch_bounds__(kBlock) GlmMultiXyKernel(GlmX g, uint32_t nv, const double *__restrict__ yb,
                                                           uint32_t pb, double *__restrict__ sxy) {
	constexpr int NTV = kBlock / NTP;
	constexpr int TV = NTV * MV, TP = NTP * MP, S = kXyS;
	__shared__ double xs[S][TV];
	__shared__ double ys[S][TP];
	const uint32_t v0 = blockIdx.x * TV, p0 = blockIdx.y * TP;
	const int tv = threadIdx.x % NTV, tp = threadIdx.x / NTV;
	double acc[MV][MP];
#pragma unroll
	for (int a = 0; a < MV; a++) {
#pragma unroll
		for (int b = 0; b < MP; b++) {
			acc[a][b] = 0.0;
		}
	}
	for (uint32_t i0 = 0; i0 < g.n_out; i0 += S) {
		for (int e = threadIdx.x; e < TV * S; e += kBlock) {
			const int s = e % S, t = e / S;
			const uint32_t v = v0 + t, i = i0 + s;
			double x = 0.0;
			if (v < nv && i < g.n_out) {
				x = GlmValue(g, v, i);
				x = x == -9.0 ? 0.0 : x;
			}
			xs[s][t] = x;
		}
		for (int e = threadIdx.x; e < TP * S; e += kBlock) {
			const int s = e % S, t = e / S;
			const uint32_t p = p0 + t, i = i0 + s;
			ys[s][t] = p < pb && i < g.n_out ? yb[static_cast<uint64_t>(p) * g.n_out + i] : 0.0;
		}
		__syncthreads();
#pragma unroll 4
		for (int s = 0; s < S; s++) {
			double xr[MV], yr[MP];
#pragma unroll
			for (int a = 0; a < MV; a++) {
				xr[a] = xs[s][tv * MV + a];
			}
#pragma unroll
			for (int b = 0; b < MP; b++) {
				yr[b] = ys[s][tp * MP + b];
			}
#pragma unroll
			for (int a = 0; a < MV; a++) {
#pragma unroll
				for (int b = 0; b < MP; b++) {
					acc[a][b] = fma(xr[a], yr[b], acc[a][b]);
				}
			}
		}
		__syncthreads();
	}
#pragma unroll
	for (int a = 0; a < MV; a++) {
#pragma unroll
		for (int b = 0; b < MP; b++) {
			const uint32_t v = v0 + tv * MV + a, p = p0 + tp * MP + b;
			if (v < nv && p < pb) {
				sxy[static_cast<uint64_t>(v) * pb + p] = acc[a][b];
			}
		}
	}
}

// whole[p][0..k+1] = {sum y_p, sum z_j y_p (j < k), sum y_p^2} over every sample (y_p = 0 where missing); one
// workgroup per phenotype, BlockSums' fixed order.
template <int KP>
__global__ void __launch_bounds__(kBlock) GlmMultiWholeKernel(uint32_t n_out, const double *__restrict__ yb,
                                                              const double *__restrict__ z, uint32_t k,
                                                              double *__restrict__ whole) {
	constexpr int NE = KP + 2;
	__shared__ double lds[kWaves * NE];
	__shared__ double tile[NE];
	const uint32_t p = blockIdx.x;
	const double *y = yb + static_cast<uint64_t>(p) * n_out;
	double acc[NE];
#pragma unroll
	for (int e = 0; e < NE; e++) {
		acc[e] = 0.0;
	}
	for (uint32_t i = threadIdx.x; i < n_out; i += kBlock) {
		const double yi = y[i];
		acc[0] += yi;
#pragma unroll
		for (int j = 0; j < KP; j++) {
			acc[1 + j] += z[static_cast<uint64_t>(i) * KP + j] * yi;
		}
		acc[KP + 1] += yi * yi;
	}
	BlockSums<NE>(acc, lds, tile);
	__syncthreads();
	double *dst = whole + static_cast<uint64_t>(p) * (k + 2);
	for (uint32_t e = threadIdx.x; e < k + 2; e += kBlock) {
		dst[e] = tile[e <= k ? e : KP + 1];
	}
}

// The missing-call corrections of one variant per workgroup, over its samples with a phenotype (the group's
// pattern: ypat is NaN where it is missing) and no value: corr_s[v] = the packed Gram of [1, z] ((k+1)(k+2)/2
// entries), corr_p[v][p][0..k+1] = {sum y_p, sum z_j y_p, sum y_p^2}.  The compacted list of those samples
// (GlmGramKernel's, per 256-sample chunk, in sample order) is contracted against the phenotype block kYSub list
// entries at a time; a thread owns up to kCorrRegs (phenotype, entry) pairs in registers.  Variants with no such
// sample (sums[v][0] == n_y) write zeros.
constexpr int kYSub = 16;
constexpr int kCorrRegs = (kGlmMultiPb * kMaxP + kBlock - 1) / kBlock;

__global__ void __launch_bounds__(kBlock) GlmMultiCorrKernel(GlmX g, const double *__restrict__ sums, uint32_t ns,
                                                             uint32_t n_y, const double *__restrict__ ypat,
                                                             const double *__restrict__ yb, uint32_t pb,
                                                             const double *__restrict__ z, uint32_t kp, uint32_t k,
                                                             double *__restrict__ corr_s, double *__restrict__ corr_p) {
	const uint32_t qs = k + 1, nes = qs * (qs + 1) / 2, qp = k + 2, nep = pb * qp;
	const uint32_t v = blockIdx.x;
	double *ds = corr_s + static_cast<uint64_t>(v) * nes;
	double *dp = corr_p + static_cast<uint64_t>(v) * nep;
	if (sums[static_cast<uint64_t>(v) * ns] == static_cast<double>(n_y)) {
		for (uint32_t e = threadIdx.x; e < nes; e += kBlock) {
			ds[e] = 0.0;
		}
		for (uint32_t e = threadIdx.x; e < nep; e += kBlock) {
			dp[e] = 0.0;
		}
		return;
	}
	extern __shared__ double lz[]; // kBlock list rows [1, z_1..z_k] (sized at launch)
	__shared__ uint32_t lidx[kBlock];
	__shared__ double ysub[kYSub * kGlmMultiPb];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int ea = -1, eb = -1;
	if (threadIdx.x < nes) {
		PackedUpper(threadIdx.x, qs, &ea, &eb);
	}
	double acc_s = 0.0;
	double acc_p[kCorrRegs];
#pragma unroll
	for (int r = 0; r < kCorrRegs; r++) {
		acc_p[r] = 0.0;
	}
	for (uint32_t c0 = 0; c0 < g.n_out; c0 += kBlock) {
		const uint32_t i = c0 + threadIdx.x;
		bool take = false;
		if (i < g.n_out) {
			const double yi = ypat[i];
			take = yi == yi && GlmValue(g, v, i) == -9.0;
		}
		// the ordered-list step (TeamRank in glm_team.hpp)
		uint32_t total;
		const uint32_t pos = TeamRank<kBlock>(take, lane, wave, &total);
		if (take) {
			double *r = lz + pos * qs;
			r[0] = 1.0;
			for (uint32_t j = 0; j < k; j++) {
				r[1 + j] = z[static_cast<uint64_t>(i) * kp + j];
			}
			lidx[pos] = i;
		}
		__syncthreads();
		// total is the same in every thread: the loop below and its barriers are uniform
		if (ea >= 0) {
			for (uint32_t s = 0; s < total; s++) {
				acc_s += lz[s * qs + ea] * lz[s * qs + eb];
			}
		}
		for (uint32_t b0 = 0; b0 < total; b0 += kYSub) {
			const uint32_t nb = min(total - b0, static_cast<uint32_t>(kYSub));
			for (uint32_t e = threadIdx.x; e < nb * pb; e += kBlock) {
				const uint32_t s = e / pb, p = e % pb;
				ysub[s * kGlmMultiPb + p] = yb[static_cast<uint64_t>(p) * g.n_out + lidx[b0 + s]];
			}
			__syncthreads();
#pragma unroll
			for (int r = 0; r < kCorrRegs; r++) {
				const uint32_t e = threadIdx.x + r * kBlock;
				if (e < nep) {
					const uint32_t p = e / qp, j = e % qp;
					double a = acc_p[r];
					for (uint32_t s = 0; s < nb; s++) {
						const double yv = ysub[s * kGlmMultiPb + p];
						const double u = j == 0 ? 1.0 : j <= k ? lz[(b0 + s) * qs + j] : yv;
						a = fma(u, yv, a);
					}
					acc_p[r] = a;
				}
			}
			__syncthreads();
		}
	}
	if (ea >= 0) {
		ds[threadIdx.x] = acc_s;
	}
#pragma unroll
	for (int r = 0; r < kCorrRegs; r++) {
		const uint32_t e = threadIdx.x + r * kBlock;
		if (e < nep) {
			dp[e] = acc_p[r];
		}
	}
}

// The OLS of (variant, phenotype) pairs, one thread each: GlmLinearSolveKernel's augmented Cholesky in the order [1,
// z, x, y_p], with the (1, z) block from the group's Gram and correction and the y_p entries from whole and corr_p.
__global__ void GlmMultiSolveKernel(uint32_t nv, uint32_t pb, const double *__restrict__ sums, uint32_t kp, uint32_t k,
                                    const double *__restrict__ sxy, const double *__restrict__ gram,
                                    const double *__restrict__ whole, const double *__restrict__ corr_s,
                                    const double *__restrict__ corr_p, pgh_glm_row *__restrict__ rows) {
	const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (t >= static_cast<uint64_t>(nv) * pb) {
		return;
	}
	const uint32_t v = static_cast<uint32_t>(t / pb), ph = static_cast<uint32_t>(t % pb);
	const uint32_t ns = kp + 4, q = k + 2, qs = k + 1, nes = qs * (qs + 1) / 2;
	const double *s = sums + static_cast<uint64_t>(v) * ns;
	const double *cs = corr_s + static_cast<uint64_t>(v) * nes;
	const double *cp = corr_p + t * q;
	const double *wp = whole + static_cast<uint64_t>(ph) * q;
	pgh_glm_row r;
	SetRowNull(r);
	const double n = s[0];
	const int p = static_cast<int>(k) + 2;
	r.obs_ct = static_cast<uint32_t>(n);
	if (n < p + 1) {
		r.errcode = PGH_GLM_TOO_FEW_SAMPLES;
		rows[t] = r;
		return;
	}
	r.a1_freq = s[1] / (2.0 * n);
	if (k ? GlmConstant(n, s[1], s[2]) : s[2] - s[1] * s[1] / n < 1e-20) {
		r.errcode = PGH_GLM_CONST_ALLELE;
		rows[t] = r;
		return;
	}
	// augmented matrix, order [1, z_1..z_k, x, y], lower triangle
	constexpr int M = kMaxP + 1;
	double a[M * M];
	const int xi = p - 1, yi = p;
	for (int ua = 0; ua < static_cast<int>(qs); ua++) {
		for (int ub = ua; ub < static_cast<int>(qs); ub++) {
			a[ub * M + ua] = gram[PackIdx(ua, ub, q)] - cs[PackIdx(ua, ub, qs)];
		}
		a[yi * M + ua] = wp[ua] - cp[ua];
	}
	a[yi * M + yi] = wp[k + 1] - cp[k + 1];
	a[xi * M + 0] = s[1];
	for (int j = 0; j < static_cast<int>(k); j++) {
		a[xi * M + 1 + j] = s[4 + j];
	}
	a[xi * M + xi] = s[2];
	a[yi * M + xi] = sxy[t];
	if (!GlmCholesky(a, p, M, k ? 1e-10 : 0.0, nullptr)) {
		r.errcode = PGH_GLM_SINGULAR_MATRIX;
		rows[t] = r;
		return;
	}
	double rss = a[yi * M + yi];
	for (int j = 0; j < p; j++) {
		double l = a[yi * M + j];
		for (int c = 0; c < j; c++) {
			l -= a[yi * M + c] * a[j * M + c];
		}
		l /= a[j * M + j];
		a[yi * M + j] = l;
		rss -= l * l;
	}
	rss = rss < 0.0 ? 0.0 : rss;
	const double lxx = a[xi * M + xi];
	const double df = n - p;
	const double se2 = rss / df / (lxx * lxx);
	const double beta = a[yi * M + xi] / lxx;
	r.beta = beta;
	if (se2 < 1e-30) {
		r.errcode = PGH_GLM_ZERO_VARIANCE;
		rows[t] = r;
		return;
	}
	r.se = sqrt(se2);
	r.stat = beta / r.se;
	r.p = GlmPFromT(r.stat, df);
	rows[t] = r;
}

uint32_t Blocks(uint32_t n, uint32_t per) {
	return (n + per - 1) / per;
}

} // namespace

uint32_t GlmPadCovar(uint32_t k) {
	for (uint32_t w : kGlmWidths) {
		if (k <= w) {
			return w;
		}
	}
	return 0xffffffffu;
}

hipError_t LaunchGlmSums(const GlmX &g, uint32_t nv, const double *y, const double *z, uint32_t kp, double *sums,
                         hipStream_t stream) {
	if (nv == 0) {
		return hipSuccess;
	}
	return GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value, T = GlmSumsTile(KP);
		GlmSumsKernel<KP, T><<<Blocks(nv, T), kBlock, 0, stream>>>(g, nv, y, z, sums);
	});
}

hipError_t LaunchGlmGram(const GlmX *g, uint32_t nv, const double *sums, uint32_t sums_stride, uint32_t n_y,
                         uint32_t n_out, const double *y, const double *z, uint32_t kp, uint32_t k, double *out,
                         hipStream_t stream) {
	if (k > 20) {
		return hipErrorInvalidValue;
	}
	if (g && nv == 0) {
		return hipSuccess;
	}
	GlmX none {};
	GlmGramKernel<<<g ? nv : 1u, kBlock, sizeof(double) * kBlock * (k + 2), stream>>>(g ? *g : none, g ? 1 : 0, sums, sums_stride, n_y, n_out, y, z,
	                                                  kp, k, out);
	return hipGetLastError();
}

hipError_t LaunchGlmLinearSolve(uint32_t nv, const double *sums, uint32_t kp, uint32_t k, const double *gram,
                                const double *corr, pgh_glm_row *rows, hipStream_t stream, const uint8_t *x_const) {
	if (nv == 0) {
		return hipSuccess;
	}
	if (x_const) {
		GlmLinearSolveKernel<true><<<Blocks(nv, 64), 64, 0, stream>>>(nv, sums, kp, k, gram, nullptr, x_const, rows);
	} else {
		GlmLinearSolveKernel<false><<<Blocks(nv, 64), 64, 0, stream>>>(nv, sums, kp, k, gram, corr, nullptr, rows);
	}
	return hipGetLastError();
}

hipError_t LaunchGlmLogisticInit(uint32_t nv, const double *sums, uint32_t kp, uint32_t k, GlmState *st, double *beta,
                                 pgh_glm_row *rows, hipStream_t stream) {
	if (nv == 0) {
		return hipSuccess;
	}
	GlmLogisticInitKernel<<<Blocks(nv, 64), 64, 0, stream>>>(nv, sums, 0, kp, k, st, beta, rows);
	return hipGetLastError();
}

hipError_t LaunchGlmIrlsAcc(int mode, const GlmX &g, const uint32_t *list, uint32_t n, const double *y, const double *z,
                            uint32_t kp, const GlmState *st, const double *beta, const double *hinv0, double *acc,
                            hipStream_t stream) {
	if (n == 0) {
		return hipSuccess;
	}
	return GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value;
		if (mode == 0) {
			GlmIrlsAccKernel<KP, 0><<<n, kBlock, 0, stream>>>(g, list, y, z, st, beta, hinv0, acc);
		} else if (mode == 1) {
			GlmIrlsAccKernel<KP, 1><<<n, kBlock, 0, stream>>>(g, list, y, z, st, beta, hinv0, acc);
		} else {
			GlmIrlsAccKernel<KP, 2><<<n, kBlock, 0, stream>>>(g, list, y, z, st, beta, hinv0, acc);
		}
	});
}

hipError_t LaunchGlmNewtonUpdate(uint32_t nv, uint32_t kp, uint32_t k, const double *acc, GlmState *st, double *beta,
                                 double *hmat, hipStream_t stream) {
	if (nv == 0) {
		return hipSuccess;
	}
	GlmNewtonUpdateKernel<<<Blocks(nv, 64), 64, 0, stream>>>(nv, kp, k, acc, st, beta, hmat);
	return hipGetLastError();
}

hipError_t LaunchGlmFirthStart(const uint32_t *list, uint32_t n, uint32_t kp, GlmState *st, double *beta,
                               hipStream_t stream) {
	if (n == 0) {
		return hipSuccess;
	}
	GlmFirthStartKernel<<<Blocks(n, 64), 64, 0, stream>>>(list, n, kp, st, beta);
	return hipGetLastError();
}

hipError_t LaunchGlmFirthUpdate(int half, const uint32_t *list, uint32_t n, uint32_t kp, uint32_t k, const double *acc,
                                GlmState *st, double *beta, double *hinv0, double *hmat, hipStream_t stream) {
	if (n == 0) {
		return hipSuccess;
	}
	GlmFirthUpdateKernel<<<Blocks(n, 64), 64, 0, stream>>>(half, list, n, kp, k, acc, st, beta, hinv0, hmat);
	return hipGetLastError();
}

hipError_t LaunchGlmLogisticFinish(uint32_t nv, uint32_t kp, uint32_t k, const GlmState *st,
                                   const double *beta, const double *hmat, pgh_glm_row *rows, hipStream_t stream) {
	if (nv == 0) {
		return hipSuccess;
	}
	GlmLogisticFinishKernel<<<Blocks(nv, 64), 64, 0, stream>>>(nv, kp, k, st, beta, hmat, rows);
	return hipGetLastError();
}

hipError_t LaunchGlmMultiXy(const GlmX &g, uint32_t nv, const double *yb, uint32_t pb, double *sxy,
                            hipStream_t stream) {
	if (nv == 0 || pb == 0) {
		return hipSuccess;
	}
	if (pb > kGlmMultiPb) {
		return hipErrorInvalidValue;
	}
	// 64 variants x 8 phenotypes (2 x 1 per thread) for small blocks, 64 x 64 (4 x 4) otherwise
	if (pb <= 8) {
		GlmMultiXyKernel<2, 1, 8><<<dim3(Blocks(nv, 64), 1), kBlock, 0, stream>>>(g, nv, yb, pb, sxy);
	} else {
		GlmMultiXyKernel<4, 4, 16><<<dim3(Blocks(nv, 64), 1), kBlock, 0, stream>>>(g, nv, yb, pb, sxy);
	}
	return hipGetLastError();
}

hipError_t LaunchGlmMultiWhole(uint32_t n_out, const double *yb, uint32_t pb, const double *z, uint32_t kp,
                               uint32_t k, double *whole, hipStream_t stream) {
	if (pb == 0) {
		return hipSuccess;
	}
	if (k > kp) {
		return hipErrorInvalidValue;
	}
	return GlmForWidth(kp, [&](auto width) {
		GlmMultiWholeKernel<decltype(width)::value><<<pb, kBlock, 0, stream>>>(n_out, yb, z, k, whole);
	});
}

hipError_t LaunchGlmMultiCorr(const GlmX &g, uint32_t nv, const double *sums, uint32_t n_y, const double *ypat,
                              const double *yb, uint32_t pb, const double *z, uint32_t kp, uint32_t k, double *corr_s,
                              double *corr_p, hipStream_t stream) {
	if (nv == 0) {
		return hipSuccess;
	}
	if (pb > kGlmMultiPb || k > 20 || k > kp) {
		return hipErrorInvalidValue;
	}
	GlmMultiCorrKernel<<<nv, kBlock, sizeof(double) * kBlock * (k + 1), stream>>>(g, sums, kp + 4, n_y, ypat, yb, pb, z,
	                                                                              kp, k, corr_s, corr_p);
	return hipGetLastError();
}

hipError_t LaunchGlmMultiSolve(uint32_t nv, uint32_t pb, const double *sums, uint32_t kp, uint32_t k,
                               const double *sxy, const double *gram, const double *whole, const double *corr_s,
                               const double *corr_p, pgh_glm_row *rows, hipStream_t stream) {
	const uint64_t n = static_cast<uint64_t>(nv) * pb;
	if (n == 0) {
		return hipSuccess;
	}
	if (k > 20 || n > 0xffffffffull - 64) {
		return hipErrorInvalidValue;
	}
	GlmMultiSolveKernel<<<Blocks(static_cast<uint32_t>(n), 64), 64, 0, stream>>>(nv, pb, sums, kp, k, sxy, gram, whole,
	                                                                            corr_s, corr_p, rows);
	return hipGetLastError();
}

} // namespace pgh
