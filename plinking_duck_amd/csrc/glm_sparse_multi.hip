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
// The entry kernel, lanes across phenotypes: the walk of glm_lanes.hpp, whose header comment has the order of the sums
// and the centring, with the linear model's weights.  A lane keeps sum_C d y_j, sum_C d (z_t - mz_j,t) (d = x - b) and
// its integer counts, gated by yv == yv.
//
// The missing-call corrections corr_j (GlmSparseMultiCorrKernel): the Gram of u over the row's list set (its code-3
// entries, or every entry of a base-3 row, where corr_j = G_j - that Gram) intersected with S_j, the correction of
// glm_lanes.hpp over the [entries][pb] tile of yv.  A row without list entries is not written: the solve reads G_j for
// it (nlist[i] == 0).
//
// The solve (GlmSparseMultiSolveKernel): one thread per (row, block phenotype).  It puts the sums back into pgh_glm's
// parameterisation, sum_N x u = b (G_j - corr_j)(1, u) + sum_C d u, and runs GlmLinearSolveRow (glm_linear_solve.hpp),
// the device function of GlmLinearSolveKernel.  The rows are written variant-major, rows[i][j].
#include "glm.hpp"
#include "glm_lanes.hpp"
#include "glm_linear_solve.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;
constexpr uint32_t kCorrGroups = 2048; // workgroups of the correction kernel's grid per tile of entries, at most

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

// The lane sums are sum_C d y and sum_C d (z_t - mz_t); sums[i][j][KP + 4] = {n, sum x, sum x^2, sum_C d y,
// sum_C d zc_t}: the first three final, the others the entry sums that the solve puts back into the raw
// parameterisation.
template <int KP>
struct LinearLanes {
	using Value = double; // yv
	static constexpr int kNL = KP + 1;
	static __device__ __forceinline__ Value Outside() {
		return NAN;
	}
	static __device__ __forceinline__ bool Used(Value y) {
		return y == y;
	}
	static __device__ __forceinline__ void Add(double dd, Value y, const double *zi, const double (&mzr)[KP > 0 ? KP : 1],
	                                           double (&ls)[kNL]) {
		ls[0] = fma(dd, y, ls[0]);
#pragma unroll
		for (int t = 0; t < KP; t++) {
			ls[1 + t] = fma(dd, zi[t] - mzr[t], ls[1 + t]);
		}
	}
	static __device__ __forceinline__ uint64_t Row(uint32_t i, uint32_t nv, uint32_t pb, int j) {
		return static_cast<uint64_t>(i) * pb + j;
	}
};

// The two forms of LanesWalkSparseRow (glm_lanes.hpp).
template <int KP, int PBW, bool LONG>
__global__ void __launch_bounds__(kBlock) GlmSparseMultiKernel(SparseRows rows, const double *__restrict__ yv,
                                                               const double *__restrict__ z,
                                                               const double *__restrict__ mz,
                                                               const uint32_t *__restrict__ ny, uint32_t pb,
                                                               double *__restrict__ sums,
                                                               uint32_t *__restrict__ nlist) {
	extern __shared__ double part[]; // the workgroup form's (LaunchEntryForms)
	LanesWalkSparseRow<LinearLanes<KP>, KP, PBW, LONG>(rows, yv, z, mz, ny, pb, sums, nlist, part);
}

// ---------------------------------------------------------------------------
// the missing-call corrections
// ---------------------------------------------------------------------------

// The tile holds yv, NaN outside S_pp and past pb: such a list row adds nothing; an owner's entry of the packed upper
// Gram of u = [1, z - mz, yv] adds u_a u_b (u_0 = 1 and yv are not centred here); corr[i][pp] = the sums, or G_pp - the
// sums under base 3.
struct LinearCorr {
	using Value = double;
	const double *yv, *gram;
	double *corr;
	uint32_t pb, ne;

	struct Own {
		int a, b;
		bool a_y, b_y;
		double ma, mb;
	};
	static __host__ __device__ __forceinline__ uint32_t Entries(uint32_t k) {
		return (k + 2) * (k + 3) / 2;
	}
	__device__ __forceinline__ Value Stage(uint32_t s, uint32_t pp) const {
		return pp < pb ? yv[static_cast<uint64_t>(s) * pb + pp] : NAN;
	}
	__device__ __forceinline__ void OwnedEntry(int e, int k, bool have, const double *mz, Own *o) const {
		o->a = o->b = -1;
		if (have) {
			PackedUpper(e, k + 2, &o->a, &o->b);
		}
		o->a_y = o->a == k + 1;
		o->b_y = o->b == k + 1;
		o->ma = o->a > 0 && o->a <= k ? mz[o->a - 1] : 0.0;
		o->mb = o->b > 0 && o->b <= k ? mz[o->b - 1] : 0.0;
	}
	__device__ __forceinline__ double Term(Value v, const double *row, const Own &o, double acc) const {
		if (v == v) { // in S_p
			const double ua = o.a_y ? v : row[o.a] - o.ma;
			const double ub = o.b_y ? v : row[o.b] - o.mb;
			acc = fma(ua, ub, acc);
		}
		return acc;
	}
	__device__ __forceinline__ void Store(uint32_t i, uint32_t pp, uint32_t e, double v, bool base3) const {
		corr[(static_cast<uint64_t>(i) * pb + pp) * ne + e] = base3 ? gram[static_cast<uint64_t>(pp) * ne + e] - v : v;
	}
};

// Workgroup (x, tile): the rows x, x + gridDim.x, .. that have list entries, and of each the entries tile * ET .. of the
// packed Gram, ET = kBlock * kCorrOwn / PBW.  Most rows of a rare-variant file have no list entry, and a workgroup per
// row that only finds that out costs more than the rows that have one: the grid is kCorrGroups wide instead.
template <int PBW>
__global__ void __launch_bounds__(kBlock) GlmSparseMultiCorrKernel(SparseRows rows, const double *__restrict__ yv,
                                                                   const double *__restrict__ z, uint32_t kp,
                                                                   uint32_t k, const double *__restrict__ mz,
                                                                   uint32_t pb, const double *__restrict__ gram,
                                                                   const uint32_t *__restrict__ nlist,
                                                                   double *__restrict__ corr) {
	extern __shared__ __attribute__((aligned(16))) double lds[]; // (LanesCorrectLds)
	const LinearCorr m = {yv, gram, corr, pb, LinearCorr::Entries(k)};
	for (uint32_t i = blockIdx.x; i < rows.nv; i += gridDim.x) {
		if (nlist[i] == 0u) {
			continue; // no list entry: the solve reads G_j (the whole workgroup)
		}
		LanesCorrectRow<LinearCorr, PBW>(rows, i, blockIdx.y, z, kp, k, mz, m, lds);
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

template <int PBW>
void LaunchCorr(const SparseRows &rows, const double *yv, const double *z, uint32_t kp, uint32_t k, const double *mz,
                uint32_t pb, const double *gram, const uint32_t *nlist, double *corr, hipStream_t stream) {
	const uint32_t ne = LinearCorr::Entries(k), et = kBlock * kCorrOwn / PBW;
	const size_t lds = LanesCorrectLds<LinearCorr, PBW>(k);
	const uint32_t groups = rows.nv < kCorrGroups ? rows.nv : kCorrGroups;
	GlmSparseMultiCorrKernel<PBW><<<dim3(groups, (ne + et - 1) / et), kBlock, lds, stream>>>(rows, yv, z, kp, k, mz, pb,
	                                                                                          gram, nlist, corr);
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
			LaunchEntryForms<LinearLanes<KP>::kNL, PBW>(nv, [&](auto lanes, auto form, uint32_t grid, size_t lds) {
				GlmSparseMultiKernel<KP, decltype(lanes)::value, decltype(form)::value>
				    <<<grid, kBlock, lds, stream>>>(rows, yv, z, mz, n_y, pb, sums, nlist);
			});
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
