// glm_score_sparse_multi.hip -- pgh_glm_score_sparse_multi: the logistic score test of every variant of a
// sparse-resident dataset (sparse.hpp) for a block of phenotypes in one walk of the entries (the launch wrappers are in
// glm.hpp).  The sums are those of glm_score_sparse.hip's header comment, per (row, phenotype).
//
// The pair block.  The null fits (LaunchGlmScoreNull, one per phenotype) leave r and w in raw-sample order; the scatter
// kernel writes them to pair[s][j] = (r, w), one double2 per (raw sample s, block phenotype j < pb), so that the pb
// pairs of a sample are contiguous.  r = NaN (w = 0): s is outside S_j or outside the subset; the block is cleared to
// that before its phenotypes write it.
//
// The entry kernel, lanes across phenotypes: the walk of glm_lanes.hpp, whose header comment has the order of the sums
// and the centring, with the score test's weights.  A lane keeps U0, A, c_0 .. c_KP and its integer counts, gated by
// r == r.
//
// The missing-call corrections H_N and g_N (GlmScoreSparseMultiCorrKernel): a workgroup per (row, tile of the packed
// {H, g} entries), the correction of glm_lanes.hpp over the [entries][pb] tile of (r, w), zero outside S_j.  A row
// without list entries copies hg.
#include "glm.hpp"
#include "glm_lanes.hpp"
#include "glm_math.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;

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

// The lane sums are U0, A, c_0, c_1 .. c_KP; sums[j][i][KP + 6] = {n, sum x, sum x^2, U0, A, c_0, c_1 .. c_KP} of the
// row i for the block phenotype j.
template <int KP>
struct ScoreLanes {
	using Value = double2; // (r, w)
	static constexpr int kNL = KP + 3;
	static __device__ __forceinline__ Value Outside() {
		return make_double2(NAN, 0.0);
	}
	static __device__ __forceinline__ bool Used(Value v) {
		return v.x == v.x;
	}
	static __device__ __forceinline__ void Add(double dd, Value v, const double *zi,
	                                           const double (&mzr)[KP > 0 ? KP : 1], double (&ls)[kNL]) {
		const double wd = v.y * dd;
		ls[0] = fma(dd, v.x, ls[0]);
		ls[1] = fma(wd, dd, ls[1]);
		ls[2] += wd;
#pragma unroll
		for (int t = 0; t < KP; t++) {
			ls[3 + t] = fma(wd, zi[t] - mzr[t], ls[3 + t]);
		}
	}
	static __device__ __forceinline__ uint64_t Row(uint32_t i, uint32_t nv, uint32_t pb, int j) {
		return static_cast<uint64_t>(j) * nv + i;
	}
};

// The two forms of LanesWalkSparseRow (glm_lanes.hpp).
template <int KP, int PBW, bool LONG>
__global__ void __launch_bounds__(kBlock) GlmScoreSparseMultiKernel(SparseRows rows, const double2 *__restrict__ pair,
                                                                    const double *__restrict__ z,
                                                                    const double *__restrict__ mz,
                                                                    const uint32_t *__restrict__ ny, uint32_t pb,
                                                                    double *__restrict__ sums,
                                                                    uint32_t *__restrict__ nlist) {
	extern __shared__ double part[]; // the workgroup form's (LaunchEntryForms)
	LanesWalkSparseRow<ScoreLanes<KP>, KP, PBW, LONG>(rows, pair, z, mz, ny, pb, sums, nlist, part);
}

// ---------------------------------------------------------------------------
// the missing-call corrections
// ---------------------------------------------------------------------------

// The tile holds (r, w), exact zeros outside S_pp so that they join its sums; an owner's entry of the packed {H, g}
// set (ScoreOwnedEntry) adds w Zt_a Zt_b or r Zt_a, Zt the list row centred on the phenotype's means (Zt_0 = 1 is
// not); hgn[pp][i] = H_N then g_N, packed as hg: hg - the sums, or the sums themselves under base 3.
struct ScoreCorr {
	using Value = double2;
	const double2 *pair;
	const double *hg;
	double *hgn;
	uint32_t pb, nv, ne;

	struct Own {
		int a, b;
		bool is_h;
		double ma, mb;
	};
	static __host__ __device__ __forceinline__ uint32_t Entries(uint32_t k) {
		return (k + 1) * (k + 2) / 2 + k + 1;
	}
	__device__ __forceinline__ Value Stage(uint32_t s, uint32_t pp) const {
		Value v = make_double2(0.0, 0.0);
		if (pp < pb) {
			v = pair[static_cast<uint64_t>(s) * pb + pp];
			if (v.x != v.x) {
				v = make_double2(0.0, 0.0);
			}
		}
		return v;
	}
	__device__ __forceinline__ void OwnedEntry(int e, int k, bool have, const double *mz, Own *o) const {
		int ew;
		ScoreOwnedEntry(e, k, &o->a, &o->b, &ew);
		if (!have) {
			o->a = -1;
		}
		o->is_h = ew == k + 1;
		o->ma = o->a > 0 ? mz[o->a - 1] : 0.0;
		o->mb = o->a >= 0 && o->b > 0 ? mz[o->b - 1] : 0.0;
	}
	__device__ __forceinline__ double Term(Value v, const double *row, const Own &o, double acc) const {
		const double za = row[o.a] - o.ma, zb = row[o.b] - o.mb;
		return fma((o.is_h ? v.y : v.x) * za, zb, acc);
	}
	__device__ __forceinline__ void Store(uint32_t i, uint32_t pp, uint32_t e, double v, bool base3) const {
		hgn[(static_cast<uint64_t>(pp) * nv + i) * ne + e] = base3 ? v : hg[static_cast<uint64_t>(pp) * ne + e] - v;
	}
};

// Workgroup (i, tile): the row i and the entries tile * ET .. of the packed {H, g} set, ET = kBlock * kCorrOwn / PBW.
template <int PBW>
__global__ void __launch_bounds__(kBlock) GlmScoreSparseMultiCorrKernel(SparseRows rows, const double2 *__restrict__ pair,
                                                                        const double *__restrict__ z, uint32_t kp,
                                                                        uint32_t k, const double *__restrict__ mz,
                                                                        uint32_t pb, const double *__restrict__ hg,
                                                                        const uint32_t *__restrict__ nlist,
                                                                        double *__restrict__ hgn) {
	extern __shared__ __attribute__((aligned(16))) double lds[]; // (LanesCorrectLds)
	const uint32_t ne = ScoreCorr::Entries(k);
	const uint32_t i = blockIdx.x, tile = blockIdx.y;
	if (nlist[i] == 0u) {
		// no list entry: H_N = H and g_N = g_S (zeros under base 3); the first tile's workgroup writes the whole row
		if (tile == 0u) {
			const bool base3 = rows.row_of[rows.v_first + i] == -4;
			for (uint32_t at = threadIdx.x; at < pb * ne; at += kBlock) {
				const uint32_t p = at / ne, e = at - p * ne;
				hgn[(static_cast<uint64_t>(p) * rows.nv + i) * ne + e] = base3 ? 0.0 : hg[at];
			}
		}
		return;
	}
	const ScoreCorr m = {pair, hg, hgn, pb, rows.nv, ne};
	LanesCorrectRow<ScoreCorr, PBW>(rows, i, tile, z, kp, k, mz, m, lds);
}

template <int PBW>
void LaunchCorr(const SparseRows &rows, const double2 *pair, const double *z, uint32_t kp, uint32_t k, const double *mz,
                uint32_t pb, const double *hg, const uint32_t *nlist, double *hgn, hipStream_t stream) {
	const uint32_t ne = ScoreCorr::Entries(k), et = kBlock * kCorrOwn / PBW;
	const size_t lds = LanesCorrectLds<ScoreCorr, PBW>(k);
	GlmScoreSparseMultiCorrKernel<PBW><<<dim3(rows.nv, (ne + et - 1) / et), kBlock, lds, stream>>>(rows, pair, z, kp, k, mz,
	                                                                                               pb, hg, nlist, hgn);
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
			LaunchEntryForms<ScoreLanes<KP>::kNL, PBW>(nv, [&](auto lanes, auto form, uint32_t grid, size_t lds) {
				GlmScoreSparseMultiKernel<KP, decltype(lanes)::value, decltype(form)::value>
				    <<<grid, kBlock, lds, stream>>>(rows, pr, z0, mz, n_y, pb, sums, nlist);
			});
			LaunchCorr<PBW>(rows, pr, z0, kp, k, mz, pb, hg, nlist, hgn, stream);
		});
	});
}

} // namespace pgh
