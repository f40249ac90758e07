// glm_sparse.hip -- pgh_glm_sparse: the sums and the correction Gram of pgh_glm's linear fit for the sparse rows of a
// sparse-resident dataset (sparse.hpp), from the rows' entries alone (LaunchGlmSparse in glm.hpp).
//
// A row is a base code b and the entries that differ from it.  With S the samples that have a phenotype, G the
// whole-call Gram of u = [1, z, y] over S and, of the entries whose sample is in S, M those with code 3 and C the
// others:
//   b in {0, 1, 2}: n = n_y - |M|, sum x = b n + sum_C (x - b), sum x^2 = b^2 n + sum_C (x^2 - b^2),
//                   sum x u_j = b (G - corr)(1, u_j) + sum_C (x - b) u_j,   corr = Gram of u over M;
//   b == 3:         n = |C|, every x sum runs over C itself,                corr = G - Gram of u over C.
// n, sum x and sum x^2 are integers until they are stored, so they equal the dense kernel's sums bit for bit.
//
// The walk of a row, its teams, its ordered list and its reductions are TeamWalkSparseRow's (glm_team.hpp); this file
// holds the linear model's arithmetic.  y and z are staged in raw-sample order (NaN y: no phenotype or outside the
// subset), so an entry's sample addresses them.  Nothing depends on which rows share a workgroup, on the chunk or on
// where the range starts.
#include "glm.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

namespace pgh {

namespace {

// The list rows are u = [1, z, y]; the lane sums are sum_C d y and sum_C d z_j; an owner's entry (a, b) of the packed
// upper Gram adds u_a u_b.  A dense-form row is written as zeros: its result row comes from the dense kernels.
template <int KP>
struct LinearModel {
	static constexpr int kNS = KP + 4; // LaunchGlmSums' row
	static constexpr int kNL = KP + 1;
	static constexpr int kTail = 1;
	static constexpr bool kWalksDense = false;
	const double *y, *gram;
	double *sums, *corr;

	struct Sample {
		double y;
	};
	struct Own {
		int a, b;
	};
	static __device__ __forceinline__ uint32_t Entries(uint32_t k) {
		return (k + 2) * (k + 3) / 2;
	}
	__device__ __forceinline__ bool Load(uint32_t s, Sample *v) const {
		v->y = y[s];
		return v->y == v->y;
	}
	__device__ __forceinline__ void Add(double dd, const Sample &v, const double *zi, double (&ls)[kNL]) const {
		ls[0] = fma(dd, v.y, ls[0]);
#pragma unroll
		for (int j = 0; j < KP; j++) {
			ls[1 + j] = fma(dd, zi[j], ls[1 + j]);
		}
	}
	__device__ __forceinline__ void Tail(const Sample &v, double *tail) const {
		tail[0] = v.y;
	}
	__device__ __forceinline__ Own OwnedEntry(int e, int k) const {
		Own o = {-1, -1};
		if (e < static_cast<int>(Entries(k))) {
			PackedUpper(e, k + 2, &o.a, &o.b);
		}
		return o;
	}
	__device__ __forceinline__ double Term(const double *list, uint32_t row, const Own &o) const {
		return list[row + o.a] * list[row + o.b];
	}
	__device__ __forceinline__ void Zero(uint32_t i, int tid, uint32_t k) const {
		const uint32_t ne = Entries(k);
		for (uint32_t e = tid; e < kNS; e += 64) {
			sums[static_cast<uint64_t>(i) * kNS + e] = 0.0;
		}
		for (uint32_t e = tid; e < ne; e += 64) {
			corr[static_cast<uint64_t>(i) * ne + e] = 0.0;
		}
	}
	template <int TEAM, int NOWN>
	__device__ __forceinline__ void Epilogue(uint32_t i, int tid, uint32_t k, bool base3, int bx,
	                                         const double (&ls)[kNL], const Own (&own)[NOWN],
	                                         const double (&acc)[NOWN]) const {
		const uint32_t q = k + 2;
		double *s_out = sums + static_cast<uint64_t>(i) * kNS;
		double *c_out = corr + static_cast<uint64_t>(i) * Entries(k);
		if (tid == 0) {
			for (uint32_t j = k; j < KP; j++) {
				s_out[4 + j] = 0.0; // the padded columns, as LaunchGlmSums leaves them
			}
		}
#pragma unroll
		for (int t = 0; t < NOWN; t++) {
			if (own[t].a < 0) {
				continue;
			}
			const uint32_t e = static_cast<uint32_t>(tid + t * TEAM);
			const double c = base3 ? gram[e] - acc[t] : acc[t];
			c_out[e] = c;
			if (t == 0 && e >= 1 && e < q) {
				// entry (1, u_e) of the Gram: u_e = z_(e-1), or y at e == q - 1
				double sc = ls[0];
#pragma unroll
				for (int j = 0; j < KP; j++) {
					sc = (e < q - 1 && e == static_cast<uint32_t>(1 + j)) ? ls[1 + j] : sc;
				}
				const double v = bx ? static_cast<double>(bx) * (gram[e] - c) + sc : sc;
				s_out[e == q - 1 ? 3 : 3 + e] = v;
			}
		}
	}
};

// TEAM == 64 covers the rows of at most kGlmSparseLong entries (and the zeros of the dense-form rows), TEAM == 256 the
// longer ones.
template <int KP, int TEAM>
__global__ void __launch_bounds__(kTeamBlock) GlmSparseKernel(const int32_t *__restrict__ row_of,
                                                              const uint64_t *__restrict__ off,
                                                              const uint32_t *__restrict__ entries, uint32_t sample_ct,
                                                              uint32_t v_first, uint32_t nv,
                                                              const double *__restrict__ y,
                                                              const double *__restrict__ z, uint32_t k, uint32_t n_y,
                                                              const double *__restrict__ gram,
                                                              double *__restrict__ sums, double *__restrict__ corr) {
	extern __shared__ double lds[]; // kTeamBlock list rows of k + 2 doubles (sized at launch)
	const SparseRows rows = {row_of, off, entries, nullptr, 0, sample_ct, v_first, nv};
	const LinearModel<KP> m = {y, gram, sums, corr};
	TeamWalkSparseRow<LinearModel<KP>, KP, TEAM>(rows, z, k, n_y, m, lds);
}

} // namespace

hipError_t LaunchGlmSparse(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *y, const double *z,
                           uint32_t kp, uint32_t k, uint32_t n_y, const double *gram, double *sums, double *corr,
                           hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp) {
		return hipErrorInvalidValue;
	}
	if (nv == 0) {
		return hipSuccess;
	}
	const size_t lds = sizeof(double) * kTeamBlock * (k + 2);
	return GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value;
		GlmSparseKernel<KP, 64><<<(nv + kTeamWaves - 1) / kTeamWaves, kTeamBlock, lds, stream>>>(
		    sv.row_of, sv.off, sv.entries, sv.sample_ct, v_first, nv, y, z, k, n_y, gram, sums, corr);
		GlmSparseKernel<KP, kTeamBlock><<<nv, kTeamBlock, lds, stream>>>(sv.row_of, sv.off, sv.entries, sv.sample_ct,
		                                                                 v_first, nv, y, z, k, n_y, gram, sums, corr);
	});
}

} // namespace pgh
