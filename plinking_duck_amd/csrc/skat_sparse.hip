// skat_sparse.hip -- pgh_skat_sparse: per variant set, the cross-product sums of the members' score contributions under
// the logistic null model of pgh_glm_score_sparse, from the carrier entries of a sparse-resident dataset
// (LaunchSkatSparse in glm.hpp).  For the memberships j, l of a set, with d_ij = val(code) - val(base) at the entries
// of member j whose sample is in S (r not NaN) and 0 elsewhere, val(0, 1, 2, 3) = (0, 1, 2, 0):
//   U0_j = sum_i d_ij r_i    c_j = sum_i w_i d_ij Zt_i (KP + 1 values)    A_jl = sum_i w_i d_ij d_il  (j <= l)
// The weights of the set, the projection on the covariates, the eigenvalues and the p-values are the host's
// (SkatSparseOne in api_glm.cpp).
//
// One workgroup takes one set at a time, from an integer counter, and owns a private vector of one double and one
// count per raw sample, all zero between sets (burden_sparse.hip's shape, and its member walk: set_walk.hpp).
//   pass 1  the memberships in set order, a barrier after each: count[sample]++ (saturating at 255; a row's entries are
//           distinct samples, so the read-add-write never collides), and the member's own sums U0_j, c_j, A_jj.
//   pass 2  linked_j = some entry of member j has count >= 2: only such members can have A_jl != 0 for l != j.
//   pass 3  for each linked anchor j in set order: w_i d_ij of its entries with count >= 2 is scattered into the
//           vector, every linked l > j walks its entries and sums vector[sample] d_il, and a second walk of j clears
//           the vector.  The other off-diagonal entries are 0.
//   clear   the counts, by a last walk.
// Which lane meets which entry follows from the row alone; the lanes are reduced by a fixed butterfly and the waves in
// the order 0..3.  So a set's numbers do not depend on the other sets of the call, on the workgroup that took it or on
// how many workgroups there are, and there are no floating-point atomics.  Cost: sum_j E_j entries for the passes 1, 2
// and the clear, plus sum over the linked pairs j < l of E_l.
#include "device_utils.hpp"
#include "glm.hpp"
#include "set_walk.hpp"

#include <hip/hip_runtime.h>

namespace pgh {

namespace {

constexpr int kBlock = kSetBlock;
constexpr int kWaves = kBlock / 64;
static_assert(PGH_SKAT_MAX_SET <= kBlock, "one thread per member finishes a row of A");

// Index of (j, l), j <= l, in the row-major packed upper triangle of an m x m matrix.
__device__ __forceinline__ uint64_t SkatPacked(uint32_t j, uint32_t l, uint32_t m) {
	return static_cast<uint64_t>(j) * m - static_cast<uint64_t>(j) * (j + 1) / 2 + l;
}

template <int KP>
__global__ void __launch_bounds__(kBlock)
    SkatSparseKernel(const SparseView sv, uint32_t n_sets, const uint64_t *__restrict__ set_off,
                     const uint32_t *__restrict__ set_vidx, const double *__restrict__ r, const double *__restrict__ w,
                     const double *__restrict__ z, uint8_t *__restrict__ scratch, uint64_t per_group, uint64_t count_off,
                     uint32_t *__restrict__ counter, const uint64_t *__restrict__ out_off, double *__restrict__ out,
                     SkatSetCounts *__restrict__ counts) {
	constexpr int NC = KP + 1; // c_j: the intercept, then the covariates
	constexpr int NP = KP + 3; // U0, A_jj, c_j
	__shared__ uint32_t next_set;
	__shared__ double part[2][kWaves][NP];
	__shared__ double pair[kWaves][PGH_SKAT_MAX_SET];
	__shared__ uint32_t linked[PGH_SKAT_MAX_SET];
	__shared__ uint32_t ipart[kWaves][2];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint8_t *mine = scratch + static_cast<uint64_t>(blockIdx.x) * per_group;
	double *vec = reinterpret_cast<double *>(mine);
	uint8_t *count = mine + count_off;

	for (;;) {
		__syncthreads(); // the last set's reads of next_set and of the partials are done
		if (tid == 0) {
			next_set = atomicAdd(counter, 1u);
		}
		__syncthreads();
		const uint32_t s = next_set;
		if (s >= n_sets) {
			return; // (the whole workgroup)
		}
		const uint64_t m0 = set_off[s];
		const uint32_t m = static_cast<uint32_t>(set_off[s + 1] - m0);
		double *a_out = out + out_off[s];
		double *c_out = a_out + static_cast<uint64_t>(m) * (m + 1) / 2;
		double *u_out = c_out + static_cast<uint64_t>(m) * NC;
		linked[tid] = 0;

		// pass 1: the counts, and every member's own sums
		uint32_t carriers = 0, nonzero = 0;
		for (uint32_t j = 0; j < m; j++) {
			const uint32_t v = set_vidx[m0 + j];
			const int32_t ro = sv.row_of[v];
			double u0 = 0.0, ajj = 0.0, c[NC];
#pragma unroll
			for (int t = 0; t < NC; t++) {
				c[t] = 0.0;
			}
			WalkMember(sv, v, ro, SetMemberBase(ro), r, tid, [&](uint32_t smp, int diff, double ri) {
				const uint32_t seen = count[smp];
				count[smp] = static_cast<uint8_t>(seen < 255u ? seen + 1u : 255u);
				carriers += seen == 0u ? 1u : 0u;
				nonzero += diff != 0 ? 1u : 0u;
				const double d = static_cast<double>(diff), wd = w[smp] * d;
				u0 = fma(d, ri, u0);
				ajj = fma(wd, d, ajj);
				c[0] += wd;
#pragma unroll
				for (int t = 0; t < KP; t++) {
					c[1 + t] = fma(wd, z[static_cast<uint64_t>(smp) * KP + t], c[1 + t]);
				}
			});
			u0 = WaveSum(u0);
			ajj = WaveSum(ajj);
#pragma unroll
			for (int t = 0; t < NC; t++) {
				c[t] = WaveSum(c[t]);
			}
			double(*pt)[NP] = part[j & 1];
			if (lane == 0) {
				pt[wave][0] = u0;
				pt[wave][1] = ajj;
#pragma unroll
				for (int t = 0; t < NC; t++) {
					pt[wave][2 + t] = c[t];
				}
			}
			__syncthreads(); // the counts of member j are in place; its partials too (member j + 2 reuses the buffer)
			if (tid < NP) {
				double t = pt[0][tid];
				for (int wv = 1; wv < kWaves; wv++) {
					t += pt[wv][tid];
				}
				double *dst = tid == 0 ? u_out + j : tid == 1 ? a_out + SkatPacked(j, j, m) : c_out + static_cast<uint64_t>(j) * NC + (tid - 2);
				*dst = t;
			}
		}

		// pass 2: the members that share a carrier with another membership
		for (uint32_t j = 0; j < m; j++) {
			const uint32_t v = set_vidx[m0 + j];
			const int32_t ro = sv.row_of[v];
			bool shares = false;
			WalkMember(sv, v, ro, SetMemberBase(ro), r, tid, [&](uint32_t smp, int, double) { shares = shares || count[smp] >= 2; });
			if (shares) {
				linked[j] = 1; // (every writer stores the same value)
			}
		}
		carriers = WaveSum(carriers);
		nonzero = WaveSum(nonzero);
		if (lane == 0) {
			ipart[wave][0] = carriers;
			ipart[wave][1] = nonzero;
		}
		__syncthreads();
		if (tid == 0) {
			SkatSetCounts sc;
			sc.n_carriers = ipart[0][0] + ipart[1][0] + ipart[2][0] + ipart[3][0];
			sc.n_nonzero = ipart[0][1] + ipart[1][1] + ipart[2][1] + ipart[3][1];
			counts[s] = sc;
		}

		// pass 3: row j of A beyond the diagonal, one thread per column when it is written
		for (uint32_t j = 0; j + 1 < m; j++) {
			if (!linked[j]) {
				if (j + 1 + tid < m) {
					a_out[SkatPacked(j, j + 1 + tid, m)] = 0.0;
				}
				continue; // (the whole workgroup)
			}
			const uint32_t vj = set_vidx[m0 + j];
			const int32_t roj = sv.row_of[vj];
			const int vbj = SetMemberBase(roj);
			WalkMember(sv, vj, roj, vbj, r, tid, [&](uint32_t smp, int diff, double) {
				if (count[smp] >= 2) {
					vec[smp] = w[smp] * static_cast<double>(diff);
				}
			});
			__syncthreads(); // the anchor is scattered
			for (uint32_t l = j + 1; l < m; l++) {
				if (!linked[l]) {
					continue;
				}
				const uint32_t vl = set_vidx[m0 + l];
				const int32_t rol = sv.row_of[vl];
				double acc = 0.0;
				WalkMember(sv, vl, rol, SetMemberBase(rol), r, tid,
				           [&](uint32_t smp, int diff, double) { acc = fma(vec[smp], static_cast<double>(diff), acc); });
				acc = WaveSum(acc);
				if (lane == 0) {
					pair[wave][l] = acc;
				}
			}
			__syncthreads(); // every column's partials are written, and the reads of the vector are done
			if (j + 1 + tid < m) {
				const uint32_t l = j + 1 + tid;
				double t = 0.0;
				if (linked[l]) {
					t = pair[0][l];
					for (int wv = 1; wv < kWaves; wv++) {
						t += pair[wv][l];
					}
				}
				a_out[SkatPacked(j, l, m)] = t;
			}
			WalkMember(sv, vj, roj, vbj, r, tid, [&](uint32_t smp, int, double) { vec[smp] = 0.0; });
			__syncthreads(); // the vector is zero again and the partials are read
		}

		// the counts back to zero
		for (uint32_t j = 0; j < m; j++) {
			const uint32_t v = set_vidx[m0 + j];
			const int32_t ro = sv.row_of[v];
			WalkMember(sv, v, ro, SetMemberBase(ro), r, tid, [&](uint32_t smp, int, double) { count[smp] = 0; });
		}
	}
}

} // namespace

hipError_t LaunchSkatSparse(const SparseView &sv, uint32_t n_sets, const uint64_t *set_off, const uint32_t *set_vidx,
                            const double *r, const double *w, const double *z, uint32_t kp, uint32_t k,
                            uint32_t n_groups, void *scratch, uint32_t *counter, const uint64_t *out_off, double *out,
                            SkatSetCounts *counts, hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp || n_groups == 0) {
		return hipErrorInvalidValue;
	}
	if (n_sets == 0) {
		return hipSuccess;
	}
	const uint64_t per_group = BurdenScratchPerGroup(sv.sample_ct), count_off = per_group / 9 * 8;
	return GlmForWidth(kp, [&](auto width) {
		SkatSparseKernel<decltype(width)::value><<<n_groups, kBlock, 0, stream>>>(
		    sv, n_sets, set_off, set_vidx, r, w, z, static_cast<uint8_t *>(scratch), per_group, count_off, counter, out_off,
		    out, counts);
	});
}

} // namespace pgh
