// burden_sparse.hip -- pgh_burden_sparse: per variant set, the sums of the linear fit of y on the weighted burden
// B_i = c_s + d_i, from the carrier entries of a sparse-resident dataset (LaunchBurdenSparse in glm.hpp).
//
//   c_s = sum_m w_m val(b_m)                           the burden of a sample that differs from no member's base
//   d_i = sum_m w_m (val(code_i,m) - val(b_m))         over the memberships m at which sample i has an entry
// with val(0, 1, 2, 3) = (0, 1, 2, 0).  The intercept absorbs c_s, so the sums are taken over d.
//
// One workgroup takes one set at a time, from an integer counter, and owns a private vector of one double and one
// visited mark per raw sample, all zero between sets.
//   pass 1  the memberships in set order, a barrier after each; within a membership the lanes take the row's entries
//           at stride.  A row's entries are distinct samples, so the read-add-write of d[sample] never collides, and a
//           sample's adds happen in set order: d_i is a bit-defined function of the set.
//   pass 2  the same walk.  The first lane to meet a marked sample takes d, clears the value and the mark, and folds d
//           into its partial sums; later memberships find the mark cleared, so a sample counts once even when its d
//           cancelled to 0.0.
// Which lane folds a sample, and in which order a lane folds its samples, follows from the set's rows alone; the lanes
// are reduced by a fixed butterfly and the waves in the order 0..3.  So a set's numbers do not depend on the other sets
// of the call, on the workgroup that took it or on how many workgroups there are.  Entries whose staged y is NaN
// (outside the subset, or no phenotype) are skipped in both passes.  A dense-form member is read from its pool row as
// base 0 with one entry per sample whose code is 1 or 2, 16 samples per word per lane (WalkMember, set_walk.hpp).
#include "device_utils.hpp"
#include "glm.hpp"
#include "set_walk.hpp"

#include <hip/hip_runtime.h>

namespace pgh {

namespace {

constexpr int kBlock = kSetBlock;
constexpr int kWaves = kBlock / 64;

template <int KP>
__global__ void __launch_bounds__(kBlock)
    BurdenSparseKernel(const SparseView sv, uint32_t n_sets, const uint64_t *__restrict__ set_off,
                       const uint32_t *__restrict__ set_vidx, const double *__restrict__ weight,
                       const double *__restrict__ y, const double *__restrict__ z, uint32_t n_y,
                       uint8_t *__restrict__ scratch, uint64_t per_group, uint64_t mark_off,
                       uint32_t *__restrict__ counter, double *__restrict__ sums, BurdenAux *__restrict__ aux,
                       uint8_t *__restrict__ x_const) {
	constexpr int NS = KP + 4;
	constexpr int NP = KP + 5; // sum d, sum d^2, sum d y, sum d z_j, min, max
	__shared__ uint32_t next_set;
	__shared__ double part[kWaves][NP];
	__shared__ uint32_t ipart[kWaves][2];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint8_t *mine = scratch + static_cast<uint64_t>(blockIdx.x) * per_group;
	double *d = reinterpret_cast<double *>(mine);
	uint8_t *mark = mine + mark_off;

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
		const uint64_t m0 = set_off[s], m1 = set_off[s + 1];

		// pass 1: d and the marks, membership by membership
		double cs = 0.0;
		for (uint64_t m = m0; m < m1; m++) {
			const uint32_t v = set_vidx[m];
			const double w = weight ? weight[m] : 1.0;
			const int32_t ro = sv.row_of[v];
			const int vb = ro < 0 && ro != -4 ? -1 - ro : 0;
			cs += w * static_cast<double>(vb);
			WalkMember(sv, v, ro, vb, y, tid, [&](uint32_t smp, int diff, double) {
				d[smp] += w * static_cast<double>(diff);
				mark[smp] = 1;
			});
			__syncthreads();
		}

		// pass 2: every marked sample once, by the first membership that holds it
		uint32_t cnt = 0, nz = 0;
		double mn = INFINITY, mx = -INFINITY, sd = 0.0, sdd = 0.0, sdy = 0.0, sz[KP > 0 ? KP : 1];
#pragma unroll
		for (int j = 0; j < KP; j++) {
			sz[j] = 0.0;
		}
		for (uint64_t m = m0; m < m1; m++) {
			const uint32_t v = set_vidx[m];
			const int32_t ro = sv.row_of[v];
			const int vb = ro < 0 && ro != -4 ? -1 - ro : 0;
			WalkMember(sv, v, ro, vb, y, tid, [&](uint32_t smp, int, double yi) {
				if (mark[smp]) {
					const double di = d[smp];
					d[smp] = 0.0;
					mark[smp] = 0;
					cnt++;
					nz += di != 0.0 ? 1u : 0u;
					mn = fmin(mn, di);
					mx = fmax(mx, di);
					sd += di;
					sdd = fma(di, di, sdd);
					sdy = fma(di, yi, sdy);
#pragma unroll
					for (int j = 0; j < KP; j++) {
						sz[j] = fma(di, z[static_cast<uint64_t>(smp) * KP + j], sz[j]);
					}
				}
			});
			__syncthreads();
		}

		// lanes by butterfly, then the waves in order
		sd = WaveSum(sd);
		sdd = WaveSum(sdd);
		sdy = WaveSum(sdy);
#pragma unroll
		for (int j = 0; j < KP; j++) {
			sz[j] = WaveSum(sz[j]);
		}
		cnt = WaveSum(cnt);
		nz = WaveSum(nz);
		for (int o = 32; o >= 1; o >>= 1) {
			mn = fmin(mn, __shfl_xor(mn, o));
			mx = fmax(mx, __shfl_xor(mx, o));
		}
		if (lane == 0) {
			part[wave][0] = sd;
			part[wave][1] = sdd;
			part[wave][2] = sdy;
#pragma unroll
			for (int j = 0; j < KP; j++) {
				part[wave][3 + j] = sz[j];
			}
			part[wave][KP + 3] = mn;
			part[wave][KP + 4] = mx;
			ipart[wave][0] = cnt;
			ipart[wave][1] = nz;
		}
		__syncthreads();
		if (tid == 0) {
			double *s_out = sums + static_cast<uint64_t>(s) * NS;
			s_out[0] = static_cast<double>(n_y);
			double sum_d = 0.0;
			for (int e = 0; e < KP + 3; e++) {
				double t = part[0][e];
				for (int w = 1; w < kWaves; w++) {
					t += part[w][e];
				}
				s_out[1 + e] = t;
				sum_d = e == 0 ? t : sum_d;
			}
			for (int w = 1; w < kWaves; w++) {
				mn = fmin(mn, part[w][KP + 3]);
				mx = fmax(mx, part[w][KP + 4]);
				cnt += ipart[w][0];
				nz += ipart[w][1];
			}
			if (cnt < n_y) { // the untouched samples have d = 0
				mn = fmin(mn, 0.0);
				mx = fmax(mx, 0.0);
			}
			BurdenAux a;
			a.c = cs;
			a.sum_d = sum_d;
			a.n_nonzero = nz;
			a.touched = cnt;
			aux[s] = a;
			x_const[s] = (cnt == 0 || mn == mx) ? 1 : 0;
		}
	}
}

} // namespace

uint64_t BurdenScratchPerGroup(uint32_t sample_ct) {
	const uint64_t n = (static_cast<uint64_t>(sample_ct) + 255) / 256 * 256;
	return 9 * (n ? n : 256); // n doubles, then n marks
}

hipError_t LaunchBurdenSparse(const SparseView &sv, uint32_t n_sets, const uint64_t *set_off, const uint32_t *set_vidx,
                              const double *weight, const double *y, const double *z, uint32_t kp, uint32_t k,
                              uint32_t n_y, uint32_t n_groups, void *scratch, uint32_t *counter, double *sums,
                              BurdenAux *aux, uint8_t *x_const, hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp || n_groups == 0) {
		return hipErrorInvalidValue;
	}
	if (n_sets == 0) {
		return hipSuccess;
	}
	const uint64_t per_group = BurdenScratchPerGroup(sv.sample_ct), mark_off = per_group / 9 * 8;
	return GlmForWidth(kp, [&](auto width) {
		BurdenSparseKernel<decltype(width)::value><<<n_groups, kBlock, 0, stream>>>(
		    sv, n_sets, set_off, set_vidx, weight, y, z, n_y, static_cast<uint8_t *>(scratch), per_group, mark_off, counter,
		    sums, aux, x_const);
	});
}

} // namespace pgh
