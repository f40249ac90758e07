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
// A team (one wave, or the whole workgroup for a row of more than kGlmSparseLong entries) walks a row's entries at
// stride; y and z are staged in raw-sample order (NaN y: no phenotype or outside the subset), so an entry's sample
// addresses them.  The FP64 sums over C are one fma chain per lane, then a butterfly (and waves 0..3 in turn).  The
// entries of the Gram set are compacted in entry order into an LDS list, and every Gram entry belongs to one thread
// that walks the list in order, as in GlmGramKernel.  Nothing depends on which rows share a workgroup, on the chunk
// or on where the range starts.
#include "device_utils.hpp"
#include "glm.hpp"

#include <hip/hip_runtime.h>

namespace pgh {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxNe = 253; // (k + 2)(k + 3) / 2 at k = PGH_GLM_MAX_COVAR

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

// TEAM == 64: a wave per row, four rows per workgroup, the rows of at most kGlmSparseLong entries (and zeros for the
// dense-form rows, whose result rows come from the dense kernels).  TEAM == 256: a workgroup per row, the longer rows.
template <int KP, int TEAM>
__global__ void __launch_bounds__(kBlock) GlmSparseKernel(const int32_t *__restrict__ row_of,
                                                          const uint64_t *__restrict__ off,
                                                          const uint32_t *__restrict__ entries, uint32_t sample_ct,
                                                          uint32_t v_first, uint32_t nv, const double *__restrict__ y,
                                                          const double *__restrict__ z, uint32_t k, uint32_t n_y,
                                                          const double *__restrict__ gram, double *__restrict__ sums,
                                                          double *__restrict__ corr) {
	constexpr int NS = KP + 4;
	constexpr int NOWN = (kMaxNe + TEAM - 1) / TEAM; // Gram entries a thread owns
	constexpr int TEAMS = kBlock / TEAM;
	extern __shared__ double lds[]; // kBlock list rows of q doubles (sized at launch)
	const uint32_t q = k + 2, ne = q * (q + 1) / 2;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int tid = TEAM == kBlock ? static_cast<int>(threadIdx.x) : lane;
	const uint32_t i = blockIdx.x * TEAMS + (TEAM == kBlock ? 0 : wave);
	if (i >= nv) {
		return; // (the whole team)
	}
	const uint32_t r = v_first + i;
	const int32_t ro = row_of[r];
	double *s_out = sums + static_cast<uint64_t>(i) * NS;
	double *c_out = corr + static_cast<uint64_t>(i) * ne;
	if (ro >= 0) {
		if (TEAM == 64) {
			for (uint32_t e = tid; e < NS; e += TEAM) {
				s_out[e] = 0.0;
			}
			for (uint32_t e = tid; e < ne; e += TEAM) {
				c_out[e] = 0.0;
			}
		}
		return;
	}
	const uint64_t e0 = off[r], e1 = off[r + 1];
	if ((e1 - e0 > kGlmSparseLong) != (TEAM == kBlock)) {
		return; // the other launch's row
	}
	const bool base3 = ro == -4;
	const int bx = base3 ? 0 : -1 - ro;
	double *list = lds + (TEAM == kBlock ? 0 : static_cast<uint32_t>(wave) * 64u * q);

	// the Gram entries this thread owns: e = tid + t * TEAM -> (ea, eb), ea <= eb
	int ea[NOWN], eb[NOWN];
	double acc[NOWN];
#pragma unroll
	for (int t = 0; t < NOWN; t++) {
		int e = tid + t * TEAM, a = 0;
		ea[t] = eb[t] = -1;
		acc[t] = 0.0;
		if (e < static_cast<int>(ne)) {
			while (e >= static_cast<int>(q) - a) {
				e -= q - a;
				a++;
			}
			ea[t] = a;
			eb[t] = a + e;
		}
	}

	double sy = 0.0, sz[KP > 0 ? KP : 1];
#pragma unroll
	for (int j = 0; j < KP; j++) {
		sz[j] = 0.0;
	}
	long long c_miss = 0, c_called = 0, sx = 0, sxx = 0;
	for (uint64_t p0 = e0; p0 < e1; p0 += TEAM) {
		const uint64_t p = p0 + tid;
		bool used = false;
		uint32_t code = 0, s = 0;
		double yi = 0.0;
		if (p < e1) {
			const uint32_t x = entries[p];
			s = x >> 2;
			code = x & 3u;
			if (s < sample_ct) {
				yi = y[s];
				used = yi == yi;
			}
		}
		double zi[KP > 0 ? KP : 1];
		if (used) {
#pragma unroll
			for (int j = 0; j < KP; j++) {
				zi[j] = z[static_cast<uint64_t>(s) * KP + j];
			}
			if (code != 3u) {
				const int d = static_cast<int>(code) - bx;
				c_called++;
				sx += d;
				sxx += static_cast<int>(code * code) - bx * bx;
				const double dd = static_cast<double>(d);
				sy = fma(dd, yi, sy);
#pragma unroll
				for (int j = 0; j < KP; j++) {
					sz[j] = fma(dd, zi[j], sz[j]);
				}
			} else {
				c_miss++;
			}
		}
		// the Gram set of this step, in entry order (base 3: the called entries, which are all of them)
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
				row[q - 1] = yi;
			}
			TeamSync<TEAM>();
#pragma unroll
			for (int t = 0; t < NOWN; t++) {
				if (ea[t] >= 0) {
					for (uint32_t m = 0; m < total; m++) {
						acc[t] += list[m * q + ea[t]] * list[m * q + eb[t]];
					}
				}
			}
		}
		TeamSync<TEAM>(); // the list and wave_ct are rewritten by the next step
	}

	// team totals, on every thread
	sy = WaveSum(sy);
#pragma unroll
	for (int j = 0; j < KP; j++) {
		sz[j] = WaveSum(sz[j]);
	}
	c_miss = WaveSum(c_miss);
	c_called = WaveSum(c_called);
	sx = WaveSum(sx);
	sxx = WaveSum(sxx);
	if constexpr (TEAM == kBlock) {
		__shared__ double part[kWaves][KP + 1];
		__shared__ long long ipart[kWaves][4];
		if (lane == 0) {
			part[wave][0] = sy;
#pragma unroll
			for (int j = 0; j < KP; j++) {
				part[wave][1 + j] = sz[j];
			}
			ipart[wave][0] = c_miss;
			ipart[wave][1] = c_called;
			ipart[wave][2] = sx;
			ipart[wave][3] = sxx;
		}
		__syncthreads();
		sy = part[0][0];
		c_miss = ipart[0][0];
		c_called = ipart[0][1];
		sx = ipart[0][2];
		sxx = ipart[0][3];
#pragma unroll
		for (int j = 0; j < KP; j++) {
			sz[j] = part[0][1 + j];
		}
		for (int w = 1; w < kWaves; w++) {
			sy += part[w][0];
#pragma unroll
			for (int j = 0; j < KP; j++) {
				sz[j] += part[w][1 + j];
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
		for (uint32_t j = k; j < KP; j++) {
			s_out[4 + j] = 0.0; // the padded columns, as LaunchGlmSums leaves them
		}
	}
#pragma unroll
	for (int t = 0; t < NOWN; t++) {
		if (ea[t] < 0) {
			continue;
		}
		const uint32_t e = static_cast<uint32_t>(tid + t * TEAM);
		const double c = base3 ? gram[e] - acc[t] : acc[t];
		c_out[e] = c;
		if (t == 0 && e >= 1 && e < q) {
			// entry (1, u_e) of the Gram: u_e = z_(e-1), or y at e == q - 1
			double sc = sy;
#pragma unroll
			for (int j = 0; j < KP; j++) {
				sc = (e < q - 1 && e == static_cast<uint32_t>(1 + j)) ? sz[j] : sc;
			}
			const double v = bx ? static_cast<double>(bx) * (gram[e] - c) + sc : sc;
			s_out[e == q - 1 ? 3 : 3 + e] = v;
		}
	}
}

uint32_t Blocks(uint32_t n, uint32_t per) {
	return (n + per - 1) / per;
}

template <int KP>
void LaunchBoth(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *y, const double *z, uint32_t k,
                uint32_t n_y, const double *gram, double *sums, double *corr, hipStream_t stream) {
	const size_t lds = sizeof(double) * kBlock * (k + 2);
	GlmSparseKernel<KP, 64><<<Blocks(nv, kWaves), kBlock, lds, stream>>>(sv.row_of, sv.off, sv.entries, sv.sample_ct,
	                                                                     v_first, nv, y, z, k, n_y, gram, sums, corr);
	GlmSparseKernel<KP, kBlock><<<nv, kBlock, lds, stream>>>(sv.row_of, sv.off, sv.entries, sv.sample_ct, v_first, nv, y,
	                                                         z, k, n_y, gram, sums, corr);
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
#define PGH_SPARSE(KP_)                                                                                                \
	case KP_:                                                                                                          \
		LaunchBoth<KP_>(sv, v_first, nv, y, z, k, n_y, gram, sums, corr, stream);                                      \
		break;
	switch (kp) {
		PGH_SPARSE(0)
		PGH_SPARSE(1)
		PGH_SPARSE(2)
		PGH_SPARSE(4)
		PGH_SPARSE(8)
		PGH_SPARSE(12)
		PGH_SPARSE(16)
		PGH_SPARSE(20)
	default:
		return hipErrorInvalidValue;
	}
#undef PGH_SPARSE
	return hipGetLastError();
}

} // namespace pgh
