// glm_score_dense_spa.hip -- pgh_glm_score_multi_spa: the saddlepoint p-value of the logistic score test of a
// (variant, phenotype) row of the dense route, from the variant's 2-bit row (the launch wrapper is in glm.hpp, the
// contract in include/pgenhip.h, the arithmetic in glm_spa.hpp).
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per (phenotype, chunk variant) its row, [t = H_N^-1 c, U, V] with
// d = x, and p_spa = p with state 0.  A bounded grid of workgroups strides over the nv x pb rows; a workgroup takes a
// row that is fitted with |stat| > cutoff:
//   the base  b = 2 when the hom-alt calls among N outnumber the hom-ref ones, else 0, from the counts kernel's
//            integers n, sum x and sum x^2.  E = the samples of N with x != b.
//   phase A  one walk of the variant-major row, a 16-code word per thread and 4,096 samples a step, under the
//            phenotype's mask word.  The entries of E are ranked in sample order (a prefix sum of the words' counts,
//            GlmScoreDenseCorrKernel's scheme); an entry gathers r and w from the phenotype's columns of the block and
//            z from the raw-order covariates minus the phenotype's means, and becomes the pair (g, mu): g = x - Zt t,
//            mu = r > 0 ? 1 - r : -r.  The pairs go to the workgroup's stash in sample order, V_E = sum_E w g^2 is a
//            chain per thread over its words' entries and then TeamSums.
//   phase B  SpaSolveStash (glm_spa.hpp), GlmScoreSpaKernel's iteration over the stash.
// A workgroup's stash is sample_ct pairs of global scratch of its own.  No atomics; nothing depends on which workgroup
// takes a row, on the grid, on the chunk, on the phenotype block or on where the range starts.
#include "glm.hpp"
#include "glm_spa.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;

struct DenseSpaArgs {
	const uint8_t *rows; // the resident rows
	uint64_t pitch;
	uint32_t v0, nv;     // the chunk: local rows v0 .. v0 + nv - 1
	uint32_t sample_ct;
	uint32_t mask_words; // 16-code words of a row and of a phenotype's mask (zero past the last sample)
	const uint32_t *mask;
	uint32_t pb;
	const double *b; // the column block
	uint32_t ld, k;
	const double *z0, *mz;    // the uncentred covariates in raw-sample order, the phenotypes' means
	const double *sums;       // [pb][nv][kp + 6]: n, sum x, sum x^2 are read
	const pgh_glm_row *out;   // [pb][nv]
	const double *tv;         // [pb][nv][kp + 3]
	double cutoff;
	double2 *stash;
	double *p_spa;  // [pb][nv]
	uint8_t *state; // [pb][nv]
};

// One row by the workgroup.  at = p * nv + v; st: the workgroup's stash of sample_ct pairs.
template <int KP>
__device__ __forceinline__ void DenseSpaRow(const DenseSpaArgs &a, uint32_t at, double2 *__restrict__ st,
                                            const pgh_glm_row *__restrict__ out, const double *__restrict__ tv,
                                            const double *__restrict__ csums, double *__restrict__ p_spa,
                                            uint8_t *__restrict__ state) {
	__shared__ uint32_t wave_ct[2][kTeamWaves]; // by the step's parity: a step's readers never meet the next step's writers
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
	if (out[at].errcode != PGH_GLM_OK || !(fabs(out[at].stat) > a.cutoff)) {
		return; // (the whole workgroup)
	}
	const uint32_t p = at / a.nv, v = at - p * a.nv;
	// n1 + 2 n2 = sum x and n1 + 4 n2 = sum x^2, all integers
	const double *cs = csums + static_cast<uint64_t>(at) * (KP + 6);
	const long long n = static_cast<long long>(cs[0]), sx = static_cast<long long>(cs[1]),
	                sxx = static_cast<long long>(cs[2]);
	const long long n2 = (sxx - sx) / 2, n0 = n - (sx - 2 * n2) - n2;
	const bool b2 = n2 > n0;
	double t[KP + 1];
#pragma unroll
	for (int j = 0; j <= KP; j++) {
		t[j] = tv[static_cast<uint64_t>(at) * (KP + 3) + j];
		// the row is the same for the whole workgroup, which would make t, and below U, V and the state of the
		// iteration, scalar registers, more than there are: keep them in vector registers
		asm volatile("" : "+v"(t[j]));
	}
	double q = fabs(tv[static_cast<uint64_t>(at) * (KP + 3) + KP + 1]), vv = tv[static_cast<uint64_t>(at) * (KP + 3) + KP + 2];
	asm volatile("" : "+v"(q), "+v"(vv));
	const uint32_t *row = reinterpret_cast<const uint32_t *>(a.rows + static_cast<uint64_t>(a.v0 + v) * a.pitch);
	const uint32_t *m = a.mask + static_cast<uint64_t>(p) * a.mask_words;
	const double *mzp = a.mz + static_cast<uint64_t>(p) * KP;
	const uint32_t col_x = p * (a.k + 2);

	// phase A
	uint32_t count = 0;
	double sums[4] = {0.0, 0.0, 0.0, 0.0};
	long long none[4] = {0, 0, 0, 0};
	for (uint32_t w0 = 0, step = 0; w0 < a.mask_words; w0 += kBlock, step++) {
		const uint32_t wi = w0 + tid;
		uint32_t c = 0, em = 0; // bit 2 i of em: sample 16 wi + i is in E
		if (wi < a.mask_words) {
			c = row[wi];
			const uint32_t lo = c & 0x55555555u, hi = (c >> 1) & 0x55555555u;
			em = (b2 ? ~hi & 0x55555555u : lo ^ hi) & m[wi]; // codes {0, 1} under b = 2, codes {1, 2} under b = 0
		}
		const uint32_t cnt = static_cast<uint32_t>(__popc(em));
		uint32_t incl = cnt;
#pragma unroll
		for (uint32_t off = 1; off < 64u; off <<= 1) {
			const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), off, 64));
			incl += static_cast<uint32_t>(lane) >= off ? up : 0u;
		}
		if (lane == 63) {
			wave_ct[step & 1u][wave] = incl;
		}
		__syncthreads();
		uint32_t pos = count + incl - cnt;
		for (int w = 0; w < kTeamWaves; w++) {
			pos += w < wave ? wave_ct[step & 1u][w] : 0u;
			count += wave_ct[step & 1u][w];
		}
		while (em) {
			const uint32_t i = static_cast<uint32_t>(__ffs(static_cast<int>(em)) - 1) >> 1;
			em &= em - 1u;
			const uint32_t s = 16u * wi + i;
			const double *br = a.b + static_cast<uint64_t>(s) * a.ld + col_x;
			const double ri = br[0];
			double g = static_cast<double>((c >> (2u * i)) & 3u) - t[0];
#pragma unroll
			for (int j = 0; j < KP; j++) {
				g = fma(-(a.z0[static_cast<uint64_t>(s) * KP + j] - mzp[j]), t[1 + j], g);
			}
			sums[0] = fma(br[1] * g, g, sums[0]);
			if (pos < a.sample_ct) {
				st[pos] = make_double2(g, ri > 0.0 ? 1.0 - ri : -ri);
			}
			pos++;
		}
	}
	TeamSums<kBlock>(sums, none, lane, wave);
	TeamSync<kBlock>(); // the pairs before their readers, and TeamSums' LDS before it is written again
	// (a fitted row has a called sample with x = b, or it would be CONST_ALLELE: V_rest is never 0 by rule here)
	const double v_rest = fmax(vv - sums[0], 0.0);

	// phase B
	double ps;
	const bool ok = SpaSolveStash<kBlock>(st, count, count <= a.sample_ct, q, vv, v_rest, tid, lane, wave, &ps);
	if (tid == 0) {
		if (ok) {
			p_spa[at] = ps;
		}
		state[at] = ok ? 1 : 2;
	}
}

// A bounded grid: workgroup g takes the rows g, g + gridDim.x, ... of the nv x pb with its own sample_ct pairs of
// a.stash.
template <int KP>
__global__ void __launch_bounds__(kBlock) GlmScoreDenseSpaKernel(const DenseSpaArgs a) {
	double2 *st = a.stash + static_cast<uint64_t>(blockIdx.x) * a.sample_ct;
	double *p_spa = a.p_spa;
	uint8_t *state = a.state;
	const pgh_glm_row *out = a.out;
	const double *tv = a.tv, *csums = a.sums;
	// (thread 0's stores and a few loads per row use them: held in vector registers, the loop's scalar registers all fit)
	asm volatile("" : "+v"(p_spa), "+v"(state), "+v"(out), "+v"(tv), "+v"(csums));
	const uint32_t n_rows = a.nv * a.pb;
	for (uint32_t at = blockIdx.x; at < n_rows; at += gridDim.x) {
		DenseSpaRow<KP>(a, at, st, out, tv, csums, p_spa, state);
		__syncthreads(); // the next row rewrites the stash
	}
}

} // namespace

hipError_t LaunchGlmScoreDenseSpa(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask, uint32_t pb,
                                  const double *b, const double *z0, const double *mz, uint32_t kp, uint32_t k,
                                  const double *sums, const pgh_glm_row *rows, const double *t, double cutoff,
                                  uint32_t n_groups, void *stash, double *p_spa, uint8_t *state, hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || k > kp || pb == 0 || pb > kGlmScoreDensePb) {
		return hipErrorInvalidValue;
	}
	if (nv == 0) {
		return hipSuccess;
	}
	if (n_groups == 0) {
		return hipErrorInvalidValue;
	}
	const uint32_t words16 = (view.sample_ct + 63u) / 64u;
	if (16ull * words16 > view.pitch) {
		return hipErrorInvalidValue; // the kernel reads whole 16-code words of a row up to the mask's length
	}
	DenseSpaArgs a {};
	a.rows = view.rows;
	a.pitch = view.pitch;
	a.v0 = v0;
	a.nv = nv;
	a.sample_ct = view.sample_ct;
	a.mask_words = 4u * words16;
	a.mask = mask;
	a.pb = pb;
	a.b = b;
	a.ld = GlmScoreDenseLayout(pb, k).ld;
	a.k = k;
	a.z0 = z0;
	a.mz = mz;
	a.sums = sums;
	a.out = rows;
	a.tv = t;
	a.cutoff = cutoff;
	a.stash = static_cast<double2 *>(stash);
	a.p_spa = p_spa;
	a.state = state;
	const uint64_t n_rows = static_cast<uint64_t>(nv) * pb;
	return GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value;
		GlmScoreDenseSpaKernel<KP><<<static_cast<uint32_t>(n_groups < n_rows ? n_groups : n_rows), kBlock, 0, stream>>>(a);
	});
}

} // namespace pgh
