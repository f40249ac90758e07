// glm_score_dense_firth.hip -- pgh_glm_score_multi_firth: the approximate Firth estimate of a (variant, phenotype) row
// of the dense route, from the variant's 2-bit row (the launch wrapper is in glm.hpp, the contract in
// include/pgenhip.h, the iteration in glm_firth.hpp).
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per (phenotype, chunk variant) its row.  A bounded grid of
// workgroups strides over the nv x pb rows and writes every row's pgh_glm_firth_row: the score row's beta, se and p with
// state 0 where the row is not fitted or |stat| <= cutoff, otherwise
//   phase A  GlmScoreDenseSpaKernel's walk of the variant-major row, a 16-code word per thread and 4,096 samples a
//            step, under the phenotype's mask word.  E = the samples of N with a code of 1 or 2, ranked in sample order
//            (a prefix sum of the words' counts); an entry gathers r from the phenotype's column of the block and
//            becomes the pair (x, mu), mu = r > 0 ? 1 - r : -r, at its rank in the workgroup's stash.  G = sum_E x r is
//            a chain per thread over its words' entries and then TeamSums.
//   phase B  FirthSolveStash (glm_firth.hpp) over the stash.
// A workgroup's stash is sample_ct pairs of global scratch of its own.  No atomics; nothing depends on which workgroup
// takes a row, on the grid, on the chunk, on the phenotype block or on where the range starts.
#include "glm.hpp"
#include "glm_firth.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;

struct DenseFirthArgs {
	const uint8_t *rows; // the resident rows
	uint64_t pitch;
	uint32_t v0, nv;     // the chunk: local rows v0 .. v0 + nv - 1
	uint32_t sample_ct;
	uint32_t mask_words; // 16-code words of a row and of a phenotype's mask (zero past the last sample)
	const uint32_t *mask;
	uint32_t pb;
	const double *b; // the column block
	uint32_t ld, k;
	const pgh_glm_row *out; // [pb][nv]
	double cutoff;
	double2 *stash;
	pgh_glm_firth_row *firth; // [pb][nv]
};

// One row by the workgroup.  at = p * nv + v; st: the workgroup's stash of sample_ct pairs.
__device__ __forceinline__ void DenseFirthRow(const DenseFirthArgs &a, uint32_t at, double2 *__restrict__ st,
                                              const pgh_glm_row *__restrict__ out,
                                              pgh_glm_firth_row *__restrict__ firth) {
	__shared__ uint32_t wave_ct[2][kTeamWaves]; // by the step's parity: a step's readers never meet the next step's writers
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
	const bool fitted = out[at].errcode == PGH_GLM_OK;
	pgh_glm_firth_row res {};
	res.beta = fitted ? out[at].beta : NAN;
	res.se = fitted ? out[at].se : NAN;
	res.p = fitted ? out[at].p : NAN;
	if (fitted && fabs(out[at].stat) > a.cutoff) { // (the whole workgroup)
		const uint32_t p = at / a.nv, v = at - p * a.nv;
		const uint32_t *row = reinterpret_cast<const uint32_t *>(a.rows + static_cast<uint64_t>(a.v0 + v) * a.pitch);
		const uint32_t *m = a.mask + static_cast<uint64_t>(p) * a.mask_words;
		const uint32_t col_r = p * (a.k + 2);

		// phase A
		uint32_t count = 0;
		double sums[1] = {0.0};
		long long none[4] = {0, 0, 0, 0};
		for (uint32_t w0 = 0, step = 0; w0 < a.mask_words; w0 += kBlock, step++) {
			const uint32_t wi = w0 + tid;
			uint32_t c = 0, em = 0; // bit 2 i of em: sample 16 wi + i is in E
			if (wi < a.mask_words) {
				c = row[wi];
				const uint32_t lo = c & 0x55555555u, hi = (c >> 1) & 0x55555555u;
				em = (lo ^ hi) & m[wi]; // codes {1, 2}
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
				const double ri = a.b[static_cast<uint64_t>(s) * a.ld + col_r];
				const double x = static_cast<double>((c >> (2u * i)) & 3u);
				sums[0] = fma(x, ri, sums[0]);
				if (pos < a.sample_ct) {
					st[pos] = make_double2(x, ri > 0.0 ? 1.0 - ri : -ri);
				}
				pos++;
			}
		}
		TeamSums<kBlock>(sums, none, lane, wave);
		TeamSync<kBlock>(); // the pairs before their readers, and TeamSums' LDS before it is written again
		// (the row is the same for the whole workgroup, which would make G and the state of the iteration scalar
		// registers: keep them in vector registers, as GlmScoreDenseSpaKernel does)
		double g = sums[0];
		asm volatile("" : "+v"(g));

		// phase B
		FirthFit fit;
		const bool ok = FirthSolveStash<kBlock>(st, count, count <= a.sample_ct, g, tid, lane, wave, &fit);
		if (ok) {
			res.beta = fit.beta;
			res.se = fit.se;
			res.p = fit.p;
		}
		res.state = ok ? 1 : 2;
	}
	if (tid == 0) {
		firth[at] = res;
	}
}

// A bounded grid: workgroup g takes the rows g, g + gridDim.x, ... of the nv x pb with its own sample_ct pairs of
// a.stash.
__global__ void __launch_bounds__(kBlock) GlmScoreDenseFirthKernel(const DenseFirthArgs a) {
	double2 *st = a.stash + static_cast<uint64_t>(blockIdx.x) * a.sample_ct;
	const uint32_t n_rows = a.nv * a.pb;
	for (uint32_t at = blockIdx.x; at < n_rows; at += gridDim.x) {
		DenseFirthRow(a, at, st, a.out, a.firth);
		__syncthreads(); // the next row rewrites the stash
	}
}

} // namespace

hipError_t LaunchGlmScoreDenseFirth(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask, uint32_t pb,
                                    const double *b, uint32_t k, const pgh_glm_row *rows, double cutoff,
                                    uint32_t n_groups, void *stash, pgh_glm_firth_row *firth, hipStream_t stream) {
	if (k > PGH_GLM_MAX_COVAR || pb == 0 || pb > kGlmScoreDensePb) {
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
	DenseFirthArgs a {};
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
	a.out = rows;
	a.cutoff = cutoff;
	a.stash = static_cast<double2 *>(stash);
	a.firth = firth;
	const uint64_t n_rows = static_cast<uint64_t>(nv) * pb;
	GlmScoreDenseFirthKernel<<<static_cast<uint32_t>(n_groups < n_rows ? n_groups : n_rows), kBlock, 0, stream>>>(a);
	return hipGetLastError();
}

} // namespace pgh
