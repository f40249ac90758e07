// glm_score_dense_firth.hip -- pgh_glm_score_multi_firth: the approximate Firth estimate of a (variant, phenotype) row
// of the dense route, from the variant's 2-bit row (the launch wrapper is in glm.hpp, the contract in
// include/pgenhip.h, the iteration in glm_firth.hpp).
//
// GlmScoreSolveKernel (glm_score_sparse.hip) has left per (phenotype, chunk variant) its row.  A bounded grid of
// workgroups strides over the nv x pb rows and writes every row's pgh_glm_firth_row: the score row's beta, se and p with
// state 0 where the row is not fitted or |stat| <= cutoff, otherwise
//   phase A  TeamStashMaskedRow (glm_team.hpp) over the variant-major row under the phenotype's mask word, selecting
//            E = the samples of N with a code of 1 or 2.  An entry gathers r from the phenotype's column of the block
//            and becomes the pair (x, mu), mu = r > 0 ? 1 - r : -r.  G = sum_E x r is the walk's chain per thread and
//            then TeamSums.
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
	DenseRows rows;
	const pgh_glm_row *out; // [pb][nv]
	double cutoff;
	double2 *stash;
	pgh_glm_firth_row *firth; // [pb][nv]
};

// One row by the workgroup.  at = p * nv + v; st: the workgroup's stash of sample_ct pairs.
__device__ __forceinline__ void DenseFirthRow(const DenseFirthArgs &a, uint32_t at, double2 *__restrict__ st,
                                              const pgh_glm_row *__restrict__ out,
                                              pgh_glm_firth_row *__restrict__ firth) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
	const bool fitted = out[at].errcode == PGH_GLM_OK;
	pgh_glm_firth_row res {};
	res.beta = fitted ? out[at].beta : NAN;
	res.se = fitted ? out[at].se : NAN;
	res.p = fitted ? out[at].p : NAN;
	if (fitted && fabs(out[at].stat) > a.cutoff) { // (the whole workgroup)
		const DenseRows &d = a.rows;
		const uint32_t p = at / d.nv, v = at - p * d.nv;
		const uint32_t col_r = p * (d.k + 2);

		// phase A
		double sums[1] = {0.0};
		long long none[4] = {0, 0, 0, 0};
		const uint32_t count = TeamStashMaskedRow(
		    d.Row(v), d.Mask(p), d.mask_words, st, d.sample_ct, tid, lane, wave,
		    [](uint32_t c, uint32_t m) {
			    const uint32_t lo = c & 0x55555555u, hi = (c >> 1) & 0x55555555u;
			    return (lo ^ hi) & m; // codes {1, 2}
		    },
		    [&](uint32_t s, uint32_t code) {
			    const double ri = d.b[static_cast<uint64_t>(s) * d.ld + col_r];
			    const double x = static_cast<double>(code);
			    sums[0] = fma(x, ri, sums[0]);
			    return make_double2(x, ri > 0.0 ? 1.0 - ri : -ri);
		    });
		TeamSums<kBlock>(sums, none, lane, wave);
		TeamSync<kBlock>(); // the pairs before their readers, and TeamSums' LDS before it is written again
		// (the row is the same for the whole workgroup, which would make G and the state of the iteration scalar
		// registers: keep them in vector registers, as GlmScoreDenseSpaKernel does)
		double g = sums[0];
		asm volatile("" : "+v"(g));

		// phase B
		FirthFit fit;
		const bool ok = FirthSolveStash<kBlock>(st, count, count <= d.sample_ct, g, tid, lane, wave, &fit);
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

// TeamGridRows over the nv x pb rows: a workgroup has its own sample_ct pairs of a.stash.
__global__ void __launch_bounds__(kBlock) GlmScoreDenseFirthKernel(const DenseFirthArgs a) {
	double2 *st = a.stash + static_cast<uint64_t>(blockIdx.x) * a.rows.sample_ct;
	TeamGridRows(a.rows.nv * a.rows.pb, [&](uint32_t at) { DenseFirthRow(a, at, st, a.out, a.firth); });
}

} // namespace

hipError_t LaunchGlmScoreDenseFirth(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask, uint32_t pb,
                                    const double *b, uint32_t k, const pgh_glm_row *rows, double cutoff,
                                    uint32_t n_groups, void *stash, pgh_glm_firth_row *firth, hipStream_t stream) {
	DenseFirthArgs a {};
	uint32_t grid;
	const hipError_t e = DenseRowsFor(view, v0, nv, mask, pb, b, k, n_groups, &a.rows, &grid);
	if (e != hipSuccess || grid == 0) {
		return e;
	}
	a.out = rows;
	a.cutoff = cutoff;
	a.stash = static_cast<double2 *>(stash);
	a.firth = firth;
	GlmScoreDenseFirthKernel<<<grid, kBlock, 0, stream>>>(a);
	return hipGetLastError();
}

} // namespace pgh
