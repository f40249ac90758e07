// glm_score_dense_dosage_firth.hip -- pgh_glm_score_multi_dosage_firth: the approximate Firth estimate of a (variant,
// phenotype) row of the dense route whose variant carries a dosage track, from the variant's expanded row of 16-bit
// values (the launch wrapper is in glm.hpp, the contract in include/pgenhip.h, the iteration in glm_firth.hpp;
// DESIGN.md 3.10).
//
// glm_score_dense_dosage.hip has left the chunk's listed variants' u16 rows (x = v / 16384, 0xFFFF for neither a dosage
// nor a call); GlmScoreSolveKernel (glm_score_sparse.hip) has left per (phenotype, listed variant) its row.  A bounded
// grid of workgroups strides over the nt x pb rows and writes every row's pgh_glm_firth_row: the score row's beta, se
// and p with state 0 where the row is not fitted or |stat| <= cutoff, otherwise
//   phase A  TeamStashMaskedU16Row (glm_team.hpp) over the u16 row under the phenotype's mask word with base 0,
//            selecting E = the samples of N whose value is not exactly 0.  An entry gathers r from the phenotype's
//            column of the block and becomes the pair (x, mu), x = v / 16384, mu = r > 0 ? 1 - r : -r.  G = sum_E x r is
//            the walk's chain per thread and then TeamSums.
//   phase B  FirthSolveStash (glm_firth.hpp) over the stash.
// The walk has the 2-bit walk's geometry, so a track that restates its calls gives GlmScoreDenseFirthKernel's chain,
// stash order and result bit for bit.  A workgroup's stash is sample_ct pairs of global scratch of its own.  No atomics;
// nothing depends on which workgroup takes a row, on the grid, on the chunk, on the phenotype block, on where the range
// starts or on which other variants carry tracks.
#include "glm.hpp"
#include "glm_firth.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;

struct DenseDosageFirthArgs {
	DenseRows rows;         // nv: the listed variants; the 2-bit rows are not read
	const uint16_t *u16;    // [nv] rows of 16 mask_words values
	const pgh_glm_row *out; // [pb][nv]
	double cutoff;
	double2 *stash;
	pgh_glm_firth_row *firth; // [pb][nv]
};

// One row by the workgroup.  at = p * nv + v; st: the workgroup's stash of sample_ct pairs.
__device__ __forceinline__ void DenseDosageFirthRow(const DenseDosageFirthArgs &a, uint32_t at, double2 *__restrict__ st,
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
		const uint16_t *row = a.u16 + static_cast<uint64_t>(v) * d.mask_words * 16u;
		asm volatile("" : "+v"(row)); // (row-uniform: kept out of the scalar registers, as in the saddlepoint sibling)

		// phase A
		double sums[1] = {0.0};
		long long none[4] = {0, 0, 0, 0};
		const uint32_t count = TeamStashMaskedU16Row(
		    row, d.Mask(p), d.mask_words, /*base=*/0u, st, d.sample_ct, tid, lane, wave, [&](uint32_t s, uint32_t val) {
			    const double ri = d.b[static_cast<uint64_t>(s) * d.ld + col_r];
			    const double x = static_cast<double>(val) * 0x1p-14; // (the product is exact)
			    sums[0] = fma(x, ri, sums[0]);
			    return make_double2(x, ri > 0.0 ? 1.0 - ri : -ri);
		    });
		TeamSums<kBlock>(sums, none, lane, wave);
		TeamSync<kBlock>(); // the pairs before their readers, and TeamSums' LDS before it is written again
		// (the row is the same for the whole workgroup, which would make G and the state of the iteration scalar
		// registers: keep them in vector registers, as GlmScoreDenseFirthKernel does)
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

// TeamGridRows over the nt x pb rows: a workgroup has its own sample_ct pairs of a.stash.
__global__ void __launch_bounds__(kBlock) GlmScoreDenseDosageFirthKernel(const DenseDosageFirthArgs a) {
	double2 *st = a.stash + static_cast<uint64_t>(blockIdx.x) * a.rows.sample_ct;
	TeamGridRows(a.rows.nv * a.rows.pb, [&](uint32_t at) { DenseDosageFirthRow(a, at, st, a.out, a.firth); });
}

} // namespace

hipError_t LaunchGlmScoreDenseDosageFirth(const RowView &view, const uint16_t *u16, uint32_t nt, const uint32_t *mask,
                                          uint32_t pb, const double *b, uint32_t k, const pgh_glm_row *rows,
                                          double cutoff, uint32_t n_groups, void *stash, pgh_glm_firth_row *firth,
                                          hipStream_t stream) {
	DenseDosageFirthArgs a {};
	uint32_t grid;
	const hipError_t e = DenseRowsFor(view, 0, nt, mask, pb, b, k, n_groups, &a.rows, &grid);
	if (e != hipSuccess || grid == 0) {
		return e;
	}
	a.u16 = u16;
	a.out = rows;
	a.cutoff = cutoff;
	a.stash = static_cast<double2 *>(stash);
	a.firth = firth;
	GlmScoreDenseDosageFirthKernel<<<grid, kBlock, 0, stream>>>(a);
	return hipGetLastError();
}

} // namespace pgh
