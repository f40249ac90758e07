// glm_score_dense_dosage_spa.hip -- pgh_glm_score_multi_dosage_spa: the saddlepoint p-value of the logistic score test
// of a (variant, phenotype) row of the dense route whose variant carries a dosage track, from the variant's expanded
// row of 16-bit values (the launch wrapper is in glm.hpp, the contract in include/pgenhip.h, the arithmetic in
// glm_spa.hpp).
//
// glm_score_dense_dosage.hip has left the chunk's listed variants' u16 rows (x = v / 16384, 0xFFFF for neither a dosage
// nor a call) and their sums; GlmScoreSolveKernel (glm_score_sparse.hip) has left per (phenotype, listed variant) its
// row, [t = H_N^-1 c, U, V] with d = x, and p_spa = p with state 0.  A bounded grid of workgroups strides over the
// nt x pb rows; a workgroup takes a row that is fitted with |stat| > cutoff:
//   the base  b = 2 when sum_N x > n, else 0: an exact comparison of the counts kernel's n and sum x, which for a row
//            of calls is glm_score_dense_spa.hip's "n2 > n0".  E = the samples of N whose value is not exactly b.
//   phase A  TeamStashMaskedU16Row (glm_team.hpp) over the u16 row under the phenotype's mask word, selecting E.  An
//            entry gathers r and w from the phenotype's columns of the block and z from the raw-order covariates minus
//            the phenotype's means, and becomes the pair (g, mu): g = x - Zt t, mu = r > 0 ? 1 - r : -r.
//            V_E = sum_E w g^2 is the walk's chain per thread and then TeamSums.
//   V_rest   0 by rule when E = N (the walk's count equals n: no sample of N sits on b, the usual case of a full
//            track), else max(V - V_E, 0).
//   phase B  SpaSolveStash (glm_spa.hpp), GlmScoreSpaKernel's iteration over the stash.
// The walk has the 2-bit walk's geometry, so a track that restates its calls gives GlmScoreDenseSpaKernel's chains, stash
// order and result bit for bit.  A workgroup's stash is sample_ct pairs of global scratch of its own.  No atomics;
// nothing depends on which workgroup takes a row, on the grid, on the chunk, on the phenotype block, on where the range
// starts or on which other variants carry tracks.
#include "glm.hpp"
#include "glm_spa.hpp"
#include "glm_team.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace pgh {

namespace {

constexpr int kBlock = kTeamBlock;

struct DenseDosageSpaArgs {
	DenseRows rows;           // nv: the listed variants; the 2-bit rows are not read
	const uint16_t *u16;      // [nv] rows of 16 mask_words values
	const double *z0, *mz;    // the uncentred covariates in raw-sample order, the phenotypes' means
	const double *sums;       // [pb][nv][kp + 6]: n and sum x are read
	const pgh_glm_row *out;   // [pb][nv]
	const double *tv;         // [pb][nv][kp + 3]
	double cutoff;
	double2 *stash;
	double *p_spa;  // [pb][nv]
	uint8_t *state; // [pb][nv]
};

// One row by the workgroup.  at = p * nv + v; st: the workgroup's stash of sample_ct pairs.
template <int KP>
__device__ __forceinline__ void DenseDosageSpaRow(const DenseDosageSpaArgs &a, uint32_t at, double2 *__restrict__ st,
                                                  const pgh_glm_row *__restrict__ out, const double *__restrict__ tv,
                                                  const double *__restrict__ csums, double *__restrict__ p_spa,
                                                  uint8_t *__restrict__ state) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
	if (out[at].errcode != PGH_GLM_OK || !(fabs(out[at].stat) > a.cutoff)) {
		return; // (the whole workgroup)
	}
	const DenseRows &d = a.rows;
	const uint32_t p = at / d.nv, v = at - p * d.nv;
	// n and sum x are exact in FP64 (sum x on the 2^-14 grid), so the comparison is
	const double *cs = csums + static_cast<uint64_t>(at) * (KP + 6);
	uint32_t n = static_cast<uint32_t>(cs[0]);
	uint32_t base = cs[1] > cs[0] ? 2u << 14 : 0u;
	const uint16_t *row = a.u16 + static_cast<uint64_t>(v) * d.mask_words * 16u;
	asm volatile("" : "+v"(n), "+v"(base), "+v"(row)); // (row-uniform too)
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
	const double *mzp = a.mz + static_cast<uint64_t>(p) * KP;
	const uint32_t col_x = p * (d.k + 2);

	// phase A
	double sums[4] = {0.0, 0.0, 0.0, 0.0};
	long long none[4] = {0, 0, 0, 0};
	const uint32_t count = TeamStashMaskedU16Row(
	    row, d.Mask(p), d.mask_words, base, st, d.sample_ct, tid, lane, wave, [&](uint32_t s, uint32_t val) {
		    const double *br = d.b + static_cast<uint64_t>(s) * d.ld + col_x;
		    const double ri = br[0];
		    double g = static_cast<double>(val) * 0x1p-14 - t[0]; // (the product is exact)
#pragma unroll
		    for (int j = 0; j < KP; j++) {
			    g = fma(-(a.z0[static_cast<uint64_t>(s) * KP + j] - mzp[j]), t[1 + j], g);
		    }
		    sums[0] = fma(br[1] * g, g, sums[0]);
		    return make_double2(g, ri > 0.0 ? 1.0 - ri : -ri);
	    });
	TeamSums<kBlock>(sums, none, lane, wave);
	TeamSync<kBlock>(); // the pairs before their readers, and TeamSums' LDS before it is written again
	const double v_rest = count == n ? 0.0 : fmax(vv - sums[0], 0.0);

	// phase B
	double ps;
	const bool ok = SpaSolveStash<kBlock>(st, count, count <= d.sample_ct, q, vv, v_rest, tid, lane, wave, &ps);
	if (tid == 0) {
		if (ok) {
			p_spa[at] = ps;
		}
		state[at] = ok ? 1 : 2;
	}
}

// TeamGridRows over the nt x pb rows: a workgroup has its own sample_ct pairs of a.stash.
template <int KP>
__global__ void __launch_bounds__(kBlock) GlmScoreDenseDosageSpaKernel(const DenseDosageSpaArgs a) {
	double2 *st = a.stash + static_cast<uint64_t>(blockIdx.x) * a.rows.sample_ct;
	double *p_spa = a.p_spa;
	uint8_t *state = a.state;
	const pgh_glm_row *out = a.out;
	const double *tv = a.tv, *csums = a.sums;
	// (thread 0's stores and a few loads per row use them: held in vector registers, the loop's scalar registers all fit)
	asm volatile("" : "+v"(p_spa), "+v"(state), "+v"(out), "+v"(tv), "+v"(csums));
	TeamGridRows(a.rows.nv * a.rows.pb,
	             [&](uint32_t at) { DenseDosageSpaRow<KP>(a, at, st, out, tv, csums, p_spa, state); });
}

} // namespace

hipError_t LaunchGlmScoreDenseDosageSpa(const RowView &view, const uint16_t *u16, uint32_t nt, const uint32_t *mask,
                                        uint32_t pb, const double *b, const double *z0, const double *mz, uint32_t kp,
                                        uint32_t k, const double *sums, const pgh_glm_row *rows, const double *t,
                                        double cutoff, uint32_t n_groups, void *stash, double *p_spa, uint8_t *state,
                                        hipStream_t stream) {
	if (k > kp) {
		return hipErrorInvalidValue;
	}
	DenseDosageSpaArgs a {};
	uint32_t grid;
	const hipError_t e = DenseRowsFor(view, 0, nt, mask, pb, b, k, n_groups, &a.rows, &grid);
	if (e != hipSuccess || grid == 0) {
		return e;
	}
	a.u16 = u16;
	a.z0 = z0;
	a.mz = mz;
	a.sums = sums;
	a.out = rows;
	a.tv = t;
	a.cutoff = cutoff;
	a.stash = static_cast<double2 *>(stash);
	a.p_spa = p_spa;
	a.state = state;
	return GlmForWidth(kp, [&](auto width) {
		constexpr int KP = decltype(width)::value;
		GlmScoreDenseDosageSpaKernel<KP><<<grid, kBlock, 0, stream>>>(a);
	});
}

} // namespace pgh
