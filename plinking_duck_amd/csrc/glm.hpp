// glm.hpp -- launch wrappers of plink_glm's kernels (glm.hip).  All pointers are device pointers; every wrapper only
// enqueues work on `stream`.  Variants are addressed by their index i in the current chunk (local row g.v0 + i).
#pragma once

#include "../../include/pgenhip.h"
#include "kernels.hpp"
#include "sparse.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <iterator>
#include <type_traits>
#include <utility>

namespace pgh {

// Where a chunk variant's genotype values come from: its dense dosage row when slot[i] >= 0 (n_out doubles, -9 =
// missing, pgh_dosage_unpack's layout), otherwise its 2-bit row (code 3 = missing).  sel: output -> raw sample.
struct GlmX {
	RowView view;
	uint32_t v0;
	const int32_t *slot; // may be null: no dosage rows
	const double *dos;
	uint32_t n_out;
	const uint32_t *sel; // null: all samples
};

// Per-variant fit state of the logistic / Firth rounds.
struct GlmState {
	int32_t status; // kGlmActive .. ; >= kGlmDecided + errcode: decided before any fit
	int32_t iter;
	int32_t firth;
	int32_t pad;
	double min_delta, delta_max, loglik, loglik_old;
};
enum : int32_t { kGlmActive = 0, kGlmConverged = 1, kGlmFailed = 2, kGlmUnfinished = 3, kGlmDecided = 16 };

// The covariate widths KP that the kernels templated on a width are instantiated for.
constexpr uint32_t kGlmWidths[] = {0, 1, 2, 4, 8, 12, 16, 20};
//! Padded covariate count of the kernels: the smallest instantiated width >= k (k <= 20).
uint32_t GlmPadCovar(uint32_t k);
// Variants per workgroup of GlmSumsKernel at the width KP.
constexpr int GlmSumsTile(int kp) {
	return kp <= 2 ? 8 : kp <= 8 ? 4 : 2;
}
// Calls launch(std::integral_constant<int, KP>()) with KP == kp, which enqueues the kernels of that width, and returns
// hipGetLastError(); hipErrorInvalidValue if kp is not an instantiated width.
template <class Launch, size_t... I>
hipError_t GlmForWidth(uint32_t kp, Launch &&launch, std::index_sequence<I...>) {
	const bool known = ((kp == kGlmWidths[I] && (launch(std::integral_constant<int, kGlmWidths[I]>()), true)) || ...);
	return known ? hipGetLastError() : hipErrorInvalidValue;
}
template <class Launch>
hipError_t GlmForWidth(uint32_t kp, Launch &&launch) {
	return GlmForWidth(kp, launch, std::make_index_sequence<std::size(kGlmWidths)>());
}
//! Accumulators of one variant in the Newton / Firth rounds: packed upper Hessian, a vector, a scalar, a flag.
inline uint32_t GlmIrlsEntries(uint32_t kp) {
	const uint32_t pp = kp + 2;
	return pp * (pp + 1) / 2 + pp + 2;
}

// sums[i][kp+4] = {n, sum x, sum x^2, sum x y, sum x z_j (j < kp)} over the samples with a phenotype and a value.
// y: n_out doubles (NaN = missing); z: n_out x kp doubles, sample-major (zero padded).
hipError_t LaunchGlmSums(const GlmX &g, uint32_t nv, const double *y, const double *z, uint32_t kp, double *sums,
                         hipStream_t stream);
// Packed upper Gram of u = [1, z_1..z_k, y] ((k+2)(k+3)/2 entries).  g == null: over every sample with a phenotype,
// one row.  Otherwise per chunk variant over its samples with a phenotype and no value (zero rows for variants that
// have none: sums[i][0] == n_y).
hipError_t LaunchGlmGram(const GlmX *g, uint32_t nv, const double *sums, uint32_t sums_stride, uint32_t n_y,
                         uint32_t n_out, const double *y, const double *z, uint32_t kp, uint32_t k, double *out,
                         hipStream_t stream);
// The OLS per variant from the sums, the whole-call Gram and the variant's correction Gram.
// x_const != null (pgh_burden_sparse, whose x is off the 2^-14 dosage grid that the solve's own constancy test is
// written for): row v is CONST_ALLELE iff x_const[v] != 0, and the correction Grams are zero (corr is not read).
hipError_t LaunchGlmLinearSolve(uint32_t nv, const double *sums, uint32_t kp, uint32_t k, const double *gram,
                                const double *corr, pgh_glm_row *rows, hipStream_t stream,
                                const uint8_t *x_const = nullptr);
// Logistic: TOO_FEW_SAMPLES / CONST_ALLELE from the kp = 0 sums, beta = 0 for the others.
hipError_t LaunchGlmLogisticInit(uint32_t nv, const double *sums, uint32_t kp, uint32_t k, GlmState *st, double *beta,
                                 pgh_glm_row *rows, hipStream_t stream);
// One accumulation pass over the active variants (list == null: chunk variants 0..n-1 with status kGlmActive).
// mode 0: Newton (Hessian, gradient); 1: Firth, I(beta) + log-likelihood; 2: Firth, second-weight Hessian + U*
// (reads hinv0: the inverse of mode 1's matrix).
hipError_t LaunchGlmIrlsAcc(int mode, const GlmX &g, const uint32_t *list, uint32_t n, const double *y, const double *z,
                            uint32_t kp, const GlmState *st, const double *beta, const double *hinv0, double *acc,
                            hipStream_t stream);
hipError_t LaunchGlmNewtonUpdate(uint32_t nv, uint32_t kp, uint32_t k, const double *acc, GlmState *st, double *beta,
                                 double *hmat, hipStream_t stream);
hipError_t LaunchGlmFirthStart(const uint32_t *list, uint32_t n, uint32_t kp, GlmState *st, double *beta,
                               hipStream_t stream);
hipError_t LaunchGlmFirthUpdate(int half, const uint32_t *list, uint32_t n, uint32_t kp, uint32_t k, const double *acc,
                                GlmState *st, double *beta, double *hinv0, double *hmat, hipStream_t stream);
// hmat: kMaxP x kMaxP doubles per variant (the last Newton Hessian; after a Firth fit, its last inverse).
constexpr uint32_t kGlmMaxP = 22;
// Rows of the logistic fits from the final state (a plain fit that failed or did not finish and was not refitted
// with Firth's penalty gives SEPARATION / NO_CONVERGENCE).
hipError_t LaunchGlmLogisticFinish(uint32_t nv, uint32_t kp, uint32_t k, const GlmState *st,
                                   const double *beta, const double *hmat, pgh_glm_row *rows, hipStream_t stream);

// ---- pgh_glm_multi, linear: the phenotypes of one missing-value pattern, at most kGlmMultiPb per launch ----
// yb: pb x n_out doubles, phenotype-major, centred, 0 where missing.  ypat: n_out doubles, NaN exactly where the
// pattern's phenotypes are missing.  Every (variant, phenotype) number is one thread's sequential sum over the
// samples, so none depends on pb, the phenotype's place in the block or the chunk.
constexpr uint32_t kGlmMultiPb = 64;
// sxy[i][p] = sum x y_p over the chunk variant's samples with a value (pb <= kGlmMultiPb)
hipError_t LaunchGlmMultiXy(const GlmX &g, uint32_t nv, const double *yb, uint32_t pb, double *sxy,
                            hipStream_t stream);
// whole[p][0..k+1] = {sum y_p, sum z_j y_p (j < k), sum y_p^2} over every sample with a phenotype
hipError_t LaunchGlmMultiWhole(uint32_t n_out, const double *yb, uint32_t pb, const double *z, uint32_t kp,
                               uint32_t k, double *whole, hipStream_t stream);
// Per chunk variant, over its samples with a phenotype and no value: corr_s[i] = packed Gram of [1, z]
// ((k+1)(k+2)/2 entries), corr_p[i][p][0..k+1] = whole's entries (zeros for variants that have none: sums[i][0] ==
// n_y).  sums: LaunchGlmSums' rows (stride kp + 4).
hipError_t LaunchGlmMultiCorr(const GlmX &g, uint32_t nv, const double *sums, uint32_t n_y, const double *ypat,
                              const double *yb, uint32_t pb, const double *z, uint32_t kp, uint32_t k, double *corr_s,
                              double *corr_p, hipStream_t stream);
// rows[i][p]: the OLS of chunk variant i and phenotype p.  gram: LaunchGlmGram's whole-call Gram of [1, z, ypat]
// (only its (1, z) block is read).
hipError_t LaunchGlmMultiSolve(uint32_t nv, uint32_t pb, const double *sums, uint32_t kp, uint32_t k,
                               const double *sxy, const double *gram, const double *whole, const double *corr_s,
                               const double *corr_p, pgh_glm_row *rows, hipStream_t stream);

// ---- pgh_glm_sparse (glm_sparse.hip): the linear fit's sums and correction Grams from a sparse row's entries ----
// A row of more than kGlmSparseLong entries is walked by a whole workgroup, a shorter one by one wave.
constexpr uint32_t kGlmSparseLong = 1024;
// For the rows v_first + i (i < nv) of `sv` that are sparse: sums[i][kp+4] in LaunchGlmSums' layout and corr[i] in
// LaunchGlmGram's per-variant layout, ready for LaunchGlmLinearSolve; zeros for the dense-form rows.
// y: sv.sample_ct doubles in RAW sample order, NaN = no phenotype or outside the subset; z: sv.sample_ct x kp doubles,
// raw sample-major.  gram: LaunchGlmGram's whole-call Gram over the n_y samples with a phenotype.
hipError_t LaunchGlmSparse(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *y, const double *z,
                           uint32_t kp, uint32_t k, uint32_t n_y, const double *gram, double *sums, double *corr,
                           hipStream_t stream);

// ---- pgh_glm_sparse_multi (glm_sparse_multi.hip): the linear fit from a sparse row's entries for a block of
// phenotypes ----
// At most kGlmSparseMultiPb phenotypes share a value block and a walk of the entries.  No number depends on the block's
// size, on a phenotype's place in it or on the chunk.
constexpr uint32_t kGlmSparseMultiPb = 64;
// Partial sums per entry of a whole-call Gram: a fixed shape, so G_j is a function of its phenotype, z and the subset.
constexpr uint32_t kGlmSparseMultiParts = 64;
// The value block of pb phenotypes: yv[s][j] = yb[j][i] - my[j] for the subset's samples s = sel[i] (sel == null: i),
// NaN everywhere else (and where yb is NaN); sample_ct x pb doubles.  yb: pb x n_out doubles, phenotype-major.
hipError_t LaunchGlmSparseMultiValues(uint32_t sample_ct, uint32_t n_out, const uint32_t *sel, const double *yb,
                                      const double *my, uint32_t pb, double *yv, hipStream_t stream);
// gram[j]: the packed upper Gram of u = [1, z - mz[j], yv[.][j]] ((k+2)(k+3)/2 entries) over the samples with a value
// of j.  z: sample_ct x kp doubles, raw sample-major, uncentred; mz: pb x kp means.  part: pb x kGlmSparseMultiParts x
// (entries) doubles of scratch.
hipError_t LaunchGlmSparseMultiGram(uint32_t sample_ct, const double *yv, uint32_t pb, const double *z, const double *mz,
                                    uint32_t kp, uint32_t k, double *part, double *gram, hipStream_t stream);
// For the rows v_first + i (i < nv) of `sv`, sparse or held in the dense form, and the block's phenotypes j < pb:
// out[i][j], the row of GlmLinearSolveKernel<false>.  n_y[j]: the samples with a value of j.  Scratch: sums
// nv x pb x (kp + 4), corr nv x pb x (entries of a Gram) doubles, nlist nv words.
hipError_t LaunchGlmSparseMulti(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *yv,
                                const uint32_t *n_y, uint32_t pb, const double *z, const double *mz, uint32_t kp,
                                uint32_t k, const double *gram, double *sums, uint32_t *nlist, double *corr,
                                pgh_glm_row *out, hipStream_t stream);

// ---- pgh_glm_score_sparse (glm_score_sparse.hip): the logistic score test from a sparse row's entries ----
// The null model y ~ Zt = [1, z_1..z_k] and its packed sums hg: H = sum_S w Zt Zt' ((k+1)(k+2)/2 entries, row-major
// upper) followed by g_S = sum_S Zt r (k + 1 entries), S being the samples with a phenotype.
struct GlmScoreBeta {
	double b[PGH_GLM_MAX_COVAR + 1];
};
// Partial sums per entry of hg: a fixed shape, so hg is a function of y, z and beta alone.
constexpr uint32_t kGlmScoreNullParts = 64;
// One Newton evaluation at beta.  y: n_out doubles (NaN = missing), z: n_out x kp doubles, output-sample order.
// Leaves r = y - mu (NaN without a phenotype) and w = mu (1 - mu) at r_raw / w_raw[sel ? sel[i] : i] (the raw samples
// outside `sel` are not written), and hg.  part: kGlmScoreNullParts x (entries of hg) doubles of scratch.
hipError_t LaunchGlmScoreNull(uint32_t n_out, const double *y, const double *z, uint32_t kp, uint32_t k,
                              const GlmScoreBeta &beta, const uint32_t *sel, double *r_raw, double *w_raw, double *part,
                              double *hg, hipStream_t stream);
// For the rows v_first + i (i < nv) of `sv`, sparse or held in the dense form: sums[i][kp + 6] = {n, sum x, sum x^2,
// U0, A, c_0 .. c_kp} and hgn[i] = H_N then g_N in hg's layout (the sums of the file's header comment).
// r, w: sv.sample_ct doubles in RAW sample order, NaN r = no phenotype or outside the subset; z: sv.sample_ct x kp
// doubles, raw sample-major.  n_y: the samples with a phenotype.
hipError_t LaunchGlmScoreSparse(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *r, const double *w,
                                const double *z, uint32_t kp, uint32_t k, uint32_t n_y, const double *hg, double *sums,
                                double *hgn, hipStream_t stream);
// What the solve kernel leaves for pgh_glm_score_sparse_spa and pgh_glm_score_multi_spa (all null: nothing, the launch
// of pgh_glm_score_sparse and pgh_glm_score_multi).
// t[i][kp + 3] = {H_N^-1 c (kp + 1 doubles, zero past k), U, V} for the fitted rows; p_spa[i] = rows[i].p (NaN when the
// row is not fitted) and state[i] = 0 for every row.
struct GlmScoreSpaOut {
	double *t = nullptr, *p_spa = nullptr;
	uint8_t *state = nullptr;
};
// The rows from the sums.  null_status: PGH_GLM_OK, or the errcode that every row not decided by its own counts gets.
hipError_t LaunchGlmScoreSolve(uint32_t nv, const double *sums, uint32_t kp, uint32_t k, const double *hgn,
                               int null_status, pgh_glm_row *rows, hipStream_t stream,
                               const GlmScoreSpaOut &spa = GlmScoreSpaOut());

// ---- pgh_glm_score_multi (glm_score_dense.hip): the score test over 2-bit rows for a block of phenotypes ----
// At most kGlmScoreDensePb phenotypes share a column block; the contraction's workgroup owns kGlmScoreDenseTileV
// variants x kGlmScoreDenseTileC columns.  No number depends on either, on the block's size or on the chunk.
constexpr uint32_t kGlmScoreDensePb = 64;
constexpr uint32_t kGlmScoreDenseTileV = 128;
constexpr uint32_t kGlmScoreDenseTileC = 64;
// The column block of pb phenotypes: ld doubles per sample row, the first n_xblocks 16-column blocks taken against x
// (phenotype j: r, w, w Zt_1 .. w Zt_k from column j (k + 2)), the rest against x^2 (phenotype j: w at
// 16 n_xblocks + j).  It holds 64 * ceil(sample_ct / 64) rows in RAW sample order.
struct GlmScoreDenseCols {
	uint32_t n_xblocks, ld;
};
GlmScoreDenseCols GlmScoreDenseLayout(uint32_t pb, uint32_t k);
// z[i][j] = z0[i][j] - mz[j] (n_out x kp; mz: kp doubles on the device)
hipError_t LaunchGlmScoreDenseCentre(uint32_t n_out, uint32_t kp, const double *z0, const double *mz, double *z,
                                     hipStream_t stream);
// Phenotype j's columns of the block `b` of pb phenotypes (ALL ZERO before its first phenotype is written), from
// LaunchGlmScoreNull's r_raw / w_raw and the centred covariates z (output-sample order): 0.0 outside S or the subset.
hipError_t LaunchGlmScoreDenseColumns(uint32_t n_out, const uint32_t *sel, const double *r_raw, const double *w_raw,
                                      const double *z, uint32_t kp, uint32_t k, uint32_t pb, uint32_t j, double *b,
                                      hipStream_t stream);
// For the local rows v0 + i (i < nv) of `view` and the block's phenotypes p < pb: sums[p][i][kp + 6] and hgn[p][i] in
// LaunchGlmScoreSparse's layouts, ready for LaunchGlmScoreSolve phenotype by phenotype.  mask: per phenotype
// 4 * ceil(sample_ct / 64) words, bit 2 (s & 15) of word s >> 4 set iff raw sample s is in S_p; n_y[p] = |S_p|.
// z0: the UNCENTRED covariates in raw-sample order (sample_ct x kp), mz: pb x kp means (LaunchGlmScoreDenseCentre's),
// hg: pb x (entries of hg).  nmiss: pb x nv words of scratch.
hipError_t LaunchGlmScoreDense(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask, const uint32_t *n_y,
                               uint32_t pb, const double *b, const double *z0, const double *mz, uint32_t kp,
                               uint32_t k, const double *hg, double *sums, uint32_t *nmiss, double *hgn,
                               hipStream_t stream);
// LaunchGlmScoreDense's last step alone: hgn[p][i] from the missing calls (code 3) of the rows v0 + i of `view` and
// nmiss[p][i] = how many of them lie in S_p.  The other arguments are LaunchGlmScoreDense's.
hipError_t LaunchGlmScoreDenseCorr(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask,
                                   const uint32_t *nmiss, uint32_t pb, const double *b, const double *z0,
                                   const double *mz, uint32_t kp, uint32_t k, const double *hg, double *hgn,
                                   hipStream_t stream);

// ---- pgh_glm_score_multi_dosage (glm_score_dense_dosage.hip): the same over variants with a dosage track ----
// LaunchGlmScoreDense's sums[p][i][kp + 6] and hgn[p][i] for the nt listed variants vlist[i] (rows of `view`, each with
// a track in `dos`), with x = the explicit dosage / 16384 where there is one and the call otherwise.  u16 and eff are
// scratch: GlmScoreDosageRowBytes(sample_ct) bytes per listed variant in all, 128 ceil(sample_ct / 64) of them in u16
// and 16 ceil(sample_ct / 64) in eff, both 16-byte aligned.  The other arguments are LaunchGlmScoreDense's.
struct DosageView;
uint64_t GlmScoreDosageRowBytes(uint32_t sample_ct);
hipError_t LaunchGlmScoreDenseDosage(const RowView &view, const DosageView &dos, const uint32_t *vlist, uint32_t nt,
                                     const uint32_t *mask, const uint32_t *n_y, uint32_t pb, const double *b,
                                     const double *z0, const double *mz, uint32_t kp, uint32_t k, const double *hg,
                                     uint16_t *u16, uint8_t *eff, double *sums, uint32_t *nmiss, double *hgn,
                                     hipStream_t stream);

// ---- pgh_glm_score_sparse_multi (glm_score_sparse_multi.hip): the score test from a sparse row's entries for a block
// of phenotypes ----
// At most kGlmScoreSparsePb phenotypes share a pair block and a walk of the entries.  No number depends on the block's
// size, on a phenotype's place in it or on the chunk.
constexpr uint32_t kGlmScoreSparsePb = 64;
// The pair block of pb phenotypes: pair[s][j] = (r, w) of raw sample s and block phenotype j, sample_ct x pb double2.
// Clear sets every pair to (NaN, 0): outside S_j or the subset.
hipError_t LaunchGlmScoreSparsePairClear(uint32_t sample_ct, uint32_t pb, double *pair, hipStream_t stream);
// Phenotype j's pairs of the subset's samples from LaunchGlmScoreNull's r_raw / w_raw.
hipError_t LaunchGlmScoreSparsePairs(uint32_t n_out, const uint32_t *sel, const double *r_raw, const double *w_raw,
                                     uint32_t pb, uint32_t j, double *pair, hipStream_t stream);
// For the rows v_first + i (i < nv) of `sv`, sparse or held in the dense form, and the block's phenotypes p < pb:
// sums[p][i][kp + 6] and hgn[p][i] in LaunchGlmScoreSparse's layouts, ready for LaunchGlmScoreSolve phenotype by
// phenotype.  n_y[p] = |S_p|; z0: the UNCENTRED covariates in raw-sample order (sample_ct x kp); mz: pb x kp means over
// S_p, the ones the null fits' covariates were centred on; hg: pb x (entries of hg).  nlist: nv words of scratch.
hipError_t LaunchGlmScoreSparseMulti(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *pair,
                                     const uint32_t *n_y, uint32_t pb, const double *z0, const double *mz, uint32_t kp,
                                     uint32_t k, const double *hg, double *sums, uint32_t *nlist, double *hgn,
                                     hipStream_t stream);

// ---- pgh_glm_score_sparse_spa (glm_score_spa.hip): saddlepoint p-values of the score test's rows ----
// Bytes of the private stash one workgroup of the workgroup form needs for `sample_ct` samples (a pair of doubles each).
inline uint64_t GlmScoreSpaStashPerGroup(uint32_t sample_ct) {
	return 16ull * (sample_ct ? sample_ct : 1u);
}
// For the rows v_first + i (i < nv) of `sv` that are fitted with |stat| > cutoff: p_spa[i] and state[i] = 1, or
// state[i] = 2 with p_spa[i] left as it is; the other rows are not touched.  r, w, z: LaunchGlmScoreSparse's; rows, t:
// LaunchGlmScoreSolve's.  stash: n_groups x GlmScoreSpaStashPerGroup bytes, whatever they hold.  Nothing in the
// output depends on n_groups (>= 1).
hipError_t LaunchGlmScoreSpa(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *r, const double *w,
                             const double *z, uint32_t kp, const pgh_glm_row *rows, const double *t,
                             double cutoff, uint32_t n_groups, void *stash, double *p_spa, uint8_t *state,
                             hipStream_t stream);

// ---- the work lists of the pair block's follow-ups (glm_score_sparse_lists.hpp) ----
// Elements of a workgroup of the list kernels, and the tiles of a chunk of n_rows = nv * pb (variant, phenotype) rows.
constexpr uint32_t kGlmScoreSparseListTile = 2048;
inline uint64_t GlmScoreSparseListTiles(uint64_t n_rows) {
	return (n_rows + kGlmScoreSparseListTile - 1) / kGlmScoreSparseListTile;
}
// Words of tile_ct for such a chunk: two counts per tile, then the two lists' lengths.
inline uint64_t GlmScoreSparseMultiTileWords(uint64_t n_rows) {
	return 2 * GlmScoreSparseListTiles(n_rows) + 2;
}

// ---- pgh_glm_score_sparse_multi_spa (glm_score_sparse_multi_spa.hip): saddlepoint p-values of the pair block's rows ----
// For the rows (phenotype p < pb, chunk variant i < nv) at p * nv + i that are fitted with |stat| > cutoff: p_spa and
// state = 1, or state = 2 with p_spa left as it is; the other rows are not touched.  sv, v_first, nv, pair, pb, z0, mz
// and kp are LaunchGlmScoreSparseMulti's; rows and t ([pb][nv][kp + 3]) are LaunchGlmScoreSolve's, phenotype by
// phenotype.  list_wave, list_group: nv * pb words each and tile_ct: GlmScoreSparseMultiTileWords words, whatever
// they hold (the applied rows of either form, listed first).  n_wave_groups: the workgroups of the wave form's grid;
// stash: n_groups x GlmScoreSpaStashPerGroup bytes, whatever they hold.  Nothing in the output depends on
// n_wave_groups or n_groups (both >= 1).
hipError_t LaunchGlmScoreSparseMultiSpa(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *pair,
                                        uint32_t pb, const double *z0, const double *mz, uint32_t kp,
                                        const pgh_glm_row *rows, const double *t, double cutoff, uint32_t *list_wave,
                                        uint32_t *list_group, uint32_t *tile_ct, uint32_t n_wave_groups,
                                        uint32_t n_groups, void *stash, double *p_spa, uint8_t *state,
                                        hipStream_t stream);

// ---- pgh_glm_score_sparse_firth (glm_score_sparse_firth.hip): approximate Firth estimates of the score test's rows ----
// For every row v_first + i (i < nv) of `sv`: firth[i], the contract's triple and state (the score row's beta, se and p
// with state 0 where the row is not fitted or |stat| <= cutoff).  r: LaunchGlmScoreSparse's; rows: LaunchGlmScoreSolve's.
// stash: n_groups x GlmScoreSpaStashPerGroup bytes, whatever they hold.  Nothing in the output depends on n_groups
// (>= 1).
hipError_t LaunchGlmScoreSparseFirth(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *r,
                                     const pgh_glm_row *rows, double cutoff, uint32_t n_groups, void *stash,
                                     pgh_glm_firth_row *firth, hipStream_t stream);

// ---- pgh_glm_score_sparse_multi_firth (glm_score_sparse_multi_firth.hip): approximate Firth estimates of the pair
// block's rows ----
// For every row (phenotype p < pb, chunk variant i < nv) at p * nv + i: firth[p * nv + i], the contract's triple and
// state (the score row's beta, se and p with state 0 where the row is not fitted or |stat| <= cutoff).  sv, v_first, nv,
// pair and pb are LaunchGlmScoreSparseMulti's; rows are LaunchGlmScoreSolve's, phenotype by phenotype.  list_wave,
// list_group, tile_ct, n_wave_groups, n_groups and stash are LaunchGlmScoreSparseMultiSpa's.  Nothing in the output
// depends on n_wave_groups or n_groups (both >= 1).
hipError_t LaunchGlmScoreSparseMultiFirth(const SparseView &sv, uint32_t v_first, uint32_t nv, const double *pair,
                                          uint32_t pb, const pgh_glm_row *rows, double cutoff, uint32_t *list_wave,
                                          uint32_t *list_group, uint32_t *tile_ct, uint32_t n_wave_groups,
                                          uint32_t n_groups, void *stash, pgh_glm_firth_row *firth,
                                          hipStream_t stream);

// ---- pgh_glm_score_multi_spa (glm_score_dense_spa.hip): saddlepoint p-values of the dense route's rows ----
// For the rows (phenotype p < pb, chunk variant i < nv) at p * nv + i that are fitted with |stat| > cutoff: p_spa and
// state = 1, or state = 2 with p_spa left as it is; the other rows are not touched.  view, v0, nv, mask, pb, b, z0, mz,
// kp, k and sums are LaunchGlmScoreDense's (sums as it left them); rows and t ([pb][nv][kp + 3]) are
// LaunchGlmScoreSolve's, phenotype by phenotype.  stash: n_groups x GlmScoreSpaStashPerGroup bytes, whatever they
// hold.  Nothing in the output depends on n_groups (>= 1).
hipError_t LaunchGlmScoreDenseSpa(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask, uint32_t pb,
                                  const double *b, const double *z0, const double *mz, uint32_t kp, uint32_t k,
                                  const double *sums, const pgh_glm_row *rows, const double *t, double cutoff,
                                  uint32_t n_groups, void *stash, double *p_spa, uint8_t *state, hipStream_t stream);

// ---- pgh_glm_score_multi_dosage_spa (glm_score_dense_dosage_spa.hip): the same for variants with a dosage track ----
// LaunchGlmScoreDenseSpa for the rows (phenotype p < pb, listed variant i < nt) at p * nt + i of the chunk that
// LaunchGlmScoreDenseDosage has just expanded: u16 and sums as it left them, rows and t ([pb][nt][kp + 3]) as
// LaunchGlmScoreSolve did.  view gives sample_ct; its rows are not read.  The base is 2 where sum x > n and else 0, the
// entries are the samples of N whose value is not exactly the base, and V_rest is 0 where every sample of N is an entry.
hipError_t LaunchGlmScoreDenseDosageSpa(const RowView &view, const uint16_t *u16, uint32_t nt, const uint32_t *mask,
                                        uint32_t pb, const double *b, const double *z0, const double *mz, uint32_t kp,
                                        uint32_t k, const double *sums, const pgh_glm_row *rows, const double *t,
                                        double cutoff, uint32_t n_groups, void *stash, double *p_spa, uint8_t *state,
                                        hipStream_t stream);

// ---- pgh_glm_score_multi_firth (glm_score_dense_firth.hip): approximate Firth estimates of the dense route's rows ----
// For every row (phenotype p < pb, chunk variant i < nv) at p * nv + i: firth[p * nv + i], the contract's triple and
// state (the score row's beta, se and p with state 0 where the row is not fitted or |stat| <= cutoff).  view, v0, nv,
// mask, pb, b and k are LaunchGlmScoreDense's; rows are LaunchGlmScoreSolve's, phenotype by phenotype.  stash: n_groups
// x GlmScoreSpaStashPerGroup bytes, whatever they hold.  Nothing in the output depends on n_groups (>= 1).
hipError_t LaunchGlmScoreDenseFirth(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask, uint32_t pb,
                                    const double *b, uint32_t k, const pgh_glm_row *rows, double cutoff,
                                    uint32_t n_groups, void *stash, pgh_glm_firth_row *firth, hipStream_t stream);

// ---- pgh_glm_score_multi_dosage_firth (glm_score_dense_dosage_firth.hip): the same for variants with a dosage track ----
// LaunchGlmScoreDenseFirth for the rows (phenotype p < pb, listed variant i < nt) at p * nt + i of the chunk that
// LaunchGlmScoreDenseDosage has just expanded: u16 as it left them, rows as LaunchGlmScoreSolve did.  view gives
// sample_ct; its rows are not read.  The entries are the samples of N whose value is not exactly 0, x = value / 16384.
// Every one of the nt x pb rows of firth is written.
hipError_t LaunchGlmScoreDenseDosageFirth(const RowView &view, const uint16_t *u16, uint32_t nt, const uint32_t *mask,
                                          uint32_t pb, const double *b, uint32_t k, const pgh_glm_row *rows,
                                          double cutoff, uint32_t n_groups, void *stash, pgh_glm_firth_row *firth,
                                          hipStream_t stream);

// ---- pgh_burden_sparse (burden_sparse.hip): the linear fit's sums of a weighted burden per variant set ----
// What the kernel leaves per set beside its sums row.
struct BurdenAux {
	double c;           // c_s = sum w_m val(b_m)
	double sum_d;       // sums[s][1] again, for the row's mean
	uint32_t n_nonzero; // samples with a phenotype and d_i != 0.0
	uint32_t touched;   // samples with a phenotype and an entry in some member
};
// Bytes of the private vector one workgroup needs for `sample_ct` samples (a double and a visited mark each).
uint64_t BurdenScratchPerGroup(uint32_t sample_ct);
// For the sets s < n_sets (CSR: set_off / set_vidx name LOCAL rows of sv, weight may be null = 1.0):
// sums[s][kp+4] = {n_y, sum d, sum d^2, sum d y, sum d z_j} in LaunchGlmSums' layout, aux[s], and x_const[s] = 1
// iff min d == max d over the n_y samples with a phenotype (LaunchGlmLinearSolve's x_const).  y, z: raw-sample order,
// as for LaunchGlmSparse.  scratch: n_groups x BurdenScratchPerGroup bytes, ALL ZERO on entry and on exit;
// counter: one uint32, zero on entry.  Nothing in the output depends on n_groups (>= 1).
hipError_t LaunchBurdenSparse(const SparseView &sv, uint32_t n_sets, const uint64_t *set_off, const uint32_t *set_vidx,
                              const double *weight, const double *y, const double *z, uint32_t kp, uint32_t k,
                              uint32_t n_y, uint32_t n_groups, void *scratch, uint32_t *counter, double *sums,
                              BurdenAux *aux, uint8_t *x_const, hipStream_t stream);

// ---- pgh_skat_sparse (skat_sparse.hip): the cross-product sums of a set's members under the score test's null model ----
struct SkatSetCounts {
	uint32_t n_carriers; // samples with a phenotype and an entry in some member
	uint32_t n_nonzero;  // (membership, entry) pairs of such samples with d != 0
};
// Doubles of one set of m memberships in `out`: packed upper A (row-major), C (m x (kp + 1)), U0 (m).
inline uint64_t SkatSetDoubles(uint64_t m, uint32_t kp) {
	return m * (m + 1) / 2 + m * (kp + 1) + m;
}
// For the sets s < n_sets (CSR as for LaunchBurdenSparse; no set holds more than PGH_SKAT_MAX_SET memberships), at
// out + out_off[s]: A_jl = sum_i w_i d_ij d_il (j <= l), c_j = sum_i w_i d_ij [1, z_i] and U0_j = sum_i d_ij r_i, the
// sums of the file's header comment; and counts[s].  r, w, z: LaunchGlmScoreSparse's (raw-sample order, NaN r = not in
// S).  scratch: n_groups x BurdenScratchPerGroup bytes, ALL ZERO on entry and on exit; counter: one uint32, zero on
// entry.  Nothing in the output depends on n_groups (>= 1).
hipError_t LaunchSkatSparse(const SparseView &sv, uint32_t n_sets, const uint64_t *set_off, const uint32_t *set_vidx,
                            const double *r, const double *w, const double *z, uint32_t kp, uint32_t k,
                            uint32_t n_groups, void *scratch, uint32_t *counter, const uint64_t *out_off, double *out,
                            SkatSetCounts *counts, hipStream_t stream);

} // namespace pgh
