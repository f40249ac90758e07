/*
 * pgenhip.h -- C ABI of libpgenhip: the MI355X (gfx950) replacement for the
 * plink-ng pgenlib calls on PlinkingDuck's .pgen decode-and-analyse hot path.
 *
 * Every entry point names the reference interface it replaces (file:line into
 * teaguesterling/plinking_duck).  Conventions, all taken from pgenlib's own:
 *   - every call returns an int status (PGH_OK == 0) and, where it can fail for
 *     a reason worth reporting, writes a NUL-terminated message into a caller
 *     buffer of PGH_ERRBUF_LEN bytes (pgenlib: PglErr + errstr_buf[kPglErrstrBufBlen]);
 *   - no exception, torch type or C++ type crosses this boundary;
 *   - the caller owns every output buffer; handles are opaque;
 *   - a pgh_dataset is immutable after creation and may be read concurrently
 *     by any number of scan threads; a pgh_reader belongs to one thread
 *     (pgenlib: one PgenReader per thread, src/plink_freq.cpp:342-390);
 *   - sample subsets follow pgenlib semantics: a bitmask over the raw samples,
 *     outputs compacted to the included samples in ascending file order
 *     (src/plink_common.cpp:1222-1250).
 *
 * Pointers named d_* are device (HBM) pointers owned by the caller; `stream`
 * is a hipStream_t passed as void* (NULL = HIP's default stream).  The
 * *_dev entry points only enqueue work; the host-buffer forms run on a stream
 * the library keeps for the calling thread, synchronise and copy the result
 * back.  Entry points that need device scratch keep one block per calling
 * thread, device and stream (grown on demand, released when the thread ends);
 * nothing is allocated from HIP's stream-ordered pool (hipMallocAsync), which
 * was seen to lose kernel-written data on this runtime.
 */
#ifndef PGENHIP_H_
#define PGENHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGH_ERRBUF_LEN 256

enum {
	PGH_OK = 0,
	PGH_ERR_OPEN = 1,        /* file cannot be opened/read      (IOException at the shell) */
	PGH_ERR_FORMAT = 2,      /* malformed or unsupported .pgen  (IOException)              */
	PGH_ERR_ARG = 3,         /* bad argument / out of range     (InvalidInputException)    */
	PGH_ERR_DEVICE = 4,      /* HIP runtime failure             (IOException)              */
	PGH_ERR_NOMEM = 5,
	PGH_ERR_UNSUPPORTED = 6  /* reserved: a track kind no path decodes (none at present: multiallelic tracks are stepped over, phased-dosage tracks are not read, as PgrGetD does not read them) */
};

typedef struct pgh_dataset pgh_dataset; /* packed 2-bit genotype matrix resident in HBM */
typedef struct pgh_subset pgh_subset;   /* sample-include mask, staged on the device    */
typedef struct pgh_reader pgh_reader;   /* per-scan-thread view (stream + staging)      */

typedef struct pgh_info {
	uint32_t raw_variant_ct;   /* pgfi.raw_variant_ct  (src/plink_freq.cpp:184) */
	uint32_t raw_sample_ct;    /* pgfi.raw_sample_ct   (src/plink_freq.cpp:185) */
	uint32_t variant_begin;    /* first variant resident on this device         */
	uint32_t variant_end;      /* one past the last resident variant            */
	uint32_t has_dosage;       /* gflags & kfPgenGlobalDosagePresent (src/plink_freq.cpp:201) */
	uint32_t has_phase;        /* gflags & kfPgenGlobalHardcallPhasePresent     */
	uint32_t max_record_bytes; /* max_vrec_width (src/plink_freq.cpp:193-197)   */
	uint32_t record_bytes;     /* ceil(N/4): bytes of one normalised 2-bit record */
	uint64_t pitch_bytes;      /* device row stride of one record               */
	uint32_t vrtype_hist[8];   /* number of records per main-track type (vrtype & 7) */
	int32_t device;            /* HIP device ordinal                            */
	uint32_t dosage_variant_ct; /* resident variants that carry a dosage track (vrtype & 0x60) */
	uint64_t dosage_value_ct;   /* explicit dosages held for them                */
} pgh_info;

/* ---- library / device --------------------------------------------------- */

/* Version string "pgenhip <n> gfx950". */
const char *pgh_version(void);
/* Number of visible HIP devices (0 without a GPU).  Never fails. */
int pgh_device_count(void);
/* Select the device used by datasets created afterwards from this thread. */
int pgh_set_device(int device, char *errbuf);

/* ---- dataset lifecycle --------------------------------------------------- */

/* Replaces PreinitPgfi + PgfiInitPhase1 + PgfiInitPhase2 + PgrInit
 * (src/plink_freq.cpp:168-208,344-390; same sequence in pgen_reader.cpp:227-266,
 * plink_hardy/missing/score/pca).  Parses the header and record tables, expands
 * every record of [variant_begin, variant_end) to a plain 2-bit row and leaves
 * the rows resident in HBM.  variant_end == UINT32_MAX means "to the last
 * variant".  pgi_path may be NULL (then "<pgen_path>.pgi" is tried for mode 0x20). */
int pgh_open(const char *pgen_path, const char *pgi_path, uint32_t variant_begin, uint32_t variant_end,
             pgh_dataset **out, char *errbuf);

/* Header probe only: no device work, works without a GPU (bind-time use:
 * src/plink_freq.cpp:168-208). */
int pgh_probe(const char *pgen_path, const char *pgi_path, pgh_info *out, char *errbuf);

/* The host half of pgh_open on its own: expand the records of [variant_begin,
 * variant_end) to plain 2-bit rows in HOST memory (row r at rows + r*row_stride,
 * row_stride >= ceil(N/4), pad bytes zeroed).  No device work; used by ingest
 * pipelines that stage rows themselves and by the CPU-only tests. */
int pgh_normalize_range_host(const char *pgen_path, const char *pgi_path, uint32_t variant_begin,
                             uint32_t variant_end, uint8_t *rows, size_t row_stride, char *errbuf);

/* Dataset over caller-supplied plain 2-bit rows in HOST memory (row v at
 * rows + v*row_stride, ceil(N/4) meaningful bytes each). */
int pgh_from_host_rows(const uint8_t *rows, size_t row_stride, uint32_t variant_ct, uint32_t sample_ct,
                       pgh_dataset **out, char *errbuf);

/* Seeded synthetic dataset written directly into HBM (BASELINE.md section 3:
 * p_v ~ U(0.01,0.5), g ~ Binomial(2,p_v), missing with probability
 * missing_rate).  Variant v of the generator lands in row v - variant_begin, so
 * ranks that own disjoint variant ranges hold slices of one global matrix. */
int pgh_synth_create(uint32_t variant_begin, uint32_t variant_end, uint32_t sample_ct, uint64_t seed,
                     double missing_rate, pgh_dataset **out, char *errbuf);
/* The same fileset with a dosage track (vrtype 0x60: presence bits + uint16 values) behind every record:
 * each sample explicit with probability dosage_rate, values uniform on 0..32768.  Ingest benchmark input. */
int pgh_synth_write_dosage_files(const char *prefix, uint32_t variant_ct, uint32_t sample_ct, uint64_t seed,
                                 double missing_rate, double dosage_rate, char *errbuf);
/* Gives every resident variant of a dataset without dosage tracks a seeded synthetic one:
 * each sample carries an explicit dosage with probability `rate`, values uniform on 0..32768.
 * Benchmark input of the shape `plink2 --import-dosage` leaves behind (vrtype 0x60). */
int pgh_synth_add_dosage(pgh_dataset *ds, double rate, uint64_t seed, char *errbuf);
/* The same generator on the host: one record (ceil(N/4) bytes) of variant v. */
int pgh_synth_record_host(uint32_t v, uint32_t sample_ct, uint64_t seed, double missing_rate, uint8_t *out);
/* Writes <prefix>.pgen (mode 0x10, vrtype-0 records), .pvar and .psam. */
int pgh_synth_write_files(const char *prefix, uint32_t variant_ct, uint32_t sample_ct, uint64_t seed,
                          double missing_rate, char *errbuf);

/* Copy resident rows [v_begin, v_end) back to HOST memory as plain 2-bit rows
 * (row r at rows + r*row_stride, ceil(N/4) bytes each). */
int pgh_copy_rows_to_host(const pgh_dataset *ds, uint32_t v_begin, uint32_t v_end, uint8_t *rows, size_t row_stride,
                          char *errbuf);

int pgh_get_info(const pgh_dataset *ds, pgh_info *out);
/* Device pointer of resident row 0 (pitch in pgh_info.pitch_bytes). */
const void *pgh_device_rows(const pgh_dataset *ds);
/* CleanupPgr + CleanupPgfi (src/plink_freq.cpp:109-115). */
void pgh_close(pgh_dataset *ds);

/* ---- sparse-resident datasets ---------------------------------------------
 * The reference's plinking_sample_counts_sparse route (PgrGetDifflistOrGenovec, src/pfile_reader.cpp:3364-3430)
 * touches only a rare variant's carriers.  pgh_open_sparse keeps each variant of [variant_begin, variant_end) in ONE
 * of two forms: sparse -- a base code (the row's majority class, any of 0..3) plus one uint32 entry
 * sample << 2 | code per sample whose call differs from it, ascending -- or dense, the plain 2-bit row in a compact
 * pool.  max_minor == 0: a row is sparse iff its entries take fewer bytes than its dense row (4 m < pitch), so the
 * genotype payload never exceeds pgh_open's; max_minor > 0: sparse iff m <= max_minor.  Counts never depend on the
 * choice.  Hardcalls only (dosage and phase tracks are stepped over; pgh_info still reports them), one device,
 * fewer than 2^30 samples (PGH_ERR_ARG otherwise).  Served by pgh_get_info, pgh_close, pgh_counts_range(_dev),
 * pgh_sample_counts(_dev), pgh_copy_rows_to_host, pgh_subset_* and the entry points made for this form:
 * pgh_glm_sparse, pgh_glm_score_sparse(_spa), pgh_burden_sparse, pgh_skat_sparse and pgh_score_sparse; every other entry point that reads
 * rows (pgh_score,
 * pgh_score_dev and the score plans among them) returns PGH_ERR_ARG, and pgh_device_rows returns NULL. */
typedef struct pgh_sparse_info {
	uint32_t sparse_variant_ct; /* variants held as base + entries                                  */
	uint32_t dense_variant_ct;  /* variants held as 2-bit rows in the pool                          */
	uint64_t entry_ct;          /* entries of the sparse variants                                   */
	uint64_t resident_bytes;    /* device bytes: entries + pool + 12 bytes of index per variant     */
	uint64_t dense_bytes;       /* what pgh_open holds for the same rows (pitch x variants)          */
	uint32_t base_hist[4];      /* sparse variants per base code (hom-ref, het, hom-alt, missing)    */
} pgh_sparse_info;
int pgh_open_sparse(const char *pgen_path, const char *pgi_path, uint32_t variant_begin, uint32_t variant_end,
                    uint32_t max_minor, pgh_dataset **out, char *errbuf);
/* PGH_ERR_ARG for a dataset that is not sparse-resident. */
int pgh_get_sparse_info(const pgh_dataset *ds, pgh_sparse_info *out);
/* pgh_open_sparse calls made by this process so far (a diagnostic, like pgh_tally_passes_started). */
uint64_t pgh_sparse_opens_started(void);

/* ---- shard groups: one process, several devices -------------------------------
 * The reference parallelises inside ONE process and merges per-thread partial sums under a mutex
 * (src/plink_score.cpp:657-664, src/plink_missing.cpp:614-619, src/plink_pca.cpp:940-954).  A shard group is
 * the same shape with devices in the place of threads: contiguous, ascending variant ranges of one file, one
 * resident dataset per device, behind ONE pgh_dataset handle.  Every host-buffer entry point of this header
 * accepts a group handle: per-variant outputs (pgh_counts_range, pgh_unpack_range, pgh_dosage_*, the pgh_get_*
 * reader calls) are filled shard by shard with no exchange; per-sample outputs are reduced per shard on its device
 * and merged across devices -- pgh_score's partials by an RCCL reduce onto the first shard, pgh_pca's by an RCCL
 * all-reduce per pass, each on the shards' own streams over xGMI (one communicator per shard, made at the first
 * collective; shards that share a device fall back to device-to-device copies and a sum on the first shard's
 * device), pgh_missing_per_sample / pgh_sample_counts (4 bytes per sample) on the host; pgh_ld_pairs computes the
 * pairs that straddle a shard boundary on a scratch dataset built from the rows they name.  Subsets and readers
 * created on a group handle are groups themselves.  The *_dev / plan entry points and pgh_device_rows take one
 * device's dataset: hand them pgh_shard(group, k).
 *
 * pgh_open_sharded: pgh_open of n_devices near-equal ranges of [variant_begin, variant_end), concurrently, shard k
 * on devices[k] (a device may be named more than once).  pgh_group_create: a group over datasets the caller made
 * (pgh_open / pgh_synth_create / pgh_from_host_rows, each with pgh_set_device in effect); it takes ownership:
 * pgh_close(group) closes them. */
int pgh_open_sharded(const char *pgen_path, const char *pgi_path, uint32_t variant_begin, uint32_t variant_end,
                     const int *devices, uint32_t n_devices, pgh_dataset **out, char *errbuf);
int pgh_group_create(pgh_dataset *const *shards, uint32_t n_shards, pgh_dataset **out, char *errbuf);
/* 1 when the group's per-sample merges run as RCCL collectives (one communicator per shard, made by this call if
 * the group had none yet: shards on distinct devices and librccl loadable), 0 when they use device-to-device copies
 * (shards sharing a device, PGH_GROUP_RCCL=0) or ds is not a group. */
int pgh_group_uses_rccl(const pgh_dataset *ds);
/* 0 for a plain dataset. */
uint32_t pgh_shard_count(const pgh_dataset *ds);
const pgh_dataset *pgh_shard(const pgh_dataset *ds, uint32_t k);

/* ---- sample subsets ------------------------------------------------------ */

/* Replaces BuildSampleSubset / PgrSetSampleSubsetIndex (src/plink_common.cpp:1222-1250,
 * src/plink_freq.cpp:393-397).  sample_include: ceil(N/64) words, bit s = sample s kept.  Bits at and above N are
 * ignored (the subset clears them in its own copy): all-ones words mean every sample.
 *
 * The empty subset (no bit below N set, pgh_subset_size() == 0) is accepted, and every entry point that takes it
 * answers one of three ways, never with PGH_ERR_DEVICE:
 *   - per-variant integer products are zeros: pgh_counts_range(_dev), the tally pass (its HWE ln p is that of zero
 *     counts), pgh_dosage_sums(_dev), pgh_ld_pairs(_dev), the reader's pgh_get_counts;
 *   - per-sample products are zero-length, PGH_OK with nothing written: pgh_unpack_range, pgh_unpack_samples,
 *     pgh_dosage_unpack(_samples), the reader's per-sample calls, pgh_sample_counts, pgh_missing_per_sample,
 *     pgh_tally_sample_missing, pgh_score, pgh_score_counts, pgh_score_sparse, pgh_het.  A score plan made for it scores
 *     nothing: pgh_score_run_dev zeroes its (raw-sample) outputs;
 *   - everything that fits or compares samples returns PGH_ERR_ARG, "the sample subset is empty ...", before any
 *     launch: pgh_glm, pgh_glm_multi, pgh_glm_sparse, pgh_glm_score_sparse(_spa), pgh_burden_sparse, pgh_skat_sparse, pgh_pca,
 *     pgh_pca_sharded, pgh_king_counts, pgh_king_table, pgh_grm, pgh_ld_window_sums, pgh_ld_prune, pgh_ld_scores. */
int pgh_subset_create(const pgh_dataset *ds, const uint64_t *sample_include, pgh_subset **out, char *errbuf);
uint32_t pgh_subset_size(const pgh_subset *ss);
void pgh_subset_destroy(pgh_subset *ss);

/* ---- variant ranges and variant lists -------------------------------------
 * Index convention.  A variant index is GLOBAL: the variant's number in the file, whatever range the dataset holds
 * (pgh_info.variant_begin / variant_end; for a shard group the union of its shards' ranges).  This goes for every
 * v_begin / v_end, every variant_begin / n_var, every vidx, vidx_a / vidx_b and the reader's vidx.  The one exception
 * is the set_vidx of pgh_burden_sparse and pgh_skat_sparse, which is DATASET-LOCAL: 0 names the first resident variant.
 *
 * Outside the resident range.  A range that is reversed or not inside [variant_begin, variant_end), and a list with
 * an entry outside it, is PGH_ERR_ARG before anything is launched, with a message that says "outside the resident
 * range" (the set tests: "is not below the dataset's variant count"); every output is untouched.
 *
 * The two forms.  Where an entry point takes (variant_begin, n_var, vidx), vidx == NULL means the n_var variants from
 * variant_begin on, and vidx != NULL means the n_var listed variants (variant_begin is then ignored).  The list
 * variant_begin, variant_begin + 1, .. gives what the range form gives, integer outputs bit for bit.  The same global
 * variants give the same answer from every dataset that holds them -- the whole file, a window of it, a shard group --
 * integer outputs bit for bit, floating outputs to rounding, and bit for bit where a row is stated to be a function of
 * its variant (or its set) alone.
 *
 * Order, repeats and the empty list, per entry point ("call order" = the order of the list; output row or column i
 * belongs to list entry i):
 *   pgh_sample_counts             any order; a repeated variant counts each time; n_var == 0: PGH_OK, every count 0
 *   pgh_dosage_sums / _unpack     any order; a repeated variant is a repeated output row; n_variants == 0: PGH_OK,
 *                                 nothing written
 *   pgh_unpack_samples,           any order; a repeated variant is a repeated output column; n_variants == 0: PGH_OK,
 *   pgh_dosage_unpack_samples     nothing written
 *   pgh_score, pgh_score_counts,  any order (the sums do not depend on it beyond rounding; allele_ct not at all); a
 *   the score plan,               repeated variant is scored each time, with the weights, flip and counts of each of
 *   pgh_score_sparse              its entries; n_scored == 0: PGH_OK, every sum and allele_ct 0
 *   pgh_ld_pairs(_dev)            the pairs in any order, a variant with itself and a repeated pair included (a
 *                                 repeated pair is a repeated output row); n_pairs == 0: PGH_OK, nothing written
 *   pgh_pca, pgh_pca_sharded      any order; a repeated variant is a repeated row of X (with the center / inv_stdev of
 *                                 each of its entries); fewer than (n_pcs + 1) 2 n_pcs variants, n_var == 0 included:
 *                                 PGH_ERR_ARG ("too few variants ...").  pgh_pca_streamed alone wants ascending order.
 *   pgh_king_counts / _table,     any order; a repeated variant counts each time (pgh_grm: with the freq of each of
 *   pgh_grm                       its entries); n_var == 0: PGH_ERR_ARG ("n_var must be at least 1")
 *   pgh_het                       any order, the same bytes from each; a repeated variant counts each time (with the freq
 *                                 of each of its entries); n_var == 0: PGH_OK, every row {0.0, NaN, 0, 0, 0}
 *   pgh_ld_window_sums            any order; a repeated variant is a repeated row and column of the rectangle;
 *                                 n_var == 0: PGH_ERR_ARG (no rectangle fits: "variant rectangle ... is empty")
 *   pgh_ld_prune, pgh_ld_scores   STRICTLY INCREASING, hence no repeats: anything else is PGH_ERR_ARG ("the variant
 *                                 list must be strictly increasing"); n_var == 0: PGH_ERR_ARG ("n_var must be at
 *                                 least 1")
 *   pgh_burden_sparse,            set_vidx (dataset-local) in any order; a repeated variant counts each time (SKAT: a
 *   pgh_skat_sparse               repeated row and column of Phi); an empty set is a row with PGH_GLM_CONST_ALLELE
 * The range-only entry points (pgh_counts_range, pgh_missing_per_sample, pgh_unpack_range, pgh_glm, pgh_glm_multi,
 * pgh_glm_sparse, pgh_glm_score_sparse(_spa)) accept v_begin == v_end inside the resident range: PGH_OK with no
 * per-variant row written; pgh_missing_per_sample's per-sample counts are then 0.
 * tests/test_variant_shapes.py pins every line of this section. */

/* ---- batched device calls (the fast path of the table functions) -------- */

/* PgrGetCounts over a variant range (src/plink_freq.cpp:482, plink_hardy.cpp:510,
 * plink_pca.cpp:394, pgen_reader.cpp:673,864): out[v - v_begin] = {hom_ref, het,
 * hom_alt, missing} over the (subset of) samples.  subset may be NULL. */
int pgh_counts_range(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                     uint32_t (*out)[4], char *errbuf);
int pgh_counts_range_dev(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                         void *d_out, void *stream, char *errbuf);

/* plink_freq's arithmetic on the device (src/plink_freq.cpp:495-544), from a
 * device counts array: d_alt_freq[i] = (het + 2 hom_alt) / (2 obs) as double, NaN
 * where the reference emits NULL (obs == 0); d_obs_ct[i] = 2 obs (int32). */
int pgh_freq_from_counts_dev(const void *d_counts, uint32_t n, void *d_alt_freq, void *d_obs_ct, void *stream,
                             char *errbuf);

/* PgrGetMissingness + PopcountWords (src/plink_missing.cpp:479-486) is column 3
 * of pgh_counts_range.  The per-sample form replaces the phase-1 accumulation of
 * plink_missing sample mode (src/plink_missing.cpp:585-619):
 * out[k] = number of variants in [v_begin, v_end) at which included sample k is missing. */
int pgh_missing_per_sample(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                           uint32_t *out, char *errbuf);
/* d_out: uint32[raw_sample_ct] (raw order, no compaction), zeroed by the call. */
int pgh_missing_per_sample_dev(const pgh_dataset *ds, uint32_t v_begin, uint32_t v_end, void *d_out, void *stream,
                               char *errbuf);

/* plink_freq + plink_hardy + plink_missing (variant and sample mode) off ONE pass over
 * the rows: d_counts uint32[v_end-v_begin][4] as pgh_counts_range_dev (all samples) and
 * d_missing uint32[raw_sample_ct] as pgh_missing_per_sample_dev, each byte read once. */
int pgh_fused_tally_dev(const pgh_dataset *ds, uint32_t v_begin, uint32_t v_end, void *d_counts, void *d_missing,
                        void *stream, char *errbuf);

/* ---- tally pass: one asynchronous walk of the matrix that serves several table functions ----------
 * The reference's plink_freq, plink_hardy and plink_missing each scan the file for themselves
 * (src/plink_freq.cpp:434-488, src/plink_hardy.cpp:472-516, src/plink_missing.cpp:463-486 and :585-619), one
 * blocking PgrGetCounts / PgrGetMissingness per variant.  A tally pass enqueues the whole range at once -- batch by
 * batch on streams it owns, results landing in pinned host memory the pass keeps -- and returns; scan threads then
 * wait only for the rows they are about to emit, while the device works on the batches behind them.  A pass is
 * immutable once its products have landed and may be read by any number of threads, so a caller that keeps it
 * (the shells cache it per dataset, subset and range) serves later functions without touching the matrix again:
 * the three scans of BASELINE config 3 cost one read of each byte.
 *
 * Products (PGH_TALLY_*): COUNTS is always made: {hom_ref, het, hom_alt, missing} per variant over the (subset of)
 * samples.  SAMPLE_MISSING: per included sample, the number of variants of the pass at which it is missing
 * (src/plink_missing.cpp:599-609); without a subset it comes out of the same kernel pass as the counts
 * (k_fused_tally), with one it is a second sweep.  HWE / HWE_MIDP: plink2::HweLnP of every variant's counts
 * (src/plink_hardy.cpp:52-79), on a side stream behind each batch's tally.
 * pgh_tally_start enqueues the products named in `products`; pgh_tally_request adds products later (a no-op for the
 * ones already there; HWE then runs from the resident counts, SAMPLE_MISSING re-reads the rows).  Both only enqueue.
 * pgh_tally_wait blocks until the named products of variants [v_begin, v_end) have landed (SAMPLE_MISSING: the whole
 * pass).  The accessors return pass-owned pinned arrays indexed by (variant - the pass's v_begin); rows are valid
 * once waited for.  Accepts a shard group: every shard walks its own range on its own device. */
typedef struct pgh_tally pgh_tally;
enum { PGH_TALLY_COUNTS = 1, PGH_TALLY_SAMPLE_MISSING = 2, PGH_TALLY_HWE = 4, PGH_TALLY_HWE_MIDP = 8 };
int pgh_tally_start(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                    uint32_t products, pgh_tally **out, char *errbuf);
int pgh_tally_request(pgh_tally *t, uint32_t products, char *errbuf);
int pgh_tally_wait(pgh_tally *t, uint32_t products, uint32_t v_begin, uint32_t v_end, char *errbuf);
const uint32_t (*pgh_tally_counts(const pgh_tally *t))[4];
/* ln p of the exact test per variant (product HWE or HWE_MIDP), NULL when that product was never requested. */
const double *pgh_tally_hwe_lnp(const pgh_tally *t, uint32_t midp);
/* Waits for the product; out[k] for the n_out included samples in ascending file order. */
int pgh_tally_sample_missing(pgh_tally *t, uint32_t *out, char *errbuf);
/* Waits for everything the pass has enqueued, then releases it. */
void pgh_tally_destroy(pgh_tally *t);
/* Passes started by this process so far (a diagnostic: the tests assert that plink_hardy after plink_freq starts none). */
uint64_t pgh_tally_passes_started(void);

/* Page-locked host memory for callers that hand output buffers to the host-buffer entry points again and again
 * (read_pgen's chunk buffers: a device-to-host copy into pinned memory runs at the link's rate and without a
 * staging hop).  Portable across the node's devices.  pgh_host_free(NULL) is a no-op. */
int pgh_host_alloc(size_t bytes, void **out, char *errbuf);
void pgh_host_free(void *p);

/* Call-scoped device work blocks of 64 MB and more (plink_pca's transposed and tile-major matrices, wide score
 * outputs) are kept on a per-device free list between calls instead of going back to the driver -- hipMalloc of
 * tens of gigabytes costs seconds once a process has done it a few times.  The list holds at
 * most PGH_BLOCK_CACHE_GB (environment, default 64, 0 = keep nothing) per device, is emptied by pgh_close and
 * whenever an allocation of the library fails, and by this call: a host that wants the memory back for its own
 * allocations right now.  No reference counterpart (the reference allocates no device memory). */
void pgh_trim_device_cache(void);

/* PgrGet + GenoarrToBytesMinus9 over a variant range (src/pgen_reader.cpp:727-733)
 * plus the validity fill of the ARRAY/LIST child (src/pgen_reader.cpp:1009-1047).
 * out: int8 [v_end-v_begin][n_out] with n_out = subset size or N; a missing call is
 * stored as missing_code (-9 for pgenlib parity, 0 for the DuckDB child vector).
 * validity (may be NULL): ceil(n_out/64) words per variant, bit set = non-missing. */
int pgh_unpack_range(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end, int8_t *out,
                     uint64_t *validity, int missing_code, char *errbuf);
/* d_out row stride = out_pitch bytes (>= n_out, multiple of 16); d_validity row
 * stride = ceil(n_out/64) words; either may be NULL.  Of a d_out row the call writes the
 * first ceil(n_out/16)*16 bytes (what lies past n_out there is unspecified) and leaves the
 * rest of the pitch untouched. */
int pgh_unpack_range_dev(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                         void *d_out, size_t out_pitch, void *d_validity, int missing_code, void *stream,
                         char *errbuf);

/* Measurement aid for pgh_unpack_range_dev: a bare kernel with that kernel's traffic shape -- a lane reads 16 bytes
 * and writes 64 + 8 -- and no arithmetic, on the current device.  d_src: n_vec x 16 B, d_dst: n_vec x 64 B, d_val:
 * n_vec x 8 B; n_vec a multiple of 64 (a wave stores whole 4 KiB tiles of d_dst; PGH_ERR_ARG otherwise).  bench.py
 * times it beside the unpack and reports it as roofline.store_ceiling. */
int pgh_probe_unpack_shape_dev(const void *d_src, size_t n_vec, void *d_dst, void *d_val, void *stream, char *errbuf);

/* plink_score phase 1 (src/plink_score.cpp:575-654) for n_scored variants and
 * n_cols weight columns (the reference has one; BASELINE config 4 uses 16).
 *   vidx[i]      variant index, in any order, repeats allowed (see "variant ranges and variant lists" above; the
 *                reference walks its score file in variant order, src/plink_score.cpp:407-408, and a file with
 *                dosage tracks is scored in an order of the plan's own)
 *   weights      [n_scored][n_cols] doubles, row-major
 *   flip[i]      scored allele is REF (dosage 2 - alt)      (may be NULL)
 *   mode         PGH_SCORE_MEAN_IMPUTE | _NO_MEAN_IMPUTATION | _CENTER
 * Outputs over the included samples (ascending file order):
 *   score_sum    [n_out][n_cols], dosage_sum [n_out], allele_ct [n_out].
 * dosage_sum (d_dosage_sum in the device forms) may be NULL when NAMED_ALLELE_DOSAGE_SUM is not
 * wanted: the one-column kernel then looks up 8-byte instead of 16-byte entries and does half
 * the adds (the reference always accumulates it; skipping it is projection pushdown). */
enum { PGH_SCORE_MEAN_IMPUTE = 0, PGH_SCORE_NO_MEAN_IMPUTATION = 1, PGH_SCORE_CENTER = 2 };
int pgh_score(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_scored, const uint32_t *vidx,
              const double *weights, const uint8_t *flip, uint32_t n_cols, int mode, double *score_sum,
              double *dosage_sum, uint32_t *allele_ct, char *errbuf);
/* pgh_score for a caller that already holds the scored variants' class tallies -- a tally pass's rows
 * (pgh_tally_counts), as plink_score after plink_freq on the same file and subset does: counts[i] =
 * {hom_ref, het, hom_alt, missing} of vidx[i] over the included samples.  The means / variances the reference
 * derives per variant (src/plink_score.cpp:598-620) then cost no read of the rows; NULL = pgh_score. */
int pgh_score_counts(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_scored, const uint32_t *vidx,
                     const double *weights, const uint8_t *flip, uint32_t n_cols, int mode, const uint32_t (*counts)[4],
                     double *score_sum, double *dosage_sum, uint32_t *allele_ct, char *errbuf);
/* Device form: raw-sample order (no compaction), outputs are caller-owned device
 * buffers of raw_sample_ct rows, overwritten -- every row, the rows of samples outside
 * the subset too.  Those are not zeroed: the kernels score every raw sample, so such a
 * row holds that sample's own sums and allele count under the per-variant means,
 * variances and skips of the included samples.  A caller that wants the included
 * samples reads the rows the subset names (the host forms compact exactly those). */
int pgh_score_dev(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_scored, const uint32_t *vidx,
                  const double *weights, const uint8_t *flip, uint32_t n_cols, int mode, void *d_score_sum,
                  void *d_dosage_sum, void *d_allele_ct, void *stream, char *errbuf);

/* The same in two steps, for callers that score the same weight set repeatedly or
 * want an enqueue-only launch: the plan uploads vidx / weights / flip once and
 * runs the tally + table kernels; pgh_score_run_dev only enqueues the memsets
 * and the accumulate kernels on `stream`.
 * The first plan over a dataset with sparse dosage tracks also builds that
 * dataset's entry records (4 bytes per explicit dosage, resident until
 * pgh_close; skipped without error when they do not fit). */
typedef struct pgh_score_plan pgh_score_plan;
int pgh_score_plan_create(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_scored, const uint32_t *vidx,
                          const double *weights, const uint8_t *flip, uint32_t n_cols, int mode,
                          pgh_score_plan **out, char *errbuf);
int pgh_score_run_dev(const pgh_score_plan *plan, void *d_score_sum, void *d_dosage_sum, void *d_allele_ct,
                      void *stream, char *errbuf);
void pgh_score_plan_destroy(pgh_score_plan *plan);

/* ---- dosage tracks ------------------------------------------------------------
 * A file's explicit dosages (vrtype bits 0x20 / 0x40 / 0x60) are brought to one resident form at
 * pgh_open: a presence bit per sample and the present samples' uint16 values, 16384 per ALT copy.
 * A sample without an explicit dosage takes its hardcall (0 / 16384 / 32768); one with neither is
 * missing.  pgh_score scores dosage-bearing variants from these values as the reference does
 * through PgrGetD (src/plink_score.cpp:586-652).
 *
 * pgh_dosage_sums: PgrGetDCounts (src/plink_freq.cpp:475-480, :525-535): per variant
 *   sums[i] = {sum of dosages, sum of squared dosages, samples with a dosage or a call}
 * on the 16384 scale over the included samples: alt dosage sum = sums[0], ref = 2*16384*sums[2] - sums[0],
 * MaCH r2 from the first two moments.  Variants: [variant_begin, variant_begin + n_variants), or the
 * n_variants listed in vidx when vidx != NULL.
 *
 * pgh_dosage_unpack: PgrGetD + Dosage16ToDoublesMinus9 (src/pgen_reader.cpp:694-705): out[i][k] =
 * dosage of output sample k at variant i as a double, -9.0 when missing; rows of n_out doubles. */
int pgh_dosage_sums(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_variants,
                    const uint32_t *vidx, uint64_t (*sums)[3], char *errbuf);
int pgh_dosage_unpack(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_variants,
                      const uint32_t *vidx, double *out, char *errbuf);
/* Enqueue-only forms over [v_begin, v_end): d_sums = uint64[n][3]; d_out = double rows of out_stride elements. */
int pgh_dosage_sums_dev(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                        void *d_sums, void *stream, char *errbuf);
int pgh_dosage_unpack_dev(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                          void *d_out, size_t out_stride, void *stream, char *errbuf);

/* read_pfile orient := 'sample' (src/pfile_reader.cpp:1560-1720: the reference pre-reads every effective
 * variant with PgrGet / PgrGetD into a variants x samples matrix and emits one row per sample): the matrix
 * sample-major, out[k][j] = call (0/1/2, missing -> missing_code) or dosage (-9.0 = missing) of output sample
 * k at listed variant vidx[j]; rows of n_variants elements. */
int pgh_unpack_samples(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_variants, const uint32_t *vidx,
                       int8_t *out, int missing_code, char *errbuf);
int pgh_dosage_unpack_samples(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_variants,
                              const uint32_t *vidx, double *out, char *errbuf);

/* read_pfile's sample-orient aggregate (src/pfile_reader.cpp:3308-3400, the streaming
 * accumulate_dense loop): counts[k] = {hom_ref, het, hom_alt, missing} of output sample k over
 * the variants [variant_begin, variant_begin + n_var) or, with vidx != NULL, the n_var listed
 * variants.  Three column-tally passes over the packed rows (het, hom-alt, missing), hom-ref by
 * subtraction as the reference derives it at emit time. */
int pgh_sample_counts(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                      const uint32_t *vidx, uint32_t (*counts)[4], char *errbuf);
/* Enqueue-only form over all raw samples: d_classes = uint32[3][ceil(N/64)*64] receives the het,
 * hom-alt and missing tallies (hom-ref = variants - the three). */
int pgh_sample_counts_dev(const pgh_dataset *ds, uint32_t variant_begin, uint32_t variant_end, void *d_classes,
                          void *stream, char *errbuf);

/* plink_ld's per-pair sums (src/plink_ld.cpp:52-84, ComputeLdStats' sample loop): for each
 * pair p of variants (vidx_a[p], vidx_b[p]) over the samples at which both calls are present
 * (and which the subset keeps),
 *   sums[p] = {n, sum_a, sum_b, sum_ab, sum_a2, sum_b2}
 * as exact integers; r2 / D' follow from them in the caller (the reference's double arithmetic
 * on the same values).  The two rows are reduced with popcounts on the packed planes -- no
 * PgrGet + per-sample decode.  Pairs that share an anchor and walk consecutive partners (the
 * windowed scan's order) read the anchor row once per four partners. */
int pgh_ld_pairs(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_pairs, const uint32_t *vidx_a,
                 const uint32_t *vidx_b, uint32_t (*sums)[6], char *errbuf);
/* Device-output form: sums land in d_sums (uint32[n_pairs][6], zeroed by the call), computed on `stream`;
 * vidx_a / vidx_b stay host arrays.  The task list built from them goes up through the calling thread's own
 * pinned staging buffer, stream-ordered; a thread's next call waits for this one's kernel before it reuses
 * that buffer.  The kernel refuses a task the host cannot have built (no partners, rows outside the resident
 * matrix) and reports it: pgh_ld_pairs_status -- and the thread's next pgh_ld_pairs(_dev) call, and
 * pgh_ld_pairs itself -- wait for the launch and return PGH_ERR_DEVICE if that happened. */
int pgh_ld_pairs_dev(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_pairs, const uint32_t *vidx_a,
                     const uint32_t *vidx_b, void *d_sums, void *stream, char *errbuf);
int pgh_ld_pairs_status(char *errbuf);

/* plink_pca's randomized subspace iteration (src/plink_pca.cpp:630-1080): n_pcs + 1
 * passes of Y = X G1 (Step A) and G1 = X^T Y / M (Step B) over the n_var effective
 * variants, thin SVD of the M x (n_pcs+1)*2*n_pcs Krylov block, then B = X^T U and
 * its thin SVD.  X is never materialised: both contractions read the packed 2-bit
 * rows and normalise on the fly (x = (g - center) * inv_stdev, missing -> 0).
 *   vidx/center/inv_stdev  effective variants and their norms, as the reference's
 *                          bind computes them (src/plink_pca.cpp:392-416)
 *   g1_init                [n_out][2*n_pcs] row-major start matrix (src/plink_pca.cpp:517-523)
 *   eigenvalues            [n_pcs]  (S^2 / n_var)
 *   eigenvectors           [n_out][n_pcs] row-major, defined up to sign
 * Everything tall stays on the device: the Krylov block is orthonormalised by block
 * Gram-Schmidt (any orthonormal basis of its column space serves where the reference
 * takes the left singular vectors), and the final SVD goes through the small
 * (n_pcs+1)*2*n_pcs square Gram matrix, whose eigen-decomposition runs on the host. */
int pgh_pca(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_var, const uint32_t *vidx,
            const double *center, const double *inv_stdev, uint32_t n_pcs, const double *g1_init,
            double *eigenvalues, double *eigenvectors, char *errbuf);

/* The same over variant shards, one process per GPU (variants
 * sharded, one exchange per pass).  Each rank passes ITS shard's effective variants
 * (n_var may be 0) and the job-wide count n_var_total; X is split by rows, so G2 = X^T Y,
 * the Gram matrices of the Krylov block and B = X^T U are sums of per-shard terms.
 * The library leaves the transport to the host: `allreduce` must sum `count` doubles at
 * device pointer `d_buf` in place over all ranks.  Work that produces d_buf has been
 * enqueued on `stream`; the callback either enqueues its collective there (RCCL:
 * ncclAllReduce(d_buf, d_buf, count, ncclDouble, ncclSum, comm, stream)) or synchronises
 * the stream itself before a host transport, and returns 0 on success.  Calls happen in
 * the same order with the same counts on every rank: n_pcs of N*2k, O(n_pcs) small Gram
 * blocks, one of N*qq.  g1_init must be identical on all ranks; eigenvalues and
 * eigenvectors come back replicated.  allreduce == NULL requires n_var_total == n_var. */
typedef int (*pgh_allreduce_fn)(void *ctx, void *d_buf, uint64_t count, void *stream);
int pgh_pca_sharded(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_var, const uint32_t *vidx,
                    const double *center, const double *inv_stdev, uint64_t n_var_total, uint32_t n_pcs,
                    const double *g1_init, pgh_allreduce_fn allreduce, void *allreduce_ctx, double *eigenvalues,
                    double *eigenvectors, char *errbuf);

/* pgh_pca over a .pgen that is NOT resident -- a file beyond the HBM budget: the effective variants (ascending) are cut
 * into windows whose file span is at most `window_variants`, and every pass of the algorithm (n_pcs + 1 power
 * iterations, then phase 3: the reference walks its 240-variant blocks once per pass too, src/plink_pca.cpp:632-676)
 * opens the windows one after the other on the current device, uses each for that pass's two contractions and closes
 * it; the Krylov block (n_var x (n_pcs + 1) 2 n_pcs doubles) stays on the device throughout.  The file is therefore
 * read n_pcs + 2 times.  sample_include: the subset's bit mask over the raw samples, or NULL.  Same results as
 * pgh_pca on a resident dataset of the same variants up to the order of FP64 additions. */
int pgh_pca_streamed(const char *pgen_path, const char *pgi_path, const uint64_t *sample_include, uint32_t n_var,
                     const uint32_t *vidx, const double *center, const double *inv_stdev, uint32_t n_pcs,
                     const double *g1_init, uint64_t window_variants, double *eigenvalues, double *eigenvectors,
                     char *errbuf);

/* ---- per-variant calls mirroring pgenlib -------------------------------- */

/* PgrInit + PgrSetSampleSubsetIndex per scan thread (src/plink_freq.cpp:381-397). */
int pgh_reader_create(const pgh_dataset *ds, const pgh_subset *subset, pgh_reader **out, char *errbuf);
void pgh_reader_destroy(pgh_reader *rd);
/* PgrGet (src/pgen_reader.cpp:727): subset-compacted 2-bit genovec, ceil(n_out/32) words. */
int pgh_get_2bit(pgh_reader *rd, uint32_t vidx, uint64_t *genovec);
/* PgrGetCounts (src/plink_freq.cpp:482). */
int pgh_get_counts(pgh_reader *rd, uint32_t vidx, uint32_t out[4]);
/* PgrGetMissingness (src/plink_missing.cpp:479): ceil(n_out/64) words, bit set = missing. */
int pgh_get_missingness(pgh_reader *rd, uint32_t vidx, uint64_t *bits);
/* PgrGet + GenoarrToBytesMinus9 (src/plink_freq.cpp:463-469): {0,1,2,-9}. */
int pgh_get_int8(pgh_reader *rd, uint32_t vidx, int8_t *out);
/* PgrGetD + Dosage16ToDoublesMinus9 (src/plink_score.cpp:586-596): -9.0 = missing.  One row of
 * pgh_dosage_unpack through the reader's stream. */
int pgh_get_dosage_f64(pgh_reader *rd, uint32_t vidx, double *out);
/* PgrGetP (src/pgen_reader.cpp:715): genovec as pgh_get_2bit plus the
 * phasepresent / phaseinfo bitarrays (ceil(n_out/64) words each, zero for
 * variants without a phase track).  The track was expanded into two resident bit rows at pgh_open. */
int pgh_get_phased(pgh_reader *rd, uint32_t vidx, uint64_t *genovec, uint64_t *phasepresent, uint64_t *phaseinfo);
/* PgrGet + GenoarrToBytesMinus9 over a range (pgh_unpack_range), enqueue-and-return on the reader's stream: calls
 * and validity words of [v_begin, v_end) go to the caller's PAGE-LOCKED buffers (pgh_host_alloc), which must stay
 * untouched until pgh_reader_unpack_wait(rd, slot).  `slot` (0 or 1) names which of the reader's two staging blocks
 * the launch uses: a scan thread keeps chunk k + 1 on its way (kernel + copy over the host link) while it fills
 * its output vector from chunk k -- the reference's scan decodes and copies one variant at a time
 * (src/pgen_reader.cpp:727-733, :1009-1047).  A slot is reused only after it has been waited for. */
int pgh_reader_unpack_start(pgh_reader *rd, int slot, uint32_t v_begin, uint32_t v_end, int8_t *out, uint64_t *validity,
                            int missing_code);
int pgh_reader_unpack_wait(pgh_reader *rd, int slot);
const char *pgh_reader_error(const pgh_reader *rd);

/* ---- plink_glm: per-variant association regressions ---------------------------
 * pgh_glm replaces plink_glm's per-variant loop (src/plink_glm.cpp:1250-1273: PgrGetD + Dosage16ToDoublesMinus9,
 * then ComputeLinearRegression or ComputeLogisticRegression, :917-1215) for the variants [v_begin, v_end) of ds
 * (a dataset or a shard group).  One output row per variant, in variant order.
 *   phenotype   one double per output sample (subset order), NaN = missing
 *   covariates  n_covar x n_out doubles, covariate-major, all finite (n_covar <= PGH_GLM_MAX_COVAR)
 *   model       PGH_GLM_LINEAR or PGH_GLM_LOGISTIC (the bind-time 'auto' rule is the caller's)
 *   firth       logistic only: a failed or unfinished Newton fit is refitted with Firth's penalty
 * A variant's samples are those with a phenotype and a call (a dosage-track variant: a dosage or a call); its
 * genotype value is the ALT dosage.  The fits run in FP64 on the device; a variant's row does not depend on the
 * variants around it (tile, chunk or shard). */
#define PGH_GLM_MAX_COVAR 20
enum { PGH_GLM_LINEAR = 0, PGH_GLM_LOGISTIC = 1 };
enum {
	PGH_GLM_OK = 0,
	PGH_GLM_TOO_FEW_SAMPLES = 1,
	PGH_GLM_CONST_ALLELE = 2,
	PGH_GLM_ZERO_VARIANCE = 3,
	PGH_GLM_SINGULAR_MATRIX = 4,
	PGH_GLM_NO_CONVERGENCE = 5,
	PGH_GLM_SEPARATION = 6
};
typedef struct pgh_glm_row {
	double beta, se, stat, p, a1_freq; /* NaN where the reference leaves NULL                 */
	uint32_t obs_ct;
	uint8_t errcode;                   /* PGH_GLM_*                                           */
	uint8_t firth;                     /* 1: the row came from the Firth fallback (FIRTH_YN)  */
	uint8_t pad[2];
} pgh_glm_row;
int pgh_glm(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end, const double *phenotype,
            uint32_t n_covar, const double *covariates, int model, int firth, pgh_glm_row *out, char *errbuf);
/* pgh_glm for n_pheno phenotypes at once.  phenotypes: n_pheno x n_out doubles, phenotype-major, NaN = missing.
 * out: (v_end - v_begin) x n_pheno rows, variant-major: out[(v - v_begin) * n_pheno + p] is phenotype p's row
 * for variant v.  Every other argument means what it means for pgh_glm; n_pheno == 0 is PGH_ERR_ARG.
 * Each row is what pgh_glm returns for that phenotype alone: logistic and Firth rows bit for bit; linear rows with
 * the same errcode, obs_ct and a1_freq, and estimates that agree to rounding (the phenotypes of one missing-value
 * pattern share one walk of the rows, and their sums are accumulated in another order).  A row does not depend on
 * the other phenotypes of the call or on its place among them. */
int pgh_glm_multi(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                  uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                  int model, int firth, pgh_glm_row *out, char *errbuf);
/* pgh_glm's LINEAR fit for the variants [v_begin, v_end) of a SPARSE-RESIDENT dataset (pgh_open_sparse),
 * from the variants' entries: cost proportional to the samples that differ from a variant's base code.
 * Hardcalls only (pgh_open_sparse steps over dosage tracks).  Arguments, row layout, error codes and argument
 * checks are pgh_glm's.  A dataset that is not sparse-resident is PGH_ERR_ARG
 * ("needs a sparse-resident dataset").
 * A row has pgh_glm's errcode, obs_ct and a1_freq for the same file bit for bit, and estimates that agree to
 * rounding (its sums are accumulated over the entries, in another order); the rows of variants held in the dense
 * form (pgh_sparse_info.dense_variant_ct) are pgh_glm's bit for bit.  A row is a function of its variant's entries,
 * the phenotype, the covariates and the subset only: not of v_begin, the chunk or the rows around it, and the same
 * call returns the same bytes every time.  Logistic Wald fits and pgh_glm's full Firth fits over a sparse-resident
 * dataset are not offered (the logistic score test is: pgh_glm_score_sparse; its approximate Firth estimate is:
 * pgh_glm_score_sparse_firth).  Many phenotypes in one walk of the entries: pgh_glm_sparse_multi. */
int pgh_glm_sparse(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                   const double *phenotype, uint32_t n_covar, const double *covariates,
                   pgh_glm_row *out, char *errbuf);
/* pgh_glm_sparse for MANY PHENOTYPES in one walk of the entries of a SPARSE-RESIDENT dataset (pgh_open_sparse): up to
 * 64 quantitative phenotypes, each with its own missing-value pattern, share the reads of every entry word and
 * covariate row.  Arguments, argument checks and the layout of `out` are pgh_glm_multi's (model LINEAR): phenotypes is
 * [n_pheno][n_out], NaN = missing; covariates is covariate-major; out[(v - v_begin) * n_pheno + p] is phenotype p's row
 * for variant v.  A dataset that is not sparse-resident ("needs a sparse-resident dataset") and a shard group are
 * PGH_ERR_ARG with `out` untouched; v_begin == v_end is PGH_OK; a phenotype with every value missing is legal, its
 * rows are TOO_FEW_SAMPLES.
 * Each row is the row pgh_glm_sparse returns for that phenotype alone over the same dataset: errcode, obs_ct, firth (0)
 * and a1_freq bit for bit, beta, se, stat and p to rounding.  The rows of variants held in the dense form
 * (pgh_sparse_info.dense_variant_ct) are walked from their pool rows as base-0 rows and obey the same contract: to
 * rounding, not bit for bit against pgh_glm.  A row is a function of its variant's entries, its own phenotype, the
 * covariates and the subset only: not of the other phenotypes of the call, its place among them, n_pheno, the rows
 * around it, v_begin, the chunk, the window the dataset was opened with or the scratch budget, and the same call
 * returns the same bytes every time.
 * PGH_GLM_SCORE_SCRATCH_BYTES (environment, read at every call, default 6 GiB) bounds the device scratch that grows
 * with the phenotypes and variants in flight (8 bytes per raw sample and 8 per subset sample and block phenotype, then
 * the chunk's sums); the result does not depend on it.
 * Not offered: dosage tracks, shard groups, a table function. */
int pgh_glm_sparse_multi(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                         uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                         pgh_glm_row *out, char *errbuf);
/* The logistic SCORE TEST of every variant of [v_begin, v_end) of a SPARSE-RESIDENT dataset (pgh_open_sparse), from
 * the variants' entries: the covariates-only model is fitted once, and a variant then costs in proportion to the
 * samples that differ from its base code.  Arguments, argument checks, row layout and error codes are
 * pgh_glm_sparse's (hardcalls only, one row per variant; a shard group or a dataset that is not sparse-resident is
 * PGH_ERR_ARG, the latter "needs a sparse-resident dataset").  In addition every non-NaN phenotype value must be
 * exactly 0.0 or 1.0 (glm_model()'s 1/2 coding is the caller's to apply) and at least one case and one control must
 * have a phenotype; otherwise PGH_ERR_ARG ("phenotype must be 0 or 1", "no cases or no controls") and `out` is
 * untouched.
 *
 * Null model.  S = the output samples with a phenotype, n_y = |S|, Zt_i = [1, z_i1 .. z_ik] with the covariates
 * centred over S (the intercept absorbs the shift).  Logistic y ~ Zt over S by Newton steps from beta = 0 in FP64:
 * H = sum_S w Zt Zt', g = sum_S Zt (y - mu), delta = H^-1 g, w = mu (1 - mu).  The fit has converged after the first
 * step with max_j |delta_j| <= 1e-10; mu, w, r = y - mu, H and g_S are then recomputed at the final beta.  The
 * Cholesky of H fails on a pivot that is not positive or is at most 1e-10 of its own diagonal entry.  A pivot failure
 * at the first step (every w is 1/4: collinear covariates) gives every row not decided earlier SINGULAR_MATRIX; one
 * at a later step, a non-finite step, or no convergence after 25 steps gives NO_CONVERGENCE.  With n_y < k + 3 the
 * fit is skipped (every row is then TOO_FEW_SAMPLES).
 *
 * Per variant.  M = the samples of S whose call is missing, N = S without M, n = |N|, x_i = the ALT count.  The row is the
 * one-step efficient score of x given Zt over N:
 *   H_N = sum_N w Zt Zt'   g_N = sum_N Zt r   c = sum_N w x Zt   A = sum_N w x^2   U0 = sum_N x r
 *   t = H_N^-1 c   V = A - c't   U = U0 - t'g_N   beta = U / V   se = 1 / sqrt(V)   stat = U / sqrt(V)
 *   p = pgh_glm_p_from_z(stat)
 * U and V do not change when a multiple of a column of Zt is added to x, so the sums are taken with d = x - b for the
 * row's base code b (d = x under a missing-majority base), over the row's called entries alone; A is defined with d.
 * n, sum x and sum x^2 are integers, so obs_ct, a1_freq, TOO_FEW_SAMPLES (n < k + 3) and CONST_ALLELE (every called
 * value equal) are pgh_glm's with model = PGH_GLM_LOGISTIC for the same file, bit for bit.
 * Decisions, in order: TOO_FEW_SAMPLES; CONST_ALLELE; the null model's status; SINGULAR_MATRIX when the Cholesky of
 * [[H_N, c], [c', A]] fails the 1e-10 pivot rule (its last pivot is V, against A); otherwise the row is fitted.
 * ZERO_VARIANCE and SEPARATION are never produced and firth is 0.  Undecided fields are NaN; obs_ct is always filled
 * and a1_freq where pgh_glm fills it.  A row held in the dense form is treated as a base-0 row whose entries are its
 * samples with a code other than 0: the same formulas, the same contract.
 *
 * A row is a function of its variant's entries, the phenotype, the covariates and the subset only: not of v_begin,
 * the chunk, the window the dataset was opened with or the rows around it, and the same call returns the same bytes
 * every time, the null fit included.  Datasets opened with another max_minor hold other base codes; their rows agree
 * to rounding (1e-9 on the scale of the estimates), not bit for bit.
 * Saddlepoint p-values over this route: pgh_glm_score_sparse_spa.  Approximate Firth estimates over this route:
 * pgh_glm_score_sparse_firth.  Many phenotypes in one walk of the entries: pgh_glm_score_sparse_multi. */
int pgh_glm_score_sparse(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                         const double *phenotype, uint32_t n_covar, const double *covariates,
                         pgh_glm_row *out, char *errbuf);
/* The logistic score test of every variant of [v_begin, v_end) of a DENSE-RESIDENT dataset (pgh_open) for n_pheno
 * case/control phenotypes in one call: one null fit per phenotype, then one pass over the 2-bit rows per block of
 * phenotypes, as an FP64 matrix product on the matrix cores.  phenotypes, covariates, subset, the range and the layout
 * of `out` are pgh_glm_multi's: out[(v - v_begin) * n_pheno + p] is phenotype p's row for variant v.
 *
 * Row contract.  Each row is the row that pgh_glm_score_sparse's contract above defines, for that phenotype alone,
 * with d = x: the dense route has no base code.  The null model, its 1e-10 stopping rule, the pivot rule and the
 * 25-step cap, S, M, N, H_N, g_N, c, A, U0, t, V, U, beta, se, stat and p, and the order of the decisions
 * (TOO_FEW_SAMPLES; CONST_ALLELE; the null model's status; SINGULAR_MATRIX on the augmented Cholesky; otherwise
 * fitted) are the ones defined there; firth is 0.  obs_ct, a1_freq, TOO_FEW_SAMPLES and CONST_ALLELE equal pgh_glm's
 * with model = PGH_GLM_LOGISTIC for the same file, bit for bit.  A null fit that fails decides only its own
 * phenotype's rows.  Against pgh_glm_score_sparse over the same file the estimates agree to rounding (1e-9 on their
 * scale), with the same errcodes.
 *
 * A row is a function of its variant's calls, its own phenotype, the covariates and the subset only: not of the other
 * phenotypes of the call or its place among them, of v_begin, the variant chunk, the phenotype block, the window the
 * dataset was opened with or the scratch budget, and the same call returns the same bytes every time.
 *
 * PGH_ERR_ARG, `out` untouched: everything pgh_glm_multi refuses in the shared arguments (n_pheno == 0 included); a
 * non-NaN phenotype value other than 0.0 or 1.0 ("phenotype must be 0 or 1") or a phenotype without a case or a
 * control ("no cases or no controls"), each followed by the phenotype's index; a sparse-resident dataset ("needs a
 * dense-resident dataset"); a shard group (pass pgh_shard(group, k)); a dataset whose pgh_info.dosage_variant_ct is
 * not 0 ("hardcalls only": the x^2 sums are defined on calls).  v_begin == v_end is PGH_OK.
 *
 * PGH_GLM_SCORE_SCRATCH_BYTES (environment, read at every call, default 6 GiB) bounds the device scratch that grows
 * with the phenotypes and variants in flight; the result does not depend on it.
 * Saddlepoint p-values over this route: pgh_glm_score_multi_spa.  Approximate Firth estimates over this route:
 * pgh_glm_score_multi_firth (from carrier lists: pgh_glm_score_sparse_firth).  Many phenotypes over a sparse-resident
 * dataset: pgh_glm_score_sparse_multi, with saddlepoint p-values pgh_glm_score_sparse_multi_spa, with approximate Firth
 * estimates pgh_glm_score_sparse_multi_firth.  A dataset with dosage tracks: pgh_glm_score_multi_dosage.  Not offered:
 * a Firth-penalised null fit, Firth and saddlepoint in one call, shard groups, a table function. */
int pgh_glm_score_multi(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                        uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                        pgh_glm_row *out, char *errbuf);
/* pgh_glm_score_multi over a dense-resident dataset that may hold DOSAGE TRACKS (imputed panels).  Arguments, argument
 * checks, error texts, the layout of `out` and the refusals are pgh_glm_score_multi's, except that a dataset whose
 * pgh_info.dosage_variant_ct is not 0 is accepted.  On any refusal `out` is untouched; v_begin == v_end is PGH_OK.
 *
 * Row contract.  The row of (variant, phenotype) is the row of pgh_glm_score_sparse's contract with d = x, as
 * pgh_glm_score_multi's is, under pgh_glm's genotype rule (pgh_dosage_unpack's): for a variant with a track,
 * x_i = value / 16384 where sample i has an explicit dosage and the ALT count of its call otherwise; M = the samples of
 * S with neither a dosage nor a call; N = S \ M; A = sum_N w x^2.  A variant without a track has x = its calls.  The
 * null model, its stopping rule, the pivot rule, the order of the decisions and the NaN fields are unchanged; firth is 0.
 * Values lie on the 2^-14 grid, so n, sum x and sum x^2 over N are exact, and obs_ct, a1_freq, TOO_FEW_SAMPLES and
 * CONST_ALLELE equal pgh_glm's with model = PGH_GLM_LOGISTIC over the same file, bit for bit, a track that is constant
 * at an off-integer value included.  sum x^2 is exact only while sample_ct < 2^23 (8,388,608).
 * A variant without a track, whatever its neighbours carry, and a variant whose track restates its calls (value =
 * 16384 x call wherever there is a call, nothing elsewhere) get pgh_glm_score_multi's row for the same calls in a file
 * without tracks, bit for bit; a dataset without any track gets pgh_glm_score_multi's bytes.
 *
 * A row is a function of its variant's calls and track, its own phenotype, the covariates and the subset only: not of
 * the other phenotypes or its place among them, of v_begin, the variant chunk, the phenotype block, which other variants
 * carry tracks, the window the dataset was opened with or PGH_GLM_SCORE_SCRATCH_BYTES (which here also holds 144 bytes
 * per 64 samples for every variant in flight), and the same call returns the same bytes every time.
 * Saddlepoint p-values over tracks: pgh_glm_score_multi_dosage_spa.  Approximate Firth estimates over tracks:
 * pgh_glm_score_multi_dosage_firth.  Not offered: shard groups, a table function. */
int pgh_glm_score_multi_dosage(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                               uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                               pgh_glm_row *out, char *errbuf);
/* The logistic score test of every variant of [v_begin, v_end) of a SPARSE-RESIDENT dataset (pgh_open_sparse) for
 * n_pheno case/control phenotypes in one call: one null fit per phenotype, then one walk of the variants' entries per
 * block of at most 64 phenotypes, in which an entry's word and covariate row are read once for the block.  The
 * arguments and the layout of `out` are pgh_glm_score_multi's: phenotypes is [n_pheno][n_out], and
 * out[(v - v_begin) * n_pheno + p] is phenotype p's row for variant v.
 *
 * Row contract.  Each row is the row that pgh_glm_score_sparse's contract above defines, for that phenotype alone: the
 * base codes, d = x - b, M, C and N, the missing-majority rule, the rows held in the dense form treated as base-0 rows
 * and the order of the decisions are the ones defined there; firth is 0.  obs_ct, a1_freq, TOO_FEW_SAMPLES and
 * CONST_ALLELE equal pgh_glm's with model = PGH_GLM_LOGISTIC for the same file, bit for bit (the counts are integers
 * until they are stored).  The estimates agree with pgh_glm_score_sparse for the same phenotype to rounding (1e-9 on
 * their scale), with equal errcodes, not bit for bit: the sums are taken in another order (a row's entries in
 * consecutive segments of 1024, each one chain, added in ascending order).  A null fit that fails decides only its own
 * phenotype's rows.
 *
 * A row is a function of its variant's entries, its own phenotype, the covariates and the subset only: not of the
 * other phenotypes of the call or its place among them, of n_pheno, the phenotype block, the rows that share a wave or
 * a workgroup with it, v_begin, the variant chunk, the window the dataset was opened with or the scratch budget, and
 * the same call returns the same bytes every time.
 *
 * PGH_ERR_ARG, `out` untouched: everything pgh_glm_score_multi refuses in the shared arguments (n_pheno == 0, "phenotype
 * must be 0 or 1" and "no cases or no controls", each followed by the phenotype's index, included); a dataset that is
 * not sparse-resident ("needs a sparse-resident dataset"); a shard group (pass pgh_shard(group, k)).
 * v_begin == v_end is PGH_OK.
 *
 * PGH_GLM_SCORE_SCRATCH_BYTES (environment, read at every call, default 6 GiB) bounds the device scratch that grows
 * with the phenotypes and variants in flight (16 bytes per sample and block phenotype, then the chunk's sums); the
 * result does not depend on it.
 * Saddlepoint p-values over this route: pgh_glm_score_sparse_multi_spa.  Approximate Firth estimates over this route:
 * pgh_glm_score_sparse_multi_firth.  Quantitative phenotypes over this route: pgh_glm_sparse_multi.  Not offered:
 * dosage tracks, shard groups, a table function. */
int pgh_glm_score_sparse_multi(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                               uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                               pgh_glm_row *out, char *errbuf);
/* pgh_glm_score_sparse with a SADDLEPOINT p-value beside the normal one, for the rows the normal tail serves badly:
 * rare variants under an unbalanced case / control ratio (the "fast SPA" of Dey et al. 2017: the exact cumulant
 * generating function over the row's entries, a normal term for every other sample).  Arguments, argument checks and
 * error codes are pgh_glm_score_sparse's.  In addition spa_cutoff must be at least 0.1 (+infinity: never apply it;
 * NaN or a smaller value is PGH_ERR_ARG, "spa_cutoff must be at least 0.1"), and p_spa and spa_state, one element per
 * variant, must not be NULL.  On any error the outputs are untouched.
 *
 * out[i] is pgh_glm_score_sparse's row for the same arguments bit for bit; its p stays the normal p-value.
 * spa_state[i]: 0 = not applied (the row is not fitted, or |stat| <= spa_cutoff), 1 = applied, 2 = attempted and
 * failed.  p_spa[i]: NaN when the row is not fitted, out[i].p bit for bit in state 0 (fitted) and in state 2, the
 * saddlepoint p in state 1.
 *
 * Definition, in pgh_glm_score_sparse's notation (S, N, Zt, w, r, d = x - b, t = H_N^-1 c in the d parameterisation,
 * U, V).  mu_i = the null model's fitted mean, recovered from the staged residual: mu = r > 0 ? 1 - r : -r.
 * gt_i = d_i - Zt_i t for i in N (d_i = 0 for a sample that is not an entry).  E = the row's used called entries: the
 * samples of N that the row holds as entries.  A row held in the dense form counts as a base-0 row, so its E is its
 * called samples with a code other than 0; a missing-majority row (b = 3) has E = N.  V_E = sum_E w gt^2; V_rest = 0
 * by rule when b = 3, otherwise max(V - V_E, 0).
 *   K(s)   = sum_E [ln(1 - mu + mu e^(gt s)) - s mu gt] + V_rest s^2 / 2
 *   K'(s)  = sum_E gt (pi - mu) + V_rest s         pi = mu / (mu + (1 - mu) e^(-gt s))
 *   K''(s) = sum_E gt^2 pi (1 - pi) + V_rest       K'(0) = 0, K''(0) = V
 * evaluated with one exp of -|gt s| per entry (log1p / expm1 of it for K), so that nothing overflows or cancels for
 * large |gt s|.  For each of q+ = |U| and q- = -|U|, s^ is the root of K'(s^) = q, found by a safeguarded Newton
 * iteration: K' is increasing, the root has the sign of q; the bracket starts as [0, open), the first point is the
 * Newton step from 0, |q| / V; while the far side is open a step may not exceed 1/sqrt(V), doubling each time the
 * limit is used; once it is closed a Newton step that leaves the bracket is replaced by its midpoint.  The root is
 * taken when |delta s| sqrt(V) <= 1e-12 (or the bracket is that narrow, or |delta s| <= 2^-50 |s|: far out the
 * first bound is below the spacing of s), after at most 64 evaluations of K', K''.
 *   omega = sign(s^) sqrt(2 (s^ q - K(s^)))   nu = s^ sqrt(K''(s^))   tail = Phibar(|omega + ln(nu / omega) / omega|)
 *   p_spa = tail(q+) + tail(q-)
 * State 2: for either tail no root within the 64 evaluations, or 2 (s^ q - K) <= 0, or nu / omega <= 0, or anything
 * not finite.  With V_rest = 0 and q outside the support of the score there is no root, and the cap is the outcome.
 *
 * p_spa depends on the form a row is held in, because E does: datasets opened with another max_minor agree to
 * rounding only for the rows whose E is the same set, and within the quality of the approximation otherwise.  A row's
 * (out, p_spa, spa_state) is a function of its variant's entries, the phenotype, the covariates, the subset and
 * spa_cutoff only: not of v_begin, the chunk, the window the dataset was opened with or the rows around it, and the
 * same call returns the same bytes every time.  Many phenotypes in one walk of the entries, with this p-value:
 * pgh_glm_score_sparse_multi_spa. */
int pgh_glm_score_sparse_spa(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                             const double *phenotype, uint32_t n_covar, const double *covariates, double spa_cutoff,
                             pgh_glm_row *out, double *p_spa, uint8_t *spa_state, char *errbuf);
/* pgh_glm_score_multi with pgh_glm_score_sparse_spa's SADDLEPOINT p-value beside the normal one, for every (variant,
 * phenotype) row of the dense route.  Arguments, argument checks and error texts are pgh_glm_score_multi's.  In
 * addition spa_cutoff must be at least 0.1 (+infinity: never apply it; NaN or a smaller value is PGH_ERR_ARG,
 * "spa_cutoff must be at least 0.1"), and p_spa and spa_state must not be NULL ("null p_spa or spa_state"); they have
 * out's layout, element (v - v_begin) * n_pheno + p.  On any error all three outputs are untouched.  The refusals are the dense route's: a
 * sparse-resident dataset, a shard group, a dataset with dosage tracks (pgh_glm_score_multi_dosage_spa gives such a
 * dataset's rows and saddlepoint p-values: this entry's walk reads 2-bit rows).
 *
 * out is pgh_glm_score_multi's result for the same arguments bit for bit; its p stays the normal p-value.  spa_state
 * and p_spa mean what they mean for pgh_glm_score_sparse_spa: 0 = not applied (the row is not fitted: p_spa NaN; or
 * |stat| <= spa_cutoff: p_spa = out.p bit for bit), 1 = applied (p_spa is the saddlepoint p), 2 = attempted and failed
 * (p_spa = out.p bit for bit).
 *
 * Definition, in the notation of pgh_glm_score_sparse and pgh_glm_score_sparse_spa with d = x.  n0 and n2 are the
 * hom-ref and hom-alt calls among N, the phenotype's called samples; b = 2 if n2 > n0, otherwise 0 (an integer rule).
 * E = the samples of N with x != b.  gt_i = x_i - Zt_i t for i in N, which does not depend on b (shifting x by b shifts
 * t_0 by b); mu_i = r_i > 0 ? 1 - r_i : -r_i; V_E = sum_E w gt^2 and V_rest = max(V - V_E, 0).  A fitted row always has
 * a called sample with x = b (otherwise it would be CONST_ALLELE), so the sparse route's V_rest = 0 by rule does not
 * arise here.  Everything else is pgh_glm_score_sparse_spa's contract word for word: K, K', K'' with one
 * exp(-|gt s|) per entry; the safeguarded Newton iteration for q+ and q- = +-|U| from |q| / V with the 1/sqrt(V) step
 * cap that doubles; the three stopping rules and the cap of 64 evaluations; omega, nu and the two tails; the state-2
 * conditions.  Membership in S comes from the phenotype's non-NaN values and the subset.
 *
 * Against pgh_glm_score_sparse_spa over the same file, a row whose sparse base code equals b (and is not 3) has the
 * same E: the states agree and p_spa agrees to rounding.
 *
 * A row's (out, p_spa, spa_state) is a function of its variant's calls, its own phenotype, the covariates, the subset
 * and spa_cutoff only: not of the other phenotypes of the call or its place among them, of v_begin, the variant
 * chunk, the phenotype block, PGH_GLM_SCORE_SCRATCH_BYTES (which here also bounds the saddlepoint kernel's scratch) or
 * the grid, and the same call returns the same bytes every time. */
int pgh_glm_score_multi_spa(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                            uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                            double spa_cutoff, pgh_glm_row *out, double *p_spa, uint8_t *spa_state, char *errbuf);
/* pgh_glm_score_multi_dosage with pgh_glm_score_sparse_spa's SADDLEPOINT p-value beside the normal one: the saddlepoint
 * over a dense-resident dataset that may hold DOSAGE TRACKS.  Arguments, argument checks, error texts and the layout of
 * the three outputs are pgh_glm_score_multi_spa's, except that a dataset whose pgh_info.dosage_variant_ct is not 0 is
 * accepted: spa_cutoff must be at least 0.1 (+infinity: never apply it; NaN or a smaller value is PGH_ERR_ARG,
 * "spa_cutoff must be at least 0.1"), p_spa and spa_state must not be NULL ("null p_spa or spa_state").  The refusals
 * are pgh_glm_score_multi_dosage's: a sparse-resident dataset, a shard group, a phenotype that is not 0 / 1, a phenotype
 * without a case or a control.  On any refusal all three outputs are untouched; v_begin == v_end is PGH_OK.
 *
 * out is pgh_glm_score_multi_dosage's result for the same arguments bit for bit; its p stays the normal p-value.
 * spa_state and p_spa mean what they mean for pgh_glm_score_sparse_spa: 0 = not applied (the row is not fitted: p_spa
 * NaN; or |stat| <= spa_cutoff: p_spa = out.p bit for bit), 1 = applied (p_spa is the saddlepoint p), 2 = attempted and
 * failed (p_spa = out.p bit for bit).
 *
 * Definition, in the notation of pgh_glm_score_sparse and pgh_glm_score_sparse_spa with d = x and
 * pgh_glm_score_multi_dosage's genotype rule (x = value / 16384 where there is an explicit dosage, the call otherwise;
 * M = neither).  n, sum x and sum x^2 over N are that route's exact integers on the 2^-14 grid.  b = 2 if sum_N x > n,
 * otherwise 0: an exact comparison, and for a row of calls sum x - n = n2 - n0, pgh_glm_score_multi_spa's "n2 > n0".
 * E = the samples of N whose value is not exactly b (v != b << 14 on the grid).  gt_i = x_i - Zt_i t for i in N, which
 * does not depend on b; mu_i = r_i > 0 ? 1 - r_i : -r_i; V_E = sum_E w gt^2.  V_rest = 0 by rule when E = N, that is
 * when no sample of N sits exactly on b, the usual case of a full track (the sparse route's rule for b = 3); otherwise
 * V_rest = max(V - V_E, 0).  Everything else is pgh_glm_score_sparse_spa's contract word for word: K, K', K'' with one
 * exp(-|gt s|) per entry; the safeguarded Newton iteration; the three stopping rules and the cap of 64 evaluations;
 * omega, nu and the two tails; the state-2 conditions.
 *
 * A variant without a track, whatever its neighbours carry, and a variant whose track restates its calls get
 * pgh_glm_score_multi_spa's triple (out, p_spa, spa_state) for the same calls in a file without tracks, bit for bit
 * (for calls E = N cannot arise in a fitted row); a dataset without any track gets pgh_glm_score_multi_spa's bytes.
 *
 * A row's triple is a function of its variant's calls and track, its own phenotype, the covariates, the subset and
 * spa_cutoff only: not of the other phenotypes or its place among them, of v_begin, the variant chunk, the phenotype
 * block, which other variants carry tracks, the window the dataset was opened with, PGH_GLM_SCORE_SCRATCH_BYTES or the
 * grid, and the same call returns the same bytes every time.  With a full track E = N, so the iteration passes over
 * every sample of the row, not over its carriers.
 * Approximate Firth estimates over tracks: pgh_glm_score_multi_dosage_firth.  Not offered: Firth and saddlepoint in one
 * call, shard groups, a table function. */
int pgh_glm_score_multi_dosage_spa(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                                   uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                                   double spa_cutoff, pgh_glm_row *out, double *p_spa, uint8_t *spa_state, char *errbuf);
/* pgh_glm_score_sparse_multi with pgh_glm_score_sparse_spa's SADDLEPOINT p-value beside the normal one, for every
 * (variant, phenotype) row of the sparse many-phenotype route.  Arguments, argument checks, error texts and refusals
 * are pgh_glm_score_sparse_multi's: a dataset that is not sparse-resident, a shard group, n_pheno == 0, "phenotype must
 * be 0 or 1" and "no cases or no controls", each followed by the phenotype's index.  In addition spa_cutoff must be at
 * least 0.1 (+infinity: never apply it; NaN or a smaller value is PGH_ERR_ARG, "spa_cutoff must be at least 0.1"), and
 * p_spa and spa_state must not be NULL ("null p_spa or spa_state"); they have out's layout, element
 * (v - v_begin) * n_pheno + p.  On any error all three outputs are untouched.  v_begin == v_end is PGH_OK.
 *
 * out is pgh_glm_score_sparse_multi's result for the same arguments bit for bit; its p stays the normal p-value.
 * spa_state and p_spa mean what they mean for pgh_glm_score_sparse_spa: 0 = not applied (the row is not fitted: p_spa
 * NaN; or |stat| <= spa_cutoff: p_spa = out.p bit for bit), 1 = applied (p_spa is the saddlepoint p), 2 = attempted and
 * failed (p_spa = out.p bit for bit).
 *
 * Definition: pgh_glm_score_sparse_spa's, word for word, per (variant, phenotype) row.  E = the samples of that
 * phenotype's N that the row holds as called entries; a row held in the dense form counts as a base-0 row, and a
 * missing-majority row (b = 3) has E = N and V_rest = 0 by rule.  gt = d - Zt t with Zt centred on that phenotype's own
 * pattern means; mu = r > 0 ? 1 - r : -r; K, K', K'' with one exp(-|gt s|) per entry; the safeguarded Newton iteration
 * for q+ and q- = +-|U| from |q| / V with the 1/sqrt(V) step cap that doubles; the three stopping rules and the cap of
 * 64 evaluations; omega, nu and the two tails; the state-2 conditions.
 *
 * Against pgh_glm_score_sparse_spa for the same phenotype alone over the same dataset, E is the same set: the states
 * agree and p_spa agrees to rounding, not bit for bit (t, U and V come from sums taken in another order).  Against
 * pgh_glm_score_multi_spa over the same file, agreement holds where the sparse base code equals the dense b, as that
 * contract says.
 *
 * A row's (out, p_spa, spa_state) is a function of its variant's entries, its own phenotype, the covariates, the subset
 * and spa_cutoff only: not of the other phenotypes of the call or its place among them, of n_pheno, the phenotype
 * block, the rows that share a wave, a workgroup or a work list with it, v_begin, the variant chunk, the window the
 * dataset was opened with, PGH_GLM_SCORE_SCRATCH_BYTES (which here also bounds the saddlepoint kernel's stashes and
 * work lists) or the grid, and the same call returns the same bytes every time.
 * Approximate Firth estimates over this route: pgh_glm_score_sparse_multi_firth.  Not offered: Firth and saddlepoint in
 * one call. */
int pgh_glm_score_sparse_multi_spa(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                                   uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                                   double spa_cutoff, pgh_glm_row *out, double *p_spa, uint8_t *spa_state, char *errbuf);
/* One (variant, phenotype) result of pgh_glm_score_multi_firth. */
typedef struct pgh_glm_firth_row {
	double beta, se, p;
	uint8_t state;      /* 0 not applied, 1 applied, 2 attempted and failed */
	uint8_t pad[7];
} pgh_glm_firth_row;   /* 32 bytes */
/* pgh_glm_score_multi with an APPROXIMATE FIRTH estimate beside the one-step score estimate, for every (variant,
 * phenotype) row of the dense route beyond a cutoff (the "approximate Firth" of Mbatchou et al. 2021: the covariate
 * effects are held fixed at the null fit and only the variant's own coefficient is estimated, under Firth's penalty).
 * Arguments, argument checks, error texts and refusals are pgh_glm_score_multi's: a sparse-resident dataset, a shard
 * group, a dataset with dosage tracks (pgh_glm_score_multi_dosage_firth gives such a dataset's score rows and Firth
 * estimates: this entry's walk reads 2-bit rows), 0/1 phenotypes, cases and controls.  In addition firth_cutoff must be at least
 * 0.1 (+infinity: never apply it; NaN or a smaller value is PGH_ERR_ARG, "firth_cutoff must be at least 0.1"), and
 * firth must not be NULL ("null firth"); it has out's layout, element (v - v_begin) * n_pheno + p.  On any error both
 * outputs are untouched.  v_begin == v_end is PGH_OK.
 *
 * out is pgh_glm_score_multi's result for the same arguments bit for bit.  Its firth byte stays 0: that byte records
 * pgh_glm's full Firth fallback, which this is not.
 *
 * firth[i].state and values; pad is zero:
 *   0  the row is not fitted:                      beta, se, p are NaN
 *   0  the row is fitted with |stat| <= cutoff:    out's beta, se, p bit for bit
 *   1  applied:                                    the Firth values below
 *   2  attempted and failed:                       out's beta, se, p bit for bit
 *
 * Definition, in pgh_glm_score_sparse's notation (S, N, r, w).  The null model is that contract's maximum-likelihood
 * fit, unchanged.
 *   mu_i = r_i > 0 ? 1 - r_i : -r_i
 *   y_i - mu_i = r_i
 *   E = the samples of N with x_i != 0
 *   G = sum_E x_i r_i
 * With pi_i(beta) = mu e^(x beta) / (1 - mu + mu e^(x beta)) and v_i = pi_i (1 - pi_i):
 *   K(beta)     = sum_E [ln(1 - mu + mu e^(x beta)) - mu x beta]
 *   K'(beta)    = sum_E x (pi - mu)
 *   K''(beta)   = sum_E x^2 v
 *   K'''(beta)  = sum_E x^3 v (1 - 2 pi)
 *   K''''(beta) = sum_E x^4 v (1 - 6 v)
 *
 *   l*(beta) = beta G - K(beta) + 1/2 ln K''(beta)          (penalised log-likelihood minus the unpenalised one at 0)
 *   F(beta)  = G - K'(beta) + 1/2 K'''(beta) / K''(beta)    (Firth's modified score)
 *   H(beta)  = K''(beta) - 1/2 [K''''(beta)/K''(beta) - (K'''(beta)/K''(beta))^2];  where not H > 0, H = K''(beta)
 * All sums are evaluated with one exp of -|x beta| per entry, as for pgh_glm_score_sparse_spa, so nothing overflows or
 * cancels.  With the covariate part fixed a sample with x = 0 contributes a constant, which is why E suffices.
 *
 * Root.  The iteration is safeguarded and is the saddlepoint code's scheme.
 *   1. Evaluate at 0.  F(0) = 0 exactly gives beta^ = 0.
 *   2. Otherwise the root lies on the side sgn = sign F(0), and the bracket is [0, open) on that side.
 *   3. From an evaluated point beta the next point is beta + F/H.
 *   4. While the far side is open, a step may not move more than 1/sqrt(K''(0)) beyond beta.  That limit doubles each
 *      time it is used.
 *   5. Once the far side is closed, a point outside the bracket is replaced by the bracket's midpoint.
 *   6. A point with F of sign sgn becomes the near end.  Any other point becomes the far end.
 *   7. beta, already evaluated, is taken as beta^ when the proposed move delta meets any of these stopping rules:
 *      |delta| sqrt(K''(0)) <= 1e-10; the closed bracket is that narrow; |delta| <= 2^-50 |beta|.
 *   8. F(beta) = 0 exactly also ends the iteration.
 *   9. There are at most 64 evaluations, the one at 0 included.
 * State 2 is any of: the cap of 64 evaluations is reached; any of l*, F, H is not finite; K'' is not > 0 at an
 * evaluated point.
 *
 * Result.  beta = beta^;  se = 1 / sqrt(K''(beta^));  D = max(2 (l*(beta^) - l*(0)), 0);  p = pgh_glm_p_from_z(sqrt(D)),
 * the chi-square tail on 1 df.
 *
 * This is a definition: the null fit is not Firth-penalised, unlike REGENIE's.  It has not been compared with another
 * program's output.
 *
 * A row's (out, firth) is a function of its variant's calls, its own phenotype, the covariates, the subset and
 * firth_cutoff only: not of the other phenotypes of the call or its place among them, of v_begin, the variant chunk,
 * the phenotype block, PGH_GLM_SCORE_SCRATCH_BYTES (which also bounds this kernel's stashes exactly as for
 * pgh_glm_score_multi_spa) or the grid, and the same call returns the same bytes every time. */
int pgh_glm_score_multi_firth(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                              uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                              double firth_cutoff, pgh_glm_row *out, pgh_glm_firth_row *firth, char *errbuf);
/* pgh_glm_score_multi_dosage with pgh_glm_score_multi_firth's APPROXIMATE FIRTH estimate beside the one-step score
 * estimate: the Firth follow-up over a dense-resident dataset that may hold DOSAGE TRACKS.  Arguments, argument checks,
 * error texts and the layout of the two outputs are pgh_glm_score_multi_firth's, except that a dataset whose
 * pgh_info.dosage_variant_ct is not 0 is accepted: firth_cutoff must be at least 0.1 (+infinity: never apply it; NaN or
 * a smaller value is PGH_ERR_ARG, "firth_cutoff must be at least 0.1"), firth must not be NULL ("null firth").  The
 * refusals are pgh_glm_score_multi_dosage's: a sparse-resident dataset, a shard group, a phenotype that is not 0 / 1, a
 * phenotype without a case or a control, the latter two followed by the phenotype's index.  On any refusal both outputs
 * are untouched; v_begin == v_end is PGH_OK.
 *
 * out is pgh_glm_score_multi_dosage's result for the same arguments bit for bit; its firth byte stays 0.
 * firth[i].state and values mean what they mean for pgh_glm_score_multi_firth: state 0 with NaN for a row that is not
 * fitted, state 0 with out's beta, se and p bit for bit where |stat| <= firth_cutoff, state 1 with the Firth values,
 * state 2 with out's values bit for bit; pad is zero.
 *
 * Definition: pgh_glm_score_multi_firth's, word for word, under pgh_glm_score_multi_dosage's genotype rule
 * (x_i = value / 16384 where there is an explicit dosage, the call's ALT count otherwise; M = the samples with neither;
 * N = S \ M).  E = the samples of N with x_i != 0 exactly (v != 0 and v != 0xFFFF on the 2^-14 grid).  G, K through
 * K'''', l*, F, H, the root rules 1-9, the state-2 conditions and the result are unchanged.  There is no base code
 * here: a sample with x = 0 contributes a constant of l*, whatever the row's majority.
 *
 * A variant without a track, whatever its neighbours carry, and a variant whose track restates its calls get
 * pgh_glm_score_multi_firth's pair (out, firth) for the same calls in a file without tracks, bit for bit; a dataset
 * without any track gets pgh_glm_score_multi_firth's bytes.
 *
 * A row's pair is a function of its variant's calls and track, its own phenotype, the covariates, the subset and
 * firth_cutoff only: not of the other phenotypes or its place among them, of v_begin, the variant chunk, the phenotype
 * block, which other variants carry tracks, the window the dataset was opened with, PGH_GLM_SCORE_SCRATCH_BYTES or the
 * grid, and the same call returns the same bytes every time.  With a full track E is usually all of N, so each
 * evaluation of the iteration passes over every sample of the row, not over its carriers.
 * Not offered: Firth and saddlepoint in one call, a Firth-penalised null fit, shard groups, a table function. */
int pgh_glm_score_multi_dosage_firth(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                                     uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                                     double firth_cutoff, pgh_glm_row *out, pgh_glm_firth_row *firth, char *errbuf);
/* pgh_glm_score_sparse with pgh_glm_score_multi_firth's APPROXIMATE FIRTH estimate beside the one-step score estimate,
 * for every variant of [v_begin, v_end) of a SPARSE-RESIDENT dataset beyond a cutoff, from the variants' entries: a
 * row costs in proportion to the samples that differ from its base code.  Arguments, argument checks, error texts and
 * refusals are pgh_glm_score_sparse's: a dense-resident dataset ("needs a sparse-resident dataset"), a shard group,
 * 0/1 phenotypes, cases and controls, at most PGH_GLM_MAX_COVAR covariates, the resident range.  In addition
 * firth_cutoff must be at least 0.1 (+infinity: never apply it; NaN or a smaller value is PGH_ERR_ARG, "firth_cutoff
 * must be at least 0.1"), and firth, one element per variant, must not be NULL ("null firth").  On any error both
 * outputs are untouched.  v_begin == v_end is PGH_OK.
 *
 * out[i] is pgh_glm_score_sparse's row for the same arguments bit for bit.  Its firth byte stays 0: that byte records
 * pgh_glm's full Firth fallback, which this is not.
 *
 * firth[i].state and values mean what they mean for pgh_glm_score_multi_firth; pad is zero:
 *   0  the row is not fitted:                      beta, se, p are NaN
 *   0  the row is fitted with |stat| <= cutoff:    out's beta, se, p bit for bit
 *   1  applied:                                    the Firth values below
 *   2  attempted and failed:                       out's beta, se, p bit for bit
 *
 * Definition, in pgh_glm_score_sparse's notation (S, N, r, w, the base code b).  The null model is that contract's
 * maximum-likelihood fit, unchanged.
 *   mu_i = r_i > 0 ? 1 - r_i : -r_i
 *   b    = the row's base code; 0 for a missing-majority row and for a row held in the dense form
 *   d_i  = x_i - b
 *   E    = the row's used called entries with d_i != 0: an entry is used when its sample is below the sample count and
 *          in S, and called when its code is not 3
 *   G    = sum_E d_i r_i
 * A missing-majority row holds its hom-ref calls as entries; they have d = 0, contribute a constant and are not in E.
 * The E of a row held in the dense form is its called samples in S with a code other than 0.
 * K and its four derivatives, l*, F, H with its fallback (where not H > 0, H = K''), the evaluation with one exp of
 * -|d beta| per entry, the nine-point root iteration, its stopping rules (|delta| sqrt(K''(0)) <= 1e-10, the closed
 * bracket that narrow, |delta| <= 2^-50 |beta|), the cap of 64 evaluations, the state-2 conditions, and the result
 * beta = beta^, se = 1 / sqrt(K''(beta^)), D = max(2 (l*(beta^) - l*(0)), 0), p = pgh_glm_p_from_z(sqrt(D)) are
 * pgh_glm_score_multi_firth's word for word, with d in place of x.
 *
 * What follows from d:
 *   - For a base-0 row, a missing-majority row and a row held in the dense form, E is the dense route's E: the row
 *     agrees with pgh_glm_score_multi_firth (one phenotype, the same file opened dense) in state and to rounding.
 *   - For a base-1 or base-2 row the coefficient is estimated with the majority genotype as the reference level and
 *     the null intercept held fixed.  That is another approximation than the dense route's, not the same number: with a
 *     fixed offset the estimate depends on the reference coding (the score row does not).  Datasets opened with
 *     another max_minor agree to rounding only where E is the same set.
 *   - A fitted row always has a non-empty E (otherwise it would be CONST_ALLELE), so K''(0) > 0.
 *
 * A row's (out, firth) is a function of its variant's entries, the phenotype, the covariates, the subset and
 * firth_cutoff only: not of v_begin, the chunk, the window the dataset was opened with, the grid or the rows around
 * it, and the same call returns the same bytes every time.  Many phenotypes in one walk of the entries, with this
 * estimate: pgh_glm_score_sparse_multi_firth.  Not offered: a Firth-penalised null fit, Firth and saddlepoint in one
 * call, the dense route's coding for base-1 and base-2 rows, dosage tracks, shard groups, a table function. */
int pgh_glm_score_sparse_firth(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                               const double *phenotype, uint32_t n_covar, const double *covariates,
                               double firth_cutoff, pgh_glm_row *out, pgh_glm_firth_row *firth, char *errbuf);
/* pgh_glm_score_sparse_multi with pgh_glm_score_sparse_firth's APPROXIMATE FIRTH estimate beside the one-step score
 * estimate, for every (variant, phenotype) row of the sparse many-phenotype route beyond a cutoff.  Arguments, argument
 * checks, error texts and refusals are pgh_glm_score_sparse_multi's: a dataset that is not sparse-resident, a shard
 * group, n_pheno == 0, "phenotype must be 0 or 1" and "no cases or no controls", each followed by the phenotype's index.
 * In addition firth_cutoff must be at least 0.1 (+infinity: never apply it; NaN or a smaller value is PGH_ERR_ARG,
 * "firth_cutoff must be at least 0.1"), and firth must not be NULL ("null firth"); it has out's layout, element
 * (v - v_begin) * n_pheno + p.  On any error both outputs are untouched.  v_begin == v_end is PGH_OK.
 *
 * out is pgh_glm_score_sparse_multi's result for the same arguments bit for bit.  Its firth byte stays 0: that byte
 * records pgh_glm's full Firth fallback, which this is not.
 *
 * firth[...].state and values mean what they mean for pgh_glm_score_multi_firth: state 0 with NaN for a row that is not
 * fitted, state 0 with out's beta, se, p bit for bit where |stat| <= cutoff, state 1 with the Firth values, state 2 with
 * out's beta, se, p bit for bit; pad is zero.
 *
 * Definition: pgh_glm_score_sparse_firth's, word for word, per (variant, phenotype) row.  b is the row's base code, 0
 * for a missing-majority row and for a row held in the dense form; d = x - b; E is that phenotype's used called entries
 * with d != 0; mu is recovered from that phenotype's r; G = sum_E d r.  The iteration, the stopping rules, the cap of 64
 * evaluations, the state-2 conditions and the result are unchanged.  What follows from d carries over: base-1 and
 * base-2 rows use another reference level than the dense route.
 *
 * Against pgh_glm_score_sparse_firth for the same phenotype alone over the same dataset, E is the same set: the states
 * agree and the values agree to rounding.  Against pgh_glm_score_multi_firth over the same file opened dense,
 * agreement holds for base-0, missing-majority and dense-form rows, as that contract says.
 *
 * A row's (out, firth) is a function of its variant's entries, its own phenotype, the covariates, the subset and
 * firth_cutoff only: not of the other phenotypes of the call or its place among them, of n_pheno, the phenotype block,
 * the rows that share a wave, a workgroup or a work list with it, v_begin, the variant chunk, the window the dataset
 * was opened with, PGH_GLM_SCORE_SCRATCH_BYTES (which here also bounds this call's stashes and work lists) or the grid,
 * and the same call returns the same bytes every time.
 * Not offered: Firth and saddlepoint in one call, a Firth-penalised null fit, quantitative phenotypes, dosage tracks,
 * shard groups, a table function. */
int pgh_glm_score_sparse_multi_firth(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                                     uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                                     double firth_cutoff, pgh_glm_row *out, pgh_glm_firth_row *firth, char *errbuf);
/* Gene-set BURDEN tests over a SPARSE-RESIDENT dataset (pgh_open_sparse), from the variants' entries: per set, the
 * variants are collapsed into one weighted burden per sample and the phenotype is regressed on it (linear).
 *
 * Inputs.  phenotype, n_covar, covariates and subset are pgh_glm_sparse's.  The n_sets >= 1 sets are in CSR form:
 * set_off[n_sets + 1] (set_off[0] == 0, not decreasing) and set_vidx[set_off[n_sets]], set s being the memberships
 * set_off[s] .. set_off[s + 1] - 1.  A set_vidx entry is a variant index OF THE DATASET: 0 names the first resident
 * variant (pgh_info.variant_begin), and every entry is below variant_end - variant_begin.  Any order; a repeated
 * variant counts each time; an empty set is allowed.  weight: NULL (every weight 1.0) or one finite double per
 * membership.
 *
 * Values.  S = the output samples with a phenotype, n_y = |S|.  val(c) = c for the codes 0, 1, 2 and val(3) = 0: a
 * MISSING CALL CONTRIBUTES NOTHING, i.e. it is imputed hom-ref.  (This is a definition.  It has not been compared
 * with any other program's output.)  For set s with memberships m = 0, 1, .. in set order, variant v_m, weight w_m and
 * b_m the base code of v_m's resident row (pgh_open_sparse: the row's majority code; 0 for a row held in the dense
 * form, whose entries are then its samples with code 1 or 2):
 *   c_s = sum_m w_m val(b_m);
 *   d_i, for a sample i of S, starts at 0.0 and takes, for each membership in set order at which sample i has an entry
 *        with code c, d_i = d_i + w_m * (double)(val(c) - val(b_m)): one multiply and one add in FP64, so d_i is a
 *        bit-defined function of the set;
 *   B_i = c_s + d_i, the burden.
 *
 * Fit.  OLS of y on [B, 1, z] over S.  The intercept absorbs c_s, so the fit runs on the sums over d (n = n_y,
 * sum d, sum d^2, sum d y, sum d z_j; y and z centred over S as pgh_glm centres them) and pgh_glm's linear solve:
 * its pivot rule, df = n_y - n_covar - 2 and the t p-value.
 *
 * Decisions, in this order: n_y < n_covar + 3: PGH_GLM_TOO_FEW_SAMPLES for every row.  PGH_GLM_CONST_ALLELE iff
 * min over S of d_i == max over S of d_i, an exact FP compare (samples without an entry have d_i = 0; an empty set
 * and a set with no carrier in S land here).  Otherwise PGH_GLM_SINGULAR_MATRIX and PGH_GLM_ZERO_VARIANCE as the
 * solve decides them.
 *
 * out: one row per set, in set order.  A set's row is a function of its memberships and weights, of the phenotype,
 * the covariates and the subset alone: not of the other sets of the call or its place among them, of how many
 * workgroups ran or which took the set, or of the window the dataset was opened with; the same call returns the same
 * bytes every time.  PGH_BURDEN_SCRATCH_BYTES (read at every call; default 1 GiB) bounds the device scratch of the
 * per-set accumulation and with it the number of sets in flight; the result does not depend on it.
 *
 * PGH_ERR_ARG, out untouched: a dataset that is not sparse-resident ("needs a sparse-resident dataset"), a shard
 * group, n_sets == 0, set_off[0] != 0 or a decreasing set_off, a set_vidx entry that is not below the variant count,
 * a weight that is not finite, and whatever pgh_glm_sparse refuses in the arguments they share. */
typedef struct pgh_burden_row {
	double beta, se, stat, p;  /* NaN where the row is undecided                     */
	double mean;               /* c_s + (sum d) / n_y; NaN when n_y == 0             */
	uint32_t obs_ct;           /* n_y                                                */
	uint32_t n_nonzero;        /* samples of S with d_i != 0.0                       */
	uint8_t errcode;           /* PGH_GLM_*                                          */
	uint8_t pad[7];
} pgh_burden_row;
int pgh_burden_sparse(const pgh_dataset *ds, const pgh_subset *subset, const double *phenotype, uint32_t n_covar,
                      const double *covariates, uint32_t n_sets, const uint64_t *set_off, const uint32_t *set_vidx,
                      const double *weight /* NULL or one per membership */, pgh_burden_row *out, char *errbuf);
/* Gene-set SKAT and BURDEN SCORE tests of a BINARY phenotype over a SPARSE-RESIDENT dataset (pgh_open_sparse), from the
 * variants' entries: per variant set, under the logistic null model of pgh_glm_score_sparse, the variance-component
 * statistic of Wu et al. (2011) with its eigenvalues and p-value, and from the same sums the score test of the weighted
 * burden sum_j omega_j x_j (the logistic counterpart of pgh_burden_sparse).  The formulas below are the definition; they
 * have not been compared with another program's output.
 *
 * Inputs.  phenotype, n_covar, covariates and subset are pgh_glm_score_sparse's (values 0 / 1 / NaN, at least one case
 * and one control).  n_sets, set_off, set_vidx (dataset-local indices, any order, repeats counted, an empty set allowed)
 * and weight (omega, finite; NULL = 1.0) are pgh_burden_sparse's, with the
 * same checks and the same PGH_ERR_ARG texts; in addition no set may hold more than PGH_SKAT_MAX_SET memberships
 * ("set larger than PGH_SKAT_MAX_SET").  A dataset that is not sparse-resident and a shard group are refused as there.
 * On any error every output is untouched.
 *
 * Null model.  Exactly pgh_glm_score_sparse's: S, n_y, Zt, the Newton rule, H, g_S, w, r; fitted once per call by the
 * same code.
 *
 * Values.  val(0, 1, 2, 3) = (0, 1, 2, 0): a missing call is imputed hom-ref, pgh_burden_sparse's rule.  For membership
 * j (variant v_j, base code b_j of its resident row; a row held in the dense form counts as base 0 with its samples of
 * code 1 or 2 as entries): d_ij = val(code) - val(b_j) at the entries of v_j whose sample is in S, 0 elsewhere.  The
 * scores do not change when a multiple of a column of Zt is added to a genotype, so d stands in for it.
 *
 * Sums of a set of m memberships (j, l < m; Omega = diag omega):
 *   U0_j = sum_i d_ij r_i      c_j = sum_i w_i d_ij Zt_i          A_jl = sum_i w_i d_ij d_il
 *   t_j  = H^-1 c_j            U_j = U0_j - t_j' g_S              Phi_jl = A_jl - c_j' H^-1 c_l
 *   K = Omega Phi Omega        q = sum_j omega_j^2 U_j^2
 *   burden: U_B = sum_j omega_j U_j   V_B = omega' Phi omega   beta = U_B / V_B   se = 1 / sqrt(V_B)
 *           stat = U_B / sqrt(V_B)    p = pgh_glm_p_from_z(stat); the four are NaN when V_B <= 1e-10 omega' A omega
 *           (the row stays decided)
 * H is factored by Cholesky under the 1e-10 pivot rule of the null fit.  A repeated variant is a repeated row and column
 * of Phi.  lambda_1 >= .. >= lambda_m are the eigenvalues of K (pgh_symmetric_eigenvalues); an eigenvalue is USED iff
 * lambda_k > 1e-10 lambda_1; n_lambda counts the used ones; lambda_sum = trace K; lambda_max = lambda_1.
 * p_skat = pgh_skat_p_from_lambda(q, the used eigenvalues, n_lambda), with its state in p_state.
 * lambda_out, if not NULL, receives all m eigenvalues of set s at set_off[s], descending; NaN for a row that is not
 * decided.
 *
 * Decisions, in this order: n_y < n_covar + 3: PGH_GLM_TOO_FEW_SAMPLES for every row.  n_carriers == 0 or every
 * d_ij == 0 (an empty set too): PGH_GLM_CONST_ALLELE.  The null model's status, as pgh_glm_score_sparse assigns it.
 * lambda_1 <= 0 or not finite: PGH_GLM_ZERO_VARIANCE.  Otherwise PGH_GLM_OK.  obs_ct and n_carriers are always filled;
 * every other number of a row that is not decided is NaN (n_lambda and p_state 0).
 *
 * A set's row and its eigenvalues are a function of its memberships and weights, of the phenotype, the covariates and
 * the subset alone: not of the other sets of the call or their order, of how many workgroups ran or which took the set,
 * of the scratch budget or of the window the dataset was opened with; the same call returns the same bytes every time.
 * Datasets opened with another max_minor hold other base codes; their rows agree to rounding (1e-9), not bit for bit.
 * PGH_SKAT_SCRATCH_BYTES (read at every call; default 1 GiB) bounds the device scratch (the workgroups' per-sample
 * vectors and the sums of the sets of one launch) and with it the sets in flight; the result does not depend on it. */
#define PGH_SKAT_MAX_SET 256
typedef struct pgh_skat_row {
	double q, p_skat;              /* SKAT statistic and its p; NaN where undecided                  */
	double beta, se, stat, p;      /* burden score test of sum_j omega_j x_j; NaN where undecided    */
	double lambda_sum, lambda_max; /* trace and largest eigenvalue of K                              */
	uint32_t obs_ct;               /* n_y                                                            */
	uint32_t n_carriers;           /* samples of S with an entry in at least one member              */
	uint32_t n_lambda;             /* eigenvalues used                                               */
	uint8_t errcode;               /* PGH_GLM_*                                                      */
	uint8_t p_state;               /* 0 none, 1 exact (one eigenvalue), 2 saddlepoint, 3 near-mean limit, 4 failed */
	uint8_t pad[2];
} pgh_skat_row; /* 80 bytes */
int pgh_skat_sparse(const pgh_dataset *ds, const pgh_subset *subset, const double *phenotype, uint32_t n_covar,
                    const double *covariates, uint32_t n_sets, const uint64_t *set_off, const uint32_t *set_vidx,
                    const double *weight /* NULL or one per membership */, pgh_skat_row *out,
                    double *lambda_out /* NULL, or set_off[n_sets] doubles */, char *errbuf);
/* The survival function of Q = sum_k lambda_k chi^2_1 (independent, one degree of freedom each) at q.  lambda: n
 * positive finite values, any order (pgh_skat_sparse passes only the used eigenvalues).  *state (may be NULL):
 * 1 exact, 2 saddlepoint, 3 near-mean limit, 4 failed.
 *   n == 1: exact, pgh_glm_p_from_z(sqrt(q / lambda_1)), state 1.
 *   n >= 2: the saddlepoint approximation of Kuonen (1999) in the Barndorff-Nielsen form, the tail form of
 *   pgh_glm_score_sparse_spa.  With Phibar the upper tail of the standard normal:
 *     K(s) = -1/2 sum ln(1 - 2 s lambda_k)   K'(s) = sum lambda_k / (1 - 2 s lambda_k)
 *     K''(s) = sum 2 lambda_k^2 / (1 - 2 s lambda_k)^2,   s < 1 / (2 lambda_1)
 *     mu = sum lambda   k2 = 2 sum lambda^2   k3 = 8 sum lambda^3
 *     |q - mu| <= 1e-3 sqrt(k2):  p = Phibar(k3 / (6 k2^1.5))      state 3: the limit of the form below at s -> 0
 *     otherwise  s^ = the root of K'(s^) = q;  omega = sign(s^) sqrt(2 (s^ q - K(s^)));  nu = s^ sqrt(K''(s^));
 *                p = Phibar(omega + ln(nu / omega) / omega)        state 2
 *   The root is found by a safeguarded Newton iteration from the Newton step at 0, (q - mu) / k2.  For q > mu the
 *   bracket is [0, 1 / (2 lambda_1)), its far end open: a step that leaves the bracket goes to the midpoint of s and
 *   the end it left by.  For q < mu the bracket is (-inf, 0]; while its far side is open a step may not exceed
 *   1 / sqrt(k2), doubling each time the limit is used.  The root is taken when |delta s| <= 1e-12 |s|, after at most
 *   100 evaluations of K', K''.  K is summed with log1p.
 *   State 4: p = NaN for q < 0, a q or a lambda that is not finite, a lambda that is not positive, n == 0, no root
 *   within the cap, 2 (s^ q - K) <= 0, nu / omega <= 0 or anything not finite; p = 1.0 for q == 0 exactly.
 * This is an approximation.  A Python model of exactly these formulas was compared with SciPy on a CPU: lambda drawn
 * Gamma(0.5) for m in {2, 3, 5, 20, 100} against Imhof inversion by scipy.integrate.quad wherever the exact p >= 1e-4
 * (below that the quadrature itself fails): within 6.8 % relative.  Equal lambda against chi2.sf down to p = 1e-20:
 * within 5.9 % (m = 2), 1.9 % (m = 5), 0.08 % (m = 50).  The near-mean limit is continuous with its neighbours to
 * 1e-3.  Nothing tighter is claimed, and it has not been compared with another program's output. */
double pgh_skat_p_from_lambda(double q, const double *lambda, uint32_t n, uint8_t *state /* may be NULL */);
/* The eigenvalues of the symmetric n x n matrix a (row-major; both triangles are read), descending, into out (n
 * doubles): Householder tridiagonalisation and implicit QL in FP64.  PGH_ERR_ARG for n == 0 or a null pointer; a
 * matrix with an entry that is not finite gives NaN eigenvalues. */
int pgh_symmetric_eigenvalues(const double *a /* n x n row-major, symmetric */, uint32_t n, double *out /* descending */);
/* pgh_score for a SPARSE-RESIDENT dataset (pgh_open_sparse), from the listed variants' entries: cost proportional to
 * the calls that differ from a variant's base code.  Arguments, output layout (score_sum [n_out][n_cols], subset
 * order) and argument checks are pgh_score's; vidx and mode mean what they mean there.
 *
 * Values.  Hardcalls only (pgh_open_sparse steps over dosage tracks): pgh_score's values for a file without dosage
 * tracks, src/plink_score.cpp:598-652, its skip rules included -- a variant with no call in the subset is skipped,
 * and under PGH_SCORE_CENTER so is one with sd == 0.  With b_i the base code of listed variant i (0 for a row held
 * in the dense form, whose entries are then its samples with a code other than 0) and ts_i[4] / td_i[4] the
 * reference's per-class values from the subset's counts of variant i:
 *   score_sum[s][c] = K_c + sum over the entries (i, g) of sample s of W[i][c] (ts_i[g] - ts_i[b_i]),
 *   K_c             = sum_i W[i][c] ts_i[b_i]            (partial sums of fixed shape: a function of column c alone),
 * dosage_sum likewise with td and unit weights, allele_ct in integers.  Entries of samples outside the subset are
 * skipped.
 *
 * Fixed point.  The per-sample sums are int64: column c has one scale 2^k_c, k_c = 62 - L - e with
 * L = ceil(log2 n_scored) and 2^e the power of two above D_c = max over i, g of |W[i][c] (ts_i[g] - ts_i[b_i])|; a
 * term is llrint(term 2^k_c), and the result is K_c + (double)sum 2^-k_c.  No sample's sum can pass 2^62.  Hence
 * weights must be finite (pgh_score itself refuses a non-finite weight on a dosage-track variant for this reason).
 *
 * Error bound.  With A_c = sum_i |W[i][c]| max_g |ts_i[g]| (so D_c <= 2 A_c) and E_s <= n_scored the listed variants
 * at which sample s has an entry, against the exact sum of the reference's terms:
 *   |score_sum[s][c] - exact| <= (n_scored + 16) 2^-53 A_c  +  E_s 2^-(62 - L) D_c
 * (the FP64 roundings of the K_c sum, of the terms and of the last add; then half a unit of 2^-k_c per entry).
 * For n_scored <= 1024 that is at most 1.2e-13 A_c + 2^-42 D_c < 1e-12 A_c.  At n_scored = 2^20 the second term is
 * E_s 2^-42 D_c: 2^-21 A_c for a sample with an entry at every listed variant, 2^-31 A_c for one with 1,000 entries.
 * Nothing tighter is claimed.  dosage_sum: the same with td and A = sum_i max_g |td_i[g]|.  allele_ct is exact.
 *
 * Determinism.  Integer adds commute, so the same call returns the same bytes every time; a column's values do not
 * depend on the other columns of the call or on its position among them, bit for bit; and the result does not depend
 * on the grid, on the number of row slices (PGH_SCORE_SPARSE_SLICES, read at every call, sets it; default: chosen
 * from the list) or on PGH_SPARSE_WINDOW_BYTES at open.  Datasets opened with different max_minor hold other base
 * codes and agree within the bound, not bit for bit.
 *
 * PGH_ERR_ARG, outputs untouched: a dataset that is not sparse-resident ("needs a sparse-resident dataset"), a shard
 * group, n_cols == 0, a weight that is not finite ("non-finite weight"), and whatever pgh_score refuses in the
 * arguments they share.  There is no _dev or plan form, and the plink_score shell does not route here.
 *
 * Measured on one MI355X (tools/score_sparse_bench.py, profiles/score_sparse_bench.txt; 1,000,000 variants x 500,000
 * samples, ~0.1 % carriers, 5.0e8 entries, whole calls): 48 ms with one column and no dosage sum, 85 ms with it,
 * 0.62 s / 0.66 s with 16 columns, beside 36 ms for pgh_sample_counts over the same rows in the same run.  No
 * kernel-only time or hardware counter was collected. */
int pgh_score_sparse(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_scored, const uint32_t *vidx,
                     const double *weights, const uint8_t *flip, uint32_t n_cols, int mode, double *score_sum,
                     double *dosage_sum /* may be NULL */, uint32_t *allele_ct, char *errbuf);
/* two-sided p of Student's t with df degrees of freedom (the reference's TstatToPvalue) */
double pgh_glm_p_from_t(double t, double df);
/* two-sided p of a standard normal z (ZstatToPvalue) */
double pgh_glm_p_from_z(double z);

/* ---- KING-robust kinship -------------------------------- */

/* For two samples i and j, over the variants of the call at which BOTH have a hardcall (dosage and phase tracks are
 * not read), five uint32 counts:
 *   NSNP      both called                         HETHET    i het and j het
 *   IBS0      one hom-ref, the other hom-alt      HET1HOM2  i het and j homozygous     HET2HOM1  i homozygous, j het
 * and from them, in FP64,
 *   min_het = HETHET + min(HET1HOM2, HET2HOM1)
 *   KINSHIP = 0.5 - (4 IBS0 + HET1HOM2 + HET2HOM1) / (4 min_het)          (NaN when min_het == 0)
 * the KING-robust between-family estimator (Manichaikul et al. 2010) with the smaller of the two het counts.  This
 * formula is the definition; it has not been compared with plink2 --make-king-table's output.
 * The counts are exact: products of 0 / +-1 indicator planes accumulated in int32 on the int8 matrix cores.
 * Both entry points take one dense-resident dataset (not a shard group, not a sparse-resident dataset). */
enum { PGH_KING_NSNP = 0, PGH_KING_HETHET = 1, PGH_KING_IBS0 = 2, PGH_KING_HET1HOM2 = 3,
       PGH_KING_HET2HOM1 = 4, PGH_KING_PLANES = 5 };

/* Counts for the rectangle of sample pairs [i_begin, i_end) x [j_begin, j_end) (indices into the output
 * samples: subset order, or raw order without a subset).  counts: PGH_KING_PLANES planes of
 * (i_end - i_begin) x (j_end - j_begin) uint32, plane-major, i-major inside a plane, host memory.
 * Variants: [variant_begin, variant_begin + n_var), or the n_var entries of vidx when it is not NULL
 * (pgh_sample_counts' convention); 1 <= n_var <= 2^31 - 1.  "1" is the row sample, "2" the column sample.  The
 * rectangle may lie anywhere, the diagonal included (there a sample is paired with itself); an empty or reversed
 * one, or one beyond the output samples, is PGH_ERR_ARG. */
int pgh_king_counts(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                    const uint32_t *vidx, uint32_t i_begin, uint32_t i_end, uint32_t j_begin, uint32_t j_end,
                    uint32_t *counts, char *errbuf);

typedef struct pgh_king_pair {
	uint32_t i, j;                                   /* output-sample indices, i < j */
	uint32_t nsnp, hethet, ibs0, het1hom2, het2hom1; /* "1" is i, "2" is j          */
	uint32_t pad;
	double kinship;
} pgh_king_pair;

/* Every pair i < j of the output samples whose KINSHIP >= min_kinship, ascending by (i, j).  A NaN kinship
 * never passes; min_kinship = -INFINITY or NaN means no filter (every pair, NaN ones included).
 * *n_pairs receives the number of qualifying pairs whether or not they fit; at most `capacity` of them
 * (the first in (i, j) order) are written to out.  out may be NULL when capacity is 0: a counting call.
 * The same call returns the same bytes every time. */
int pgh_king_table(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                   const uint32_t *vidx, double min_kinship, pgh_king_pair *out, uint64_t capacity,
                   uint64_t *n_pairs, char *errbuf);

/* The formula above, on the host (the table's KINSHIP is this function of its own counts, bit for bit). */
double pgh_king_kinship(uint32_t hethet, uint32_t ibs0, uint32_t het1hom2, uint32_t het2hom1);

/* ---- windowed r2 and LD pruning -------------------------- */

/* For two variants a and b of the call, over the output samples at which BOTH have a hardcall (dosage and phase
 * tracks are not read; a sample outside the subset counts as missing everywhere), pgh_ld_pairs' six uint32 sums
 *   n, sum_a, sum_b, sum_ab, sum_a2, sum_b2            (genotype = ALT copies 0 / 1 / 2)
 * as products of three small-integer planes per variant on the int8 matrix cores, exact in int32 for up to 2^29 - 1
 * samples (more: PGH_ERR_ARG).  From them, in int64 and then FP64,
 *   num = n sum_ab - sum_a sum_b     va = n sum_a2 - sum_a^2     vb = n sum_b2 - sum_b^2
 *   the pair EXCEEDS r2_threshold iff n >= 2, va > 0, vb > 0 and ((double)num * (double)num) / ((double)va *
 *   (double)vb) > r2_threshold
 * so a variant that is monomorphic over the pair's samples never exceeds.  This is not plink_ld's mean-based
 * arithmetic; plink_ld's output is unchanged.  Minor-allele order, per variant over the output samples:
 *   alt = het + 2 hom_alt, obs = 2 called, mc = min(alt, obs - alt); k has the LOWER MAF than u iff
 *   mc_k obs_u < mc_u obs_k in uint64 (obs = 0 compares as equal to everything).
 * Pruning rule over the call's variants k = 0 .. n_var - 1 in call order, win_end[k] the exclusive end of k's window:
 *   keep[:] = 1
 *   for k in 0 .. n_var-1:   if keep[k]:
 *     for u in k+1 .. win_end[k]-1:   if keep[u] and exceeds(k, u):
 *       if lower_maf(k, u): keep[k] = 0; break      else: keep[u] = 0        (ties remove the later variant)
 * These formulas are the definition; they have not been compared with plink2 --indep-pairwise's output
 * (DESIGN.md 3.13).  Both device entry points take one dense-resident dataset (not a shard group, not a
 * sparse-resident dataset). */
enum { PGH_LD_N = 0, PGH_LD_SUM_A = 1, PGH_LD_SUM_B = 2, PGH_LD_SUM_AB = 3, PGH_LD_SUM_A2 = 4, PGH_LD_SUM_B2 = 5,
       PGH_LD_PLANES = 6 };

/* Sums for the rectangle of variant pairs [a_begin, a_end) x [b_begin, b_end) (indices into the call's variants:
 * [variant_begin, variant_begin + n_var), or the n_var entries of vidx when it is not NULL, in any order).
 * sums: PGH_LD_PLANES planes of (a_end - a_begin) x (b_end - b_begin) uint32, plane-major, a-major inside a plane,
 * host memory.  The rectangle may lie anywhere, the diagonal included; an empty or reversed one, or one beyond
 * n_var, is PGH_ERR_ARG.  1 <= n_var <= 2^31 - 1. */
int pgh_ld_window_sums(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                       const uint32_t *vidx, uint32_t a_begin, uint32_t a_end, uint32_t b_begin, uint32_t b_end,
                       uint32_t *sums, char *errbuf);

/* The pruning rule above: keep[k] = 1 or 0 for each of the call's n_var variants, *n_kept (may be NULL) their sum.
 * win_end: n_var entries with k < win_end[k] <= n_var, not decreasing in k (variant-count windows, kb windows and
 * chromosome boundaries are all this one array).  A vidx list must be strictly increasing; r2_threshold must be
 * finite and in [0, 1].  Any violation is PGH_ERR_ARG.  Only the tiles of pairs that meet the band
 * k < u < win_end[k] are computed; a pair's sums never leave the registers, one bit per band pair comes back.
 * The band is walked in launches of at most PGH_LD_PRUNE_CHUNK_TILES tiles of 96 x 128 pairs (environment
 * variable, read at every call; default and maximum 32768 = 48 MiB of device scratch for the bits); the result
 * does not depend on it.  The same call returns the same bytes every time, from any thread. */
int pgh_ld_prune(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                 const uint32_t *vidx, const uint32_t *win_end, double r2_threshold, uint8_t *keep,
                 uint64_t *n_kept, char *errbuf);

/* "Exceeds" above on the host, of sums = {n, sum_a, sum_b, sum_ab, sum_a2, sum_b2}: 1 or 0.  The device evaluates
 * the same function of the same sums, bit for bit.  The int64 terms are exact for sums the library can return
 * (n <= 2^29 - 1); larger hand-made values may wrap. */
int pgh_ld_exceeds(const uint32_t sums[6], double r2_threshold);

/* Windowed LD scores.  With the six sums, num, va and vb of a pair as above,
 *   defined(a, b)  iff  n >= 2 (n >= 3 with PGH_LDSCORE_UNBIASED) and va > 0 and vb > 0
 *   r2   = ((double)num * (double)num) / ((double)va * (double)vb)
 *   term = r2                                           (flags == 0)
 *   term = r2 - (1.0 - r2) / (double)(n - 2)            (PGH_LDSCORE_UNBIASED: ldsc's adjustment, with the pair's own n)
 * each statement one IEEE operation.  The pairs of the band are k < u < win_end[k] (win_end as for pgh_ld_prune), and
 *   self[k]       = 1.0 if defined(k, k) from k's own class counts over the output samples (n = called,
 *                   sum_a = sum_b = het + 2 hom_alt, sum_ab = sum_a2 = sum_b2 = het + 4 hom_alt), else 0.0
 *   score[k]      = self[k] + sum of term(k, u) over the defined band pairs (k, u)
 *                           + sum of term(j, k) over the defined band pairs (j, k)
 *   n_partners[k] = the number of those defined pairs (self not counted)
 * so a band pair contributes to both of its variants (for kb windows: the symmetric window |pos_u - pos_k| <= kb),
 * and a variant that is monomorphic or uncalled over a pair's samples contributes nothing and receives nothing.
 * Missing calls are handled by pairwise-complete samples, not by mean imputation.  These formulas are the
 * definition; they have NOT been compared with `ldsc --l2` output (ldsc mean-imputes).
 *
 * Order of the sum (no atomics): score[k] starts at self[k]; then the band's tiles of 96 anchors x 128 partners
 * (origins at multiples of 96 and 128) are taken by anchor tile row ascending, partner tile ascending, and each adds
 * its 96 row sums to its anchors and then its 128 column sums to its partners; inside a tile the terms are added in a
 * fixed order that depends only on the position in the tile.  The result is therefore a function of
 * the variant list, the subset, win_end and flags alone: the same bytes on every run, from any thread, and whatever
 * PGH_LD_SCORE_CHUNK_TILES (environment variable, read at every call: tiles per launch, default and maximum 32768 =
 * 84 MiB of device scratch for the partial sums) is.
 * score: n_var doubles; n_partners: n_var uint32, may be NULL.  Validation is pgh_ld_prune's (win_end, strictly
 * increasing vidx); flag bits other than PGH_LDSCORE_UNBIASED are PGH_ERR_ARG.  One dense-resident dataset. */
enum { PGH_LDSCORE_UNBIASED = 1 };
int pgh_ld_scores(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                  const uint32_t *vidx, const uint32_t *win_end, uint32_t flags, double *score, uint32_t *n_partners,
                  char *errbuf);

/* "term" above on the host, of sums = {n, sum_a, sum_b, sum_ab, sum_a2, sum_b2}: returns 1 and stores *term when the
 * pair is defined, else 0 (also for unknown flag bits).  The device evaluates the same function of the same sums, bit
 * for bit. */
int pgh_ld_r2(const uint32_t sums[6], uint32_t flags, double *term);

/* ---- variance-standardised relationship matrix, GRM ------- */

/* Over the output samples (subset order, or raw order without a subset) and the variants of the call, hardcalls only
 * (dosage and phase tracks are not read).  Per variant v, with het, alt and called counted over the output samples,
 *   p = double(het + 2 alt) / double(2 called)        or p = freq[v] when the caller supplies freq
 * and v is SKIPPED when called == 0, or when p is not finite, p <= 0 or p >= 1: it contributes nothing.  For the
 * other ("used") variants, in this exact sequence of FP64 operations on the host,
 *   q = 1 - p      s = sqrt((2 p) q)      z[c] = (c - 2 p) / s  for the codes c = 0, 1, 2      z = 0 for a missing call
 *   nobs_ij = number of used variants at which both i and j are called                          (uint32, exact)
 *   rel_ij  = (sum over used v of z_iv z_jv) / nobs_ij                                           (NaN when nobs_ij == 0)
 * With PGH_GRM_MEANIMPUTE the divisor is the number of used variants for every pair (NaN when it is 0).
 * This is the matrix of plink2 --make-rel / GCTA's GRM; the formulas above are the definition, they have not been
 * compared with either program's output.  The sum runs on the FP64 matrix cores in the order of the
 * call's variants: a pair's value does not depend on the rectangle asked for or on which of the two is the row
 * sample, and the same call returns the same bytes every time.
 * Takes one dense-resident dataset (not a shard group, not a sparse-resident dataset). */
enum { PGH_GRM_MEANIMPUTE = 1 };
#define PGH_GRM_TILE 128 /* sample pairs per workgroup: PGH_GRM_TILE x PGH_GRM_TILE */

/* rel (and nobs, unless NULL): (i_end - i_begin) x (j_end - j_begin), i-major, host memory, for the rectangle of
 * output-sample pairs [i_begin, i_end) x [j_begin, j_end).  Variants, rectangle and errors as pgh_king_counts:
 * [variant_begin, variant_begin + n_var), or the n_var entries of vidx when it is not NULL; 1 <= n_var <= 2^31 - 1;
 * the rectangle may lie anywhere, the diagonal included; an empty or reversed one, or one beyond the output samples,
 * is PGH_ERR_ARG, and so are unknown flag bits.  freq: NULL, or one frequency per variant of the call.
 * *n_used (unless NULL) receives the number of variants not skipped.
 * The rows are walked in bands through device blocks of at most PGH_GRM_BAND_BYTES bytes (environment variable, read at
 * every call; default and maximum 268435456; a band is never less than PGH_GRM_TILE rows); the result does not depend
 * on it. */
int pgh_grm(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
            const uint32_t *vidx, const double *freq /* NULL or n_var */, uint32_t i_begin, uint32_t i_end,
            uint32_t j_begin, uint32_t j_end, uint32_t flags, double *rel, uint32_t *nobs /* may be NULL */,
            uint32_t *n_used /* may be NULL */, char *errbuf);

/* The standardisation above on the host: returns p, or NaN when the variant is skipped; z[0..2] is written only when
 * it is not (z may be NULL).  pgh_grm's tables are this function of the counts, bit for bit. */
double pgh_grm_standardize(uint32_t het, uint32_t alt, uint32_t called, double z[3]);

/* ---- per-sample inbreeding coefficients, plink's --het, in exact fixed point ------- */

/* Per output sample (subset order, or raw order without a subset): the observed and the expected number of homozygous
 * calls over the variants of the call and the method-of-moments inbreeding coefficient F.  Hardcalls only (dosage and
 * phase tracks are not read).  The formulas below are the definition; they have not been compared with plink's output.
 *
 * Per variant v, with het, alt and called counted over the output samples, in this exact sequence of FP64 operations
 * on the host, one IEEE operation per statement:
 *   p = double(het + 2 alt) / double(2 called)        or p = freq[v] when the caller supplies freq
 * and v is SKIPPED when called == 0, or when p is not finite, p <= 0 or p >= 1 (a NaN freq[v] skips v).  Otherwise
 *   q = 1 - p      u = (2 p) q
 *   with PGH_HET_SMALL_SAMPLE:   r = double(2 called) / double(2 called - 1)      u = u r
 *   e = 1 - u                                                                      (0 <= e <= 1)
 * pgh_het_expected is this function of the counts.
 *
 * Fixed point.  L is the smallest integer with 2^L >= max(n_var, 1), n_var being the CALLER's count (also inside a
 * shard group); k = 62 - L = pgh_het_scale(n_var); q_v = llrint(e_v 2^k).  Per sample i
 *   e_sum_i = sum of q_v over the used variants at which i is called         (an exact int64, at most 2^62)
 *   e_hom   = ldexp((double)e_sum, -k)
 *   hom_ct  = used variants at which i's call is 0 or 2,    obs_ct = used variants at which i has a call
 *   f       = (double(hom_ct) - e_hom) / (double(obs_ct) - e_hom)            (NaN when obs_ct == 0 or the divisor is 0)
 * A repeated list entry counts each time; the order of the list does not matter; n_var == 0 is PGH_OK with every row
 * {0.0, NaN, 0, 0, 0}.  Under the empty subset nothing is written to out, every variant is skipped and *n_used is 0.
 *
 * Determinism.  Everything summed is an integer, so the same global variants give the same BYTES from a range or the
 * equal list, from any permutation of the list, from the whole file, a window of it or a shard group, on every run,
 * from any thread, and whatever the kernel's grid is: PGH_HET_SLICES (environment variable, read at every call) sets
 * the number of variant slices of the grid, 1 to 65535; by default it is chosen from the list length.  A sample's row
 * does not depend on the samples outside the subset except through het, alt and called.
 *
 * out: one row per output sample.  used (unless NULL): n_var bytes, 1 where the call's entry was used, else 0.
 * *n_used (unless NULL): the number of used entries.  PGH_ERR_ARG, every output untouched: a null ds or out ("null
 * argument"), unknown flag bits, freq together with PGH_HET_SMALL_SAMPLE (the correction needs the counts' own n), a
 * sparse-resident dataset ("needs a dense-resident dataset"), and the range, list and subset refusals of every entry
 * point.  A shard group is accepted: every shard sums its share under the call's k, the integers are added and e_hom
 * and f are formed once.  There is no _dev form: the tables are built on the host.
 * Not offered: a table function, sparse-resident datasets, dosage-weighted heterozygosity, and the male-haploid
 * frequency rule of plink's --check-sex (a caller passes freq and a chrX list). */
enum { PGH_HET_SMALL_SAMPLE = 1 };
#define PGH_HET_TILE 4096 /* samples per workgroup tile of the kernel: 1 KiB of a row, 32 KiB of sums in LDS */
typedef struct pgh_het_row {
	double e_hom;    /* (double)e_sum * 2^-k                                  E(HOM) */
	double f;        /* (hom_ct - e_hom) / (obs_ct - e_hom), NaN: see above        F */
	int64_t e_sum;   /* the fixed-point sum itself                                   */
	uint32_t hom_ct; /* used variants at which the sample's call is 0 or 2   O(HOM)  */
	uint32_t obs_ct; /* used variants at which the sample has a call         N(NM)   */
} pgh_het_row;       /* 32 bytes */
int pgh_het(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
            const uint32_t *vidx, const double *freq /* NULL or n_var */, uint32_t flags,
            pgh_het_row *out /* n_out rows, subset order */, uint8_t *used /* NULL or n_var */,
            uint32_t *n_used /* may be NULL */, char *errbuf);
/* e of one variant from its counts: returns 1 and stores *e when the variant is used, else 0 (also for unknown flag
 * bits, for a freq that is not NaN together with PGH_HET_SMALL_SAMPLE, and for a null e).  freq: NaN takes p from the
 * counts.  pgh_het's tables are this function, bit for bit. */
int pgh_het_expected(uint32_t het, uint32_t alt, uint32_t called, double freq /* NaN: from the counts */, uint32_t flags,
                     double *e);
uint32_t pgh_het_scale(uint32_t n_var); /* k */

/* ---- HWE exact tests (host) --------------------------------------------- */

/* plink2::HweLnP (src/plink_hardy.cpp:78): ln of the two-sided exact-test p. */
double pgh_hwe_lnp(int32_t obs_hets, int32_t obs_hom1, int32_t obs_hom2, uint32_t midp);
/* plink2::HweXchrLnP (src/plink_hardy.cpp:94). */
double pgh_hwe_xchr_lnp(int32_t female_hets, int32_t female_hom1, int32_t female_hom2, int32_t male1, int32_t male2,
                        uint32_t midp);
/* Batch of autosomal tests on the device, straight from a counts array:
 * ln_p[i] from counts[i] = {hom_ref, het, hom_alt, missing}. */
int pgh_hwe_lnp_batch(const uint32_t (*counts)[4], uint32_t n, uint32_t midp, double *ln_p, char *errbuf);

/* plink2::HweXchrLnP (src/plink_hardy.cpp:94) for n variants at once, one workgroup per variant:
 * strata[i] = {female_hets, female_hom1, female_hom2, male1, male2}.  The host form
 * pgh_hwe_xchr_lnp costs ~0.1 s per variant at 500k samples; this is what the plink_hardy shell
 * calls for the chrX variants of a device batch. */
int pgh_hwe_xchr_lnp_batch(const int32_t (*strata)[5], uint32_t n, uint32_t midp, double *ln_p, char *errbuf);
/* Same with device buffers: d_counts uint32[n][4] -> d_ln_p double[n]. */
int pgh_hwe_lnp_batch_dev(const void *d_counts, uint32_t n, uint32_t midp, void *d_ln_p, void *stream, char *errbuf);

#ifdef __cplusplus
}
#endif
#endif /* PGENHIP_H_ */
