// api_glm.cpp -- pgh_glm: plink_glm's per-variant linear / logistic / Firth regressions (glm.hip) behind the C ABI;
// pgh_glm_multi: the same for many phenotypes in one call; pgh_glm_sparse: the linear fit over a sparse-resident
// dataset, from its entries (glm_sparse.hip); pgh_burden_sparse: gene-set burden fits over such a dataset
// (burden_sparse.hip); pgh_glm_score_sparse: the logistic score test over such a dataset, from its entries
// (glm_score_sparse.hip); pgh_glm_score_multi: that test over a dense-resident dataset for many phenotypes in one
// call, on the FP64 matrix cores (glm_score_dense.hip); pgh_glm_score_sparse_multi: that test over a sparse-resident
// dataset for many phenotypes in one walk of its entries (glm_score_sparse_multi.hip), with its saddlepoint and
// approximate Firth follow-ups (glm_score_sparse_multi_spa.hip, glm_score_sparse_multi_firth.hip); pgh_glm_sparse_multi:
// the linear fit over such a dataset for many phenotypes in one walk of its entries (glm_sparse_multi.hip);
// pgh_skat_sparse: SKAT and burden score tests of variant sets under that test's null model (skat_sparse.hip,
// skat_math.hpp, linalg.cpp).
#include "api_internal.hpp"
#include "glm.hpp"
#include "glm_math.hpp"
#include "linalg.hpp"
#include "skat_math.hpp"

#include <unordered_map>

namespace {

// Variants per chunk: bounds the per-variant state (logistic: ~9 KB a variant) and, on a file with dosage tracks,
// the dense dosage rows of the chunk (512 MB at most).
constexpr uint32_t kGlmChunk = 16384;
constexpr uint64_t kGlmDosageBytes = 512ull << 20;

// The mean of y over its n_y samples with a value (NaN = missing).  One pass in sample order, here and in every sum
// of GlmStage: the entry points agree bit for bit only because they all sum in this order.
double GlmMean(const double *y, uint32_t n_out, uint32_t n_y) {
	double my = 0.0;
	for (uint32_t i = 0; i < n_out; i++) {
		my += std::isnan(y[i]) ? 0.0 : y[i];
	}
	return my / (n_y ? n_y : 1u);
}

// y and z of a fit as the kernels read them: hy the phenotype (NaN = missing), hz the covariates sample-major and zero
// padded to kp columns; and, for the kernels whose entries name raw samples, the same in raw-sample order with NaN y
// outside the subset (hy_raw, hz_raw: only with a subset -- without one the two orders are one).
struct GlmStaged {
	std::vector<double> hy, hz, hy_raw, hz_raw;
	uint32_t n_y = 0, kp = 0;
	bool raw = false; // hy_raw, hz_raw are staged
};

// What GlmStage centres on its mean over the samples with a phenotype.  kYZ, the linear fit: y and the covariates; the
// intercept absorbs the shift, so beta, SE and RSS are unchanged, and the whole-call Gram minus a variant's correction
// Gram then subtracts numbers of the data's spread rather than of its offset.  kZ, pgh_glm_multi's linear fit: the
// covariates over the samples of a missing-value pattern, hy being the pattern itself (every phenotype of the pattern
// is centred on its own mean as its block is staged).  kNone: the logistic fit.
enum class GlmCentre { kNone, kZ, kYZ };

GlmStaged GlmStage(const pgh_dataset *ds, const pgh_subset *subset, const double *phenotype, uint32_t k,
                   const double *covariates, GlmCentre centre, bool raw_order) {
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct, n_raw = ds->sample_ct;
	const uint32_t kp = pgh::GlmPadCovar(k);
	GlmStaged sg;
	sg.kp = kp;
	std::vector<double> &hz = sg.hz, &hy = sg.hy;
	hz.assign(static_cast<size_t>(n_out) * kp, 0.0);
	for (uint32_t j = 0; j < k; j++) {
		for (uint32_t i = 0; i < n_out; i++) {
			hz[static_cast<size_t>(i) * kp + j] = covariates[static_cast<size_t>(j) * n_out + i];
		}
	}
	uint32_t n_y = 0;
	for (uint32_t i = 0; i < n_out; i++) {
		n_y += std::isnan(phenotype[i]) ? 0u : 1u;
	}
	sg.n_y = n_y;
	hy.assign(phenotype, phenotype + n_out);
	if (centre != GlmCentre::kNone && n_y) {
		if (centre == GlmCentre::kYZ) {
			const double my = GlmMean(hy.data(), n_out, n_y);
			for (uint32_t i = 0; i < n_out; i++) {
				hy[i] -= my;
			}
		}
		for (uint32_t j = 0; j < k; j++) {
			double mz = 0.0;
			for (uint32_t i = 0; i < n_out; i++) {
				mz += std::isnan(hy[i]) ? 0.0 : hz[static_cast<size_t>(i) * kp + j];
			}
			mz /= n_y;
			for (uint32_t i = 0; i < n_out; i++) {
				hz[static_cast<size_t>(i) * kp + j] -= mz;
			}
		}
	}
	if (subset && raw_order) {
		sg.raw = true;
		sg.hy_raw.assign(n_raw, std::nan(""));
		sg.hz_raw.assign(static_cast<size_t>(n_raw) * kp, 0.0);
		for (uint32_t i = 0; i < n_out; i++) {
			const uint32_t s = subset->sel[i];
			sg.hy_raw[s] = hy[i];
			std::copy_n(hz.data() + static_cast<size_t>(i) * kp, kp, sg.hz_raw.data() + static_cast<size_t>(s) * kp);
		}
	}
	return sg;
}

// Uploads sg's y and z to d_y / d_z and, where sg holds the raw-order copies, those to d_yr / d_zr.  sg must outlive
// the copies (the caller's HostSourceFence).  `who` and `y_name` go into the error text.
int GlmUpload(const GlmStaged &sg, double *d_y, double *d_z, double *d_yr, double *d_zr, hipStream_t st, const char *who,
              const char *y_name, char *errbuf) {
	const auto what = [&](const char *name, const char *tail) { return std::string(who) + " " + name + " upload" + tail; };
	PGH_HIP(hipMemcpyAsync(d_y, sg.hy.data(), 8ull * sg.hy.size(), hipMemcpyHostToDevice, st), what(y_name, "").c_str());
	if (sg.kp) {
		PGH_HIP(hipMemcpyAsync(d_z, sg.hz.data(), 8ull * sg.hz.size(), hipMemcpyHostToDevice, st),
		        what("covariate", "").c_str());
	}
	if (sg.raw) {
		PGH_HIP(hipMemcpyAsync(d_yr, sg.hy_raw.data(), 8ull * sg.hy_raw.size(), hipMemcpyHostToDevice, st),
		        what(y_name, " (raw order)").c_str());
		if (sg.kp) {
			PGH_HIP(hipMemcpyAsync(d_zr, sg.hz_raw.data(), 8ull * sg.hz_raw.size(), hipMemcpyHostToDevice, st),
			        what("covariate", " (raw order)").c_str());
		}
	}
	return PGH_OK;
}

// The dosage tracks of a call over the variants [v_begin, v_end) of a dense-resident dataset.  Its vectors feed
// asynchronous uploads: declare it before the caller's HostSourceFence.
struct GlmDosage {
	const pgh_dataset *ds;
	const pgh_subset *subset;
	uint32_t v_begin, n_out;
	std::vector<int32_t> slot_all; // per variant of the call: >= 0 with a track
	bool any;
	std::vector<int32_t> slot;   // per variant of a chunk: its row of the chunk's dense dosages, or -1
	std::vector<uint32_t> vlist; // the chunk's variants with a track (resident row indices)

	// Once per call: which variants carry a track; with any, *chunk shrinks until a chunk's dense dosage rows keep
	// kGlmDosageBytes.
	GlmDosage(const pgh_dataset *ds_, const pgh_subset *subset_, uint32_t v_begin_, uint32_t v_end, uint32_t *chunk)
	    : ds(ds_), subset(subset_), v_begin(v_begin_), n_out(subset_ ? subset_->n_out : ds_->sample_ct),
	      slot_all(v_end - v_begin_, -1) {
		for (uint32_t v = v_begin; v < v_end && ds->dos_rows; v++) {
			if (ds->dos_row_of[v - ds->v_begin] >= 0) {
				slot_all[v - v_begin] = 0;
			}
		}
		any = std::any_of(slot_all.begin(), slot_all.end(), [](int32_t s) { return s >= 0; });
		if (any) {
			*chunk = static_cast<uint32_t>(
			    std::min<uint64_t>(*chunk, std::max<uint64_t>(1, kGlmDosageBytes / (8ull * std::max(1u, n_out)))));
		}
		slot.resize(*chunk);
		vlist.resize(*chunk);
	}

	// Per chunk: *g for the nv variants from c0 of the call, their tracks unpacked into d_dos (d_slot: each variant's
	// row there) when the chunk has any.
	int Chunk(uint32_t c0, uint32_t nv, int32_t *d_slot, uint32_t *d_list, double *d_dos, hipStream_t st, const char *who,
	          pgh::GlmX *g, char *errbuf) {
		*g = pgh::GlmX {};
		g->view = ds->View();
		g->v0 = v_begin + c0 - ds->v_begin;
		g->n_out = n_out;
		g->sel = subset ? subset->d_sel : nullptr;
		uint32_t n_dos = 0;
		if (any) {
			for (uint32_t i = 0; i < nv; i++) {
				slot[i] = slot_all[c0 + i] >= 0 ? static_cast<int32_t>(n_dos) : -1;
				if (slot[i] >= 0) {
					vlist[n_dos++] = g->v0 + i;
				}
			}
		}
		if (n_dos) {
			const std::string w(who);
			PGH_HIP(hipMemcpyAsync(d_slot, slot.data(), 4ull * nv, hipMemcpyHostToDevice, st),
			        (w + " slot upload").c_str());
			PGH_HIP(hipMemcpyAsync(d_list, vlist.data(), 4ull * n_dos, hipMemcpyHostToDevice, st),
			        (w + " dosage list upload").c_str());
			PGH_HIP(pgh::LaunchDosageUnpack(ds->View(), ds->Dosage(), 0, d_list, n_dos, g->sel, n_out, d_dos, n_out, st),
			        (w + " dosage unpack").c_str());
			g->slot = d_slot;
			g->dos = d_dos;
		}
		return PGH_OK;
	}
};

int GlmOne(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end, const double *phenotype,
           uint32_t k, const double *covariates, int model, int firth, pgh_glm_row *out, char *errbuf) {
	PGH_ENTER(ds);
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	const uint32_t nv_all = v_end - v_begin;
	const uint32_t kp = pgh::GlmPadCovar(k);
	hipStream_t st = PghThreadStream();

	const bool logistic = model == PGH_GLM_LOGISTIC;
	const GlmStaged sg = GlmStage(ds, subset, phenotype, k, covariates, logistic ? GlmCentre::kNone : GlmCentre::kYZ, false);
	const uint32_t n_y = sg.n_y;
	uint32_t chunk = std::min(kGlmChunk, std::max(1u, nv_all));
	GlmDosage dos(ds, subset, v_begin, v_end, &chunk);

	const uint32_t ns = kp + 4, q = k + 2, ne_gram = q * (q + 1) / 2;
	const uint32_t ne_irls = pgh::GlmIrlsEntries(kp), pp = kp + 2;
	const uint64_t hm = static_cast<uint64_t>(pgh::kGlmMaxP) * pgh::kGlmMaxP, n = n_out, c = chunk;
	double *d_y, *d_z, *d_gram, *d_sums, *d_corr, *d_beta, *d_acc, *d_hm, *d_h0, *d_dos;
	pgh_glm_row *d_rows;
	int32_t *d_slot;
	uint32_t *d_list;
	pgh::GlmState *d_st;
	ScratchLayout lay;
	lay.Add(&d_y, n);
	lay.Add(&d_z, n * kp + 1); // one element of slack
	lay.Add(&d_gram, ne_gram);
	lay.Add(&d_sums, c * ns);
	lay.Add(&d_corr, c * ne_gram);
	lay.Add(&d_rows, c);
	lay.Add(&d_slot, c);
	lay.Add(&d_list, c);
	lay.Add(&d_st, c, logistic);
	lay.Add(&d_beta, c * pp, logistic);
	lay.Add(&d_acc, c * ne_irls, logistic);
	lay.Add(&d_hm, c * hm, logistic);
	lay.Add(&d_h0, c * pp * pp, logistic && firth);
	lay.Add(&d_dos, c * n, dos.any);
	void *scratch = nullptr;
	PGH_HIP(PghThreadScratch(lay.total, st, &scratch), "glm scratch");
	lay.Bind(scratch);

	std::vector<uint32_t> flist;
	std::vector<pgh::GlmState> hst;
	HostSourceFence fence(st); // sg, dos, flist feed asynchronous uploads
	PGH_TRY(GlmUpload(sg, d_y, d_z, nullptr, nullptr, st, "glm", "phenotype", errbuf));
	if (!logistic) {
		PGH_HIP(pgh::LaunchGlmGram(nullptr, 1, nullptr, 0, n_y, n_out, d_y, d_z, kp, k, d_gram, st), "glm gram kernel");
	}
	for (uint32_t c0 = 0; c0 < nv_all; c0 += chunk) {
		const uint32_t nv = std::min(chunk, nv_all - c0);
		pgh::GlmX g;
		PGH_TRY(dos.Chunk(c0, nv, d_slot, d_list, d_dos, st, "glm", &g, errbuf));
		if (!logistic) {
			PGH_HIP(pgh::LaunchGlmSums(g, nv, d_y, d_z, kp, d_sums, st), "glm sums kernel");
			PGH_HIP(pgh::LaunchGlmGram(&g, nv, d_sums, ns, n_y, n_out, d_y, d_z, kp, k, d_corr, st), "glm correction kernel");
			PGH_HIP(pgh::LaunchGlmLinearSolve(nv, d_sums, kp, k, d_gram, d_corr, d_rows, st), "glm solve kernel");
		} else {
			PGH_HIP(pgh::LaunchGlmSums(g, nv, d_y, d_z, 0, d_sums, st), "glm sums kernel");
			PGH_HIP(pgh::LaunchGlmLogisticInit(nv, d_sums, kp, k, d_st, d_beta, d_rows, st), "glm logistic init");
			// the Newton rules end every fit by its 15th iteration
			for (int it = 0; it < 15; it++) {
				PGH_HIP(pgh::LaunchGlmIrlsAcc(0, g, nullptr, nv, d_y, d_z, kp, d_st, d_beta, nullptr, d_acc, st),
				        "glm newton pass");
				PGH_HIP(pgh::LaunchGlmNewtonUpdate(nv, kp, k, d_acc, d_st, d_beta, d_hm, st), "glm newton update");
			}
			if (firth) {
				hst.resize(nv);
				PGH_HIP(hipMemcpyAsync(hst.data(), d_st, sizeof(pgh::GlmState) * nv, hipMemcpyDeviceToHost, st),
				        "glm state copy");
				PGH_HIP(hipStreamSynchronize(st), "glm state sync");
				flist.clear();
				for (uint32_t i = 0; i < nv; i++) {
					if (hst[i].status == pgh::kGlmFailed || hst[i].status == pgh::kGlmUnfinished) {
						flist.push_back(i);
					}
				}
				const uint32_t nf = static_cast<uint32_t>(flist.size());
				if (nf) {
					PGH_HIP(hipMemcpyAsync(d_list, flist.data(), 4ull * nf, hipMemcpyHostToDevice, st), "glm firth list");
					PGH_HIP(pgh::LaunchGlmFirthStart(d_list, nf, kp, d_st, d_beta, st), "glm firth start");
					// 25 iterations and the test after the 26th: 27 evaluations at most
					for (int it = 0; it < 27; it++) {
						PGH_HIP(pgh::LaunchGlmIrlsAcc(1, g, d_list, nf, d_y, d_z, kp, d_st, d_beta, nullptr, d_acc, st),
						        "glm firth pass 1");
						PGH_HIP(pgh::LaunchGlmFirthUpdate(0, d_list, nf, kp, k, d_acc, d_st, d_beta, d_h0, d_hm, st),
						        "glm firth update 1");
						PGH_HIP(pgh::LaunchGlmIrlsAcc(2, g, d_list, nf, d_y, d_z, kp, d_st, d_beta, d_h0, d_acc, st),
						        "glm firth pass 2");
						PGH_HIP(pgh::LaunchGlmFirthUpdate(1, d_list, nf, kp, k, d_acc, d_st, d_beta, d_h0, d_hm, st),
						        "glm firth update 2");
					}
				}
			}
			PGH_HIP(pgh::LaunchGlmLogisticFinish(nv, kp, k, d_st, d_beta, d_hm, d_rows, st), "glm logistic finish");
		}
		PGH_HIP(hipMemcpyAsync(out + c0, d_rows, sizeof(pgh_glm_row) * nv, hipMemcpyDeviceToHost, st), "glm rows copy");
		PGH_HIP(hipStreamSynchronize(st), "glm sync");
	}
	return PGH_OK;
}

// pgh_glm_multi, linear: variants per chunk, and the bound of a chunk's scratch (sums, corrections and rows of a
// phenotype block grow with both; dense dosage rows keep kGlmDosageBytes).
constexpr uint32_t kGlmMultiChunk = 65536;
constexpr uint64_t kGlmMultiChunkBytes = 1ull << 30;

// The phenotypes of `phenotypes` (n_pheno x n_out) grouped by missing-value pattern, each group in phenotype order and
// the groups in the order of their first phenotype.
std::vector<std::vector<uint32_t>> GlmPatternGroups(uint32_t n_pheno, const double *phenotypes, uint32_t n_out) {
	const size_t words = (static_cast<size_t>(n_out) + 63) / 64;
	std::vector<uint64_t> masks(words * n_pheno, 0);
	std::unordered_map<uint64_t, std::vector<uint32_t>> by_hash; // hash -> group ids
	std::vector<std::vector<uint32_t>> groups;
	for (uint32_t p = 0; p < n_pheno; p++) {
		uint64_t *m = masks.data() + words * p;
		const double *y = phenotypes + static_cast<size_t>(p) * n_out;
		for (uint32_t i = 0; i < n_out; i++) {
			m[i >> 6] |= static_cast<uint64_t>(std::isnan(y[i])) << (i & 63);
		}
		uint64_t h = 1469598103934665603ull; // FNV-1a over the words
		for (size_t w = 0; w < words; w++) {
			h = (h ^ m[w]) * 1099511628211ull;
		}
		std::vector<uint32_t> &cands = by_hash[h];
		bool placed = false;
		for (uint32_t gi : cands) {
			if (std::equal(m, m + words, masks.data() + words * groups[gi][0])) {
				groups[gi].push_back(p);
				placed = true;
				break;
			}
		}
		if (!placed) {
			cands.push_back(static_cast<uint32_t>(groups.size()));
			groups.push_back({p});
		}
	}
	return groups;
}

// Linear fits of the phenotypes `idx` (one missing-value pattern) over the variants [v_begin, v_end) of one dataset:
// out[(v - v_begin) * n_pheno + idx[j]].  The covariates are centred on the pattern's samples and each phenotype on
// its own mean, as GlmOne does.
int GlmMultiLinear(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end, uint32_t n_pheno,
                   const double *phenotypes, const std::vector<uint32_t> &idx, uint32_t k, const double *covariates,
                   pgh_glm_row *out, char *errbuf) {
	PGH_ENTER(ds);
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	const uint32_t nv_all = v_end - v_begin;
	const uint32_t kp = pgh::GlmPadCovar(k);
	const uint32_t np = static_cast<uint32_t>(idx.size());
	hipStream_t st = PghThreadStream();

	// sg.hy: the group's first phenotype as it is, NaN exactly at the pattern
	const GlmStaged sg = GlmStage(ds, subset, phenotypes + static_cast<size_t>(idx[0]) * n_out, k, covariates, GlmCentre::kZ,
	                              false);
	const uint32_t n_y = sg.n_y;

	const uint32_t pb_max = std::min(pgh::kGlmMultiPb, np);
	const uint32_t ns = kp + 4, q = k + 2, ne_gram = q * (q + 1) / 2, nes = (k + 1) * (k + 2) / 2;
	const uint64_t per_variant = 8ull * (ns + nes) + static_cast<uint64_t>(pb_max) * (8 + 8 * q + sizeof(pgh_glm_row)) + 8;
	uint32_t chunk = std::min(kGlmMultiChunk, std::max(1u, nv_all));
	chunk = static_cast<uint32_t>(std::min<uint64_t>(chunk, std::max<uint64_t>(1, kGlmMultiChunkBytes / per_variant)));
	GlmDosage dos(ds, subset, v_begin, v_end, &chunk);

	const uint64_t n = n_out, c = chunk;
	double *d_pat, *d_z, *d_yb, *d_gram, *d_whole, *d_sums, *d_sxy, *d_cs, *d_cp, *d_dos;
	pgh_glm_row *d_rows;
	int32_t *d_slot;
	uint32_t *d_list;
	ScratchLayout lay;
	lay.Add(&d_pat, n);
	lay.Add(&d_z, n * kp + 1); // one element of slack
	lay.Add(&d_yb, n * pb_max);
	lay.Add(&d_gram, ne_gram);
	lay.Add(&d_whole, static_cast<uint64_t>(pb_max) * q);
	lay.Add(&d_sums, c * ns);
	lay.Add(&d_sxy, c * pb_max);
	lay.Add(&d_cs, c * nes);
	lay.Add(&d_cp, c * pb_max * q);
	lay.Add(&d_rows, c * pb_max);
	lay.Add(&d_slot, c);
	lay.Add(&d_list, c);
	lay.Add(&d_dos, c * n, dos.any);
	void *scratch = nullptr;
	PGH_HIP(PghThreadScratch(lay.total, st, &scratch), "glm_multi scratch");
	lay.Bind(scratch);

	std::vector<double> hyb(static_cast<size_t>(n_out) * pb_max);
	std::vector<pgh_glm_row> hrows(static_cast<size_t>(chunk) * pb_max);
	HostSourceFence fence(st); // sg, dos, hyb feed asynchronous uploads
	PGH_TRY(GlmUpload(sg, d_pat, d_z, nullptr, nullptr, st, "glm_multi", "pattern", errbuf));
	PGH_HIP(pgh::LaunchGlmGram(nullptr, 1, nullptr, 0, n_y, n_out, d_pat, d_z, kp, k, d_gram, st), "glm_multi gram kernel");
	for (uint32_t b0 = 0; b0 < np; b0 += pb_max) {
		const uint32_t pb = std::min(pb_max, np - b0);
		// every upload of the previous block has completed: each chunk below ends with a stream synchronisation
		for (uint32_t j = 0; j < pb; j++) {
			// NaN becomes 0.0 here; GlmStage's single phenotype keeps its NaN
			const double *y = phenotypes + static_cast<size_t>(idx[b0 + j]) * n_out;
			const double my = GlmMean(y, n_out, n_y);
			double *dst = hyb.data() + static_cast<size_t>(j) * n_out;
			for (uint32_t i = 0; i < n_out; i++) {
				dst[i] = std::isnan(y[i]) ? 0.0 : y[i] - my;
			}
		}
		PGH_HIP(hipMemcpyAsync(d_yb, hyb.data(), 8ull * n_out * pb, hipMemcpyHostToDevice, st), "glm_multi phenotype upload");
		PGH_HIP(pgh::LaunchGlmMultiWhole(n_out, d_yb, pb, d_z, kp, k, d_whole, st), "glm_multi whole-call kernel");
		for (uint32_t c0 = 0; c0 < nv_all; c0 += chunk) {
			const uint32_t nv = std::min(chunk, nv_all - c0);
			pgh::GlmX g;
			PGH_TRY(dos.Chunk(c0, nv, d_slot, d_list, d_dos, st, "glm_multi", &g, errbuf));
			PGH_HIP(pgh::LaunchGlmSums(g, nv, d_pat, d_z, kp, d_sums, st), "glm_multi sums kernel");
			PGH_HIP(pgh::LaunchGlmMultiXy(g, nv, d_yb, pb, d_sxy, st), "glm_multi genotype x phenotype kernel");
			PGH_HIP(pgh::LaunchGlmMultiCorr(g, nv, d_sums, n_y, d_pat, d_yb, pb, d_z, kp, k, d_cs, d_cp, st),
			        "glm_multi correction kernel");
			PGH_HIP(pgh::LaunchGlmMultiSolve(nv, pb, d_sums, kp, k, d_sxy, d_gram, d_whole, d_cs, d_cp, d_rows, st),
			        "glm_multi solve kernel");
			PGH_HIP(hipMemcpyAsync(hrows.data(), d_rows, sizeof(pgh_glm_row) * nv * pb, hipMemcpyDeviceToHost, st),
			        "glm_multi rows copy");
			PGH_HIP(hipStreamSynchronize(st), "glm_multi sync");
			for (uint32_t i = 0; i < nv; i++) {
				for (uint32_t j = 0; j < pb; j++) {
					out[static_cast<size_t>(c0 + i) * n_pheno + idx[b0 + j]] = hrows[static_cast<size_t>(i) * pb + j];
				}
			}
		}
	}
	return PGH_OK;
}

// pgh_glm_multi on one dataset (not a group): linear fits by missing-value pattern, logistic fits phenotype by
// phenotype through GlmOne (so their rows are pgh_glm's bit for bit).
int GlmMultiOne(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end, uint32_t n_pheno,
                const double *phenotypes, uint32_t k, const double *covariates, int model, int firth, pgh_glm_row *out,
                char *errbuf) {
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	const uint32_t nv = v_end - v_begin;
	if (model == PGH_GLM_LOGISTIC) {
		std::vector<pgh_glm_row> rows(nv);
		for (uint32_t p = 0; p < n_pheno; p++) {
			PGH_TRY(GlmOne(ds, subset, v_begin, v_end, phenotypes + static_cast<size_t>(p) * n_out, k, covariates, model, firth,
			               rows.data(), errbuf));
			for (uint32_t v = 0; v < nv; v++) {
				out[static_cast<size_t>(v) * n_pheno + p] = rows[v];
			}
		}
		return PGH_OK;
	}
	for (const std::vector<uint32_t> &idx : GlmPatternGroups(n_pheno, phenotypes, n_out)) {
		PGH_TRY(GlmMultiLinear(ds, subset, v_begin, v_end, n_pheno, phenotypes, idx, k, covariates, out, errbuf));
	}
	return PGH_OK;
}

// The argument checks that pgh_glm (n_pheno = 1), pgh_glm_multi and pgh_glm_sparse share: everything but the
// resident form of the dataset.
int GlmCheckCommon(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end, uint32_t n_pheno,
                   const double *phenotypes, uint32_t n_covar, const double *covariates, int model,
                   const pgh_glm_row *out, char *errbuf) {
	PGH_TRY(CheckRange(ds, v_begin, v_end, errbuf));
	if (model != PGH_GLM_LINEAR && model != PGH_GLM_LOGISTIC) {
		SetErr(errbuf, "model must be PGH_GLM_LINEAR or PGH_GLM_LOGISTIC");
		return PGH_ERR_ARG;
	}
	if (n_pheno == 0) {
		SetErr(errbuf, "at least one phenotype is needed");
		return PGH_ERR_ARG;
	}
	if (n_covar > PGH_GLM_MAX_COVAR) {
		SetErr(errbuf, "at most " + std::to_string(PGH_GLM_MAX_COVAR) + " covariates are supported, got " +
		                   std::to_string(n_covar));
		return PGH_ERR_ARG;
	}
	PGH_TRY(CheckSubset(ds, subset, errbuf));
	PGH_TRY(RefuseEmptySubset(subset, errbuf));
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	if ((n_out && !phenotypes) || (n_covar && n_out && !covariates) || (v_end > v_begin && !out)) {
		SetErr(errbuf, "null argument");
		return PGH_ERR_ARG;
	}
	for (uint64_t i = 0; i < static_cast<uint64_t>(n_covar) * n_out; i++) {
		if (!std::isfinite(covariates[i])) {
			SetErr(errbuf, "covariate " + std::to_string(i / n_out) + " is not finite at sample " +
			                   std::to_string(i % n_out));
			return PGH_ERR_ARG;
		}
	}
	return PGH_OK;
}

// The argument checks of pgh_glm (n_pheno = 1) and pgh_glm_multi.
int GlmCheckArgs(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end, uint32_t n_pheno,
                 const double *phenotypes, uint32_t n_covar, const double *covariates, int model, const pgh_glm_row *out,
                 char *errbuf) {
	PGH_DENSE_ROWS(ds);
	return GlmCheckCommon(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, model, out, errbuf);
}

// pgh_glm_sparse on one sparse-resident dataset.  y and z are staged twice when there is a subset: in output-sample
// order for the dense kernels (the whole-call Gram and the dense-form rows), and in raw-sample order, NaN y outside
// the subset, for the entry kernel, whose entries name raw samples.  Without a subset the two orders are one.
int GlmSparseOne(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                 const double *phenotype, uint32_t k, const double *covariates, pgh_glm_row *out, char *errbuf) {
	PGH_ENTER(ds);
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct, n_raw = ds->sample_ct;
	const uint32_t nv_all = v_end - v_begin;
	const uint32_t kp = pgh::GlmPadCovar(k);
	hipStream_t st = PghThreadStream();
	const GlmStaged sg = GlmStage(ds, subset, phenotype, k, covariates, GlmCentre::kYZ, true);
	const uint32_t n_y = sg.n_y;

	const uint32_t chunk = std::min(kGlmChunk, std::max(1u, nv_all));
	// the dense-form rows of a chunk are consecutive pool rows
	const uint32_t l_begin = v_begin - ds->v_begin;
	uint32_t dense_max = 0;
	for (uint32_t c0 = 0; c0 < nv_all; c0 += chunk) {
		const uint32_t l0 = l_begin + c0, l1 = l0 + std::min(chunk, nv_all - c0);
		dense_max = std::max(dense_max, ds->sp_dense_before[l1] - ds->sp_dense_before[l0]);
	}
	const uint32_t ns = kp + 4, q = k + 2, ne_gram = q * (q + 1) / 2;
	const uint64_t n = n_out, nr = n_raw, c = chunk, dm = dense_max;
	double *d_y, *d_z, *d_gram, *d_yr, *d_zr, *d_sums, *d_corr, *d_dsums, *d_dcorr;
	pgh_glm_row *d_rows, *d_drows;
	ScratchLayout lay;
	lay.Add(&d_y, n);
	lay.Add(&d_z, n * kp + 1); // one element of slack, here and in d_zr
	lay.Add(&d_gram, ne_gram);
	lay.Add(&d_yr, nr, subset != nullptr);
	lay.Add(&d_zr, nr * kp + 1, subset != nullptr);
	lay.Add(&d_sums, c * ns);
	lay.Add(&d_corr, c * ne_gram);
	lay.Add(&d_rows, c);
	lay.Add(&d_dsums, dm * ns);
	lay.Add(&d_dcorr, dm * ne_gram);
	lay.Add(&d_drows, dm);
	void *scratch = nullptr;
	PGH_HIP(PghThreadScratch(lay.total, st, &scratch), "glm_sparse scratch");
	lay.Bind(scratch);
	if (!subset) {
		d_yr = d_y;
		d_zr = d_z;
	}

	std::vector<pgh_glm_row> hdrows(dense_max);
	HostSourceFence fence(st); // sg feeds asynchronous uploads
	PGH_TRY(GlmUpload(sg, d_y, d_z, d_yr, d_zr, st, "glm_sparse", "phenotype", errbuf));
	PGH_HIP(pgh::LaunchGlmGram(nullptr, 1, nullptr, 0, n_y, n_out, d_y, d_z, kp, k, d_gram, st), "glm_sparse gram kernel");
	for (uint32_t c0 = 0; c0 < nv_all; c0 += chunk) {
		const uint32_t nv = std::min(chunk, nv_all - c0);
		const uint32_t l0 = l_begin + c0;
		PGH_HIP(pgh::LaunchGlmSparse(ds->Sparse(), l0, nv, d_yr, d_zr, kp, k, n_y, d_gram, d_sums, d_corr, st),
		        "glm_sparse entry kernel");
		PGH_HIP(pgh::LaunchGlmLinearSolve(nv, d_sums, kp, k, d_gram, d_corr, d_rows, st), "glm_sparse solve kernel");
		PGH_HIP(hipMemcpyAsync(out + c0, d_rows, sizeof(pgh_glm_row) * nv, hipMemcpyDeviceToHost, st), "glm_sparse rows copy");
		// the dense-form rows: pgh_glm's kernels over their pool rows
		const uint32_t dense_first = ds->sp_dense_before[l0];
		const uint32_t dense_ct = ds->sp_dense_before[l0 + nv] - dense_first;
		if (dense_ct) {
			pgh::GlmX g {};
			g.view = ds->PoolView();
			g.v0 = dense_first;
			g.n_out = n_out;
			g.sel = subset ? subset->d_sel : nullptr;
			PGH_HIP(pgh::LaunchGlmSums(g, dense_ct, d_y, d_z, kp, d_dsums, st), "glm_sparse sums kernel (dense pool)");
			PGH_HIP(pgh::LaunchGlmGram(&g, dense_ct, d_dsums, ns, n_y, n_out, d_y, d_z, kp, k, d_dcorr, st),
			        "glm_sparse correction kernel (dense pool)");
			PGH_HIP(pgh::LaunchGlmLinearSolve(dense_ct, d_dsums, kp, k, d_gram, d_dcorr, d_drows, st),
			        "glm_sparse solve kernel (dense pool)");
			PGH_HIP(hipMemcpyAsync(hdrows.data(), d_drows, sizeof(pgh_glm_row) * dense_ct, hipMemcpyDeviceToHost, st),
			        "glm_sparse rows copy (dense pool)");
		}
		PGH_HIP(hipStreamSynchronize(st), "glm_sparse sync");
		for (uint32_t i = 0, j = 0; i < nv && j < dense_ct; i++) {
			if (ds->sp_dense_before[l0 + i + 1] != ds->sp_dense_before[l0 + i]) {
				out[c0 + i] = hdrows[j++];
			}
		}
	}
	return PGH_OK;
}

// The covariates-only logistic fit of pgh_glm_score_sparse: Newton steps from beta = 0, each one evaluation on the
// device (LaunchGlmScoreNull) and a (k + 1)-wide Cholesky step here.  On return r, w and hg on the device are those of
// the last beta evaluated: the final one when the fit converged.  *status: PGH_GLM_OK, SINGULAR_MATRIX (a pivot failed
// at the first step, where every w is 1/4: collinear covariates) or NO_CONVERGENCE.  With fit == false (too few
// samples for any row) only beta = 0 is evaluated, which stages r's NaN pattern for the entry kernel's counts.
int GlmScoreNullFit(uint32_t n_out, const double *d_y, const double *d_z, uint32_t kp, uint32_t k, const uint32_t *d_sel,
                    bool fit, double *d_r, double *d_w, double *d_part, double *d_hg, hipStream_t st, int *status,
                    char *errbuf) {
	constexpr int kMaxSteps = 25;
	constexpr int M = PGH_GLM_MAX_COVAR + 1;
	const int q1 = static_cast<int>(k) + 1, nh = q1 * (q1 + 1) / 2;
	pgh::GlmScoreBeta beta {};
	std::vector<double> hg(nh + q1);
	double a[M * M], delta[M];
	*status = PGH_GLM_OK;
	bool final = !fit;
	for (int step = 0;; step++) {
		PGH_HIP(pgh::LaunchGlmScoreNull(n_out, d_y, d_z, kp, k, beta, d_sel, d_r, d_w, d_part, d_hg, st),
		        "glm_score_sparse null kernel");
		if (final) {
			return PGH_OK; // what the device holds is the fitted model's
		}
		if (step == kMaxSteps) {
			*status = PGH_GLM_NO_CONVERGENCE;
			return PGH_OK;
		}
		PGH_HIP(hipMemcpyAsync(hg.data(), d_hg, 8ull * hg.size(), hipMemcpyDeviceToHost, st), "glm_score_sparse null copy");
		PGH_HIP(hipStreamSynchronize(st), "glm_score_sparse null sync");
		for (int ia = 0, e = 0; ia < q1; ia++) {
			for (int ib = ia; ib < q1; ib++, e++) {
				a[ib * M + ia] = hg[e];
			}
		}
		if (!pgh::GlmCholesky(a, q1, M, 1e-10, nullptr)) {
			*status = step == 0 ? PGH_GLM_SINGULAR_MATRIX : PGH_GLM_NO_CONVERGENCE;
			return PGH_OK;
		}
		std::copy_n(hg.data() + nh, q1, delta);
		pgh::GlmCholSolve(a, q1, M, delta);
		double dmax = 0.0;
		bool finite = true;
		for (int j = 0; j < q1; j++) {
			finite = finite && std::isfinite(delta[j]) && std::isfinite(beta.b[j] + delta[j]);
			dmax = std::max(dmax, std::fabs(delta[j]));
		}
		if (!finite) {
			*status = PGH_GLM_NO_CONVERGENCE;
			return PGH_OK;
		}
		for (int j = 0; j < q1; j++) {
			beta.b[j] += delta[j];
		}
		final = dmax <= 1e-10; // converged: one more evaluation, at the final beta
	}
}

// What a call of a score-test route does after a chunk of rows: nothing; the saddlepoint kernel (GlmScoreSpaKernel,
// GlmScoreDenseSpaKernel, GlmScoreSparseMultiSpaKernel), which replaces the p-value of the rows beyond the cutoff
// (pgh_glm_score_sparse_spa, pgh_glm_score_multi_spa, pgh_glm_score_sparse_multi_spa); or the Firth kernel
// (GlmScoreSparseFirthKernel, GlmScoreDenseFirthKernel, GlmScoreSparseMultiFirthKernel), which leaves every row's
// pgh_glm_firth_row (pgh_glm_score_sparse_firth, pgh_glm_score_multi_firth, pgh_glm_score_sparse_multi_firth).  One of
// the three; the outputs belong to the kind.
struct GlmScoreFollowUp {
	enum Kind { kNone, kSpa, kFirth };
	Kind kind = kNone;
	double cutoff = 0.0;
	double *p_spa = nullptr;            // kSpa
	uint8_t *state = nullptr;           // kSpa
	pgh_glm_firth_row *firth = nullptr; // kFirth
};

// pgh_glm_score_sparse on one sparse-resident dataset.  y and z are staged in output-sample order for the null fit,
// which leaves r and w in raw-sample order (NaN r outside the subset: uploaded so, the fit writes the subset's
// samples only); z is staged a second time in raw-sample order when there is a subset, as in GlmSparseOne.
// fu.kind == kSpa (pgh_glm_score_sparse_spa): after a chunk's rows, GlmScoreSpaKernel replaces the p-value of the rows
// beyond the cutoff.  kFirth (pgh_glm_score_sparse_firth): GlmScoreSparseFirthKernel writes the chunk's
// pgh_glm_firth_rows.  Either way the workgroup form's stashes are cut from the same scratch block, within
// kSpaStashBytes.
constexpr uint64_t kSpaStashBytes = 256ull << 20;

int GlmScoreSparseOne(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                      const double *phenotype, uint32_t k, const double *covariates, pgh_glm_row *out, char *errbuf,
                      const GlmScoreFollowUp &fu = GlmScoreFollowUp()) {
	PGH_ENTER(ds);
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct, n_raw = ds->sample_ct;
	const uint32_t nv_all = v_end - v_begin;
	const uint32_t kp = pgh::GlmPadCovar(k);
	hipStream_t st = PghThreadStream();
	const GlmStaged sg = GlmStage(ds, subset, phenotype, k, covariates, GlmCentre::kZ, true);
	const uint32_t n_y = sg.n_y;

	const uint32_t chunk = std::min(kGlmChunk, std::max(1u, nv_all));
	const uint32_t l_begin = v_begin - ds->v_begin;
	const uint32_t ns = kp + 6, ne = (k + 1) * (k + 2) / 2 + k + 1;
	const uint64_t n = n_out, nr = n_raw, c = chunk;
	double *d_y, *d_z, *d_zr, *d_r, *d_w, *d_part, *d_hg, *d_sums, *d_hgn;
	pgh_glm_row *d_rows;
	ScratchLayout lay;
	lay.Add(&d_y, n);
	lay.Add(&d_z, n * kp + 1); // one element of slack, here and in d_zr
	lay.Add(&d_zr, nr * kp + 1, subset != nullptr);
	lay.Add(&d_r, nr);
	lay.Add(&d_w, nr);
	lay.Add(&d_part, static_cast<uint64_t>(pgh::kGlmScoreNullParts) * ne);
	lay.Add(&d_hg, ne);
	lay.Add(&d_sums, c * ns);
	lay.Add(&d_hgn, c * ne);
	lay.Add(&d_rows, c);
	// the saddlepoint path: [t, U, V], p_spa and the state per chunk variant; the Firth path: a pgh_glm_firth_row per
	// chunk variant; both: a stash per workgroup of the workgroup form, at most four workgroups per compute unit
	const bool spa = fu.kind == GlmScoreFollowUp::kSpa, firth = fu.kind == GlmScoreFollowUp::kFirth;
	pgh::GlmScoreSpaOut so;
	pgh_glm_firth_row *d_firth = nullptr;
	uint8_t *d_stash = nullptr;
	uint32_t n_groups = 0;
	if (spa || firth) {
		const uint64_t per_group = pgh::GlmScoreSpaStashPerGroup(n_raw);
		PGH_TRY(StashGroups(chunk, 4, per_group, kSpaStashBytes, &n_groups,
		                    spa ? "glm_score_sparse_spa" : "glm_score_sparse_firth", errbuf));
		lay.Add(&so.t, c * (kp + 3), spa);
		lay.Add(&so.p_spa, c, spa);
		lay.Add(&so.state, c, spa);
		lay.Add(&d_firth, c, firth);
		lay.Add(&d_stash, per_group * n_groups);
	}
	void *scratch = nullptr;
	PGH_HIP(PghThreadScratch(lay.total, st, &scratch), "glm_score_sparse scratch");
	lay.Bind(scratch);
	if (!subset) {
		d_zr = d_z;
	}

	HostSourceFence fence(st); // sg feeds asynchronous uploads
	PGH_TRY(GlmUpload(sg, d_y, d_z, d_r, d_zr, st, "glm_score_sparse", "phenotype", errbuf));
	if (subset) {
		PGH_HIP(hipMemsetAsync(d_w, 0, 8ull * nr, st), "glm_score_sparse weight clear");
	}
	int null_status = PGH_GLM_OK;
	PGH_TRY(GlmScoreNullFit(n_out, d_y, d_z, kp, k, subset ? subset->d_sel : nullptr, n_y >= k + 3, d_r, d_w, d_part, d_hg, st,
	                        &null_status, errbuf));
	for (uint32_t c0 = 0; c0 < nv_all; c0 += chunk) {
		const uint32_t nv = std::min(chunk, nv_all - c0);
		PGH_HIP(pgh::LaunchGlmScoreSparse(ds->Sparse(), l_begin + c0, nv, d_r, d_w, d_zr, kp, k, n_y, d_hg, d_sums, d_hgn, st),
		        "glm_score_sparse entry kernel");
		PGH_HIP(pgh::LaunchGlmScoreSolve(nv, d_sums, kp, k, d_hgn, null_status, d_rows, st, so),
		        "glm_score_sparse solve kernel");
		PGH_HIP(hipMemcpyAsync(out + c0, d_rows, sizeof(pgh_glm_row) * nv, hipMemcpyDeviceToHost, st),
		        "glm_score_sparse rows copy");
		if (spa) {
			PGH_HIP(pgh::LaunchGlmScoreSpa(ds->Sparse(), l_begin + c0, nv, d_r, d_w, d_zr, kp, d_rows, so.t, fu.cutoff,
			                               n_groups, d_stash, so.p_spa, so.state, st),
			        "glm_score_sparse_spa kernel");
			PGH_HIP(hipMemcpyAsync(fu.p_spa + c0, so.p_spa, 8ull * nv, hipMemcpyDeviceToHost, st),
			        "glm_score_sparse_spa p copy");
			PGH_HIP(hipMemcpyAsync(fu.state + c0, so.state, nv, hipMemcpyDeviceToHost, st),
			        "glm_score_sparse_spa state copy");
		} else if (firth) {
			PGH_HIP(pgh::LaunchGlmScoreSparseFirth(ds->Sparse(), l_begin + c0, nv, d_r, d_rows, fu.cutoff, n_groups, d_stash,
			                                       d_firth, st),
			        "glm_score_sparse_firth kernel");
			PGH_HIP(hipMemcpyAsync(fu.firth + c0, d_firth, sizeof(pgh_glm_firth_row) * nv, hipMemcpyDeviceToHost, st),
			        "glm_score_sparse_firth rows copy");
		}
		PGH_HIP(hipStreamSynchronize(st), "glm_score_sparse sync");
	}
	return PGH_OK;
}

constexpr uint64_t kBurdenScratchBytes = 1ull << 30;
const char *const kBurdenScratchEnv = "PGH_BURDEN_SCRATCH_BYTES";

// The byte budget of the workgroups' private vectors (read at every call; the result does not depend on it: it only
// bounds how many sets are in flight, and anything below one vector still gives one workgroup).
uint64_t BurdenScratchBytes() {
	return EnvBytes(kBurdenScratchEnv, kBurdenScratchBytes);
}

// pgh_burden_sparse on one sparse-resident dataset, after the argument checks.  n_memb = set_off[n_sets].
int BurdenSparseOne(const pgh_dataset *ds, const pgh_subset *subset, const double *phenotype, uint32_t k,
                    const double *covariates, uint32_t n_sets, const uint64_t *set_off, const uint32_t *set_vidx,
                    const double *weight, pgh_burden_row *out, char *errbuf) {
	PGH_ENTER(ds);
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct, n_raw = ds->sample_ct;
	const uint32_t kp = pgh::GlmPadCovar(k);
	const uint64_t n_memb = set_off[n_sets];
	hipStream_t st = PghThreadStream();
	const GlmStaged sg = GlmStage(ds, subset, phenotype, k, covariates, GlmCentre::kYZ, true);
	const uint32_t n_y = sg.n_y;

	// the grid: a private vector per workgroup within the byte budget, at most eight workgroups per compute unit
	const uint64_t per_group = pgh::BurdenScratchPerGroup(n_raw);
	uint32_t n_groups = 0;
	PGH_TRY(StashGroups(n_sets, 8, per_group, BurdenScratchBytes(), &n_groups, "burden_sparse", errbuf));
	DevBuf vectors;
	PGH_HIP(vectors.Alloc(per_group * n_groups), "burden_sparse vectors");

	const uint32_t ns = kp + 4, q = k + 2, ne_gram = q * (q + 1) / 2;
	const uint64_t n = n_out, nr = n_raw, nsets = n_sets, ctr_bytes = 256;
	double *d_y, *d_z, *d_gram, *d_yr, *d_zr, *d_w, *d_sums;
	uint64_t *d_off;
	uint32_t *d_vidx, *d_ctr;
	pgh::BurdenAux *d_aux;
	uint8_t *d_flag;
	pgh_glm_row *d_rows;
	ScratchLayout lay;
	lay.Add(&d_y, n);
	lay.Add(&d_z, n * kp + 1); // one element of slack, here and in d_zr, d_vidx, d_w
	lay.Add(&d_gram, ne_gram);
	lay.Add(&d_yr, nr, subset != nullptr);
	lay.Add(&d_zr, nr * kp + 1, subset != nullptr);
	lay.Add(&d_off, nsets + 1);
	lay.Add(&d_vidx, n_memb + 1);
	lay.Add(&d_w, n_memb + 1, weight != nullptr);
	lay.Add(&d_ctr, ctr_bytes / 4);
	lay.Add(&d_sums, nsets * ns);
	lay.Add(&d_aux, nsets);
	lay.Add(&d_flag, nsets);
	lay.Add(&d_rows, nsets);
	void *scratch = nullptr;
	PGH_HIP(PghThreadScratch(lay.total, st, &scratch), "burden_sparse scratch");
	lay.Bind(scratch);
	if (!subset) {
		d_yr = d_y;
		d_zr = d_z;
	}

	std::vector<pgh_glm_row> rows(n_sets);
	std::vector<pgh::BurdenAux> aux(n_sets);
	HostSourceFence fence(st); // sg's vectors and the caller's set arrays feed asynchronous uploads
	PGH_TRY(GlmUpload(sg, d_y, d_z, d_yr, d_zr, st, "burden_sparse", "phenotype", errbuf));
	PGH_HIP(hipMemcpyAsync(d_off, set_off, 8ull * (n_sets + 1ull), hipMemcpyHostToDevice, st), "burden_sparse set upload");
	if (n_memb) {
		PGH_HIP(hipMemcpyAsync(d_vidx, set_vidx, 4ull * n_memb, hipMemcpyHostToDevice, st), "burden_sparse member upload");
		if (weight) {
			PGH_HIP(hipMemcpyAsync(d_w, weight, 8ull * n_memb, hipMemcpyHostToDevice, st), "burden_sparse weight upload");
		}
	}
	// zeroed at every call: nothing is assumed of what an earlier call, or another user of the block, left there
	PGH_HIP(hipMemsetAsync(vectors.p, 0, per_group * n_groups, st), "burden_sparse vectors clear");
	PGH_HIP(hipMemsetAsync(d_ctr, 0, ctr_bytes, st), "burden_sparse counter clear");
	PGH_HIP(pgh::LaunchGlmGram(nullptr, 1, nullptr, 0, n_y, n_out, d_y, d_z, kp, k, d_gram, st), "burden_sparse gram kernel");
	PGH_HIP(pgh::LaunchBurdenSparse(ds->Sparse(), n_sets, d_off, d_vidx, d_w, d_yr, d_zr, kp, k, n_y, n_groups, vectors.p,
	                                d_ctr, d_sums, d_aux, d_flag, st),
	        "burden_sparse set kernel");
	PGH_HIP(pgh::LaunchGlmLinearSolve(n_sets, d_sums, kp, k, d_gram, nullptr, d_rows, st, d_flag),
	        "burden_sparse solve kernel");
	PGH_HIP(hipMemcpyAsync(rows.data(), d_rows, sizeof(pgh_glm_row) * n_sets, hipMemcpyDeviceToHost, st),
	        "burden_sparse rows copy");
	PGH_HIP(hipMemcpyAsync(aux.data(), d_aux, sizeof(pgh::BurdenAux) * n_sets, hipMemcpyDeviceToHost, st),
	        "burden_sparse sums copy");
	PGH_HIP(hipStreamSynchronize(st), "burden_sparse sync");
	for (uint32_t s = 0; s < n_sets; s++) {
		pgh_burden_row r;
		std::memset(&r, 0, sizeof r);
		r.beta = rows[s].beta;
		r.se = rows[s].se;
		r.stat = rows[s].stat;
		r.p = rows[s].p;
		r.mean = n_y ? aux[s].c + aux[s].sum_d / n_y : std::nan("");
		r.obs_ct = n_y;
		r.n_nonzero = aux[s].n_nonzero;
		r.errcode = rows[s].errcode;
		out[s] = r;
	}
	return PGH_OK;
}


constexpr uint64_t kSkatScratchBytes = 1ull << 30;
const char *const kSkatScratchEnv = "PGH_SKAT_SCRATCH_BYTES";

// One set's row and eigenvalues from the kernel's sums (LaunchSkatSparse's layout at `sums`), in FP64.  chol: the lower
// Cholesky factor of H (stride M); yg = L^-1 g_S.  With Y_j = L^-1 c_j, c_j' H^-1 c_l = Y_j . Y_l and t_j' g_S =
// Y_j . yg, so Phi is symmetric as it is computed.  omega: the set's weights, null = 1.0.  lambda (m doubles) is
// written only for a decided row; work is the caller's, reused across the sets.
struct SkatWork {
	std::vector<double> y, u, phi, km, lam;
};
void SkatFinishSet(uint32_t m, uint32_t kp, uint32_t k, const double *sums, const double *omega, const double *chol,
                   const double *yg, int null_status, uint32_t n_y, const pgh::SkatSetCounts &cnt, SkatWork &wk,
                   pgh_skat_row *row, double *lambda) {
	constexpr int M = PGH_GLM_MAX_COVAR + 1;
	const double nan = std::nan("");
	std::memset(row, 0, sizeof *row);
	row->q = row->p_skat = row->beta = row->se = row->stat = row->p = row->lambda_sum = row->lambda_max = nan;
	row->obs_ct = n_y;
	row->n_carriers = cnt.n_carriers;
	if (n_y < k + 3) {
		row->errcode = PGH_GLM_TOO_FEW_SAMPLES;
		return;
	}
	if (cnt.n_carriers == 0 || cnt.n_nonzero == 0) {
		row->errcode = PGH_GLM_CONST_ALLELE;
		return;
	}
	if (null_status != PGH_GLM_OK) {
		row->errcode = static_cast<uint8_t>(null_status);
		return;
	}
	const uint32_t q1 = k + 1, nc = kp + 1;
	const double *a = sums, *c = a + static_cast<uint64_t>(m) * (m + 1) / 2, *u0 = c + static_cast<uint64_t>(m) * nc;
	wk.y.resize(static_cast<size_t>(m) * q1);
	wk.u.resize(m);
	wk.phi.resize(static_cast<size_t>(m) * m);
	wk.km.resize(static_cast<size_t>(m) * m);
	wk.lam.resize(m);
	for (uint32_t j = 0; j < m; j++) {
		double *yj = wk.y.data() + static_cast<size_t>(j) * q1;
		double dot = 0.0;
		for (uint32_t i = 0; i < q1; i++) {
			double t = c[static_cast<uint64_t>(j) * nc + i];
			for (uint32_t e = 0; e < i; e++) {
				t -= chol[i * M + e] * yj[e];
			}
			yj[i] = t / chol[i * M + i];
			dot += yj[i] * yg[i];
		}
		wk.u[j] = u0[j] - dot;
	}
	double q = 0.0, trace = 0.0, ub = 0.0, vb = 0.0, ab = 0.0;
	bool finite = true;
	for (uint32_t j = 0; j < m; j++) {
		const double wj = omega ? omega[j] : 1.0;
		const double *yj = wk.y.data() + static_cast<size_t>(j) * q1;
		q += wj * wj * wk.u[j] * wk.u[j];
		ub += wj * wk.u[j];
		for (uint32_t l = j; l < m; l++) {
			const double wl = omega ? omega[l] : 1.0;
			const double *yl = wk.y.data() + static_cast<size_t>(l) * q1;
			const double ajl = a[static_cast<uint64_t>(j) * m - static_cast<uint64_t>(j) * (j + 1) / 2 + l];
			double dot = 0.0;
			for (uint32_t i = 0; i < q1; i++) {
				dot += yj[i] * yl[i];
			}
			const double phi = ajl - dot, kjl = wj * wl * phi;
			wk.phi[static_cast<size_t>(j) * m + l] = wk.phi[static_cast<size_t>(l) * m + j] = phi;
			wk.km[static_cast<size_t>(j) * m + l] = wk.km[static_cast<size_t>(l) * m + j] = kjl;
			finite = finite && std::isfinite(kjl);
			const double twice = l == j ? 1.0 : 2.0;
			vb += twice * kjl;
			ab += twice * wj * wl * ajl;
			trace += l == j ? kjl : 0.0;
		}
	}
	if (finite) {
		pgh::SymmetricEigenvalues(wk.km.data(), m, wk.lam.data());
	}
	if (!finite || !std::isfinite(wk.lam[0]) || !(wk.lam[0] > 0.0)) {
		row->errcode = PGH_GLM_ZERO_VARIANCE;
		return;
	}
	row->errcode = PGH_GLM_OK;
	uint32_t used = 0;
	while (used < m && wk.lam[used] > 1e-10 * wk.lam[0]) { // (descending: the used eigenvalues come first)
		used++;
	}
	row->q = q;
	row->lambda_sum = trace;
	row->lambda_max = wk.lam[0];
	row->n_lambda = used;
	row->p_skat = pgh::SkatPFromLambda(q, wk.lam.data(), used, &row->p_state);
	if (vb > 1e-10 * ab) {
		row->beta = ub / vb;
		row->se = 1.0 / std::sqrt(vb);
		row->stat = ub / std::sqrt(vb);
		row->p = pgh::GlmPFromZ(row->stat);
	}
	std::copy_n(wk.lam.data(), m, lambda);
}

// pgh_skat_sparse on one sparse-resident dataset, after the argument checks.  The staging and the null fit are
// GlmScoreSparseOne's; the sets are taken in chunks of consecutive sets whose sums fit the scratch budget, every chunk
// one launch of LaunchSkatSparse and a host pass over its sets.  out and lambda_out are written only when every chunk
// has been served.
int SkatSparseOne(const pgh_dataset *ds, const pgh_subset *subset, const double *phenotype, uint32_t k,
                  const double *covariates, uint32_t n_sets, const uint64_t *set_off, const uint32_t *set_vidx,
                  const double *weight, pgh_skat_row *out, double *lambda_out, char *errbuf) {
	PGH_ENTER(ds);
	constexpr int M = PGH_GLM_MAX_COVAR + 1;
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct, n_raw = ds->sample_ct;
	const uint32_t kp = pgh::GlmPadCovar(k);
	const uint64_t n_memb = set_off[n_sets];
	hipStream_t st = PghThreadStream();
	const GlmStaged sg = GlmStage(ds, subset, phenotype, k, covariates, GlmCentre::kZ, true);
	const uint32_t n_y = sg.n_y;

	// the grid and the chunks: the workgroups' private vectors take at most half of the byte budget (one vector at
	// least, eight workgroups per compute unit at most), a chunk's sums the rest (one set at least)
	const uint64_t budget = EnvBytes(kSkatScratchEnv, kSkatScratchBytes);
	const uint64_t per_group = pgh::BurdenScratchPerGroup(n_raw);
	uint32_t n_groups = 0;
	PGH_TRY(StashGroups(n_sets, 8, per_group, budget / 2, &n_groups, "skat_sparse", errbuf));
	const uint64_t vec_bytes = per_group * n_groups;
	uint64_t largest = 0;
	for (uint32_t s = 0; s < n_sets; s++) {
		largest = std::max(largest, pgh::SkatSetDoubles(set_off[s + 1] - set_off[s], kp));
	}
	const uint64_t chunk_doubles = std::max<uint64_t>(std::max<uint64_t>(largest, 1), (budget > vec_bytes ? budget - vec_bytes : 0) / 8);
	// out_off[s]: where set s starts in its chunk's sums; chunk_first: the first set of every chunk, then n_sets
	std::vector<uint64_t> out_off(n_sets);
	std::vector<uint32_t> chunk_first;
	uint64_t fill = 0, region = 0;
	for (uint32_t s = 0; s < n_sets; s++) {
		const uint64_t need = pgh::SkatSetDoubles(set_off[s + 1] - set_off[s], kp);
		if (s == 0 || fill + need > chunk_doubles) {
			chunk_first.push_back(s);
			fill = 0;
		}
		out_off[s] = fill;
		fill += need;
		region = std::max(region, fill);
	}
	chunk_first.push_back(n_sets);
	DevBuf vectors, sums;
	PGH_HIP(vectors.Alloc(vec_bytes), "skat_sparse vectors");
	PGH_HIP(sums.Alloc(8 * region), "skat_sparse sums");

	const uint32_t ne = (k + 1) * (k + 2) / 2 + k + 1;
	const uint64_t n = n_out, nr = n_raw, nsets = n_sets, ctr_bytes = 256;
	double *d_y, *d_z, *d_zr, *d_r, *d_w, *d_part, *d_hg;
	uint64_t *d_off, *d_out_off;
	uint32_t *d_vidx, *d_ctr;
	pgh::SkatSetCounts *d_counts;
	ScratchLayout lay;
	lay.Add(&d_y, n);
	lay.Add(&d_z, n * kp + 1); // one element of slack, here and in d_zr, d_vidx
	lay.Add(&d_zr, nr * kp + 1, subset != nullptr);
	lay.Add(&d_r, nr);
	lay.Add(&d_w, nr);
	lay.Add(&d_part, static_cast<uint64_t>(pgh::kGlmScoreNullParts) * ne);
	lay.Add(&d_hg, ne);
	lay.Add(&d_off, nsets + 1);
	lay.Add(&d_out_off, nsets);
	lay.Add(&d_vidx, n_memb + 1);
	lay.Add(&d_ctr, ctr_bytes / 4);
	lay.Add(&d_counts, nsets);
	void *scratch = nullptr;
	PGH_HIP(PghThreadScratch(lay.total, st, &scratch), "skat_sparse scratch");
	lay.Bind(scratch);
	if (!subset) {
		d_zr = d_z;
	}

	std::vector<pgh_skat_row> rows(n_sets);
	std::vector<double> lam(std::max<uint64_t>(n_memb, 1), std::nan("")), hsums(std::max<uint64_t>(region, 1)), hg(ne);
	std::vector<pgh::SkatSetCounts> counts(n_sets);
	HostSourceFence fence(st); // sg's vectors, out_off and the caller's set arrays feed asynchronous uploads
	PGH_TRY(GlmUpload(sg, d_y, d_z, d_r, d_zr, st, "skat_sparse", "phenotype", errbuf));
	if (subset) {
		PGH_HIP(hipMemsetAsync(d_w, 0, 8ull * nr, st), "skat_sparse weight clear");
	}
	PGH_HIP(hipMemcpyAsync(d_off, set_off, 8ull * (n_sets + 1ull), hipMemcpyHostToDevice, st), "skat_sparse set upload");
	PGH_HIP(hipMemcpyAsync(d_out_off, out_off.data(), 8ull * n_sets, hipMemcpyHostToDevice, st), "skat_sparse offset upload");
	if (n_memb) {
		PGH_HIP(hipMemcpyAsync(d_vidx, set_vidx, 4ull * n_memb, hipMemcpyHostToDevice, st), "skat_sparse member upload");
	}
	// zeroed at every call: nothing is assumed of what an earlier call, or another user of the block, left there
	PGH_HIP(hipMemsetAsync(vectors.p, 0, vec_bytes, st), "skat_sparse vectors clear");
	int null_status = PGH_GLM_OK;
	PGH_TRY(GlmScoreNullFit(n_out, d_y, d_z, kp, k, subset ? subset->d_sel : nullptr, n_y >= k + 3, d_r, d_w, d_part, d_hg, st,
	                        &null_status, errbuf));
	// the Cholesky factor of the final H and L^-1 g_S
	double chol[M * M] = {}, yg[M] = {};
	const bool fitted = n_y >= k + 3 && null_status == PGH_GLM_OK;
	if (fitted) {
		PGH_HIP(hipMemcpyAsync(hg.data(), d_hg, 8ull * ne, hipMemcpyDeviceToHost, st), "skat_sparse null copy");
		PGH_HIP(hipStreamSynchronize(st), "skat_sparse null sync");
		const uint32_t q1 = k + 1, nh = q1 * (q1 + 1) / 2;
		for (uint32_t ia = 0, e = 0; ia < q1; ia++) {
			for (uint32_t ib = ia; ib < q1; ib++, e++) {
				chol[ib * M + ia] = hg[e];
			}
		}
		if (!pgh::GlmCholesky(chol, static_cast<int>(q1), M, 1e-10, nullptr)) {
			null_status = PGH_GLM_SINGULAR_MATRIX; // (the fit factored this H up to its last step of at most 1e-10)
		}
		for (uint32_t i = 0; i < q1 && null_status == PGH_GLM_OK; i++) {
			double t = hg[nh + i];
			for (uint32_t e = 0; e < i; e++) {
				t -= chol[i * M + e] * yg[e];
			}
			yg[i] = t / chol[i * M + i];
		}
	}
	SkatWork wk;
	for (size_t ci = 0; ci + 1 < chunk_first.size(); ci++) {
		const uint32_t s0 = chunk_first[ci], ns = chunk_first[ci + 1] - s0;
		const uint64_t used = out_off[s0 + ns - 1] + pgh::SkatSetDoubles(set_off[s0 + ns] - set_off[s0 + ns - 1], kp);
		PGH_HIP(hipMemsetAsync(d_ctr, 0, ctr_bytes, st), "skat_sparse counter clear");
		PGH_HIP(pgh::LaunchSkatSparse(ds->Sparse(), ns, d_off + s0, d_vidx, d_r, d_w, d_zr, kp, k, std::min(n_groups, ns),
		                              vectors.p, d_ctr, d_out_off + s0, sums.As<double>(), d_counts + s0, st),
		        "skat_sparse set kernel");
		if (used) {
			PGH_HIP(hipMemcpyAsync(hsums.data(), sums.p, 8ull * used, hipMemcpyDeviceToHost, st), "skat_sparse sums copy");
		}
		PGH_HIP(hipMemcpyAsync(counts.data() + s0, d_counts + s0, sizeof(pgh::SkatSetCounts) * ns, hipMemcpyDeviceToHost, st),
		        "skat_sparse counts copy");
		PGH_HIP(hipStreamSynchronize(st), "skat_sparse sync");
		for (uint32_t s = s0; s < s0 + ns; s++) {
			const uint64_t m0 = set_off[s];
			SkatFinishSet(static_cast<uint32_t>(set_off[s + 1] - m0), kp, k, hsums.data() + out_off[s], weight ? weight + m0 : nullptr,
			              chol, yg, null_status, n_y, counts[s], wk, &rows[s], lam.data() + m0);
		}
	}
	std::copy(rows.begin(), rows.end(), out);
	if (lambda_out) {
		std::copy_n(lam.data(), n_memb, lambda_out);
	}
	return PGH_OK;
}

} // namespace

extern "C" double pgh_glm_p_from_t(double t, double df) {
	return pgh::GlmPFromT(t, df);
}

extern "C" double pgh_glm_p_from_z(double z) {
	return pgh::GlmPFromZ(z);
}

extern "C" int pgh_glm(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                       const double *phenotype, uint32_t n_covar, const double *covariates, int model, int firth,
                       pgh_glm_row *out, char *errbuf) {
	const int rc = GlmCheckArgs(ds, subset, v_begin, v_end, 1, phenotype, n_covar, covariates, model, out, errbuf);
	if (rc != PGH_OK || v_end == v_begin) {
		return rc;
	}
	if (ds->IsGroup()) {
		// every shard fills its own slice of out; nothing is exchanged
		return ForShardSlices(ds, subset, v_begin, v_end,
		                      [&](const pgh_dataset *s, const pgh_subset *part, uint32_t lo, uint32_t hi) {
			                      return GlmOne(s, part, lo, hi, phenotype, n_covar, covariates, model, firth,
			                                    out + (lo - v_begin), errbuf);
		                      });
	}
	return GlmOne(ds, subset, v_begin, v_end, phenotype, n_covar, covariates, model, firth, out, errbuf);
}

extern "C" int pgh_glm_multi(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                             uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                             int model, int firth, pgh_glm_row *out, char *errbuf) {
	const int rc = GlmCheckArgs(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, model, out, errbuf);
	if (rc != PGH_OK || v_end == v_begin) {
		return rc;
	}
	if (ds->IsGroup()) {
		// every shard fills its own slice of out, as in pgh_glm
		return ForShardSlices(ds, subset, v_begin, v_end,
		                      [&](const pgh_dataset *s, const pgh_subset *part, uint32_t lo, uint32_t hi) {
			                      return GlmMultiOne(s, part, lo, hi, n_pheno, phenotypes, n_covar, covariates, model, firth,
			                                         out + static_cast<size_t>(lo - v_begin) * n_pheno, errbuf);
		                      });
	}
	return GlmMultiOne(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, model, firth, out, errbuf);
}

extern "C" int pgh_glm_sparse(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                              const double *phenotype, uint32_t n_covar, const double *covariates, pgh_glm_row *out,
                              char *errbuf) {
	PGH_SPARSE_ROWS(ds);
	const int rc = GlmCheckCommon(ds, subset, v_begin, v_end, 1, phenotype, n_covar, covariates, PGH_GLM_LINEAR, out,
	                              errbuf);
	if (rc != PGH_OK || v_end == v_begin) {
		return rc;
	}
	return GlmSparseOne(ds, subset, v_begin, v_end, phenotype, n_covar, covariates, out, errbuf);
}

namespace {

// The score tests' phenotype: every value 0, 1 or NaN, with a case and a control.
int GlmCheckBinary(const double *phenotype, uint32_t n_out, char *errbuf) {
	uint32_t cases = 0, controls = 0;
	for (uint32_t i = 0; i < n_out; i++) {
		if (std::isnan(phenotype[i])) {
			continue;
		}
		if (phenotype[i] != 0.0 && phenotype[i] != 1.0) {
			SetErr(errbuf, "phenotype must be 0 or 1 (NaN = missing), got " + std::to_string(phenotype[i]) + " at sample " +
			                   std::to_string(i));
			return PGH_ERR_ARG;
		}
		(phenotype[i] != 0.0 ? cases : controls)++;
	}
	if (!cases || !controls) {
		SetErr(errbuf, "no cases or no controls among the samples with a phenotype");
		return PGH_ERR_ARG;
	}
	return PGH_OK;
}

// pgh_glm_score_sparse_spa's, pgh_glm_score_multi_spa's and pgh_glm_score_sparse_multi_spa's own arguments.
int GlmCheckSpa(double spa_cutoff, const double *p_spa, const uint8_t *spa_state, char *errbuf) {
	if (!(spa_cutoff >= 0.1)) { // (NaN too)
		SetErr(errbuf, "spa_cutoff must be at least 0.1");
		return PGH_ERR_ARG;
	}
	if (!p_spa || !spa_state) {
		SetErr(errbuf, "null p_spa or spa_state");
		return PGH_ERR_ARG;
	}
	return PGH_OK;
}

// pgh_glm_score_sparse_firth's, pgh_glm_score_multi_firth's and pgh_glm_score_sparse_multi_firth's own arguments.
int GlmCheckFirth(double firth_cutoff, const pgh_glm_firth_row *firth, char *errbuf) {
	if (!(firth_cutoff >= 0.1)) { // (NaN too)
		SetErr(errbuf, "firth_cutoff must be at least 0.1");
		return PGH_ERR_ARG;
	}
	if (!firth) {
		SetErr(errbuf, "null firth");
		return PGH_ERR_ARG;
	}
	return PGH_OK;
}

// The set arguments that pgh_burden_sparse and pgh_skat_sparse share (out: the caller's rows).
int GlmCheckSets(const pgh_dataset *ds, uint32_t n_sets, const uint64_t *set_off, const uint32_t *set_vidx,
                 const double *weight, const void *out, char *errbuf) {
	if (n_sets == 0) {
		SetErr(errbuf, "at least one set is needed");
		return PGH_ERR_ARG;
	}
	if (!set_off || !out) {
		SetErr(errbuf, "null argument");
		return PGH_ERR_ARG;
	}
	if (set_off[0] != 0) {
		SetErr(errbuf, "set_off[0] must be 0, got " + std::to_string(set_off[0]));
		return PGH_ERR_ARG;
	}
	for (uint32_t s = 0; s < n_sets; s++) {
		if (set_off[s + 1] < set_off[s]) {
			SetErr(errbuf, "set_off decreases at set " + std::to_string(s) + " (" + std::to_string(set_off[s]) + " -> " +
			                   std::to_string(set_off[s + 1]) + ")");
			return PGH_ERR_ARG;
		}
	}
	const uint64_t n_memb = set_off[n_sets];
	const uint32_t n_var = ds->v_end - ds->v_begin;
	if (n_memb && !set_vidx) {
		SetErr(errbuf, "null argument");
		return PGH_ERR_ARG;
	}
	for (uint64_t m = 0; m < n_memb; m++) {
		if (set_vidx[m] >= n_var) {
			SetErr(errbuf, "set_vidx[" + std::to_string(m) + "] = " + std::to_string(set_vidx[m]) +
			                   " is not below the dataset's variant count " + std::to_string(n_var));
			return PGH_ERR_ARG;
		}
	}
	for (uint64_t m = 0; weight && m < n_memb; m++) {
		if (!std::isfinite(weight[m])) {
			SetErr(errbuf, "weight " + std::to_string(m) + " is not finite");
			return PGH_ERR_ARG;
		}
	}
	return PGH_OK;
}

// pgh_glm_score_sparse, pgh_glm_score_sparse_spa and pgh_glm_score_sparse_firth after the latter two's own argument
// checks.
int GlmScoreSparseEntry(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                        const double *phenotype, uint32_t n_covar, const double *covariates, pgh_glm_row *out,
                        const GlmScoreFollowUp &fu, char *errbuf) {
	PGH_ONE_DEVICE(ds);
	PGH_SPARSE_ROWS(ds);
	PGH_TRY(GlmCheckCommon(ds, subset, v_begin, v_end, 1, phenotype, n_covar, covariates, PGH_GLM_LOGISTIC, out, errbuf));
	PGH_TRY(GlmCheckBinary(phenotype, subset ? subset->n_out : ds->sample_ct, errbuf));
	if (v_end == v_begin) {
		return PGH_OK;
	}
	return GlmScoreSparseOne(ds, subset, v_begin, v_end, phenotype, n_covar, covariates, out, errbuf, fu);
}

// pgh_glm_score_multi: the byte budget of the scratch that grows with the phenotype block and the variant chunk (read
// at every call; the result does not depend on it).  Three quarters of it at most go to the column block, which
// decides how many phenotypes share a walk of the matrix; the rest bounds the chunk.  The default holds the block of
// 64 phenotypes with 10 covariates over 500 k samples (3.3 GB).  A handful of sample-length vectors of the null fit
// are outside it, and below one phenotype and one variant nothing shrinks further.
constexpr uint64_t kGlmScoreScratchBytes = 6ull << 30;
const char *const kGlmScoreScratchEnv = "PGH_GLM_SCORE_SCRATCH_BYTES";
constexpr uint32_t kGlmScoreMultiChunk = 65536;

// The device arrays that scale with the chunk, per (block phenotype, chunk variant).  AddTo is their one declaration:
// the scratch layout binds it, and the plan charges a chunk variant what it declares for c = 1.
struct GlmScoreMultiChunkArrays {
	double *sums = nullptr, *hgn = nullptr;
	uint32_t *nmiss = nullptr;
	pgh_glm_row *rows = nullptr;
	pgh::GlmScoreSpaOut so;             // kSpa: [t, U, V], p_spa and the state
	pgh_glm_firth_row *firth = nullptr; // kFirth
	void AddTo(ScratchLayout &lay, uint64_t pb_max, uint64_t c, uint32_t kp, uint32_t k, GlmScoreFollowUp::Kind kind) {
		const uint64_t n = pb_max * c, ns = kp + 6, ne = (k + 1) * (k + 2) / 2 + k + 1;
		lay.Add(&sums, n * ns);
		lay.Add(&hgn, n * ne);
		lay.Add(&nmiss, n);
		lay.Add(&rows, n);
		lay.Add(&so.t, n * (kp + 3), kind == GlmScoreFollowUp::kSpa);
		lay.Add(&so.p_spa, n, kind == GlmScoreFollowUp::kSpa);
		lay.Add(&so.state, n, kind == GlmScoreFollowUp::kSpa);
		lay.Add(&firth, n, kind == GlmScoreFollowUp::kFirth);
	}
};

// How a call splits its budget.  The column block of pb_max phenotypes takes three quarters of it at most.  A
// follow-up's workgroups' stashes take up to three quarters of what the block leaves (StashGroupsFor: at least one
// stash, at most four workgroups per compute unit, since the time of the kernel's iteration falls with their number).
// What is left then bounds the chunk, at GlmScoreMultiChunkArrays' bytes per variant before ScratchLayout's rounding:
// the rounding and the block's own small arrays are not charged, so the scratch block can pass the budget by that much.
struct GlmScoreMultiPlan {
	uint32_t pb_max = 0;   // phenotypes of a column block
	uint32_t n_groups = 0; // workgroups of the follow-up kernel (0: there is none)
	uint32_t chunk = 0;    // variants of a chunk
	uint64_t stash_bytes = 0;
};
// extra_variant_bytes: what a chunk variant takes besides (pgh_glm_score_multi_dosage's expanded rows).
GlmScoreMultiPlan GlmScoreMultiPlanFor(uint32_t n_raw, uint32_t n_pheno, uint32_t k, uint32_t nv_all, uint64_t budget,
                                       int cus, GlmScoreFollowUp::Kind kind, uint64_t extra_variant_bytes = 0) {
	const uint32_t kp = pgh::GlmPadCovar(k);
	const uint64_t n_pad = 64ull * ((static_cast<uint64_t>(n_raw) + 63) / 64), mask_words = n_pad / 16;
	const auto block_bytes = [&](uint32_t pb) {
		return 8ull * n_pad * pgh::GlmScoreDenseLayout(pb, k).ld + 4ull * mask_words * pb;
	};
	GlmScoreMultiPlan plan;
	plan.pb_max = std::min(pgh::kGlmScoreDensePb, n_pheno);
	while (plan.pb_max > 1 && block_bytes(plan.pb_max) > budget / 4 * 3) {
		plan.pb_max--;
	}
	GlmScoreMultiChunkArrays unit;
	ScratchLayout one_variant;
	unit.AddTo(one_variant, plan.pb_max, 1, kp, k, kind);
	uint64_t left = budget > block_bytes(plan.pb_max) ? budget - block_bytes(plan.pb_max) : 0;
	const uint32_t nv_most = std::min(kGlmScoreMultiChunk, nv_all);
	if (kind != GlmScoreFollowUp::kNone) {
		const uint64_t per_group = pgh::GlmScoreSpaStashPerGroup(n_raw);
		plan.n_groups = StashGroupsFor(static_cast<uint64_t>(nv_most) * plan.pb_max, 4, per_group, left / 4 * 3, cus);
		plan.stash_bytes = per_group * plan.n_groups;
		left = left > plan.stash_bytes ? left - plan.stash_bytes : 0;
	}
	plan.chunk = static_cast<uint32_t>(
	    std::min<uint64_t>(nv_most, std::max<uint64_t>(1, left / (one_variant.payload + extra_variant_bytes))));
	return plan;
}

// The work lists of a chunk of pgh_glm_score_sparse_multi_spa and pgh_glm_score_sparse_multi_firth
// (glm_score_sparse_lists.hpp): the applied rows of the wave form and of the workgroup form, and the list kernels'
// counts per tile.  AddTo is their one declaration, as above.
struct GlmScoreSparseMultiLists {
	uint32_t *wave = nullptr, *group = nullptr, *tile_ct = nullptr;
	void AddTo(ScratchLayout &lay, uint64_t pb_max, uint64_t c, bool present) {
		lay.Add(&wave, pb_max * c, present);
		lay.Add(&group, pb_max * c, present);
		lay.Add(&tile_ct, pgh::GlmScoreSparseMultiTileWords(pb_max * c), present);
	}
};

// pgh_glm_score_sparse_multi*: how a call splits the same budget.  The pair block takes 16 n_raw bytes per phenotype; it
// gets the most phenotypes, kGlmScoreSparsePb at most, that leave one chunk variant's arrays (and, with a follow-up,
// one stash) within the budget (one phenotype whatever the budget).  A follow-up (kSpa, kFirth): the stashes of its
// workgroup form take up to a quarter of what the block leaves (StashGroupsFor: at least one stash, at most four
// workgroups per compute unit); a quarter and not GlmScoreMultiPlanFor's three, because only the rows of more than
// kGlmSparseLong entries and the dense-form rows use one, and the chunk, which every row needs, should not shrink for
// them.  What is left bounds the chunk at the bytes per variant of GlmScoreMultiChunkArrays and, with a follow-up, of
// the work lists.  The rounding and the block's own small arrays are not charged, as in GlmScoreMultiPlanFor.
// The split itself, shared with pgh_glm_sparse_multi: block_bytes(pb) the block of pb phenotypes, variant_bytes(pb) a
// chunk variant's arrays, per_group a follow-up's stash (0: there is no follow-up).
template <class BlockBytes, class VariantBytes>
GlmScoreMultiPlan GlmSparseBlockPlanFor(uint32_t pb_most, uint32_t n_pheno, uint32_t nv_all, uint64_t budget, int cus,
                                        uint64_t per_group, BlockBytes block_bytes, VariantBytes variant_bytes) {
	GlmScoreMultiPlan plan;
	plan.pb_max = std::min(pb_most, n_pheno);
	while (plan.pb_max > 1 && block_bytes(plan.pb_max) + variant_bytes(plan.pb_max) + per_group > budget) {
		plan.pb_max--;
	}
	uint64_t left = budget > block_bytes(plan.pb_max) ? budget - block_bytes(plan.pb_max) : 0;
	const uint32_t nv_most = std::min(kGlmScoreMultiChunk, nv_all);
	if (per_group) {
		plan.n_groups = StashGroupsFor(static_cast<uint64_t>(nv_most) * plan.pb_max, 4, per_group, left / 4, cus);
		plan.stash_bytes = per_group * plan.n_groups;
		left = left > plan.stash_bytes ? left - plan.stash_bytes : 0;
	}
	plan.chunk = static_cast<uint32_t>(std::min<uint64_t>(nv_most, std::max<uint64_t>(1, left / variant_bytes(plan.pb_max))));
	return plan;
}

GlmScoreMultiPlan GlmScoreSparseMultiPlanFor(uint32_t n_raw, uint32_t n_pheno, uint32_t k, uint32_t nv_all,
                                             uint64_t budget, int cus, GlmScoreFollowUp::Kind kind) {
	const uint32_t kp = pgh::GlmPadCovar(k);
	const bool follow = kind != GlmScoreFollowUp::kNone;
	const uint64_t per_group = follow ? pgh::GlmScoreSpaStashPerGroup(n_raw) : 0;
	const auto block_bytes = [&](uint32_t pb) { return 16ull * n_raw * pb; };
	const auto variant_bytes = [&](uint32_t pb) {
		GlmScoreMultiChunkArrays unit;
		GlmScoreSparseMultiLists lists;
		ScratchLayout one_variant;
		unit.AddTo(one_variant, pb, 1, kp, k, kind);
		lists.AddTo(one_variant, pb, 1, follow);
		return one_variant.payload;
	};
	return GlmSparseBlockPlanFor(pgh::kGlmScoreSparsePb, n_pheno, nv_all, budget, cus, per_group, block_bytes, variant_bytes);
}

// sg.hz (and hz_raw): the covariates as they are, into d_z0 and, in raw-sample order, into *d_zr0, which without a
// subset is d_z0 itself.  who: the entry point's name in the error texts.
int GlmUploadCovariates(const pgh_subset *subset, uint32_t kp, const GlmStaged &sg, double *d_z0, double **d_zr0,
                        hipStream_t st, const char *who, char *errbuf) {
	if (!subset) {
		*d_zr0 = d_z0;
	}
	if (kp) {
		PGH_HIP(hipMemcpyAsync(d_z0, sg.hz.data(), 8ull * sg.hz.size(), hipMemcpyHostToDevice, st),
		        (std::string(who) + " covariate upload").c_str());
	}
	if (sg.raw && kp) {
		PGH_HIP(hipMemcpyAsync(*d_zr0, sg.hz_raw.data(), 8ull * sg.hz_raw.size(), hipMemcpyHostToDevice, st),
		        (std::string(who) + " covariate upload (raw order)").c_str());
	}
	return PGH_OK;
}

// What one call of pgh_glm_score_multi* (a dense-resident dataset) and of pgh_glm_score_sparse_multi* (a sparse-resident
// one) share after the argument checks: the pattern order, the staging of a pattern group, the null fit of a block
// phenotype, the solve of a chunk's rows phenotype by phenotype and their scatter into the caller's rows.
// The null models are fitted phenotype by phenotype by GlmScoreNullFit, as GlmScoreSparseOne fits its one: on the
// covariates centred over the phenotype's missing-value pattern, which the phenotypes of a pattern share (GlmStage's
// sums and subtraction, the latter on the device).
struct GlmScoreBlockCall {
	const pgh_dataset *ds;
	const pgh_subset *subset;
	uint32_t v_begin, nv_all, n_pheno, k;
	const double *phenotypes, *covariates;
	GlmScoreFollowUp fu;
	char *errbuf;
	const char *who; // the entry point's name in the error texts
	bool want_mask;  // a group's S as the dense kernels' sample mask
	hipStream_t st = PghThreadStream();
	uint32_t n_out = subset ? subset->n_out : ds->sample_ct, n_raw = ds->sample_ct;
	uint32_t kp = pgh::GlmPadCovar(k), ns = kp + 6, ne = (k + 1) * (k + 2) / 2 + k + 1;
	uint64_t n_pad = 64ull * ((static_cast<uint64_t>(n_raw) + 63) / 64), mask_words = n_pad / 16;
	const uint32_t *d_sel = subset ? subset->d_sel : nullptr;
	GlmScoreMultiPlan plan;

	// the phenotypes in the order of their pattern groups, so that a pattern's covariates are centred once; per group,
	// staged when its first phenotype comes up: |S|, the covariates' means over S and S as the kernels' sample mask
	// (one bit per 2-bit code, raw-sample order)
	struct GroupStage {
		bool ready = false;
		uint32_t n_y = 0;
		std::vector<double> mz;
		std::vector<uint32_t> mask;
	};
	std::vector<uint32_t> order, group_of;
	std::vector<GroupStage> gs;
	uint32_t centred_for = UINT32_MAX; // the group d_z is centred for

	double *d_y, *d_z0, *d_z, *d_zr0, *d_r, *d_w, *d_part, *d_hg1, *d_hg, *d_mz;
	uint32_t *d_ny;
	GlmScoreMultiChunkArrays ch;
	// the current block's |S| and null-fit status per phenotype, the current chunk's rows
	std::vector<uint32_t> h_ny;
	std::vector<int> status;
	std::vector<pgh_glm_row> hrows;

	std::string What(const char *part) const {
		return std::string(who) + " " + part;
	}
	void PatternOrder();
	void AddShared(ScratchLayout &lay);
	int UploadCovariates(const GlmStaged &sg);
	GroupStage &StageGroup(uint32_t p);
	int FitPhenotype(uint32_t b0, uint32_t j);
	int SolveRows(uint32_t pb, uint32_t nv);
	template <class T>
	void Scatter(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, const std::vector<T> &from, T *to,
	             const uint32_t *pos = nullptr) const;
};

void GlmScoreBlockCall::PatternOrder() {
	const std::vector<std::vector<uint32_t>> groups = GlmPatternGroups(n_pheno, phenotypes, n_out);
	group_of.resize(n_pheno);
	for (uint32_t g = 0; g < groups.size(); g++) {
		for (uint32_t p : groups[g]) {
			order.push_back(p);
			group_of[p] = g;
		}
	}
	gs.resize(groups.size());
}

// The arrays of every route, after the plan is made; sizes the host buffers of a block and a chunk.
void GlmScoreBlockCall::AddShared(ScratchLayout &lay) {
	const uint64_t n = n_out, nr = n_raw, pbm = plan.pb_max;
	lay.Add(&d_y, n);
	lay.Add(&d_z0, n * kp + 1); // one element of slack, here and in d_z, d_zr0, d_mz
	lay.Add(&d_z, n * kp + 1);
	lay.Add(&d_zr0, nr * kp + 1, subset != nullptr);
	lay.Add(&d_r, nr);
	lay.Add(&d_w, nr);
	lay.Add(&d_part, static_cast<uint64_t>(pgh::kGlmScoreNullParts) * ne);
	lay.Add(&d_hg1, ne);
	lay.Add(&d_hg, pbm * ne);
	lay.Add(&d_mz, pbm * kp + 1);
	lay.Add(&d_ny, pbm);
	h_ny.resize(plan.pb_max);
	status.resize(plan.pb_max);
	hrows.resize(static_cast<size_t>(plan.chunk) * plan.pb_max);
}

int GlmScoreBlockCall::UploadCovariates(const GlmStaged &sg) {
	return GlmUploadCovariates(subset, kp, sg, d_z0, &d_zr0, st, who, errbuf);
}

GlmScoreBlockCall::GroupStage &GlmScoreBlockCall::StageGroup(uint32_t p) {
	const double *y = phenotypes + static_cast<size_t>(p) * n_out;
	GroupStage &gr = gs[group_of[p]];
	if (!gr.ready) {
		gr.ready = true;
		gr.mask.assign(want_mask ? mask_words : 0, 0u);
		for (uint32_t i = 0; i < n_out; i++) {
			if (!std::isnan(y[i])) {
				if (want_mask) {
					const uint32_t s = subset ? subset->sel[i] : i;
					gr.mask[s >> 4] |= 1u << (2u * (s & 15u));
				}
				gr.n_y++;
			}
		}
		gr.mz.assign(kp + 1, 0.0);
		for (uint32_t jz = 0; jz < k && gr.n_y; jz++) {
			const double *zc = covariates + static_cast<size_t>(jz) * n_out;
			double mz = 0.0;
			for (uint32_t i = 0; i < n_out; i++) {
				mz += std::isnan(y[i]) ? 0.0 : zc[i];
			}
			gr.mz[jz] = mz / gr.n_y;
		}
	}
	return gr;
}

// Block phenotype j, the phenotype order[b0 + j]: its group's stage, the means and the centring, and the null fit,
// which leaves r and w in d_r / d_w (raw-sample order, the subset's samples) and the packed sums in d_hg[j].
int GlmScoreBlockCall::FitPhenotype(uint32_t b0, uint32_t j) {
	const uint32_t p = order[b0 + j], g = group_of[p];
	const double *y = phenotypes + static_cast<size_t>(p) * n_out;
	const GroupStage &gr = StageGroup(p);
	h_ny[j] = gr.n_y;
	if (kp) {
		PGH_HIP(hipMemcpyAsync(d_mz + static_cast<uint64_t>(j) * kp, gr.mz.data(), 8ull * kp, hipMemcpyHostToDevice, st),
		        What("mean upload").c_str());
		if (centred_for != g) {
			PGH_HIP(pgh::LaunchGlmScoreDenseCentre(n_out, kp, d_z0, d_mz + static_cast<uint64_t>(j) * kp, d_z, st),
			        What("centring kernel").c_str());
			centred_for = g;
		}
	}
	PGH_HIP(hipMemcpyAsync(d_y, y, 8ull * n_out, hipMemcpyHostToDevice, st), What("phenotype upload").c_str());
	PGH_TRY(GlmScoreNullFit(n_out, d_y, d_z, kp, k, d_sel, gr.n_y >= k + 3, d_r, d_w, d_part, d_hg1, st, &status[j], errbuf));
	PGH_HIP(hipMemcpyAsync(d_hg + static_cast<uint64_t>(j) * ne, d_hg1, 8ull * ne, hipMemcpyDeviceToDevice, st),
	        What("null model copy").c_str());
	return PGH_OK;
}

// The rows of the chunk's nv variants from ch.sums and ch.hgn, phenotype by phenotype, and their copy to hrows.
int GlmScoreBlockCall::SolveRows(uint32_t pb, uint32_t nv) {
	for (uint32_t j = 0; j < pb; j++) {
		const uint64_t at = static_cast<uint64_t>(j) * nv;
		pgh::GlmScoreSpaOut soj;
		if (fu.kind == GlmScoreFollowUp::kSpa) {
			soj.t = ch.so.t + at * (kp + 3);
			soj.p_spa = ch.so.p_spa + at;
			soj.state = ch.so.state + at;
		}
		PGH_HIP(pgh::LaunchGlmScoreSolve(nv, ch.sums + at * ns, kp, k, ch.hgn + at * ne, status[j], ch.rows + at, st, soj),
		        What("solve kernel").c_str());
	}
	PGH_HIP(hipMemcpyAsync(hrows.data(), ch.rows, sizeof(pgh_glm_row) * nv * pb, hipMemcpyDeviceToHost, st),
	        What("rows copy").c_str());
	return PGH_OK;
}

// from[block phenotype j][chunk variant i] into the caller's [variant][phenotype], the phenotypes in the caller's order.
// pos (may be null): row i belongs to variant c0 + pos[i] of the range instead of c0 + i.
template <class T>
void GlmScoreBlockCall::Scatter(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, const std::vector<T> &from, T *to,
                                const uint32_t *pos) const {
	for (uint32_t i = 0; i < nv; i++) {
		for (uint32_t j = 0; j < pb; j++) {
			to[static_cast<size_t>(c0 + (pos ? pos[i] : i)) * n_pheno + order[b0 + j]] = from[static_cast<size_t>(j) * nv + i];
		}
	}
}

// One call of pgh_glm_score_multi* on one dense-resident dataset.  Each fit's r and w go straight into the phenotype's
// columns of the block (glm_score_dense.hip).
// tracks (pgh_glm_score_multi_dosage over a dataset that holds dosage tracks): a chunk's variants without a track go
// through the same kernels, from the first such variant to the last; the ones with a track are listed, expanded into
// d_u16 / d_eff and contracted by glm_score_dense_dosage.hip, and their rows replace what the first pass left for them.
// With the saddlepoint follow-up (pgh_glm_score_multi_dosage_spa) the first pass may leave a triple for a track variant
// from its calls; the track pass (glm_score_dense_dosage_spa.hip over d_u16) overwrites it.  The same holds for the
// Firth follow-up (pgh_glm_score_multi_dosage_firth) and its pgh_glm_firth_row: the track pass
// (glm_score_dense_dosage_firth.hip over d_u16) writes every listed row.
struct GlmScoreMultiCall : GlmScoreBlockCall {
	double *d_b;
	uint32_t *d_mask;
	uint8_t *d_stash;
	bool tracks = false;
	uint16_t *d_u16;
	uint8_t *d_eff;
	uint32_t *d_tlist;
	std::vector<uint32_t> tlist, tpos; // the chunk's variants with a track: resident rows, places in the chunk
	std::vector<double> hp_spa;
	std::vector<uint8_t> hstate;
	std::vector<pgh_glm_firth_row> hfirth;

	int Prepare();
	int StageBlock(uint32_t b0, uint32_t pb);
	int RunChunk(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, pgh_glm_row *out);
	int RunHard(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, pgh_glm_row *out);
	int RunTracks(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nt, pgh_glm_row *out);
};

// The pattern order, the plan, the scratch block and the host buffers.
int GlmScoreMultiCall::Prepare() {
	PatternOrder();
	int cus = 0;
	if (fu.kind != GlmScoreFollowUp::kNone) {
		PGH_TRY(DeviceCus(&cus, "glm_score_multi stash", errbuf));
	}
	// every chunk variant is charged its expanded rows and its list entry, as if each had a track
	const uint64_t row_bytes = tracks ? pgh::GlmScoreDosageRowBytes(n_raw) : 0;
	plan = GlmScoreMultiPlanFor(n_raw, n_pheno, k, nv_all, EnvBytes(kGlmScoreScratchEnv, kGlmScoreScratchBytes), cus, fu.kind,
	                            tracks ? row_bytes + 4 : 0);

	ScratchLayout lay;
	AddShared(lay);
	lay.Add(&d_mask, plan.pb_max * mask_words);
	lay.Add(&d_b, n_pad * pgh::GlmScoreDenseLayout(plan.pb_max, k).ld);
	ch.AddTo(lay, plan.pb_max, plan.chunk, kp, k, fu.kind);
	lay.Add(&d_u16, n_pad * plan.chunk, tracks);
	lay.Add(&d_eff, n_pad / 4 * plan.chunk, tracks);
	lay.Add(&d_tlist, plan.chunk, tracks);
	tlist.resize(tracks ? plan.chunk : 0);
	tpos.resize(tracks ? plan.chunk : 0);
	lay.Add(&d_stash, plan.stash_bytes, fu.kind != GlmScoreFollowUp::kNone);
	void *scratch = nullptr;
	PGH_HIP(PghThreadScratch(lay.total, st, &scratch), "glm_score_multi scratch");
	lay.Bind(scratch);

	hp_spa.resize(fu.kind == GlmScoreFollowUp::kSpa ? hrows.size() : 0);
	hstate.resize(fu.kind == GlmScoreFollowUp::kSpa ? hrows.size() : 0);
	hfirth.resize(fu.kind == GlmScoreFollowUp::kFirth ? hrows.size() : 0);
	return PGH_OK;
}

// The block of the phenotypes order[b0 .. b0 + pb): per phenotype its null fit, its group's mask and the columns.
int GlmScoreMultiCall::StageBlock(uint32_t b0, uint32_t pb) {
	const uint32_t ld = pgh::GlmScoreDenseLayout(pb, k).ld;
	PGH_HIP(hipMemsetAsync(d_b, 0, 8ull * n_pad * ld, st), "glm_score_multi column block clear");
	for (uint32_t j = 0; j < pb; j++) {
		PGH_TRY(FitPhenotype(b0, j));
		PGH_HIP(hipMemcpyAsync(d_mask + j * mask_words, StageGroup(order[b0 + j]).mask.data(), 4ull * mask_words,
		                       hipMemcpyHostToDevice, st),
		        "glm_score_multi mask upload");
		PGH_HIP(pgh::LaunchGlmScoreDenseColumns(n_out, d_sel, d_r, d_w, d_z, kp, k, pb, j, d_b, st),
		        "glm_score_multi column kernel");
	}
	PGH_HIP(hipMemcpyAsync(d_ny, h_ny.data(), 4ull * pb, hipMemcpyHostToDevice, st), "glm_score_multi count upload");
	return PGH_OK;
}

// The variants c0 .. c0 + nv - 1 of the range against the staged block.
int GlmScoreMultiCall::RunChunk(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, pgh_glm_row *out) {
	if (!tracks) {
		return RunHard(b0, pb, c0, nv, out);
	}
	const uint32_t l0 = v_begin + c0 - ds->v_begin;
	uint32_t nt = 0, hard_lo = nv, hard_hi = 0;
	for (uint32_t i = 0; i < nv; i++) {
		if (ds->dos_row_of[l0 + i] >= 0) {
			tlist[nt] = l0 + i;
			tpos[nt++] = i;
		} else {
			hard_lo = std::min(hard_lo, i);
			hard_hi = i + 1;
		}
	}
	if (hard_hi > hard_lo) {
		PGH_TRY(RunHard(b0, pb, c0 + hard_lo, hard_hi - hard_lo, out));
	}
	return nt ? RunTracks(b0, pb, c0, nt, out) : PGH_OK;
}

// The chunk's nt listed variants, all with a track: the launches, the copy, and the scatter to their places.
int GlmScoreMultiCall::RunTracks(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nt, pgh_glm_row *out) {
	PGH_HIP(hipMemcpyAsync(d_tlist, tlist.data(), 4ull * nt, hipMemcpyHostToDevice, st), "glm_score_multi_dosage list upload");
	PGH_HIP(pgh::LaunchGlmScoreDenseDosage(ds->View(), ds->Dosage(), d_tlist, nt, d_mask, d_ny, pb, d_b, d_zr0, d_mz, kp, k,
	                                       d_hg, d_u16, d_eff, ch.sums, ch.nmiss, ch.hgn, st),
	        "glm_score_multi_dosage kernels");
	PGH_TRY(SolveRows(pb, nt));
	if (fu.kind == GlmScoreFollowUp::kSpa) {
		// over the u16 rows and the sums the launches above have just left: nothing is expanded twice
		const size_t n_rows = static_cast<size_t>(nt) * pb;
		PGH_HIP(pgh::LaunchGlmScoreDenseDosageSpa(ds->View(), d_u16, nt, d_mask, pb, d_b, d_zr0, d_mz, kp, k, ch.sums, ch.rows,
		                                          ch.so.t, fu.cutoff, plan.n_groups, d_stash, ch.so.p_spa, ch.so.state, st),
		        "glm_score_multi_dosage_spa kernel");
		PGH_HIP(hipMemcpyAsync(hp_spa.data(), ch.so.p_spa, 8ull * n_rows, hipMemcpyDeviceToHost, st),
		        "glm_score_multi_dosage_spa p copy");
		PGH_HIP(hipMemcpyAsync(hstate.data(), ch.so.state, n_rows, hipMemcpyDeviceToHost, st),
		        "glm_score_multi_dosage_spa state copy");
	} else if (fu.kind == GlmScoreFollowUp::kFirth) {
		PGH_HIP(pgh::LaunchGlmScoreDenseDosageFirth(ds->View(), d_u16, nt, d_mask, pb, d_b, k, ch.rows, fu.cutoff,
		                                            plan.n_groups, d_stash, ch.firth, st),
		        "glm_score_multi_dosage_firth kernel");
		PGH_HIP(hipMemcpyAsync(hfirth.data(), ch.firth, sizeof(pgh_glm_firth_row) * nt * pb, hipMemcpyDeviceToHost, st),
		        "glm_score_multi_dosage_firth rows copy");
	}
	PGH_HIP(hipStreamSynchronize(st), "glm_score_multi_dosage sync");
	Scatter(b0, pb, c0, nt, hrows, out, tpos.data());
	if (fu.kind == GlmScoreFollowUp::kSpa) {
		Scatter(b0, pb, c0, nt, hp_spa, fu.p_spa, tpos.data());
		Scatter(b0, pb, c0, nt, hstate, fu.state, tpos.data());
	} else if (fu.kind == GlmScoreFollowUp::kFirth) {
		Scatter(b0, pb, c0, nt, hfirth, fu.firth, tpos.data());
	}
	return PGH_OK;
}

// nv variants from c0 of the range by their calls: the launches, the copies, and the scatter into the caller's arrays.
int GlmScoreMultiCall::RunHard(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, pgh_glm_row *out) {
	const uint32_t l0 = v_begin + c0 - ds->v_begin;
	const size_t n_rows = static_cast<size_t>(nv) * pb;
	PGH_HIP(pgh::LaunchGlmScoreDense(ds->View(), l0, nv, d_mask, d_ny, pb, d_b, d_zr0, d_mz, kp, k, d_hg, ch.sums, ch.nmiss,
	                                 ch.hgn, st),
	        "glm_score_multi kernels");
	PGH_TRY(SolveRows(pb, nv));
	if (fu.kind == GlmScoreFollowUp::kSpa) {
		PGH_HIP(pgh::LaunchGlmScoreDenseSpa(ds->View(), l0, nv, d_mask, pb, d_b, d_zr0, d_mz, kp, k, ch.sums, ch.rows, ch.so.t,
		                                    fu.cutoff, plan.n_groups, d_stash, ch.so.p_spa, ch.so.state, st),
		        "glm_score_multi_spa kernel");
		PGH_HIP(hipMemcpyAsync(hp_spa.data(), ch.so.p_spa, 8ull * n_rows, hipMemcpyDeviceToHost, st),
		        "glm_score_multi_spa p copy");
		PGH_HIP(hipMemcpyAsync(hstate.data(), ch.so.state, n_rows, hipMemcpyDeviceToHost, st),
		        "glm_score_multi_spa state copy");
	} else if (fu.kind == GlmScoreFollowUp::kFirth) {
		PGH_HIP(pgh::LaunchGlmScoreDenseFirth(ds->View(), l0, nv, d_mask, pb, d_b, k, ch.rows, fu.cutoff, plan.n_groups,
		                                      d_stash, ch.firth, st),
		        "glm_score_multi_firth kernel");
		PGH_HIP(hipMemcpyAsync(hfirth.data(), ch.firth, sizeof(pgh_glm_firth_row) * n_rows, hipMemcpyDeviceToHost, st),
		        "glm_score_multi_firth rows copy");
	}
	PGH_HIP(hipStreamSynchronize(st), "glm_score_multi sync");
	Scatter(b0, pb, c0, nv, hrows, out);
	if (fu.kind == GlmScoreFollowUp::kSpa) {
		Scatter(b0, pb, c0, nv, hp_spa, fu.p_spa);
		Scatter(b0, pb, c0, nv, hstate, fu.state);
	} else if (fu.kind == GlmScoreFollowUp::kFirth) {
		Scatter(b0, pb, c0, nv, hfirth, fu.firth);
	}
	return PGH_OK;
}

// One call of pgh_glm_score_sparse_multi* on one sparse-resident dataset.  Each fit's r and w go into the phenotype's
// column of the pair block (glm_score_sparse_multi.hip); the entry kernel centres the raw-order covariates per lane on
// the block's means d_mz.  With a follow-up, after a chunk's rows the applied ones are listed, and
// GlmScoreSparseMultiSpaKernel (kSpa, glm_score_sparse_multi_spa.hip) replaces their p_spa, or
// GlmScoreSparseMultiFirthKernel (kFirth, glm_score_sparse_multi_firth.hip) their pgh_glm_firth_row.
struct GlmScoreSparseMultiCall : GlmScoreBlockCall {
	double *d_pair;
	uint8_t *d_stash;
	GlmScoreSparseMultiLists lists;
	uint32_t wave_groups = 0; // workgroups of the wave form's grid
	std::vector<double> hp_spa;
	std::vector<uint8_t> hstate;
	std::vector<pgh_glm_firth_row> hfirth;

	int Prepare();
	int StageBlock(uint32_t b0, uint32_t pb);
	int RunChunk(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, pgh_glm_row *out);
};

int GlmScoreSparseMultiCall::Prepare() {
	PatternOrder();
	const bool spa = fu.kind == GlmScoreFollowUp::kSpa, follow = fu.kind != GlmScoreFollowUp::kNone;
	int cus = 0;
	if (follow) {
		PGH_TRY(DeviceCus(&cus, "glm_score_sparse_multi stash", errbuf));
		// the wave form keeps two workgroups on a compute unit (their stashes are LDS): a few rounds of them, so that the
		// rows' unequal lengths even out
		wave_groups = 8u * static_cast<uint32_t>(std::max(cus, 1));
	}
	plan = GlmScoreSparseMultiPlanFor(n_raw, n_pheno, k, nv_all, EnvBytes(kGlmScoreScratchEnv, kGlmScoreScratchBytes), cus,
	                                  fu.kind);
	ScratchLayout lay;
	AddShared(lay);
	lay.Add(&d_pair, 2ull * n_raw * plan.pb_max);
	ch.AddTo(lay, plan.pb_max, plan.chunk, kp, k, fu.kind);
	lists.AddTo(lay, plan.pb_max, plan.chunk, follow);
	lay.Add(&d_stash, plan.stash_bytes, follow);
	void *scratch = nullptr;
	PGH_HIP(PghThreadScratch(lay.total, st, &scratch), "glm_score_sparse_multi scratch");
	lay.Bind(scratch);
	hp_spa.resize(spa ? hrows.size() : 0);
	hstate.resize(spa ? hrows.size() : 0);
	hfirth.resize(fu.kind == GlmScoreFollowUp::kFirth ? hrows.size() : 0);
	return PGH_OK;
}

// The block of the phenotypes order[b0 .. b0 + pb): the pair block cleared, then per phenotype its null fit and its
// pairs.  With a subset the fit writes the subset's samples only, and only those are scattered.
int GlmScoreSparseMultiCall::StageBlock(uint32_t b0, uint32_t pb) {
	PGH_HIP(pgh::LaunchGlmScoreSparsePairClear(n_raw, pb, d_pair, st), "glm_score_sparse_multi pair block clear");
	for (uint32_t j = 0; j < pb; j++) {
		PGH_TRY(FitPhenotype(b0, j));
		PGH_HIP(pgh::LaunchGlmScoreSparsePairs(n_out, d_sel, d_r, d_w, pb, j, d_pair, st), "glm_score_sparse_multi pair kernel");
	}
	PGH_HIP(hipMemcpyAsync(d_ny, h_ny.data(), 4ull * pb, hipMemcpyHostToDevice, st), "glm_score_sparse_multi count upload");
	return PGH_OK;
}

int GlmScoreSparseMultiCall::RunChunk(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, pgh_glm_row *out) {
	const uint32_t l0 = v_begin + c0 - ds->v_begin;
	PGH_HIP(pgh::LaunchGlmScoreSparseMulti(ds->Sparse(), l0, nv, d_pair, d_ny, pb, d_zr0, d_mz, kp, k, d_hg, ch.sums, ch.nmiss,
	                                       ch.hgn, st),
	        "glm_score_sparse_multi kernels");
	PGH_TRY(SolveRows(pb, nv));
	const size_t n_rows = static_cast<size_t>(nv) * pb;
	if (fu.kind == GlmScoreFollowUp::kSpa) {
		PGH_HIP(pgh::LaunchGlmScoreSparseMultiSpa(ds->Sparse(), l0, nv, d_pair, pb, d_zr0, d_mz, kp, ch.rows, ch.so.t, fu.cutoff,
		                                          lists.wave, lists.group, lists.tile_ct, wave_groups, plan.n_groups, d_stash,
		                                          ch.so.p_spa, ch.so.state, st),
		        "glm_score_sparse_multi_spa kernels");
		PGH_HIP(hipMemcpyAsync(hp_spa.data(), ch.so.p_spa, 8ull * n_rows, hipMemcpyDeviceToHost, st),
		        "glm_score_sparse_multi_spa p copy");
		PGH_HIP(hipMemcpyAsync(hstate.data(), ch.so.state, n_rows, hipMemcpyDeviceToHost, st),
		        "glm_score_sparse_multi_spa state copy");
	} else if (fu.kind == GlmScoreFollowUp::kFirth) {
		PGH_HIP(pgh::LaunchGlmScoreSparseMultiFirth(ds->Sparse(), l0, nv, d_pair, pb, ch.rows, fu.cutoff, lists.wave, lists.group,
		                                            lists.tile_ct, wave_groups, plan.n_groups, d_stash, ch.firth, st),
		        "glm_score_sparse_multi_firth kernels");
		PGH_HIP(hipMemcpyAsync(hfirth.data(), ch.firth, sizeof(pgh_glm_firth_row) * n_rows, hipMemcpyDeviceToHost, st),
		        "glm_score_sparse_multi_firth rows copy");
	}
	PGH_HIP(hipStreamSynchronize(st), "glm_score_sparse_multi sync");
	Scatter(b0, pb, c0, nv, hrows, out);
	if (fu.kind == GlmScoreFollowUp::kSpa) {
		Scatter(b0, pb, c0, nv, hp_spa, fu.p_spa);
		Scatter(b0, pb, c0, nv, hstate, fu.state);
	} else if (fu.kind == GlmScoreFollowUp::kFirth) {
		Scatter(b0, pb, c0, nv, hfirth, fu.firth);
	}
	return PGH_OK;
}

// The block loop over the chunk loop of either route.
template <class Call>
int GlmScoreBlocksRun(Call &c, pgh_glm_row *out) {
	// sg.hz (and hz_raw): the covariates as they are
	const GlmStaged sg = GlmStage(c.ds, c.subset, c.phenotypes, c.k, c.covariates, GlmCentre::kNone, true);
	HostSourceFence fence(c.st); // sg, c's vectors and the caller's phenotypes feed asynchronous uploads
	PGH_TRY(c.Prepare());
	PGH_TRY(c.UploadCovariates(sg));
	for (uint32_t b0 = 0; b0 < c.n_pheno; b0 += c.plan.pb_max) {
		const uint32_t pb = std::min(c.plan.pb_max, c.n_pheno - b0);
		PGH_TRY(c.StageBlock(b0, pb));
		for (uint32_t c0 = 0; c0 < c.nv_all; c0 += c.plan.chunk) {
			PGH_TRY(c.RunChunk(b0, pb, c0, std::min(c.plan.chunk, c.nv_all - c0), out));
		}
	}
	return PGH_OK;
}

// The device arrays of pgh_glm_sparse_multi that scale with the chunk, per (chunk variant, block phenotype).  AddTo is
// their one declaration, as GlmScoreMultiChunkArrays' is.
struct GlmSparseMultiChunkArrays {
	double *sums = nullptr, *corr = nullptr;
	uint32_t *nlist = nullptr;
	pgh_glm_row *rows = nullptr;
	void AddTo(ScratchLayout &lay, uint64_t pb_max, uint64_t c, uint32_t kp, uint32_t k) {
		const uint64_t n = pb_max * c, q = k + 2;
		lay.Add(&sums, n * (kp + 4));
		lay.Add(&corr, n * (q * (q + 1) / 2));
		lay.Add(&nlist, c);
		lay.Add(&rows, n);
	}
};

// One call of pgh_glm_sparse_multi on one sparse-resident dataset (glm_sparse_multi.hip), run by GlmScoreBlocksRun.  The
// phenotypes are taken in the caller's order, blocks of consecutive ones: a block's values are uploaded as they are and
// written into the value block centred on each phenotype's own mean; the covariates stay as they are on the device and
// the kernels centre them per phenotype on d_mz, the means over the phenotype's own samples (GlmStage's sums, so the
// numbers are pgh_glm_sparse's).  A chunk's rows come back variant-major and go into `out` with one strided copy.
struct GlmSparseMultiCall {
	const pgh_dataset *ds;
	const pgh_subset *subset;
	uint32_t v_begin, nv_all, n_pheno, k;
	const double *phenotypes, *covariates;
	char *errbuf;
	hipStream_t st = PghThreadStream();
	uint32_t n_out = subset ? subset->n_out : ds->sample_ct, n_raw = ds->sample_ct;
	uint32_t kp = pgh::GlmPadCovar(k), ne = (k + 2) * (k + 3) / 2;
	const uint32_t *d_sel = subset ? subset->d_sel : nullptr;
	GlmScoreMultiPlan plan;
	const GlmStaged *staged = nullptr; // the covariates, sample-major (UploadCovariates)

	double *d_z0, *d_zr0, *d_yb, *d_yv, *d_my, *d_mz, *d_part, *d_gram;
	uint32_t *d_ny;
	GlmSparseMultiChunkArrays ch;
	std::vector<double> h_my, h_mz;
	std::vector<uint32_t> h_ny;

	int Prepare();
	int UploadCovariates(const GlmStaged &sg);
	int StageBlock(uint32_t b0, uint32_t pb);
	int RunChunk(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, pgh_glm_row *out);
};

// The plan (the value block and the uploaded phenotypes take 8 (n_raw + n_out) bytes per phenotype), the scratch block
// and the host buffers.
int GlmSparseMultiCall::Prepare() {
	const auto block_bytes = [&](uint32_t pb) { return 8ull * (static_cast<uint64_t>(n_raw) + n_out) * pb; };
	const auto variant_bytes = [&](uint32_t pb) {
		GlmSparseMultiChunkArrays unit;
		ScratchLayout one_variant;
		unit.AddTo(one_variant, pb, 1, kp, k);
		return one_variant.payload;
	};
	plan = GlmSparseBlockPlanFor(pgh::kGlmSparseMultiPb, n_pheno, nv_all, EnvBytes(kGlmScoreScratchEnv, kGlmScoreScratchBytes),
	                             0, 0, block_bytes, variant_bytes);
	const uint64_t n = n_out, nr = n_raw, pbm = plan.pb_max;
	ScratchLayout lay;
	lay.Add(&d_z0, n * kp + 1); // one element of slack, here and in d_zr0, d_mz
	lay.Add(&d_zr0, nr * kp + 1, subset != nullptr);
	lay.Add(&d_yb, n * pbm);
	lay.Add(&d_yv, nr * pbm);
	lay.Add(&d_my, pbm);
	lay.Add(&d_mz, pbm * kp + 1);
	lay.Add(&d_part, pbm * pgh::kGlmSparseMultiParts * ne);
	lay.Add(&d_gram, pbm * ne);
	lay.Add(&d_ny, pbm);
	ch.AddTo(lay, plan.pb_max, plan.chunk, kp, k);
	void *scratch = nullptr;
	PGH_HIP(PghThreadScratch(lay.total, st, &scratch), "glm_sparse_multi scratch");
	lay.Bind(scratch);
	h_my.resize(plan.pb_max);
	h_mz.resize(static_cast<size_t>(plan.pb_max) * kp + 1);
	h_ny.resize(plan.pb_max);
	return PGH_OK;
}

int GlmSparseMultiCall::UploadCovariates(const GlmStaged &sg) {
	staged = &sg;
	return GlmUploadCovariates(subset, kp, sg, d_z0, &d_zr0, st, "glm_sparse_multi", errbuf);
}

// The block of the phenotypes b0 .. b0 + pb: per phenotype |S|, its mean and the covariates' means over S, each summed
// in sample order as GlmStage sums them; then the value block and the whole-call Grams.  Every upload of the previous
// block has completed: each chunk ends with a stream synchronisation.
int GlmSparseMultiCall::StageBlock(uint32_t b0, uint32_t pb) {
	const double *yb = phenotypes + static_cast<size_t>(b0) * n_out;
	const double *hz = staged->hz.data();
	for (uint32_t j = 0; j < pb; j++) {
		const double *y = yb + static_cast<size_t>(j) * n_out;
		uint32_t n_y = 0;
		for (uint32_t i = 0; i < n_out; i++) {
			n_y += std::isnan(y[i]) ? 0u : 1u;
		}
		h_ny[j] = n_y;
		h_my[j] = n_y ? GlmMean(y, n_out, n_y) : 0.0;
		double *mz = h_mz.data() + static_cast<size_t>(j) * kp;
		std::fill_n(mz, kp, 0.0);
		if (n_y) {
			for (uint32_t i = 0; i < n_out; i++) {
				if (!std::isnan(y[i])) {
					for (uint32_t t = 0; t < k; t++) {
						mz[t] += hz[static_cast<size_t>(i) * kp + t];
					}
				}
			}
			for (uint32_t t = 0; t < k; t++) {
				mz[t] /= n_y;
			}
		}
	}
	PGH_HIP(hipMemcpyAsync(d_yb, yb, 8ull * n_out * pb, hipMemcpyHostToDevice, st), "glm_sparse_multi phenotype upload");
	PGH_HIP(hipMemcpyAsync(d_my, h_my.data(), 8ull * pb, hipMemcpyHostToDevice, st), "glm_sparse_multi mean upload");
	if (kp) {
		PGH_HIP(hipMemcpyAsync(d_mz, h_mz.data(), 8ull * pb * kp, hipMemcpyHostToDevice, st),
		        "glm_sparse_multi covariate mean upload");
	}
	PGH_HIP(hipMemcpyAsync(d_ny, h_ny.data(), 4ull * pb, hipMemcpyHostToDevice, st), "glm_sparse_multi count upload");
	PGH_HIP(pgh::LaunchGlmSparseMultiValues(n_raw, n_out, d_sel, d_yb, d_my, pb, d_yv, st), "glm_sparse_multi value kernels");
	PGH_HIP(pgh::LaunchGlmSparseMultiGram(n_raw, d_yv, pb, d_zr0, d_mz, kp, k, d_part, d_gram, st),
	        "glm_sparse_multi gram kernels");
	return PGH_OK;
}

// The variants c0 .. c0 + nv - 1 of the range against the staged block; the rows [nv][pb] go into out[.][b0 .. b0 + pb).
int GlmSparseMultiCall::RunChunk(uint32_t b0, uint32_t pb, uint32_t c0, uint32_t nv, pgh_glm_row *out) {
	const uint32_t l0 = v_begin + c0 - ds->v_begin;
	PGH_HIP(pgh::LaunchGlmSparseMulti(ds->Sparse(), l0, nv, d_yv, d_ny, pb, d_zr0, d_mz, kp, k, d_gram, ch.sums, ch.nlist,
	                                  ch.corr, ch.rows, st),
	        "glm_sparse_multi kernels");
	PGH_HIP(hipMemcpy2DAsync(out + static_cast<size_t>(c0) * n_pheno + b0, sizeof(pgh_glm_row) * n_pheno, ch.rows,
	                         sizeof(pgh_glm_row) * pb, sizeof(pgh_glm_row) * pb, nv, hipMemcpyDeviceToHost, st),
	        "glm_sparse_multi rows copy");
	PGH_HIP(hipStreamSynchronize(st), "glm_sparse_multi sync");
	return PGH_OK;
}

int GlmScoreMultiOne(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end, uint32_t n_pheno,
                     const double *phenotypes, uint32_t k, const double *covariates, pgh_glm_row *out, char *errbuf,
                     const GlmScoreFollowUp &fu) {
	PGH_ENTER(ds);
	GlmScoreMultiCall c {{ds, subset, v_begin, v_end - v_begin, n_pheno, k, phenotypes, covariates, fu, errbuf,
	                      "glm_score_multi", true}};
	c.tracks = ds->dos_rows != 0; // the pgh_glm_score_multi_dosage* entries alone let such a dataset through
	return GlmScoreBlocksRun(c, out);
}

int GlmScoreSparseMultiOne(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                           uint32_t n_pheno, const double *phenotypes, uint32_t k, const double *covariates,
                           pgh_glm_row *out, char *errbuf, const GlmScoreFollowUp &fu) {
	PGH_ENTER(ds);
	GlmScoreSparseMultiCall c {{ds, subset, v_begin, v_end - v_begin, n_pheno, k, phenotypes, covariates, fu, errbuf,
	                            "glm_score_sparse_multi", false}};
	return GlmScoreBlocksRun(c, out);
}

int GlmSparseMultiOne(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end, uint32_t n_pheno,
                      const double *phenotypes, uint32_t k, const double *covariates, pgh_glm_row *out, char *errbuf) {
	PGH_ENTER(ds);
	GlmSparseMultiCall c {ds, subset, v_begin, v_end - v_begin, n_pheno, k, phenotypes, covariates, errbuf};
	return GlmScoreBlocksRun(c, out);
}

} // namespace

extern "C" int pgh_glm_score_sparse(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                                    const double *phenotype, uint32_t n_covar, const double *covariates,
                                    pgh_glm_row *out, char *errbuf) {
	return GlmScoreSparseEntry(ds, subset, v_begin, v_end, phenotype, n_covar, covariates, out, {}, errbuf);
}

extern "C" int pgh_glm_score_sparse_spa(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                        uint32_t v_end, const double *phenotype, uint32_t n_covar,
                                        const double *covariates, double spa_cutoff, pgh_glm_row *out, double *p_spa,
                                        uint8_t *spa_state, char *errbuf) {
	PGH_TRY(GlmCheckSpa(spa_cutoff, p_spa, spa_state, errbuf));
	const GlmScoreFollowUp fu = {GlmScoreFollowUp::kSpa, spa_cutoff, p_spa, spa_state, nullptr};
	return GlmScoreSparseEntry(ds, subset, v_begin, v_end, phenotype, n_covar, covariates, out, fu, errbuf);
}

extern "C" int pgh_glm_score_sparse_firth(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                          uint32_t v_end, const double *phenotype, uint32_t n_covar,
                                          const double *covariates, double firth_cutoff, pgh_glm_row *out,
                                          pgh_glm_firth_row *firth, char *errbuf) {
	PGH_TRY(GlmCheckFirth(firth_cutoff, firth, errbuf));
	const GlmScoreFollowUp fu = {GlmScoreFollowUp::kFirth, firth_cutoff, nullptr, nullptr, firth};
	return GlmScoreSparseEntry(ds, subset, v_begin, v_end, phenotype, n_covar, covariates, out, fu, errbuf);
}

extern "C" int pgh_glm_sparse_multi(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                                    uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                                    pgh_glm_row *out, char *errbuf) {
	PGH_ONE_DEVICE(ds);
	PGH_SPARSE_ROWS(ds);
	PGH_TRY(GlmCheckCommon(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, PGH_GLM_LINEAR, out, errbuf));
	if (v_end == v_begin) {
		return PGH_OK;
	}
	return GlmSparseMultiOne(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, errbuf);
}

namespace {

// The phenotype checks of the block routes: every phenotype binary with a case and a control, the failing one named.
int GlmCheckBinaryEach(const double *phenotypes, uint32_t n_pheno, uint32_t n_out, char *errbuf) {
	for (uint32_t p = 0; p < n_pheno; p++) {
		char why[PGH_ERRBUF_LEN];
		why[0] = '\0';
		if (GlmCheckBinary(phenotypes + static_cast<size_t>(p) * n_out, n_out, why) != PGH_OK) {
			SetErr(errbuf, std::string(why) + " (phenotype " + std::to_string(p) + ")");
			return PGH_ERR_ARG;
		}
	}
	return PGH_OK;
}

// pgh_glm_score_multi, pgh_glm_score_multi_spa and pgh_glm_score_multi_firth after the latter two's own argument
// checks, and pgh_glm_score_multi_dosage, pgh_glm_score_multi_dosage_spa and pgh_glm_score_multi_dosage_firth
// (with_tracks: a dataset that holds dosage tracks is accepted).
int GlmScoreMultiEntry(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                       uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                       pgh_glm_row *out, const GlmScoreFollowUp &fu, char *errbuf, bool with_tracks = false) {
	PGH_ONE_DEVICE(ds);
	PGH_DENSE_ROWS(ds);
	PGH_TRY(GlmCheckCommon(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, PGH_GLM_LOGISTIC, out,
	                       errbuf));
	if (ds->dos_rows && !with_tracks) {
		SetErr(errbuf, "hardcalls only: the dataset holds " + std::to_string(ds->dos_rows) + " dosage tracks");
		return PGH_ERR_ARG;
	}
	PGH_TRY(GlmCheckBinaryEach(phenotypes, n_pheno, subset ? subset->n_out : ds->sample_ct, errbuf));
	if (v_end == v_begin) {
		return PGH_OK;
	}
	return GlmScoreMultiOne(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, errbuf, fu);
}

} // namespace

namespace {

// pgh_glm_score_sparse_multi, pgh_glm_score_sparse_multi_spa and pgh_glm_score_sparse_multi_firth after the latter two's
// own argument checks.
int GlmScoreSparseMultiEntry(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                             uint32_t n_pheno, const double *phenotypes, uint32_t n_covar, const double *covariates,
                             pgh_glm_row *out, const GlmScoreFollowUp &fu, char *errbuf) {
	PGH_ONE_DEVICE(ds);
	PGH_SPARSE_ROWS(ds);
	PGH_TRY(GlmCheckCommon(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, PGH_GLM_LOGISTIC, out,
	                       errbuf));
	PGH_TRY(GlmCheckBinaryEach(phenotypes, n_pheno, subset ? subset->n_out : ds->sample_ct, errbuf));
	if (v_end == v_begin) {
		return PGH_OK;
	}
	return GlmScoreSparseMultiOne(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, errbuf, fu);
}

} // namespace

extern "C" int pgh_glm_score_sparse_multi(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                          uint32_t v_end, uint32_t n_pheno, const double *phenotypes, uint32_t n_covar,
                                          const double *covariates, pgh_glm_row *out, char *errbuf) {
	return GlmScoreSparseMultiEntry(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, {}, errbuf);
}

extern "C" int pgh_glm_score_sparse_multi_spa(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                              uint32_t v_end, uint32_t n_pheno, const double *phenotypes,
                                              uint32_t n_covar, const double *covariates, double spa_cutoff,
                                              pgh_glm_row *out, double *p_spa, uint8_t *spa_state, char *errbuf) {
	PGH_TRY(GlmCheckSpa(spa_cutoff, p_spa, spa_state, errbuf));
	const GlmScoreFollowUp fu = {GlmScoreFollowUp::kSpa, spa_cutoff, p_spa, spa_state, nullptr};
	return GlmScoreSparseMultiEntry(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, fu, errbuf);
}

extern "C" int pgh_glm_score_sparse_multi_firth(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                                uint32_t v_end, uint32_t n_pheno, const double *phenotypes,
                                                uint32_t n_covar, const double *covariates, double firth_cutoff,
                                                pgh_glm_row *out, pgh_glm_firth_row *firth, char *errbuf) {
	PGH_TRY(GlmCheckFirth(firth_cutoff, firth, errbuf));
	const GlmScoreFollowUp fu = {GlmScoreFollowUp::kFirth, firth_cutoff, nullptr, nullptr, firth};
	return GlmScoreSparseMultiEntry(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, fu, errbuf);
}

extern "C" int pgh_glm_score_multi(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin, uint32_t v_end,
                                   uint32_t n_pheno, const double *phenotypes, uint32_t n_covar,
                                   const double *covariates, pgh_glm_row *out, char *errbuf) {
	return GlmScoreMultiEntry(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, {}, errbuf);
}

extern "C" int pgh_glm_score_multi_dosage(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                          uint32_t v_end, uint32_t n_pheno, const double *phenotypes, uint32_t n_covar,
                                          const double *covariates, pgh_glm_row *out, char *errbuf) {
	return GlmScoreMultiEntry(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, {}, errbuf, true);
}

extern "C" int pgh_glm_score_multi_dosage_spa(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                              uint32_t v_end, uint32_t n_pheno, const double *phenotypes,
                                              uint32_t n_covar, const double *covariates, double spa_cutoff,
                                              pgh_glm_row *out, double *p_spa, uint8_t *spa_state, char *errbuf) {
	PGH_TRY(GlmCheckSpa(spa_cutoff, p_spa, spa_state, errbuf));
	const GlmScoreFollowUp fu = {GlmScoreFollowUp::kSpa, spa_cutoff, p_spa, spa_state, nullptr};
	return GlmScoreMultiEntry(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, fu, errbuf,
	                          /*with_tracks=*/true);
}

extern "C" int pgh_glm_score_multi_dosage_firth(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                                uint32_t v_end, uint32_t n_pheno, const double *phenotypes,
                                                uint32_t n_covar, const double *covariates, double firth_cutoff,
                                                pgh_glm_row *out, pgh_glm_firth_row *firth, char *errbuf) {
	PGH_TRY(GlmCheckFirth(firth_cutoff, firth, errbuf));
	const GlmScoreFollowUp fu = {GlmScoreFollowUp::kFirth, firth_cutoff, nullptr, nullptr, firth};
	return GlmScoreMultiEntry(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, fu, errbuf,
	                          /*with_tracks=*/true);
}

extern "C" int pgh_glm_score_multi_spa(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                       uint32_t v_end, uint32_t n_pheno, const double *phenotypes, uint32_t n_covar,
                                       const double *covariates, double spa_cutoff, pgh_glm_row *out, double *p_spa,
                                       uint8_t *spa_state, char *errbuf) {
	PGH_TRY(GlmCheckSpa(spa_cutoff, p_spa, spa_state, errbuf));
	const GlmScoreFollowUp fu = {GlmScoreFollowUp::kSpa, spa_cutoff, p_spa, spa_state, nullptr};
	return GlmScoreMultiEntry(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, fu, errbuf);
}

extern "C" int pgh_glm_score_multi_firth(const pgh_dataset *ds, const pgh_subset *subset, uint32_t v_begin,
                                         uint32_t v_end, uint32_t n_pheno, const double *phenotypes, uint32_t n_covar,
                                         const double *covariates, double firth_cutoff, pgh_glm_row *out,
                                         pgh_glm_firth_row *firth, char *errbuf) {
	PGH_TRY(GlmCheckFirth(firth_cutoff, firth, errbuf));
	const GlmScoreFollowUp fu = {GlmScoreFollowUp::kFirth, firth_cutoff, nullptr, nullptr, firth};
	return GlmScoreMultiEntry(ds, subset, v_begin, v_end, n_pheno, phenotypes, n_covar, covariates, out, fu, errbuf);
}

extern "C" int pgh_burden_sparse(const pgh_dataset *ds, const pgh_subset *subset, const double *phenotype,
                                 uint32_t n_covar, const double *covariates, uint32_t n_sets, const uint64_t *set_off,
                                 const uint32_t *set_vidx, const double *weight, pgh_burden_row *out, char *errbuf) {
	PGH_ONE_DEVICE(ds);
	PGH_SPARSE_ROWS(ds);
	// the arguments pgh_glm_sparse has too, over the whole resident range (its `out` is checked below)
	PGH_TRY(GlmCheckCommon(ds, subset, ds ? ds->v_begin : 0, ds ? ds->v_begin : 0, 1, phenotype, n_covar, covariates,
	                       PGH_GLM_LINEAR, nullptr, errbuf));
	PGH_TRY(GlmCheckSets(ds, n_sets, set_off, set_vidx, weight, out, errbuf));
	return BurdenSparseOne(ds, subset, phenotype, n_covar, covariates, n_sets, set_off, set_vidx, weight, out, errbuf);
}

extern "C" int pgh_skat_sparse(const pgh_dataset *ds, const pgh_subset *subset, const double *phenotype, uint32_t n_covar,
                               const double *covariates, uint32_t n_sets, const uint64_t *set_off,
                               const uint32_t *set_vidx, const double *weight, pgh_skat_row *out, double *lambda_out,
                               char *errbuf) {
	PGH_ONE_DEVICE(ds);
	PGH_SPARSE_ROWS(ds);
	// the arguments pgh_glm_score_sparse has too, over the whole resident range (`out` is checked with the sets)
	int rc = GlmCheckCommon(ds, subset, ds ? ds->v_begin : 0, ds ? ds->v_begin : 0, 1, phenotype, n_covar, covariates,
	                        PGH_GLM_LOGISTIC, nullptr, errbuf);
	if (rc == PGH_OK) {
		rc = GlmCheckBinary(phenotype, subset ? subset->n_out : ds->sample_ct, errbuf);
	}
	if (rc == PGH_OK) {
		rc = GlmCheckSets(ds, n_sets, set_off, set_vidx, weight, out, errbuf);
	}
	if (rc != PGH_OK) {
		return rc;
	}
	for (uint32_t s = 0; s < n_sets; s++) {
		if (set_off[s + 1] - set_off[s] > PGH_SKAT_MAX_SET) {
			SetErr(errbuf, "set larger than PGH_SKAT_MAX_SET (" + std::to_string(PGH_SKAT_MAX_SET) + "): set " +
			                   std::to_string(s) + " holds " + std::to_string(set_off[s + 1] - set_off[s]) + " memberships");
			return PGH_ERR_ARG;
		}
	}
	return SkatSparseOne(ds, subset, phenotype, n_covar, covariates, n_sets, set_off, set_vidx, weight, out, lambda_out,
	                     errbuf);
}

extern "C" double pgh_skat_p_from_lambda(double q, const double *lambda, uint32_t n, uint8_t *state) {
	return pgh::SkatPFromLambda(q, lambda, n, state);
}

extern "C" int pgh_symmetric_eigenvalues(const double *a, uint32_t n, double *out) {
	if (!a || !out || n == 0) {
		return PGH_ERR_ARG;
	}
	pgh::SymmetricEigenvalues(a, n, out);
	return PGH_OK;
}
