// api_het.cpp -- pgh_het / pgh_het_expected / pgh_het_scale: per-sample observed and expected homozygosity and the
// method-of-moments inbreeding coefficient, in exact fixed point (kernel in het.hip, per-variant formulas in
// het_math.hpp).
#include "api_internal.hpp"
#include "het.hpp"
#include "het_math.hpp"

static_assert(PGH_HET_TILE == pgh::kHetTile, "tile size");
static_assert(sizeof(pgh_het_row) == 32, "pgh_het_row layout");

namespace {

const char *const kHetSlicesEnv = "PGH_HET_SLICES";

} // namespace

// One dense-resident dataset's raw integer sums under the scale k: e_sum, hom_ct and obs_ct of the n_out output
// samples (set, not added to), and per variant of the call whether it was used.  Entry i of the call reads
// freq[pos ? pos[i] : i] and writes used[pos ? pos[i] : i] (freq and used may be null); *n_used is set.  The checks of
// pgh_het's flags are the caller's.
int PghHetSums(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
               const uint32_t *vidx, const double *freq, const uint32_t *pos, uint32_t flags, uint32_t k, int64_t *e_sum,
               uint32_t *hom_ct, uint32_t *obs_ct, uint8_t *used, uint32_t *n_used_out, char *errbuf) {
	PGH_DENSE_ROWS(ds);
	PGH_ENTER(ds);
	PGH_TRY(CheckSubset(ds, subset, errbuf));
	const uint32_t N = ds->sample_ct;
	const uint32_t n_out = subset ? subset->n_out : N;
	const uint32_t padded = (N + 63) / 64 * 64;
	const bool small_sample = (flags & PGH_HET_SMALL_SAMPLE) != 0;
	hipStream_t st = PghThreadStream();
	DevBuf d_counts, d_cls, d_scratch, d_q, d_msum;
	std::vector<unsigned long long> q;
	std::vector<uint32_t> counts, cls;
	std::vector<unsigned long long> msum;
	std::vector<uint8_t> used_local(n_var, 0);
	HostSourceFence fence(st); // `q` feeds an asynchronous upload
	VariantRows rows;
	PGH_TRY(rows.ResolveAndUpload(ds, variant_begin, n_var, vidx, pgh::kVariantRowsExpand, st, errbuf));

	// ---- counts over the output samples, the fixed-point weights, and the list of the variants that are used ----
	uint32_t n_used = 0;
	uint64_t q_tot = 0;
	if (n_var && n_out) { // under the empty subset nothing is called anywhere: every variant is skipped
		counts.resize(static_cast<size_t>(n_var) * 4);
		PGH_HIP(d_counts.Alloc(counts.size() * sizeof(uint32_t)), "hipMalloc(het counts)");
		PGH_HIP(pgh::LaunchCounts(ds->View(), 0, rows.Device(), n_var, subset ? subset->d_mask2 : nullptr, n_out,
		                          d_counts.As<uint32_t>(), st),
		        "counts kernel");
		PGH_HIP(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st),
		        "het counts copy");
		PGH_HIP(hipStreamSynchronize(st), "het counts sync"); // also: the list upload is done with rows.local
		q.reserve(n_var);
		for (uint32_t i = 0; i < n_var; i++) {
			const uint32_t *c = &counts[4 * static_cast<size_t>(i)]; // hom-ref, het, hom-alt, missing
			const uint32_t called = c[0] + c[1] + c[2];
			double e = 0.0;
			bool use;
			if (freq) {
				const double p = freq[pos ? pos[i] : i];
				use = !std::isnan(p) && pgh::HetExpected(c[1], c[2], called, p, false, &e);
			} else {
				use = pgh::HetExpected(c[1], c[2], called, std::numeric_limits<double>::quiet_NaN(), small_sample, &e);
			}
			if (use) {
				const uint64_t qv = static_cast<uint64_t>(pgh::HetFixed(e, k));
				rows.local[n_used++] = rows.local[i];
				q.push_back(qv);
				q_tot += qv;
				used_local[i] = 1;
			}
		}
	}

	// ---- het and missing per raw sample over the used rows, and the weights summed on the missing side ----
	if (n_used) {
		PGH_HIP(d_cls.Alloc(sizeof(uint32_t) * 3ull * padded), "hipMalloc(het sample counts)");
		PGH_HIP(d_scratch.Alloc(pgh::ClassCounts3ScratchBytes(ds->record_bytes)), "hipMalloc(het sample counts)");
		PGH_HIP(d_q.Alloc(sizeof(unsigned long long) * q.size()), "hipMalloc(het weights)");
		PGH_HIP(d_msum.Alloc(sizeof(unsigned long long) * static_cast<size_t>(N)), "hipMalloc(het sums)");
		PGH_TRY(rows.Upload(st, errbuf, n_used)); // the used prefix of the list, into the same block
		PGH_HIP(hipMemcpyAsync(d_q.p, q.data(), sizeof(unsigned long long) * q.size(), hipMemcpyHostToDevice, st),
		        "het weights upload");
		PGH_HIP(pgh::LaunchClassCounts3(ds->View(), 0, rows.Device(), n_used, d_scratch.As<uint8_t>(), d_cls.As<uint32_t>(),
		                                padded, st),
		        "sample counts kernel");
		int cus = 0;
		PGH_TRY(DeviceCus(&cus, "het", errbuf));
		const uint64_t env = EnvBytes(kHetSlicesEnv, 0);
		const uint32_t slices = env ? static_cast<uint32_t>(std::min<uint64_t>(env, pgh::kHetMaxSlices))
		                            : pgh::HetDefaultSlices(N, n_used, cus);
		PGH_HIP(pgh::LaunchHetMissingSum(ds->View(), rows.Device(), n_used, d_q.As<unsigned long long>(), slices,
		                                 d_msum.As<unsigned long long>(), st),
		        "het kernel");
		cls.resize(3ull * padded);
		msum.resize(N);
		PGH_HIP(hipMemcpyAsync(cls.data(), d_cls.p, sizeof(uint32_t) * cls.size(), hipMemcpyDeviceToHost, st),
		        "het sample counts copy");
		PGH_HIP(hipMemcpyAsync(msum.data(), d_msum.p, sizeof(unsigned long long) * msum.size(), hipMemcpyDeviceToHost, st),
		        "het sums copy");
		PGH_HIP(hipStreamSynchronize(st), "het sync");
	}

	// ---- the subset's samples, in subset order ----
	for (uint32_t j = 0; j < n_out; j++) {
		const uint32_t s = subset ? subset->sel[j] : j;
		const uint32_t het = n_used ? cls[s] : 0u, miss = n_used ? cls[2ull * padded + s] : 0u;
		obs_ct[j] = n_used - miss;
		hom_ct[j] = n_used - miss - het;
		e_sum[j] = static_cast<int64_t>(n_used ? q_tot - msum[s] : 0ull);
	}
	for (uint32_t i = 0; used && i < n_var; i++) {
		used[pos ? pos[i] : i] = used_local[i];
	}
	*n_used_out = n_used;
	return PGH_OK;
}

extern "C" uint32_t pgh_het_scale(uint32_t n_var) {
	return pgh::HetScale(n_var);
}

extern "C" int pgh_het_expected(uint32_t het, uint32_t alt, uint32_t called, double freq, uint32_t flags, double *e) {
	if ((flags & ~static_cast<uint32_t>(PGH_HET_SMALL_SAMPLE)) || (flags && !std::isnan(freq)) || !e) {
		return 0;
	}
	double v;
	if (!pgh::HetExpected(het, alt, called, freq, (flags & PGH_HET_SMALL_SAMPLE) != 0, &v)) {
		return 0;
	}
	*e = v;
	return 1;
}

extern "C" int pgh_het(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                       const uint32_t *vidx, const double *freq, uint32_t flags, pgh_het_row *out, uint8_t *used,
                       uint32_t *n_used_out, char *errbuf) {
	// the flags first: these refusals need no dataset
	if (flags & ~static_cast<uint32_t>(PGH_HET_SMALL_SAMPLE)) {
		SetErr(errbuf, "unknown flag bits");
		return PGH_ERR_ARG;
	}
	if (freq && (flags & PGH_HET_SMALL_SAMPLE)) {
		SetErr(errbuf, "PGH_HET_SMALL_SAMPLE cannot be combined with freq: the correction needs the counts' own n");
		return PGH_ERR_ARG;
	}
	if (!ds || !out) {
		SetErr(errbuf, "null argument");
		return PGH_ERR_ARG;
	}
	PGH_DENSE_ROWS(ds);
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	const uint32_t k = pgh::HetScale(n_var);
	std::vector<int64_t> e_sum(n_out);
	std::vector<uint32_t> hom_ct(n_out), obs_ct(n_out);
	std::vector<uint8_t> used_local(used ? n_var : 0);
	uint8_t *used_p = used ? used_local.data() : nullptr;
	uint32_t n_used = 0;
	if (ds->IsGroup()) {
		PGH_TRY(pgh_group::Het(ds, subset, variant_begin, n_var, vidx, freq, flags, k, e_sum.data(), hom_ct.data(),
		                       obs_ct.data(), used_p, &n_used, errbuf));
	} else {
		PGH_TRY(PghHetSums(ds, subset, variant_begin, n_var, vidx, freq, nullptr, flags, k, e_sum.data(), hom_ct.data(),
		                   obs_ct.data(), used_p, &n_used, errbuf));
	}
	for (uint32_t j = 0; j < n_out; j++) {
		pgh_het_row &r = out[j];
		r.e_sum = e_sum[j];
		r.hom_ct = hom_ct[j];
		r.obs_ct = obs_ct[j];
		r.e_hom = std::ldexp(static_cast<double>(e_sum[j]), -static_cast<int>(k));
		const double num = static_cast<double>(hom_ct[j]) - r.e_hom;
		const double den = static_cast<double>(obs_ct[j]) - r.e_hom;
		r.f = obs_ct[j] == 0 || den == 0.0 ? std::numeric_limits<double>::quiet_NaN() : num / den;
	}
	if (used && n_var) {
		std::memcpy(used, used_local.data(), n_var);
	}
	if (n_used_out) {
		*n_used_out = n_used;
	}
	return PGH_OK;
}
