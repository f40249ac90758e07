// api_grm.cpp -- pgh_grm / pgh_grm_standardize: the variance-standardised relationship matrix of the resident
// hardcalls (kernel in grm.hip, standardisation in grm_math.hpp).
#include "api_internal.hpp"
#include "grm.hpp"
#include "grm_math.hpp"

static_assert(PGH_GRM_TILE == pgh::kGrmTile, "tile size");

namespace {

constexpr uint32_t kGrmMaxVariants = 0x7fffffffu; // nobs is accumulated in int32
constexpr size_t kGrmBandBytes = 256ull << 20;     // device block of one band of rows (and its mirror strip)
const char *const kGrmBandEnv = "PGH_GRM_BAND_BYTES";

// The byte budget of a band: kGrmBandBytes, or less when the environment variable asks for it (read at every call;
// the result does not depend on it -- a test walks a small square in many bands with it)
uint64_t BandBytes() {
	const uint64_t v = EnvBytes(kGrmBandEnv, kGrmBandBytes);
	return v >= 1 ? std::min<uint64_t>(v, kGrmBandBytes) : kGrmBandBytes;
}

// raw samples [lo, hi) behind the output samples [begin, end): sel ascends
void RawRange(const pgh_subset *subset, uint32_t begin, uint32_t end, uint32_t &lo, uint32_t &hi) {
	lo = subset ? subset->sel[begin] : begin;
	hi = (subset ? subset->sel[end - 1] : end - 1) + 1;
	lo = lo / 256u * 256u; // the transpose works in blocks of 256 samples
}

} // namespace

extern "C" double pgh_grm_standardize(uint32_t het, uint32_t alt, uint32_t called, double z[3]) {
	const double p = pgh::GrmFreq(het, alt, called);
	double t[3];
	if (!pgh::GrmTable(p, t)) {
		return std::numeric_limits<double>::quiet_NaN();
	}
	if (z) {
		z[0] = t[0];
		z[1] = t[1];
		z[2] = t[2];
	}
	return p;
}

extern "C" int pgh_grm(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                       const uint32_t *vidx, const double *freq, uint32_t i_begin, uint32_t i_end, uint32_t j_begin,
                       uint32_t j_end, uint32_t flags, double *rel, uint32_t *nobs, uint32_t *n_used_out, char *errbuf) {
	if (!ds || !rel) {
		SetErr(errbuf, "null argument");
		return PGH_ERR_ARG;
	}
	PGH_ONE_DEVICE(ds);
	PGH_DENSE_ROWS(ds);
	PGH_ENTER(ds);
	int rc = CheckSubset(ds, subset, errbuf);
	if (rc == PGH_OK) {
		rc = RefuseEmptySubset(subset, errbuf);
	}
	if (rc != PGH_OK) {
		return rc;
	}
	if (flags & ~static_cast<uint32_t>(PGH_GRM_MEANIMPUTE)) {
		SetErr(errbuf, "unknown flag bits");
		return PGH_ERR_ARG;
	}
	const bool meanimpute = (flags & PGH_GRM_MEANIMPUTE) != 0;
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	rc = CheckSampleRect(i_begin, i_end, j_begin, j_end, n_out, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	if (n_var == 0) {
		SetErr(errbuf, "n_var must be at least 1");
		return PGH_ERR_ARG;
	}
	if (n_var > kGrmMaxVariants) {
		SetErr(errbuf, "n_var must not exceed 2^31 - 1 (the counts are accumulated in int32)");
		return PGH_ERR_ARG;
	}
	hipStream_t st = PghThreadStream();
	std::vector<double> table;
	HostSourceFence fence(st); // `table` feeds an asynchronous upload
	const uint32_t ni = i_end - i_begin, nj = j_end - j_begin;
	const uint64_t n_pairs = static_cast<uint64_t>(ni) * nj;

	// ---- counts over the output samples, the tables, and the list of the variants that are used ----
	VariantRows rows;
	rc = rows.ResolveAndUpload(ds, variant_begin, n_var, vidx, pgh::kVariantRowsExpand, st, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	uint32_t n_used = 0;
	{
		std::vector<uint32_t> counts(static_cast<size_t>(n_var) * 4);
		{
			DevBuf d_counts;
			PGH_HIP(d_counts.Alloc(counts.size() * sizeof(uint32_t)), "hipMalloc(grm counts)");
			PGH_HIP(pgh::LaunchCounts(ds->View(), 0, rows.Device(), n_var, subset ? subset->d_mask2 : nullptr, n_out,
			                          d_counts.As<uint32_t>(), st),
			        "counts kernel");
			PGH_HIP(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st),
			        "grm counts copy");
			PGH_HIP(hipStreamSynchronize(st), "grm counts sync"); // also: the list upload is done with rows.local
		}
		table.reserve(4 * (static_cast<size_t>(n_var) + pgh::kGrmKStep));
		for (uint32_t k = 0; k < n_var; k++) {
			double z[3];
			bool used;
			const uint32_t *c = &counts[4 * static_cast<size_t>(k)]; // hom-ref, het, hom-alt, missing
			const uint32_t called = c[0] + c[1] + c[2];
			if (freq) {
				used = called != 0 && pgh::GrmTable(freq[k], z);
			} else {
				used = !std::isnan(pgh_grm_standardize(c[1], c[2], called, z));
			}
			if (used) {
				rows.local[n_used++] = rows.local[k];
				table.insert(table.end(), {z[0], z[1], z[2], 0.0});
			}
		}
	}
	if (n_used_out) {
		*n_used_out = n_used;
	}
	if (n_used == 0) {
		std::fill(rel, rel + n_pairs, std::numeric_limits<double>::quiet_NaN());
		if (nobs) {
			std::fill(nobs, nobs + n_pairs, 0u);
		}
		return PGH_OK;
	}
	table.resize(4 * ((static_cast<size_t>(n_used) + pgh::kGrmKStep - 1) / pgh::kGrmKStep * pgh::kGrmKStep), 0.0);

	// ---- the sample-major 2-bit matrix of the used variants, for the samples the rectangle touches ----
	uint32_t lo_i, hi_i, lo_j, hi_j;
	RawRange(subset, i_begin, i_end, lo_i, hi_i);
	RawRange(subset, j_begin, j_end, lo_j, hi_j);
	const bool one_range = lo_i <= hi_j && lo_j <= hi_i; // overlapping or adjacent: one transpose of the union
	if (one_range) {
		lo_i = lo_j = std::min(lo_i, lo_j);
		hi_i = hi_j = std::max(hi_i, hi_j);
	}
	const uint64_t pitch = pgh::TransposedPitch(n_used);
	const uint64_t rows_i = hi_i - lo_i, rows_j = one_range ? 0 : hi_j - lo_j;
	DevBuf d_xt, d_table;
	PGH_HIP(d_xt.Alloc(pitch * (rows_i + rows_j)), "hipMalloc(grm sample-major matrix)");
	PGH_HIP(d_table.Alloc(sizeof(double) * table.size()), "hipMalloc(grm tables)");
	rc = rows.Upload(st, errbuf, n_used); // the used prefix of the list, into the same block
	if (rc != PGH_OK) {
		return rc;
	}
	PGH_HIP(hipMemcpyAsync(d_table.p, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st),
	        "grm tables upload");
	pgh::GrmOperand op {};
	op.xt_i = d_xt.As<uint8_t>();
	op.xt_j = one_range ? op.xt_i : op.xt_i + pitch * rows_i;
	op.raw_i0 = lo_i;
	op.raw_j0 = lo_j;
	op.pitch = pitch;
	op.sel = subset ? subset->d_sel : nullptr;
	op.table = d_table.As<double>();
	op.n_used = n_used;
	PGH_HIP(pgh::LaunchTranspose2bitRange(ds->View(), rows.Device(), n_used, lo_i, hi_i, d_xt.As<uint8_t>(), st),
	        "grm transpose kernel");
	if (!one_range) {
		PGH_HIP(pgh::LaunchTranspose2bitRange(ds->View(), rows.Device(), n_used, lo_j, hi_j,
		                                      d_xt.As<uint8_t>() + pitch * rows_i, st),
		        "grm transpose kernel");
	}

	// ---- bands of whole tile rows, so that the device block of a band stays bounded whatever the rectangle.  The
	// full square computes the tiles on and right of the diagonal only: a band writes its own rows from its first
	// column on, and the mirror of what lies below it into a strip of `rows` columns. ----
	const bool triangle = i_begin == j_begin && i_end == j_end;
	const uint64_t pair_bytes = sizeof(double) + (nobs ? sizeof(uint32_t) : 0);
	uint64_t band = BandBytes() / (pair_bytes * nj * (triangle ? 2 : 1)) / pgh::kGrmTile * pgh::kGrmTile;
	band = std::min<uint64_t>(std::max<uint64_t>(band, pgh::kGrmTile), 65535ull * pgh::kGrmTile);
	band = std::min<uint64_t>(band, ni);
	const uint64_t block = band * nj; // entries of the band's rows; the mirror strip is never larger
	DevBuf d_rel, d_nobs, d_rel_m, d_nobs_m;
	PGH_HIP(d_rel.Alloc(sizeof(double) * block), "hipMalloc(grm rel)");
	if (nobs) {
		PGH_HIP(d_nobs.Alloc(sizeof(uint32_t) * block), "hipMalloc(grm nobs)");
	}
	if (triangle && band < ni) {
		PGH_HIP(d_rel_m.Alloc(sizeof(double) * block), "hipMalloc(grm rel)");
		if (nobs) {
			PGH_HIP(d_nobs_m.Alloc(sizeof(uint32_t) * block), "hipMalloc(grm nobs)");
		}
	}
	for (uint64_t b0 = 0; b0 < ni; b0 += band) {
		const uint32_t rows = static_cast<uint32_t>(std::min<uint64_t>(band, ni - b0));
		const uint64_t b1 = b0 + rows;
		pgh::GrmOutput out {};
		out.rel = d_rel.As<double>();
		out.nobs = nobs ? d_nobs.As<uint32_t>() : nullptr;
		out.ld = nj;
		out.rel_m = d_rel_m.As<double>();
		out.nobs_m = nobs ? d_nobs_m.As<uint32_t>() : nullptr;
		out.ld_m = rows;
		PGH_HIP(pgh::LaunchGrm(op, i_begin + static_cast<uint32_t>(b0), i_begin + static_cast<uint32_t>(b1), j_begin, j_end,
		                       triangle, meanimpute, out, st),
		        "grm kernel");
		if (!triangle) {
			PGH_HIP(hipMemcpyAsync(rel + b0 * nj, d_rel.p, sizeof(double) * static_cast<uint64_t>(rows) * nj,
			                       hipMemcpyDeviceToHost, st),
			        "grm rel copy");
			if (nobs) {
				PGH_HIP(hipMemcpyAsync(nobs + b0 * nj, d_nobs.p, sizeof(uint32_t) * static_cast<uint64_t>(rows) * nj,
				                       hipMemcpyDeviceToHost, st),
				        "grm nobs copy");
			}
			continue;
		}
		// rows [b0, b1) x columns [b0, n), then rows [b1, n) x columns [b0, b1)
		const uint64_t right = nj - b0, below = nj - b1;
		PGH_HIP(hipMemcpy2DAsync(rel + b0 * nj + b0, sizeof(double) * nj, d_rel.As<double>() + b0, sizeof(double) * nj,
		                         sizeof(double) * right, rows, hipMemcpyDeviceToHost, st),
		        "grm rel copy");
		if (nobs) {
			PGH_HIP(hipMemcpy2DAsync(nobs + b0 * nj + b0, sizeof(uint32_t) * nj, d_nobs.As<uint32_t>() + b0,
			                         sizeof(uint32_t) * nj, sizeof(uint32_t) * right, rows, hipMemcpyDeviceToHost, st),
			        "grm nobs copy");
		}
		if (below) {
			PGH_HIP(hipMemcpy2DAsync(rel + b1 * nj + b0, sizeof(double) * nj, d_rel_m.p, sizeof(double) * rows,
			                         sizeof(double) * rows, below, hipMemcpyDeviceToHost, st),
			        "grm rel copy");
			if (nobs) {
				PGH_HIP(hipMemcpy2DAsync(nobs + b1 * nj + b0, sizeof(uint32_t) * nj, d_nobs_m.p, sizeof(uint32_t) * rows,
				                         sizeof(uint32_t) * rows, below, hipMemcpyDeviceToHost, st),
				        "grm nobs copy");
			}
		}
	}
	PGH_HIP(hipStreamSynchronize(st), "grm sync");
	return PGH_OK;
}
