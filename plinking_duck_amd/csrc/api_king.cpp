// api_king.cpp -- pgh_king_counts / pgh_king_table / pgh_king_kinship: KING-robust pair counts and kinship of the
// resident hardcalls (kernels in king.hip, formula in king_math.hpp).
#include "api_internal.hpp"
#include "king.hpp"
#include "king_math.hpp"

static_assert(sizeof(pgh_king_pair) == sizeof(pgh::KingPair) && sizeof(pgh_king_pair) == 40, "pgh_king_pair layout");
static_assert(offsetof(pgh_king_pair, kinship) == offsetof(pgh::KingPair, kinship), "pgh_king_pair layout");
static_assert(PGH_KING_PLANES == pgh::kKingPlanes, "plane count");

namespace {

constexpr uint32_t kKingMaxVariants = 0x7fffffffu;  // an int32 accumulator holds any count
constexpr size_t kCountsBandBytes = 256ull << 20;    // device block of one band of pgh_king_counts' rows
constexpr uint64_t kTableBandTiles = 4096;           // tiles per launch of pgh_king_table, at least
constexpr uint64_t kTableFirstCapacity = 1ull << 20; // records of the first device list (grown on demand)

// The call's operand: the sample-major 2-bit matrix of its variants, on `st`.
struct KingCall {
	DevBuf d_xt;
	pgh::KingOperand op {};
};

int Prepare(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
            const uint32_t *vidx, hipStream_t st, KingCall &call, char *errbuf) {
	if (n_var == 0) {
		SetErr(errbuf, "n_var must be at least 1");
		return PGH_ERR_ARG;
	}
	if (n_var > kKingMaxVariants) {
		SetErr(errbuf, "n_var must not exceed 2^31 - 1 (the counts are accumulated in int32)");
		return PGH_ERR_ARG;
	}
	VariantRows rows; // local: the list serves the transpose alone, and its drain is the one this function ends with
	const int rc = rows.ResolveAndUpload(ds, variant_begin, n_var, vidx, pgh::kVariantRowsExpand, st, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	const uint64_t pitch = pgh::TransposedPitch(n_var);
	PGH_HIP(call.d_xt.Alloc(pitch * ds->sample_ct), "hipMalloc(king sample-major matrix)");
	PGH_HIP(pgh::LaunchTranspose2bit(ds->View(), rows.Device(), n_var, call.d_xt.As<uint8_t>(), st),
	        "king transpose kernel");
	call.op.xt = call.d_xt.As<uint8_t>();
	call.op.pitch = pitch;
	call.op.sel = subset ? subset->d_sel : nullptr;
	call.op.n_var = n_var;
	return PGH_OK;
}

} // namespace

extern "C" double pgh_king_kinship(uint32_t hethet, uint32_t ibs0, uint32_t het1hom2, uint32_t het2hom1) {
	return pgh::KingKinship(hethet, ibs0, het1hom2, het2hom1);
}

extern "C" int pgh_king_counts(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                               const uint32_t *vidx, uint32_t i_begin, uint32_t i_end, uint32_t j_begin, uint32_t j_end,
                               uint32_t *counts, char *errbuf) {
	if (!ds || !counts) {
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
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	rc = CheckSampleRect(i_begin, i_end, j_begin, j_end, n_out, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	hipStream_t st = PghThreadStream();
	KingCall call;
	rc = Prepare(ds, subset, variant_begin, n_var, vidx, st, call, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	// bands of whole tile rows, so that the device block of a band stays bounded whatever the rectangle
	const uint32_t ni = i_end - i_begin, nj = j_end - j_begin;
	const uint64_t row_bytes = sizeof(uint32_t) * static_cast<uint64_t>(pgh::kKingPlanes) * nj;
	uint64_t band = kCountsBandBytes / row_bytes / pgh::kKingTile * pgh::kKingTile;
	band = std::min<uint64_t>(std::max<uint64_t>(band, pgh::kKingTile), 65535ull * pgh::kKingTile);
	band = std::min<uint64_t>(band, ni);
	DevBuf d_out;
	PGH_HIP(d_out.Alloc(row_bytes * band), "hipMalloc(king counts)");
	const uint64_t plane = static_cast<uint64_t>(ni) * nj;
	for (uint64_t b0 = 0; b0 < ni; b0 += band) {
		const uint32_t rows = static_cast<uint32_t>(std::min<uint64_t>(band, ni - b0));
		PGH_HIP(pgh::LaunchKingCounts(call.op, i_begin + static_cast<uint32_t>(b0), i_begin + static_cast<uint32_t>(b0) + rows,
		                              j_begin, j_end, d_out.As<uint32_t>(), st),
		        "king counts kernel");
		for (uint32_t p = 0; p < pgh::kKingPlanes; p++) {
			PGH_HIP(hipMemcpyAsync(counts + p * plane + b0 * nj, d_out.As<uint32_t>() + static_cast<uint64_t>(p) * rows * nj,
			                       sizeof(uint32_t) * static_cast<uint64_t>(rows) * nj, hipMemcpyDeviceToHost, st),
			        "king counts copy");
		}
	}
	PGH_HIP(hipStreamSynchronize(st), "king counts sync");
	return PGH_OK;
}

extern "C" int pgh_king_table(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                              const uint32_t *vidx, double min_kinship, pgh_king_pair *out, uint64_t capacity,
                              uint64_t *n_pairs, char *errbuf) {
	if (!ds || !n_pairs || (!out && capacity)) {
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
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	hipStream_t st = PghThreadStream();
	KingCall call;
	rc = Prepare(ds, subset, variant_begin, n_var, vidx, st, call, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	const bool no_filter = std::isnan(min_kinship) || (std::isinf(min_kinship) && min_kinship < 0);
	const uint32_t tiles = (n_out + pgh::kKingTile - 1) / pgh::kKingTile;
	const uint64_t all_pairs = static_cast<uint64_t>(n_out) * (n_out ? n_out - 1 : 0) / 2;
	// The survivors of a band of tile rows land in a device list in the order the waves' counter adds arrive, and
	// are sorted by (i, j) here: the bands ascend in i, so the table is in (i, j) order and the same every run.
	// A band that outgrows the list is run again with a list of the size it asked for.
	uint64_t list_cap = capacity ? std::max<uint64_t>(1, std::min(all_pairs, kTableFirstCapacity)) : 0;
	DevBuf d_count;
	std::unique_ptr<DevBuf> d_list(new DevBuf);
	PGH_HIP(d_count.Alloc(sizeof(unsigned long long)), "hipMalloc(king table)");
	if (list_cap) {
		PGH_HIP(d_list->Alloc(sizeof(pgh::KingPair) * list_cap), "hipMalloc(king table)");
	}
	std::vector<pgh::KingPair> band_pairs;
	uint64_t total = 0, written = 0;
	for (uint32_t r0 = 0; r0 < tiles;) {
		uint32_t r1 = r0;
		for (uint64_t in_band = 0; r1 < tiles && in_band < kTableBandTiles; r1++) {
			in_band += tiles - r1;
		}
		r1 = std::min(r1, r0 + 65535u);
		const bool keep = written < capacity;
		unsigned long long found = 0;
		for (int attempt = 0; attempt < 2; attempt++) {
			PGH_HIP(hipMemsetAsync(d_count.p, 0, sizeof(unsigned long long), st), "king table memset");
			PGH_HIP(pgh::LaunchKingTable(call.op, n_out, r0, r1, min_kinship, no_filter, d_list->As<pgh::KingPair>(),
			                             keep ? list_cap : 0, d_count.As<unsigned long long>(), st),
			        "king table kernel");
			PGH_HIP(hipMemcpyAsync(&found, d_count.p, sizeof found, hipMemcpyDeviceToHost, st), "king table copy");
			PGH_HIP(hipStreamSynchronize(st), "king table sync");
			if (!keep || found <= list_cap) {
				break;
			}
			d_list.reset(new DevBuf); // frees the old list first
			list_cap = found;
			PGH_HIP(d_list->Alloc(sizeof(pgh::KingPair) * list_cap), "hipMalloc(king table)");
		}
		total += found;
		if (keep && found) {
			band_pairs.resize(found);
			PGH_HIP(hipMemcpyAsync(band_pairs.data(), d_list->p, sizeof(pgh::KingPair) * found, hipMemcpyDeviceToHost, st),
			        "king table copy");
			PGH_HIP(hipStreamSynchronize(st), "king table sync");
			std::sort(band_pairs.begin(), band_pairs.end(), [](const pgh::KingPair &x, const pgh::KingPair &y) {
				return x.i != y.i ? x.i < y.i : x.j < y.j;
			});
			const uint64_t take = std::min<uint64_t>(found, capacity - written);
			std::memcpy(out + written, band_pairs.data(), sizeof(pgh::KingPair) * take);
			written += take;
		}
		r0 = r1;
	}
	*n_pairs = total;
	return PGH_OK;
}
