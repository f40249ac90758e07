// api_ldband.cpp -- pgh_ld_window_sums / pgh_ld_prune / pgh_ld_exceeds / pgh_ld_scores / pgh_ld_r2: the six r2 sums
// of a rectangle of variant pairs, greedy LD pruning over a band of them, and the LD score of every variant of a band
// (kernel in ldband.hip, formulas in ld_math.hpp).
#include "api_internal.hpp"
#include "ld_math.hpp"
#include "ldband.hpp"

#include <cstdlib>

static_assert(PGH_LD_PLANES == pgh::kLdPlanes, "plane count");
static_assert(PGH_LDSCORE_UNBIASED == pgh::kLdScoreUnbiased, "flag value");

namespace {

constexpr uint32_t kLdMaxVariants = 0x7fffffffu;        // tile origins + tile size stay inside uint32
constexpr size_t kSumsBandBytes = 256ull << 20;          // device block of one band of pgh_ld_window_sums' rows
constexpr uint32_t kPruneChunkTiles = 32768;             // tiles per launch of pgh_ld_prune: 48 MiB of band bits
constexpr const char *kPruneChunkEnv = "PGH_LD_PRUNE_CHUNK_TILES";
constexpr uint32_t kScoreChunkTiles = 32768;             // tiles per launch of pgh_ld_scores: 84 MiB of partial sums
constexpr const char *kScoreChunkEnv = "PGH_LD_SCORE_CHUNK_TILES";

// The call's operand: the local row of each of its variants, on `st`.
struct LdCall {
	VariantRows rows;
	pgh::LdBandOperand op {};
};

int Prepare(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
            const uint32_t *vidx, bool increasing, hipStream_t st, LdCall &call, char *errbuf) {
	if (n_var == 0) {
		SetErr(errbuf, "n_var must be at least 1");
		return PGH_ERR_ARG;
	}
	if (n_var > kLdMaxVariants) {
		SetErr(errbuf, "n_var must not exceed 2^31 - 1");
		return PGH_ERR_ARG;
	}
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	if (n_out > pgh::kLdBandMaxSamples || ds->sample_ct > pgh::kLdBandMaxSamples) {
		SetErr(errbuf, "more than 2^29 - 1 samples (the sums are accumulated in int32)");
		return PGH_ERR_ARG;
	}
	const uint32_t flags = pgh::kVariantRowsExpand | (increasing ? pgh::kVariantRowsIncreasing : 0u);
	const int rc = call.rows.ResolveAndUpload(ds, variant_begin, n_var, vidx, flags, st, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	call.op.view = ds->View();
	call.op.list = call.rows.Device();
	call.op.n_var = n_var;
	call.op.mask2 = subset ? subset->d_mask2 : nullptr;
	return PGH_OK;
}

// tiles per launch: the environment variable when it holds a number of at least 1, capped at `most`
uint32_t ChunkTiles(const char *env, uint32_t most) {
	const uint64_t v = EnvBytes(env, most);
	return v >= 1 ? static_cast<uint32_t>(std::min<uint64_t>(v, most)) : most;
}

int CheckWindows(const uint32_t *win_end, uint32_t n_var, char *errbuf) {
	for (uint32_t k = 0; k < n_var; k++) {
		if (win_end[k] <= k || win_end[k] > n_var || (k && win_end[k] < win_end[k - 1])) {
			char msg[200];
			std::snprintf(msg, sizeof msg, "win_end[%u] = %u: need k < win_end[k] <= n_var (%u), not decreasing in k", k,
			              win_end[k], n_var);
			SetErr(errbuf, msg);
			return PGH_ERR_ARG;
		}
	}
	return PGH_OK;
}

// The tiles of anchor tile row ta that meet the band: partner tiles [first, first + count)
struct BandRow {
	uint32_t first = 0, count = 0;
};

BandRow RowTiles(uint32_t ta, uint32_t n_var, const uint32_t *win_end) {
	const uint64_t k0 = static_cast<uint64_t>(ta) * pgh::kLdTileA;
	const uint32_t k_last = static_cast<uint32_t>(std::min<uint64_t>(k0 + pgh::kLdTileA, n_var) - 1);
	const uint64_t lo = k0 + 1, hi = win_end[k_last]; // partners [lo, hi): win_end does not decrease
	BandRow row;
	if (lo < hi) {
		row.first = static_cast<uint32_t>(lo / pgh::kLdTileB);
		row.count = static_cast<uint32_t>((hi - 1) / pgh::kLdTileB) - row.first + 1;
	}
	return row;
}

} // namespace

extern "C" int pgh_ld_exceeds(const uint32_t sums[6], double r2_threshold) {
	return sums && pgh::LdExceeds(sums[0], sums[1], sums[2], sums[3], sums[4], sums[5], r2_threshold) ? 1 : 0;
}

extern "C" int pgh_ld_window_sums(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin,
                                  uint32_t n_var, const uint32_t *vidx, uint32_t a_begin, uint32_t a_end,
                                  uint32_t b_begin, uint32_t b_end, uint32_t *sums, char *errbuf) {
	if (!ds || !sums) {
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
	if (a_begin >= a_end || b_begin >= b_end || a_end > n_var || b_end > n_var) {
		char msg[200];
		std::snprintf(msg, sizeof msg, "variant rectangle [%u, %u) x [%u, %u) is empty, reversed or beyond the call's %u variants",
		              a_begin, a_end, b_begin, b_end, n_var);
		SetErr(errbuf, msg);
		return PGH_ERR_ARG;
	}
	hipStream_t st = PghThreadStream();
	LdCall call;
	rc = Prepare(ds, subset, variant_begin, n_var, vidx, false, st, call, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	// bands of whole tile rows, so that the device block of a band stays bounded whatever the rectangle
	const uint32_t na = a_end - a_begin, nb = b_end - b_begin;
	const uint32_t tiles_b = (nb + pgh::kLdTileB - 1) / pgh::kLdTileB;
	const uint64_t row_bytes = sizeof(uint32_t) * static_cast<uint64_t>(pgh::kLdPlanes) * nb;
	uint64_t band = kSumsBandBytes / row_bytes / pgh::kLdTileA * pgh::kLdTileA;
	band = std::min<uint64_t>(std::max<uint64_t>(band, pgh::kLdTileA), na);
	const uint32_t band_tile_rows = static_cast<uint32_t>((band + pgh::kLdTileA - 1) / pgh::kLdTileA);
	std::vector<pgh::LdTile> tiles(static_cast<size_t>(band_tile_rows) * tiles_b);
	HostSourceFence fence(st); // `tiles` feeds asynchronous uploads
	DevBuf d_out, d_tiles;
	PGH_HIP(d_out.Alloc(row_bytes * band), "hipMalloc(ld window sums)");
	PGH_HIP(d_tiles.Alloc(sizeof(pgh::LdTile) * tiles.size()), "hipMalloc(ld window tiles)");
	const uint64_t plane = static_cast<uint64_t>(na) * nb;
	for (uint64_t r0 = 0; r0 < na; r0 += band) {
		const uint32_t rows = static_cast<uint32_t>(std::min<uint64_t>(band, na - r0));
		const uint32_t first = a_begin + static_cast<uint32_t>(r0);
		uint32_t n_tiles = 0;
		for (uint32_t ta = 0; ta * pgh::kLdTileA < rows; ta++) {
			for (uint32_t tb = 0; tb < tiles_b; tb++) {
				tiles[n_tiles++] = pgh::LdTile {first + ta * pgh::kLdTileA, b_begin + tb * pgh::kLdTileB};
			}
		}
		PGH_HIP(hipStreamSynchronize(st), "ld window sums sync"); // the previous band's upload is done with `tiles`
		PGH_HIP(hipMemcpyAsync(d_tiles.p, tiles.data(), sizeof(pgh::LdTile) * n_tiles, hipMemcpyHostToDevice, st),
		        "ld window tiles upload");
		PGH_HIP(pgh::LaunchLdBandSums(call.op, d_tiles.As<pgh::LdTile>(), n_tiles, first, first + rows, b_begin, b_end,
		                              d_out.As<uint32_t>(), st),
		        "ld band kernel");
		for (uint32_t p = 0; p < pgh::kLdPlanes; p++) {
			PGH_HIP(hipMemcpyAsync(sums + p * plane + r0 * nb, d_out.As<uint32_t>() + static_cast<uint64_t>(p) * rows * nb,
			                       sizeof(uint32_t) * static_cast<uint64_t>(rows) * nb, hipMemcpyDeviceToHost, st),
			        "ld window sums copy");
		}
	}
	PGH_HIP(hipStreamSynchronize(st), "ld window sums sync");
	return PGH_OK;
}

extern "C" int pgh_ld_prune(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                            const uint32_t *vidx, const uint32_t *win_end, double r2_threshold, uint8_t *keep,
                            uint64_t *n_kept, char *errbuf) {
	if (!ds || !win_end || !keep) {
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
	if (!(r2_threshold >= 0.0 && r2_threshold <= 1.0)) { // NaN fails both
		SetErr(errbuf, "r2_threshold must be a finite number in [0, 1]");
		return PGH_ERR_ARG;
	}
	rc = CheckWindows(win_end, n_var, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	hipStream_t st = PghThreadStream();
	LdCall call;
	rc = Prepare(ds, subset, variant_begin, n_var, vidx, true, st, call, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;

	// per-variant minor-allele count and observation count from the class tallies
	std::vector<uint32_t> mc(n_var), obs(n_var);
	DevBuf d_win;
	{
		DevBuf d_counts;
		std::vector<uint32_t> counts(static_cast<size_t>(n_var) * 4);
		PGH_HIP(d_counts.Alloc(counts.size() * sizeof(uint32_t)), "hipMalloc(ld prune counts)");
		PGH_HIP(pgh::LaunchCounts(call.op.view, 0, call.op.list, n_var, call.op.mask2, n_out, d_counts.As<uint32_t>(), st),
		        "counts kernel");
		PGH_HIP(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st),
		        "ld prune counts copy");
		PGH_HIP(d_win.Alloc(sizeof(uint32_t) * static_cast<size_t>(n_var)), "hipMalloc(ld prune windows)");
		PGH_HIP(hipMemcpyAsync(d_win.p, win_end, sizeof(uint32_t) * static_cast<size_t>(n_var), hipMemcpyHostToDevice, st),
		        "ld prune windows upload");
		PGH_HIP(hipStreamSynchronize(st), "ld prune sync"); // the caller's win_end is read before the call returns
		for (uint32_t k = 0; k < n_var; k++) {
			const uint32_t *c = &counts[4 * static_cast<size_t>(k)];
			const uint32_t alt = c[1] + 2 * c[2];
			obs[k] = 2 * (c[0] + c[1] + c[2]);
			mc[k] = std::min(alt, obs[k] - alt);
		}
	}

	// Launches of at most `chunk` band tiles in (anchor tile row, partner tile) order; a tile row's bits are pruned
	// over once all of its tiles are back.  keep[] depends only on the bits, never on where the launches were cut.
	const uint32_t chunk = ChunkTiles(kPruneChunkEnv, kPruneChunkTiles);
	const uint32_t tile_rows = (n_var + pgh::kLdTileA - 1) / pgh::kLdTileA;
	std::memset(keep, 1, n_var);
	std::vector<pgh::LdTile> tiles;
	std::vector<uint32_t> bits;     // tile-major words of the tile rows [done_row, ...) that are on the host
	tiles.reserve(chunk);
	HostSourceFence fence(st);      // `tiles` feeds asynchronous uploads
	DevBuf d_tiles, d_bits;
	PGH_HIP(d_tiles.Alloc(sizeof(pgh::LdTile) * static_cast<size_t>(chunk)), "hipMalloc(ld prune tiles)");
	PGH_HIP(d_bits.Alloc(sizeof(uint32_t) * pgh::kLdTileBitWords * static_cast<size_t>(chunk)), "hipMalloc(ld prune bits)");
	uint32_t done_row = 0;          // tile rows below are pruned over
	uint32_t next_row = 0, next_tile = 0; // the next tile to launch: tile next_tile of tile row next_row
	constexpr uint32_t kWordsPerRow = pgh::kLdTileB / 32;
	while (done_row < tile_rows) {
		tiles.clear();
		while (next_row < tile_rows && tiles.size() < chunk) {
			const BandRow row = RowTiles(next_row, n_var, win_end);
			while (next_tile < row.count && tiles.size() < chunk) {
				tiles.push_back(pgh::LdTile {next_row * pgh::kLdTileA, (row.first + next_tile) * pgh::kLdTileB});
				next_tile++;
			}
			if (next_tile == row.count) {
				next_row++;
				next_tile = 0;
			}
		}
		if (!tiles.empty()) {
			const size_t had = bits.size(), words = tiles.size() * pgh::kLdTileBitWords;
			bits.resize(had + words);
			PGH_HIP(hipMemcpyAsync(d_tiles.p, tiles.data(), sizeof(pgh::LdTile) * tiles.size(), hipMemcpyHostToDevice, st),
			        "ld prune tiles upload");
			PGH_HIP(pgh::LaunchLdBandBits(call.op, d_tiles.As<pgh::LdTile>(), static_cast<uint32_t>(tiles.size()),
			                              d_win.As<uint32_t>(), r2_threshold, d_bits.As<uint32_t>(), st),
			        "ld band kernel");
			PGH_HIP(hipMemcpyAsync(bits.data() + had, d_bits.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost, st),
			        "ld prune bits copy");
			PGH_HIP(hipStreamSynchronize(st), "ld prune sync");
		}
		// the sequential rule over every tile row whose tiles are all here
		size_t used = 0;
		for (; done_row < next_row; done_row++) {
			const BandRow row = RowTiles(done_row, n_var, win_end);
			const uint32_t *rb = bits.data() + used;
			const uint64_t k0 = static_cast<uint64_t>(done_row) * pgh::kLdTileA;
			for (uint32_t r = 0; r < pgh::kLdTileA && k0 + r < n_var; r++) {
				const uint32_t k = static_cast<uint32_t>(k0 + r);
				bool k_kept = keep[k] != 0;
				for (uint32_t ti = 0; ti < row.count && k_kept; ti++) {
					const uint32_t *w = rb + (static_cast<size_t>(ti) * pgh::kLdTileA + r) * kWordsPerRow;
					for (uint32_t j = 0; j < kWordsPerRow && k_kept; j++) {
						for (uint32_t word = w[j]; word; word &= word - 1) {
							const uint32_t u = (row.first + ti) * pgh::kLdTileB + 32 * j + static_cast<uint32_t>(__builtin_ctz(word));
							if (!keep[u]) {
								continue;
							}
							if (pgh::LdLowerMaf(mc[k], obs[k], mc[u], obs[u])) {
								keep[k] = 0;
								k_kept = false;
								break;
							}
							keep[u] = 0; // ties remove the later variant
						}
					}
				}
			}
			used += static_cast<size_t>(row.count) * pgh::kLdTileBitWords;
		}
		bits.erase(bits.begin(), bits.begin() + static_cast<ptrdiff_t>(used));
	}
	if (n_kept) {
		uint64_t kept = 0;
		for (uint32_t k = 0; k < n_var; k++) {
			kept += keep[k];
		}
		*n_kept = kept;
	}
	return PGH_OK;
}

extern "C" int pgh_ld_r2(const uint32_t sums[6], uint32_t flags, double *term) {
	double v = 0.0;
	if (!sums || (flags & ~static_cast<uint32_t>(PGH_LDSCORE_UNBIASED)) ||
	    !pgh::LdR2Term(sums[0], sums[1], sums[2], sums[3], sums[4], sums[5], flags, &v)) {
		return 0;
	}
	if (term) {
		*term = v;
	}
	return 1;
}

extern "C" int pgh_ld_scores(const pgh_dataset *ds, const pgh_subset *subset, uint32_t variant_begin, uint32_t n_var,
                             const uint32_t *vidx, const uint32_t *win_end, uint32_t flags, double *score,
                             uint32_t *n_partners, char *errbuf) {
	if (!ds || !win_end || !score) {
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
	if (flags & ~static_cast<uint32_t>(PGH_LDSCORE_UNBIASED)) {
		SetErr(errbuf, "unknown flag bits (PGH_LDSCORE_UNBIASED is the only flag)");
		return PGH_ERR_ARG;
	}
	rc = CheckWindows(win_end, n_var, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	hipStream_t st = PghThreadStream();
	LdCall call;
	rc = Prepare(ds, subset, variant_begin, n_var, vidx, true, st, call, errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;

	// self terms from the class tallies: a variant against itself has r2 = 1 wherever it has an r2 at all
	std::vector<uint32_t> partners(n_var, 0u);
	DevBuf d_win;
	{
		DevBuf d_counts;
		std::vector<uint32_t> counts(static_cast<size_t>(n_var) * 4);
		PGH_HIP(d_counts.Alloc(counts.size() * sizeof(uint32_t)), "hipMalloc(ld scores counts)");
		PGH_HIP(pgh::LaunchCounts(call.op.view, 0, call.op.list, n_var, call.op.mask2, n_out, d_counts.As<uint32_t>(), st),
		        "counts kernel");
		PGH_HIP(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st),
		        "ld scores counts copy");
		PGH_HIP(d_win.Alloc(sizeof(uint32_t) * static_cast<size_t>(n_var)), "hipMalloc(ld scores windows)");
		PGH_HIP(hipMemcpyAsync(d_win.p, win_end, sizeof(uint32_t) * static_cast<size_t>(n_var), hipMemcpyHostToDevice, st),
		        "ld scores windows upload");
		PGH_HIP(hipStreamSynchronize(st), "ld scores sync"); // the caller's win_end is read before the call returns
		for (uint32_t k = 0; k < n_var; k++) {
			const uint32_t *c = &counts[4 * static_cast<size_t>(k)];
			const uint32_t called = c[0] + c[1] + c[2], s1 = c[1] + 2 * c[2], s2 = c[1] + 4 * c[2];
			double self = 0.0;
			score[k] = pgh::LdR2Term(called, s1, s1, s2, s2, s2, flags, &self) ? 1.0 : 0.0;
		}
	}

	// Launches of at most `chunk` band tiles in (anchor tile row, partner tile) order.  Each tile's 96 row sums go to
	// its anchors and then its 128 column sums to its partners, tile after tile in that order: the result is a function
	// of the tile list alone, never of where the launches were cut.
	const uint32_t chunk = ChunkTiles(kScoreChunkEnv, kScoreChunkTiles);
	const uint32_t tile_rows = (n_var + pgh::kLdTileA - 1) / pgh::kLdTileA;
	constexpr uint32_t kSlots = pgh::kLdTileScoreSlots;
	std::vector<pgh::LdTile> tiles;
	std::vector<double> part;
	std::vector<uint32_t> cnt;
	tiles.reserve(chunk);
	HostSourceFence fence(st); // `tiles` feeds asynchronous uploads
	DevBuf d_tiles, d_part, d_cnt;
	PGH_HIP(d_tiles.Alloc(sizeof(pgh::LdTile) * static_cast<size_t>(chunk)), "hipMalloc(ld scores tiles)");
	PGH_HIP(d_part.Alloc(sizeof(double) * kSlots * static_cast<size_t>(chunk)), "hipMalloc(ld scores partial sums)");
	PGH_HIP(d_cnt.Alloc(sizeof(uint32_t) * kSlots * static_cast<size_t>(chunk)), "hipMalloc(ld scores partial counts)");
	uint32_t next_row = 0, next_tile = 0; // the next tile to launch: tile next_tile of tile row next_row
	while (next_row < tile_rows) {
		tiles.clear();
		while (next_row < tile_rows && tiles.size() < chunk) {
			const BandRow row = RowTiles(next_row, n_var, win_end);
			while (next_tile < row.count && tiles.size() < chunk) {
				tiles.push_back(pgh::LdTile {next_row * pgh::kLdTileA, (row.first + next_tile) * pgh::kLdTileB});
				next_tile++;
			}
			if (next_tile == row.count) {
				next_row++;
				next_tile = 0;
			}
		}
		if (tiles.empty()) {
			continue;
		}
		const size_t slots = tiles.size() * kSlots;
		part.resize(slots);
		cnt.resize(slots);
		PGH_HIP(hipMemcpyAsync(d_tiles.p, tiles.data(), sizeof(pgh::LdTile) * tiles.size(), hipMemcpyHostToDevice, st),
		        "ld scores tiles upload");
		PGH_HIP(pgh::LaunchLdBandScores(call.op, d_tiles.As<pgh::LdTile>(), static_cast<uint32_t>(tiles.size()),
		                                d_win.As<uint32_t>(), flags, d_part.As<double>(), d_cnt.As<uint32_t>(), st),
		        "ld band kernel");
		PGH_HIP(hipMemcpyAsync(part.data(), d_part.p, sizeof(double) * slots, hipMemcpyDeviceToHost, st),
		        "ld scores partial sums copy");
		PGH_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(uint32_t) * slots, hipMemcpyDeviceToHost, st),
		        "ld scores partial counts copy");
		PGH_HIP(hipStreamSynchronize(st), "ld scores sync");
		for (size_t ti = 0; ti < tiles.size(); ti++) {
			const double *p = &part[ti * kSlots];
			const uint32_t *c = &cnt[ti * kSlots];
			const uint64_t a0 = tiles[ti].a0, b0 = tiles[ti].b0;
			for (uint32_t r = 0; r < pgh::kLdTileA && a0 + r < n_var; r++) {
				score[a0 + r] += p[r];
				partners[a0 + r] += c[r];
			}
			for (uint32_t j = 0; j < pgh::kLdTileB && b0 + j < n_var; j++) {
				score[b0 + j] += p[pgh::kLdTileA + j];
				partners[b0 + j] += c[pgh::kLdTileA + j];
			}
		}
	}
	if (n_partners) {
		std::memcpy(n_partners, partners.data(), sizeof(uint32_t) * static_cast<size_t>(n_var));
	}
	return PGH_OK;
}
