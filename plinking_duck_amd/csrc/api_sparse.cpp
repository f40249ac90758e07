// api_sparse.cpp -- the sparse-resident form of a dataset (pgh_open_sparse; layout in sparse.hpp): built window by
// window from the ordinary decoder (PghOpenRows of [w0, w1): every record type, LD bases before the window, .pgi
// tables), each window's rows classified and compacted on the device, the window dropped, the windows' parts
// concatenated at the end.  Peak device memory: the sparse data twice plus one window.
// Also pgh_score_sparse, plink_score over such a dataset (kernels in score_sparse.hip).
#include "api_internal.hpp"

#include <atomic>

namespace {

std::atomic<uint64_t> g_sparse_opens {0};

// rows per window: PGH_SPARSE_WINDOW_BYTES of rows (default 2 GB)
uint32_t WindowRows(uint64_t pitch) {
	uint64_t bytes = 2ull << 30;
	if (const char *e = std::getenv("PGH_SPARSE_WINDOW_BYTES")) {
		const long long v = std::atoll(e);
		if (v > 0) {
			bytes = static_cast<uint64_t>(v);
		}
	}
	return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(bytes / pitch, 1u << 30)));
}

// one window's compacted rows (device blocks owned until the concatenation)
struct Part {
	uint32_t rows = 0;
	uint32_t dense = 0;
	uint64_t entries = 0;
	std::vector<int32_t> row_of; // window-local pool rows / -1 - base
	std::vector<uint64_t> off;   // window-local entry offsets, rows + 1
	uint32_t *d_entries = nullptr;
	uint8_t *d_pool = nullptr;
	void Free() {
		if (d_entries) {
			(void)hipFree(d_entries);
			d_entries = nullptr;
		}
		if (d_pool) {
			(void)hipFree(d_pool);
			d_pool = nullptr;
		}
	}
};

// Classify and compact the rows of one decoded window into `part`.
int CompactWindow(const pgh_dataset *win, uint32_t max_minor, hipStream_t st, Part &part, char *errbuf) {
	const uint32_t n = win->v_end - win->v_begin;
	part.rows = n;
	std::vector<uint32_t> cls(2ull * n);
	{
		DevBuf d_cls;
		PGH_HIP(d_cls.Alloc(sizeof(uint32_t) * 2ull * n), "hipMalloc(sparse classes)");
		PGH_HIP(pgh::LaunchSparseClassify(win->View(), n, d_cls.As<uint32_t>(), st), "sparse classify kernel");
		PGH_HIP(hipMemcpyAsync(cls.data(), d_cls.p, sizeof(uint32_t) * 2ull * n, hipMemcpyDeviceToHost, st),
		        "sparse classes copy");
		PGH_HIP(hipStreamSynchronize(st), "sparse classify sync");
	}
	part.row_of.resize(n);
	part.off.resize(static_cast<size_t>(n) + 1);
	uint64_t entries = 0;
	uint32_t dense = 0;
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t major = cls[2ull * i], minor = cls[2ull * i + 1];
		// default rule: sparse iff its entries take fewer bytes than its dense row, so the genotype payload never
		// exceeds what pgh_open holds; max_minor > 0 overrides it (tests force either form)
		const bool sp = max_minor ? minor <= max_minor : 4ull * minor < win->pitch;
		part.off[i] = entries;
		if (sp) {
			part.row_of[i] = -1 - static_cast<int32_t>(major);
			entries += minor;
		} else {
			part.row_of[i] = static_cast<int32_t>(dense++);
		}
	}
	part.off[n] = entries;
	part.entries = entries;
	part.dense = dense;
	PGH_HIP(PghMalloc(&part.d_entries, sizeof(uint32_t) * std::max<uint64_t>(1, entries)), "hipMalloc(sparse entries)");
	PGH_HIP(PghMalloc(&part.d_pool, win->pitch * std::max<uint64_t>(1, dense)), "hipMalloc(sparse pool)");
	DevBuf d_row_of, d_off;
	HostSourceFence fence(st);
	PGH_HIP(d_row_of.Alloc(sizeof(int32_t) * n), "hipMalloc(sparse rows)");
	PGH_HIP(d_off.Alloc(sizeof(uint64_t) * (n + 1ull)), "hipMalloc(sparse offsets)");
	PGH_HIP(hipMemcpyAsync(d_row_of.p, part.row_of.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st),
	        "sparse rows upload");
	PGH_HIP(hipMemcpyAsync(d_off.p, part.off.data(), sizeof(uint64_t) * (n + 1ull), hipMemcpyHostToDevice, st),
	        "sparse offsets upload");
	PGH_HIP(pgh::LaunchSparseEmit(win->View(), n, d_row_of.As<int32_t>(), d_off.As<uint64_t>(), part.d_entries,
	                              part.d_pool, st),
	        "sparse emit kernel");
	PGH_HIP(hipStreamSynchronize(st), "sparse emit sync");
	return PGH_OK;
}

struct StreamGuard {
	hipStream_t st = nullptr;
	~StreamGuard() {
		if (st) {
			(void)hipStreamDestroy(st);
		}
	}
};

} // namespace

extern "C" uint64_t pgh_sparse_opens_started(void) {
	return g_sparse_opens.load();
}

extern "C" int pgh_open_sparse(const char *pgen_path, const char *pgi_path, uint32_t variant_begin,
                               uint32_t variant_end, uint32_t max_minor, pgh_dataset **out, char *errbuf) {
	if (!pgen_path || !out) {
		SetErr(errbuf, "null argument");
		return PGH_ERR_ARG;
	}
	*out = nullptr;
	std::unique_ptr<pgh_dataset> ds(new pgh_dataset());
	std::string err;
	if (!pgh::ParsePgenIndex(pgen_path, pgi_path ? pgi_path : "", ds->index, err)) {
		SetErr(errbuf, err);
		return err.find("cannot open") != std::string::npos ? PGH_ERR_OPEN : PGH_ERR_FORMAT;
	}
	const PgenIndex &ix = ds->index;
	if (variant_end == UINT32_MAX) {
		variant_end = ix.variant_ct;
	}
	if (variant_begin > variant_end || variant_end > ix.variant_ct) {
		SetErr(errbuf, "variant range out of bounds");
		return PGH_ERR_ARG;
	}
	if (ix.sample_ct >= (1u << 30)) {
		SetErr(errbuf, "pgh_open_sparse: an entry holds sample << 2, so the file must have fewer than 2^30 samples");
		return PGH_ERR_ARG;
	}
	g_sparse_opens.fetch_add(1);
	ds->has_file = true;
	ds->sparse = true;
	ds->pgen_path = pgen_path;
	ds->raw_variant_ct = ix.variant_ct;
	ds->sample_ct = ix.sample_ct;
	ds->record_bytes = ix.RecordBytes();
	ds->pitch = ChoosePitch(ds->record_bytes);
	ds->v_begin = variant_begin;
	ds->v_end = variant_end;
	PGH_HIP(hipGetDevice(&ds->device), "hipGetDevice");
	struct CloseOnFail { // whatever the dataset already holds goes back on every early return
		std::unique_ptr<pgh_dataset> &p;
		~CloseOnFail() {
			if (p) {
				pgh_close(p.release());
			}
		}
	} close_on_fail {ds};
	StreamGuard sg;
	PGH_HIP(hipStreamCreateWithFlags(&sg.st, hipStreamNonBlocking), "hipStreamCreate");
	const hipStream_t st = sg.st;

	std::vector<Part> parts;
	struct PartsGuard {
		std::vector<Part> &p;
		~PartsGuard() {
			for (auto &x : p) {
				x.Free();
			}
		}
	} parts_guard {parts};
	const uint32_t window = WindowRows(ds->pitch);
	for (uint32_t w0 = variant_begin; w0 < variant_end;) {
		const uint32_t w1 = static_cast<uint32_t>(std::min<uint64_t>(variant_end, static_cast<uint64_t>(w0) + window));
		pgh_dataset *win = nullptr;
		int rc = PghOpenRows(pgen_path, pgi_path, w0, w1, true, &win, errbuf);
		if (rc != PGH_OK) {
			return rc;
		}
		parts.emplace_back();
		rc = CompactWindow(win, max_minor, st, parts.back(), errbuf);
		pgh_close(win);
		if (rc != PGH_OK) {
			return rc;
		}
		w0 = w1;
	}

	// concatenate: pool rows and entry offsets shift by what the windows before hold
	const uint32_t rows = variant_end - variant_begin;
	uint64_t entries = 0;
	uint32_t dense = 0;
	for (const auto &p : parts) {
		entries += p.entries;
		dense += p.dense;
	}
	std::vector<int32_t> row_of(rows);
	std::vector<uint64_t> off(static_cast<size_t>(rows) + 1);
	ds->sp_dense_before.assign(static_cast<size_t>(rows) + 1, 0);
	HostSourceFence fence(st); // row_of / off feed asynchronous uploads
	PGH_HIP(PghMalloc(&ds->d_sp_entries, sizeof(uint32_t) * std::max<uint64_t>(1, entries)), "hipMalloc(sparse entries)");
	PGH_HIP(PghMalloc(&ds->d_sp_pool, ds->pitch * std::max<uint64_t>(1, dense)), "hipMalloc(sparse pool)");
	PGH_HIP(PghMalloc(&ds->d_sp_row_of, sizeof(int32_t) * std::max<uint32_t>(1, rows)), "hipMalloc(sparse rows)");
	PGH_HIP(PghMalloc(&ds->d_sp_off, sizeof(uint64_t) * (rows + 1ull)), "hipMalloc(sparse offsets)");
	uint32_t at = 0, dense_at = 0;
	uint64_t entry_at = 0;
	for (auto &p : parts) {
		uint32_t k = 0; // dense rows of this window before row i
		for (uint32_t i = 0; i < p.rows; i++) {
			const int32_t ro = p.row_of[i];
			row_of[at + i] = ro >= 0 ? ro + static_cast<int32_t>(dense_at) : ro;
			off[at + i] = p.off[i] + entry_at;
			ds->sp_dense_before[at + i] = dense_at + k;
			if (ro >= 0) {
				k++;
			} else {
				ds->sp_base_hist[-1 - ro]++;
			}
		}
		if (p.entries) {
			PGH_HIP(hipMemcpyAsync(ds->d_sp_entries + entry_at, p.d_entries, sizeof(uint32_t) * p.entries,
			                       hipMemcpyDeviceToDevice, st),
			        "sparse entries concatenation");
		}
		if (p.dense) {
			PGH_HIP(hipMemcpyAsync(ds->d_sp_pool + static_cast<uint64_t>(dense_at) * ds->pitch, p.d_pool,
			                       ds->pitch * p.dense, hipMemcpyDeviceToDevice, st),
			        "sparse pool concatenation");
		}
		at += p.rows;
		dense_at += p.dense;
		entry_at += p.entries;
		PGH_HIP(hipStreamSynchronize(st), "sparse concatenation sync");
		p.Free();
	}
	off[rows] = entries;
	ds->sp_dense_before[rows] = dense;
	if (rows) {
		PGH_HIP(hipMemcpyAsync(ds->d_sp_row_of, row_of.data(), sizeof(int32_t) * rows, hipMemcpyHostToDevice, st),
		        "sparse rows upload");
	}
	PGH_HIP(hipMemcpyAsync(ds->d_sp_off, off.data(), sizeof(uint64_t) * (rows + 1ull), hipMemcpyHostToDevice, st),
	        "sparse offsets upload");
	PGH_HIP(hipStreamSynchronize(st), "sparse upload sync");
	ds->sp_entry_ct = entries;
	ds->sp_dense_rows = dense;
	ds->sp_sparse_rows = rows - dense;
	*out = ds.release();
	return PGH_OK;
}

extern "C" int pgh_get_sparse_info(const pgh_dataset *ds, pgh_sparse_info *out) {
	if (!ds || !out || !ds->sparse) {
		return PGH_ERR_ARG;
	}
	std::memset(out, 0, sizeof *out);
	const uint64_t rows = ds->v_end - ds->v_begin;
	out->sparse_variant_ct = ds->sp_sparse_rows;
	out->dense_variant_ct = ds->sp_dense_rows;
	out->entry_ct = ds->sp_entry_ct;
	// entries + pool + the per-variant index (row_of int32, offset uint64)
	out->resident_bytes = 4 * ds->sp_entry_ct + ds->pitch * ds->sp_dense_rows + 12 * rows + 8;
	out->dense_bytes = ds->pitch * rows;
	for (int k = 0; k < 4; k++) {
		out->base_hist[k] = ds->sp_base_hist[k];
	}
	return PGH_OK;
}

namespace pgh_sparse {

void Free(pgh_dataset *ds) {
	for (void *p : {static_cast<void *>(ds->d_sp_row_of), static_cast<void *>(ds->d_sp_off),
	                static_cast<void *>(ds->d_sp_entries), static_cast<void *>(ds->d_sp_pool)}) {
		if (p) {
			(void)hipFree(p);
		}
	}
	ds->d_sp_row_of = nullptr;
	ds->d_sp_off = nullptr;
	ds->d_sp_entries = nullptr;
	ds->d_sp_pool = nullptr;
}

int CountsRangeDev(const pgh_dataset *ds, const pgh_subset *ss, uint32_t v_begin, uint32_t v_end, void *d_out,
                   hipStream_t st, char *errbuf) {
	const uint32_t n = v_end - v_begin;
	if (n == 0) {
		return PGH_OK;
	}
	const uint32_t l0 = v_begin - ds->v_begin, l1 = v_end - ds->v_begin;
	// the range's dense rows are consecutive pool rows: one ordinary counts launch over them
	const uint32_t dense_first = ds->sp_dense_before[l0];
	const uint32_t dense_ct = ds->sp_dense_before[l1] - dense_first;
	const uint32_t n_out = ss ? ss->n_out : ds->sample_ct;
	void *scratch = nullptr;
	if (dense_ct) {
		PGH_HIP(PghThreadScratch(16ull * dense_ct, st, &scratch), "sparse counts scratch");
		PGH_HIP(pgh::LaunchCounts(ds->PoolView(), dense_first, nullptr, dense_ct, ss ? ss->d_mask2 : nullptr, n_out,
		                          static_cast<uint32_t *>(scratch), st),
		        "counts kernel (dense pool)");
	}
	PGH_HIP(pgh::LaunchSparseCounts(ds->Sparse(), l0, n, ss ? ss->d_include : nullptr, n_out,
	                                static_cast<const uint32_t *>(scratch), dense_first, static_cast<uint32_t *>(d_out),
	                                st),
	        "sparse counts kernel");
	return PGH_OK;
}

int SampleClasses(const pgh_dataset *ds, uint32_t v_first, const uint32_t *vlist, const uint32_t *h_vlist,
                  uint32_t n_var, uint32_t *d_classes, uint32_t out_stride, hipStream_t st, bool scratch_from_thread,
                  char *errbuf) {
	// the dense rows: LaunchClassCounts3 over their pool rows (it also zeroes / overwrites d_classes); a range's
	// dense rows are consecutive pool rows, a list's are listed
	std::vector<uint32_t> pool_list;
	uint32_t dense_first = 0, dense_ct = 0;
	if (vlist) {
		for (uint32_t i = 0; i < n_var; i++) {
			const uint32_t r = h_vlist[i];
			if (ds->sp_dense_before[r + 1] != ds->sp_dense_before[r]) {
				pool_list.push_back(ds->sp_dense_before[r]);
			}
		}
		dense_ct = static_cast<uint32_t>(pool_list.size());
	} else {
		dense_first = ds->sp_dense_before[v_first];
		dense_ct = ds->sp_dense_before[v_first + n_var] - dense_first;
	}
	const size_t cols_bytes = pgh::ClassCounts3ScratchBytes(ds->record_bytes);
	const size_t list_at = (cols_bytes + 255) / 256 * 256;
	const size_t need = list_at + sizeof(uint32_t) * pool_list.size();
	DevBuf own;
	void *scratch = nullptr;
	if (scratch_from_thread) {
		PGH_HIP(PghThreadScratch(need, st, &scratch), "sample counts scratch");
	} else {
		PGH_HIP(own.Alloc(need), "hipMalloc(sample counts)");
		scratch = own.p;
	}
	HostSourceFence fence(st); // pool_list feeds an asynchronous upload
	uint32_t *d_pool_list = nullptr;
	if (!pool_list.empty()) {
		d_pool_list = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(scratch) + list_at);
		PGH_HIP(hipMemcpyAsync(d_pool_list, pool_list.data(), sizeof(uint32_t) * pool_list.size(), hipMemcpyHostToDevice,
		                       st),
		        "sample counts upload");
	}
	PGH_HIP(pgh::LaunchClassCounts3(ds->PoolView(), dense_first, d_pool_list, dense_ct, static_cast<uint8_t *>(scratch),
	                                d_classes, out_stride, st),
	        "sample counts kernel (dense pool)");
	const uint64_t rows = std::max<uint64_t>(1, ds->v_end - ds->v_begin);
	const uint64_t entries_hint = ds->sp_entry_ct * n_var / rows;
	PGH_HIP(pgh::LaunchSparseSampleClasses(ds->Sparse(), v_first, vlist, n_var, entries_hint, d_classes, out_stride, st),
	        "sparse sample counts kernel");
	return PGH_OK;
}

int CopyRowsToHost(const pgh_dataset *ds, uint32_t v_begin, uint32_t v_end, uint8_t *rows, size_t row_stride,
                   char *errbuf) {
	PGH_ENTER(ds);
	hipStream_t st = PghThreadStream();
	const uint32_t chunk = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(v_end - v_begin, (256ull << 20) / ds->pitch)));
	DevBuf buf;
	PGH_HIP(buf.Alloc(ds->pitch * chunk), "hipMalloc(expanded rows)");
	for (uint32_t v = v_begin; v < v_end; v += chunk) {
		const uint32_t n = std::min<uint32_t>(chunk, v_end - v);
		PGH_HIP(hipMemsetAsync(buf.p, 0, ds->pitch * n, st), "expanded rows clear");
		PGH_HIP(pgh::LaunchSparseExpand(ds->Sparse(), v - ds->v_begin, n, buf.As<uint8_t>(), ds->pitch, st),
		        "sparse expand kernel");
		PGH_HIP(hipMemcpy2DAsync(rows + static_cast<uint64_t>(v - v_begin) * row_stride, row_stride, buf.p, ds->pitch,
		                         ds->record_bytes, n, hipMemcpyDeviceToHost, st),
		        "row download");
		PGH_HIP(hipStreamSynchronize(st), "row download sync");
	}
	return PGH_OK;
}

} // namespace pgh_sparse

namespace {

// PGH_SCORE_SPARSE_SLICES (read at every call): the row slices per sample tile of pgh_score_sparse's walks, 0 or unset
// = chosen from the list's entries.  The result does not depend on it.
uint32_t ScoreSparseSlices() {
	const char *s = std::getenv("PGH_SCORE_SPARSE_SLICES");
	if (s && *s) {
		char *end = nullptr;
		const unsigned long v = std::strtoul(s, &end, 10);
		if (end && *end == '\0') {
			return static_cast<uint32_t>(std::min<unsigned long>(v, 65535));
		}
	}
	return 0;
}

// pgh_score_sparse on one sparse-resident dataset, after the argument checks (n_scored >= 1); local: the rows scored.
int ScoreSparseOne(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_scored, const uint32_t *local,
                   const double *weights, const uint8_t *flip, uint32_t n_cols, int mode, double *score_sum,
                   double *dosage_sum, uint32_t *allele_ct, char *errbuf) {
	PGH_ENTER(ds);
	const uint32_t N = ds->sample_ct;
	hipStream_t st = PghThreadStream();
	uint32_t l_min = UINT32_MAX, l_max = 0;
	uint64_t dense_listed = 0;
	for (uint32_t i = 0; i < n_scored; i++) {
		const uint32_t l = local[i];
		l_min = std::min(l_min, l);
		l_max = std::max(l_max, l);
		dense_listed += ds->sp_dense_before[l + 1] - ds->sp_dense_before[l];
	}
	const uint32_t span = l_max - l_min + 1;
	const uint64_t rows = std::max<uint64_t>(1, ds->v_end - ds->v_begin);
	const uint64_t entries_hint = ds->sp_entry_ct * n_scored / rows + dense_listed * (N / 4);
	// CENTER keeps no dosage sum (its td tables are zero): the output is 0.0, as pgh_score's
	const bool track = dosage_sum && mode != PGH_SCORE_CENTER;

	DevBuf d_score, d_dos, d_alc, work;
	PGH_HIP(d_score.Alloc(8ull * N * n_cols), "hipMalloc(score_sparse out)");
	if (track) {
		PGH_HIP(d_dos.Alloc(8ull * N), "hipMalloc(score_sparse out)");
	}
	PGH_HIP(d_alc.Alloc(4ull * N), "hipMalloc(score_sparse out)");
	const uint64_t ns = n_scored, nc1 = n_cols + 1ull, alc0_bytes = 256;
	uint32_t *d_vlist, *d_range, *d_counts, *d_ac, *d_alc0;
	double *d_w, *d_ts, *d_td, *d_part, *d_k0;
	uint8_t *d_flip;
	int32_t *d_kexp;
	ScratchLayout lay;
	lay.Add(&d_vlist, ns);
	lay.Add(&d_w, ns * n_cols);
	lay.Add(&d_flip, ns, flip != nullptr);
	lay.Add(&d_range, 4ull * span);
	lay.Add(&d_counts, 4 * ns);
	lay.Add(&d_ts, 4 * ns);
	lay.Add(&d_td, 4 * ns);
	lay.Add(&d_ac, ns);
	lay.Add(&d_part, 2 * nc1 * pgh::kScoreSparseParts);
	lay.Add(&d_k0, nc1);
	lay.Add(&d_kexp, nc1);
	lay.Add(&d_alc0, alc0_bytes / 4);
	// (not PghThreadScratch: CountsRangeDev below takes that block for the dense rows' counts)
	PGH_HIP(work.Alloc(lay.total), "hipMalloc(score_sparse)");
	lay.Bind(work.p);

	std::vector<double> h_score(static_cast<size_t>(N) * n_cols), h_dos(track ? N : 0);
	std::vector<uint32_t> h_ac(N);
	HostSourceFence fence(st); // local and the caller's arrays feed asynchronous uploads, the three above take downloads
	PGH_HIP(hipMemcpyAsync(d_vlist, local, 4ull * n_scored, hipMemcpyHostToDevice, st), "score_sparse upload");
	PGH_HIP(hipMemcpyAsync(d_w, weights, 8ull * n_scored * n_cols, hipMemcpyHostToDevice, st), "score_sparse upload");
	if (flip) {
		PGH_HIP(hipMemcpyAsync(d_flip, flip, n_scored, hipMemcpyHostToDevice, st), "score_sparse upload");
	}
	PGH_HIP(hipMemsetAsync(d_score.p, 0, 8ull * N * n_cols, st), "score_sparse clear");
	if (track) {
		PGH_HIP(hipMemsetAsync(d_dos.p, 0, 8ull * N, st), "score_sparse clear");
	}
	PGH_HIP(hipMemsetAsync(d_alc.p, 0, 4ull * N, st), "score_sparse clear");
	// the subset's counts of the rows the list spans, the listed ones picked out, and the reference's tables from them
	const int rc = pgh_sparse::CountsRangeDev(ds, subset, ds->v_begin + l_min, ds->v_begin + l_min + span, d_range, st,
	                                          errbuf);
	if (rc != PGH_OK) {
		return rc;
	}
	PGH_HIP(pgh::LaunchScoreSparseGather(d_range, d_vlist, l_min, n_scored, d_counts, st), "score_sparse gather kernel");
	PGH_HIP(pgh::LaunchScoreTables(d_counts, d_flip, n_scored, mode, d_ts, d_td, d_ac, st), "score table kernel");
	PGH_HIP(pgh::LaunchScoreSparseStats(ds->Sparse(), d_vlist, n_scored, d_w, n_cols, d_ts, d_td, d_ac, d_part, d_k0,
	                                    d_kexp, d_alc0, st),
	        "score_sparse column kernels");
	const uint32_t slices = ScoreSparseSlices();
	for (uint32_t c0 = 0; c0 < n_cols; c0 += pgh::kScoreSparseChunk) {
		const bool first = c0 == 0;
		PGH_HIP(pgh::LaunchScoreSparse(ds->Sparse(), subset ? subset->d_include : nullptr, d_vlist, n_scored, d_w, n_cols,
		                               c0, std::min(pgh::kScoreSparseChunk, n_cols - c0), d_ts, d_td, d_ac, d_kexp,
		                               entries_hint, slices, d_score.As<unsigned long long>(),
		                               first && track ? d_dos.As<unsigned long long>() : nullptr,
		                               first ? d_alc.As<uint32_t>() : nullptr, st),
		        "score_sparse entry kernel");
	}
	PGH_HIP(pgh::LaunchScoreSparseFlush(N, n_cols, d_k0, d_kexp, d_alc0, d_score.As<unsigned long long>(),
	                                    track ? d_dos.As<unsigned long long>() : nullptr, d_alc.As<uint32_t>(), st),
	        "score_sparse flush kernels");
	PGH_HIP(hipMemcpyAsync(h_score.data(), d_score.p, 8ull * N * n_cols, hipMemcpyDeviceToHost, st), "score_sparse copy");
	if (track) {
		PGH_HIP(hipMemcpyAsync(h_dos.data(), d_dos.p, 8ull * N, hipMemcpyDeviceToHost, st), "score_sparse copy");
	}
	PGH_HIP(hipMemcpyAsync(h_ac.data(), d_alc.p, 4ull * N, hipMemcpyDeviceToHost, st), "score_sparse copy");
	PGH_HIP(hipStreamSynchronize(st), "score_sparse sync");
	Compact<double>(subset, h_score.data(), n_cols, score_sum, N);
	if (track) {
		Compact<double>(subset, h_dos.data(), 1, dosage_sum, N);
	} else if (dosage_sum) {
		std::fill_n(dosage_sum, subset ? subset->n_out : N, 0.0);
	}
	Compact<uint32_t>(subset, h_ac.data(), 1, allele_ct, N);
	return PGH_OK;
}

} // namespace

extern "C" int pgh_score_sparse(const pgh_dataset *ds, const pgh_subset *subset, uint32_t n_scored, const uint32_t *vidx,
                                const double *weights, const uint8_t *flip, uint32_t n_cols, int mode, double *score_sum,
                                double *dosage_sum, uint32_t *allele_ct, char *errbuf) {
	if (!ds) {
		SetErr(errbuf, "null dataset");
		return PGH_ERR_ARG;
	}
	PGH_ONE_DEVICE(ds);
	PGH_SPARSE_ROWS(ds);
	if (!score_sum || !allele_ct || (n_scored && (!vidx || !weights))) {
		SetErr(errbuf, "null argument");
		return PGH_ERR_ARG;
	}
	if (mode < 0 || mode > 2) {
		SetErr(errbuf, "unknown score mode");
		return PGH_ERR_ARG;
	}
	if (n_cols == 0 || n_cols > 4096) {
		SetErr(errbuf, "n_cols must be between 1 and 4096");
		return PGH_ERR_ARG;
	}
	VariantRows rows; // host list only: it goes up with the call's other arrays, behind ScoreSparseOne's fence
	int rc = CheckSubset(ds, subset, errbuf);
	if (rc == PGH_OK) {
		rc = rows.Resolve(ds, 0, n_scored, vidx, pgh::kVariantRowsListOnly, errbuf);
	}
	if (rc != PGH_OK) {
		return rc;
	}
	const size_t total = static_cast<size_t>(n_scored) * n_cols;
	for (size_t j = 0; j < total; j++) {
		if (!std::isfinite(weights[j])) {
			SetErr(errbuf, "non-finite weight at variant " + std::to_string(j / n_cols) + ", column " +
			                   std::to_string(j % n_cols) + ": pgh_score_sparse accumulates in fixed point");
			return PGH_ERR_ARG;
		}
	}
	const uint32_t n_out = subset ? subset->n_out : ds->sample_ct;
	if (n_scored == 0 || n_out == 0) { // pgh_score's answer for an empty list; nothing to write for an empty subset
		std::fill_n(score_sum, static_cast<size_t>(n_out) * n_cols, 0.0);
		if (dosage_sum) {
			std::fill_n(dosage_sum, n_out, 0.0);
		}
		std::fill_n(allele_ct, n_out, 0u);
		return PGH_OK;
	}
	return ScoreSparseOne(ds, subset, n_scored, rows.local.data(), weights, flip, n_cols, mode, score_sum, dosage_sum,
	                      allele_ct, errbuf);
}
