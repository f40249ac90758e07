// glm_team.hpp -- the device code the GLM kernels share: a team's barrier, the ordered-list step (rank, write, walk),
// the team reduction, the packed-upper decode, and the walk of a sparse row's entries that GlmSparseKernel
// (glm_sparse.hip) and GlmScoreSparseKernel (glm_score_sparse.hip) instantiate with their arithmetic.
//
// A team is one wave (TEAM == 64) or the whole 256-thread workgroup (TEAM == 256).  Everything here is called by
// every thread of the team under team-uniform control flow: each function that says so holds a barrier.
#pragma once

#include "device_utils.hpp"
#include "glm.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pgh {

namespace {

constexpr int kTeamBlock = 256;
constexpr int kTeamWaves = kTeamBlock / 64;
// (k + 2)(k + 3) / 2 at k = PGH_GLM_MAX_COVAR: the most entries the owners of one list share
constexpr int kTeamMaxOwned = 253;

// Orders a team's LDS writes before its LDS reads.  A wave's LDS instructions complete in issue order, so a team of
// one wave only has to keep the compiler from moving them.
template <int TEAM>
__device__ __forceinline__ void TeamSync() {
	if constexpr (TEAM == kTeamBlock) {
		__syncthreads();
	} else {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
}

// Entry e of the packed row-major upper triangle of order q -> (a, b), a <= b < q.  e < q (q + 1) / 2.
__device__ __forceinline__ void PackedUpper(int e, int q, int *a, int *b) {
	int row = 0;
	while (e >= q - row) {
		e -= q - row;
		row++;
	}
	*a = row;
	*b = row + e;
}

// The score test's owned entries (glm_score_sparse.hip, glm_score_dense.hip).  Entry e of the packed set {H: sum w
// Zt_a Zt_b (a <= b <= k, row-major upper), then g: sum r Zt_a (a <= k)} as columns of a list row [Zt_0..Zt_k, w, r]:
// its term is row[ew] * row[ea] * row[eb] (eb = 0, the 1.0, for g).  ea < 0: there is no such entry.
__device__ __forceinline__ void ScoreOwnedEntry(int e, int k, int *ea, int *eb, int *ew) {
	const int q1 = k + 1, nh = q1 * (q1 + 1) / 2;
	*ea = *eb = *ew = -1;
	if (e < nh) {
		PackedUpper(e, q1, ea, eb);
		*ew = k + 1;
	} else if (e < nh + q1) {
		*ea = e - nh;
		*eb = 0;
		*ew = k + 2;
	}
}

// The ordered-list step, part one.  Returns how many threads before this one in thread order have `take` set, and in
// *total how many of the team have: the takers' ranks are 0 .. *total - 1 in thread order, and *total is the same on
// every thread, so code under `if (*total)` is team-uniform and may hold a barrier.
//
// How a caller uses it, once per step of its loop over the samples or entries:
//   rank = TeamRank(take, ..., &total);  if (take) write list row `rank`;  TeamSync;  every owner walks rows
//   0 .. total - 1 in order;  TeamSync.
// The first TeamSync puts the rows before their readers.  The second keeps the next step from rewriting the list under
// a thread that still walks it; it also stands between this call's reads of wave_ct and the next call's writes, which
// is why a caller that skips the walk when total == 0 still runs the second one.
template <int TEAM>
__device__ __forceinline__ uint32_t TeamRank(bool take, int lane, int wave, uint32_t *total) {
	const uint64_t bal = __ballot(take);
	uint32_t before = 0;
	*total = static_cast<uint32_t>(__popcll(bal));
	if constexpr (TEAM == kTeamBlock) {
		__shared__ uint32_t wave_ct[kTeamWaves];
		if (lane == 0) {
			wave_ct[wave] = *total;
		}
		__syncthreads();
		*total = 0;
		for (int w = 0; w < kTeamWaves; w++) {
			before += w < wave ? wave_ct[w] : 0u;
			*total += wave_ct[w];
		}
	}
	return before + static_cast<uint32_t>(__popcll(bal & ((1ull << lane) - 1ull)));
}

// TeamRank for a workgroup whose threads each bring a count, not a bool.  Returns how many selected items the threads
// before this one in thread order hold, and in *total the workgroup's sum, the same on every thread: an inclusive
// __shfl_up scan of the counts per wave, then the waves' totals from LDS.  step: the number of the caller's step, 0,
// 1, 2, ...  The totals sit in wave_ct[step & 1], so a step's readers never meet the next step's writers: between a
// thread's reads of step s and any thread's writes of step s + 2 stands the barrier of step s + 1, and one barrier a
// step is enough.  Every thread of the workgroup calls it, under workgroup-uniform control flow.
__device__ __forceinline__ uint32_t TeamRankCounts(uint32_t cnt, uint32_t step, int lane, int wave, uint32_t *total) {
	__shared__ uint32_t wave_ct[2][kTeamWaves];
	uint32_t incl = cnt;
#pragma unroll
	for (uint32_t off = 1; off < 64u; off <<= 1) {
		const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), off, 64));
		incl += static_cast<uint32_t>(lane) >= off ? up : 0u;
	}
	if (lane == 63) {
		wave_ct[step & 1u][wave] = incl;
	}
	__syncthreads();
	uint32_t before = incl - cnt;
	*total = 0;
	for (int w = 0; w < kTeamWaves; w++) {
		before += w < wave ? wave_ct[step & 1u][w] : 0u;
		*total += wave_ct[step & 1u][w];
	}
	return before;
}

// Team totals of N doubles and four integer counts, on every thread: a butterfly per wave, then (TEAM == 256) the
// waves' partials added in the order 0..3 from LDS.  One barrier, between the partials' writes and their reads: a
// caller that calls it again (GlmScoreSpaKernel does, once per evaluation) puts a TeamSync between the calls, or the
// next call's writes race this call's reads.
template <int TEAM, int N>
__device__ __forceinline__ void TeamSums(double (&v)[N], long long (&c)[4], int lane, int wave) {
#pragma unroll
	for (int j = 0; j < N; j++) {
		v[j] = WaveSum(v[j]);
	}
#pragma unroll
	for (int j = 0; j < 4; j++) {
		c[j] = WaveSum(c[j]);
	}
	if constexpr (TEAM == kTeamBlock) {
		__shared__ double part[kTeamWaves][N];
		__shared__ long long ipart[kTeamWaves][4];
		if (lane == 0) {
#pragma unroll
			for (int j = 0; j < N; j++) {
				part[wave][j] = v[j];
			}
#pragma unroll
			for (int j = 0; j < 4; j++) {
				ipart[wave][j] = c[j];
			}
		}
		__syncthreads();
#pragma unroll
		for (int j = 0; j < N; j++) {
			v[j] = part[0][j];
		}
#pragma unroll
		for (int j = 0; j < 4; j++) {
			c[j] = ipart[0][j];
		}
		for (int w = 1; w < kTeamWaves; w++) {
#pragma unroll
			for (int j = 0; j < N; j++) {
				v[j] += part[w][j];
			}
#pragma unroll
			for (int j = 0; j < 4; j++) {
				c[j] += ipart[w][j];
			}
		}
	}
}

// The bounded grid of the workgroup-form kernels whose workgroups own a stash: workgroup g takes the rows g,
// g + gridDim.x, ... of n_rows, and a barrier after each, because the next row rewrites the stash.
template <class Row>
__device__ __forceinline__ void TeamGridRows(uint32_t n_rows, Row row) {
	for (uint32_t at = blockIdx.x; at < n_rows; at += gridDim.x) {
		row(at);
		__syncthreads();
	}
}

// What the follow-up kernels of the dense score route (glm_score_dense_spa.hip, glm_score_dense_firth.hip) read of a
// chunk of a phenotype block: row at = p * nv + v is block phenotype p and chunk variant v.
struct DenseRows {
	const uint8_t *rows; // the resident rows
	uint64_t pitch;
	uint32_t v0, nv;     // the chunk: local rows v0 .. v0 + nv - 1
	uint32_t sample_ct;
	uint32_t mask_words; // 16-code words of a row and of a phenotype's mask (zero past the last sample)
	const uint32_t *mask;
	uint32_t pb;
	const double *b; // the column block
	uint32_t ld, k;

	__device__ const uint32_t *Row(uint32_t v) const {
		return reinterpret_cast<const uint32_t *>(rows + static_cast<uint64_t>(v0 + v) * pitch);
	}
	__device__ const uint32_t *Mask(uint32_t p) const {
		return mask + static_cast<uint64_t>(p) * mask_words;
	}
};

// The checks the two launch wrappers share and the fields of DenseRows.  hipSuccess with *grid == 0: an empty chunk,
// nothing to launch.  Otherwise *grid workgroups (n_groups at most, one per row at most) each own a stash.
inline hipError_t DenseRowsFor(const RowView &view, uint32_t v0, uint32_t nv, const uint32_t *mask, uint32_t pb,
                               const double *b, uint32_t k, uint32_t n_groups, DenseRows *a, uint32_t *grid) {
	*grid = 0;
	if (k > PGH_GLM_MAX_COVAR || pb == 0 || pb > kGlmScoreDensePb) {
		return hipErrorInvalidValue;
	}
	if (nv == 0) {
		return hipSuccess;
	}
	const uint32_t words16 = (view.sample_ct + 63u) / 64u;
	if (n_groups == 0 || 16ull * words16 > view.pitch) {
		return hipErrorInvalidValue; // the kernels read whole 16-code words of a row up to the mask's length
	}
	*a = {view.rows, view.pitch, v0, nv, view.sample_ct, 4u * words16, mask, pb, b, GlmScoreDenseLayout(pb, k).ld, k};
	const uint64_t n_rows = static_cast<uint64_t>(nv) * pb;
	*grid = static_cast<uint32_t>(n_groups < n_rows ? n_groups : n_rows);
	return hipSuccess;
}

// Phase A of those kernels: the walk of one 2-bit row under one phenotype's mask by the workgroup, a 16-code word per
// thread and 4,096 samples a step.  select(c, m) -> em, bit 2 i set where sample 16 wi + i of the word is selected;
// the selected samples are ranked in sample order (TeamRankCounts over the words' popcounts, then bit order inside a
// word), and entry(s, code) -> the double2 that goes to st[rank] when rank < cap.  Returns the number selected, on
// every thread; the caller tests it against cap.
//
// The contract is the order: a thread visits its entries by ascending word and, inside a word, ascending bit, and
// calls entry once for each, so a sum that entry keeps with one fma per call is one chain per thread in that order.
// The caller reduces it with TeamSums and then runs TeamSync (the pairs before their readers, and TeamSums' LDS before
// it is written again).  That order of summation is the result, bit for bit: do not reorder the visits.
template <class Select, class Entry>
__device__ __forceinline__ uint32_t TeamStashMaskedRow(const uint32_t *row, const uint32_t *m, uint32_t mask_words,
                                                       double2 *__restrict__ st, uint32_t cap, int tid, int lane,
                                                       int wave, Select select, Entry entry) {
	uint32_t count = 0;
	for (uint32_t w0 = 0, step = 0; w0 < mask_words; w0 += kTeamBlock, step++) {
		const uint32_t wi = w0 + tid;
		uint32_t c = 0, em = 0;
		if (wi < mask_words) {
			c = row[wi];
			em = select(c, m[wi]);
		}
		uint32_t total;
		uint32_t pos = count + TeamRankCounts(static_cast<uint32_t>(__popc(em)), step, lane, wave, &total);
		while (em) {
			const uint32_t i = static_cast<uint32_t>(__ffs(static_cast<int>(em)) - 1) >> 1;
			em &= em - 1u;
			const double2 pair = entry(16u * wi + i, (c >> (2u * i)) & 3u);
			if (pos < cap) {
				st[pos] = pair;
			}
			pos++;
		}
		count += total;
	}
	return count;
}

// TeamStashMaskedRow for a row of 16-bit values on the 2^-14 grid (glm_score_dense_dosage.hip's u16 row: 16 values per
// mask word, 0xFFFF for neither a dosage nor a call), with the same geometry on purpose: a 16-sample word per thread,
// 4,096 samples a step, TeamRankCounts over the words' popcounts, ascending sample order inside a word.  A thread loads
// its word's 32 bytes as two 16-byte loads (row is 16-byte aligned and holds 16 mask_words values) and one mask word.
// Sample i of the word is selected when its mask bit (bit 2 i) is set and its value is neither 0xFFFF nor `base`;
// entry(s, v) -> the double2 that goes to st[rank] when rank < cap.  Returns the number selected, on every thread.
//
// The contract is TeamStashMaskedRow's, the order: for a row whose values restate 2-bit codes (v = code << 14) and the
// selection that goes with it, the visits, the ranks and so a caller's fma chains are that walk's, bit for bit.
template <class Entry>
__device__ __forceinline__ uint32_t TeamStashMaskedU16Row(const uint16_t *row, const uint32_t *m, uint32_t mask_words,
                                                          uint32_t base, double2 *__restrict__ st, uint32_t cap, int tid,
                                                          int lane, int wave, Entry entry) {
	const uint4 *row4 = reinterpret_cast<const uint4 *>(row);
	uint32_t count = 0;
	for (uint32_t w0 = 0, step = 0; w0 < mask_words; w0 += kTeamBlock, step++) {
		const uint32_t wi = w0 + tid;
		uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
		uint32_t em = 0; // bit i: sample 16 wi + i is selected
		if (wi < mask_words) {
			lo = row4[2u * wi];
			hi = row4[2u * wi + 1u];
			const uint32_t mm = m[wi];
			const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
			for (uint32_t i = 0; i < 16u; i++) {
				// bit 16 of x + 0xffff says whether the 16-bit x is not 0: integer arithmetic, because sixteen
				// comparisons in flight hold sixteen pairs of scalar registers, more than there are to spare
				const uint32_t v = (d[i >> 1] >> (16u * (i & 1u))) & 0xffffu;
				const uint32_t keep = (((v ^ 0xffffu) + 0xffffu) & ((v ^ base) + 0xffffu)) >> 16;
				em |= (keep & (mm >> (2u * i)) & 1u) << i;
			}
		}
		uint32_t total;
		uint32_t pos = count + TeamRankCounts(static_cast<uint32_t>(__popc(em)), step, lane, wave, &total);
		while (em) {
			const uint32_t i = static_cast<uint32_t>(__ffs(static_cast<int>(em)) - 1);
			em &= em - 1u;
			// (a chain of selects, not an indexed array, which would live in scratch memory)
			const uint32_t h = i >> 1;
			const uint32_t a = h & 1u ? lo.y : lo.x, b = h & 1u ? lo.w : lo.z, c = h & 1u ? hi.y : hi.x,
			               e = h & 1u ? hi.w : hi.z;
			const uint32_t pair2 = h & 4u ? (h & 2u ? e : c) : (h & 2u ? b : a);
			const double2 pair = entry(16u * wi + i, (pair2 >> (16u * (i & 1u))) & 0xffffu);
			if (pos < cap) {
				st[pos] = pair;
			}
			pos++;
		}
		count += total;
	}
	return count;
}

// The rows of a sparse-resident dataset (SparseView's arrays) that one launch of an entry kernel covers.
struct SparseRows {
	const int32_t *row_of;
	const uint64_t *off;
	const uint32_t *entries;
	const uint8_t *pool; // read only by a Model that walks dense-form rows
	uint64_t pitch;
	uint32_t sample_ct, v_first, nv;
};

// The walk of one row by one team.  TEAM == 64: a wave per row, four rows per workgroup, the sparse rows of at most
// kGlmSparseLong entries.  TEAM == 256: a workgroup per row, the longer sparse rows and (Model::kWalksDense) the rows
// held in the dense form, walked from their pool row, one sample per lane per step, as base-0 rows whose entries are
// the samples with a code other than 0.  The two launches cover the same rows and each returns from the other's.
//
// A row is a base code b and the entries that differ from it.  Of the entries that are used (sample below sample_ct,
// m.Load says its staged value is a number), M are those with code 3 and C the others.  The walk leaves
//   n = n_y - |M|, sum x = b n + sum_C (x - b), sum x^2 = b^2 n + sum_C (x^2 - b^2)   (b == 3: n = |C|, sums over C)
// in sums[i][0..2], integers until they are stored; the Model's NL lane sums over C, one fma chain per lane and then
// TeamSums; and per entry of the Model's packed set the sum of m.Term over the list set (M, or C when b == 3) in entry
// order, by the one thread that owns the entry.  m.Epilogue stores them.  z: the kp = KP doubles of a sample's
// covariates at z[s * KP], raw-sample order.  lds: 256 list rows [1, z_1..z_k, Model's tail] of q = k + 1 + Model::kTail
// doubles.
//
// A Model supplies
//   kNS, kNL, kTail, kWalksDense;  double *sums (rows of kNS);
//   Sample: what Load(s, &v) reads of sample s (false: the sample is not used);
//   Add(dd, v, zi, ls): a called entry's d = x - b joins the lane sums;  Tail(v, row + k + 1): the list row past z;
//   Own, OwnedEntry(e, k), Term(list, row, own): an owner's entry (own.a < 0: there is no entry e) and its term of the
//   list row that starts at list[row];
//   Zero(i, tid, k) unless kWalksDense: the result row of a dense-form row, by a wave;
//   Epilogue<TEAM>(i, tid, k, base3, bx, ls, own, acc): the rest of sums[i] and the owned sums; thread tid owns the
//   entries tid + t * TEAM, acc[t] is the sum of entry own[t].
template <class Model, int KP, int TEAM>
__device__ __forceinline__ void TeamWalkSparseRow(const SparseRows &rows, const double *__restrict__ z, uint32_t k,
                                                  uint32_t n_y, const Model &m, double *lds) {
	constexpr int NOWN = (kTeamMaxOwned + TEAM - 1) / TEAM; // entries a thread owns
	constexpr int TEAMS = kTeamBlock / TEAM;
	const uint32_t q = k + 1 + Model::kTail;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int tid = TEAM == kTeamBlock ? static_cast<int>(threadIdx.x) : lane;
	const uint32_t i = blockIdx.x * TEAMS + (TEAM == kTeamBlock ? 0 : wave);
	if (i >= rows.nv) {
		return; // (the whole team)
	}
	const uint32_t r = rows.v_first + i;
	const int32_t ro = rows.row_of[r];
	const bool dense = ro >= 0;
	double *s_out = m.sums + static_cast<uint64_t>(i) * Model::kNS;
	uint64_t e0 = 0, e1 = rows.sample_ct; // a dense-form row: its samples
	if (dense) {
		if constexpr (!Model::kWalksDense) {
			if (TEAM == 64) {
				m.Zero(i, tid, k); // its result row comes from the dense kernels
			}
			return;
		} else if (TEAM != kTeamBlock) {
			return; // the workgroup launch's row
		}
	} else {
		e0 = rows.off[r];
		e1 = rows.off[r + 1];
		if ((e1 - e0 > kGlmSparseLong) != (TEAM == kTeamBlock)) {
			return; // the other launch's row
		}
	}
	const uint8_t *prow = Model::kWalksDense && dense ? rows.pool + static_cast<uint64_t>(ro) * rows.pitch : nullptr;
	const bool base3 = ro == -4;
	const int bx = (dense || base3) ? 0 : -1 - ro;
	double *list = lds + (TEAM == kTeamBlock ? 0 : static_cast<uint32_t>(wave) * 64u * q);

	// the entries this thread owns: e = tid + t * TEAM
	typename Model::Own own[NOWN];
	double acc[NOWN];
#pragma unroll
	for (int t = 0; t < NOWN; t++) {
		own[t] = m.OwnedEntry(tid + t * TEAM, static_cast<int>(k));
		acc[t] = 0.0;
	}

	double ls[Model::kNL];
#pragma unroll
	for (int j = 0; j < Model::kNL; j++) {
		ls[j] = 0.0;
	}
	long long c_miss = 0, c_called = 0, sx = 0, sxx = 0; // |M|, |C|, sum_C (x - b), sum_C (x^2 - b^2)
	for (uint64_t p0 = e0; p0 < e1; p0 += TEAM) {
		const uint64_t p = p0 + tid;
		bool used = false;
		uint32_t code = 0, s = 0;
		typename Model::Sample v {};
		if (p < e1) {
			bool entry;
			if (Model::kWalksDense && dense) {
				s = static_cast<uint32_t>(p);
				code = (prow[s >> 2] >> (2 * (s & 3u))) & 3u;
				entry = code != 0u;
			} else {
				const uint32_t x = rows.entries[p];
				s = x >> 2;
				code = x & 3u;
				entry = s < rows.sample_ct;
			}
			if (entry) {
				used = m.Load(s, &v);
			}
		}
		double zi[KP > 0 ? KP : 1];
		if (used) {
#pragma unroll
			for (int j = 0; j < KP; j++) {
				zi[j] = z[static_cast<uint64_t>(s) * KP + j];
			}
			if (code != 3u) {
				const int d = static_cast<int>(code) - bx;
				c_called++;
				sx += d;
				sxx += static_cast<int>(code * code) - bx * bx;
				m.Add(static_cast<double>(d), v, zi, ls);
			} else {
				c_miss++;
			}
		}
		// the list set of this step, in entry order (base 3: the called entries, which are all of them)
		const bool take = used && (base3 || code == 3u);
		uint32_t total;
		const uint32_t rank = TeamRank<TEAM>(take, lane, wave, &total);
		if (total) { // (the whole team agrees)
			if (take) {
				double *row = list + rank * q;
				row[0] = 1.0;
#pragma unroll
				for (int j = 0; j < KP; j++) {
					if (j < static_cast<int>(k)) {
						row[1 + j] = zi[j];
					}
				}
				m.Tail(v, row + k + 1);
			}
			TeamSync<TEAM>();
#pragma unroll
			for (int t = 0; t < NOWN; t++) {
				if (own[t].a >= 0) {
					for (uint32_t l = 0; l < total; l++) {
						acc[t] += m.Term(list, l * q, own[t]);
					}
				}
			}
		}
		TeamSync<TEAM>(); // the list and TeamRank's counts are rewritten by the next step
	}

	long long ct[4] = {c_miss, c_called, sx, sxx};
	TeamSums<TEAM>(ls, ct, lane, wave);
	m.template Epilogue<TEAM>(i, tid, k, base3, bx, ls, own, acc);
	const long long n = base3 ? ct[1] : static_cast<long long>(n_y) - ct[0];
	if (tid == 0) {
		s_out[0] = static_cast<double>(n);
		s_out[1] = static_cast<double>(bx * n + ct[2]);
		s_out[2] = static_cast<double>(bx * bx * n + ct[3]);
	}
}

} // namespace

} // namespace pgh
