// glm_lanes.hpp -- the device code the multi-phenotype sparse kernels share (glm_score_sparse_multi.hip,
// glm_sparse_multi.hip): the walk of a sparse row's entries with lanes across phenotypes, its two launches, and the
// missing-call correction of one (row, tile of owned entries) with a phenotype axis.  Each file instantiates them with a
// model that holds its arithmetic, as the single-phenotype files instantiate TeamWalkSparseRow (glm_team.hpp).
//
// The value block.  val[s][j] is one Model::Value per (raw sample s, block phenotype j < pb), the pb values of a sample
// contiguous; Model::Outside() where s is outside S_j (the samples that have a value of phenotype j) or outside the subset.
//
// The entry kernel, lanes across phenotypes.  A group of PBW lanes (pb rounded up to a power of two) walks a row, lane j
// for phenotype j: per entry the group reads the entry word and the covariate row once (the same address on every
// lane; with PBW == 64 they are scalar loads) and the lanes read the pb contiguous values of the sample.  A lane keeps
// the model's kNL sums and its integer counts, gated by Model::Used.  A wave holds 64 / PBW rows.  The entry words,
// values and covariate rows of several entries are loaded before their FMAs.
//
// The order of the sums, a function of the row alone.  A sparse row's entries are cut into consecutive segments of
// kGlmSparseLong entries, a dense-form row's samples (it is walked from its pool row as a base-0 row) into consecutive
// segments of kGlmSparseLong samples.  Each (segment, phenotype, sum) is one fma chain in entry order, and the
// segments' chains are added in ascending order.  A sparse row of at most kGlmSparseLong entries is one segment, one
// chain (the group form); the longer rows and the dense-form rows go to a workgroup whose lane groups take the
// segments round robin and add them in order through LDS, where the row's totals live too (the workgroup form).
// Neither depends on pb, on which rows share a wave, on the chunk or on where the range starts, and there are no
// floating-point atomics.  That order is the result, bit for bit, of every entry point built on this walk.
//
// Centring.  Phenotype j's covariates are centred on the means over its own missing-value pattern: a lane subtracts its
// means mz[j] from the covariate row per entry.
//
// The missing-call corrections.  The list set of a row (its code-3 entries, or every entry of a base-3 row) does not
// depend on the phenotype; its rows [1, z] and their [list row][PBW] tile of values are staged in LDS kCorrStep at a
// time, and a thread owns kCorrOwn (entry, phenotype) pairs of the model's packed set, phenotype fastest across lanes,
// each summed over the list in entry order (the owners' rule of glm_team.hpp with a phenotype axis).
#pragma once

#include "glm_team.hpp"

#include <type_traits>

namespace pgh {

namespace {

constexpr int kCorrOwn = 8;   // (entry, phenotype) pairs a thread of a correction kernel owns
constexpr int kCorrStep = 32; // list rows of one LDS step of a correction kernel

uint32_t Blocks(uint64_t n, uint32_t per) {
	return static_cast<uint32_t>((n + per - 1) / per);
}

// ---------------------------------------------------------------------------
// the entry walk
// ---------------------------------------------------------------------------

// A Model of the walk, LanesWalkSparseRow<Model, KP, PBW, LONG>, supplies (all static)
//   Value, kNL: what a lane loads per (sample, phenotype), and the number of its fma chains;
//   Outside(): the Value of a sample outside S_j;  Used(v): v is not that;
//   Add(dd, v, zi, mzr, ls): a called entry's d = x - b, of a sample whose value is v and whose covariate row is zi,
//   joins the lane's chains ls (mzr: the lane's means);
//   Row(i, nv, pb, j): the row of sums, kNL + 3 doubles each, that takes (chunk variant i, block phenotype j).
// The walk stores n, sum x, sum x^2 in the row's first three doubles, integers until then, and the chains after them.

// One lane's sums of one phenotype: the model's chains ls and |M|, |C|, sum_C (x - b), sum_C (x^2 - b^2).
template <int NL>
struct LaneSums {
	double ls[NL];
	long long cm, cc, sx, sxx;
	__device__ __forceinline__ void Clear() {
#pragma unroll
		for (int t = 0; t < NL; t++) {
			ls[t] = 0.0;
		}
		cm = cc = sx = sxx = 0;
	}
};

// An entry (code, its covariate row zi) of a sample whose value is v joins the lane's sums.
template <class Model, int KP>
__device__ __forceinline__ void AddEntry(const typename Model::Value v, uint32_t code, int bx, const double *zi,
                                         const double (&mzr)[KP > 0 ? KP : 1], LaneSums<Model::kNL> *a) {
	if (Model::Used(v)) {
		if (code != 3u) {
			const int d = static_cast<int>(code) - bx;
			a->cc++;
			a->sx += d;
			a->sxx += static_cast<int>(code * code) - bx * bx;
			Model::Add(static_cast<double>(d), v, zi, mzr, a->ls);
		} else {
			a->cm++;
		}
	}
}

// The entries [p0, p1) of a sparse row, in order; returns how many belong to the list set.
template <class Model, int KP, int PBW, bool LONG>
__device__ __forceinline__ uint32_t WalkEntries(const uint32_t *__restrict__ entries, uint64_t p0, uint64_t p1,
                                                uint32_t sample_ct, const typename Model::Value *__restrict__ val,
                                                uint32_t pb, int j, const double *__restrict__ z, int bx, bool base3,
                                                const double (&mzr)[KP > 0 ? KP : 1], LaneSums<Model::kNL> *a) {
	// entries whose loads are in flight together; with PBW == 64 the covariate rows are held in scalar registers, 2 KP U
	// of them, which must leave the kernel's other scalars their room; the workgroup form at the two widest widths takes
	// one entry at a time, which keeps it within the vector registers (the table of DESIGN.md section 3.10)
	constexpr int U = PBW == 64 ? (KP <= 4 ? 4 : KP <= 12 ? 2 : 1) : (KP <= 8 ? 4 : LONG && KP >= 16 ? 1 : 2);
	uint32_t n_list = 0;
	for (uint64_t p = p0; p < p1; p += U) {
		uint32_t x[U];
		typename Model::Value v[U];
		double zi[U][KP > 0 ? KP : 1];
#pragma unroll
		for (int u = 0; u < U; u++) {
			x[u] = p + u < p1 ? entries[p + u] : 0xFFFFFFFFu;
			if constexpr (PBW == 64) {
				x[u] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x[u])));
			}
		}
#pragma unroll
		for (int u = 0; u < U; u++) {
			const uint32_t s = x[u] >> 2;
			v[u] = Model::Outside();
			if (s < sample_ct) {
				v[u] = val[static_cast<uint64_t>(s) * pb + j];
#pragma unroll
				for (int t = 0; t < KP; t++) {
					zi[u][t] = z[static_cast<uint64_t>(s) * KP + t];
				}
			}
		}
#pragma unroll
		for (int u = 0; u < U; u++) {
			const uint32_t s = x[u] >> 2, code = x[u] & 3u;
			if (s < sample_ct) {
				n_list += (base3 || code == 3u) ? 1u : 0u;
				AddEntry<Model, KP>(v[u], code, bx, zi[u], mzr, a);
			}
		}
	}
	return n_list;
}

// The samples [s0, s1) of a dense-form row (s0 a multiple of 4), in order, as a base-0 row.
template <class Model, int KP>
__device__ __forceinline__ uint32_t WalkSamples(const uint8_t *__restrict__ prow, uint32_t s0, uint32_t s1,
                                                const typename Model::Value *__restrict__ val, uint32_t pb, int j,
                                                const double *__restrict__ z, const double (&mzr)[KP > 0 ? KP : 1],
                                                LaneSums<Model::kNL> *a) {
	uint32_t n_list = 0;
	for (uint32_t sb = s0; sb < s1; sb += 4) {
		const uint32_t byte = prow[sb >> 2];
		if (byte == 0u) {
			continue;
		}
		for (uint32_t q = 0; q < 4u && sb + q < s1; q++) {
			const uint32_t code = (byte >> (2u * q)) & 3u, s = sb + q;
			if (code != 0u) {
				n_list += code == 3u ? 1u : 0u;
				double zi[KP > 0 ? KP : 1];
#pragma unroll
				for (int t = 0; t < KP; t++) {
					zi[t] = z[static_cast<uint64_t>(s) * KP + t];
				}
				AddEntry<Model, KP>(val[static_cast<uint64_t>(s) * pb + j], code, 0, zi, mzr, a);
			}
		}
	}
	return n_list;
}

// The row of sums of the row i for the block phenotype j.
template <class Model>
__device__ __forceinline__ void StoreSums(const LaneSums<Model::kNL> &a, uint32_t i, uint32_t nv, uint32_t pb, int j,
                                          uint32_t n_y, int bx, bool base3, double *__restrict__ sums) {
	double *so = sums + Model::Row(i, nv, pb, j) * (Model::kNL + 3);
	const long long n = base3 ? a.cc : static_cast<long long>(n_y) - a.cm;
	so[0] = static_cast<double>(n);
	so[1] = static_cast<double>(bx * n + a.sx);
	so[2] = static_cast<double>(bx * bx * n + a.sxx);
#pragma unroll
	for (int t = 0; t < Model::kNL; t++) {
		so[3 + t] = a.ls[t];
	}
}

// The body of an entry kernel of kTeamBlock threads.  LONG == false, the group form: a group of PBW lanes per row,
// kTeamBlock / PBW rows per workgroup, the sparse rows of at most kGlmSparseLong entries.  LONG == true, the workgroup
// form: a workgroup per row, the longer sparse rows and the dense-form rows.  The two launches cover the same rows and
// each returns from the other's.  z: the KP doubles of a sample's covariates at z[s * KP], raw-sample order; mz[j][KP]
// and ny[j]: phenotype j's means and |S_j|; nlist[i]: the row's list-set count; part: the workgroup form's LDS
// (LaunchEntryForms sizes it).
template <class Model, int KP, int PBW, bool LONG>
__device__ __forceinline__ void LanesWalkSparseRow(const SparseRows &rows, const typename Model::Value *__restrict__ val,
                                                   const double *__restrict__ z, const double *__restrict__ mz,
                                                   const uint32_t *__restrict__ ny, uint32_t pb,
                                                   double *__restrict__ sums, uint32_t *__restrict__ nlist,
                                                   double *part) {
	constexpr int G = kTeamBlock / PBW; // lane groups of a workgroup
	constexpr int NL = Model::kNL;
	constexpr uint32_t kSeg = kGlmSparseLong;
	const int j = static_cast<int>(threadIdx.x) & (PBW - 1), g = static_cast<int>(threadIdx.x) / PBW;
	uint32_t i = LONG ? blockIdx.x : blockIdx.x * G + static_cast<uint32_t>(g);
	if constexpr (PBW == 64) {
		i = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(i)));
	}
	if (i >= rows.nv) {
		return; // (LONG: the whole workgroup)
	}
	const uint32_t r = rows.v_first + i;
	const int32_t ro = rows.row_of[r];
	const bool dense = ro >= 0;
	uint64_t e0 = 0, e1 = rows.sample_ct;
	if (!dense) {
		e0 = rows.off[r];
		e1 = rows.off[r + 1];
	}
	if ((dense || e1 - e0 > kSeg) != LONG) {
		return; // the other launch's row (LONG: the whole workgroup)
	}
	const bool live = static_cast<uint32_t>(j) < pb;
	if (!LONG && !live) {
		return;
	}
	const bool base3 = ro == -4;
	const int bx = (dense || base3) ? 0 : -1 - ro;
	const int jj = live ? j : 0; // (an idle lane of the workgroup form reads phenotype 0's values and stores nothing)
	double mzr[KP > 0 ? KP : 1];
#pragma unroll
	for (int t = 0; t < KP; t++) {
		mzr[t] = mz[static_cast<uint64_t>(jj) * KP + t];
	}
	LaneSums<NL> a;
	a.Clear();
	uint32_t n_list = 0;
	if constexpr (!LONG) {
		n_list = WalkEntries<Model, KP, PBW, false>(rows.entries, e0, e1, rows.sample_ct, val, pb, jj, z, bx, base3, mzr, &a);
	} else {
		// the groups' chains of a round, G x max(NL, 5) x PBW doubles, then the row's totals, NL x PBW doubles: group 0's
		// lanes alone read and write the totals, each its own, so they cost no registers and need no barrier
		double *tot = part + kTeamBlock * (NL > 5 ? NL : 5);
		const uint8_t *prow = dense ? rows.pool + static_cast<uint64_t>(ro) * rows.pitch : nullptr;
		const uint64_t n_seg = (e1 - e0 + kSeg - 1) / kSeg;
		if (g == 0) {
#pragma unroll
			for (int t = 0; t < NL; t++) {
				tot[t * PBW + j] = 0.0;
			}
		}
		long long cm = 0, cc = 0, sx = 0, sxx = 0;
		for (uint64_t seg0 = 0; seg0 < n_seg; seg0 += G) {
			const uint64_t seg = seg0 + static_cast<uint64_t>(g);
			a.Clear();
			if (seg < n_seg) {
				const uint64_t p0 = e0 + seg * kSeg, p1 = p0 + kSeg < e1 ? p0 + kSeg : e1;
				if (dense) {
					n_list += WalkSamples<Model, KP>(prow, static_cast<uint32_t>(p0), static_cast<uint32_t>(p1), val, pb, jj, z,
					                                 mzr, &a);
				} else {
					n_list += WalkEntries<Model, KP, PBW, true>(rows.entries, p0, p1, rows.sample_ct, val, pb, jj, z, bx, base3,
					                                            mzr, &a);
				}
			}
			cm += a.cm;
			cc += a.cc;
			sx += a.sx;
			sxx += a.sxx;
#pragma unroll
			for (int t = 0; t < NL; t++) {
				part[(g * NL + t) * PBW + j] = a.ls[t];
			}
			__syncthreads();
			if (g == 0) {
				const uint64_t left = n_seg - seg0;
				const int n_here = left < static_cast<uint64_t>(G) ? static_cast<int>(left) : G;
#pragma unroll
				for (int t = 0; t < NL; t++) {
					double sum = tot[t * PBW + j];
					for (int gg = 0; gg < n_here; gg++) {
						sum += part[(gg * NL + t) * PBW + j];
					}
					tot[t * PBW + j] = sum;
				}
			}
			__syncthreads();
		}
		// the integer counts of the groups: any order gives the same number
		long long *ipart = reinterpret_cast<long long *>(part);
		ipart[(g * 5 + 0) * PBW + j] = cm;
		ipart[(g * 5 + 1) * PBW + j] = cc;
		ipart[(g * 5 + 2) * PBW + j] = sx;
		ipart[(g * 5 + 3) * PBW + j] = sxx;
		ipart[(g * 5 + 4) * PBW + j] = static_cast<long long>(n_list);
		__syncthreads();
		if (g != 0 || !live) {
			return;
		}
		a.cm = a.cc = a.sx = a.sxx = 0;
		long long nl = 0;
		for (int gg = 0; gg < G; gg++) {
			a.cm += ipart[(gg * 5 + 0) * PBW + j];
			a.cc += ipart[(gg * 5 + 1) * PBW + j];
			a.sx += ipart[(gg * 5 + 2) * PBW + j];
			a.sxx += ipart[(gg * 5 + 3) * PBW + j];
			nl += ipart[(gg * 5 + 4) * PBW + j];
		}
		n_list = static_cast<uint32_t>(nl);
#pragma unroll
		for (int t = 0; t < NL; t++) {
			a.ls[t] = tot[t * PBW + j];
		}
	}
	StoreSums<Model>(a, i, rows.nv, pb, j, ny[j], bx, base3, sums);
	if (j == 0) {
		nlist[i] = n_list;
	}
}

// The two launches of an entry kernel over nv rows: launch(width, form, grid, lds) starts the kernel's instantiation
// <KP, decltype(width)::value, decltype(form)::value> (form: LONG) on grid workgroups of kTeamBlock threads with lds
// bytes of dynamic LDS.  NL: the model's kNL.
template <int NL, int PBW, class Launch>
void LaunchEntryForms(uint32_t nv, Launch &&launch) {
	// the workgroup form of one lane per group holds the means in scalar registers and spilled some of them: a block of
	// one phenotype takes the form of two lanes per group there, with one lane idle
	constexpr int G = kTeamBlock / PBW, PBL = PBW == 1 ? 2 : PBW;
	const size_t lds = sizeof(double) * (kTeamBlock * (NL > 5 ? NL : 5) + NL * PBL);
	launch(std::integral_constant<int, PBW>(), std::false_type(), Blocks(nv, G), size_t {0});
	launch(std::integral_constant<int, PBL>(), std::true_type(), nv, lds);
}

// Calls launch(std::integral_constant<int, PBW>()) with PBW = pb rounded up to a power of two (pb <= 64).
template <class Launch>
void ForGroupWidth(uint32_t pb, Launch &&launch) {
	if (pb <= 1) {
		launch(std::integral_constant<int, 1>());
	} else if (pb <= 2) {
		launch(std::integral_constant<int, 2>());
	} else if (pb <= 4) {
		launch(std::integral_constant<int, 4>());
	} else if (pb <= 8) {
		launch(std::integral_constant<int, 8>());
	} else if (pb <= 16) {
		launch(std::integral_constant<int, 16>());
	} else if (pb <= 32) {
		launch(std::integral_constant<int, 32>());
	} else {
		launch(std::integral_constant<int, 64>());
	}
}

// ---------------------------------------------------------------------------
// the missing-call corrections
// ---------------------------------------------------------------------------

// A Model of LanesCorrectRow<Model, PBW> supplies
//   Value: the element of the [list row][PBW] tile;  pb, the block's phenotypes, as a member;  Stage(s, pp): the
//   element of (sample s, phenotype column pp), pp < PBW, with the model's rule for pp >= pb and for a sample outside
//   S_pp;
//   Entries(k): the entries of its packed set;
//   Own, OwnedEntry(e, k, have, mz, &own): an owner's entry e, its columns of a list row [1, z_1 .. z_k] and their
//   centring means of mz, the kp means of the owner's phenotype; own.a < 0: there is no entry, which is so whenever
//   `have` is false (the owner's lane is past pb or e past the tile: e may then be past the set, and mz is not read);
//   Term(v, row, own, acc): acc with the entry's term of the list row `row` and the tile element v added.  v is
//   taken by value: a term that reads one half of an element through a reference costs vector registers;
//   Store(i, pp, e, v, base3): v is the sum of entry e of (chunk variant i, block phenotype pp).

// The LDS of LanesCorrectRow, in bytes: the list rows zl[kCorrStep][k + 1], their tile [kCorrStep][PBW] of Value, the
// transposed sums stage[kTeamBlock * kCorrOwn], and the list rows' samples.
template <class Model, int PBW>
size_t LanesCorrectLds(uint32_t k) {
	return sizeof(double) * (kCorrStep * (k + 1) + kTeamBlock * kCorrOwn) + sizeof(typename Model::Value) * kCorrStep * PBW +
	       4 * kCorrStep;
}

// This workgroup, the row i (which has list entries), and the entries tile * ET .. of the model's packed set,
// ET = kTeamBlock * kCorrOwn / PBW (the grid has tile * ET < Entries(k)): collects the list set in entry order, stages
// its rows and the value tile kCorrStep at a time, runs the owners' loops, and hands the sums, transposed through LDS so
// that a phenotype's entries are stored side by side, to m.Store.  Every thread of the workgroup calls it, under
// workgroup-uniform control flow; a caller that calls it again puts a barrier between the calls (the next row rewrites
// the stage and the list).
template <class Model, int PBW>
__device__ __forceinline__ void LanesCorrectRow(const SparseRows &rows, uint32_t i, uint32_t tile,
                                                const double *__restrict__ z, uint32_t kp, uint32_t k,
                                                const double *__restrict__ mz, const Model &m, double *lds) {
	using Value = typename Model::Value;
	constexpr int GR = kTeamBlock / PBW; // entries of one pass of the workgroup's threads
	constexpr int ET = GR * kCorrOwn;    // entries of a tile
	const uint32_t q1 = k + 1, ne = Model::Entries(k);
	const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
	const uint32_t r = rows.v_first + i;
	const int32_t ro = rows.row_of[r];
	const bool dense = ro >= 0, base3 = ro == -4;
	const uint32_t e_first = tile * ET;
	const uint32_t e_ct = ne - e_first < static_cast<uint32_t>(ET) ? ne - e_first : ET;

	double *zl = lds;
	Value *vt = reinterpret_cast<Value *>(lds + kCorrStep * q1);
	double *stage = reinterpret_cast<double *>(vt + kCorrStep * PBW);
	uint32_t *sl = reinterpret_cast<uint32_t *>(stage + kTeamBlock * kCorrOwn);

	const int p = tid & (PBW - 1), el0 = tid / PBW;
	const uint32_t pb = m.pb;
	const bool live = static_cast<uint32_t>(p) < pb;
	typename Model::Own own[kCorrOwn];
	double acc[kCorrOwn];
#pragma unroll
	for (int t = 0; t < kCorrOwn; t++) {
		const uint32_t el = static_cast<uint32_t>(el0 + t * GR);
		m.OwnedEntry(static_cast<int>(e_first + el), static_cast<int>(k), live && el < e_ct,
		             mz + static_cast<uint64_t>(p) * kp, &own[t]);
		acc[t] = 0.0;
	}

	uint64_t e0 = 0, e1 = rows.sample_ct;
	if (!dense) {
		e0 = rows.off[r];
		e1 = rows.off[r + 1];
	}
	const uint8_t *prow = dense ? rows.pool + static_cast<uint64_t>(ro) * rows.pitch : nullptr;
	for (uint64_t p0 = e0; p0 < e1; p0 += kTeamBlock) {
		const uint64_t at = p0 + static_cast<uint64_t>(tid);
		bool take = false;
		uint32_t s = 0;
		if (at < e1) {
			if (dense) {
				s = static_cast<uint32_t>(at);
				take = ((prow[s >> 2] >> (2u * (s & 3u))) & 3u) == 3u;
			} else {
				const uint32_t x = rows.entries[at];
				s = x >> 2;
				take = s < rows.sample_ct && (base3 || (x & 3u) == 3u);
			}
		}
		uint32_t total;
		const uint32_t rank = TeamRank<kTeamBlock>(take, lane, wave, &total);
		for (uint32_t sub = 0; sub < total; sub += kCorrStep) {
			if (take && rank >= sub && rank < sub + kCorrStep) {
				const uint32_t l = rank - sub;
				sl[l] = s;
				zl[l * q1] = 1.0;
				for (uint32_t t = 0; t < k; t++) {
					zl[l * q1 + 1 + t] = z[static_cast<uint64_t>(s) * kp + t];
				}
			}
			__syncthreads();
			const uint32_t nl = total - sub < static_cast<uint32_t>(kCorrStep) ? total - sub : kCorrStep;
			for (uint32_t c = static_cast<uint32_t>(tid); c < nl * PBW; c += kTeamBlock) {
				vt[c] = m.Stage(sl[c / PBW], c & (PBW - 1));
			}
			__syncthreads();
#pragma unroll
			for (int t = 0; t < kCorrOwn; t++) {
				if (own[t].a >= 0) {
					for (uint32_t l = 0; l < nl; l++) {
						acc[t] = m.Term(vt[l * PBW + p], zl + l * q1, own[t], acc[t]);
					}
				}
			}
			__syncthreads();
		}
		__syncthreads(); // TeamRank's counts are rewritten by the next step
	}

	// the tile's sums, transposed through LDS so that a phenotype's entries are stored side by side
#pragma unroll
	for (int t = 0; t < kCorrOwn; t++) {
		stage[(el0 + t * GR) * PBW + p] = acc[t];
	}
	__syncthreads();
	for (uint32_t c = static_cast<uint32_t>(tid); c < pb * e_ct; c += kTeamBlock) {
		const uint32_t pp = c / e_ct, el = c - pp * e_ct;
		m.Store(i, pp, e_first + el, stage[el * PBW + pp], base3);
	}
}

} // namespace

} // namespace pgh
