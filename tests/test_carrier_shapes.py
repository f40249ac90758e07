"""Every entry point that reads the sparse-resident form, under the structured carrier rows of tests/carrier_shapes.py.

The catalogue puts a row's entries on the hard edges of the walks: 64 and 256 entries a step, the team split at
kGlmSparseLong = 1024 entries (which is also the wave stash of the saddlepoint and Firth kernels and the segment of the
multi kernels), the levels of the 64-way search, the 8192-sample tiles of the per-sample tallies and every tile
pgh_score_sparse takes, base codes 1, 2 and 3, and dense-form rows.  One matrix per sample count, one variant per
designed row, written with every record type and opened dense and in three sparse forms: the default rule, every row
sparse, and max_minor = kGlmSparseLong, where the form split and the team split fall on the same rows.

One GPU test per family.  The reference of every output is the family's own float64 oracle (glm_oracle,
glm_score_oracle, glm_spa_oracle, glm_firth_sparse_oracle, skat_oracle, test_score_sparse's and test_burden_sparse's),
integer outputs are compared with np.array_equal, and every floating comparison takes the constant the entry point's
own test file uses; none is introduced here.  No designed row is skipped: a row the oracles refuse is compared by its
errcode, which the CPU test pins by name."""

import re
import types

import numpy as np
import pytest

import carrier_shapes as CS
import subset_shapes as SS

W = SS.W
N_WIDE, N_TILE = CS.N_WIDE, CS.N_TILE
FORMS = ("default", "all", "long")  # max_minor = 0, n and kGlmSparseLong
WINDOW_ROWS = 23                     # PGH_SPARSE_WINDOW_BYTES in row pitches: an open spans four windows
CUTOFF = 0.1                         # the lowest cutoff the saddlepoint and Firth entry points accept
KS = (2, 0)                          # covariate counts
ROW_COUNTS = {N_TILE: 72, N_WIDE: 91}
# the rows the oracles refuse under the single-phenotype calls' phenotypes, with and without covariates
REFUSED = {"b1_E0": "CONST_ALLELE", "b2_E0": "CONST_ALLELE", "allmiss_entries": "CONST_ALLELE",
           "carriers_without_phenotype": "CONST_ALLELE", "b3_E0": "TOO_FEW_SAMPLES", "b3_E1": "TOO_FEW_SAMPLES"}


def max_minor_of(form, n):
    return {"default": 0, "all": n, "long": CS.LONG}[form]


def kinds_of(n, codes):
    return W.choose_kinds(codes, np.random.default_rng(n))


# ---- the catalogue itself (no GPU) -------------------------------------------------------------------------------

def _spec(n, name):
    """(base, entries, first entry sample, last entry sample) of a designed row, from its name alone -- written out
    independently of carrier_shapes.rows()."""
    gone = np.flatnonzero(SS.nan_samples(n))
    m = re.fullmatch(r"E(\d+)_(tile0|tile1|last|spread)", name)
    if m:
        e, where = int(m.group(1)), m.group(2)
        first = {"tile0": 0, "tile1": 8192, "last": n - e, "spread": 0}[where]
        last = {"tile0": e - 1, "tile1": 8191 + e, "last": n - 1, "spread": (e - 1) * n // e}[where]
        return 0, e, first, last
    m = re.fullmatch(r"b([123])_E(\d+)", name)
    if m:
        b, e = int(m.group(1)), int(m.group(2))
        return (b, e, 0, (e - 1) * n // e) if e else (b, 0, None, None)
    return {
        "edges": (0, 6 if n == N_WIDE else 2, 0, n - 1),
        "stride64": (0, 2 * (n // 64) + (n % 64 > 0), 0, n - 1 if n % 64 == 0 else n // 64 * 64),
        "run64_then_next": (0, 67, 8128, 8194),
        "run128_then_next": (0, 131, 8064, 8194),
        "allmiss_entries": (0, 100, 0, 99 * n // 100),
        "nocall_missing": (0, 1500, 0, 1499 * n // 1500),
        "carriers_without_phenotype": (0, len(gone), int(gone[0]), int(gone[-1])),
        "long_held_short_used": (0, 1100, None, None),
    }[name]


def test_the_catalogue_is_what_the_walks_are_meant_to_see():
    """The entry count, the base (majority) code and the first and last entry sample of every row are what its name
    says, the entry codes cycle through the codes other than the base, and the rows that are aimed at one edge sit on
    it: a later edit cannot quietly move a row off the edge it was made for."""
    assert (CS.LONG, CS.SPARSE_TILE, CS.SCORE_ACC_BYTES, CS.SCORE_CHUNK) == (1024, 8192, 131072, 8)
    assert (N_TILE, N_WIDE) == (8192, 16451) and N_WIDE == 2 * 8192 + 67 and (N_WIDE + 3) // 4 > 4096
    assert CS.score_tiles() == sorted({131072 // (8 * a + 4) // 64 * 64 for a in range(1, 10)})
    assert len(CS.score_tiles()) == 9 and max(CS.score_tiles()) < N_WIDE
    for n in CS.SAMPLE_COUNTS:
        cat = CS.rows(n)
        names, codes = CS.matrix(n)
        assert names == list(cat) and len(names) == ROW_COUNTS[n]
        assert set(kinds_of(n, codes)) == {0, 1, 2, 3, 4, 6, 7}, "every record type"
        have = ~SS.nan_samples(n)
        for name, row in cat.items():
            assert row.dtype == np.uint8 and row.shape == (n,) and row.max() <= 3, name
            want_base, want_e, first, last = _spec(n, name)
            base, at = CS.entry_samples(row)
            assert (base, len(at)) == (want_base, want_e), (n, name, base, len(at))
            if first is not None:
                assert (int(at[0]), int(at[-1])) == (first, last), (n, name)
            cycle = {"allmiss_entries": [3], "nocall_missing": [1, 2]}.get(name, [c for c in range(4) if c != base])
            assert row[at].tolist() == [cycle[i % len(cycle)] for i in range(len(at))], (n, name)
        # every count in every placement that fits, every base at the split
        for e in CS.ENTRY_COUNTS:
            fits = [w for w in CS.PLACEMENTS if f"E{e}_{w}" in cat]
            assert fits == (list(CS.PLACEMENTS) if n == N_WIDE else ["tile0", "last", "spread"]), (n, e)
        assert {CS.LONG - 1, CS.LONG, CS.LONG + 1, 2 * CS.LONG, 2 * CS.LONG + 1, 63, 64, 65, 255, 256, 257, 4096,
                4097} <= set(CS.ENTRY_COUNTS)
        assert all(f"b{b}_E{e}" in cat for b in (1, 2, 3) for e in (0, 1, 64, CS.LONG, CS.LONG + 1))
        # stride64 carries an entry on both sides of every tile boundary there is
        stride = cat["stride64"]
        for tile in CS.score_tiles() + [CS.SPARSE_TILE]:
            assert tile % 64 == 0
            for edge in range(tile, n, tile):
                assert stride[edge - 1] != 0 and stride[edge] != 0, (n, tile, edge)
        edges = [0, 8191, 8192, 16383, 16384, 16450] if n == N_WIDE else [0, 8191]
        assert np.flatnonzero(cat["edges"]).tolist() == edges
        # the used entries of long_held_short_used are exactly kGlmSparseLong of more held
        held = np.flatnonzero(cat["long_held_short_used"])
        assert len(held) == CS.HELD > CS.LONG and int(have[held].sum()) == CS.LONG
        assert not have[np.flatnonzero(cat["carriers_without_phenotype"])].any()
        assert not (cat["nocall_missing"] == 3).any() and len(np.flatnonzero(cat["nocall_missing"])) > CS.LONG
        # the phenotypes: the single calls' own first, and the two that are aimed at a row
        for binary in (True, False):
            y = CS.distinct_phenotypes(n, binary)
            single = CS.binary_phenotype(n) if binary else CS.linear_phenotype(n)
            assert np.array_equal(y[CS.PHENO_PLAIN], single, equal_nan=True)
            assert np.array_equal(np.isnan(single), SS.nan_samples(n))
            gone = np.isnan(y)
            assert gone[CS.PHENO_ROW_GONE][CS.entry_samples(cat[CS.ROW_GONE])[1]].all()
            past = CS.entry_samples(cat[CS.ROW_PAST_LONG])[1]
            assert len(past) == CS.LONG + 1 and not gone[CS.PHENO_PAST_LONG][past[:CS.LONG]].any()
            assert gone[CS.PHENO_PAST_LONG][past[CS.LONG:]].all() and gone[CS.PHENO_PLAIN][past[:CS.LONG]].any()
            assert not gone[CS.PHENO_COMPLETE].any() and len({g.tobytes() for g in gone}) == 5
            if binary:
                assert set(np.unique(y[~gone])) == {0.0, 1.0}
            for count in CS.BLOCK_COUNTS:
                block = CS.phenotype_block(n, count, binary)
                assert block.shape == (count, n)
                assert all(np.array_equal(block[j], y[j % 5], equal_nan=True) for j in range(count))
        assert CS.BLOCK_COUNTS[0] & (CS.BLOCK_COUNTS[0] - 1) and CS.BLOCK_COUNTS[-1] > CS.PHENO_BLOCK
    wide = CS.rows(N_WIDE)
    # the ragged last tile [16384, 16451): 64 and 65 entries fill it but for three and two samples, 128 straddle it
    assert [int(np.flatnonzero(wide[f"E{e}_last"])[0]) for e in (64, 65, 128)] == [16387, 16386, 16323]
    for run in (64, 128):  # a whole number of wave steps ends with tile 0, and the row goes on
        at = np.flatnonzero(wide[f"run{run}_then_next"])
        assert (at < 8192).sum() == run and at[run - 1] == 8191 and at[run:].tolist() == [8192, 8193, 8194]
    labels, sets = CS.variant_sets(list(wide))
    assert labels[:len(wide)] == list(wide)
    assert [s.tolist() for s in sets[:len(wide)]] == [[i] for i in range(len(wide))]
    assert labels[len(wide):] == ["all_tile1", "mixed_bases", "long_twice"] and len(sets[-3]) == len(CS.ENTRY_COUNTS)
    assert sorted(CS.entry_samples(wide[list(wide)[i]])[0] for i in sets[-2]) == [0, 1, 2, 3]
    assert sets[-1][0] == sets[-1][1] and len(np.flatnonzero(wide[list(wide)[sets[-1][0]]])) == 4097


def _refused(p, names):
    """The refused rows of distinct phenotype p, from REFUSED and what the phenotype was made for."""
    out = dict(REFUSED)
    if p in (CS.PHENO_COMPLETE, CS.PHENO_PAST_LONG):
        # a value everywhere, or at samples 0..1023 (ROW_PAST_LONG's first entries): some of its carriers count
        del out["carriers_without_phenotype"]
    return {k: v for k, v in out.items() if k in names}


def test_the_oracles_fit_every_designed_row_but_the_refused_ones():
    """glm_oracle (linear) and glm_score_oracle fit every designed row under the single-phenotype calls' phenotypes,
    with two covariates and with none, except REFUSED, whose errcodes are pinned; no row trips the score oracle's
    pivot-rule assertion; no |stat| lies at CUTOFF; the linear fits are well conditioned (test_glm_sparse_multi's
    RSS_FLOOR).  Under the block's other phenotypes the refused rows are those plus the rows the phenotype's gaps
    empty, the row PHENO_ROW_GONE was aimed at among them."""
    G = pytest.importorskip("glm_oracle")
    import glm_score_oracle as O
    import glm_spa_oracle as S
    from test_glm_sparse_multi import RSS_FLOOR

    for n in CS.SAMPLE_COUNTS:
        names, codes = CS.matrix(n)
        x = SS.values(codes)
        for k in KS:
            z = CS.covariates(n, k)
            for binary in (False, True):
                ys = CS.distinct_phenotypes(n, binary)
                for p, y in enumerate(ys):
                    if binary:
                        nul = O.Null(y, z)
                        assert nul.status is None
                        rows = [O.oracle_row(r, nul) for r in x]
                        stats = [abs(r["stat"]) for r in rows if r["errcode"] is None]
                        assert all(abs(t - CUTOFF) > 100 * S.UNDECIDED for t in stats)
                    else:
                        rows = [G.oracle_row(r, y, z, "linear") for r in x]
                        assert all(r["rss"] >= RSS_FLOOR * r["tss"] for r in rows if r["errcode"] is None)
                    got = {name: r["errcode"] for name, r in zip(names, rows) if r["errcode"] is not None}
                    ctx = (n, k, binary, p, got)
                    want = _refused(p, names)
                    if p == CS.PHENO_PLAIN:
                        assert got == want and len(names) - len(got) == ROW_COUNTS[n] - 6, ctx
                        if binary:  # the rows at the split are beyond CUTOFF: the follow-up kernels will take them
                            beyond = {name for name, r in zip(names, rows)
                                      if r["errcode"] is None and abs(r["stat"]) > CUTOFF}
                            assert {name for name in names if re.fullmatch(r"E102[45]_\w+", name)} <= beyond, ctx
                        continue
                    if binary and p == CS.PHENO_PAST_LONG:
                        assert abs(rows[names.index(CS.ROW_PAST_LONG)]["stat"]) > CUTOFF, ctx
                    # the others lose more samples: the refused rows stay refused alike, and what joins them is a
                    # row whose entries all fall into the phenotype's gaps
                    assert {name: got.get(name) for name in want} == want, ctx
                    gone = np.isnan(y)
                    for name in set(got) - set(want):
                        base, at = CS.entry_samples(codes[names.index(name)])
                        assert got[name] == "CONST_ALLELE" and gone[at].all(), (name, ctx)
                    assert (CS.ROW_GONE in got) == (p == CS.PHENO_ROW_GONE), ctx
                    assert CS.ROW_PAST_LONG not in got, ctx


# ---- the files, the forms and the oracles' rows, built once per module --------------------------------------------

def _col(out, p):
    return {key: v[:, p] for key, v in out.items()}


def _rows(out, idx):
    return {key: v[idx] for key, v in out.items()}


def _same_bytes(a, b, ctx, names=None):
    """The two results hold the same bytes; names: the designed rows along axis 0, so that a failure names its rows."""
    assert a.keys() == b.keys(), ctx
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape, (key, ctx)
        if x.dtype == object:
            differ = x != y
        else:
            bits = f"u{x.dtype.itemsize}"
            differ = np.ascontiguousarray(x).view(bits) != np.ascontiguousarray(y).view(bits)
        if differ.any():
            rows = sorted(set(np.argwhere(differ)[:, 0].tolist()))
            raise AssertionError((key, ctx, [names[i] if names is not None else i for i in rows[:8]]))


def _row_by_row(c, check):
    """check(idx) over one designed row at a time: a failure is raised again with the row's name in front."""
    out = []
    for i, name in enumerate(c.names):
        try:
            out.append(check([i]))
        except AssertionError as err:
            raise AssertionError(f"designed row {name}: {err}") from err
    return out


class _Cat:
    """The catalogue of one N as a .pgen of every record type, resident dense and in the three sparse forms."""

    def __init__(self, L, tmp, n):
        import glm_spa_oracle as S

        self.L, self.n = L, n
        self.names, self.codes = CS.matrix(n)
        self.m = len(self.names)
        self.at = {name: i for i, name in enumerate(self.names)}
        self.x = SS.values(self.codes)
        self.minor = np.array([len(CS.entry_samples(r)[1]) for r in self.codes])
        self.path = str(tmp / f"carriers_{n}.pgen")
        W.write_pgen(self.path, self.codes, kinds_of(n, self.codes))
        self.dense = L.Dataset.open(self.path)
        self.pitch = self.dense.info.pitch_bytes
        self.forms, self.row_forms = {}, {}
        for form in FORMS:
            mm = max_minor_of(form, n)
            with pytest.MonkeyPatch.context() as mp:  # several windows per open
                mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(WINDOW_ROWS * self.pitch))
                self.forms[form] = L.Dataset.open(self.path, sparse=True, max_minor=mm)
            self.row_forms[form] = [S.row_form(r, mm) for r in self.codes]
        assert self.m > 3 * WINDOW_ROWS
        self._check_forms()
        self._made = {}

    def dense_form(self, form):
        return np.array([d for _, d in self.row_forms[form]])

    def _check_forms(self):
        """Each form holds the mix it was opened for (sparse_info)."""
        base = np.array([b for b, _ in self.row_forms["all"]])
        for form in FORMS:
            info = self.forms[form].sparse_info()
            dense = self.dense_form(form)
            assert (info.sparse_variant_ct, info.dense_variant_ct) == (int((~dense).sum()), int(dense.sum())), form
            assert info.entry_ct == int(self.minor[~dense].sum()), form
            assert list(info.base_hist) == [int(((base == b) & ~dense).sum()) for b in range(4)], form
        assert not self.dense_form("all").any() and self.minor.max() >= 4097
        # max_minor = kGlmSparseLong: the longest sparse rows hold exactly 1,024 entries, every longer row is dense-form
        long_form = self.dense_form("long")
        assert np.array_equal(long_form, self.minor > CS.LONG)
        assert self.minor[~long_form].max() == CS.LONG and self.minor[long_form].min() == CS.LONG + 1
        # the default rule: 4 m < pitch.  At N_WIDE the split is above the team split (rows of 1,025 entries stay
        # sparse and go to the workgroup form), at N_TILE below it
        assert np.array_equal(self.dense_form("default"), 4 * self.minor >= self.pitch)
        sparse_long = (~self.dense_form("default") & (self.minor > CS.LONG)).sum()
        assert (sparse_long > 0) == (self.n == N_WIDE) and self.dense_form("default").sum() > 0

    def once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    # -- inputs and the oracles' rows ----------------------------------------------------------------------------
    def z(self, k):
        return self.once(("z", k), lambda: CS.covariates(self.n, k))

    def ys(self, binary):
        return self.once(("ys", binary), lambda: CS.distinct_phenotypes(self.n, binary))

    def nul(self, k, p):
        import glm_score_oracle as O
        return self.once(("nul", k, p), lambda: O.Null(self.ys(True)[p], self.z(k)))

    def beyond(self, k, p):
        """bool per row: the score oracle fits the row under distinct phenotype p with |stat| > CUTOFF."""
        import glm_score_oracle as O

        def make():
            rows = [O.oracle_row(r, self.nul(k, p)) for r in self.x]
            return np.array([r["errcode"] is None and abs(r["stat"]) > CUTOFF for r in rows])
        return self.once(("beyond", k, p), make)

    def close(self):
        for ds in list(self.forms.values()) + [self.dense]:
            ds.close()


@pytest.fixture(scope="module")
def cats(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("carrier_shapes")
    made = {}

    def get(n):
        if n not in made:
            made[n] = _Cat(gpu_lib, tmp, n)
        return made[n]

    yield get
    for c in made.values():
        c.close()


def _same_ints(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _packed(codes):
    return np.stack([np.frombuffer(W._pack2(r), dtype=np.uint8) for r in codes])


# ---- 1. the resident form ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", CS.SAMPLE_COUNTS)
def test_resident_form(gpu_lib, cats, n):
    """The rows expanded back to 2 bits, the counts and the per-sample tallies of every sparse form equal the matrix:
    at full range, on a range that starts and ends inside the designed rows, and on a gapped list."""
    c = cats(n)
    packed = _packed(c.codes)
    counts, per_sample = SS.counts_ref(c.codes), SS.sample_counts_ref(c.codes)
    lo, hi = 5, c.m - 7
    gapped = np.array([c.m - 1, 0] + list(range(3, c.m - 2, 2)), dtype=np.uint32)
    assert len(set(gapped.tolist())) == len(gapped) and c.dense.info.record_bytes == packed.shape[1]
    for form, sp in c.forms.items():
        ctx = (n, form)
        assert sp.info.record_bytes == packed.shape[1], ctx
        for i in range(c.m):  # a row alone first, by name: a failure says which designed row
            assert _same_ints(sp.copy_rows_to_host(i, i + 1), packed[i:i + 1]), (c.names[i], ctx)
            assert _same_ints(sp.counts_range(i, i + 1), counts[i:i + 1]), (c.names[i], ctx)
            assert _same_ints(sp.sample_counts(i, i + 1), SS.sample_counts_ref(c.codes[i:i + 1])), (c.names[i], ctx)
        assert _same_ints(sp.copy_rows_to_host(0, c.m), packed), ctx
        assert _same_ints(sp.copy_rows_to_host(lo, hi), packed[lo:hi]), ctx
        assert _same_ints(sp.counts_range(), counts), ctx
        assert _same_ints(sp.counts_range(lo, hi), counts[lo:hi]), ctx
        assert _same_ints(sp.sample_counts(), per_sample), ctx
        assert _same_ints(sp.sample_counts(lo, hi), SS.sample_counts_ref(c.codes[lo:hi])), ctx
        assert _same_ints(sp.sample_counts(vidx=gapped), SS.sample_counts_ref(c.codes[gapped])), ctx


# ---- 2. pgh_score_sparse -----------------------------------------------------------------------------------------

SCORE_COLUMNS = (1, 3, CS.SCORE_CHUNK, CS.SCORE_CHUNK + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", CS.SAMPLE_COUNTS)
def test_score_sparse(gpu_lib, cats, n):
    """Every designed row in one list, with 1, 3, 8 and 9 weight columns (one chunk, then a chunk and one more column,
    so the accumulators per sample and with them the tile change), in the three modes, with flips: within
    test_score_sparse's 1e-12 A of its oracle, the allele counts exact, and the same bytes with the row slices forced
    to one and to several.  Before that every row alone, so that a failure names it."""
    from test_score_sparse import _Case, _tables, _within

    L = gpu_lib
    c = cats(n)
    rng = np.random.default_rng(40 + n)
    order = rng.permutation(c.m).astype(np.uint32)  # a list, not a range: any order
    w9 = rng.normal(size=(c.m, SCORE_COLUMNS[-1])) * 10.0 ** rng.integers(-3, 4, SCORE_COLUMNS[-1])[None, :]
    flip = (rng.random(c.m) < 0.4).astype(np.uint8)
    tiles = {CS.score_tile(min(cols, CS.SCORE_CHUNK) + 1) for cols in SCORE_COLUMNS} | {CS.score_tile(1)}
    assert len(tiles) >= 4
    # first a row alone, one column and nine, with the mean imputed: one term per sample, so test_score_sparse's tables
    # are the oracle (its sums are of one term), and a failure names the designed row
    mode = L.SCORE_MEAN_IMPUTE
    for i in range(c.m):
        one = np.array([i], dtype=np.uint32)
        g = c.codes[i]
        ts, td, inc = _tables(c.codes[i:i + 1], flip[i:i + 1], mode, L)
        allele = np.where(g == 3, inc[0, 1], inc[0, 0]).astype(np.uint32)
        for cols in (1, SCORE_COLUMNS[-1]):
            w = np.ascontiguousarray(w9[i:i + 1, :cols])
            want = ts[0][g][:, None] * w
            bound = 1e-12 * np.abs(w) * np.abs(ts[0]).max()
            for form, sp in c.forms.items():
                ctx = (c.names[i], n, form, cols)
                score, dos, ac = sp.score_sparse(one, w, flip[i:i + 1], mode)
                assert _same_ints(ac, allele), ctx
                assert np.all(np.abs(score - want) <= bound), ctx
                assert np.all(np.abs(dos - td[0][g]) <= 1e-12 * np.abs(td[0]).max()), ctx
    for mode in (L.SCORE_MEAN_IMPUTE, L.SCORE_NO_MEAN_IMPUTATION, L.SCORE_CENTER):
        for cols in SCORE_COLUMNS:
            w = np.ascontiguousarray(w9[:, :cols])
            case = _Case(L, c.codes, order, w, flip, mode, None)
            for form, sp in c.forms.items():
                ctx = (n, form, mode, cols)
                score, dos, ac = sp.score_sparse(order, w, flip, mode)
                assert score.shape == case.score.shape and _same_ints(ac, case.allele), ctx
                _within(score, case.score, case.A[None, :], 1e-12, ctx + ("score",))
                _within(dos, case.dosage, np.float64(case.A_dos), 1e-12, ctx + ("dosage",))
                for slices in ("1", "5"):
                    with pytest.MonkeyPatch.context() as mp:
                        mp.setenv(L.SCORE_SPARSE_SLICES_ENV, slices)
                        sliced = sp.score_sparse(order, w, flip, mode)
                    assert all(a.tobytes() == b.tobytes() for a, b in zip((score, dos, ac), sliced)), ctx + (slices,)


# ---- 3. the linear fits ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", CS.SAMPLE_COUNTS)
def test_linear(gpu_lib, cats, n, k):
    """pgh_glm_sparse and every column of pgh_glm_sparse_multi against glm_oracle at test_glm_sparse's and
    test_glm_sparse_multi's 1e-9, every designed row, in every form; the refused rows by errcode."""
    G = pytest.importorskip("glm_oracle")
    from test_glm_sparse_multi import REL  # 1e-9, the literal of test_glm_sparse's check_rows calls too

    c = cats(n)
    z, ys = c.z(k), c.ys(False)
    zc = z if k else None
    for form, sp in c.forms.items():
        lin = sp.glm_sparse(ys[CS.PHENO_PLAIN], zc)
        seen = {}
        fitted = _row_by_row(c, lambda idx: G.check_rows(lin, c.x, ys[CS.PHENO_PLAIN], z, "linear", rel=REL, idx=idx,
                                                         seen=seen))
        assert {c.names[i]: r["errcode"] for i, r in seen.items() if r["errcode"]} == _refused(0, c.names), (n, k, form)
        assert sum(fitted) == c.m - 6
        multi = sp.glm_sparse_multi(ys, zc)
        assert multi["beta"].shape == (c.m, len(ys))
        for p, y in enumerate(ys):
            col = _col(multi, p)
            fitted = _row_by_row(c, lambda idx: G.check_rows(col, c.x, y, z, "linear", rel=REL, idx=idx))
            assert sum(fitted) >= c.m - 12, (n, k, form, p)


# ---- 4. the score test, its saddlepoint and its Firth estimate ----------------------------------------------------

def _applied_on_both_sides(c, form, state, beyond, what):
    """The follow-up kernels ran their stash paths: the state column says applied for the sparse rows of exactly
    kGlmSparseLong entries (the wave stash full), for the longer sparse rows the form holds (the workgroup's), and for
    the dense-form rows -- for every one of them that the oracle fits with |stat| beyond the cutoff (`beyond`), which
    is all of them but a few."""
    dense = c.dense_form(form)
    full = [i for i in range(c.m) if c.minor[i] == CS.LONG and not dense[i]]
    longer = [i for i in range(c.m) if c.minor[i] > CS.LONG and not dense[i]]
    assert (len(full) > 0) == (form != "default" or c.n == N_WIDE), (what, form)
    assert (len(longer) > 0) == (form == "all" or (form == "default" and c.n == N_WIDE)), (what, form)
    assert (dense.sum() > 0) == (form != "all"), (what, form)
    for group, idx in (("full stash", full), ("longer", longer), ("dense form", np.flatnonzero(dense).tolist())):
        if not idx:
            continue
        got = {c.names[i]: int(state[i]) for i in idx if beyond[i]}
        assert len(got) >= 4 and 4 * len(got) >= 3 * len(idx), (what, form, group, len(got), len(idx))
        assert all(v == 1 for v in got.values()), (what, form, group, got)


def _score_family_by_name(c, rows, spa, firth, nul, forms, rel, tol_spa, tol_firth):
    """The three oracles over one designed row at a time: (fitted, worst score difference, what check_spa saw, what
    check_firth saw), summed over the rows."""
    import glm_firth_sparse_oracle as FS
    import glm_score_oracle as O
    import glm_spa_oracle as S

    score = _row_by_row(c, lambda idx: O.check_rows(rows, c.x, nul, rel=rel, idx=idx))
    seen_spa = _row_by_row(c, lambda idx: S.check_spa(spa, c.x, c.codes, nul, forms, CUTOFF, tol_spa, idx=idx))
    seen_firth = _row_by_row(c, lambda idx: FS.check_firth(firth, c.x, c.codes, nul, forms, CUTOFF, tol_firth, idx=idx))
    total = lambda seen: dict(applied=sum(d["applied"] for d in seen), failed=sum(d["failed"] for d in seen),
                              worst=max(d["worst"] for d in seen))
    return sum(f for f, _ in score), max(w for _, w in score), total(seen_spa), total(seen_firth)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", CS.SAMPLE_COUNTS)
def test_score_test_single(gpu_lib, cats, n, k):
    """pgh_glm_score_sparse at test_glm_score_sparse.REL of glm_score_oracle, then pgh_glm_score_sparse_spa and
    pgh_glm_score_sparse_firth at CUTOFF = 0.1, where nearly every fitted row is applied, against glm_spa_oracle and
    glm_firth_sparse_oracle at those tests' TOL; the rows on both sides of 1,024 entries and the dense-form rows are
    applied (state 1) in fact."""
    from test_glm_score_sparse import REL
    from test_glm_score_sparse_firth import TOL as TOL_FIRTH
    from test_glm_score_sparse_spa import TOL as TOL_SPA

    c = cats(n)
    z, y = c.z(k), c.ys(True)[CS.PHENO_PLAIN]
    zc = z if k else None
    nul = c.nul(k, CS.PHENO_PLAIN)
    assert nul.status is None
    for form, sp in c.forms.items():
        ctx = (n, k, form)
        rows = sp.glm_score_sparse(y, zc)
        assert {c.names[i]: e for i, e in enumerate(rows["errcode"]) if e} == _refused(0, c.names), ctx
        spa = sp.glm_score_sparse_spa(y, zc, cutoff=CUTOFF)
        firth = sp.glm_score_sparse_firth(y, zc, firth_cutoff=CUTOFF)
        for out in (spa, firth):
            _same_bytes({key: out[key] for key in rows}, rows, ctx, c.names)
        fitted, worst, seen_spa, seen_firth = _score_family_by_name(c, rows, spa, firth, nul, c.row_forms[form], REL,
                                                                    TOL_SPA, TOL_FIRTH)
        assert fitted == c.m - 6, ctx
        print(f"{ctx}: score worst {worst:.3g}; saddlepoint {seen_spa['applied']} applied, {seen_spa['failed']} "
              f"failed, worst {seen_spa['worst']:.3g}; Firth {seen_firth['applied']} applied, {seen_firth['failed']} "
              f"failed, worst {seen_firth['worst']:.3g}")
        _applied_on_both_sides(c, form, spa["spa_state"], c.beyond(k, CS.PHENO_PLAIN), "saddlepoint")
        _applied_on_both_sides(c, form, firth["firth_state"], c.beyond(k, CS.PHENO_PLAIN), "Firth")


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", CS.SAMPLE_COUNTS)
def test_score_test_multi(gpu_lib, cats, n, k):
    """The five distinct phenotypes in one call of pgh_glm_score_sparse_multi, _spa and _firth: every column against
    the single-phenotype oracles of its own phenotype, at test_glm_score_sparse_multi.REL and the multi tests' TOL.
    PHENO_PAST_LONG uses 1,024 of the 1,025 entries its row holds: the row is still the workgroup's."""
    from test_glm_score_sparse_multi import REL
    from test_glm_score_sparse_multi_firth import TOL as TOL_FIRTH
    from test_glm_score_sparse_multi_spa import TOL as TOL_SPA

    c = cats(n)
    z, ys = c.z(k), c.ys(True)
    zc = z if k else None
    past = c.at[CS.ROW_PAST_LONG]
    for form, sp in c.forms.items():
        rows = sp.glm_score_sparse_multi(ys, zc)
        spa = sp.glm_score_sparse_multi_spa(ys, zc, spa_cutoff=CUTOFF)
        firth = sp.glm_score_sparse_multi_firth(ys, zc, firth_cutoff=CUTOFF)
        assert rows["beta"].shape == (c.m, len(ys))
        for out in (spa, firth):
            _same_bytes({key: out[key] for key in rows}, rows, (n, k, form), c.names)
        for p in range(len(ys)):
            ctx = (n, k, form, p)
            nul = c.nul(k, p)
            fitted, worst, seen_spa, seen_firth = _score_family_by_name(
                c, _col(rows, p), _col(spa, p), _col(firth, p), nul, c.row_forms[form], REL, TOL_SPA, TOL_FIRTH)
            assert fitted >= c.m - 12, ctx
            print(f"{ctx}: score worst {worst:.3g}; saddlepoint {seen_spa['applied']} applied, worst "
                  f"{seen_spa['worst']:.3g}; Firth {seen_firth['applied']} applied, worst {seen_firth['worst']:.3g}")
            if p == CS.PHENO_PLAIN:
                _applied_on_both_sides(c, form, spa["spa_state"][:, p], c.beyond(k, p), "saddlepoint")
                _applied_on_both_sides(c, form, firth["firth_state"][:, p], c.beyond(k, p), "Firth")
        # the row holds 1,025 entries and uses 1,024 of them: held sparse it is still the workgroup's (every row is
        # sparse under "all"), and in any form the follow-ups are applied to it
        assert c.minor[past] == CS.LONG + 1 and (form != "all" or not c.dense_form(form)[past])
        assert spa["spa_state"][past, CS.PHENO_PAST_LONG] == 1 and firth["firth_state"][past, CS.PHENO_PAST_LONG] == 1


# ---- 5. the variant sets -----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", CS.SAMPLE_COUNTS)
def test_sets(gpu_lib, cats, n):
    """pgh_burden_sparse against test_burden_sparse's oracle at its 1e-9 and pgh_skat_sparse against skat_oracle at
    test_skat_sparse's tolerances: a set per designed row, every tile1 row together, the four base codes together and
    a long row twice, weighted, with two covariates."""
    import test_skat_sparse as TS
    from test_burden_sparse import _check as burden_check, _csr, _expected as burden_expected, _Forms

    L = gpu_lib
    c = cats(n)
    labels, sets = CS.variant_sets(c.names)
    off, vidx = _csr(sets)
    rng = np.random.default_rng(50 + n)
    w = rng.uniform(0.25, 25.0, len(vidx)) * np.where(rng.random(len(vidx)) < 0.2, -1.0, 1.0)
    z = c.z(2)
    y_lin, y_bin = c.ys(False)[CS.PHENO_PLAIN], c.ys(True)[CS.PHENO_PLAIN]
    for form, sp in c.forms.items():
        ctx = (n, form)
        forms = _Forms(c.codes, max_minor_of(form, n), c.pitch)
        assert np.array_equal(forms.dense, c.dense_form(form)), ctx
        burden = sp.burden_sparse(y_lin, off, vidx, w, z)
        expected = burden_expected(c.codes, forms, sets, w, y_lin, z)
        assert sum(e["errcode"] is None for e in expected) == len(sets) - 6, ctx
        for s, label in enumerate(labels):  # a set at a time, so that a failure names the set
            burden_check(L, burden[s:s + 1], expected[s:s + 1], ctx=(label, ctx))
        skat, lam = sp.skat_sparse(y_bin, off, vidx, w, z, return_lambda=True)
        want = TS.expected(types.SimpleNamespace(codes=c.codes), forms, sets, w, y_bin, z)
        assert sum(e["errcode"] is None for e, _ in want) == len(sets) - 6, ctx
        for s, label in enumerate(labels):
            TS.check(L, skat[s:s + 1], lam, want[s:s + 1], off[s:s + 2], ctx=(label, ctx))


# ---- 6. the order of a row's sums is a function of the row alone --------------------------------------------------

def _multi_calls(sp):
    return {
        "glm_sparse_multi": (False, lambda y, z, **kw: sp.glm_sparse_multi(y, z, **kw)),
        "glm_score_sparse_multi": (True, lambda y, z, **kw: sp.glm_score_sparse_multi(y, z, **kw)),
        "glm_score_sparse_multi_spa":
            (True, lambda y, z, **kw: sp.glm_score_sparse_multi_spa(y, z, spa_cutoff=CUTOFF, **kw)),
        "glm_score_sparse_multi_firth":
            (True, lambda y, z, **kw: sp.glm_score_sparse_multi_firth(y, z, firth_cutoff=CUTOFF, **kw)),
    }


def _single_calls(sp):
    return {
        "glm_sparse": (False, lambda y, z, **kw: sp.glm_sparse(y, z, **kw)),
        "glm_score_sparse": (True, lambda y, z, **kw: sp.glm_score_sparse(y, z, **kw)),
        "glm_score_sparse_spa": (True, lambda y, z, **kw: sp.glm_score_sparse_spa(y, z, cutoff=CUTOFF, **kw)),
        "glm_score_sparse_firth": (True, lambda y, z, **kw: sp.glm_score_sparse_firth(y, z, firth_cutoff=CUTOFF, **kw)),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("n", CS.SAMPLE_COUNTS)
def test_a_row_does_not_depend_on_its_neighbours_the_block_or_the_chunk(gpu_lib, cats, n):
    """include/pgenhip.h and glm_lanes.hpp: a row of a multi entry point is a function of its entries, its phenotype
    and the covariates, bit for bit.  Within one form the bytes of a row stay when the range starts one, two or three
    rows later (other rows share its wave or workgroup), when the block holds 3, 5 or 67 phenotypes (phenotype j of a
    block is distinct phenotype j % 5, so a column must equal the column of its phenotype wherever it stands), and
    when the scratch budget cuts the call into chunks of one variant.  The single-phenotype entry points promise the
    same of v_begin and of the rows around a row: the same check over shifted ranges and over the range in parts."""
    from test_glm_score_sparse_multi import SCRATCH_ENV

    c = cats(n)
    z = c.z(2)
    cut = c.at["E1024_tile0"] + 1  # a part ends between the rows at the split
    for form, sp in c.forms.items():
        for name, (binary, call) in _multi_calls(sp).items():
            ctx = (n, form, name)
            five = c.ys(binary)
            whole = call(five, z)
            for shift in (1, 2, 3):
                _same_bytes(call(five, z, v_begin=shift), _rows(whole, slice(shift, None)), ctx + ("shift", shift),
                            c.names[shift:])
            for count in CS.BLOCK_COUNTS:
                block = call(CS.phenotype_block(n, count, binary), z)
                want = {key: v[:, np.arange(count) % 5] for key, v in whole.items()}
                _same_bytes(block, want, ctx + ("phenotypes", count), c.names)
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv(SCRATCH_ENV, "1")
                _same_bytes(call(five[:3], z), {key: v[:, :3] for key, v in whole.items()}, ctx + ("chunks of one",),
                            c.names)
        for name, (binary, call) in _single_calls(sp).items():
            ctx = (n, form, name)
            y = c.ys(binary)[CS.PHENO_PLAIN]
            whole = call(y, z)
            for shift in (1, 2, 3):
                _same_bytes(call(y, z, v_begin=shift), _rows(whole, slice(shift, None)), ctx + ("shift", shift),
                            c.names[shift:])
            for lo, hi in ((0, cut), (cut, c.m)):
                _same_bytes(call(y, z, v_begin=lo, v_end=hi), _rows(whole, slice(lo, hi)), ctx + ("part", lo, hi),
                            c.names[lo:hi])
