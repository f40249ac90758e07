"""Every entry point that reads the resident dosage tracks, under the structured tracks of tests/dosage_shapes.py.

The catalogue puts a track's entries on the hard edges of dosage.hip: the sixteen values k_score_dosage_fix preloads
per word, the 512 records k_score_dosage_records fetches at a time, the 2/5 cut between the explicit-entry kernels and
the sample-owning ones, a full track but for one sample, a full track that ends the value run, entries on missing
calls only, the values 0, 16384 and 32768 under every call, and lists of 1, 63 .. 129 rows of one class (the kernels
stage 128 and 64 variants' constants at a time).  One file per sample count, every row in the three track encodings,
written without and with phase tracks in front.

The reference of every output is the catalogue's own arrays restated in NumPy float64 (DS.values, DS.moments), fed to
oracle.score, glm_score_oracle and glm_oracle; integer outputs are compared with np.array_equal and every floating
comparison takes the constant the entry point's own test file uses; none is introduced here."""

import re

import numpy as np
import pytest

import dosage_shapes as DS
import pgen_writer as W
import subset_shapes as SS

N_TILE, N_WIDE = DS.N_TILE, DS.N_WIDE
SMALL_COUNTS = DS.TINY_COUNTS + DS.ID_COUNTS
ALL_COUNTS = DS.SAMPLE_COUNTS + SMALL_COUNTS + (DS.N_IDS3,)
ROW_COUNTS = {N_TILE: 77, N_WIDE: 95}
CLASS_NAMES = {DS.HARD: "hard", DS.SPARSE: "sparse", DS.GAPS: "gaps", DS.FULL: "full"}
LIST_COUNTS = (1, 63, 64, 65, 127, 128, 129)
ROUTES = {"records": None, "bitwalk": ("PGH_SCORE_DOSAGE_RECORDS", "0"), "lanes": ("PGH_SCORE_DOSAGE_LANES", "1")}
MODES = (("default", "SCORE_MEAN_IMPUTE"), ("no_mean_imputation", "SCORE_NO_MEAN_IMPUTATION"), ("center", "SCORE_CENTER"))
GLM_KS = (0, 3)
# the rows the regression oracles refuse under every phenotype: nothing to regress on, or nobody observed
REFUSED = {"E0_ref": "CONST_ALLELE", "E0_missing": "TOO_FEW_SAMPLES"}
# ... and the tracks a logistic fit without Firth cannot take: one carrier over an all-hom-ref row is fitted exactly as
# beta goes to infinity.  (The score test and the linear fit take them.)
LOGISTIC_UNFIT = {"E1_tile0_ref": "NO_CONVERGENCE", "E1_last_ref": "NO_CONVERGENCE"}


def _layout(n, _made={}):
    if n not in _made:
        _made[n] = DS.Layout(n)
    return _made[n]


# ---- the catalogue itself (no GPU) -------------------------------------------------------------------------------

def _spec(n, name):
    """(entry count, first entry sample, last entry sample, background, class) of a wide row, from its name alone --
    written out independently of dosage_shapes.rows().  None: not pinned by the name."""
    lo, hi = (1638, 1639) if n == 4096 else (3303, 3304)
    words, missing = (n + 63) // 64, None

    def cls(e):
        return DS.FULL if e == n else DS.GAPS if e >= hi else DS.SPARSE

    m = re.fullmatch(r"E(\d+)_(tile0|tile1|last|spread)_(ref|common|het)", name)
    if m:
        e, where, bg = int(m.group(1)), m.group(2), m.group(3)
        first = {"tile0": 0, "tile1": 4096, "last": n - e, "spread": 0}[where]
        last = {"tile0": e - 1, "tile1": 4095 + e, "last": n - 1, "spread": (e - 1) * n // e}[where]
        return e, first, last, bg, cls(e)
    m = re.fullmatch(r"E0_(ref|common|missing)", name)
    if m:
        return 0, None, None, m.group(1), DS.SPARSE
    m = re.fullmatch(r"phase_het(\d+)", name)
    if m:
        return 100, 0, 99 * n // 100, "common", DS.SPARSE
    full_words = n // 64
    return {
        "word64_only": (64, 320, 383, "ref", DS.SPARSE),
        "one_per_word": (words, 0, None, "ref", DS.SPARSE),
        "word16": (16 * full_words, 0, None, "ref", DS.SPARSE),
        "word17": (17 * full_words, 0, None, "ref", DS.SPARSE),
        "tile_gap": (44, 0, n - 1, "ref", DS.SPARSE),
        "boundaries": (2 * full_words + (2 if n % 64 else 0), 0, n - 1, "common", DS.SPARSE),
        "val0": (600, 0, 599 * n // 600, "common", DS.SPARSE),
        "val16384": (600, 0, 599 * n // 600, "common", DS.SPARSE),
        "val32768": (600, 0, 599 * n // 600, "common", DS.SPARSE),
        "val_cycle": (24, None, None, "common", DS.SPARSE),
        "all_on_missing": (missing, None, None, "common", DS.SPARSE),
        "none_on_missing": (500, None, None, "common", DS.SPARSE),
        "full_over_allmissing": (n, 0, n - 1, "missing", DS.FULL),
        "restated_gaps": (missing, None, None, "common", DS.GAPS),
        "restated_sparse": (300, None, None, "common", DS.SPARSE),
        "restated_full": (n, 0, n - 1, "common", DS.FULL),
    }[name]


def _check_background(hard, bg, name):
    if bg == "common":
        share = np.bincount(hard, minlength=4) / len(hard)
        assert share[:3].min() > 0.05 and 0.01 < share[3] < 0.06, (name, share)
    else:
        assert (hard == {"ref": 0, "het": 1, "missing": 3}[bg]).all(), name


def test_the_catalogue_is_what_the_kernels_are_meant_to_see():
    """The entry count, the placement, the background under the entries and the class under the plan's rule of every
    row are what its name says, and the rows that are aimed at one edge sit on it."""
    assert (DS.WORD, DS.TILE, DS.REC_FETCH, DS.ENTRY_STAGE, DS.LANE_STAGE, DS.CUT_NUM, DS.CUT_DEN) == \
        (64, 4096, 512, 128, 64, 2, 5)
    assert (N_TILE, N_WIDE) == (4096, 8259) and N_WIDE % 64 == 3
    assert [DS.cut_counts(n) for n in DS.SAMPLE_COUNTS] == [(1638, 1639), (3303, 3304)]
    for n in DS.SAMPLE_COUNTS:
        cat = DS.rows(n)
        assert len(cat) == ROW_COUNTS[n] and list(cat)[-1] == f"E{n}_tile0_ref"
        lo, hi = DS.cut_counts(n)
        assert lo * 5 < 2 * n <= hi * 5 and hi == lo + 1
        for name, (hard, dos) in cat.items():
            assert hard.dtype == np.uint8 and dos.dtype == np.uint16 and hard.shape == dos.shape == (n,), name
            assert hard.max() <= 3 and dos[dos != DS.NONE].max(initial=0) <= 32768, name
            count, first, last, bg, cls = _spec(n, name)
            at = np.flatnonzero(dos != DS.NONE)
            if count is not None:
                assert len(at) == count, (n, name, len(at))
            if first is not None:
                assert int(at[0]) == first, (n, name)
            if last is not None:
                assert int(at[-1]) == last, (n, name)
            assert DS.track_class(len(at), n) == cls, (n, name)
            if not name.startswith("phase_het") and name != "restated_full":
                _check_background(hard, bg, name)
            if re.fullmatch(r"E\d+_(tile0|tile1|last)_\w+", name):
                assert np.array_equal(at, np.arange(first, last + 1)), (n, name)
        # every count in every placement that fits
        for e in DS.entry_counts(n)[1:-1]:
            fits = [w for w in DS.PLACEMENTS if f"E{e}_{w}_{DS.BACKGROUND_OF[w]}" in cat]
            want = ["tile0"] + (["tile1"] if 4096 + e <= n else []) + ["last"] + (["spread"] if 2 * e <= n else [])
            assert fits == want, (n, e, fits)
        assert {0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 511, 512, 513, 1023, 1024, 1025, lo, hi, n - 1, n} == \
            set(DS.entry_counts(n))
        # the cut pair falls on the two sides of the cut, full-minus-one is not full
        assert DS.track_class(lo, n) == DS.SPARSE and DS.track_class(hi, n) == DS.GAPS
        assert DS.track_class(n - 1, n) == DS.GAPS and DS.track_class(n, n) == DS.FULL
        # the word-fill rows
        fills = {name: DS.word_fills(cat[name][1]) for name in ("word64_only", "one_per_word", "word16", "word17")}
        assert fills["word64_only"].tolist() == [64 if w == 5 else 0 for w in range((n + 63) // 64)]
        assert (fills["one_per_word"] == 1).all()
        ragged = n % 64 > 0
        for fill in (16, 17):
            f = fills[f"word{fill}"]
            assert (f[:n // 64] == fill).all() and (not ragged or f[-1] == 0)
        if n > 2 * 4096:
            runs = DS.tile_runs(cat["tile_gap"][1])
            assert runs[0] > 0 and runs[1] == 0 and runs[2] == 3 and cat["tile_gap"][1][n - 1] != DS.NONE
        edge = cat["boundaries"][1] != DS.NONE
        for s in range(64, n, 64):
            assert edge[s - 1] and edge[s], (n, s)
        assert edge[0] and edge[n - 1] and all(edge[t - 1] and edge[t] for t in range(4096, n, 4096))
        # the value rows
        for value in (0, 16384, 32768):
            hard, dos = cat[f"val{value}"]
            assert (dos[dos != DS.NONE] == value).all()
            assert {int(c) for c in hard[dos != DS.NONE]} == {0, 1, 2, 3}, "the value meets every call"
        hard, dos = cat["val_cycle"]
        met = {(int(c), int(v)) for c, v in zip(hard[dos != DS.NONE], dos[dos != DS.NONE])}
        assert met == {(c, v) for c in range(4) for v in (0, 16384, 32768)}
        # the missing-call rows
        hard, dos = cat["all_on_missing"]
        assert np.array_equal(dos != DS.NONE, hard == 3) and (hard == 3).sum() > 64
        hard, dos = cat["none_on_missing"]
        assert not ((dos != DS.NONE) & (hard == 3)).any() and (hard == 3).sum() > 64
        for name in ("restated_gaps", "restated_sparse", "restated_full"):
            hard, dos = cat[name]
            have = dos != DS.NONE
            assert np.array_equal(dos[have], hard[have].astype(np.uint16) * 16384) and not (hard[have] == 3).any()
        hard, dos = cat["restated_gaps"]
        assert np.array_equal(dos != DS.NONE, hard != 3) and (hard == 3).any()
        assert not (cat["restated_full"][0] == 3).any()
        for hets in DS.PHASE_HETS:
            hard, dos = cat[f"phase_het{hets}"]
            assert int((hard == 1).sum()) == hets and (1 + hets) % 8 in (1, 0)
        assert (cat["E64_spread_het"][0] == 1).all()
    for n in SMALL_COUNTS:
        cat = DS.small_rows(n)
        assert f"E{n}_tile0_common" == list(cat)[-1]
        for name, (hard, dos) in cat.items():
            at = np.flatnonzero(dos != DS.NONE)
            m = re.fullmatch(r"E(\d+)_(tile0|last)_common", name)
            if m:
                e = int(m.group(1))
                want = np.arange(e) if m.group(2) == "tile0" else n - e + np.arange(e)
                assert np.array_equal(at, want), (n, name)
        assert {f"E{n - 1}_tile0_common", f"E{n - 1}_last_common"} <= set(cat) or n == 1
        assert (cat["full_over_allmissing"][0] == 3).all() and (cat["full_over_allmissing"][1] != DS.NONE).all()
    cat = DS.ids3_rows()
    assert len(cat) == 12 and W._id_bytes(DS.N_IDS3) == 3 and [W._id_bytes(n) for n in DS.ID_COUNTS] == [1, 2]
    for name, (hard, dos) in cat.items():
        e = int(re.fullmatch(r"E(\d+)_(spread|last)_common", name).group(1))
        at = np.flatnonzero(dos != DS.NONE)
        assert len(at) == e and (not name.endswith("last_common") or at[0] == DS.N_IDS3 - e)
    assert {64, 65, 128, 129} <= {int((d != DS.NONE).sum()) for _, d in cat.values()}, "the difflist group steps"


def test_the_files_cover_the_offsets_runs_and_fills():
    """The value offsets k_dosage_offsets assigns -- the running sum of the entry counts in file order -- take all eight
    residues mod 8 among the rows with entries (k_dosage_sums streams from o0 & ~7); a full row is the last track of
    its file; the (row, tile) runs hold 511 .. 1025 records and the words 0, 1, 16, 17 and 64 entries; every
    encoding and track-less neighbours on both sides of a track occur."""
    for n in DS.SAMPLE_COUNTS:
        lay = _layout(n)
        assert lay.m == 4 * ROW_COUNTS[n] and sorted(set(lay.kinds.tolist())) == [0, 0x20, 0x40, 0x60]
        tracks = np.flatnonzero(lay.kinds != 0)
        off = np.concatenate([[0], np.cumsum(lay.have[tracks])])
        assert {int(o) % 8 for o, e in zip(off[:-1], lay.have[tracks]) if e} == set(range(8)), n
        assert lay.cls[tracks[-1]] == DS.FULL and tracks[-1] == lay.m - 1, "a full row ends the value run"
        runs, fills = set(), set()
        for hard, dos in DS.rows(n).values():
            if DS.track_class(int((dos != DS.NONE).sum()), n) == DS.SPARSE:  # the rows that have entry records
                runs |= set(DS.tile_runs(dos))
            fills |= set(DS.word_fills(dos).tolist())
        assert {511, 512, 513, 1023, 1024, 1025} <= runs and {0, 1, 16, 17, 64} <= fills, n
        left = {(int(lay.kinds[v - 1]) == 0) for v in tracks if v}
        right = {(int(lay.kinds[v + 1]) == 0) for v in tracks if v + 1 < lay.m}
        assert left == right == {False, True}
        # every class in numbers that the lists of one class can be drawn from
        assert [int((lay.cls == c).sum()) >= 9 for c in range(4)] == [True] * 4
        assert int((lay.cls == DS.SPARSE).sum()) >= max(LIST_COUNTS)
    for n in SMALL_COUNTS:
        lay = _layout(n)
        assert lay.cls[-1] == DS.FULL and {DS.HARD, DS.SPARSE, DS.FULL} <= set(lay.cls.tolist())
    assert set(_layout(DS.N_IDS3).kinds.tolist()) == {0, 0x20}


def test_the_record_order_is_round_major():
    dos = np.full(4096, DS.NONE, dtype=np.uint16)
    dos[[0, 1, 2, 64, 65, 130]] = 7
    assert DS.record_order(dos, 0).tolist() == [0, 64, 130, 1, 65, 2]


# ---- what a subtly wrong kernel would compute: the catalogue tells them apart (CPU only) --------------------------

def _mutated(n, hard, dos, what):
    """The value row a kernel with one fault would see."""
    hard, dos = hard.copy(), dos.copy()
    have = np.flatnonzero(dos != DS.NONE)
    if what == "17th value of a word from the 16th":
        word = have // 64
        nth = np.arange(len(have)) - np.searchsorted(word, word)
        dos[have[nth == 16]] = dos[have[np.flatnonzero(nth == 16) - 1]]
    elif what == "513th record of a run dropped":
        if DS.track_class(len(have), n) == DS.SPARSE:
            for tile in range((n + 4095) // 4096):
                order = DS.record_order(dos, tile)
                if len(order) > 512:
                    dos[order[512]] = DS.NONE
    elif what == "entry on a missing call still missing":
        dos[have[hard[have] == 3]] = DS.NONE
    elif what == "full minus one treated as full":
        if len(have) == n - 1:
            run = np.concatenate([dos[have], [0]])
            dos = run.astype(np.uint16)
    elif what == "32768 read as 0":
        dos[dos == 32768] = 0
    else:
        raise ValueError(what)
    return DS.values(hard, dos)


MUTATIONS = ("17th value of a word from the 16th", "513th record of a run dropped",
             "entry on a missing call still missing", "full minus one treated as full", "32768 read as 0")


@pytest.mark.parametrize("what", MUTATIONS)
def test_the_catalogue_tells_a_faulty_kernel_apart(what):
    """Each fault changes the expected values of at least one catalogue row at each wide sample count, so the GPU
    assertions against DS.values are not vacuous for it."""
    for n in DS.SAMPLE_COUNTS:
        hit = [name for name, (hard, dos) in DS.rows(n).items()
               if not np.array_equal(_mutated(n, hard, dos, what), DS.values(hard, dos))]
        assert hit, (n, what)
        if what == "full minus one treated as full":
            # (the row whose one gap is the last sample reads a zero there: its hom-ref call in other words)
            assert hit == [f"E{n - 1}_last_ref"]
        if what == "513th record of a run dropped":
            assert {"E513_tile0_ref", "E1025_tile0_ref"} <= set(hit)
        if what == "entry on a missing call still missing":
            assert {"all_on_missing", "full_over_allmissing", "val_cycle"} <= set(hit)


# ---- the files ---------------------------------------------------------------------------------------------------

class _File:
    def __init__(self, tmp, n, with_phase):
        self.lay = lay = _layout(n)
        self.n, self.with_phase = n, with_phase
        self.path = str(tmp / f"shapes_{n}_{int(with_phase)}.pgen")
        kinds = W.choose_kinds(lay.hard, np.random.default_rng(n))
        W.write_pgen(self.path, lay.hard, kinds, dosage=lay.dos, dosage_kinds=lay.kinds.tolist(),
                     phase_rng=np.random.default_rng(n + 1) if with_phase else None)
        self.x = DS.values(lay.hard, lay.dos)
        self._made = {}

    def once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def ds(self, L):
        return self.once("ds", lambda: L.Dataset.open(self.path))

    def pg(self, oracle):
        return self.once("pg", lambda: oracle.Pgen(self.path))

    def moments(self, mask_name="all"):
        return self.once(("moments", mask_name), lambda: DS.moments(self.x[:, self.masks()[mask_name]]))

    def masks(self):
        return self.once("masks", lambda: _masks(self.lay))


def _masks(lay):
    """name -> bool[n]: everyone, a word-aligned half, every other sample, masks that drop exactly the samples that
    hold a row's entries, and subset_shapes' own."""
    n = lay.n
    s = np.arange(n)
    out = {"all": np.ones(n, dtype=bool), "every_other": s % 2 == 0}
    if n in DS.SAMPLE_COUNTS:
        out["half_words"] = s < 64 * ((n + 63) // 128)
        for name in ("boundaries", "E513_tile0_ref"):
            out["drop_" + name] = lay.dos[lay.variants(name, 0x60)[0]] == DS.NONE
        shapes = SS.shapes(n)
        out.update({k: shapes[k] for k in ("all_but_one", "last_word", "stride4")})
    elif n > 1:
        out["all_but_first"] = s > 0
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dosage_shapes")
    made = {}

    def get(n, with_phase=False):
        if (n, with_phase) not in made:
            made[n, with_phase] = _File(tmp, n, with_phase)
        return made[n, with_phase]

    yield get
    for f in made.values():
        if "ds" in f._made:
            f._made["ds"].close()


@pytest.mark.parametrize("with_phase", [False, True])
@pytest.mark.parametrize("n", ALL_COUNTS)
def test_oracle_reads_the_written_tracks(files, oracle, n, with_phase):
    """The oracle reads every written file back to the catalogue's values: the writer is honest."""
    f = files(n, with_phase)
    lay = f.lay
    pg = f.pg(oracle)
    assert pg.has_dosage and pg.has_phase == (with_phase and bool((lay.hard == 1).any()))
    for v in range(lay.m):
        assert pg.vrtype(v) & 0x60 == lay.kinds[v], (n, v)
        assert bool(pg.vrtype(v) & 0x10) == (with_phase and bool((lay.hard[v] == 1).any())), (n, v)
        assert np.array_equal(pg.dosage(v), f.x[v]), (n, lay.names[v], hex(lay.kinds[v]))


# ---- the regression inputs and which rows the oracles refuse (no GPU) ---------------------------------------------

def _glm_inputs(n, k):
    """(Z, Y): k covariates and the five phenotypes of test_glm_score_multi_dosage.PHENO_SPECS."""
    from test_glm_score_multi_dosage import _covariates, _phenotypes

    rng = np.random.default_rng(7000 + n + k)
    Z = _covariates(rng, k, n)
    return Z, _phenotypes(rng, n, Z)


def _linear_inputs(n, k):
    rng = np.random.default_rng(7100 + n + k)
    Z = rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]
    Y = 0.3 * (Z.sum(axis=0) if k else 0.0) + rng.normal(size=(3, n))
    Y[rng.random((3, n)) < 0.03] = np.nan
    return Z, Y


def _glm_test_inputs(n, model):
    """test_glm's (Z, Y): two covariates; three quantitative phenotypes, or the first and fourth of PHENO_SPECS."""
    if model == "linear":
        return _linear_inputs(n, 2)
    Z, Y = _glm_inputs(n, 2)
    return Z, Y[[0, 3]]


def _distinct_rows(lay, x):
    """(rows, of): the distinct value rows of the file and, per variant, which of them it holds -- the three encodings
    of a row are one row to an oracle."""
    seen, rows, of = {}, [], []
    for v in range(lay.m):
        key = x[v].tobytes()
        if key not in seen:
            seen[key] = len(rows)
            rows.append(v)
        of.append(seen[key])
    return rows, np.array(of)


def _may_be_refused(lay, v, in_s):
    """A row the numeric comparison may leave out: not of the common background, and fewer than two distinct values
    among the phenotype's samples."""
    name = lay.names[v]
    common = re.search(r"_common$", name) or name in (
        "boundaries", "val0", "val16384", "val32768", "val_cycle", "all_on_missing", "none_on_missing", "restated_gaps",
        "restated_sparse", "restated_full") or name.startswith("phase_het")
    x = DS.values(lay.hard[v], lay.dos[v])[in_s]
    return not common and len(np.unique(x[x != -9.0])) < 2


@pytest.mark.parametrize("k", GLM_KS)
@pytest.mark.parametrize("n", DS.SAMPLE_COUNTS)
def test_the_score_oracle_fits_every_row_but_the_refused_ones(n, k):
    """glm_score_oracle fits every row under the five phenotypes except REFUSED, whose errcodes are pinned by name, and
    rows off the common background that hold fewer than two distinct values among the phenotype's samples."""
    import glm_score_oracle as O

    lay = _layout(n)
    x = DS.values(lay.hard, lay.dos)
    rows, of = _distinct_rows(lay, x)
    Z, Y = _glm_inputs(n, k)
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        assert nul.status is None, (n, k, p)
        codes = [O.oracle_row(x[v], nul)["errcode"] for v in rows]
        for v, code in zip(rows, codes):
            name = lay.names[v]
            if name in REFUSED:
                assert code == REFUSED[name], (n, k, p, name, code)
            elif code is not None:
                assert _may_be_refused(lay, v, nul.in_s), (n, k, p, name, code)
        assert sum(c is None for c in codes) >= len(rows) - 12, (n, k, p)


@pytest.mark.parametrize("model", ["linear", "logistic"])
@pytest.mark.parametrize("n", DS.SAMPLE_COUNTS)
def test_the_glm_oracle_fits_every_row_but_the_refused_ones(n, model):
    """glm_oracle under test_glm's inputs: the rows left out of the numeric comparison are REFUSED, rows off the common
    background with fewer than two distinct values among the phenotype's samples, and, for the logistic fit without
    Firth, the tracks of LOGISTIC_UNFIT with exactly that code -- nothing else, and no row of the common background."""
    import glm_oracle as G

    lay = _layout(n)
    x = DS.values(lay.hard, lay.dos)
    rows, of = _distinct_rows(lay, x)
    Z, Y = _glm_test_inputs(n, model)
    for p, y in enumerate(Y):
        in_s = ~np.isnan(y)
        unfit = {}
        for v in rows:
            code = G.oracle_row(x[v], y, Z, model, False)["errcode"]
            if code is not None and not (lay.names[v] in REFUSED or _may_be_refused(lay, v, in_s)):
                unfit[lay.names[v]] = code
                assert lay.kinds[v], (n, model, p, lay.names[v])
        assert unfit == (LOGISTIC_UNFIT if model == "logistic" else {}), (n, model, p, unfit)


# ---- on the GPU --------------------------------------------------------------------------------------------------

def _same_ints(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _by_name(lay, got, want, ctx):
    """np.array_equal over the variants, a failure naming the designed rows."""
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        raise AssertionError((ctx, [(lay.names[v], hex(int(lay.kinds[v]))) for v in bad[:8]]))


# ---- 1. ingest ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("with_phase", [False, True])
@pytest.mark.parametrize("n", ALL_COUNTS)
def test_ingest(gpu_lib, files, n, with_phase, monkeypatch):
    """pgh_open's device decode and the host parser of the same tracks: dosage_unpack() equals the catalogue bit for
    bit for every (row, encoding), the counts of the info are exact, the hardcall tallies are untouched, and a dataset
    opened just before and just after a full row and an empty track holds the same rows."""
    f = files(n, with_phase)
    lay = f.lay
    ds = f.ds(gpu_lib)
    counts = SS.counts_ref(lay.hard)
    monkeypatch.setenv("PGH_HOST_NORMALIZE", "1")
    hosted = gpu_lib.Dataset.open(f.path)
    monkeypatch.delenv("PGH_HOST_NORMALIZE")
    for how, d in (("device", ds), ("host", hosted)):
        ctx = (n, with_phase, how)
        _by_name(lay, d.dosage_unpack(), f.x, ctx)
        assert d.info.dosage_variant_ct == int((lay.kinds != 0).sum()), ctx
        assert d.info.dosage_value_ct == int(lay.have.sum()), ctx
        _by_name(lay, d.counts_range(), counts, ctx)
        _by_name(lay, d.dosage_sums(), f.moments(), ctx)
    hosted.close()
    full = lay.variants("restated_full" if n in DS.SAMPLE_COUNTS else f"E{n}_tile0_common", 0x20)[0] \
        if n != DS.N_IDS3 else lay.variants("E129_spread_common", 0x20)[0]
    empty = lay.variants("E0_common", 0x60)[0] if n != DS.N_IDS3 else lay.variants("E0_spread_common", 0x20)[0]
    for lo in (full, full + 1, empty, empty + 1):
        hi = min(lay.m, max(lo + 1, lay.m - 3 if lo >= full else lo + 41))
        part = gpu_lib.Dataset.open(f.path, variant_begin=lo, variant_end=hi)
        assert np.array_equal(part.dosage_unpack(), f.x[lo:hi]), (n, with_phase, lo, hi)
        assert _same_ints(part.dosage_sums(), f.moments()[lo:hi]), (n, with_phase, lo, hi)
        part.close()


# ---- 2. and 3. the moments and the unpacked values ---------------------------------------------------------------

def _picks(lay):
    """A gapped list in no order that starts with the file's last track (a full row) and holds every fourth variant."""
    return np.array([lay.m - 1, 0] + list(range(3, lay.m - 1, 4)) + [2, 1], dtype=np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ALL_COUNTS)
def test_dosage_sums(gpu_lib, files, n):
    """pgh_dosage_sums and pgh_dosage_sums_dev equal the integer moments exactly: without a subset (the streamed value
    run) and with one (the rank walk), over the whole range, a sub-range and a list."""
    import torch

    from test_device_entry_points import Guarded

    f = files(n)
    lay, ds = f.lay, f.ds(gpu_lib)
    pick = _picks(lay)
    lo, hi = 5, lay.m - 2
    st = torch.cuda.current_stream().cuda_stream
    for name, mask in f.masks().items():
        ss = None if name == "all" else ds.subset(mask)
        want = f.moments(name)
        ctx = (n, name)
        _by_name(lay, ds.dosage_sums(subset=ss), want, ctx)
        assert _same_ints(ds.dosage_sums(lo, hi, subset=ss), want[lo:hi]), ctx
        assert _same_ints(ds.dosage_sums(vidx=pick, subset=ss), want[pick]), ctx
        whole, part = Guarded(24 * lay.m), Guarded(24 * (hi - lo))
        ds.dosage_sums_dev(0, lay.m, whole.ptr, st, subset=ss)
        ds.dosage_sums_dev(lo, hi, part.ptr, st, subset=ss)
        torch.cuda.synchronize()
        whole.check(want)
        part.check(want[lo:hi])
        if name == "all":  # the same through a subset that keeps everyone: the other kernel
            everyone = ds.subset(mask)
            _by_name(lay, ds.dosage_sums(subset=everyone), want, ctx + ("subset of everyone",))
            everyone.close()
        if ss is not None:
            ss.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", ALL_COUNTS)
def test_dosage_unpack(gpu_lib, files, n):
    """pgh_dosage_unpack, pgh_dosage_unpack_dev, pgh_dosage_unpack_samples and the reader's pgh_get_dosage_f64, bit
    for bit, with and without the subsets, range and list forms."""
    import torch

    from test_device_entry_points import Guarded

    f = files(n)
    lay, ds = f.lay, f.ds(gpu_lib)
    pick = _picks(lay)
    lo, hi = 5, lay.m - 2
    st = torch.cuda.current_stream().cuda_stream
    for name, mask in f.masks().items():
        ss = None if name == "all" else ds.subset(mask)
        want = f.x[:, mask]
        n_out = want.shape[1]
        ctx = (n, name)
        _by_name(lay, ds.dosage_unpack(subset=ss), want, ctx)
        assert np.array_equal(ds.dosage_unpack(lo, hi, subset=ss), want[lo:hi]), ctx
        assert np.array_equal(ds.dosage_unpack(vidx=pick, subset=ss), want[pick]), ctx
        assert np.array_equal(ds.dosage_unpack_samples(pick, subset=ss), want[pick].T), ctx
        stride = n_out + 3
        g = Guarded(8 * (hi - lo) * stride)
        ds.dosage_unpack_dev(lo, hi, g.ptr, stride, st, subset=ss)
        torch.cuda.synchronize()
        img = g.image().view(np.float64).reshape(hi - lo, stride)
        img[:, :n_out] = want[lo:hi]
        g.check(img)
        rd = ds.reader(ss)
        step = 1 if name == "all" or n not in DS.SAMPLE_COUNTS else 3
        for v in range(0, lay.m, step):
            assert np.array_equal(rd.get_dosage_f64(v), want[v]), (ctx, lay.names[v], hex(int(lay.kinds[v])))
        rd.close()
        if ss is not None:
            ss.close()


# ---- 4. plink_score ----------------------------------------------------------------------------------------------

def _score_lists(lay):
    """name -> variant list.  The whole file, each class alone, 1 .. 129 rows of one class alone and among rows of the
    other classes (a class with fewer rows than that is cycled through: a list may name a track again), the cut pair,
    the full-minus-one and full rows, the restated rows and their track-less twins."""
    n = lay.n
    of = {c: np.flatnonzero(lay.cls == c) for c in range(4)}
    out = {"whole": np.arange(lay.m)}
    for c in range(4):
        if len(of[c]):
            out[CLASS_NAMES[c]] = of[c]
    if n in DS.SAMPLE_COUNTS:
        for c in (DS.SPARSE, DS.GAPS, DS.FULL):
            others = np.concatenate([of[o][:3] for o in range(4) if o != c])
            for count in LIST_COUNTS:
                alone = np.resize(of[c], count)
                out[f"{CLASS_NAMES[c]}x{count}"] = alone
                out[f"{CLASS_NAMES[c]}x{count}_among_others"] = np.concatenate([others[:4], alone, others[4:]])
        lo, hi = DS.cut_counts(n)
        out["cut_pair"] = np.array(lay.variants(f"E{lo}_tile0_ref") + lay.variants(f"E{hi}_tile0_ref"))
        out["full_minus_one_and_full"] = np.array(
            [v for name in (f"E{n - 1}_tile0_ref", f"E{n - 1}_last_ref", f"E{n}_tile0_ref") for v in lay.variants(name)])
    return {name: np.asarray(v, dtype=np.uint32) for name, v in out.items()}


def _score_mask(n):
    """A subset that removes some of every row's entries: every third sample and a block of two words."""
    s = np.arange(n)
    return (s % 3 != 1) & ~((s >= 64) & (s < 192))


def _score_inputs(name, count):
    rng = np.random.default_rng([count, len(name)])
    w = rng.standard_normal((count, 3))
    w[:, 2] = 1.0  # a unit column: it comes out as the dosage sum, bit for bit
    return w, (rng.random(count) < 0.3).astype(np.uint8)


def _check_score(got, want, w, ctx):
    """test_dosage_tracks.test_score_over_dosage_tracks' comparison."""
    from test_dosage_tracks import REL

    (s, d, ac), (es, ed, eac) = got, want
    assert s.shape == es.shape and _same_ints(ac, eac), ctx
    scale = np.abs(w).sum(axis=0) * 2.0
    bound = REL * np.maximum(np.abs(es), 1e-3 * scale)
    err = np.abs(s - es)
    if not np.all(err <= bound):
        k, c = np.unravel_index(np.argmax(err / bound), err.shape)
        raise AssertionError(f"{ctx}: score_sum off by {err[k, c]:.3g} at sample {k}, column {c} ({s[k, c]!r} for "
                             f"{es[k, c]!r}), {err[k, c] / bound[k, c]:.3g} times the bound {bound[k, c]:.3g}; "
                             f"{int((err > bound).any(axis=1).sum())} samples beyond it")
    assert np.allclose(d, ed, rtol=REL, atol=1e-9), ctx


def _run_plan_twice(ds, n, vidx, w, flip, code, ss):
    """pgh_score_plan_create and two pgh_score_run_dev: (score, dosage sum, allele count) per RAW sample of each run,
    from buffers that held 7s."""
    import torch

    plan = ds.score_plan(vidx, w, flip, code, ss)
    out = []
    for _ in range(2):
        d_score = torch.full((n, w.shape[1]), 7.0, dtype=torch.float64, device="cuda")
        d_dos = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
        d_ac = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        plan.run_dev(d_score.data_ptr(), d_dos.data_ptr(), d_ac.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out.append((d_score.cpu().numpy(), d_dos.cpu().numpy(), d_ac.cpu().numpy().astype(np.uint32)))
    plan.close()
    return out


# the lists of 1 .. 129 sparse rows are cases of their own: see test_score's docstring
SCORE_CASES = [(n, "rows") for n in ALL_COUNTS] + [(n, "sparse_counts") for n in DS.SAMPLE_COUNTS]


def _in_group(name, group):
    return name.startswith("sparsex") == (group == "sparse_counts")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,const", MODES)
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("n,group", SCORE_CASES)
def test_score(gpu_lib, files, oracle, n, group, route, mode, const, monkeypatch):
    """pgh_score and pgh_score_plan_create + pgh_score_run_dev over the lists of _score_lists, with 1 and 3 weight
    columns and flips, on the three routes, without a subset and under one that removes some of the entries' samples:
    ALLELE_CT exact, the sums within test_score_over_dosage_tracks' bounds of oracle.score on the written file, a column
    of unit weights the dosage sum bit for bit outside center mode.

    The sparse_counts lists are mostly rare tracks over an all-hom-ref row (E1_tile0_ref: sd = sqrt(2 f (1 - f)) =
    0.0127).  In center mode their 1 / sd would set the fixed-point scale of the whole weight column through table
    entries of codes that no sample carries; k_score_tables_dosage keeps those entries flat,
    and these cases are what holds it to that: with PGH_SCORE_DOSAGE_CODES=0 they miss the bound by up to 3.9 times.

    A kept plan is run on every list with three columns, and with one column on four of them."""
    L = gpu_lib
    if ROUTES[route]:
        monkeypatch.setenv(*ROUTES[route])
    f = files(n, True)
    lay, ds, pg = f.lay, f.ds(L), f.pg(oracle)
    code = getattr(L, const)
    masks = {"everyone": None}
    if n > 4:
        masks["thinned"] = _score_mask(n) if n > 256 else np.arange(n) % 3 != 1
    missed = []  # every list is checked: a list beyond the bound does not hide the lists after it
    for mask_name, mask in masks.items():
        ss = None if mask is None else ds.subset(mask)
        inc = None if mask is None else mask.astype(np.uint8)
        keep = slice(None) if mask is None else mask
        for name, vidx in _score_lists(lay).items():
            if not _in_group(name, group):
                continue
            w, flip = _score_inputs(name, len(vidx))
            want = f.once(("score", name, mode, mask_name),
                          lambda: oracle.score(pg, vidx, w, flip=flip, mode=mode, include=inc))
            ctx = (n, route, mode, mask_name, name)
            try:
                got = ds.score(vidx, w, flip=flip, mode=code, subset=ss)
                _check_score(got, want, w, ctx)
                if code != L.SCORE_CENTER:
                    assert got[0][:, 2].tobytes() == got[1].tobytes(), ctx
                one = ds.score(vidx, w[:, :1], flip=flip, mode=code, subset=ss)
                _check_score(one, (want[0][:, :1], want[1], want[2]), w[:, :1], ctx + ("one column",))
                for cols in (1, 3) if name in ("whole", "cut_pair", "sparse", "gaps") else (3,):
                    for raw in _run_plan_twice(ds, n, vidx, w[:, :cols], flip, code, ss):
                        _check_score(tuple(a[keep] for a in raw), (want[0][:, :cols], want[1], want[2]), w[:, :cols],
                                     ctx + ("plan", cols))
            except AssertionError as err:
                missed.append(str(err))
        if ss is not None:
            ss.close()
    print(f"n={n} {group} {route} {mode}: {len(missed)} lists beyond the bound")
    assert not missed, "\n".join(missed)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["records", "bitwalk"])
@pytest.mark.parametrize("n", DS.SAMPLE_COUNTS)
def test_center_mode_sums_are_the_same_values_with_and_without_the_row_codes(gpu_lib, files, oracle, n, route,
                                                                             monkeypatch):
    """PGH_SCORE_DOSAGE_CODES=0 keeps every table entry, which is also what a dataset without room for the codes
    gets: on the lists whose scale no rare track sets (the whole file, each class alone, the cut pair) both forms are
    within the bound of the oracle, so they are the same sums apart from rounding; ALLELE_CT is the same."""
    L = gpu_lib
    if ROUTES[route]:
        monkeypatch.setenv(*ROUTES[route])
    f = files(n, True)
    lay, ds, pg = f.lay, f.ds(L), f.pg(oracle)
    lists = _score_lists(lay)
    for name in ("whole", "hard", "sparse", "gaps", "full", "cut_pair"):
        vidx = lists[name]
        w, flip = _score_inputs(name, len(vidx))
        want = f.once(("score", name, "center", "everyone"), lambda: oracle.score(pg, vidx, w, flip=flip, mode="center"))
        flat = ds.score(vidx, w, flip=flip, mode=L.SCORE_CENTER)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PGH_SCORE_DOSAGE_CODES", "0")
            kept = ds.score(vidx, w, flip=flip, mode=L.SCORE_CENTER)
        _check_score(flat, want, w, (n, route, name, "codes"))
        _check_score(kept, want, w, (n, route, name, "no codes"))
        assert _same_ints(flat[2], kept[2]), (n, route, name)


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("n", DS.SAMPLE_COUNTS)
def test_a_row_that_restates_its_calls_scores_as_the_calls(gpu_lib, files, oracle, n, route, monkeypatch):
    """The restated rows (sparse, with gaps, full; every encoding) against their track-less twins, same weights and
    flips: ALLELE_CT equal, the sums within the same bounds of each other and of the oracle."""
    from test_dosage_tracks import REL

    L = gpu_lib
    if ROUTES[route]:
        monkeypatch.setenv(*ROUTES[route])
    f = files(n, True)
    lay, ds, pg = f.lay, f.ds(L), f.pg(oracle)
    names = ("restated_sparse", "restated_gaps", "restated_full")
    tracks = np.array([v for name in names for v in lay.variants(name) if lay.kinds[v]], dtype=np.uint32)
    twins = np.array([lay.variants(lay.names[v], 0)[0] for v in tracks], dtype=np.uint32)
    assert len(tracks) == 9 and not lay.kinds[twins].any() and np.array_equal(lay.hard[tracks], lay.hard[twins])
    w, flip = _score_inputs("restated", len(tracks))
    for mode, const in MODES:
        code = getattr(L, const)
        a = ds.score(tracks, w, flip=flip, mode=code)
        b = ds.score(twins, w, flip=flip, mode=code)
        want = oracle.score(pg, twins, w, flip=flip, mode=mode)
        ctx = (n, route, mode)
        _check_score(a, want, w, ctx + ("tracks",))
        _check_score(b, want, w, ctx + ("twins",))
        assert _same_ints(a[2], b[2]), ctx
        scale = np.abs(w).sum(axis=0) * 2.0
        assert np.all(np.abs(a[0] - b[0]) <= REL * np.maximum(np.abs(want[0]), 1e-3 * scale)), ctx
        assert np.allclose(a[1], b[1], rtol=REL, atol=1e-9), ctx


# ---- 5. the dense score test over dosage tracks -------------------------------------------------------------------

def _col(out, p):
    return {key: v[:, p] for key, v in out.items()}


def _check_by_distinct_row(lay, x, got, check, ctx):
    """check(variant, value row) once per distinct value row -- the oracle's rows are the expensive part -- and every
    other variant of the same values equal to that variant bit for bit.  Returns the rows fitted."""
    rows, of = _distinct_rows(lay, x)
    fitted = 0
    for v in rows:
        try:
            fitted += int(check(v))
        except AssertionError as err:
            raise AssertionError(f"designed row {lay.names[v]} ({hex(int(lay.kinds[v]))}) {ctx}: {err}") from err
    first = np.array(rows)[of]
    for key, col in got.items():
        a, b = np.asarray(col), np.asarray(col)[first]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.flatnonzero(np.array([p != q for p, q in zip(a.tolist(), b.tolist())]))
        assert bad.size == 0, (key, ctx, [(lay.names[v], hex(int(lay.kinds[v]))) for v in bad[:8]])
    return fitted


@pytest.mark.gpu
@pytest.mark.parametrize("k", GLM_KS)
@pytest.mark.parametrize("n", DS.SAMPLE_COUNTS)
def test_glm_score_multi_dosage(gpu_lib, files, n, k):
    """Every row of the five phenotypes against glm_score_oracle fed the catalogue's values, at
    test_glm_score_multi_dosage.REL; the three encodings of a row and its restatements bit for bit; a row that restates
    its calls and a row without a track equal pgh_glm_score_multi's row over a hardcall-only file of the same calls bit
    for bit."""
    import glm_score_oracle as O
    from test_glm_score_multi_dosage import REL, _same

    f = files(n)
    lay, ds = f.lay, f.ds(gpu_lib)
    Z, Y = _glm_inputs(n, k)
    zc = Z if k else None
    got = ds.glm_score_multi_dosage(Y, zc)
    assert got["beta"].shape == (lay.m, len(Y))
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        col = _col(got, p)
        worst = [0.0]

        def check(v):
            fitted, w = O.check_rows(col, f.x, nul, rel=REL, idx=[v])
            worst[0] = max(worst[0], w)
            exp = O.oracle_row(f.x[v], nul)  # the counts exactly: the dosages are multiples of 2^-14, their sum is exact
            assert col["obs_ct"][v] == exp["obs_ct"] and col["errcode"][v] == exp["errcode"]
            assert np.array_equal(col["a1_freq"][v], exp["a1_freq"], equal_nan=True), (col["a1_freq"][v], exp["a1_freq"])
            assert fitted or lay.names[v] in REFUSED or _may_be_refused(lay, v, nul.in_s)
            return fitted

        fitted = _check_by_distinct_row(lay, f.x, col, check, (n, k, p))
        print(f"n={n} k={k} phenotype {p}: {fitted} distinct rows fitted, worst {worst[0]:.3g}")
    # the hardcall route over the same calls
    hard_path = f.path[:-5] + "_hard.pgen"
    W.write_pgen(hard_path, lay.hard, W.choose_kinds(lay.hard, np.random.default_rng(n)))
    hard = gpu_lib.Dataset.open(hard_path)
    want = hard.glm_score_multi(Y, zc)
    hard.close()
    calls = np.array([not lay.kinds[v] or lay.names[v].startswith("restated_") for v in range(lay.m)])
    assert calls.sum() == ROW_COUNTS[n] + 9
    _same({key: v[calls] for key, v in got.items()}, {key: v[calls] for key, v in want.items()}, ctx=(n, k))


# ---- 6. pgh_glm and pgh_glm_multi: the dense-dosage-row route -----------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("model", ["linear", "logistic"])
@pytest.mark.parametrize("n", DS.SAMPLE_COUNTS)
def test_glm(gpu_lib, files, n, model):
    """pgh_glm and every column of pgh_glm_multi, linear and logistic without Firth, against glm_oracle at
    test_glm_widths_chunks' 1e-9 and 1e-6."""
    import glm_oracle as G
    from glm_oracle import _same_rows

    f = files(n)
    lay, ds = f.lay, f.ds(gpu_lib)
    Z, Y = _glm_test_inputs(n, model)
    rel = 1e-9 if model == "linear" else 1e-6
    multi = ds.glm_multi(Y, Z, model=model, firth=False)
    single = ds.glm(Y[0], Z, model=model, firth=False)
    for what, p, col in [("glm", 0, single)] + [("glm_multi", p, _col(multi, p)) for p in range(len(Y))]:
        y = Y[p]
        in_s = ~np.isnan(y)

        def check(v):
            seen = {}
            fitted = G.check_rows(col, f.x, y, Z, model, False, rel=rel, idx=[v], seen=seen)
            code = seen[v]["errcode"]
            assert fitted or lay.names[v] in REFUSED or _may_be_refused(lay, v, in_s) or \
                (model == "logistic" and LOGISTIC_UNFIT.get(lay.names[v]) == code and lay.kinds[v]), code
            return fitted

        fitted = _check_by_distinct_row(lay, f.x, col, check, (n, model, what, p))
        print(f"n={n} {model} {what} phenotype {p}: {fitted} distinct rows fitted")
        assert fitted > len(_distinct_rows(lay, f.x)[0]) // 2
    if model == "logistic":  # include/pgenhip.h: pgh_glm_multi's logistic rows are pgh_glm's bit for bit
        _same_rows(single, _col(multi, 0))


# ---- 7. small lists and empty forms ------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", DS.SAMPLE_COUNTS)
def test_small_lists_and_empty_forms(gpu_lib, files, oracle, n):
    """A list that names a track twice, a list in descending order, and no variants at all, through every entry point
    that takes a list (the _dev forms of the moments and the values, pgh_glm, pgh_glm_multi and
    pgh_glm_score_multi_dosage take ranges only: for them the empty range).  The two lists against the references; no
    variants: PGH_OK with nothing written, which the guarded buffers of the _dev forms show; of the score the header
    promises zeros in every sum and allele count, which buffers that held 7s show."""
    import torch

    from test_device_entry_points import Guarded

    L = gpu_lib
    f = files(n, True)
    lay, ds, pg = f.lay, f.ds(L), f.pg(oracle)
    mask = _score_mask(n)
    st = torch.cuda.current_stream().cuda_stream
    by_class = {c: np.flatnonzero(lay.cls == c) for c in range(4)}
    twice = np.array([v for c in (DS.SPARSE, DS.GAPS, DS.FULL) for v in (by_class[c][1], by_class[c][1])], dtype=np.uint32)
    descending = np.arange(lay.m - 1, -1, -3, dtype=np.uint32)
    for subset_name, m in (("everyone", None), ("thinned", mask)):
        ss = None if m is None else ds.subset(m)
        keep = slice(None) if m is None else m
        inc = None if m is None else m.astype(np.uint8)
        x = f.x[:, keep]
        for what, vidx in (("twice", twice), ("descending", descending)):
            ctx = (n, subset_name, what)
            assert _same_ints(ds.dosage_sums(vidx=vidx, subset=ss), DS.moments(x[vidx])), ctx
            assert np.array_equal(ds.dosage_unpack(vidx=vidx, subset=ss), x[vidx]), ctx
            assert np.array_equal(ds.dosage_unpack_samples(vidx, subset=ss), x[vidx].T), ctx
            rd = ds.reader(ss)
            for v in vidx:  # the reader takes one variant a call: the same calls in the list's order
                assert np.array_equal(rd.get_dosage_f64(int(v)), x[v]), ctx + (int(v),)
            rd.close()
            w, flip = _score_inputs(what, len(vidx))
            for route, env in ROUTES.items():
                with pytest.MonkeyPatch.context() as mp:
                    if env:
                        mp.setenv(*env)
                    for mode, const in MODES:
                        want = f.once(("small", what, mode, subset_name),
                                      lambda: oracle.score(pg, vidx, w, flip=flip, mode=mode, include=inc))
                        _check_score(ds.score(vidx, w, flip=flip, mode=getattr(L, const), subset=ss), want, w,
                                     ctx + (route, mode))
                        for raw in _run_plan_twice(ds, n, vidx, w, flip, getattr(L, const), ss):
                            _check_score(tuple(a[keep] for a in raw), want, w, ctx + (route, mode, "plan"))
        # no variants: PGH_OK, nothing written
        none = np.zeros(0, dtype=np.uint32)
        assert ds.dosage_sums(7, 7, subset=ss).shape == (0, 3) and ds.dosage_sums(vidx=none, subset=ss).shape == (0, 3)
        assert ds.dosage_unpack(7, 7, subset=ss).shape[0] == 0 and ds.dosage_unpack(vidx=none, subset=ss).shape[0] == 0
        g, h = Guarded(240), Guarded(8 * n)
        ds.dosage_sums_dev(7, 7, g.ptr, st, subset=ss)
        ds.dosage_unpack_dev(7, 7, h.ptr, n, st, subset=ss)
        torch.cuda.synchronize()
        g.check(g.image())
        h.check(h.image())
        assert ds.dosage_unpack_samples(none, subset=ss).shape == (x.shape[1], 0)
        for mode, const in MODES:
            s, d, ac = ds.score(none, np.zeros((0, 2)), mode=getattr(L, const), subset=ss)
            assert s.shape == (x.shape[1], 2) and not s.any() and not d.any() and not ac.any(), mode
            for raw in _run_plan_twice(ds, n, none, np.zeros((0, 2)), None, getattr(L, const), ss):
                assert all(not a[keep].any() for a in raw), (n, subset_name, mode)  # zeros over the 7s
        if ss is not None:
            ss.close()
    for k in GLM_KS:
        Z, Y = _glm_inputs(n, k)
        zc = Z if k else None
        assert ds.glm_score_multi_dosage(Y, zc, v_begin=7, v_end=7)["beta"].shape == (0, len(Y))
        for model in ("linear", "logistic"):
            assert ds.glm_multi(Y, zc, model=model, firth=False, v_begin=7, v_end=7)["beta"].shape == (0, len(Y))
            assert ds.glm(Y[0], zc, model=model, firth=False, v_begin=7, v_end=7)["beta"].shape == (0,)
