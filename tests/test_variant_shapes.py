"""Every entry point that takes a variant list or range, under the structured lists and placements of
tests/variant_shapes.py.

One test function per family, parametrised over (placement, list).  The reference of every output is the operation in
NumPy on codes[list] (variant_shapes.py and the yardsticks it borrows from the family's own test file), the same for
every placement, so that `window` and `group` are held to what `whole` is held to; integer outputs are compared with
np.array_equal, floating outputs with the tolerance the family's own test uses against the same reference (each is
named where it is used).  Under `window` and `group` the integer outputs must also equal the `whole` dataset's for the
same global variants bit for bit, and so must the floating rows that include/pgenhip.h calls a function of the variant
alone (the GLM rows, burden, SKAT).  A list that an entry point refuses is pinned to PGH_ERR_ARG, the header's message
and untouched outputs.

plan() is the grid: what every (entry point, placement, list) cell is meant to do.  The tests record what they did
through _Grid, and test_the_grid_is_counted asserts that the only cells neither run nor pinned to a refusal are those
of EXCLUDED.  Run the whole file: the count needs every case of a family that ran at all."""

import contextlib

import numpy as np
import pytest

import subset_shapes as SS
import variant_shapes as VS

DENSE, SPARSE = VS.DENSE_PLACEMENTS, VS.SPARSE_PLACEMENTS
DENSE_CASES, SPARSE_CASES = VS.cases(DENSE), VS.cases(SPARSE)
ALL_CASES = DENSE_CASES + SPARSE_CASES
PCA_MIN = 63                   # plink_pca: lists of at least this many variants (12 Krylov columns need rank to spare)
MAX_MINORS = (0, VS.N)         # the sparse forms: the default rule, and every row held sparse
ONE_DEVICE = "takes one device's dataset"
RESIDENT = "resident range"
INCREASING = "the variant list must be strictly increasing"
N_VAR_ZERO = "n_var must be at least 1"


def _ids(cases):
    return [f"{p}-{name}" for p, name in cases]


# ---- the grid ----------------------------------------------------------------------------------------------------

# entry point -> where it runs, the form its variants take (range: v_begin / v_end; list: vidx; both), and its rules:
# one_device (a shard group is refused), increasing (reversed, shuffled and repeated are refused), empty (None: the
# empty list is answered; else the message of its refusal), outside (the message that names the resident range)
ENTRIES = {
    "counts_range": dict(where=DENSE + SPARSE, form="range"),
    "missing_per_sample": dict(where=DENSE, form="range"),
    "unpack_range": dict(where=DENSE, form="range"),
    "unpack_samples": dict(where=DENSE, form="list"),
    "sample_counts": dict(where=DENSE + SPARSE, form="both"),
    "reader": dict(where=DENSE, form="list"),
    "dosage_sums": dict(where=DENSE, form="both"),
    "dosage_unpack": dict(where=DENSE, form="both"),
    "dosage_unpack_samples": dict(where=DENSE, form="list"),
    "reader_dosage": dict(where=DENSE, form="list"),
    "score_dosage": dict(where=DENSE, form="list"),
    "score": dict(where=DENSE, form="list"),
    "score_counts": dict(where=DENSE, form="list"),
    "score_plan": dict(where=DENSE, form="list", one_device=True),
    "score_sparse": dict(where=SPARSE, form="list"),
    "ld_pairs": dict(where=DENSE, form="list"),
    "ld_window_sums": dict(where=DENSE, form="both", one_device=True, empty="variant rectangle"),
    "ld_prune": dict(where=DENSE, form="both", one_device=True, increasing=True, empty=N_VAR_ZERO),
    "ld_scores": dict(where=DENSE, form="both", one_device=True, increasing=True, empty=N_VAR_ZERO),
    "king_counts": dict(where=DENSE, form="both", one_device=True, empty=N_VAR_ZERO),
    "king_table": dict(where=DENSE, form="both", one_device=True, empty=N_VAR_ZERO),
    "grm": dict(where=DENSE, form="both", one_device=True, empty=N_VAR_ZERO),
    "pca": dict(where=DENSE, form="list", empty="too few variants"),
    "glm": dict(where=DENSE, form="range"),
    "glm_multi": dict(where=DENSE, form="range"),
    "glm_sparse": dict(where=SPARSE, form="range"),
    "glm_score_sparse": dict(where=SPARSE, form="range"),
    "glm_score_sparse_spa": dict(where=SPARSE, form="range"),
    "burden_sparse": dict(where=SPARSE, form="list", outside="is not below the dataset's variant count"),
    "skat_sparse": dict(where=SPARSE, form="list", outside="is not below the dataset's variant count"),
}
SKAT_TOO_LARGE = "set larger than PGH_SKAT_MAX_SET"

# The cells that are neither run nor pinned to a refusal, and why.  Nothing else is left out.
EXCLUDED = {
    "range": "the entry point takes v_begin / v_end only, and the list is not a run of consecutive variants",
    "list": "the entry point takes a list only: it has no variant_begin / n_var form (all_listed is the same variants)",
    "pca": "plink_pca needs more variants than its (n_pcs + 1) 2 n_pcs = 12 Krylov columns, with rank to spare: "
           f"lists of fewer than {PCA_MIN} variants that it would accept are left out",
}


def _length(placement, name):
    b, e = VS.resident(placement)
    lst = VS.shapes(b, e)[name]
    return e - b if lst is None else len(lst)


def plan(entry, placement, name):
    """("run", None), ("refused", message) or ("excluded", key of EXCLUDED) for a cell of the grid."""
    rule = ENTRIES[entry]
    b, e = VS.resident(placement)
    assert placement in rule["where"] and name in VS.shapes(b, e)
    if rule["form"] == "range" and VS.as_range(name, b, e) is None:
        return "excluded", "range"
    if rule["form"] == "list" and name == "range_all":
        return "excluded", "list"
    if placement == "group" and rule.get("one_device"):
        return "refused", ONE_DEVICE
    if name in VS.OUTSIDE:
        return "refused", rule.get("outside", RESIDENT)
    if name == "empty":
        return ("refused", rule["empty"]) if rule.get("empty") else ("run", None)
    if rule.get("increasing") and name in VS.UNORDERED:
        return "refused", INCREASING
    if entry == "pca" and _length(placement, name) < PCA_MIN:
        return "excluded", "pca"
    if entry == "skat_sparse" and _length(placement, name) > 256:
        return "refused", SKAT_TOO_LARGE
    return "run", None


def grid():
    """Every cell: (entry, placement, list) -> plan."""
    return {(entry, p, name): plan(entry, p, name) for entry, rule in ENTRIES.items() for p in rule["where"]
            for name in VS.shapes(*VS.resident(p))}


class _Grid:
    """What the tests did, cell by cell."""

    done = {}

    @classmethod
    def record(cls, entry, placement, name, outcome):
        assert plan(entry, placement, name)[0] == outcome, (entry, placement, name, outcome)
        cls.done[(entry, placement, name)] = outcome


# ---- the catalogue itself (no GPU) -------------------------------------------------------------------------------

def _catalogue(b, e):
    """name -> (length, first local, last local), written out independently of shapes()."""
    n = e - b
    out = {
        "all_listed": (n, 0, n - 1), "first": (1, 0, 0), "last": (1, n - 1, n - 1), "ends": (2, 0, n - 1),
        "tile64": (64, 64, 127), "tile64_plus": (65, 61, 125), "tile64_minus": (63, 3, 65),
        "tile96_plus": (97, 2, 98), "tile128_plus": (129, 5, 133), "stride3": ((n + 2) // 3, 0, 3 * ((n - 1) // 3)),
        "all_but_one": (n - 1, 0, n - 1), "reversed": (n, n - 1, 0), "repeated": (65, 61, 125),
        "outside_high": (1, n, n), "empty": (0, None, None),
    }
    if b:
        out["outside_low"] = (1, -1, -1)
    return out


def test_the_catalogue_is_what_the_kernels_are_meant_to_see():
    """The length, the first and the last local index and the tile residues of every list at every placement, so
    that a later edit cannot quietly move a list off its edge."""
    assert (VS.N, VS.M_V, VS.WINDOW, VS.CUT) == (1003, 323, (37, 318), 150)
    assert VS.M_V == 5 * 64 + 3 == 2 * 128 + 67 == 3 * 96 + 35
    assert VS.WINDOW[0] % 2 == 1 and VS.WINDOW[0] % 4 and VS.WINDOW[0] % 64 and VS.WINDOW[1] - VS.WINDOW[0] == 281
    assert VS.CUT % 64 and VS.CUT % 96 and VS.CUT % 128
    assert all(VS.WINDOW[0] <= r < VS.WINDOW[1] for r in VS.MADE_ROWS + VS.HET_ROWS)
    assert [k * VS.SPARSE_WINDOW_ROWS for k in (1, 2, 3)] == [97, 194, 291]
    for placement in DENSE + SPARSE:
        b, e = VS.resident(placement)
        assert (b, e) == (VS.WINDOW if "window" in placement else (0, VS.M_V))
        lists = VS.shapes(b, e)
        want = _catalogue(b, e)
        assert list(lists) == [name for name in VS.LIST_NAMES if name == "outside_low" and b or name != "outside_low"]
        assert lists["range_all"] is None and ("outside_low" in lists) == (b > 0)
        for name, lst in lists.items():
            if name in want:
                length, first, last = want[name]
                assert lst.dtype == np.int64 and len(lst) == length, (placement, name)
                if length:
                    assert (int(lst[0]) - b, int(lst[-1]) - b) == (first, last), (placement, name)
            if lst is not None and name not in VS.OUTSIDE:
                assert ((lst >= b) & (lst < e)).all(), (placement, name)
        local = {name: lst - b for name, lst in lists.items() if lst is not None}
        # at a 64-variant tile and next to it, one past a 96- and a 128-variant tile, none starting on a tile
        assert {len(local[k]) - 64 for k in ("tile64", "tile64_plus", "tile64_minus")} == {0, 1, -1}
        assert local["tile64"][0] % 64 == 0 and local["tile64_plus"][0] % 4 == 1 and local["tile64_minus"][0] == 3
        assert len(local["tile96_plus"]) == 96 + 1 and len(local["tile128_plus"]) == 128 + 1
        for name in VS.CONTIGUOUS:
            assert (np.diff(lists[name]) == 1).all() and VS.as_range(name, b, e) == (lists[name][0], lists[name][-1] + 1)
        assert (np.diff(local["stride3"]) == 3).all() and (local["stride3"] % 3 == 0).all()
        assert sorted(set(range(e - b)) - set(local["all_but_one"].tolist())) == [VS.DROPPED_LOCAL]
        assert lists["made_only"].tolist() == list(VS.MADE_ROWS)
        assert (np.diff(local["reversed"]) == -1).all()
        assert sorted(local["shuffled"].tolist()) == local["stride3"].tolist() and (np.diff(local["shuffled"]) < 0).any()
        # repeated: tile64_plus with [a, a, c, a, d, c] at positions 10..15 -- a three times, c twice, three left out
        rep, plus = local["repeated"], local["tile64_plus"]
        at = VS.REPEAT_AT
        a, c, d = plus[at], plus[at + 2], plus[at + 4]
        assert rep[at:at + 6].tolist() == [a, a, c, a, d, c] and np.array_equal(np.delete(rep, np.s_[at:at + 6]),
                                                                                 np.delete(plus, np.s_[at:at + 6]))
        assert len(set(rep.tolist())) == 65 - 3 and (np.diff(rep) <= 0).sum() == 3
        for name in ("stride3", "all_but_one", "made_only", "reversed", "shuffled", "repeated", "ends"):
            assert VS.as_range(name, b, e) is None
        assert VS.as_range("range_all", b, e) == (b, e) and VS.as_range("empty", b, e) == (b + 5, b + 5)
        assert VS.as_range("outside_high", b, e) == (e, e + 1)
        if b:
            assert VS.as_range("outside_low", b, e) == (b - 1, b)
    # the group's cut and the sparse windows fall inside the lists that are meant to straddle them
    whole = VS.shapes(0, VS.M_V)
    for name in ("stride3", "shuffled", "all_but_one"):  # both sides of the cut, in a list that is not a range
        assert whole[name].min() < VS.CUT <= whole[name].max() and VS.CUT in whole[name] and VS.CUT - 1 not in whole["stride3"]
    assert whole["tile96_plus"][0] < VS.SPARSE_WINDOW_ROWS <= whole["tile96_plus"][-1]
    window = VS.shapes(*VS.WINDOW)  # and the window's tile lists lie across global variant 150 and sparse row 97
    assert window["tile64"][0] < VS.CUT <= window["tile64"][-1]
    assert window["tile96_plus"][0] - VS.WINDOW[0] < VS.SPARSE_WINDOW_ROWS <= window["tile96_plus"][-1] - VS.WINDOW[0]


def test_the_matrices_hold_the_made_rows():
    """The made rows, and every NumPy reference of this file against the brute force the suite already has."""
    from test_king import brute_counts, brute_table
    from test_ld_prune import brute_prune, brute_sums, windows
    from test_ld_scores import brute_scores

    codes = VS.hard_codes()
    assert codes.shape == (VS.M_V, VS.N) and codes.max() == 3
    assert sorted(VS._interleave()) == list(range(VS.M_V))  # a permutation of subset_shapes.hard_codes' rows
    plain = SS.hard_codes(VS.N, m=VS.M_V)
    untouched = [k for k in range(VS.M_V) if k not in VS.MADE_ROWS]
    assert np.array_equal(codes[untouched], plain[VS._interleave()][untouched])
    assert (codes[list(VS.ROWS_ALL_MISSING)] == 3).all() and (codes[list(VS.ROWS_MONO)] == 0).all()
    rest = np.delete(codes, list(VS.MADE_ROWS) + [2 * SS.ROW_ALL_MISSING, 2 * SS.ROW_MONO, 2 * SS.ROW_BLOCK], axis=0)
    assert 0.07 < (rest == 3).mean() < 0.09
    rare, y = VS.rare_codes()
    assert rare.shape == (VS.M_V, VS.N) and set(np.unique(y)) == {0.0, 1.0}
    assert (rare[list(VS.ROWS_ALL_MISSING)] == 3).all() and (rare[list(VS.ROWS_MONO)] == 0).all()
    for placement in ("whole", "window"):
        b, e = VS.resident(placement)
        assert {int(np.bincount(r, minlength=4).argmax()) for r in rare[b:e]} == {0, 1, 2, 3}
    assert [int(np.bincount(rare[r], minlength=4).argmax()) for r in VS.HET_ROWS] == [1, 1]
    # the pair sums, the planes, the pruning and the scores of a reordered list with repeats and of a plain one
    lists = VS.shapes(*VS.WINDOW)
    for name in ("repeated", "tile64_minus"):
        lst = lists[name]
        sub = codes[lst]
        planes = SS.ld_planes(sub)
        assert np.array_equal(planes, brute_sums(sub))
        a, b = VS.ld_pair_lists(lst)
        assert len(a) == len(lst) + 2 and a[-1] == b[-1] and (a[-2], b[-2]) == (lst[-1], lst[0])
        pos = {int(v): k for k, v in enumerate(lst)}  # (for a repeated variant: its last place, the same row)
        ia, ib = [pos[int(v)] for v in a], [pos[int(v)] for v in b]
        assert np.array_equal(VS.ld_pairs_ref(codes, a, b), np.stack([planes[p][ia, ib] for p in range(6)], axis=1))
        if name == "tile64_minus":
            win_end = windows(len(lst), 50)
            assert np.array_equal(SS.ld_prune_ref(planes, sub, win_end, LD_R2, 1e-12), brute_prune(sub, win_end, LD_R2))
            for x, y2 in zip(SS.ld_scores_ref(planes, sub, win_end, True), brute_scores(sub, win_end, True)):
                assert np.array_equal(x, y2)
    assert VS.ld_pairs_ref(codes, [], []).shape == (0, 6)
    # the king table: the vectorised reference against test_king's loop in Python integers, on a corner of the square
    few = codes[lists["repeated"]][:, :40]
    i, j, nsnp, hethet, ibs0, h1, h2, kin = VS.king_table_ref(brute_counts(few))
    loop = brute_table(few, -np.inf)
    assert [tuple(r[:7]) for r in loop] == list(zip(i, j, nsnp, hethet, ibs0, h1, h2))
    assert np.array([r[7] for r in loop]).tobytes() == kin.tobytes()
    # the score reference on a list with repeats is the sum of the single-variant scores
    orc_score = _oracle_module().score
    pg = SS.MatrixPgen(SS.values(codes))
    lst = lists["repeated"][8:18]
    w, flip = VS.score_inputs(len(lst), 2)
    whole_sum = orc_score(pg, lst, w, flip=flip, mode="no_mean_imputation")
    parts = [orc_score(pg, lst[k:k + 1], w[k:k + 1], flip=flip[k:k + 1], mode="no_mean_imputation") for k in range(len(lst))]
    assert np.allclose(whole_sum[0], sum(p[0] for p in parts), rtol=0, atol=1e-12)
    assert np.array_equal(whole_sum[2], sum(p[2] for p in parts))
    f = VS.supplied_freq(65)
    assert (f[1], f[5]) == (0.0, 1.0) and np.isnan(f[9]) and ((f > 0) & (f < 1)).sum() == 62


def _oracle_module():
    from oracle import oracle as orc
    return orc


def test_the_plan_covers_every_cell():
    """The grid without a device: every cell is run, refused or in EXCLUDED, and the counts are what they are."""
    cells = grid()
    kinds = {}
    for (entry, placement, name), (outcome, why) in cells.items():
        kinds[outcome] = kinds.get(outcome, 0) + 1
        if outcome == "excluded":
            assert why in EXCLUDED, (entry, placement, name)
            if why == "pca":
                assert entry == "pca" and _length(placement, name) < PCA_MIN
            elif why == "range":
                assert ENTRIES[entry]["form"] == "range" and name not in VS.CONTIGUOUS
            else:
                assert ENTRIES[entry]["form"] == "list" and name == "range_all"
        elif outcome == "refused":
            assert why
    assert set(kinds) == {"run", "refused", "excluded"}
    assert sum(kinds.values()) == len(cells) == sum(len(VS.shapes(*VS.resident(p))) for rule in ENTRIES.values()
                                                     for p in rule["where"])
    # every list-taking entry point meets every unordered list and both outside lists somewhere
    for entry, rule in ENTRIES.items():
        names = {name for (en, _, name), (outcome, _) in cells.items() if en == entry and outcome != "excluded"}
        assert {"outside_low", "outside_high", "empty"} <= names, entry
        if rule["form"] != "range":
            assert set(VS.UNORDERED) <= names or entry == "pca", entry


# ---- datasets and references, built once per module ---------------------------------------------------------------

def _key(lst):
    return np.asarray(lst, dtype=np.int64).tobytes()


class _World:
    def __init__(self, L, orc, tmp):
        from test_dosage_tracks import make_dosage_file

        self.L, self.orc = L, orc
        self._cache = {}
        # the hardcall matrix, of every record type
        self.codes = VS.hard_codes()
        self.hard_path = str(tmp / "hard.pgen")
        SS.W.write_pgen(self.hard_path, self.codes, SS.W.choose_kinds(self.codes, np.random.default_rng(VS.M_V)))
        self.hard = self._placements(self.hard_path)
        self.pg = SS.MatrixPgen(SS.values(self.codes))
        self.z, self.y_lin, self.y_bin = VS.phenotypes()
        # a dosage- and phase-bearing file from the writer
        self.dose_path = str(tmp / "dose.pgen")
        self.dcodes, self.dos, self.dkinds, self.want = make_dosage_file(self.dose_path, VS.M_V, VS.N, 300 + VS.N, True)
        self.dose = self._placements(self.dose_path)
        self.dpg = orc.Pgen(self.dose_path)  # the phase tracks are random bits of the writer's: the oracle reads them
        assert self.dpg.has_dosage and self.dpg.has_phase
        for b, e in ((0, VS.M_V), VS.WINDOW):
            assert {0, 0x20, 0x40, 0x60} == set(self.dkinds[b:e])
        self.dose_pg = SS.MatrixPgen(self.want)
        # the rare matrix, sparse-resident under several windows per open
        self.rare, y = VS.rare_codes()
        self.rare_path = str(tmp / "rare.pgen")
        SS.W.write_pgen(self.rare_path, self.rare, SS.W.choose_kinds(self.rare, np.random.default_rng(7 * VS.M_V)))
        dense = L.Dataset.open(self.rare_path)
        self.pitch = dense.info.pitch_bytes
        dense.close()
        self.sparse = {}
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(VS.SPARSE_WINDOW_ROWS * self.pitch))
            for placement in SPARSE:
                b, e = VS.resident(placement)
                for mm in MAX_MINORS:
                    self.sparse[(placement, mm)] = L.Dataset.open(self.rare_path, variant_begin=b, variant_end=e,
                                                                  sparse=True, max_minor=mm)
        for (placement, mm), sp in self.sparse.items():
            info = sp.sparse_info()
            assert (sp.v_begin, sp.v_end) == VS.resident(placement)
            assert (info.dense_variant_ct == 0) == (mm == VS.N) and info.sparse_variant_ct > 0
        self.rz = SS.covariates(VS.N, seed=9)
        self.ry_lin = SS.linear_phenotypes(VS.N, self.rz)[0]
        self.ry_bin = np.where(SS.nan_samples(VS.N), np.nan, y)
        self.rx = SS.values(self.rare)

    def _placements(self, path):
        L = self.L
        out = {"whole": L.Dataset.open(path),
               "window": L.Dataset.open(path, variant_begin=VS.WINDOW[0], variant_end=VS.WINDOW[1]),
               "group": L.Dataset.group([L.Dataset.open(path, variant_begin=0, variant_end=VS.CUT),
                                         L.Dataset.open(path, variant_begin=VS.CUT, variant_end=VS.M_V)])}
        assert out["group"].shard_count == 2 and (out["window"].v_begin, out["window"].v_end) == VS.WINDOW
        assert (out["group"].v_begin, out["group"].v_end) == (0, VS.M_V)
        return out

    def ref(self, kind, lst, make):
        """A reference of codes[list], computed once and shared by the placements."""
        key = (kind, _key(lst))
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]


@pytest.fixture(scope="module")
def world(gpu_lib, oracle, tmp_path_factory):
    return _World(gpu_lib, oracle, tmp_path_factory.mktemp("variant_shapes"))


class _Untouched:
    """Stands in for numpy inside plinking_duck_amd.lib while a refused call runs: the output arrays the wrapper
    makes (np.zeros, its only source of them) are filled with 0xA5 bytes and kept, so that the test can see whether
    the library wrote to them."""

    def __init__(self):
        self.made = []

    def zeros(self, shape, dtype=float):
        a = np.zeros(shape, dtype=dtype)
        a.view(np.uint8)[...] = 0xA5
        self.made.append(a)
        return a

    def __getattr__(self, name):
        return getattr(np, name)


def _refused(L, call, match, outputs=True):
    """PGH_ERR_ARG, the message, and outputs untouched (outputs=False: the wrapper has no output array)."""
    proxy = _Untouched()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(L, "np", proxy)
        with pytest.raises(L.PghArgError, match=match) as info:
            call()
    assert info.value.code == L.PGH_ERR_ARG
    assert bool(proxy.made) == outputs, "the wrapper's output arrays are not where this helper looks for them"
    for a in proxy.made:
        assert (a.view(np.uint8) == 0xA5).all(), "a refused call wrote to an output"


@contextlib.contextmanager
def _written(L, name):
    """Under the empty list, the wrappers' output arrays start as 0xA5 bytes, not as zeros: what comes back is then what
    the library wrote, so "PGH_OK, every count 0" is told from "PGH_OK, nothing written"."""
    with pytest.MonkeyPatch.context() as mp:
        if name == "empty":
            mp.setattr(L, "np", _Untouched())
        yield


def _same_ints(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def _u32(lst):
    return np.asarray(lst, dtype=np.uint32)


def _cell(entry, placement, name, L, run, refuse=None, outputs=True):
    """Do what plan() says of a cell: run it (run() asserts), or pin its refusal (refuse: the call, or the calls, that
    must each be refused; default: run), or nothing for an excluded one.  Returns whether it ran."""
    outcome, why = plan(entry, placement, name)
    if outcome == "run":
        run()
    elif outcome == "refused":
        for call in (refuse if isinstance(refuse, list) else [refuse or run]):
            _refused(L, call, why, outputs)
    else:
        return False
    _Grid.record(entry, placement, name, outcome)
    return outcome == "run"


def _forms_of(placement, name):
    """The ways a cell names its variants: ("list", vidx), ("range", (v0, v1)) or both."""
    b, e = VS.resident(placement)
    lst = VS.shapes(b, e)[name]
    out = []
    if lst is not None:
        out.append(("list", lst))
    if VS.as_range(name, b, e) is not None:
        out.append(("range", VS.as_range(name, b, e)))
    return out


def _variants(placement, name):
    """The global variants of a cell, in call order (range_all: the resident range)."""
    b, e = VS.resident(placement)
    lst = VS.shapes(b, e)[name]
    return np.arange(b, e, dtype=np.int64) if lst is None else lst


def _args(form, how):
    """Keyword arguments of a wrapper that takes v_begin / v_end / vidx."""
    if form == "list":
        return dict(vidx=_u32(how))
    return dict(v_begin=int(how[0]), v_end=int(how[1]))


# ---- calls and tallies -------------------------------------------------------------------------------------------

def _range_entries(codes):
    """entry -> (call(ds, v0, v1) -> tuple of arrays, ref(v0, v1) -> tuple of arrays) of the range-taking calls."""
    return {
        "counts_range": (lambda d, v0, v1: (d.counts_range(v0, v1),), lambda v0, v1: (SS.counts_ref(codes[v0:v1]),)),
        "missing_per_sample": (lambda d, v0, v1: (d.missing_per_sample(v0, v1),),
                               lambda v0, v1: (SS.sample_counts_ref(codes[v0:v1])[:, 3].copy(),)),
        "unpack_range": (lambda d, v0, v1: d.unpack_range(v0, v1),
                         lambda v0, v1: (SS.calls(codes[v0:v1]), SS.validity_ref(codes[v0:v1]))),
    }


def _check_range_entries(L, ds, whole, codes, placement, name, entries):
    b, e = VS.resident(placement)
    span = VS.as_range(name, b, e)
    for entry in entries:
        call, ref = _range_entries(codes)[entry]

        def run():
            with _written(L, name):
                got = call(ds, *((None, None) if name == "range_all" else span))  # range_all: the wrapper's defaults
            for g, want in zip(got, ref(*span)):
                assert _same_ints(g, want), (entry, placement, name)
            for g, w in zip(got, call(whole, *span)):
                assert _same_ints(g, w), (entry, placement, name)

        _cell(entry, placement, name, L, run, lambda: call(ds, *span))


@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", ALL_CASES, ids=_ids(ALL_CASES))
def test_calls_and_tallies(gpu_lib, world, placement, name):
    L = gpu_lib
    if placement in SPARSE:
        codes = world.rare
        for mm in MAX_MINORS:
            ds, whole = world.sparse[(placement, mm)], world.sparse[("sparse_whole", mm)]
            _check_range_entries(L, ds, whole, codes, placement, name, ["counts_range"])
            _check_sample_counts(L, ds, whole, codes, placement, name)
        return
    codes, ds, whole = world.codes, world.hard[placement], world.hard["whole"]
    _check_range_entries(L, ds, whole, codes, placement, name, ["counts_range", "missing_per_sample", "unpack_range"])
    _check_sample_counts(L, ds, whole, codes, placement, name)
    lst = _variants(placement, name)

    def unpack_samples():
        got = ds.unpack_samples(_u32(lst))
        assert _same_ints(got, np.ascontiguousarray(SS.calls(codes[lst]).T))
        assert _same_ints(got, whole.unpack_samples(_u32(lst)))

    _cell("unpack_samples", placement, name, L, unpack_samples)
    _check_reader(L, world, placement, name)


def _check_sample_counts(L, ds, whole, codes, placement, name):
    def run():
        with _written(L, name):
            got = [ds.sample_counts(**_args(form, how)) for form, how in _forms_of(placement, name)]
        want = SS.sample_counts_ref(codes[_variants(placement, name)])
        for g in got:  # all_listed and range_all, the two forms of a contiguous list: the same integers
            assert _same_ints(g, want), (placement, name)
        if name == "range_all":
            assert _same_ints(ds.sample_counts(), want)
        assert _same_ints(whole.sample_counts(**_args(*_forms_of(placement, name)[0])), want)

    _cell("sample_counts", placement, name, L, run,
          [lambda kw=_args(form, how): ds.sample_counts(**kw) for form, how in _forms_of(placement, name)])


def _check_reader(L, world, placement, name):
    """The per-variant calls at every variant of the list: the calls over the hardcall file (it has the made rows),
    the phase and dosage tracks over the writer's file."""
    lst = _variants(placement, name)
    codes, dcodes = world.codes, world.dcodes
    every = np.ones(VS.N, dtype=np.uint8)

    def calls(rd, v):
        assert _same_ints(rd.get_counts(v), SS.counts_ref(codes[v:v + 1])[0])
        assert _same_ints(rd.get_2bit(v), SS.packed_2bit_ref(codes[v]))
        assert _same_ints(rd.get_int8(v), SS.calls(codes[v]))
        assert _same_ints(rd.get_missingness(v), SS.bits_ref(codes[v] == 3))

    def tracks(rd, v):
        assert np.array_equal(rd.get_dosage_f64(v), world.want[v])
        g, pp, pi = rd.get_phased(v)
        eg, epp, epi = world.ref("phase", [v], lambda: world.dpg.phase(v, every))
        assert np.array_equal(eg, SS.calls(dcodes[v])) and _same_ints(g, SS.packed_2bit_ref(dcodes[v]))
        assert np.array_equal(_bits(pp, VS.N), epp != 0)
        assert np.array_equal(_bits(pi, VS.N) & _bits(pp, VS.N), (epi != 0) & (epp != 0))

    for entry, dsets, each in (("reader", world.hard, calls), ("reader_dosage", world.dose, tracks)):
        rd = dsets[placement].reader()

        def run():
            for v in dict.fromkeys(int(v) for v in lst):  # a repeated variant once
                each(rd, v)

        gets = ((rd.get_counts, rd.get_2bit, rd.get_int8, rd.get_missingness) if entry == "reader"
                else (rd.get_dosage_f64, rd.get_phased))
        try:
            _cell(entry, placement, name, L, run, [lambda get=get: get(int(lst[0])) for get in gets])
        finally:
            rd.close()


# ---- dosage ------------------------------------------------------------------------------------------------------

DOSAGE_REL = 1e-12  # test_dosage_tracks.REL, as test_score_over_dosage_tracks applies it below
DOSAGE_ROUTES = ((None, None), ("PGH_SCORE_DOSAGE_RECORDS", "0"), ("PGH_SCORE_DOSAGE_LANES", "1"))
SCORE_MODES = (("default", "SCORE_MEAN_IMPUTE"), ("no_mean_imputation", "SCORE_NO_MEAN_IMPUTATION"),
               ("center", "SCORE_CENTER"))


@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_dosage(gpu_lib, world, placement, name):
    L = gpu_lib
    ds, whole, want = world.dose[placement], world.dose["whole"], world.want
    lst = _variants(placement, name)
    forms = _forms_of(placement, name)

    def both(entry, call, make_ref):
        def run():
            ref = make_ref()
            for form, how in forms:
                got = call(ds, **_args(form, how))
                assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), (entry, form)
            assert call(whole, **_args(*forms[0])).tobytes() == ref.tobytes()

        _cell(entry, placement, name, L, run, [lambda kw=_args(form, how): call(ds, **kw) for form, how in forms])

    both("dosage_sums", lambda d, **kw: d.dosage_sums(**kw), lambda: SS.dosage_moments_ref(want[lst]))
    both("dosage_unpack", lambda d, **kw: d.dosage_unpack(**kw), lambda: want[lst])

    def samples():
        got = ds.dosage_unpack_samples(_u32(lst))
        assert got.shape == (VS.N, len(lst)) and np.array_equal(got, want[lst].T)
        assert got.tobytes() == whole.dosage_unpack_samples(_u32(lst)).tobytes()

    _cell("dosage_unpack_samples", placement, name, L, samples)

    def score():
        """plink_score over the tracks, through the three routes a sparse track is scored by."""
        for ncols in (1, 3):
            w, flip = VS.score_inputs(len(lst), ncols)
            for mode, const in SCORE_MODES:
                es, ed, eac = world.ref(("dscore", ncols, mode), lst,
                                        lambda: world.orc.score(world.dose_pg, lst, w, flip=flip, mode=mode))
                scale = np.abs(w).sum(axis=0) * 2.0
                for env, value in DOSAGE_ROUTES:
                    with pytest.MonkeyPatch.context() as mp:
                        if env:
                            mp.setenv(env, value)
                        with _written(L, name):
                            s, d, ac = ds.score(_u32(lst), w, flip=flip, mode=getattr(L, const))
                    # test_score_over_dosage_tracks' comparison
                    assert _same_ints(ac, eac), (ncols, mode, env)
                    assert np.all(np.abs(s - es) <= DOSAGE_REL * np.maximum(np.abs(es), 1e-3 * scale)), (ncols, mode, env)
                    assert np.allclose(d, ed, rtol=DOSAGE_REL, atol=1e-9), (ncols, mode, env)

    def refuse_score():
        w, flip = VS.score_inputs(len(lst), 1)
        ds.score(_u32(lst), w, flip=flip)

    _cell("score_dosage", placement, name, L, score, refuse_score)


# ---- score -------------------------------------------------------------------------------------------------------

SCORE_REL = 1e-6  # test_gpu_parity.REL, as test_score_matches_oracle applies it below
SCORE_COLS = (1, 9)


def _check_score(got, want, w, dosage_sum=True):
    """test_gpu_parity.test_score_matches_oracle's comparison (as tests/test_subset_shapes.py has it)."""
    (s, d, ac), (es, ed, eac) = got, want
    assert s.shape == es.shape and _same_ints(ac, eac)
    scale = np.abs(w).sum(axis=0) * 2.0  # magnitude of the terms being summed
    assert np.all(np.abs(s - es) <= SCORE_REL * np.maximum(np.abs(es), 1e-9 * scale))
    if dosage_sum:
        assert d.shape == ed.shape and np.allclose(d, ed, rtol=SCORE_REL, atol=1e-9)
    else:
        assert d is None


@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_score(gpu_lib, world, placement, name):
    import torch

    L = gpu_lib
    ds, whole, codes = world.hard[placement], world.hard["whole"], world.codes
    lst = _variants(placement, name)
    vidx = _u32(lst)

    def want_of(ncols, mode):
        w, flip = VS.score_inputs(len(lst), ncols)
        return w, flip, world.ref(("score", ncols, mode), lst,
                                  lambda: world.orc.score(world.pg, lst, w, flip=flip, mode=mode))

    def score():
        for ncols in SCORE_COLS:
            for mode, const in SCORE_MODES:
                w, flip, want = want_of(ncols, mode)
                code = getattr(L, const)
                with _written(L, name):
                    got = ds.score(vidx, w, flip=flip, mode=code)
                _check_score(got, want, w)
                _check_score(ds.score(vidx, w, flip=flip, mode=code, want_dosage_sum=False), want, w, False)
                if ncols > 1 and code != L.SCORE_CENTER:  # the unit column is the dosage sum, bit for bit
                    assert got[0][:, ncols - 1].tobytes() == got[1].tobytes()
                assert _same_ints(got[2], whole.score(vidx, w, flip=flip, mode=code)[2])
                if name == "empty":
                    assert not got[0].any() and not got[1].any() and not got[2].any()

    def counts():
        tallies = SS.counts_ref(codes[lst])
        for ncols in SCORE_COLS:
            for mode, const in SCORE_MODES:
                w, flip, want = want_of(ncols, mode)
                with _written(L, name):
                    got = ds.score(vidx, w, flip=flip, mode=getattr(L, const), counts=tallies)
                _check_score(got, want, w)

    def a_plan():
        """A kept plan, run twice."""
        for ncols in SCORE_COLS:
            w, flip, want = want_of(ncols, "default")
            plan_ = ds.score_plan(vidx, w, flip, L.SCORE_MEAN_IMPUTE)
            for _ in range(2):
                d_score = torch.full((VS.N, ncols), 7.0, dtype=torch.float64, device="cuda")
                d_dos = torch.full((VS.N,), 7.0, dtype=torch.float64, device="cuda")
                d_ac = torch.full((VS.N,), 7, dtype=torch.int32, device="cuda")
                plan_.run_dev(d_score.data_ptr(), d_dos.data_ptr(), d_ac.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                _check_score((d_score.cpu().numpy(), d_dos.cpu().numpy(), d_ac.cpu().numpy().astype(np.uint32)), want, w)
            plan_.close()

    w9, flip9 = VS.score_inputs(len(lst), 9)
    no_counts = np.ones((len(lst), 4), dtype=np.uint32)
    _cell("score", placement, name, L, score, lambda: ds.score(vidx, w9, flip=flip9))
    _cell("score_counts", placement, name, L, counts, lambda: ds.score(vidx, w9, flip=flip9, counts=no_counts))
    # (creating a plan has no output array: the status and the message)
    _cell("score_plan", placement, name, L, a_plan, lambda: ds.score_plan(vidx, w9, flip9, L.SCORE_MEAN_IMPUTE),
          outputs=False)


@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", SPARSE_CASES, ids=_ids(SPARSE_CASES))
def test_score_sparse(gpu_lib, world, placement, name):
    from test_score_sparse import _Case, _within

    L = gpu_lib
    lst = _variants(placement, name)
    vidx = _u32(lst)

    def run():
        for ncols in (1, 3):
            w, flip = VS.score_inputs(len(lst), ncols)
            w = w * np.array([1.0, 1e3, 1e-3])[None, :ncols]
            for _, const in SCORE_MODES:
                mode = getattr(L, const)
                case = world.ref(("sparse score", ncols, mode), lst, lambda: _Case(L, world.rare, lst, w, flip, mode, None))
                for mm in MAX_MINORS:
                    with _written(L, name):
                        score, dos, ac = world.sparse[(placement, mm)].score_sparse(vidx, w, flip, mode)
                    ctx = (placement, name, mm, ncols, mode)
                    assert score.shape == case.score.shape and _same_ints(ac, case.allele), ctx
                    # test_score_sparse's oracle and the header's bound of 1e-12 A for lists of at most 1024 variants
                    _within(score, case.score, case.A[None, :], 1e-12, ctx + ("score",))
                    _within(dos, case.dosage, np.float64(case.A_dos), 1e-12, ctx + ("dosage",))
                    assert _same_ints(ac, world.sparse[("sparse_whole", mm)].score_sparse(vidx, w, flip, mode)[2])

    w3, flip3 = VS.score_inputs(len(lst), 3)
    _cell("score_sparse", placement, name, L, run,
          [lambda mm=mm: world.sparse[(placement, mm)].score_sparse(vidx, w3, flip3) for mm in MAX_MINORS])


# ---- LD ----------------------------------------------------------------------------------------------------------

LD_WINDOW, LD_R2 = 50, 0.2137  # no band pair of any list sits on the threshold (the reference asserts it)


@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_ld(gpu_lib, world, placement, name):
    from test_ld_prune import windows

    L = gpu_lib
    ds, whole, codes = world.hard[placement], world.hard["whole"], world.codes
    lst = _variants(placement, name)
    forms = _forms_of(placement, name)
    sub = codes[lst] if name not in VS.OUTSIDE else None
    n = len(lst)

    def pairs():
        a, b = VS.ld_pair_lists(lst)
        got = ds.ld_pairs(a, b)
        assert _same_ints(got, VS.ld_pairs_ref(codes, a, b))
        assert _same_ints(got, whole.ld_pairs(a, b))

    _cell("ld_pairs", placement, name, L, pairs)

    def planes():
        return world.ref("ld planes", lst, lambda: SS.ld_planes(sub))

    def sums():
        for form, how in forms:
            assert _same_ints(ds.ld_window_sums(**_args(form, how)), planes().astype(np.uint32)), form
        if n > 130:  # a rectangle that starts inside a 96- and a 128-variant tile and ends in the ragged last ones
            rect = ds.ld_window_sums(**_args(*forms[0]), a_range=(90, n - 1), b_range=(1, n))
            assert _same_ints(rect, planes()[:, 90:n - 1, 1:n].astype(np.uint32))

    def band(entry, call):
        """call(dataset, window, win_end, **variants) makes the call and checks it against the reference of win_end."""
        def run():
            for window in sorted({min(LD_WINDOW, max(n, 1)), max(n, 1)}):  # the window of 50 and the full one
                for form, how in forms:
                    call(ds, window, windows(n, window), **_args(form, how))
                call(whole, window, windows(n, window), **_args(*forms[0]))

        _cell(entry, placement, name, L, run,
              [lambda kw=_args(form, how): call(ds, LD_WINDOW, None, **kw) for form, how in forms])

    kept = {}

    def prune(d, window, win_end, **kw):
        keep = d.ld_prune(LD_R2, window=window, **kw)
        want = world.ref(("prune", window), lst, lambda: SS.ld_prune_ref(planes(), sub, win_end, LD_R2, near=1e-12))
        assert keep.dtype == bool and np.array_equal(keep, want), (window, kw.keys())

    def scores(d, window, win_end, **kw):
        for unbiased in (False, True):  # test_ld_scores.check_against_brute: partners equal, scores within its bound
            score, partners = d.ld_scores(window=window, unbiased=unbiased, want_counts=True, **kw)
            exp, bound, exp_n = world.ref(("ld scores", window, unbiased), lst,
                                          lambda: SS.ld_scores_ref(planes(), sub, win_end, unbiased))
            assert score.dtype == np.float64 and _same_ints(partners, exp_n)
            err = np.abs(score - exp)
            assert (err <= bound).all(), (window, unbiased, int(np.argmax(err - bound)), float(err.max()))
            # a function of the variant list alone (the header): the same bytes from every placement and form
            assert kept.setdefault((window, unbiased), score.tobytes()) == score.tobytes()

    _cell("ld_window_sums", placement, name, L, sums,
          [lambda kw=_args(form, how): ds.ld_window_sums(**kw) for form, how in forms])
    band("ld_prune", prune)
    band("ld_scores", scores)


# ---- pair matrices -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_pair_matrices(gpu_lib, world, placement, name):
    from test_grm import Yardstick, check
    from test_king import brute_counts

    L = gpu_lib
    ds, whole, codes = world.hard[placement], world.hard["whole"], world.codes
    lst = _variants(placement, name)
    forms = _forms_of(placement, name)
    sub = codes[lst] if name not in VS.OUTSIDE else None

    def counts_ref():
        return world.ref("king counts", lst, lambda: brute_counts(sub))

    def king_counts():
        for form, how in forms:
            assert _same_ints(ds.king_counts(**_args(form, how)), counts_ref()), form
        corner = whole.king_counts(**_args(*forms[0]), i_range=(900, VS.N), j_range=(0, 130))
        assert _same_ints(corner, counts_ref()[:, 900:, :130])

    def king_table():
        i, j, nsnp, hethet, ibs0, h1, h2, kin = world.ref("king table", lst, lambda: VS.king_table_ref(counts_ref()))
        for form, how in forms:
            table = ds.king_table(**_args(form, how))
            assert len(table) == VS.N * (VS.N - 1) // 2
            for key, want in (("i", i), ("j", j), ("nsnp", nsnp), ("hethet", hethet), ("ibs0", ibs0), ("het1hom2", h1),
                              ("het2hom1", h2)):
                assert np.array_equal(table[key].astype(np.int64), want), (key, form)
            assert table["kinship"].tobytes() == kin.tobytes(), form  # the formula of its own counts, bit for bit
        cut = 0.0884
        with np.errstate(invalid="ignore"):
            passing = kin >= cut
        filtered = ds.king_table(cut, **_args(*forms[0]))
        assert np.array_equal(filtered["i"], i[passing]) and np.array_equal(filtered["j"], j[passing])

    def grm():
        freq = VS.supplied_freq(len(lst))
        for f in (None, freq):  # test_grm's derived bound, with the counted and with supplied frequencies
            y = world.ref(("grm", f is not None), lst, lambda: Yardstick(sub, freq=f))
            for form, how in forms:
                rel, nobs, n_used = ds.grm(**_args(form, how), freq=f)
                check(rel, nobs, n_used, y)
            rel, nobs, n_used = whole.grm(**_args(*forms[0]), freq=f, meanimpute=True, i_range=(900, VS.N), j_range=(0, 130))
            check(rel, nobs, n_used, y, rows=np.arange(900, VS.N), cols=np.arange(130), meanimpute=True)

    for entry, run, call in (("king_counts", king_counts, lambda **kw: ds.king_counts(**kw)),
                             ("king_table", king_table, lambda **kw: ds.king_table(**kw)),
                             ("grm", grm, lambda **kw: ds.grm(**kw))):
        _cell(entry, placement, name, L, run, [lambda kw=_args(form, how), call=call: call(**kw) for form, how in forms])


# ---- plink_pca ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_pca(gpu_lib, world, placement, name):
    L, orc = gpu_lib, world.orc
    ds, codes = world.hard[placement], world.codes
    lst = _variants(placement, name)
    n_pcs = 2
    g1 = orc.fill_g1(VS.N, 2 * n_pcs)

    def run():
        sub = codes[lst]
        ev, vecs, keep, spectrum = world.ref("pca", lst, lambda: SS.pca_ref(sub, n_pcs, g1))
        assert len(keep) >= PCA_MIN - 4 and spectrum[0] > 1.1 * spectrum[1] and spectrum[1] > 1.1 * spectrum[2]  # separated
        _, center, inv = SS.freq_norm(SS.counts_ref(sub))
        got_ev, got_vecs = ds.pca(_u32(lst[keep]), center, inv, n_pcs, g1)
        # test_gpu_parity.test_pca_matches_oracle_on_wide_rows, exactly as tests/test_subset_shapes.py applies it:
        # eigenvalues within 1e-6, an orthonormal basis within 1e-8, the eigenvectors within 1e-5 (each up to its sign)
        assert np.allclose(got_ev, ev, rtol=1e-6)
        assert np.allclose(got_vecs.T @ got_vecs, np.eye(n_pcs), atol=1e-8)
        assert np.allclose(got_vecs @ got_vecs.T @ vecs, vecs, atol=1e-5)
        for c in range(n_pcs):
            sign = np.sign(np.dot(got_vecs[:, c], vecs[:, c]))
            assert np.allclose(got_vecs[:, c], sign * vecs[:, c], atol=1e-5), c

    def refuse():
        k = len(lst)
        ds.pca(_u32(lst), np.ones(k), np.ones(k), n_pcs, g1)

    _cell("pca", placement, name, L, run, refuse)


# ---- the GLMs over ranges ----------------------------------------------------------------------------------------

GLM_KEYS = ("beta", "se", "stat", "p", "a1_freq", "obs_ct", "errcode", "firth")


def _rows_equal(a, b, rows_a, rows_b, keys=GLM_KEYS, ctx=None):
    """The rows rows_a of output a and rows_b of output b hold the same bytes."""
    for key in keys:
        x, y = a[key][rows_a], b[key][rows_b]
        if x.dtype == object:
            assert x.tolist() == y.tolist(), (key, ctx)
        else:
            assert x.tobytes() == y.tobytes(), (key, ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_glm_dense(gpu_lib, world, placement, name):
    orc = pytest.importorskip("glm_oracle")
    L = gpu_lib
    ds, whole = world.hard[placement], world.hard["whole"]
    b, e = VS.resident(placement)
    span = VS.as_range(name, b, e)
    x, z, y_lin, y_bin = world.pg.vals, world.z, world.y_lin, world.y_bin

    def everything(d, kind):
        """The call over a dataset's whole resident range, made once."""
        key = ("glm whole", kind, id(d))
        if key not in world._cache:
            world._cache[key] = (d.glm(y_lin[0], z, model="linear") if kind == "linear" else
                                 d.glm(y_bin[0], z, model="logistic") if kind == "logistic" else
                                 d.glm_multi(y_lin[:2], z, model="linear") if kind == "multi linear" else
                                 d.glm_multi(y_bin[:2], z, model="logistic"))
        return world._cache[key]

    def glm():
        v0, v1 = span
        idx = range(v0, v1)
        lin = ds.glm(y_lin[0], z, model="linear", v_begin=v0, v_end=v1)
        log = ds.glm(y_bin[0], z, model="logistic", v_begin=v0, v_end=v1)
        assert len(lin["beta"]) == len(log["beta"]) == v1 - v0
        # test_glm_gpu / test_glm_widths_chunks: 1e-9 for the linear fit, 1e-6 for the logistic one, on check_rows' scale
        fitted = orc.check_rows(lin, x, y_lin[0], z, "linear", rel=1e-9, idx=idx, got_idx=lambda i: i - v0)
        fitted += orc.check_rows(log, x, y_bin[0], z, "logistic", rel=1e-6, idx=idx, got_idx=lambda i: i - v0)
        if v1 - v0 >= 63:
            assert fitted >= v1 - v0
        # a variant's row does not depend on the variants around it (tile, chunk or shard): the same bytes as in the
        # call over the whole resident range, of this placement and of the whole dataset
        for got, kind in ((lin, "linear"), (log, "logistic")):
            _rows_equal(got, everything(ds, kind), slice(None), slice(v0 - b, v1 - b), ctx=(kind, placement, name))
            _rows_equal(got, everything(whole, kind), slice(None), slice(v0, v1), ctx=(kind, "whole", name))

    def multi():
        v0, v1 = span
        idx = range(v0, v1)
        lin = ds.glm_multi(y_lin[:2], z, model="linear", v_begin=v0, v_end=v1)
        log = ds.glm_multi(y_bin[:2], z, model="logistic", v_begin=v0, v_end=v1)
        assert lin["beta"].shape == log["beta"].shape == (v1 - v0, 2)
        for p in range(2):
            orc.check_rows({k: v[:, p] for k, v in lin.items()}, x, y_lin[p], z, "linear", rel=1e-9, idx=idx,
                           got_idx=lambda i: i - v0)
        orc.check_rows({k: v[:, 1] for k, v in log.items()}, x, y_bin[1], z, "logistic", rel=1e-6, idx=idx,
                       got_idx=lambda i: i - v0)
        # a logistic row is pgh_glm's bit for bit, hence the whole call's of any placement too
        _rows_equal({k: v[:, 0] for k, v in log.items()}, everything(whole, "logistic"), slice(None), slice(v0, v1))
        _rows_equal(log, everything(ds, "multi logistic"), slice(None), slice(v0 - b, v1 - b))
        # a linear row agrees with pgh_glm's in errcode, obs_ct and a1_freq bit for bit
        _rows_equal({k: v[:, 0] for k, v in lin.items()}, everything(whole, "linear"), slice(None), slice(v0, v1),
                    keys=("errcode", "obs_ct", "a1_freq"))

    _cell("glm", placement, name, L, glm, lambda: ds.glm(y_lin[0], z, v_begin=span[0], v_end=span[1]))
    _cell("glm_multi", placement, name, L, multi, lambda: ds.glm_multi(y_lin[:2], z, v_begin=span[0], v_end=span[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", SPARSE_CASES, ids=_ids(SPARSE_CASES))
def test_glm_sparse(gpu_lib, world, placement, name):
    glm = pytest.importorskip("glm_oracle")
    import glm_score_oracle as O
    import glm_spa_oracle as S
    from test_glm_score_sparse_spa import CUTOFF, TOL

    L = gpu_lib
    b, e = VS.resident(placement)
    span = VS.as_range(name, b, e)
    x, z, y_lin, y_bin = world.rx, world.rz, world.ry_lin, world.ry_bin
    nul = world.ref("null", [], lambda: O.Null(y_bin, z))
    assert nul.status is None
    calls = {
        "glm_sparse": lambda d, v0, v1: d.glm_sparse(y_lin, z, v_begin=v0, v_end=v1),
        "glm_score_sparse": lambda d, v0, v1: d.glm_score_sparse(y_bin, z, v_begin=v0, v_end=v1),
        "glm_score_sparse_spa": lambda d, v0, v1: d.glm_score_sparse_spa(y_bin, z, cutoff=CUTOFF, v_begin=v0, v_end=v1),
    }

    def everything(d, entry):
        key = ("sparse whole", entry, id(d))
        if key not in world._cache:
            world._cache[key] = calls[entry](d, d.v_begin, d.v_end)
        return world._cache[key]

    for entry, call in calls.items():
        def run():
            v0, v1 = span
            idx = range(v0, v1)
            for mm in MAX_MINORS:
                ds, whole = world.sparse[(placement, mm)], world.sparse[("sparse_whole", mm)]
                got = call(ds, v0, v1)
                assert len(got["beta"]) == v1 - v0
                if entry == "glm_sparse":  # test_glm_sparse's 1e-9 against glm_oracle
                    glm.check_rows(got, x, y_lin, z, "linear", rel=1e-9, idx=idx, got_idx=lambda i: i - v0)
                else:  # test_glm_score_sparse.REL = 1e-9; test_glm_score_sparse_spa.TOL for the saddlepoint
                    O.check_rows(got, x, nul, rel=1e-9, idx=idx, got_idx=lambda i: i - v0)
                keys = GLM_KEYS
                if entry == "glm_score_sparse_spa":
                    keys = GLM_KEYS + ("p_spa", "spa_state")
                    row_forms = [S.row_form(world.rare[i], mm) for i in idx]  # the form comes from all raw samples
                    S.check_spa(got, x[v0:v1], world.rare[v0:v1], nul, row_forms, CUTOFF, TOL)
                    _rows_equal(got, everything(ds, "glm_score_sparse"), slice(None), slice(v0 - b, v1 - b))
                # a row is a function of its variant's entries, the phenotype and the covariates only: not of v_begin,
                # the window the dataset was opened with or the rows around it
                _rows_equal(got, everything(ds, entry), slice(None), slice(v0 - b, v1 - b), keys, (entry, mm, placement))
                _rows_equal(got, everything(whole, entry), slice(None), slice(v0, v1), keys, (entry, mm, "whole"))

        _cell(entry, placement, name, L, run,
              [lambda mm=mm, call=call: call(world.sparse[(placement, mm)], *span) for mm in MAX_MINORS])


# ---- the set tests -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("placement,name", SPARSE_CASES, ids=_ids(SPARSE_CASES))
def test_set_tests(gpu_lib, world, placement, name):
    """One set per list, set_vidx in the dataset-local convention (0 names the first resident variant), between two
    other sets so that its memberships do not start at offset 0."""
    import skat_oracle as K
    from test_burden_sparse import _check as burden_check, _csr, _expected as burden_expected, _Forms
    from test_skat_sparse import check as skat_check

    L = gpu_lib
    b, e = VS.resident(placement)
    lst = _variants(placement, name)
    lead, trail = np.array([VS.HET_ROWS[0], VS.MADE_ROWS[0]]), np.array([VS.HET_ROWS[1]])
    sets = [lead, lst, trail]
    off, glob = _csr([s.astype(np.uint32) for s in sets])
    local = (np.concatenate(sets) - b).astype(np.uint32)  # outside_low: b - 1 - b wraps to 2^32 - 1
    assert len(local) == len(glob)
    weights = VS.set_weights(len(local))
    z, y_lin, y_bin = world.rz, world.ry_lin, world.ry_bin

    def burden():
        for mm in MAX_MINORS:
            forms = _Forms(world.rare, mm, world.pitch)
            rows = world.sparse[(placement, mm)].burden_sparse(y_lin, off, local, weights, z)
            # test_burden_sparse's oracle and its 1e-9
            burden_check(L, rows, burden_expected(world.rare, forms, sets, weights, y_lin, z), rel=1e-9, ctx=(placement, name, mm))
            # a set's row is a function of its memberships and weights alone: the whole dataset, the same global variants
            again = world.sparse[("sparse_whole", mm)].burden_sparse(y_lin, off, glob, weights, z)
            assert rows.tobytes() == again.tobytes(), (placement, name, mm)

    def skat():
        nul = world.ref("skat null", [], lambda: K.Null(y_bin, z))
        for mm in MAX_MINORS:
            forms = _Forms(world.rare, mm, world.pitch)
            rows, lam = world.sparse[(placement, mm)].skat_sparse(y_bin, off, local, weights, z, return_lambda=True)
            exp, pos = [], 0
            for members in sets:
                exp.append(K.oracle_row(world.rare, forms, members, weights[pos:pos + len(members)], nul))
                pos += len(members)
            skat_check(L, rows, lam, exp, off, ctx=(placement, name, mm))  # test_skat_sparse's oracle and its REL
            again, lam2 = world.sparse[("sparse_whole", mm)].skat_sparse(y_bin, off, glob, weights, z, return_lambda=True)
            assert rows.tobytes() == again.tobytes() and lam.tobytes() == lam2.tobytes(), (placement, name, mm)

    def refuse(call):
        return [lambda mm=mm: call(world.sparse[(placement, mm)]) for mm in MAX_MINORS]

    def burden_call(d):
        return d.burden_sparse(y_lin, off, local, weights, z)

    def skat_call(d):
        return d.skat_sparse(y_bin, off, local, weights, z, return_lambda=True)

    _cell("burden_sparse", placement, name, L, burden, refuse(burden_call))
    _cell("skat_sparse", placement, name, L, skat, refuse(skat_call))


# ---- the count ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_the_grid_is_counted(gpu_lib):
    """Every cell of every entry point whose family ran was run or pinned to its refusal, as plan() says; what is
    left are the cells of EXCLUDED."""
    cells = grid()
    ran = {entry for entry, _, _ in _Grid.done}
    assert ran, "run the file as a whole: this test counts what the others did"
    missing = [(cell, outcome) for cell, (outcome, _) in cells.items()
               if cell[0] in ran and outcome != "excluded" and _Grid.done.get(cell) != outcome]
    assert not missing, missing[:10]
    extra = [cell for cell in _Grid.done if cells[cell][0] == "excluded"]
    assert not extra, extra[:10]
    if ran == set(ENTRIES):
        counts = {k: sum(1 for o in _Grid.done.values() if o == k) for k in ("run", "refused")}
        left = sum(1 for outcome, _ in cells.values() if outcome == "excluded")
        print(f"grid: {counts['run']} cells run, {counts['refused']} refused, {left} excluded of {len(cells)}")
        assert counts["run"] + counts["refused"] + left == len(cells)
