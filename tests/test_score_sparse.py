"""pgh_score_sparse / Dataset.score_sparse: plink_score's per-sample sums over a sparse-resident dataset, from the
listed variants' entries, in int64 fixed point.

The oracle is numpy over the unpacked calls: the reference's formula (src/plink_score.cpp:598-652, hardcalls) term by
term in float64 -- weight * value, as the reference multiplies -- and math.fsum per sample and column, i.e. the exact
sum of those terms.  allele_ct is summed in integers.

Bound.  The header states |score - exact| <= (n + 16) 2^-53 A_c + E 2^-(62 - L) D_c with n = n_scored,
L = ceil(log2 n), E <= n the sample's entries, D_c <= 2 A_c and A_c = sum_i |W[i][c]| max_g |ts_i[g]|; for n <= 1024
that is below 1e-12 A_c, which is what every value is held to here (dosage_sum: A = sum_i max_g |td_i[g]|).  The
longest list of this file has 323 variants, for which the same formula gives (339 2^-53 + 2 * 323 * 2^-53) A_c =
1.1e-13 A_c per resident form: two forms of one file (other base codes, other K_c) are therefore within 1e-12 A_c of
each other.  Against Dataset.score on the dense dataset the issue's 2e-12 A_c holds.  Same call, same column in another
call, another window at open, another number of row slices: bit for bit.

N = 20,011 samples is no multiple of 64 and spans at least two sample tiles at every tile size the kernel takes: the
widest tile (one weight column, no dosage sum) holds 10,880 samples."""

import ctypes as C
import math
import os
import types

import numpy as np
import pytest

from conftest import ROOT

import pgen_writer as W

M, N = 400, 20011
NEW_SYMBOLS = ["pgh_score_sparse"]
# the special rows of the file
R_NONE, R_ONE, R_THREE, R_200, R_HET, R_ALT, R_MISS, R_ALLMISS, R_MONO, R_LAST, R_EDGES, R_COMMON = range(12)


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_score_sparse(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "score_sparse")


def test_wrapper_checks_shapes_before_the_library_is_called(lib):
    """The stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    good = dict(vidx=np.array([1, 4, 7]), weights=np.ones((3, 2)))
    for bad, text in ((dict(weights=np.ones((2, 2))), "weights"), (dict(weights=np.ones(4)), "weights"),
                      (dict(weights=np.ones((3, 2, 1))), "weights"), (dict(flip=np.zeros(2)), "flip"),
                      (dict(vidx=np.array([[1, 4, 7]])), "vidx"), (dict(vidx=np.array([1, -4, 7])), "vidx"),
                      (dict(vidx=np.array([1.0, 4.0, 7.0])), "vidx"), (dict(vidx=np.array([1, 4, 2 ** 32])), "vidx")):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match=text):
            lib.Dataset.score_sparse(fake, **kw)


def test_a_null_dataset_is_refused_without_a_device(lib):
    score = np.full(4, 0xAB, dtype=np.uint8).repeat(8).view(np.float64)
    dos, ac = score.copy(), np.full(4, 0xABABABAB, dtype=np.uint32)
    before = (score.tobytes(), dos.tobytes(), ac.tobytes())
    vidx, w = np.array([0, 1], dtype=np.uint32), np.ones(2)
    eb = C.create_string_buffer(lib.ERRBUF_LEN)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.raw().pgh_score_sparse(None, None, 2, p(vidx), p(w), None, 1, lib.SCORE_MEAN_IMPUTE, p(score), p(dos),
                                    p(ac), eb)
    assert rc == lib.PGH_ERR_ARG and b"null dataset" in eb.value
    assert (score.tobytes(), dos.tobytes(), ac.tobytes()) == before


# ---- the file ----------------------------------------------------------------------------------------------------

def _tiles(L):
    """Every tile size the kernel takes: n_acc accumulators of 8 bytes and 4 bytes per sample in the LDS budget."""
    return sorted({L.SCORE_SPARSE_ACC_BYTES // (8 * a + 4) // 64 * 64 for a in range(1, L.SCORE_SPARSE_CHUNK + 2)})


def _matrix(L):
    rng = np.random.default_rng(20011)
    geno = np.zeros((M, N), dtype=np.uint8)
    for v in range(M):  # hom-ref majority, rare carriers
        hit = rng.random(N) < float(rng.choice([0.0005, 0.002, 0.01]))
        geno[v, hit] = rng.integers(1, 4, hit.sum(), dtype=np.uint8)
    tiles = _tiles(L)
    assert max(tiles) < N, "raise N: the widest tile must leave a second one"
    last_start = max((N - 1) // t * t for t in tiles)  # samples from here on are in the last, partial tile of all
    assert N - last_start < 64 and N % 64 != 0
    geno[R_NONE] = 0
    geno[R_ONE] = 0
    geno[R_ONE, 7000] = 1  # (the subset below drops this sample: the row is monomorphic there)
    geno[R_THREE] = 0
    geno[R_THREE, [64, 9999, 20010]] = [1, 2, 3]
    geno[R_200] = 0
    geno[R_200, rng.choice(N, 200, replace=False)] = rng.integers(1, 4, 200, dtype=np.uint8)
    for row, major, rate in ((R_HET, 1, 0.2), (R_ALT, 2, 0.15), (R_MISS, 3, 0.3)):
        geno[row] = major
        hit = rng.random(N) < rate
        geno[row, hit] = rng.integers(0, 4, hit.sum(), dtype=np.uint8)
    geno[R_ALLMISS] = 3
    geno[R_MONO] = 2
    geno[R_LAST] = 0
    geno[R_LAST, [last_start, last_start + 5, N - 1]] = [1, 2, 1]
    geno[R_EDGES] = 0
    edges = sorted({s for t in tiles for s in (0, t - 1, t, 2 * t - 1, N // t * t) if s < N} | {N - 1})
    geno[R_EDGES, edges] = rng.integers(1, 4, len(edges), dtype=np.uint8)
    geno[R_COMMON] = rng.binomial(2, 0.3, N)
    geno[R_COMMON, rng.random(N) < 0.02] = 3
    # every record type where its difference list stays short (a long one only costs the writer time); R_LAST is the
    # inverse of the row before it but for three calls
    rng_k = np.random.default_rng(5)
    kinds, base = [], None
    for g in geno:
        options = [0, 1] + [k for k, const in ((4, 0), (6, 2), (7, 3)) if (g != const).sum() < 300]
        if base is not None:
            options += [k for k, target in ((2, g), (3, W._INV[g])) if (target != base).sum() < 300]
        kinds.append({R_MONO: 6, R_ALLMISS: 7, R_LAST: 3}.get(len(kinds), int(rng_k.choice(options))))
        if kinds[-1] not in (2, 3):
            base = g
    assert set(kinds) == {0, 1, 2, 3, 4, 6, 7}, sorted(set(kinds))
    return geno, kinds


def _tables(G, flip, mode, L):
    """ts, td (value per class), inc (allele increments: classes 0..2, missing) of every row of G."""
    nv = G.shape[0]
    ts, td, inc = np.zeros((nv, 4)), np.zeros((nv, 4)), np.zeros((nv, 2), dtype=np.int64)
    for i in range(nv):
        het, alt, nm = int((G[i] == 1).sum()), int((G[i] == 2).sum()), int((G[i] != 3).sum())
        if nm == 0:
            continue
        mean_alt = (float(het) + 2.0 * float(alt)) / float(nm)
        scored = [2.0 - g if flip[i] else float(g) for g in range(3)]
        mean_scored = 2.0 - mean_alt if flip[i] else mean_alt
        if mode == L.SCORE_CENTER:
            freq = mean_alt / 2.0
            sd = math.sqrt(2.0 * freq * (1.0 - freq))
            if sd == 0.0:
                continue
            ts[i, :3] = [(s - mean_scored) / sd for s in scored]
            inc[i] = [2, 0]
        else:
            ts[i, :3] = td[i, :3] = scored
            inc[i] = [2, 0]
            if mode == L.SCORE_MEAN_IMPUTE:
                ts[i, 3] = td[i, 3] = mean_scored
                inc[i] = [2, 2]
    return ts, td, inc


def _fsum_rows(T):
    return np.array([math.fsum(r) for r in T.T.tolist()])


class _Case:
    """One (list, weights, flip, mode, subset) and its oracle, computed once."""

    def __init__(self, L, geno, vidx, weights, flip, mode, keep):
        self.vidx, self.weights, self.flip, self.mode, self.keep = vidx, weights, flip, mode, keep
        G = geno[vidx] if keep is None else geno[vidx][:, keep]
        self.G = G
        ts, td, inc = _tables(G, flip, mode, L)
        self.ts = ts
        rows = np.arange(len(vidx))[:, None]
        val = ts[rows, G]
        self.score = np.stack([_fsum_rows(weights[:, c, None] * val) for c in range(weights.shape[1])], axis=1)
        self.dosage = _fsum_rows(td[rows, G])
        self.allele = np.where(G == 3, inc[:, 1, None], inc[:, 0, None]).sum(axis=0).astype(np.uint32)
        self.A = (np.abs(weights) * np.abs(ts).max(axis=1)[:, None]).sum(axis=0)
        self.A_dos = np.abs(td).max(axis=1).sum()


class _World:
    def __init__(self, L, tmp):
        self.L = L
        self.geno, kinds = _matrix(L)
        self.path = str(tmp / "score_sparse.pgen")
        W.write_pgen(self.path, self.geno, kinds)
        self.dense = L.Dataset.open(self.path)
        self.pitch = self.dense.info.pitch_bytes
        # the default rule, nearly every row dense-form, every row sparse (base codes 0..3)
        self.forms = {mm: L.Dataset.open(self.path, sparse=True, max_minor=mm) for mm in (0, 1, N)}
        info = {mm: sp.sparse_info() for mm, sp in self.forms.items()}
        assert info[0].dense_variant_ct >= 4 and info[0].sparse_variant_ct > M - 20
        assert info[1].dense_variant_ct > M - 10 and info[1].sparse_variant_ct >= 4
        assert info[N].dense_variant_ct == 0 and all(info[N].base_hist[b] > 0 for b in range(4))
        rng = np.random.default_rng(99)
        special = np.arange(12)
        rest = np.arange(12, M)
        self.lists = {"mini": np.concatenate([special, rest[::8]]).astype(np.uint32),            # 61 variants
                      "short": np.concatenate([special, rest[::4]]).astype(np.uint32),           # 109
                      "long": np.concatenate([special, rest[rest % 5 != 0]]).astype(np.uint32)}  # 323
        self.long = self.lists["long"]
        assert len(self.long) == 323 and np.all(np.diff(self.long) > 0) and np.any(np.diff(self.long) > 1)
        self.w17 = rng.normal(size=(M, 17)) * 10.0 ** rng.integers(-3, 4, 17)[None, :]
        self.w17[:, 4] = 1.0  # a unit column: the dense path copies it into the dosage sum
        self.flip = (rng.random(M) < 0.4).astype(np.uint8)
        self.keep = np.arange(N) % 3 != 1  # a third of the samples is out
        assert (self.geno[R_200][~self.keep] != 0).sum() > 30 and not self.keep[7000] and not self.keep[64]
        self.subsets = {}
        self.cases = {}

    def subset(self, ds):
        key = id(ds)
        if key not in self.subsets:
            self.subsets[key] = ds.subset(self.keep)
        return self.subsets[key]

    def case(self, name):
        """name: (list, columns, mode, subset?) -- the oracle of each is computed once and shared."""
        if name not in self.cases:
            which, cols, mode, sub = name
            vidx = self.lists[which]
            self.cases[name] = _Case(self.L, self.geno, vidx, np.ascontiguousarray(self.w17[vidx][:, list(cols)]),
                                     self.flip[vidx], mode, self.keep if sub else None)
        return self.cases[name]

    def close(self):
        for s in self.subsets.values():
            s.close()
        for d in list(self.forms.values()) + [self.dense]:
            d.close()


@pytest.fixture(scope="module")
def world(gpu_lib, tmp_path_factory):
    w = _World(gpu_lib, tmp_path_factory.mktemp("score_sparse"))
    yield w
    w.close()


def _run(world, ds, case, dosage_sum=True, sparse=True):
    ss = world.subset(ds) if case.keep is not None else None
    if sparse:
        return ds.score_sparse(case.vidx, case.weights, case.flip, case.mode, ss, dosage_sum)
    return ds.score(case.vidx, case.weights, case.flip, case.mode, ss, dosage_sum)


def _within(got, want, scale, factor, ctx):
    err = np.abs(got - want)
    bound = factor * scale
    worst = float((err / np.where(scale > 0, scale, 1.0)).max()) if err.size else 0.0
    print(ctx, "largest error / A =", worst)
    assert np.all(err <= bound), (ctx, worst)


COLS17 = tuple(range(17))
CASES = [
    # list, columns, mode, subset
    ("long", (5,), 0, False),
    ("short", (0, 9, 16), 0, False),
    ("mini", COLS17, 0, False),
    ("short", (0, 9, 16), 1, True),
    ("short", (2,), 1, False),
    ("short", (0, 9, 16), 2, False),
    ("short", (11,), 2, True),
    ("short", (3, 4), 0, True),
]


# ---- on the GPU --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES, ids=lambda n: f"{n[0]}-{len(n[1])}col-mode{n[2]}-{'subset' if n[3] else 'all'}")
def test_bound_exact_allele_ct_dense_path_and_forms(gpu_lib, world, name):
    L = gpu_lib
    case = world.case(name)
    n_cols = len(name[1])
    if n_cols == 17:
        assert n_cols > L.SCORE_SPARSE_CHUNK  # more than one column chunk (three: 8 + 8 + 1)
    d_score, d_dos, d_ac = _run(world, world.dense, case, sparse=False)
    got = {}
    for mm, sp in world.forms.items():
        score, dos, ac = _run(world, sp, case)
        ctx = (name, mm)
        assert score.shape == case.score.shape and dos.shape == case.dosage.shape
        _within(score, case.score, case.A[None, :], 1e-12, ctx + ("score",))
        _within(dos, case.dosage, np.float64(case.A_dos), 1e-12, ctx + ("dosage",))
        assert np.array_equal(ac, case.allele), ctx
        _within(score, d_score, case.A[None, :], 2e-12, ctx + ("score vs dense",))
        _within(dos, d_dos, np.float64(case.A_dos), 2e-12, ctx + ("dosage vs dense",))
        assert np.array_equal(ac, d_ac), ctx
        # without the dosage sum: the same scores and counts, bit for bit (other tiles)
        score2, none, ac2 = _run(world, sp, case, dosage_sum=False)
        assert none is None and score2.tobytes() == score.tobytes() and ac2.tobytes() == ac.tobytes(), ctx
        got[mm] = (score, dos)
    for a, b in ((0, 1), (0, N), (1, N)):
        _within(got[a][0], got[b][0], case.A[None, :], 1e-12, (name, a, b, "forms"))
        _within(got[a][1], got[b][1], np.float64(case.A_dos), 1e-12, (name, a, b, "forms, dosage"))


@pytest.mark.gpu
def test_the_skip_rules_and_the_special_rows(gpu_lib, world):
    """One listed variant at a time, unit weight: the special rows do what the reference does with them."""
    L = gpu_lib
    sp = world.forms[N]
    for row in (R_ALLMISS, R_MONO, R_NONE, R_ONE, R_LAST, R_EDGES, R_MISS):
        for mode in (0, 1, 2):
            case = _Case(L, world.geno, np.array([row], dtype=np.uint32), np.array([[1.5]]), np.array([0], np.uint8),
                         mode, None)
            score, dos, ac = sp.score_sparse(case.vidx, case.weights, case.flip, mode)
            _within(score, case.score, case.A[None, :], 1e-12, (row, mode))
            _within(dos, case.dosage, np.float64(case.A_dos), 1e-12, (row, mode, "dosage"))
            assert np.array_equal(ac, case.allele), (row, mode)
            skipped = row == R_ALLMISS or (mode == 2 and row in (R_MONO, R_NONE))
            assert (not ac.any() and not score.any()) == skipped, (row, mode)


@pytest.mark.gpu
def test_same_bytes_again_per_column_per_window_and_per_slice_count(gpu_lib, world):
    L = gpu_lib
    case = world.case(("mini", COLS17, 0, False))
    for mm, sp in world.forms.items():
        want = _run(world, sp, case)
        again = _run(world, sp, case)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, again)), (mm, "again")
        # a column alone (another tile size, another chunk) and at another place among other columns
        for j in range(17):
            alone = sp.score_sparse(case.vidx, case.weights[:, j], case.flip, case.mode)
            assert alone[0][:, 0].tobytes() == want[0][:, j].tobytes(), (mm, j)
            assert alone[1].tobytes() == want[1].tobytes() and alone[2].tobytes() == want[2].tobytes(), (mm, j)
        shuffled = [16, 3, 0, 8, 12]
        part = sp.score_sparse(case.vidx, case.weights[:, shuffled], case.flip, case.mode)
        assert part[0].tobytes() == np.ascontiguousarray(want[0][:, shuffled]).tobytes(), (mm, "shuffled")
        # the row slices: global adds across several workgroups per tile
        for slices in ("1", "3", "16"):
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv(L.SCORE_SPARSE_SLICES_ENV, slices)
                sliced = _run(world, sp, case)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(want, sliced)), (mm, slices)
        # several windows at open against one
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(37 * world.pitch))
            other = L.Dataset.open(world.path, sparse=True, max_minor=mm)
        windows = _run(world, other, case)
        other.close()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, windows)), (mm, "windows")


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched_and_the_library_usable(gpu_lib, world):
    L = gpu_lib
    sp = world.forms[0]
    group = L.Dataset.open_sharded(world.path, [0, 0])
    other_ss = world.subset(world.forms[1])
    vidx = np.array([3, 5, 11], dtype=np.uint32)
    good = np.array([[1.0, 2.0], [0.5, -1.0], [3.0, 0.25]])
    nan_w, inf_w = good.copy(), good.copy()
    nan_w[1, 1] = float("nan")
    inf_w[2, 0] = float("-inf")

    def call(ds, v, w, n_cols=None, mode=0, subset=None):
        n_cols = w.shape[1] if n_cols is None else n_cols
        score = np.full(N * max(1, n_cols), 0xAB, dtype=np.uint8).repeat(8).view(np.float64)
        dos = np.full(N, 0xAB, dtype=np.uint8).repeat(8).view(np.float64)
        ac = np.full(N, 0xABABABAB, dtype=np.uint32)
        before = (score.tobytes(), dos.tobytes(), ac.tobytes())
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = L.raw().pgh_score_sparse(ds._h, subset._h if subset else None, len(v), p(v), p(w), None, n_cols, mode,
                                      p(score), p(dos), p(ac), eb)
        return rc, eb.value.decode(), (score.tobytes(), dos.tobytes(), ac.tobytes()) == before

    cases = [
        ("needs a sparse-resident dataset", (world.dense, vidx, good), {}),
        ("one device's dataset", (group, vidx, good), {}),
        ("non-finite weight at variant 1, column 1", (sp, vidx, nan_w), {}),
        ("non-finite weight at variant 2, column 0", (sp, vidx, inf_w), {}),
        ("n_cols must be between 1 and 4096", (sp, vidx, good), dict(n_cols=0)),
        ("unknown score mode", (sp, vidx, good), dict(mode=3)),
        ("outside the resident range", (sp, np.array([3, M, 11], dtype=np.uint32), good), {}),
        ("different dataset", (sp, vidx, good), dict(subset=other_ss)),
    ]
    for text, args, kw in cases:
        rc, msg, untouched = call(*args, **kw)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
        rc, msg, untouched = call(sp, vidx, good)  # the next call is served
        assert rc == L.PGH_OK and not untouched, (text, rc, msg)
    with pytest.raises(ValueError, match="sparse-resident"):
        world.dense.score_sparse(vidx, good)
    with pytest.raises(ValueError, match="non-finite weight"):
        sp.score_sparse(vidx, nan_w)
    # the dense entry points keep refusing a sparse-resident dataset
    with pytest.raises(ValueError, match="dense-resident"):
        sp.score(vidx, good)
    # an empty list: pgh_score's zeros
    score, dos, ac = sp.score_sparse(np.zeros(0, dtype=np.uint32), np.zeros((0, 2)))
    assert score.shape == (N, 2) and not score.any() and not dos.any() and not ac.any()
    group.close()
