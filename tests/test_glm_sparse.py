"""pgh_glm_sparse / Dataset.glm_sparse: pgh_glm's linear fit over a sparse-resident dataset, from each variant's
entries.  Against the dense dataset of the same file: errcode, obs_ct and a1_freq equal, the estimates within 1e-9
(and within 1e-9 of the FP64 oracle, tests/glm_oracle.py); the rows of variants held in the dense form bit for bit.
A row does not depend on the range, the window the dataset was opened with or the chunk: bit for bit."""

import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import pgen_writer as W

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_sparse"]


def _oracle():
    # glm_oracle needs scipy: only the device tests, which compare against it, skip without it
    return pytest.importorskip("glm_oracle")


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_sparse(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_sparse")


@pytest.mark.parametrize("shape", [(4,), (6,), (1, 5)])
def test_glm_sparse_rejects_a_phenotype_array_of_the_wrong_shape(lib, shape):
    """The shape check runs before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotype"):
        lib.Dataset.glm_sparse(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_sparse(fake, np.zeros(5), np.zeros((2, 4)))


# ---- on the GPU --------------------------------------------------------------------------------------------------

def _same(a, b, ctx=None):
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    for key in ("obs_ct", "errcode", "firth"):
        assert np.asarray(a[key]).tolist() == np.asarray(b[key]).tolist(), (key, ctx)


def _close(a, b, rel=1e-9, ctx=None):
    """The linear contract (tests/test_glm_multi.py): errcode, obs_ct, firth and a1_freq equal; the estimates within
    rel, on check_rows' scale (beta relative to |beta| + SE, the statistic to |t| + 1)."""
    for key in ("obs_ct", "errcode", "firth"):
        assert list(a[key]) == list(b[key]), (key, ctx)
    assert np.array_equal(a["a1_freq"], b["a1_freq"], equal_nan=True), ("a1_freq", ctx)
    se = np.nan_to_num(b["se"], nan=0.0)
    for key in ("beta", "se", "stat", "p"):
        g, e = a[key], b[key]
        assert np.array_equal(np.isnan(g), np.isnan(e)), (key, ctx)
        scale = np.abs(e) + (se if key == "beta" else 1.0 if key == "stat" else 0.0)
        ok = np.isnan(e) | (np.abs(g - e) <= rel * scale + 1e-300)
        bad = np.flatnonzero(~ok)
        assert not len(bad), (key, ctx, bad[:5], g[bad[:5]], e[bad[:5]])


def _rows(out, idx):
    return {key: v[idx] for key, v in out.items()}


def _values(geno):
    """Codes (3 = missing) as the oracle's values (-9 = missing)."""
    return np.where(geno == 3, -9.0, geno.astype(np.float64))


def _covariates(rng, k, n):
    return rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]


HET_ROWS = (7, 8)  # rare_matrix draws no het-majority rows: these two are made so


def _matrix(m, n, seed):
    rng = np.random.default_rng(seed)
    geno = W.rare_matrix(m, n, rng)
    for v, rate in zip(HET_ROWS, (0.01, 0.3)):
        hit = rng.random(n) < rate
        geno[v] = 1
        geno[v, hit] = rng.integers(0, 4, hit.sum(), dtype=np.uint8)
    return geno, W.choose_kinds(geno, rng)


class _File:
    """A .pgen of every record type, its dense dataset and its calls."""

    def __init__(self, L, tmp, m, n, seed):
        self.L, self.m, self.n = L, m, n
        self.geno, self.kinds = _matrix(m, n, seed)
        self.path = str(tmp / f"rare_{n}.pgen")
        W.write_pgen(self.path, self.geno, self.kinds)
        self.dense = L.Dataset.open(self.path)
        self.x = _values(self.geno)

    def sparse(self, **kw):
        # several windows per open, so that parts are concatenated and windows start after LD bases
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(97 * self.dense.info.pitch_bytes))
            return self.L.Dataset.open(self.path, sparse=True, **kw)


M_R = 600


@pytest.fixture(scope="module")
def rare_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_sparse")
    return {n: _File(gpu_lib, tmp, M_R, n, n) for n in (257, 4099)}


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("n", [257, 4099])
def test_parity_with_the_dense_form_for_every_base_code(gpu_lib, rare_files, n, k):
    f = rare_files[n]
    rng = np.random.default_rng(100 * n + k)
    Z = _covariates(rng, k, n)
    y = _oracle()._pheno(rng, n, "linear", Z)
    zc = Z if k else None
    want = f.dense.glm(y, zc, model="linear")
    idx = sorted(set(range(0, M_R, 23)) | set(HET_ROWS))
    _oracle().check_rows(_rows(want, idx), f.x[idx], y, Z, "linear", rel=1e-9)
    for max_minor in (0, 1, n):
        sp = f.sparse(max_minor=max_minor)
        info = sp.sparse_info()
        got = sp.glm_sparse(y, zc)
        _close(got, want, ctx=(n, k, max_minor))
        _oracle().check_rows(_rows(got, idx), f.x[idx], y, Z, "linear", rel=1e-9)
        if max_minor == n:
            # het-, hom-alt- and missing-majority rows all run from their entries
            assert info.dense_variant_ct == 0 and all(info.base_hist[b] > 0 for b in (1, 2, 3))
            if n == 4099:  # both sides of the wave / workgroup threshold
                minor = n - np.array([np.bincount(r, minlength=4).max() for r in f.geno])
                assert (minor > 1024).any() and ((minor > 0) & (minor <= 1024)).any()
        if max_minor == 1:
            assert info.dense_variant_ct > 0 and info.sparse_variant_ct > 0
            minor = n - np.array([np.bincount(r, minlength=4).max() for r in f.geno])
            held_dense = np.flatnonzero(minor > 1)
            assert len(held_dense) == info.dense_variant_ct
            _same(_rows(got, held_dense), _rows(want, held_dense), ctx=(n, k, "dense-form rows"))
        sp.close()


@pytest.mark.gpu
def test_long_rows_take_the_workgroup_path(gpu_lib, tmp_path):
    n, m, k = 70_000, 120, 20
    f = _File(gpu_lib, tmp_path, m, n, 70)
    entries = n - np.array([np.bincount(r, minlength=4).max() for r in f.geno])
    in_missing_list = np.array([(r == 3).sum() if np.bincount(r, minlength=4).argmax() != 3 else 0 for r in f.geno])
    assert entries.max() > 10_000 and in_missing_list.max() > 1_000
    rng = np.random.default_rng(71)
    Z = _covariates(rng, k, n)
    y = _oracle()._pheno(rng, n, "linear", Z)
    want = f.dense.glm(y, Z, model="linear")
    sp = f.sparse(max_minor=n)
    assert sp.sparse_info().dense_variant_ct == 0
    got = sp.glm_sparse(y, Z)
    _close(got, want)
    # the longest entry lists, the longest missing lists, the het-majority rows and a spread: 16 rows
    idx = list(dict.fromkeys(np.argsort(entries)[-5:].tolist() + np.argsort(in_missing_list)[-3:].tolist()
                             + list(HET_ROWS) + list(range(3, m, 9))))[:16]
    assert len(idx) == 16
    _oracle().check_rows(_rows(got, idx), f.x[idx], y, Z, "linear", rel=1e-9)
    sp.close()
    f.dense.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kp", [1, 2, 4, 8, 12, 16, 20])
def test_every_instantiated_width(gpu_lib, rare_files, kp):
    """k = kp and kp - 1 for every width GlmPadCovar returns (kp = 1 covers the width 0)."""
    f = rare_files[4099]
    idx = sorted(set(range(5, M_R, 55)) | set(HET_ROWS))[:12]
    assert len(idx) == 12
    sp = f.sparse(max_minor=f.n)
    assert sp.sparse_info().dense_variant_ct == 0
    for k in (kp, kp - 1):
        rng = np.random.default_rng(3000 + k)
        Z = _covariates(rng, k, f.n)
        y = _oracle()._pheno(rng, f.n, "linear", Z)
        zc = Z if k else None
        got = sp.glm_sparse(y, zc)
        _close(got, f.dense.glm(y, zc, model="linear"), ctx=k)
        _oracle().check_rows(_rows(got, idx), f.x[idx], y, Z, "linear", rel=1e-9)
    sp.close()


@pytest.mark.gpu
def test_sample_subset(gpu_lib, rare_files):
    f = rare_files[4099]
    rng = np.random.default_rng(12)
    keep = rng.random(f.n) < 0.5
    n = int(keep.sum())
    k = 3
    Z = _covariates(rng, k, n)
    y = _oracle()._pheno(rng, n, "linear", Z)
    ss_d = f.dense.subset(keep)
    want = f.dense.glm(y, Z, model="linear", subset=ss_d)
    idx = sorted(set(range(0, M_R, 29)) | set(HET_ROWS))
    for max_minor in (0, f.n):
        sp = f.sparse(max_minor=max_minor)
        ss = sp.subset(keep)
        got = sp.glm_sparse(y, Z, subset=ss)
        _close(got, want, ctx=max_minor)
        _oracle().check_rows(_rows(got, idx), f.x[idx][:, keep], y, Z, "linear", rel=1e-9)
        with pytest.raises(ValueError, match="different dataset"):
            sp.glm_sparse(y, Z, subset=ss_d)
        ss.close()
        sp.close()
    ss_d.close()


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_range_or_the_window(gpu_lib, rare_files):
    f = rare_files[4099]
    rng = np.random.default_rng(44)
    k = 3
    Z = _covariates(rng, k, f.n)
    y = _oracle()._pheno(rng, f.n, "linear", Z)
    v0 = next(v for v in range(150, M_R) if f.kinds[v] in (2, 3))  # a window that starts after an LD base
    v1 = min(M_R, v0 + 150)
    for max_minor in (0, f.n):
        sp = f.sparse(max_minor=max_minor)
        whole = sp.glm_sparse(y, Z)
        assert whole["beta"].tobytes() == sp.glm_sparse(y, Z)["beta"].tobytes()
        _same(sp.glm_sparse(y, Z), whole, ctx="again")
        _same(sp.glm_sparse(y, Z, v_begin=40, v_end=333), _rows(whole, slice(40, 333)), ctx=max_minor)
        assert sp.glm_sparse(y, Z, v_begin=77, v_end=77)["beta"].shape == (0,)
        part = f.sparse(max_minor=max_minor, variant_begin=v0, variant_end=v1)
        _same(part.glm_sparse(y, Z), _rows(whole, slice(v0, v1)), ctx=(max_minor, v0))
        part.close()
        sp.close()


CHUNK = 16384  # variants per chunk of pgh_glm and pgh_glm_sparse


@pytest.mark.gpu
def test_rows_across_a_chunk_boundary(gpu_lib, tmp_path):
    L = gpu_lib
    m, n = CHUNK + 300, 96
    prefix = str(tmp_path / "chunks")
    L.synth_write_files(prefix, m, n, 5151, 0.02)
    dense = L.Dataset.open(prefix + ".pgen")
    rng = np.random.default_rng(61)
    Z = rng.normal(size=(2, n))
    y = _oracle()._pheno(rng, n, "linear", Z)
    want = dense.glm(y, Z, model="linear")
    for max_minor in (30, n):  # dense-form and sparse rows mixed, and every row sparse
        sp = L.Dataset.open(prefix + ".pgen", sparse=True, max_minor=max_minor)
        info = sp.sparse_info()
        assert info.sparse_variant_ct > 0 and (info.dense_variant_ct > 0) == (max_minor == 30)
        whole = sp.glm_sparse(y, Z, v_begin=5)
        _close(whole, _rows(want, slice(5, m)), ctx=max_minor)
        for lo, hi in ((5 + CHUNK - 40, 5 + CHUNK + 60), (m - 30, m)):
            _same(sp.glm_sparse(y, Z, v_begin=lo, v_end=hi), _rows(whole, slice(lo - 5, hi - 5)), ctx=(max_minor, lo))
        sp.close()
    dense.close()


@pytest.mark.gpu
def test_decisions_equal_the_dense_form(gpu_lib, tmp_path):
    L = gpu_lib
    n, k = 64, 1
    rng = np.random.default_rng(5)
    y = rng.normal(size=n)
    no_pheno = np.array([3, 17, 40])
    y[no_pheno] = NAN
    geno = np.zeros((8, n), dtype=np.uint8)
    geno[0, no_pheno] = 1                        # every sample with a phenotype is hom-ref
    geno[1, 17] = 2                              # a singleton whose carrier has no phenotype
    geno[2] = 2
    geno[2, no_pheno[:2]] = [0, 1]               # the same under a hom-alt base
    geno[3] = 3
    geno[3, [1, 2, 5]] = [0, 1, 2]               # k + 2 = 3 used samples
    geno[4] = 3
    geno[4, [1, 2, 5, 9]] = [0, 1, 2, 1]         # k + 3: enough to fit
    geno[5] = rng.binomial(2, 0.2, n)            # the covariate
    geno[6] = rng.binomial(2, 0.3, n)
    geno[6, rng.random(n) < 0.1] = 3
    geno[7] = 1
    geno[7, rng.random(n) < 0.2] = 3             # het base: constant among the called
    path = str(tmp_path / "decisions.pgen")
    W.write_pgen(path, geno, [0] * len(geno))
    Z = geno[5].astype(np.float64)[None, :]
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True, max_minor=n)
    assert sp.sparse_info().dense_variant_ct == 0
    want = dense.glm(y, Z, model="linear")
    got = sp.glm_sparse(y, Z)
    assert list(got["errcode"]) == ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", "TOO_FEW_SAMPLES", None,
                                    "SINGULAR_MATRIX", None, "CONST_ALLELE"]
    assert got["obs_ct"].tolist() == [61, 61, 61, 3, 4, 61, int(((geno[6] != 3) & ~np.isnan(y)).sum()),
                                      int(((geno[7] != 3) & ~np.isnan(y)).sum())]
    _close(got, want)
    _oracle().check_rows(got, _values(geno), y, Z, "linear", rel=1e-9)
    # and without covariates, where the reference tests its one-pass variance
    want0, got0 = dense.glm(y, model="linear"), sp.glm_sparse(y)
    assert list(got0["errcode"][:4]) == ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", None]
    _close(got0, want0)
    sp.close()
    dense.close()


@pytest.mark.gpu
def test_refusals(gpu_lib):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    n = sp.n_samples
    y = np.arange(n, dtype=np.float64) % 3
    with pytest.raises(ValueError, match="sparse-resident"):
        dense.glm_sparse(y, v_begin=0, v_end=8)
    with pytest.raises(ValueError, match="at most 20 covariates"):
        sp.glm_sparse(y, np.zeros((21, n)))
    bad = np.zeros((2, n))
    bad[1, 5] = np.inf
    with pytest.raises(ValueError, match="covariate 1 is not finite at sample 5"):
        sp.glm_sparse(y, bad)
    with pytest.raises(ValueError, match="outside the resident range"):
        sp.glm_sparse(y, v_begin=0, v_end=sp.v_end + 1)
    with pytest.raises(ValueError, match="outside the resident range"):
        sp.glm_sparse(y, v_begin=9, v_end=8)
    with pytest.raises(ValueError, match="phenotype"):
        sp.glm_sparse(y[:-1])
    with pytest.raises(ValueError, match="dense-resident"):
        sp.glm(y, model="linear", v_begin=0, v_end=8)
    # pgh_glm's own messages for the same arguments
    with pytest.raises(ValueError, match="at most 20 covariates"):
        dense.glm(y, np.zeros((21, n)))
    with pytest.raises(ValueError, match="covariate 1 is not finite at sample 5"):
        dense.glm(y, bad)
    assert sp.glm_sparse(y, v_begin=3, v_end=3)["errcode"].shape == (0,)
    sp.close()
    dense.close()
