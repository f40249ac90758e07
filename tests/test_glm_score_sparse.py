"""pgh_glm_score_sparse / Dataset.glm_score_sparse: the logistic score test over a sparse-resident dataset, from each
variant's entries.  Against the FP64 oracle (tests/glm_score_oracle.py: Householder QR, no base codes) within 1e-9 on
check_rows' scale; obs_ct, a1_freq and the count decisions equal pgh_glm's logistic fit on the dense dataset of the
same file; datasets opened with other base codes agree within 2e-9 (two results, each within 1e-9 of the oracle).  A
row does not depend on the range, the window the dataset was opened with or the chunk: bit for bit."""

import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import glm_score_oracle as O
import pgen_writer as W

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_score_sparse"]
REL = 1e-9


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_score_sparse(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_score_sparse")


@pytest.mark.parametrize("shape", [(4,), (6,), (1, 5)])
def test_glm_score_sparse_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotype"):
        lib.Dataset.glm_score_sparse(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_sparse(fake, np.zeros(5), np.zeros((2, 4)))


def _values(geno):
    """Codes (3 = missing) as the oracle's values (-9 = missing)."""
    return np.where(geno == 3, -9.0, geno.astype(np.float64))


def _covariates(rng, k, n):
    return rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]


@pytest.mark.parametrize("k", [0, 1, 3])
def test_oracle_score_is_the_first_newton_step_of_the_full_model(k):
    """For a row without a missing call, U / V is the genotype component of the first Newton step of the full
    logistic model [1, x, z] started at (beta_null, 0)."""
    rng = np.random.default_rng(900 + k)
    n = 400
    Z = _covariates(rng, k, n)
    y = O.pheno(rng, n, Z)
    nul = O.Null(y, Z)
    assert nul.status is None and 2 <= nul.steps <= 25
    s = nul.in_s
    for maf in (0.01, 0.1, 0.4):
        x = rng.binomial(2, maf, n).astype(np.float64)
        row = O.oracle_row(x, nul)
        assert row["errcode"] is None and row["obs_ct"] == int(s.sum())
        X = np.column_stack([nul.zt[s, 0], x[s], nul.zt[s, 1:]])
        h = (X * nul.w[s][:, None]).T @ X
        step = np.linalg.solve(h, X.T @ nul.r[s])
        assert abs(step[1] - row["beta"]) <= REL * (abs(row["beta"]) + row["se"])
        assert abs(np.linalg.inv(h)[1, 1] - row["se"] ** 2) <= REL * row["se"] ** 2


# ---- on the GPU --------------------------------------------------------------------------------------------------

def _same(a, b, ctx=None):
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    for key in ("obs_ct", "errcode", "firth"):
        assert np.asarray(a[key]).tolist() == np.asarray(b[key]).tolist(), (key, ctx)


def _close(a, b, rel, ctx=None):
    """Two results for the same rows: errcode, obs_ct, firth and a1_freq equal, the estimates within rel on
    check_rows' scale."""
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


def _counts_equal_the_dense_logistic_fit(got, want, ctx=None):
    """obs_ct and a1_freq for all rows; errcode wherever either side decided from the counts."""
    assert got["obs_ct"].tolist() == want["obs_ct"].tolist(), ctx
    assert np.array_equal(got["a1_freq"], want["a1_freq"], equal_nan=True), ctx
    for code in ("TOO_FEW_SAMPLES", "CONST_ALLELE"):
        assert (got["errcode"] == code).tolist() == (want["errcode"] == code).tolist(), (code, ctx)
    assert not got["firth"].any(), ctx


def _rows(out, idx):
    return {key: v[idx] for key, v in out.items()}


HET_ROWS = (7, 8)  # rare_matrix draws no het-majority rows: these two are made so


def _matrix(m, n, seed):
    rng = np.random.default_rng(seed)
    geno = W.rare_matrix(m, n, rng)
    for v, rate in zip(HET_ROWS, (0.01, 0.3)):
        hit = rng.random(n) < rate
        geno[v] = 1
        geno[v, hit] = rng.integers(0, 4, hit.sum(), dtype=np.uint8)
    return geno, W.choose_kinds(geno, rng)


def _minor(geno):
    return geno.shape[1] - np.array([np.bincount(r, minlength=4).max() for r in geno])


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
    tmp = tmp_path_factory.mktemp("glm_score_sparse")
    return {n: _File(gpu_lib, tmp, M_R, n, n) for n in (257, 4099)}


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("n", [257, 4099])
def test_parity_with_the_oracle_for_every_base_code(gpu_lib, rare_files, n, k):
    f = rare_files[n]
    rng = np.random.default_rng(100 * n + k)
    Z = _covariates(rng, k, n)
    y = O.pheno(rng, n, Z)
    zc = Z if k else None
    nul = O.Null(y, Z)
    assert nul.status is None
    want = f.dense.glm(y, zc, model="logistic", firth=False)
    idx = sorted(set(range(0, M_R, 23)) | set(HET_ROWS))
    minor = _minor(f.geno)
    results = {}
    for max_minor in (0, 1, n):
        sp = f.sparse(max_minor=max_minor)
        info = sp.sparse_info()
        got = results[max_minor] = sp.glm_score_sparse(y, zc)
        fitted, worst = O.check_rows(_rows(got, idx), f.x[idx], nul, rel=REL)
        print(f"n={n} k={k} max_minor={max_minor}: {fitted} fitted of {len(idx)}, worst {worst:.3g}")
        assert fitted > len(idx) // 3
        _counts_equal_the_dense_logistic_fit(got, want, ctx=(n, k, max_minor))
        if max_minor == n:
            # het-, hom-alt- and missing-majority rows all run from their entries
            assert info.dense_variant_ct == 0 and all(info.base_hist[b] > 0 for b in (1, 2, 3))
            if n == 4099:  # both sides of the wave / workgroup threshold
                assert (minor > 1024).any() and ((minor > 0) & (minor <= 1024)).any()
        if max_minor == 1:
            assert info.dense_variant_ct > 0 and info.sparse_variant_ct > 0
            assert int((minor > 1).sum()) == info.dense_variant_ct
        sp.close()
    for a, b in ((0, 1), (0, n), (1, n)):
        _close(results[a], results[b], 2 * REL, ctx=(n, k, a, b))


@pytest.mark.gpu
def test_long_rows_and_long_missing_lists(gpu_lib, tmp_path):
    n, m, k = 70_000, 120, 20
    f = _File(gpu_lib, tmp_path, m, n, 70)
    entries = _minor(f.geno)
    in_missing_list = np.array([(r == 3).sum() if np.bincount(r, minlength=4).argmax() != 3 else 0 for r in f.geno])
    assert entries.max() > 10_000 and in_missing_list.max() > 1_000
    rng = np.random.default_rng(71)
    Z = _covariates(rng, k, n)
    y = O.pheno(rng, n, Z)
    nul = O.Null(y, Z)
    assert nul.status is None
    sp = f.sparse(max_minor=n)
    assert sp.sparse_info().dense_variant_ct == 0
    got = sp.glm_score_sparse(y, Z)
    _counts_equal_the_dense_logistic_fit(got, f.dense.glm(y, Z, model="logistic", firth=False))
    # the longest entry lists, the longest missing lists, the het-majority rows and a spread: 16 rows
    idx = list(dict.fromkeys(np.argsort(entries)[-5:].tolist() + np.argsort(in_missing_list)[-3:].tolist()
                             + list(HET_ROWS) + list(range(3, m, 9))))[:16]
    assert len(idx) == 16
    fitted, worst = O.check_rows(_rows(got, idx), f.x[idx], nul, rel=REL)
    print(f"long rows: {fitted} fitted of 16, worst {worst:.3g}")
    assert fitted >= 8
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
    for k in (kp, kp - 1):
        rng = np.random.default_rng(3000 + k)
        Z = _covariates(rng, k, f.n)
        y = O.pheno(rng, f.n, Z)
        nul = O.Null(y, Z)
        assert nul.status is None
        got = sp.glm_score_sparse(y, Z if k else None, v_begin=0, v_end=max(idx) + 1)
        fitted, worst = O.check_rows(got, f.x, nul, rel=REL, idx=idx)
        print(f"k={k}: {fitted} fitted of 12, worst {worst:.3g}")
        assert fitted >= 4
    sp.close()


@pytest.mark.gpu
def test_sample_subset(gpu_lib, rare_files):
    f = rare_files[4099]
    rng = np.random.default_rng(12)
    keep = rng.random(f.n) < 0.5
    n = int(keep.sum())
    k = 3
    Z = _covariates(rng, k, n)
    y = O.pheno(rng, n, Z)
    nul = O.Null(y, Z)
    assert nul.status is None
    ss_d = f.dense.subset(keep)
    want = f.dense.glm(y, Z, model="logistic", firth=False, subset=ss_d)
    idx = sorted(set(range(0, M_R, 29)) | set(HET_ROWS))
    for max_minor in (0, f.n):
        sp = f.sparse(max_minor=max_minor)
        ss = sp.subset(keep)
        got = sp.glm_score_sparse(y, Z, subset=ss)
        _counts_equal_the_dense_logistic_fit(got, want, ctx=max_minor)
        fitted, worst = O.check_rows(_rows(got, idx), f.x[idx][:, keep], nul, rel=REL)
        print(f"subset max_minor={max_minor}: {fitted} fitted of {len(idx)}, worst {worst:.3g}")
        with pytest.raises(ValueError, match="different dataset"):
            sp.glm_score_sparse(y, Z, subset=ss_d)
        ss.close()
        sp.close()
    ss_d.close()


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_range_or_the_window(gpu_lib, rare_files):
    f = rare_files[4099]
    rng = np.random.default_rng(44)
    k = 3
    Z = _covariates(rng, k, f.n)
    y = O.pheno(rng, f.n, Z)
    v0 = next(v for v in range(150, M_R) if f.kinds[v] in (2, 3))  # a window that starts after an LD base
    v1 = min(M_R, v0 + 150)
    for max_minor in (0, f.n):
        sp = f.sparse(max_minor=max_minor)
        whole = sp.glm_score_sparse(y, Z)
        assert (whole["errcode"] == None).sum() > M_R // 3  # noqa: E711
        _same(sp.glm_score_sparse(y, Z), whole, ctx="again")
        _same(sp.glm_score_sparse(y, Z, v_begin=40, v_end=333), _rows(whole, slice(40, 333)), ctx=max_minor)
        assert sp.glm_score_sparse(y, Z, v_begin=77, v_end=77)["beta"].shape == (0,)
        part = f.sparse(max_minor=max_minor, variant_begin=v0, variant_end=v1)
        _same(part.glm_score_sparse(y, Z), _rows(whole, slice(v0, v1)), ctx=(max_minor, v0))
        part.close()
        sp.close()


CHUNK = 16384  # variants per chunk of the GLM family


@pytest.mark.gpu
def test_rows_across_a_chunk_boundary(gpu_lib, tmp_path):
    L = gpu_lib
    m, n = CHUNK + 300, 96
    prefix = str(tmp_path / "chunks")
    L.synth_write_files(prefix, m, n, 5151, 0.02)
    rng = np.random.default_rng(61)
    Z = rng.normal(size=(2, n))
    y = O.pheno(rng, n, Z, case_rate=0.3)
    dense = L.Dataset.open(prefix + ".pgen")
    want = dense.glm(y, Z, model="logistic", firth=False)
    dense.close()
    for max_minor in (30, n):  # dense-form and sparse rows mixed, and every row sparse
        sp = L.Dataset.open(prefix + ".pgen", sparse=True, max_minor=max_minor)
        info = sp.sparse_info()
        assert info.sparse_variant_ct > 0 and (info.dense_variant_ct > 0) == (max_minor == 30)
        whole = sp.glm_score_sparse(y, Z, v_begin=5)
        _counts_equal_the_dense_logistic_fit(whole, _rows(want, slice(5, m)), ctx=max_minor)
        assert (whole["errcode"] == None).sum() > m // 3  # noqa: E711
        for lo, hi in ((5 + CHUNK - 40, 5 + CHUNK + 60), (m - 30, m)):
            _same(sp.glm_score_sparse(y, Z, v_begin=lo, v_end=hi), _rows(whole, slice(lo - 5, hi - 5)),
                  ctx=(max_minor, lo))
        sp.close()


def _decision_file(tmp_path):
    """An 8-variant file like test_glm_sparse's test_decisions_equal_the_dense_form's, with a 0/1 phenotype."""
    n = 64
    rng = np.random.default_rng(5)
    y = (rng.random(n) < 0.35).astype(np.float64)
    no_pheno = np.array([3, 17, 40])
    y[no_pheno] = NAN
    y[[1, 2, 5, 9]] = [0.0, 0.0, 1.0, 1.0]       # cases and controls among the few used samples of rows 3 and 4
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
    return path, geno, y


@pytest.mark.gpu
def test_decisions(gpu_lib, tmp_path):
    L = gpu_lib
    path, geno, y = _decision_file(tmp_path)
    n = geno.shape[1]
    Z = geno[5].astype(np.float64)[None, :]
    nul = O.Null(y, Z)
    assert nul.status is None
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True, max_minor=n)
    assert sp.sparse_info().dense_variant_ct == 0
    got = sp.glm_score_sparse(y, Z)
    exp = [O.oracle_row(x, nul) for x in _values(geno)]
    assert [e["errcode"] for e in exp] == ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", "TOO_FEW_SAMPLES", None,
                                           "SINGULAR_MATRIX", None, "CONST_ALLELE"]
    assert list(got["errcode"]) == [e["errcode"] for e in exp]
    assert got["obs_ct"].tolist() == [e["obs_ct"] for e in exp]
    assert got["obs_ct"].tolist() == [61, 61, 61, 3, 4, 61, int(((geno[6] != 3) & ~np.isnan(y)).sum()),
                                      int(((geno[7] != 3) & ~np.isnan(y)).sum())]
    O.check_rows(got, _values(geno), nul, rel=REL)
    _counts_equal_the_dense_logistic_fit(got, dense.glm(y, Z, model="logistic", firth=False))
    sp.close()
    dense.close()


@pytest.mark.gpu
def test_null_model_outcomes(gpu_lib, rare_files):
    """A null model that cannot be fitted: the rows decided by their counts stay, every other row gets its status."""
    f = rare_files[257]
    rng = np.random.default_rng(77)
    z, z2 = rng.normal(size=(2, f.n))
    y = O.pheno(rng, f.n, z[None, :])
    sp = f.sparse(max_minor=f.n)
    # (the covariates that fail, covariates of the same count that do not, the status)
    for bad, good, code in ((np.stack([z, z]), np.stack([z, z2]), "SINGULAR_MATRIX"),  # a duplicated covariate
                            (np.nan_to_num(y, nan=0.0)[None, :], z[None, :], "NO_CONVERGENCE")):  # one equal to y
        assert O.Null(y, bad).status == code and O.Null(y, good).status is None
        base = sp.glm_score_sparse(y, good)
        assert (base["errcode"] == None).sum() > M_R // 3  # noqa: E711
        decided = np.isin(base["errcode"], ["TOO_FEW_SAMPLES", "CONST_ALLELE"])
        assert (base["errcode"] == "CONST_ALLELE").any() and not decided.all()
        got = sp.glm_score_sparse(y, bad)
        assert got["errcode"][decided].tolist() == base["errcode"][decided].tolist()
        assert set(got["errcode"][~decided]) == {code}
        assert got["obs_ct"].tolist() == base["obs_ct"].tolist()
        assert np.array_equal(got["a1_freq"], base["a1_freq"], equal_nan=True)
        for key in ("beta", "se", "stat", "p"):
            assert np.isnan(got[key]).all(), key
    sp.close()


@pytest.mark.gpu
def test_refusals(gpu_lib):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    n = sp.n_samples
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    rows = sp.glm_score_sparse(y, v_begin=0, v_end=8)
    assert rows["errcode"].shape == (8,)
    y2 = y.copy()
    y2[4] = 2.0
    with pytest.raises(ValueError, match="phenotype must be 0 or 1"):
        sp.glm_score_sparse(y2)
    for const in (0.0, 1.0):
        yc = np.full(n, const)
        yc[::5] = NAN
        with pytest.raises(ValueError, match="no cases or no controls"):
            sp.glm_score_sparse(yc)
    with pytest.raises(ValueError, match="sparse-resident"):
        dense.glm_score_sparse(y, v_begin=0, v_end=8)
    with pytest.raises(ValueError, match="at most 20 covariates"):
        sp.glm_score_sparse(y, np.zeros((21, n)))
    bad = np.zeros((2, n))
    bad[1, 5] = np.inf
    with pytest.raises(ValueError, match="covariate 1 is not finite at sample 5"):
        sp.glm_score_sparse(y, bad)
    with pytest.raises(ValueError, match="outside the resident range"):
        sp.glm_score_sparse(y, v_begin=0, v_end=sp.v_end + 1)
    with pytest.raises(ValueError, match="outside the resident range"):
        sp.glm_score_sparse(y, v_begin=9, v_end=8)
    with pytest.raises(ValueError, match="dense-resident"):
        sp.glm(y, model="logistic", v_begin=0, v_end=8)
    assert sp.glm_score_sparse(y, v_begin=3, v_end=3)["errcode"].shape == (0,)
    sp.close()
    dense.close()
