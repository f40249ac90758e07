"""pgh_glm_multi / Dataset.glm_multi: many phenotypes in one walk of the matrix.  Every (variant, phenotype) row is
what pgh_glm returns for that phenotype alone: logistic and Firth rows bit for bit, linear rows with a1_freq and
obs_ct bit for bit and the estimates within 1e-9 (and within 1e-9 of the FP64 oracle, tests/glm_oracle.py).  A row
does not depend on the other phenotypes of the call, its place among them, the window start, the chunk or the
shard: those comparisons are bit for bit."""

import math
import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

NAN = float("nan")


def _oracle():
    # glm_oracle needs scipy: only the device tests, which compare against it, skip without it
    return pytest.importorskip("glm_oracle")


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_multi(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    assert "pgh_glm_multi(" in header
    assert "pgh_glm_multi" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.raw(), "pgh_glm_multi")


@pytest.mark.parametrize("shape", [(5,), (2, 4), (2, 6), (0, 5), (1, 2, 5)])
def test_glm_multi_rejects_a_phenotype_array_of_the_wrong_shape(lib, shape):
    """The shape check runs before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_multi(fake, np.zeros(shape))


# ---- on the GPU --------------------------------------------------------------------------------------------------

M_W, N_W = 400, 3001
SEP = 5


@pytest.fixture(scope="module")
def widths_fixture(gpu_lib):
    """test_glm_widths_chunks' matrix: 400 x 3,001, 2 % missing calls, the edge variants in rows 0-4 (constant, all
    missing, constant among the called, too few samples, 60 % missing) and a variant to separate in row 5."""
    rows_2bit = _oracle().rows_2bit
    rng = np.random.default_rng(20261017)
    geno = rng.binomial(2, rng.uniform(0.05, 0.5, M_W)[:, None], size=(M_W, N_W)).astype(np.int8)
    geno[rng.random((M_W, N_W)) < 0.02] = -9
    geno[0, :] = 1
    geno[1, :] = -9
    geno[2, :] = np.where(rng.random(N_W) < 0.5, 0, -9)
    geno[3, :] = -9
    geno[3, :2] = [0, 2]
    geno[4, rng.random(N_W) < 0.6] = -9
    geno[SEP, :] = rng.binomial(2, 0.1, N_W)
    ds = gpu_lib.Dataset.from_host_rows(rows_2bit(geno), N_W)
    return ds, geno.astype(np.float64)


def _col(out, p):
    return {key: out[key][:, p] for key in out}


def _same(a, b, ctx=None):
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    for key in ("obs_ct", "errcode", "firth"):
        assert np.asarray(a[key]).tolist() == np.asarray(b[key]).tolist(), (key, ctx)


def _close(a, b, rel=1e-9, ctx=None):
    """The linear contract: errcode, obs_ct, firth and a1_freq equal; the estimates within rel, on check_rows'
    scale (beta relative to |beta| + SE, the statistic to |t| + 1)."""
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


def _phenotypes(rng, n, P, k, Z, kind="linear", mode="mix"):
    """P phenotypes.  mode 'shared': one missing-value pattern; 'distinct': each its own (_pheno's 3 %); 'mix': the
    first third on pattern A, the next third on pattern B, the rest their own, and with P >= 7 phenotype 1 constant
    on pattern A and phenotype P - 1 with k + 2 values (TOO_FEW_SAMPLES at every variant)."""
    pheno = _oracle()._pheno
    pats = [rng.random(n) < 0.03 for _ in range(2)]

    def draw(size):
        return rng.normal(size=size) if kind == "linear" else (rng.random(size) < 0.5).astype(np.float64)

    Y = np.empty((P, n))
    for p in range(P):
        y = pheno(rng, n, kind, Z)
        if mode == "shared" or (mode == "mix" and p < 2 * P // 3):
            gap = np.isnan(y)
            y[gap] = draw(int(gap.sum()))
            y[pats[0] if mode == "shared" or p < P // 3 else pats[1]] = NAN
        Y[p] = y
    if mode == "mix" and P >= 7:
        Y[1] = np.where(pats[0], NAN, 3.0 if kind == "linear" else 1.0)
        Y[P - 1] = NAN
        Y[P - 1, rng.choice(n, k + 2, replace=False)] = draw(k + 2)
    return Y


def _singles(ds, Y, Z, model, **kw):
    return [ds.glm(Y[p], Z, model=model, **kw) for p in range(Y.shape[0])]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 3, 12, 20])
@pytest.mark.parametrize("P", [1, 7, 33, 100])
def test_linear_matches_single_calls_and_oracle(gpu_lib, widths_fixture, k, P):
    ds, x = widths_fixture
    rng = np.random.default_rng(1000 * k + P)
    Z = rng.normal(size=(k, N_W)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]
    Y = _phenotypes(rng, N_W, P, k, Z)
    zc = Z if k else None
    out = ds.glm_multi(Y, zc, model="linear")
    assert out["beta"].shape == (M_W, P)
    for p, single in enumerate(_singles(ds, Y, zc, "linear")):
        _close(_col(out, p), single, ctx=(k, P, p))
    assert list(out["errcode"][:4, 0]) == ["CONST_ALLELE", "TOO_FEW_SAMPLES", "CONST_ALLELE", "TOO_FEW_SAMPLES"]
    if P >= 7:
        assert set(out["errcode"][:, P - 1]) == {"TOO_FEW_SAMPLES"}
        assert "ZERO_VARIANCE" in set(out["errcode"][6:, 1])
    idx = list(range(8)) + list(range(8, M_W, 37))
    for p in sorted({0, P // 2, P - 2} & set(range(P))):
        got = {key: v[idx] for key, v in _col(out, p).items()}
        _oracle().check_rows(got, x[idx], Y[p], Z, "linear", rel=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["shared", "distinct"])
def test_linear_one_pattern_and_every_pattern_distinct(gpu_lib, widths_fixture, mode):
    ds, x = widths_fixture
    rng = np.random.default_rng(7 if mode == "shared" else 8)
    k, P = 3, 33
    Z = rng.normal(size=(k, N_W))
    Y = _phenotypes(rng, N_W, P, k, Z, mode=mode)
    assert len({np.isnan(Y[p]).tobytes() for p in range(P)}) == (1 if mode == "shared" else P)
    out = ds.glm_multi(Y, Z)
    for p, single in enumerate(_singles(ds, Y, Z, "linear")):
        _close(_col(out, p), single, ctx=(mode, p))


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 5, 17])
def test_logistic_and_firth_are_bit_identical_to_single_calls(gpu_lib, widths_fixture, P):
    ds, x = widths_fixture
    rng = np.random.default_rng(50 + P)
    k = 2
    Z = rng.normal(size=(k, N_W))
    Y = _phenotypes(rng, N_W, P, k, Z, kind="logistic")
    # the last phenotype: every carrier of variant SEP is a case, so that variant's Newton fit fails and Firth's runs
    sep = np.where(x[SEP] > 0, 1.0, (rng.random(N_W) < 0.3).astype(np.float64))
    sep[x[SEP] < 0] = 0.0
    Y[-1] = sep
    for firth in (True, False):
        out = ds.glm_multi(Y, Z, model="logistic", firth=firth)
        for p, single in enumerate(_singles(ds, Y, Z, "logistic", firth=firth)):
            _same(_col(out, p), single, ctx=(P, p, firth))
        if firth:
            assert out["firth"][SEP, P - 1]
        else:
            assert out["errcode"][SEP, P - 1] in ("SEPARATION", "NO_CONVERGENCE")


@pytest.mark.gpu
def test_row_does_not_depend_on_the_other_phenotypes(gpu_lib, widths_fixture):
    """One phenotype alone, at position 23 of a call of 40 (sharing its pattern with twelve of the others), and at
    position 16 of the same call reversed."""
    ds, x = widths_fixture
    rng = np.random.default_rng(404)
    k = 12
    Z = rng.normal(size=(k, N_W))
    Y = _phenotypes(rng, N_W, 40, k, Z)
    y = Y[5].copy()  # on pattern A
    Y[5] = _phenotypes(rng, N_W, 1, k, Z, mode="distinct")[0]
    Y[23] = y
    among = ds.glm_multi(Y, Z)
    _same(_col(ds.glm_multi(y[None, :], Z), 0), _col(among, 23))
    _same(_col(ds.glm_multi(Y[::-1], Z), 16), _col(among, 23))


# more than one variant chunk of pgh_glm_multi (65,536 variants at this shape)
CHUNK = 65536
M_C, N_C, SEED_C = 2 * CHUNK + 77, 96, 5151


@pytest.mark.gpu
def test_windows_chunks_and_shards_bit_for_bit(gpu_lib):
    ds = gpu_lib.Dataset.synth(0, M_C, N_C, SEED_C, 0.02)
    rng = np.random.default_rng(61)
    Z = rng.normal(size=(2, N_C))
    Y = _phenotypes(rng, N_C, 7, 2, Z)
    v0 = 5
    whole = ds.glm_multi(Y, Z, v_begin=v0)
    assert whole["beta"].shape == (M_C - v0, 7)
    for lo, hi in ((16000, 16800), (v0 + CHUNK - 300, v0 + CHUNK + 500), (M_C - 40, M_C)):
        win = ds.glm_multi(Y, Z, v_begin=lo, v_end=hi)
        _same(win, {key: v[lo - v0:hi - v0] for key, v in whole.items()}, ctx=(lo, hi))
    grp = gpu_lib.Dataset.group([gpu_lib.Dataset.synth(0, 20000, N_C, SEED_C, 0.02),
                                 gpu_lib.Dataset.synth(20000, M_C, N_C, SEED_C, 0.02)])
    _same(grp.glm_multi(Y, Z, v_begin=v0), whole)
    # and pgh_glm's rows around the chunk boundary
    lo, hi = v0 + CHUNK - 20, v0 + CHUNK + 20
    for p in range(7):
        _close({key: v[lo - v0:hi - v0, p] for key, v in whole.items()},
               ds.glm(Y[p], Z, v_begin=lo, v_end=hi), ctx=p)


@pytest.mark.gpu
def test_sample_subset(gpu_lib, widths_fixture):
    ds, x = widths_fixture
    rng = np.random.default_rng(12)
    keep = rng.random(N_W) < 0.7
    ss = ds.subset(keep)
    n = int(keep.sum())
    Z = rng.normal(size=(12, n))
    Y = _phenotypes(rng, n, 7, 12, Z)
    out = ds.glm_multi(Y, Z, subset=ss)
    for p, single in enumerate(_singles(ds, Y, Z, "linear", subset=ss)):
        _close(_col(out, p), single, ctx=p)
    idx = list(range(8)) + list(range(8, M_W, 41))
    got = {key: v[idx] for key, v in _col(out, 0).items()}
    _oracle().check_rows(got, x[idx][:, keep], Y[0], Z, "linear", rel=1e-9)
    Yb = _phenotypes(rng, n, 7, 12, Z, kind="logistic")
    lo = ds.glm_multi(Yb, Z, model="logistic", subset=ss, v_begin=0, v_end=40)
    for p, single in enumerate(_singles(ds, Yb, Z, "logistic", subset=ss, v_begin=0, v_end=40)):
        _same(_col(lo, p), single, ctx=p)


M_D, N_D = 2100, 70001


@pytest.fixture(scope="module")
def dosage_fixture(gpu_lib, tmp_path_factory):
    prefix = str(tmp_path_factory.mktemp("glm_multi_dosage") / "dos")
    gpu_lib.synth_write_dosage_files(prefix, M_D, N_D, 21, 0.02, 0.3)
    ds = gpu_lib.Dataset.open(prefix + ".pgen")
    assert ds.info.dosage_variant_ct > 0
    return ds


@pytest.mark.gpu
def test_dosage_track_variants_across_dosage_chunks(gpu_lib, dosage_fixture):
    """512 MiB of dense dosages per chunk: 958 variants at 70,001 samples, so three chunks; then under a subset."""
    ds = dosage_fixture
    rng = np.random.default_rng(41)
    Z = rng.normal(size=(2, N_D))
    Y = _phenotypes(rng, N_D, 5, 2, Z, mode="shared")
    out = ds.glm_multi(Y, Z)
    for p, single in enumerate(_singles(ds, Y, Z, "linear")):
        _close(_col(out, p), single, ctx=p)
    keep = rng.random(N_D) < 0.6
    n = int(keep.sum())
    ss = ds.subset(keep)
    Zs = rng.normal(size=(2, n))
    Ys = _phenotypes(rng, n, 3, 2, Zs, mode="distinct")
    out = ds.glm_multi(Ys, Zs, subset=ss)
    for p, single in enumerate(_singles(ds, Ys, Zs, "linear", subset=ss)):
        _close(_col(out, p), single, ctx=("subset", p))


@pytest.mark.gpu
def test_arguments_and_sparse_refusal(gpu_lib, widths_fixture):
    L = gpu_lib
    ds, x = widths_fixture
    Y = np.zeros((2, N_W))
    with pytest.raises(ValueError, match="phenotypes"):
        ds.glm_multi(Y[:, :-1])
    with pytest.raises(ValueError):
        ds.glm_multi(Y, np.zeros((21, N_W)))
    with pytest.raises(ValueError):
        ds.glm_multi(Y, model=7)
    assert ds.glm_multi(Y, v_begin=10, v_end=10)["beta"].shape == (0, 2)
    sp = L.Dataset.open(data_path("rare_small.pgen"), sparse=True)
    with pytest.raises(ValueError, match="dense-resident"):
        sp.glm_multi(np.zeros((3, sp.n_samples)), v_begin=0, v_end=8)
    sp.close()
