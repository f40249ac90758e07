"""pgh_glm / Dataset.glm over its whole dispatch, against the FP64 oracle (tests/glm_oracle.py): every padded
covariate width of the linear sums and of the logistic / Firth accumulation (GlmPadCovar: 0, 1, 2, 4, 8, 12, 16,
20), fits that take more than one variant chunk (16,384 variants) or dosage chunk (512 MiB of dense dosages),
windows and shard groups across those chunks, the sample-count boundary and the CONST_ALLELE rule on dosages."""

import numpy as np
import pytest

pytest.importorskip("scipy.stats")

import pgen_writer as W  # noqa: E402
from glm_oracle import (NAN, _pheno, _same_rows, calls_of_rows, check_rows, one_pass_sxx, rows_2bit,  # noqa: E402
                        scipy_stats, two_pass_sxx)

pytestmark = pytest.mark.gpu

# each padded width at its exact value and just above the bucket below it (padded columns present)
WIDTHS = [1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 20]
M_W, N_W = 400, 3001
SEP = 5  # the variant the Firth phenotypes are built from


@pytest.fixture(scope="module")
def widths_fixture(gpu_lib):
    """A 400 x 3,001 matrix (2 % missing calls), the edge variants of test_glm_gpu's fixture in rows 0-4, and in
    row 5 a common variant that the Firth phenotypes separate."""
    rng = np.random.default_rng(20261017)
    geno = rng.binomial(2, rng.uniform(0.05, 0.5, M_W)[:, None], size=(M_W, N_W)).astype(np.int8)
    geno[rng.random((M_W, N_W)) < 0.02] = -9
    geno[0, :] = 1                   # constant
    geno[1, :] = -9                  # all missing
    geno[2, :] = np.where(rng.random(N_W) < 0.5, 0, -9)  # constant among the called
    geno[3, :] = -9
    geno[3, :2] = [0, 2]             # too few samples
    geno[4, rng.random(N_W) < 0.6] = -9  # many missing calls: the dense correction
    geno[SEP, :] = rng.binomial(2, 0.1, N_W)
    ds = gpu_lib.Dataset.from_host_rows(rows_2bit(geno), N_W)
    return ds, geno.astype(np.float64)


EDGE_CODES = ["CONST_ALLELE", "TOO_FEW_SAMPLES", "CONST_ALLELE", "TOO_FEW_SAMPLES"]


@pytest.mark.parametrize("k", [0] + WIDTHS)
def test_linear_every_width(gpu_lib, widths_fixture, k):
    ds, x = widths_fixture
    rng = np.random.default_rng(100 + k)
    Z = rng.normal(size=(k, N_W)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]
    y = _pheno(rng, N_W, "linear", Z)
    out = ds.glm(y, Z if k else None, model="linear")
    idx = list(range(12)) + list(range(12, M_W, 9))
    fitted = check_rows(out, x, y, Z, "linear", rel=1e-9, idx=idx)
    assert fitted > len(idx) // 2
    assert list(out["errcode"][:4]) == EDGE_CODES


@pytest.mark.parametrize("k", [0] + WIDTHS)
def test_logistic_every_width(gpu_lib, widths_fixture, k):
    ds, x = widths_fixture
    rng = np.random.default_rng(200 + k)
    Z = rng.normal(size=(k, N_W))
    y = _pheno(rng, N_W, "logistic", Z)
    out = ds.glm(y, Z if k else None, model="logistic")
    idx = list(range(12)) + list(range(12, M_W, 17))
    fitted = check_rows(out, x, y, Z, "logistic", rel=1e-6, idx=idx)
    assert fitted > len(idx) // 2
    assert list(out["errcode"][:4]) == EDGE_CODES


@pytest.mark.parametrize("k", [0, 1, 3, 8, 11, 16, 20])
def test_firth_every_width(gpu_lib, widths_fixture, k):
    """Every carrier of variant SEP is a case (quasi-separation): its Newton fit fails and Firth's takes over, so
    GlmIrlsAccKernel's two Firth passes run at this width next to ordinary fits."""
    ds, x = widths_fixture
    rng = np.random.default_rng(300 + k)
    Z = rng.normal(size=(k, N_W))
    y = np.where(x[SEP] > 0, 1.0, (rng.random(N_W) < 0.3).astype(np.float64))
    y[x[SEP] < 0] = 0.0
    with_f = ds.glm(y, Z if k else None, model="logistic")
    without = ds.glm(y, Z if k else None, model="logistic", firth=False)
    idx = list(range(12)) + list(range(12, M_W, 23))
    seen = {}
    check_rows(with_f, x, y, Z, "logistic", True, rel=1e-6, idx=idx, seen=seen)
    check_rows(without, x, y, Z, "logistic", False, rel=1e-6, idx=idx)
    assert seen[SEP]["firth"] and with_f["firth"][SEP]
    assert without["errcode"][SEP] in ("SEPARATION", "NO_CONVERGENCE")
    assert any(r["errcode"] is None and not r["firth"] for r in seen.values())


@pytest.mark.parametrize("model", ["linear", "logistic"])
def test_subset_width_12(gpu_lib, widths_fixture, model):
    ds, x = widths_fixture
    rng = np.random.default_rng(12)
    keep = rng.random(N_W) < 0.7
    ss = ds.subset(keep)
    n = int(keep.sum())
    Z = rng.normal(size=(12, n))
    y = _pheno(rng, n, model, Z)
    out = ds.glm(y, Z, model=model, subset=ss)
    idx = list(range(12)) + list(range(12, M_W, 19))
    fitted = check_rows(out, x[:, keep], y, Z, model, rel=1e-9 if model == "linear" else 1e-6, idx=idx)
    assert fitted > len(idx) // 2


def test_linear_offsets_and_scales(gpu_lib, widths_fixture):
    """Covariates far from zero and of very different scales, and a phenotype offset: the host centres y and z
    before the device's Gram, and the result must match the QR oracle of the raw design."""
    ds, x = widths_fixture
    rng = np.random.default_rng(77)
    age = 2e4 + 4e3 * rng.normal(size=N_W)      # age in days
    pc = 1e-3 * rng.normal(size=N_W)            # a principal component
    batch = (rng.random(N_W) < 0.4).astype(np.float64)
    Z = np.vstack([age, pc, batch])
    y = 1e4 + 2e-4 * (age - 2e4) + 300.0 * pc + 0.5 * batch + rng.normal(size=N_W)
    y[rng.random(N_W) < 0.03] = NAN
    out = ds.glm(y, Z, model="linear")
    idx = list(range(12)) + list(range(12, M_W, 5))
    fitted = check_rows(out, x, y, Z, "linear", rel=1e-9, idx=idx)
    assert fitted > len(idx) // 2


def test_sample_count_boundary(gpu_lib, widths_fixture):
    """k = 20: a fit needs n >= p + 1 = 23 called samples with a phenotype; with exactly 23 it has df = 1."""
    ds, x = widths_fixture
    rng = np.random.default_rng(23)
    k = 20
    for n in (22, 23):
        sub = np.zeros(N_W, bool)
        sub[:n] = True
        Z = rng.normal(size=(k, n))
        y = rng.normal(size=n)
        out = ds.glm(y, Z, model="linear", subset=ds.subset(sub))
        xs = x[:, sub]
        called = (xs != -9.0).sum(axis=1)
        assert list(out["obs_ct"]) == list(called)
        if n == 22:
            assert set(out["errcode"]) == {"TOO_FEW_SAMPLES"}
            continue
        # one residual degree of freedom: the fit can be close to exact, and the RSS, which any normal-equations
        # solve (the device's and the reference's) takes as a difference of sums of squares, keeps fewer digits
        fitted = check_rows(out, xs, y, Z, "linear", rel=1e-9,
                            rel_of=lambda e: 1e-9 * max(1.0, e["tss"] / max(e["rss"], 1e-300)))
        full = called == 23
        assert fitted > M_W // 3
        assert all(out["errcode"][~full] == "TOO_FEW_SAMPLES")
        for v in np.flatnonzero(full):
            if out["errcode"][v] is None:
                assert out["p"][v] == pytest.approx(2 * scipy_stats.t.sf(abs(out["stat"][v]), 1), rel=1e-9)


# ---------------------------------------------------------------------------
# more than one variant chunk (kGlmChunk = 16,384 variants)
# ---------------------------------------------------------------------------

CHUNK = 16384
M_C, N_C, SEED_C = 2 * CHUNK + 77, 96, 5150
V0_C = 5  # the calls start here, so the chunk boundaries fall at 16389 and 32773


@pytest.fixture(scope="module")
def chunk_fixture(gpu_lib):
    ds = gpu_lib.Dataset.synth(0, M_C, N_C, SEED_C, 0.02)
    x = calls_of_rows(ds.copy_rows_to_host(0, M_C), N_C)
    rng = np.random.default_rng(31)
    Z = rng.normal(size=(2, N_C))
    pheno = {"linear": _pheno(rng, N_C, "linear", Z),
             # few cases: rare variants without a case carrier are separated, and Firth fits them
             "logistic": np.where(rng.random(N_C) < 0.1, 1.0, 0.0)}
    whole = {m: ds.glm(pheno[m], Z, model=m, v_begin=V0_C) for m in pheno}
    return ds, x, Z, pheno, whole


@pytest.mark.parametrize("model", ["linear", "logistic"])
def test_variant_chunks_against_oracle(gpu_lib, chunk_fixture, model):
    ds, x, Z, pheno, whole = chunk_fixture
    out = whole[model]
    assert len(out["beta"]) == M_C - V0_C
    b1, b2 = V0_C + CHUNK, V0_C + 2 * CHUNK
    idx = set(range(b1 - 9, b1 + 7)) | set(range(M_C - 10, M_C)) | set(range(V0_C, M_C, 250)) | {b2 - 1, b2}
    if model == "logistic":
        # Firth rows in the second and the third chunk, and the oracle checks some of each
        for lo, hi in ((b1, b2), (b2, M_C)):
            f = [v for v in range(lo, hi) if out["firth"][v - V0_C]]
            assert f, (lo, hi)
            idx |= set(f[:5])
    rel = 1e-9 if model == "linear" else 1e-6
    fitted = check_rows(out, x, pheno[model], Z, model, rel=rel, idx=sorted(idx), got_idx=lambda v: v - V0_C)
    assert fitted > len(idx) // 2


@pytest.mark.parametrize("model", ["linear", "logistic"])
def test_variant_chunks_window_and_group(gpu_lib, chunk_fixture, model):
    """A variant's row does not depend on its chunk or shard: a window across the first boundary and a two-shard
    group (its first shard spanning two chunks) reproduce the whole-range call bit for bit."""
    ds, x, Z, pheno, whole = chunk_fixture
    ref = whole[model]
    lo, hi = 16000, 16800
    _same_rows(ds.glm(pheno[model], Z, model=model, v_begin=lo, v_end=hi),
               {key: v[lo - V0_C:hi - V0_C] for key, v in ref.items()})
    grp = gpu_lib.Dataset.group([gpu_lib.Dataset.synth(0, 20000, N_C, SEED_C, 0.02),
                                 gpu_lib.Dataset.synth(20000, M_C, N_C, SEED_C, 0.02)])
    _same_rows(grp.glm(pheno[model], Z, model=model, v_begin=V0_C), ref)


# ---------------------------------------------------------------------------
# more than one dosage chunk (512 MiB of dense FP64 dosages per chunk)
# ---------------------------------------------------------------------------

M_D, N_D = 2100, 70001


def _dosage_chunk(n_out):
    return min(CHUNK, (512 << 20) // (8 * n_out))


@pytest.fixture(scope="module")
def dosage_fixture(gpu_lib, oracle, tmp_path_factory):
    prefix = str(tmp_path_factory.mktemp("glm_dosage") / "dos")
    gpu_lib.synth_write_dosage_files(prefix, M_D, N_D, 21, 0.02, 0.3)
    path = prefix + ".pgen"
    ds = gpu_lib.Dataset.open(path)
    assert ds.info.dosage_variant_ct > 0
    return path, ds, oracle.Pgen(path)


def _boundary_rows(m, chunk):
    idx = {0, 1, m - 2, m - 1}
    for b in range(chunk, m, chunk):
        idx |= set(range(b - 3, b + 3))
    return sorted(idx | set(range(0, m, 151)))


@pytest.mark.parametrize("model", ["linear", "logistic"])
def test_dosage_chunks(gpu_lib, dosage_fixture, model):
    path, ds, pg = dosage_fixture
    chunk = _dosage_chunk(N_D)
    assert 2 * chunk < M_D  # three chunks
    rng = np.random.default_rng(41)
    Z = rng.normal(size=(2, N_D))
    y = _pheno(rng, N_D, model, Z)
    out = ds.glm(y, Z, model=model)
    idx = _boundary_rows(M_D, chunk)
    xs = {v: pg.dosage(v) for v in idx}
    rel = 1e-9 if model == "linear" else 1e-6
    fitted = check_rows(out, xs, y, Z, model, rel=rel, idx=idx)
    assert fitted > len(idx) // 2
    # a window opened inside the file: its own chunks start at variant 137
    win = gpu_lib.Dataset.open(path, variant_begin=137, variant_end=1500)
    _same_rows(win.glm(y, Z, model=model), {key: v[137:1500] for key, v in out.items()})


def test_dosage_chunks_subset(gpu_lib, dosage_fixture):
    path, ds, pg = dosage_fixture
    rng = np.random.default_rng(43)
    keep = rng.random(N_D) < 0.6
    n = int(keep.sum())
    chunk = _dosage_chunk(n)
    assert chunk < M_D  # two chunks
    Z = rng.normal(size=(2, n))
    for model in ("linear", "logistic"):
        y = _pheno(rng, n, model, Z)
        out = ds.glm(y, Z, model=model, subset=ds.subset(keep))
        idx = _boundary_rows(M_D, chunk)
        xs = {v: pg.dosage(v)[keep] for v in idx}
        rel = 1e-9 if model == "linear" else 1e-6
        fitted = check_rows(out, xs, y, Z, model, rel=rel, idx=idx)
        assert fitted > len(idx) // 2


# ---------------------------------------------------------------------------
# CONST_ALLELE on dosages: the reference's two-pass variance, not the one-pass form
# ---------------------------------------------------------------------------

N_K = 20001
D_K = 4915  # 4915 / 16384 ~ 0.3: n x^2 - (n x)^2 / n rounds to a positive number at n = 20,001


@pytest.fixture(scope="module")
def const_fixture(gpu_lib, tmp_path_factory):
    """Dosage-track variants: 0 every sample at D_K; 1 the same with 10 missing calls; 2 one sample at 1.0 (a
    normal fit); 3 every sample at 0.5 (exact in either form); 4 random dosages."""
    rng = np.random.default_rng(53)
    m = 5
    geno = np.zeros((m, N_K), np.uint8)
    dos = np.full((m, N_K), D_K, np.uint16)
    miss = rng.choice(N_K, 10, replace=False)
    geno[1, miss] = 3
    dos[1, miss] = 0xFFFF
    dos[2, 7] = 16384
    dos[3] = 8192
    dos[4] = rng.integers(0, 32769, N_K)
    path = str(tmp_path_factory.mktemp("glm_const") / "const.pgen")
    W.write_pgen(path, geno, [0] * m, dosage=dos, dosage_kinds=[0x40] * m)
    x = np.where(dos == 0xFFFF, -9.0, dos / 16384.0)
    return gpu_lib.Dataset.open(path), x


def test_const_allele_dosage(gpu_lib, const_fixture):
    ds, x = const_fixture
    c = D_K / 16384.0
    # the host facts the test rests on: the one-pass form misses the constant rows, the two-pass form does not
    for v in (0, 1):
        xs = x[v][x[v] != -9.0]
        assert one_pass_sxx(xs) > 0.0 and two_pass_sxx(xs) == 0.0, v
    assert (x[1] != -9.0).sum() == N_K - 10
    rng = np.random.default_rng(59)
    for model, ks in (("linear", (1, 3)), ("logistic", (0, 2))):
        for k in ks:
            Z = rng.normal(size=(k, N_K))
            y = rng.normal(size=N_K) if model == "linear" else (rng.random(N_K) < 0.4).astype(np.float64)
            out = ds.glm(y, Z if k else None, model=model)
            ctx = (model, k, list(out["errcode"]), list(out["obs_ct"]))
            assert list(out["errcode"][[0, 1, 3]]) == ["CONST_ALLELE"] * 3, ctx
            assert list(out["obs_ct"][[0, 1, 3]]) == [N_K, N_K - 10, N_K], ctx
            assert list(out["a1_freq"][[0, 1, 3]]) == [c / 2, c / 2, 0.25], ctx
            assert np.isnan(out["beta"][[0, 1, 3]]).all(), ctx
            fitted = check_rows(out, x, y, Z, model, rel=1e-9 if model == "linear" else 1e-6)
            assert fitted == 2 and out["errcode"][2] is None and out["errcode"][4] is None, ctx
