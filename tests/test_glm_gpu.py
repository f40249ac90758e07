"""pgh_glm / Dataset.glm on the device: the reference's plink_glm expectations (test/sql/plink_glm.test and
plink_glm_pthreshold.test, replayed with the bind steps done here), random fixtures against an FP64 numpy oracle of
the same rules (tests/glm_oracle.py), dosage tracks, many sample chunks, shard groups and adjacent windows."""

import math

import numpy as np
import pytest

from conftest import data_path
from glm_oracle import NAN, _pheno, _same_rows, check_rows

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------
# the reference's expectations
# ---------------------------------------------------------------------------

PGEN = "pgen_example.pgen"
LARGE = "large_example.pgen"
P4 = [1.5, 2.3, 3.7, 0.8]
P8 = [1.2, 3.4, 2.1, 5.6, 4.3, 0.9, 3.8, 2.7]
AGE = [25.0, 30.0, 35.0, 40.0, 45.0, 50.0, 55.0, 60.0]
BMI = [22.1, 24.5, 23.0, 28.3, 26.1, 21.5, 25.8, 23.2]


def _glm(gpu_lib, name, pheno, covars=None, model="auto", firth=True):
    """The reference's bind: NULL -> NaN, the model rule, then one pgh_glm call over the file."""
    m, y = gpu_lib.glm_model(pheno, model)
    ds = gpu_lib.Dataset.open(data_path(name))
    z = None if covars is None else np.array(covars, dtype=np.float64)
    out = ds.glm(y, z, model=m, firth=firth)
    if m == gpu_lib.GLM_LOGISTIC:
        out["or"] = np.exp(out["beta"])
    return out


def _printed(got, exp):
    """The unrounded expectations are plink2's own output (the reference test says so) and agree with an exact FP64
    fit to 1e-5 relative, the tolerance of the reference's test runner for REAL columns (rs2's SE is 2.6e-6 off:
    0.332603367... is the closed-form value).  The ROUND()ed expectations below are matched digit for digit."""
    return got == pytest.approx(exp, rel=1e-5, abs=1e-12)


def test_reference_linear_no_covariates(gpu_lib):
    out = _glm(gpu_lib, PGEN, P4)
    exp = [
        (0.5, 3, 1.1, 0.17320508075688776, 6.350852961085884, 0.09942530566691602),
        (0.5, 4, -1.45, 0.33260250429475794, -4.359548017600793, 0.04879676508539067),
        (0.5, 3, 0.3500000000000001, 1.4722431864335457, 0.23773160637676483, 0.8514126919174483),
        (0.375, 4, -0.33636363636363636, 0.8879360193399447, -0.37881508091390906, 0.7412587024131992),
    ]
    assert len(out["beta"]) == 4
    for i, (af, obs, beta, se, t, p) in enumerate(exp):
        assert out["errcode"][i] is None and not out["firth"][i]
        assert out["obs_ct"][i] == obs
        for key, e in (("a1_freq", af), ("beta", beta), ("se", se), ("stat", t), ("p", p)):
            assert _printed(out[key][i], e), (i, key, out[key][i], e)
    # ROUND(BETA, 4) and the P < 0.1 join (ROUND(P, 6))
    assert [round(b, 4) for b in out["beta"]] == [1.1, -1.45, 0.35, -0.3364]
    small = sorted((p, i) for i, p in enumerate(out["p"]) if p < 0.1)
    assert [i for _, i in small] == [1, 0]
    # the reference prints rs2's ROUND(P, 6) as 0.04880: within its runner's tolerance of 0.048797
    assert abs(small[0][0] - 0.04880) < 1e-5 and round(small[1][0], 6) == 0.099425


def test_reference_p_threshold(gpu_lib):
    def kept(out, thr):
        return [i for i in range(len(out["p"]))
                if out["errcode"][i] is None and not math.isnan(out["p"][i]) and out["p"][i] <= thr]

    out = _glm(gpu_lib, PGEN, P4)
    assert len(kept(out, 1.0)) == 4
    assert kept(out, 0.1) == [0, 1]
    assert kept(out, 0.05) == [1]
    out = _glm(gpu_lib, PGEN, [1.5, None, 3.7, 0.8])
    assert kept(out, 1.0) == [1, 2, 3]
    big = _glm(gpu_lib, LARGE, P8)
    assert len(big["beta"]) == 3000
    assert 0 < len(kept(big, 0.5)) <= len(kept(big, 1.0)) <= 3000


def test_reference_null_phenotype(gpu_lib):
    out = _glm(gpu_lib, PGEN, [1.5, None, 3.7, 0.8])
    assert list(out["obs_ct"]) == [2, 3, 3, 3]
    assert list(out["errcode"]) == ["TOO_FEW_SAMPLES", None, None, None]
    assert math.isnan(out["beta"][0]) and math.isnan(out["a1_freq"][0])
    assert [round(b, 4) for b in out["beta"][1:]] == [-1.45, 0.35, -0.35]


def test_reference_linear_large(gpu_lib):
    out = _glm(gpu_lib, LARGE, P8)
    assert round(out["a1_freq"][0], 4) == 0.5 and out["obs_ct"][0] == 6
    assert round(out["beta"][0], 6) == -1.0 and round(out["se"][0], 6) == 0.878505
    out = _glm(gpu_lib, LARGE, P8, [AGE])
    assert (round(out["beta"][0], 6), round(out["se"][0], 6), round(out["p"][0], 6)) == (-1.120455, 1.062566, 0.369083)
    assert out["obs_ct"][0] == 6
    out = _glm(gpu_lib, LARGE, P8, [AGE, BMI])
    assert (round(out["beta"][0], 6), round(out["se"][0], 6), round(out["p"][0], 6)) == (0.020132, 0.247427, 0.942561)
    # forced linear on a binary phenotype
    out = _glm(gpu_lib, LARGE, [0, 1, 0, 1, 1, 0, 1, 0], model="linear")
    assert round(out["beta"][0], 6) == 0.0 and not out["firth"][0] and "or" not in out


def test_reference_logistic(gpu_lib):
    def near(got, exp):
        return abs(got - exp) <= 1e-5 + 5e-7

    out = _glm(gpu_lib, LARGE, [0, 1, 0, 1, 1, 0, 1, 0], [AGE])
    assert out["errcode"][0] is None and not out["firth"][0]
    for key, e in (("beta", -0.287203), ("se", 1.11879), ("or", 0.75036), ("p", 0.797404)):
        assert near(out[key][0], e), (key, out[key][0], e)
    assert len(out["beta"]) == 3000
    for pheno in ([0, 1, 0, 1, 1, 0, 1, 0], [1, 2, 1, 2, 2, 1, 2, 1]):
        out = _glm(gpu_lib, LARGE, pheno)
        assert not out["firth"][0]
        for key, e in (("beta", 0.0), ("se", 1.0), ("or", 1.0)):
            assert near(out[key][0], e), (key, out[key][0], e)
    out = _glm(gpu_lib, LARGE, [0, 1, 0, 1, 1, 0, 1, 0], firth=False)
    assert near(out["or"][0], 1.0) and not out["firth"][0]


def test_reference_firth(gpu_lib):
    pheno = [0, 1, 0, 0, 1, 1, 0, 0]
    out = _glm(gpu_lib, LARGE, pheno)
    assert out["errcode"][0] is None and out["firth"][0]
    for key, e in (("beta", 1.855205), ("se", 1.248652), ("stat", 1.485766), ("p", 0.137341), ("or", 6.393007)):
        assert abs(out[key][0] - e) <= 1e-5 + 5e-7, (key, out[key][0], e)
    assert round(out["beta"][0], 4) == 1.8552 and round(out["or"][0], 4) == 6.393
    out = _glm(gpu_lib, LARGE, pheno, firth=False)
    assert out["errcode"][0] == "NO_CONVERGENCE" and math.isnan(out["beta"][0]) and not out["firth"][0]
    # forced logistic on a continuous phenotype
    out = _glm(gpu_lib, LARGE, P8, model="logistic")
    assert out["errcode"][0] == "NO_CONVERGENCE"


def test_argument_errors(gpu_lib):
    ds = gpu_lib.Dataset.open(data_path(LARGE))
    y = np.array(P8)
    with pytest.raises(ValueError, match="model"):
        ds.glm(y, model=7)
    with pytest.raises(ValueError, match="not finite"):
        ds.glm(y, np.array([AGE[:7] + [NAN]]))
    with pytest.raises(ValueError, match="covariates"):
        ds.glm(y, np.ones((21, 8)))
    with pytest.raises(ValueError, match="outside"):
        ds.glm(y, v_begin=10, v_end=3001)


# ---------------------------------------------------------------------------
# random fixtures against the oracle
# ---------------------------------------------------------------------------

M_RAND, N_RAND = 2000, 3001


@pytest.fixture(scope="module")
def rand_fixture(gpu_lib, tmp_path_factory):
    """A 2,000 x 3,001 matrix (2 % missing calls) with edge variants written over the first rows."""
    rng = np.random.default_rng(20261016)
    geno = rng.binomial(2, rng.uniform(0.05, 0.5, M_RAND)[:, None], size=(M_RAND, N_RAND)).astype(np.int8)
    geno[rng.random((M_RAND, N_RAND)) < 0.02] = -9
    geno[0, :] = 1                   # constant
    geno[1, :] = -9                  # all missing
    geno[2, :] = np.where(rng.random(N_RAND) < 0.5, 0, -9)  # constant among the called
    geno[3, :] = -9
    geno[3, :2] = [0, 2]             # too few samples
    geno[4, rng.random(N_RAND) < 0.6] = -9  # many missing calls: the dense correction
    # rows as 2-bit records (00 hom-ref, 01 het, 10 hom-alt, 11 missing)
    codes = np.where(geno < 0, 3, geno).astype(np.uint8)
    pad = (-N_RAND) % 4
    codes = np.concatenate([codes, np.zeros((M_RAND, pad), np.uint8)], axis=1).reshape(M_RAND, -1, 4)
    rows = (codes[:, :, 0] | (codes[:, :, 1] << 2) | (codes[:, :, 2] << 4) | (codes[:, :, 3] << 6)).astype(np.uint8)
    ds = gpu_lib.Dataset.from_host_rows(rows, N_RAND)
    x = geno.astype(np.float64)
    return ds, x, rows, rng


@pytest.mark.parametrize("k", [0, 3, 20])
def test_random_linear(gpu_lib, rand_fixture, k):
    ds, x, _, rng = rand_fixture
    Z = rng.normal(size=(k, N_RAND)) * [[10.0 ** (j % 3)] for j in range(k)] if k else np.zeros((0, N_RAND))
    y = _pheno(rng, N_RAND, "linear", Z)
    out = ds.glm(y, Z if k else None, model="linear")
    idx = list(range(0, 12)) + list(range(12, M_RAND, 7 if k < 20 else 41))
    fitted = check_rows(out, x, y, Z, "linear", rel=1e-9, idx=idx)
    assert fitted > len(idx) // 2
    assert list(out["errcode"][:4]) == ["CONST_ALLELE", "TOO_FEW_SAMPLES", "CONST_ALLELE", "TOO_FEW_SAMPLES"]


def test_random_linear_subset_and_singular(gpu_lib, rand_fixture):
    ds, x, _, rng = rand_fixture
    keep = rng.random(N_RAND) < 0.7
    ss = ds.subset(keep)
    n = int(keep.sum())
    Z = rng.normal(size=(3, n))
    y = _pheno(rng, n, "linear", Z)
    out = ds.glm(y, Z, model="linear", subset=ss)
    xs = x[:, keep]
    check_rows(out, xs, y, Z, "linear", rel=1e-9, idx=range(0, M_RAND, 11))
    # a duplicated covariate
    Zd = np.vstack([Z, Z[1:2]])
    out = ds.glm(y, Zd, model="linear", subset=ss)
    assert set(out["errcode"][5:]) == {"SINGULAR_MATRIX"}
    check_rows(out, xs, y, Zd, "linear", idx=range(0, 40))


@pytest.mark.parametrize("k", [0, 2, 3])
def test_random_logistic(gpu_lib, rand_fixture, k):
    ds, x, _, rng = rand_fixture
    Z = rng.normal(size=(k, N_RAND)) if k else np.zeros((0, N_RAND))
    y = _pheno(rng, N_RAND, "logistic", Z)
    out = ds.glm(y, Z if k else None, model="logistic")
    idx = list(range(0, 12)) + list(range(12, M_RAND, 13))
    fitted = check_rows(out, x, y, Z, "logistic", rel=1e-6, idx=idx)
    assert fitted > len(idx) // 2


def test_random_logistic_separation_and_firth(gpu_lib, rand_fixture):
    """Variants that separate the cases: Firth rows with it, SEPARATION / NO_CONVERGENCE rows without."""
    ds, x, _, rng = rand_fixture
    n = 60
    sub = np.zeros(N_RAND, bool)
    sub[:n] = True
    ss = ds.subset(sub)
    xs = x[:, :n]
    y = (xs[40] > 0).astype(np.float64)  # a case status that variant 40 predicts perfectly where it is called
    y[xs[40] < 0] = 0.0
    Z = rng.normal(size=(2, n))
    with_f = ds.glm(y, Z, model="logistic", subset=ss)
    without = ds.glm(y, Z, model="logistic", firth=False, subset=ss)
    idx = list(range(30, 60))
    check_rows(with_f, xs, y, Z, "logistic", True, rel=1e-6, idx=idx)
    check_rows(without, xs, y, Z, "logistic", False, rel=1e-6, idx=idx)
    assert with_f["firth"][40] and without["errcode"][40] in ("SEPARATION", "NO_CONVERGENCE")


def test_dosage_tracks(gpu_lib, oracle, tmp_path):
    prefix = str(tmp_path / "dos")
    m, n = 300, 1001
    gpu_lib.synth_write_dosage_files(prefix, m, n, 11, 0.02, 0.3)
    ds = gpu_lib.Dataset.open(prefix + ".pgen")
    assert ds.info.dosage_variant_ct > 0
    pg = oracle.Pgen(prefix + ".pgen")
    xs = np.stack([pg.dosage(v) for v in range(m)])
    rng = np.random.default_rng(5)
    Z = rng.normal(size=(2, n))
    y = _pheno(rng, n, "linear", Z)
    check_rows(ds.glm(y, Z, model="linear"), xs, y, Z, "linear", rel=1e-9)
    yb = _pheno(rng, n, "logistic", Z)
    check_rows(ds.glm(yb, Z, model="logistic"), xs, yb, Z, "logistic", rel=1e-6, idx=range(0, m, 5))


def test_many_sample_chunks(gpu_lib):
    n, m = 200_003, 6
    ds = gpu_lib.Dataset.synth(0, m, n, 77, 0.02)
    rows = ds.copy_rows_to_host(0, m)
    codes = np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(m, -1)[:, :n]
    x = np.where(codes == 3, -9.0, codes.astype(np.float64))
    rng = np.random.default_rng(9)
    Z = rng.normal(size=(3, n))
    y = _pheno(rng, n, "linear", Z)
    check_rows(ds.glm(y, Z, model="linear"), x, y, Z, "linear", rel=1e-9)
    yb = _pheno(rng, n, "logistic", Z)
    check_rows(ds.glm(yb, Z, model="logistic"), x, yb, Z, "logistic", rel=1e-6)


@pytest.mark.parametrize("model", ["linear", "logistic"])
def test_shard_group_and_windows(gpu_lib, model):
    m, n = 900, 2003
    rng = np.random.default_rng(3)
    Z = rng.normal(size=(2, n))
    y = _pheno(rng, n, model, Z)
    whole = gpu_lib.Dataset.synth(0, m, n, 4242, 0.02)
    ref = whole.glm(y, Z, model=model)
    # a group with one device named twice
    grp = gpu_lib.Dataset.group([gpu_lib.Dataset.synth(0, 377, n, 4242, 0.02),
                                 gpu_lib.Dataset.synth(377, m, n, 4242, 0.02)])
    _same_rows(grp.glm(y, Z, model=model), ref)
    _same_rows(grp.glm(y, Z, model=model, v_begin=300, v_end=500),
               {k: v[300:500] for k, v in ref.items()})
    # two windows opened on adjacent ranges (the streamed-file use)
    a = gpu_lib.Dataset.synth(0, 450, n, 4242, 0.02)
    b = gpu_lib.Dataset.synth(450, m, n, 4242, 0.02)
    ra, rb = a.glm(y, Z, model=model), b.glm(y, Z, model=model)
    _same_rows({k: np.concatenate([ra[k], rb[k]]) for k in ref}, ref)
