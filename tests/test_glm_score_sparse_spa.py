"""pgh_glm_score_sparse_spa / Dataset.glm_score_sparse_spa: the saddlepoint p-value of the logistic score test over a
sparse-resident dataset.  Against the FP64 oracle (tests/glm_spa_oracle.py: QR residuals, its own null fit, bisection,
the score's support) the states are equal and p_spa is within TOL in state 1; the rows are pgh_glm_score_sparse's bit
for bit; a row's triple does not depend on the range, the window or the chunk.

TOL is 100 x the worst relative difference between the numpy model of the kernel's accumulation order
(tools/glm_score_spa_model.py) and the oracle on the parity test's inputs, MODEL_WORST below.  The cases at every
covariate width are held to TOL_WIDTHS, the same rule on their own rows: MODEL_WORST_WIDTHS is what
`python tools/glm_score_spa_model.py --widths` prints."""

import math
import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import glm_score_oracle as O
import glm_spa_oracle as S
import pgen_writer as W

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_score_sparse_spa"]
MODEL_WORST = 8.13e-12  # printed by tools/glm_score_spa_model.py
TOL = 100 * MODEL_WORST
MODEL_WORST_WIDTHS = 1.78e-12  # printed by tools/glm_score_spa_model.py --widths: the width cases, on their rows
TOL_WIDTHS = 100 * MODEL_WORST_WIDTHS
CUTOFF = 2.0
ROW_KEYS = ("beta", "se", "stat", "p", "a1_freq", "obs_ct", "errcode", "firth")


# ---- inputs ------------------------------------------------------------------------------------------------------

def _values(geno):
    return np.where(geno == 3, -9.0, geno.astype(np.float64))


def _pheno(rng, n, case_rate=0.1, missing=0.03):
    y = (rng.random(n) < case_rate).astype(np.float64)
    y[rng.random(n) < missing] = NAN
    return y


def _covariates(rng, k, y):
    """Covariates on three scales that the phenotype depends on (each is shifted among the cases)."""
    z = rng.normal(size=(k, len(y))) + 0.5 * np.nan_to_num(y, nan=0.0)
    return z * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]


HET_ROWS = (7, 8)  # rare_matrix draws no het-majority rows: these two are made so
LONG_ROW, FAILING_AT = 9, 10
FAILING_ROW = {257: ([47, 86, 99, 175, 196, 251], [2, 0, 0, 0, 0, 0])}  # found by a search on the CPU with the oracle
M_R = 600
PARITY_N = (257, 4099)
SEEDS = {257: 257, 4099: 4102}  # seeds whose matrices hold no row the contract leaves undecided (the oracle asserts it)
PARITY_K = (0, 1, 3)
# every padded covariate width of kGlmWidths at its exact value and one above the bucket below it
# (test_glm_widths_chunks.WIDTHS without the k = 1 of PARITY_K), at the count that crosses a 4,096-sample step
WIDTHS = [2, 4, 5, 8, 9, 12, 13, 16, 17, 20]
WIDTHS_N = 4099
WIDTHS_STRIDE = 5  # the rows the width cases check: the oracle's time is the test's
# ... of this file: with the het-majority rows and the row beyond the wave form, so that both teams run at every width
WIDTHS_ROWS = sorted(set(range(0, M_R, WIDTHS_STRIDE)) | set(HET_ROWS) | {LONG_ROW})


class ParityInputs:
    """The parity test's matrix for n samples: 600 rare_matrix variants, the two het-majority rows, and every fourth
    hom-ref-majority variant enriched for ALT calls among the cases of the one phenotype all k share."""

    def __init__(self, n, m=M_R, seed=None, plant=0, assoc=1.0):
        rng = np.random.default_rng(SEEDS.get(n, n) if seed is None else seed)
        self.n, self.m = n, m
        geno = W.rare_matrix(m, n, rng)
        for v, rate in zip(HET_ROWS, (0.01, 0.3)):
            hit = rng.random(n) < rate
            geno[v] = 1
            geno[v, hit] = rng.integers(0, 4, hit.sum(), dtype=np.uint8)
        self.y = _pheno(rng, n)
        cases = self.y == 1.0
        # ... and associated: hom-alt among the cases (assoc scales the made rows' effects down for a large n)
        for v, rate in zip(HET_ROWS, (0.3, 0.5)):
            geno[v, cases & (rng.random(n) < rate * assoc)] = 2
        # a hom-ref-majority row of about 0.35 n entries (beyond the wave form at n = 4,099), associated too
        hit = rng.random(n) < 0.3
        geno[LONG_ROW] = 0
        geno[LONG_ROW, hit] = rng.integers(1, 4, hit.sum(), dtype=np.uint8)
        geno[LONG_ROW, cases & (rng.random(n) < 0.6 * assoc)] = 1
        if n in FAILING_ROW:  # a missing-majority row whose -|U| lies outside the support of its score for some k
            samples, codes = FAILING_ROW[n]
            geno[FAILING_AT] = 3
            geno[FAILING_AT, samples] = codes
        # plant: as many of the rows with a hom-alt majority, or a hom-ref majority and more than 0.2 n other calls,
        # get another call in a hundredth of the cases
        for v in range(FAILING_AT + 1, m):
            counts = np.bincount(geno[v], minlength=4)
            if plant and (counts.argmax() == 2 or (counts.argmax() == 0 and n - counts[0] > 0.2 * n)):
                geno[v, cases & (rng.random(n) < 0.01)] = 1 if counts.argmax() == 2 else 2
                plant -= 1
        self.geno = S.enriched_matrix(geno, self.y, rng, 5.0 * assoc)
        self.kinds = W.choose_kinds(self.geno, rng)
        self.x = _values(self.geno)

    def covariates(self, k):
        return _covariates(np.random.default_rng(100 * self.n + k), k, self.y)


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_score_sparse_spa(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_score_sparse_spa")


@pytest.mark.parametrize("shape", [(4,), (6,), (1, 5)])
def test_glm_score_sparse_spa_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotype"):
        lib.Dataset.glm_score_sparse_spa(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_sparse_spa(fake, np.zeros(5), np.zeros((2, 4)))


@pytest.fixture(scope="module")
def small_case():
    """n = 257, k = 3 of the parity inputs, its null fit and its fitted rows beyond the cutoff (the first 25)."""
    case = ParityInputs(257)
    nul = O.Null(case.y, case.covariates(3))
    assert nul.status is None
    rows = []
    for i in range(case.m):
        row = O.oracle_row(case.x[i], nul)
        if row["errcode"] is None and abs(row["stat"]) > CUTOFF:
            rows.append(i)
    assert len(rows) >= 25
    return case, nul, rows[:25]


def test_oracle_cgf_derivatives_at_zero_and_by_differences(small_case):
    case, nul, rows = small_case
    for i in rows:
        for max_minor in (0, case.n):
            base, dense_form = S.row_form(case.geno[i], max_minor)
            cgf, u, v = S.cgf_of(case.x[i], case.geno[i], nul, base, dense_form)
            if base == 3 and not dense_form:
                continue  # V_rest = 0 by rule and E = N: K''(0) = V still
            assert abs(cgf.k1(0.0)) <= 1e-12 * math.sqrt(v) * max(1.0, abs(u) / math.sqrt(v))
            assert abs(cgf.k2(0.0) - v) <= 1e-12 * v
            for s in (0.7 / math.sqrt(v), -1.9 / math.sqrt(v)):
                h = 1e-4 / math.sqrt(v)
                d1 = (cgf.k0(s + h) - cgf.k0(s - h)) / (2 * h)
                d2 = (cgf.k1(s + h) - cgf.k1(s - h)) / (2 * h)
                assert abs(d1 - cgf.k1(s)) <= 1e-6 * math.sqrt(v), (i, s)
                assert abs(d2 - cgf.k2(s)) <= 1e-6 * v, (i, s)


def test_oracle_base3_rows_have_all_of_v_in_e(small_case):
    case, nul, _ = small_case
    seen = 0
    for i in range(case.m):
        base, dense_form = S.row_form(case.geno[i], case.n)
        if base == 3 and O.oracle_row(case.x[i], nul)["errcode"] is None:
            cgf, _, v = S.cgf_of(case.x[i], case.geno[i], nul, base, dense_form)
            assert cgf.v_rest == 0.0 and abs(cgf.k2(0.0) - v) <= 1e-12 * v
            seen += 1
    assert seen


def test_oracle_cutoff_above_every_stat_leaves_p(small_case):
    case, nul, rows = small_case
    for i in rows:
        row, p_spa, state = S.spa_row(case.x[i], case.geno[i], nul, *S.row_form(case.geno[i], 0), cutoff=1e9)
        assert state == 0 and p_spa == row["p"]


def _tiny_design():
    """18 samples, 2 cases, one covariate; the rows are every carrier set of one to three samples (hets)."""
    import itertools
    rng = np.random.default_rng(22)
    n = 18
    y = np.zeros(n)
    y[[2, 11]] = 1.0
    Z = rng.normal(size=(1, n)) + 0.8 * y
    nul = O.Null(y, Z)
    assert nul.status is None
    rows = []
    for size in (1, 2, 3):
        for carriers in itertools.combinations(range(n), size):
            codes = np.zeros(n, dtype=np.uint8)
            codes[list(carriers)] = 1
            rows.append(codes)
    return nul, rows


class _Exact:
    """P(|S| >= |u|), both tails inclusive, S = sum g (Y - mu), Y independent Bernoulli(mu): all 2^n outcomes."""

    def __init__(self, mu):
        n = len(mu)
        bits = ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(np.float64)
        self.mu = mu
        self.prob = np.prod(np.where(bits == 1.0, mu, 1.0 - mu), axis=1)
        self.centred = bits - mu

    def two_sided(self, g, u):
        s = self.centred @ g
        tol = 1e-9 * max(1.0, abs(u))
        return float(self.prob[s >= abs(u) - tol].sum() + self.prob[s <= -abs(u) + tol].sum())


TINY_EXCLUDED = 1  # rows with exact p < 0.01 that have no saddlepoint (|U| at, or -|U| outside, the support)
EXACT_SHARE = 1.0  # the share of the rows with exact p < 0.01 where the saddlepoint p is the closer one


def test_oracle_saddlepoint_is_closer_to_the_exact_p_than_the_normal_p():
    """E = N on a tiny skewed design (the rows are held as if under a missing-majority base: every sample an entry,
    V_rest = 0): against the enumeration of the score's null distribution.  Guards the formulas, not the device."""
    nul, rows = _tiny_design()
    closer = total = excluded = 0
    exact_of = None
    for codes in rows:
        x = codes.astype(np.float64)
        row = O.oracle_row(x, nul)
        if row["errcode"] is not None:
            continue
        cgf, u, v = S.cgf_of(x, codes, nul, 3, False)
        if exact_of is None:
            exact_of = _Exact(cgf.mu)  # no call is missing: every row has the same N and mu
        assert np.array_equal(exact_of.mu, cgf.mu)
        exact = exact_of.two_sided(cgf.g, u)
        if not exact < 0.01:
            continue
        lo, hi = cgf.support()
        if min(hi - abs(u), -lo - abs(u)) <= 1e-3 * math.sqrt(v):
            excluded += 1
            continue  # the observed score is the most extreme one, or -|U| is not in the support: no saddlepoint
        tails = [cgf.tail(q, v) for q in (abs(u), -abs(u))]
        assert None not in tails
        total += 1
        closer += abs(math.log(sum(tails) / exact)) < abs(math.log(row["p"] / exact))
    print(f"saddlepoint closer than normal on {closer} of {total} rows with exact p < 0.01; {excluded} more such rows "
          f"have no saddlepoint")
    assert total >= 15 and excluded == TINY_EXCLUDED
    assert closer >= EXACT_SHARE * total


@pytest.mark.parametrize("k", WIDTHS)
def test_the_width_inputs_have_applied_rows_of_both_teams(k):
    """Conditions on the inputs, not on the device: at every width the null model is fitted, the oracle decides every
    checked row (it asserts where the contract does not), and with every row held sparse the applied rows lie on both
    sides of the wave / workgroup threshold of 1,024 entries."""
    case = ParityInputs(WIDTHS_N)
    nul = O.Null(case.y, case.covariates(k))
    assert nul.status is None
    for max_minor in (case.n, 0):
        entries = []
        for i in WIDTHS_ROWS:
            base, dense_form = S.row_form(case.geno[i], max_minor)
            row, p_spa, state = S.spa_row(case.x[i], case.geno[i], nul, base, dense_form, CUTOFF)
            if state == 1:
                entries.append(int(S.entry_mask(case.geno[i], base, dense_form).sum()))
        print(f"k={k} max_minor={max_minor}: {len(entries)} applied, {min(entries)} to {max(entries)} entries")
        assert len(entries) >= 3, (k, max_minor)
        if max_minor:
            assert min(entries) <= 1024 < max(entries), (k, entries)


# ---- on the GPU --------------------------------------------------------------------------------------------------

def _same_rows(a, b, ctx=None):
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    for key in ("obs_ct", "errcode", "firth"):
        assert np.asarray(a[key]).tolist() == np.asarray(b[key]).tolist(), (key, ctx)


def _same(a, b, ctx=None):
    _same_rows(a, b, ctx)
    assert np.array_equal(a["p_spa"], b["p_spa"], equal_nan=True), ctx
    assert a["spa_state"].tolist() == b["spa_state"].tolist(), ctx


def _rows(out, idx):
    return {key: v[idx] for key, v in out.items()}


class _File(ParityInputs):
    """The inputs as a .pgen of every record type."""

    def __init__(self, L, tmp, n, m=M_R, seed=None, plant=0, assoc=1.0):
        super().__init__(n, m, seed, plant, assoc)
        self.L = L
        self.path = str(tmp / f"spa_{n}.pgen")
        W.write_pgen(self.path, self.geno, self.kinds)

    def sparse(self, **kw):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(97 * ((self.n + 3) // 4 + 15) // 16 * 16))
            return self.L.Dataset.open(self.path, sparse=True, **kw)


@pytest.fixture(scope="module")
def spa_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_sparse_spa")
    return {n: _File(gpu_lib, tmp, n) for n in PARITY_N}


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_parity_with_the_oracle_for_every_form(gpu_lib, spa_files, n, k):
    f = spa_files[n]
    Z = f.covariates(k)
    zc = Z if k else None
    nul = O.Null(f.y, Z)
    assert nul.status is None
    results, seen = {}, {}
    for max_minor in (0, 1, n):
        sp = f.sparse(max_minor=max_minor)
        got = results[max_minor] = sp.glm_score_sparse_spa(f.y, zc, cutoff=CUTOFF)
        _same_rows(got, sp.glm_score_sparse(f.y, zc), ctx=(n, k, max_minor))
        s = seen[max_minor] = S.check_spa(got, f.x, f.geno, nul, max_minor, CUTOFF, TOL)
        print(f"n={n} k={k} max_minor={max_minor}: {s['applied']} applied, {s['differ']} beyond 2x, {s['failed']} failed, "
              f"worst {s['worst']:.3g}")
        assert s["applied"] >= 30 and s["differ"] >= 10
        sp.close()
    # applied rows of every base code held sparse, and (n = 257, k = 1) the made row that fails
    assert {0, 1, 2} <= {r[1] for r in seen[n]["rows"] if not r[2]}
    if (n, k) == (257, 1):
        assert seen[n]["failed"] >= 1 and got["spa_state"][FAILING_AT] == 2
    if n == 4099:  # both sides of the wave / workgroup threshold, and dense-form rows
        entries = [r[3] for r in seen[n]["rows"]]
        assert min(entries) <= 1024 < max(entries)
        assert any(r[2] for r in seen[1]["rows"])
    # rows whose E is the same set under two max_minor values
    for a, b in ((0, 1), (0, n), (1, n)):
        ea = {r[0]: r for r in seen[a]["rows"]}
        both = 0
        for r in seen[b]["rows"]:
            o = ea.get(r[0])
            if o is None:
                continue
            same_e = np.array_equal(S.entry_mask(f.geno[r[0]], o[1], o[2]), S.entry_mask(f.geno[r[0]], r[1], r[2]))
            if same_e and (o[1] == 3 and not o[2]) == (r[1] == 3 and not r[2]):
                pa, pb = results[a]["p_spa"][r[0]], results[b]["p_spa"][r[0]]
                assert abs(pa - pb) <= 2 * TOL * pb, (n, k, a, b, r, pa, pb)
                both += 1
        assert both > 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_instantiated_width(gpu_lib, spa_files, k):
    """GlmScoreSpaKernel<KP, TEAM> for every width GlmPadCovar returns, at k = KP and one above the width below: with
    every row held sparse and under the default rule."""
    f = spa_files[WIDTHS_N]
    Z = f.covariates(k)
    nul = O.Null(f.y, Z)
    assert nul.status is None
    for max_minor in (f.n, 0):
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_spa(f.y, Z, cutoff=CUTOFF)
        _same_rows(got, sp.glm_score_sparse(f.y, Z), ctx=(k, max_minor))
        s = S.check_spa(got, f.x, f.geno, nul, max_minor, CUTOFF, TOL_WIDTHS, idx=WIDTHS_ROWS)
        print(f"k={k} max_minor={max_minor}: {s['applied']} applied, {s['failed']} failed, worst {s['worst']:.3g} "
              f"(TOL {TOL_WIDTHS:.3g})")
        assert s["applied"] >= 3
        if max_minor:
            entries = [r[3] for r in s["rows"]]
            assert min(entries) <= 1024 < max(entries)
        sp.close()


@pytest.mark.gpu
def test_cutoff(gpu_lib, spa_files):
    f = spa_files[257]
    k = 1
    Z = f.covariates(k)
    nul = O.Null(f.y, Z)
    sp = f.sparse(max_minor=f.n)
    base = sp.glm_score_sparse(f.y, Z)
    got = sp.glm_score_sparse_spa(f.y, Z, cutoff=math.inf)
    _same_rows(got, base)
    assert not got["spa_state"].any()
    assert np.array_equal(got["p_spa"], base["p"], equal_nan=True)
    at2 = sp.glm_score_sparse_spa(f.y, Z, cutoff=CUTOFF)
    low = sp.glm_score_sparse_spa(f.y, Z, cutoff=0.1)
    _same_rows(low, base)
    s = S.check_spa(low, f.x, f.geno, nul, f.n, 0.1, TOL)
    print(f"cutoff 0.1: {s['applied']} applied, {s['failed']} failed, worst {s['worst']:.3g}")
    assert (low["spa_state"] == 1).sum() > (at2["spa_state"] == 1).sum()
    # refused before anything is written
    raw = gpu_lib.raw()
    import ctypes as C
    y = np.ascontiguousarray(f.y)
    z = np.ascontiguousarray(Z)
    for bad in (NAN, 0.0, -1.0, 0.0999):
        rows = np.full(f.m, 0x5A, dtype=np.uint8).repeat(gpu_lib.GLM_ROW_DTYPE.itemsize)
        p_spa = np.full(f.m, 123.0)
        state = np.full(f.m, 77, dtype=np.uint8)
        eb = C.create_string_buffer(1024)
        rc = raw.pgh_glm_score_sparse_spa(sp._h, None, 0, f.m, y.ctypes.data, k, z.ctypes.data, C.c_double(bad),
                                          rows.ctypes.data, p_spa.ctypes.data, state.ctypes.data, eb)
        assert rc != 0 and b"spa_cutoff must be at least 0.1" in eb.value, (bad, rc, eb.value)
        assert (rows == 0x5A).all() and (p_spa == 123.0).all() and (state == 77).all()
        with pytest.raises(ValueError, match="spa_cutoff must be at least 0.1"):
            sp.glm_score_sparse_spa(f.y, Z, cutoff=bad)
    sp.close()


@pytest.mark.gpu
def test_a_triple_does_not_depend_on_the_range_or_the_window(gpu_lib, spa_files):
    f = spa_files[4099]
    Z = f.covariates(3)
    v0 = next(v for v in range(150, M_R) if f.kinds[v] in (2, 3))  # a window that starts after an LD base
    v1 = min(M_R, v0 + 150)
    for max_minor in (0, 1, f.n):
        sp = f.sparse(max_minor=max_minor)
        whole = sp.glm_score_sparse_spa(f.y, Z)
        assert (whole["spa_state"] == 1).sum() >= 30
        _same(sp.glm_score_sparse_spa(f.y, Z), whole, ctx="again")
        _same(sp.glm_score_sparse_spa(f.y, Z, v_begin=40, v_end=333), _rows(whole, slice(40, 333)), ctx=max_minor)
        empty = sp.glm_score_sparse_spa(f.y, Z, v_begin=77, v_end=77)
        assert empty["p_spa"].shape == (0,) and empty["spa_state"].shape == (0,)
        part = f.sparse(max_minor=max_minor, variant_begin=v0, variant_end=v1)
        _same(part.glm_score_sparse_spa(f.y, Z), _rows(whole, slice(v0, v1)), ctx=(max_minor, v0))
        part.close()
        sp.close()


CHUNK = 16384  # variants per chunk of the GLM family


@pytest.mark.gpu
def test_triples_across_a_chunk_boundary(gpu_lib, tmp_path):
    L = gpu_lib
    m, n = CHUNK + 300, 257
    prefix = str(tmp_path / "chunks")
    L.synth_write_files(prefix, m, n, 5152, 0.02)
    rng = np.random.default_rng(62)
    y = _pheno(rng, n, case_rate=0.1)
    Z = _covariates(rng, 2, y)
    for max_minor in (8, n):  # dense-form and sparse rows mixed, and every row sparse
        sp = L.Dataset.open(prefix + ".pgen", sparse=True, max_minor=max_minor)
        info = sp.sparse_info()
        assert info.sparse_variant_ct > 0 and (info.dense_variant_ct > 0) == (max_minor == 8)
        whole = sp.glm_score_sparse_spa(y, Z, v_begin=5)
        _same_rows(whole, sp.glm_score_sparse(y, Z, v_begin=5), ctx=max_minor)
        applied = np.flatnonzero(whole["spa_state"] == 1)
        assert (applied < CHUNK - 5).any() and (applied >= CHUNK - 5).any()
        for lo, hi in ((5 + CHUNK - 40, 5 + CHUNK + 60), (5, 5 + CHUNK), (5 + CHUNK, m), (m - 30, m)):
            _same(sp.glm_score_sparse_spa(y, Z, v_begin=lo, v_end=hi), _rows(whole, slice(lo - 5, hi - 5)),
                  ctx=(max_minor, lo))
        sp.close()


@pytest.mark.gpu
def test_sample_subset(gpu_lib, spa_files):
    f = spa_files[4099]
    rng = np.random.default_rng(13)
    keep = rng.random(f.n) < 0.5
    assert int(keep.sum()) % 64
    y = f.y[keep]
    k = 3
    Z = _covariates(rng, k, y)
    nul = O.Null(y, Z)
    assert nul.status is None
    idx = list(range(0, M_R, 2))
    for max_minor in (0, 1, f.n):
        sp = f.sparse(max_minor=max_minor)
        ss = sp.subset(keep)
        got = sp.glm_score_sparse_spa(y, Z, subset=ss)
        _same_rows(got, sp.glm_score_sparse(y, Z, subset=ss), ctx=max_minor)
        forms = [S.row_form(f.geno[i], max_minor) for i in range(f.m)]  # the form comes from all raw samples
        s = S.check_spa(got, f.x[:, keep], f.geno[:, keep], nul, forms, CUTOFF, TOL, idx=idx)
        print(f"subset max_minor={max_minor}: {s['applied']} applied, {s['failed']} failed, worst {s['worst']:.3g}")
        assert s["applied"] >= 10
        ss.close()
        sp.close()


LONG_N, LONG_M, LONG_K = 70_000, 120, 20


def long_inputs(cls=ParityInputs, *args):
    """The long-row shape.  The made rows' effects and the enrichment are scaled down (7,000 cases carry more
    evidence than 25), and twelve rows of many entries get an effect of their own: |stat| stays below 11."""
    return cls(*args, LONG_N, m=LONG_M, seed=70, plant=12, assoc=0.02)


@pytest.mark.gpu
def test_long_dense_form_rows(gpu_lib, tmp_path):
    """n = 70,000, k = 20: with max_minor = 1 the rows are held in the dense form, and a hom-alt- or missing-majority
    row has most of its samples as entries, beyond any LDS stash.  Every dense-form row of more than 10,000 entries
    is checked against the oracle, state and p_spa."""
    n, m, k = LONG_N, LONG_M, LONG_K
    f = long_inputs(_File, gpu_lib, tmp_path)
    Z = f.covariates(k)
    nul = O.Null(f.y, Z)
    assert nul.status is None
    sp = f.sparse(max_minor=1)
    got = sp.glm_score_sparse_spa(f.y, Z)
    _same_rows(got, sp.glm_score_sparse(f.y, Z))
    forms = [S.row_form(f.geno[i], 1) for i in range(m)]
    entries = np.array([S.entry_mask(f.geno[i], *forms[i]).sum() for i in range(m)])
    idx = [i for i in range(m) if forms[i][1] and entries[i] > 10_000]
    s = S.check_spa(got, f.x, f.geno, nul, forms, CUTOFF, TOL, idx=idx)
    print(f"long rows: {s['applied']} applied of {len(idx)} checked, worst {s['worst']:.3g}")
    assert s["applied"] >= 5
    sp.close()


def _decision_file(tmp_path):
    """test_glm_score_sparse's decision file: CONST_ALLELE, TOO_FEW_SAMPLES and SINGULAR_MATRIX rows."""
    n = 64
    rng = np.random.default_rng(5)
    y = (rng.random(n) < 0.35).astype(np.float64)
    no_pheno = np.array([3, 17, 40])
    y[no_pheno] = NAN
    y[[1, 2, 5, 9]] = [0.0, 0.0, 1.0, 1.0]
    geno = np.zeros((8, n), dtype=np.uint8)
    geno[0, no_pheno] = 1
    geno[1, 17] = 2
    geno[2] = 2
    geno[2, no_pheno[:2]] = [0, 1]
    geno[3] = 3
    geno[3, [1, 2, 5]] = [0, 1, 2]
    geno[4] = 3
    geno[4, [1, 2, 5, 9]] = [0, 1, 2, 1]
    geno[5] = rng.binomial(2, 0.2, n)
    geno[6] = rng.binomial(2, 0.3, n)
    geno[6, rng.random(n) < 0.1] = 3
    geno[7] = 1
    geno[7, rng.random(n) < 0.2] = 3
    path = str(tmp_path / "decisions.pgen")
    W.write_pgen(path, geno, [0] * len(geno))
    return path, geno, y


@pytest.mark.gpu
def test_undecided_rows(gpu_lib, tmp_path, spa_files):
    L = gpu_lib
    path, geno, y = _decision_file(tmp_path)
    Z = geno[5].astype(np.float64)[None, :]
    sp = L.Dataset.open(path, sparse=True, max_minor=geno.shape[1])
    got = sp.glm_score_sparse_spa(y, Z, cutoff=0.1)
    _same_rows(got, sp.glm_score_sparse(y, Z))
    assert list(got["errcode"]) == ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", "TOO_FEW_SAMPLES", None,
                                    "SINGULAR_MATRIX", None, "CONST_ALLELE"]
    undecided = got["errcode"] != None  # noqa: E711
    assert np.isnan(got["p_spa"][undecided]).all() and not got["spa_state"][undecided].any()
    assert not np.isnan(got["p_spa"][~undecided]).any()
    sp.close()
    # a collinear-covariate call: the null status on every row it leaves undecided
    f = spa_files[257]
    z = f.covariates(1)[0]
    sp = f.sparse(max_minor=f.n)
    got = sp.glm_score_sparse_spa(f.y, np.stack([z, z]))
    _same_rows(got, sp.glm_score_sparse(f.y, np.stack([z, z])))
    assert "SINGULAR_MATRIX" in set(got["errcode"]) and not (got["errcode"] == None).any()  # noqa: E711
    assert np.isnan(got["p_spa"]).all() and not got["spa_state"].any()
    sp.close()


@pytest.mark.gpu
def test_refusals(gpu_lib):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    n = sp.n_samples
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    rows = sp.glm_score_sparse_spa(y, v_begin=0, v_end=8)
    assert rows["p_spa"].shape == (8,) and rows["spa_state"].dtype == np.uint8
    y2 = y.copy()
    y2[4] = 2.0
    with pytest.raises(ValueError, match="phenotype must be 0 or 1"):
        sp.glm_score_sparse_spa(y2)
    with pytest.raises(ValueError, match="sparse-resident"):
        dense.glm_score_sparse_spa(y, v_begin=0, v_end=8)
    with pytest.raises(ValueError, match="at most 20 covariates"):
        sp.glm_score_sparse_spa(y, np.zeros((21, n)))
    with pytest.raises(ValueError, match="outside the resident range"):
        sp.glm_score_sparse_spa(y, v_begin=0, v_end=sp.v_end + 1)
    with pytest.raises(ValueError, match="outside the resident range"):
        sp.glm_score_sparse_spa(y, v_begin=9, v_end=8)
    sp.close()
    dense.close()
