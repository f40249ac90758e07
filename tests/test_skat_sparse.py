"""pgh_skat_sparse / Dataset.skat_sparse: per variant set, the SKAT test and the burden score test of a binary
phenotype under pgh_glm_score_sparse's null model, from the entries of a sparse-resident dataset; and the two host
functions it is finished with, pgh_symmetric_eigenvalues and pgh_skat_p_from_lambda.

The yardstick is tests/skat_oracle.py: dense float64 numpy over the subsetted code matrix, numpy.linalg.eigvalsh, and a
line-for-line transcription of the p-value definition, which is itself held against scipy (chi2.sf for equal
eigenvalues, Imhof's inversion integral otherwise).  errcode, obs_ct, n_carriers, n_lambda and p_state are equal; q,
beta, se, stat, p and lambda_sum within 1e-9 relative on tests/test_glm_score_sparse.py's scales; the eigenvalues within
1e-9 lambda_1; p_skat is pgh_skat_p_from_lambda of the returned q and eigenvalues bit for bit, and within 1e-6 relative
of the oracle's.  A set's row does not depend on the other sets, their order, the scratch budget or the window: bit
for bit."""

import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT, data_path

import pgen_writer as W
import subset_shapes as SS

NAN = float("nan")
NEW_SYMBOLS = ["pgh_skat_sparse", "pgh_skat_p_from_lambda", "pgh_symmetric_eigenvalues"]
SCRATCH_ENV = "PGH_SKAT_SCRATCH_BYTES"
REL = 1e-9  # tests/test_glm_score_sparse.py's tolerance for its estimates


def _oracle():
    # the oracle's null fit and the references of the p-value need scipy, as the glm oracles do
    pytest.importorskip("scipy")
    import skat_oracle
    return skat_oracle


# ---- no device: the surface --------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_skat_sparse(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert "} pgh_skat_row;" in header and "#define PGH_SKAT_MAX_SET 256" in header
    assert lib.SKAT_MAX_SET == 256
    assert hasattr(lib.Dataset, "skat_sparse") and hasattr(lib, "skat_p_from_lambda")
    # the struct of the header, field for field: 8 doubles, three uint32, errcode, p_state, 2 bytes of padding
    assert C.sizeof(lib.PghSkatRow) == 80 == lib.SKAT_ROW_DTYPE.itemsize
    assert [f[0] for f in lib.PghSkatRow._fields_] == list(lib.SKAT_ROW_DTYPE.names)
    want = dict(q=0, p_skat=8, beta=16, se=24, stat=32, p=40, lambda_sum=48, lambda_max=56, obs_ct=64, n_carriers=68,
                n_lambda=72, errcode=76, p_state=77, pad=78)
    for name in lib.SKAT_ROW_DTYPE.names:
        assert getattr(lib.PghSkatRow, name).offset == lib.SKAT_ROW_DTYPE.fields[name][1] == want[name], name


def test_wrapper_checks_shapes_before_the_library_is_called(lib):
    """The stand-in dataset has no handle to call with."""
    import types
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    off, vidx = np.array([0, 2, 3]), np.array([1, 0, 2])
    for bad, text in ((dict(phenotype=np.zeros(4)), "phenotype"), (dict(covariates=np.zeros((2, 4))), "covariates"),
                      (dict(set_vidx=vidx[:2]), "memberships"), (dict(weights=np.ones(2)), "weights"),
                      (dict(set_off=np.zeros(0, dtype=np.int64)), "n_sets"), (dict(set_vidx=np.array([1, -1, 2])), "set_vidx"),
                      (dict(set_off=np.array([0.0, 2.0, 3.0])), "set_off")):
        kw = dict(phenotype=np.zeros(5), set_off=off, set_vidx=vidx)
        kw.update(bad)
        with pytest.raises(ValueError, match=text):
            lib.Dataset.skat_sparse(fake, **kw)
    with pytest.raises(ValueError, match="one-dimensional"):
        lib.skat_p_from_lambda(1.0, np.ones((2, 2)))


def test_a_null_dataset_is_refused_without_a_device(lib):
    out = np.full(80, 0xAB, dtype=np.uint8)
    lam = np.full(8, 0xAB, dtype=np.uint8)
    eb = C.create_string_buffer(lib.ERRBUF_LEN)
    off = np.array([0, 1], dtype=np.uint64)
    vidx = np.array([0], dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.raw().pgh_skat_sparse(None, None, None, 0, None, 1, p(off), p(vidx), None, p(out), p(lam), eb)
    assert rc == lib.PGH_ERR_ARG and b"null dataset" in eb.value and (out == 0xAB).all() and (lam == 0xAB).all()


# ---- no device: the eigenvalues ----------------------------------------------------------------------------------

def _eig_cases():
    rng = np.random.default_rng(20261019)
    cases = []
    for n in (1, 2, 3, 17, 64, 256):
        a = rng.normal(size=(n, n))
        cases.append((f"random {n}", a + a.T))
    b = rng.normal(size=(40, 7))
    cases.append(("rank-deficient Gram", b @ b.T))
    r = rng.normal(size=(6, 30))
    r = r[[0, 1, 2, 0, 3, 1, 4, 0, 5]]
    cases.append(("repeated rows", r @ r.T))
    cases.append(("diagonal", np.diag(rng.normal(size=12) * 10.0 ** rng.integers(-3, 4, 12))))
    cases.append(("zero", np.zeros((5, 5))))
    return cases


def test_symmetric_eigenvalues_against_eigvalsh(lib):
    for name, a in _eig_cases():
        n = len(a)
        got = lib.symmetric_eigenvalues(a)
        want = np.linalg.eigvalsh(a)[::-1]
        assert got.shape == (n,) and np.all(np.diff(got) <= 0), name
        bound = 1e-12 * n * np.abs(want).max()
        worst = np.abs(got - want).max()
        print(f"{name}: worst |difference| {worst:.3e}, bound {bound:.3e}")
        assert worst <= bound, name
    out = np.zeros(2)
    a = np.eye(2)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.raw().pgh_symmetric_eigenvalues(p(a), 0, p(out)) == lib.PGH_ERR_ARG
    assert lib.raw().pgh_symmetric_eigenvalues(None, 2, p(out)) == lib.PGH_ERR_ARG
    assert lib.raw().pgh_symmetric_eigenvalues(p(a), 2, None) == lib.PGH_ERR_ARG
    a[0, 1] = a[1, 0] = np.inf
    assert np.isnan(lib.symmetric_eigenvalues(a)).all()


# ---- no device: the p-value --------------------------------------------------------------------------------------

P_M = (1, 2, 3, 5, 20, 100, 256)


def _p_grid():
    """(lambda, q) pairs: for every m, Gamma(0.5) and equal eigenvalues; q from mu - 0.8 sd to mu + 40 sd, with points
    inside and just outside the near-mean band |q - mu| <= 1e-3 sd."""
    rng = np.random.default_rng(1999)
    steps = [-0.8, -0.5, -0.1, -2e-3, -1.001e-3, -0.999e-3, -1e-4, 0.0, 1e-4, 0.999e-3, 1.001e-3, 2e-3, 0.1, 0.5, 1.0,
             2.0, 5.0, 10.0, 20.0, 40.0]
    for m in P_M:
        for lam in (np.sort(rng.gamma(0.5, size=m))[::-1] + 1e-6, np.full(m, 0.37)):
            mu, sd = lam.sum(), math.sqrt(2.0 * (lam ** 2).sum())
            for t in steps:
                yield lam, mu + t * sd


def test_p_from_lambda_is_the_transcription(lib):
    K = _oracle()
    seen = set()
    worst = 0.0
    for lam, q in _p_grid():
        got, state = lib.skat_p_from_lambda(q, lam, return_state=True)
        want, wstate = K.p_from_lambda(q, lam)
        assert state == wstate, (len(lam), q, got, want)
        seen.add(state)
        if math.isnan(want):
            assert math.isnan(got), (len(lam), q)
        else:
            worst = max(worst, abs(got - want) / want)
            assert abs(got - want) <= 1e-8 * want, (len(lam), q, got, want)
    print(f"worst relative difference from the transcription: {worst:.3e}")
    assert seen == {K.EXACT, K.SADDLE, K.NEAR_MEAN, K.FAILED}
    # the state pointer may be NULL
    lam = np.array([2.0, 1.0])
    assert lib.raw().pgh_skat_p_from_lambda(3.0, lam.ctypes.data_as(C.c_void_p), 2, None) == lib.skat_p_from_lambda(3.0, lam)


def test_one_eigenvalue_is_glm_p_from_z_bit_for_bit(lib):
    rng = np.random.default_rng(3)
    for _ in range(200):
        lam, q = float(rng.gamma(0.5)) + 1e-9, float(rng.gamma(2.0) * 10.0 ** rng.integers(-3, 3))
        got, state = lib.skat_p_from_lambda(q, [lam], return_state=True)
        assert state == lib.SKAT_P_EXACT and got == lib.glm_p_from_z(math.sqrt(q / lam))


def test_failures_are_state_4(lib):
    for q, lam in ((-1.0, [1.0, 0.5]), (-1e-300, [1.0]), (NAN, [1.0, 0.5]), (math.inf, [1.0, 0.5]), (1.0, [1.0, NAN]),
                   (1.0, [math.inf, 1.0]), (1.0, [1.0, 0.0]), (1.0, [1.0, -0.5]), (1.0, [])):
        got, state = lib.skat_p_from_lambda(q, lam, return_state=True)
        assert state == lib.SKAT_P_FAILED and math.isnan(got), (q, lam)
    assert lib.skat_p_from_lambda(0.0, [1.0, 0.5], return_state=True) == (1.0, lib.SKAT_P_FAILED)


# the figures of the header for equal eigenvalues, per m, times 1.25
EQUAL_BOUND = {2: 1.25 * 0.059, 5: 1.25 * 0.019, 50: 1.25 * 0.0008}


def test_equal_eigenvalues_against_chi2(lib):
    from scipy.stats import chi2
    for m, bound in EQUAL_BOUND.items():
        worst = 0.0
        for lg in np.arange(-0.5, -20.01, -0.5):
            exact = 10.0 ** lg
            lam = 0.37
            q = lam * chi2.isf(exact, m)
            got = lib.skat_p_from_lambda(q, np.full(m, lam))
            worst = max(worst, abs(got - exact) / exact)
        print(f"m = {m}: worst relative deviation from chi2.sf {worst:.4f}, bound {bound:.4f}")
        assert worst <= bound, m


IMHOF_BOUND = 0.10


def test_transcription_against_imhof_quadrature():
    """The worst relative deviation of the saddlepoint p from Imhof's inversion over a seeded grid, where the exact
    p >= 1e-3 (the quadrature's own error estimate is asserted to be far below the bound)."""
    K = _oracle()
    rng = np.random.default_rng(1961)
    worst, count = 0.0, 0
    for m in (2, 3, 5, 20, 100):
        for _ in range(3):
            lam = rng.gamma(0.5, size=m) + 1e-6
            mu, sd = lam.sum(), math.sqrt(2.0 * (lam ** 2).sum())
            for t in (-0.5, 0.3, 1.0, 2.0, 3.0, 4.5):
                q = mu + t * sd
                if q <= 0.0:
                    continue
                exact, err = K.imhof_sf(q, lam)
                if exact < 1e-3:
                    continue
                assert err <= 1e-3 * exact, (m, t, exact, err)
                p, state = K.p_from_lambda(q, lam)
                assert state == K.SADDLE
                worst = max(worst, abs(p - exact) / exact)
                count += 1
    print(f"worst relative deviation from Imhof over {count} points: {worst:.4f}")
    assert count >= 60 and worst <= IMHOF_BOUND


# ---- the fixtures of the device tests ----------------------------------------------------------------------------

from test_burden_sparse import _Forms, _csr  # noqa: E402  (the resident forms and the CSR of a set list)

ROW_ALL_MISSING, ROW_MONO, HET_ROWS = 3, 4, (7, 8)


class _File:
    """subset_shapes.rare_codes(n) with an all-missing and a monomorphic row, as a .pgen of every record type."""

    def __init__(self, L, tmp, n):
        self.L, self.n = L, n
        self.codes, self.y = SS.rare_codes(n)
        self.codes = self.codes.copy()
        self.codes[ROW_ALL_MISSING] = 3
        self.codes[ROW_MONO] = 0
        self.m = len(self.codes)
        self.path = str(tmp / f"skat_{n}.pgen")
        W.write_pgen(self.path, self.codes, W.choose_kinds(self.codes, np.random.default_rng(7 * n)))
        dense = L.Dataset.open(self.path)
        self.pitch = dense.info.pitch_bytes
        dense.close()
        self._open = {}

    def sparse(self, max_minor, window=97):
        key = (max_minor, window)
        if key not in self._open:
            with pytest.MonkeyPatch.context() as mp:  # several windows per open, as the sparse tests do
                mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(window * self.pitch))
                self._open[key] = self.L.Dataset.open(self.path, sparse=True, max_minor=max_minor)
        return self._open[key], _Forms(self.codes, max_minor, self.pitch)

    def close(self):
        for sp in self._open.values():
            sp.close()


@pytest.fixture(scope="module")
def files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("skat_sparse")
    made = {}

    def get(n):
        if n not in made:
            made[n] = _File(gpu_lib, tmp, n)
        return made[n]

    yield get
    for f in made.values():
        f.close()


def set_list(codes, seed):
    """The sets of the parity tests and the variant whose carriers lose their phenotype (set "no carrier in S")."""
    rng = np.random.default_rng(seed)
    m, n = codes.shape
    major = _Forms(codes, n, 16).major
    entries = codes != major[:, None]
    count = entries.sum(axis=1)
    alt = ((codes == 1) | (codes == 2)).sum(axis=1)
    ref = np.flatnonzero((major == 0) & (alt > 0))
    # members with no shared carrier: hom-ref-majority rows whose non-reference samples are disjoint
    apart, taken = [], np.zeros(n, dtype=bool)
    for v in ref[np.argsort(count[ref], kind="stable")]:
        if not (entries[v] & taken).any():
            apart.append(int(v))
            taken |= entries[v]
        if len(apart) == 6:
            break
    assert len(apart) == 6
    # members that all share carriers: the rows with the most entries (held in the dense form under max_minor = 0)
    common = [int(v) for v in np.argsort(-count, kind="stable")[:5]]
    shared = entries[common].astype(np.int64)
    assert ((shared @ shared.T) > 0).all()
    miss_major = [int(v) for v in np.flatnonzero((major == 3) & (count > 0))[:2]]
    alt_major = int(np.flatnonzero((major == 2) & (count > 0))[0])
    assert len(miss_major) == 2 and major[list(HET_ROWS)].tolist() == [1, 1]
    lone = int(next(v for v in ref[6:] if 1 <= count[v] <= 6 and v not in apart and v not in common))
    sets = [[int(ref[0])], [int(ref[1])], [HET_ROWS[0]], [HET_ROWS[1]], [miss_major[0]], [alt_major],  # singletons
            [int(ref[2]), int(ref[3]), int(ref[2])],                                                   # a repeat
            apart,                                                                                     # the skip path
            common,                                                                                    # all linked
            [HET_ROWS[0], miss_major[0], HET_ROWS[1], miss_major[1], alt_major, int(ref[4])],
            [ROW_ALL_MISSING], [ROW_MONO], [ROW_ALL_MISSING, ROW_MONO],
            [],                                                                                        # empty
            [lone], [lone, lone],                                                                      # no carrier in S
            rng.integers(0, m, 256).tolist(),                                                          # the largest
            [int(ref[5]), common[0]]]                                                                  # (zero weights)
    return [np.array(s, dtype=np.uint32) for s in sets], lone


ZERO_SET = -1  # under random weights every weight of the last set is 0: K = 0, ZERO_VARIANCE


def set_weights(sets, seed):
    """One weight per membership: uniform sizes, one in five negative, a zero and a negative weight in the all-linked
    set, zeros only in the last set."""
    rng = np.random.default_rng(seed)
    w = [rng.uniform(0.25, 25.0, len(s)) * np.where(rng.random(len(s)) < 0.2, -1.0, 1.0) for s in sets]
    w[8][1], w[8][2] = 0.0, -3.5
    w[ZERO_SET][:] = 0.0
    return np.concatenate(w)


def phenotype(f, lone, k, case_rate, seed):
    """(y, Z) over the raw samples: ~case_rate cases, ~3 % without a phenotype, none for the carriers of `lone`."""
    import glm_score_oracle as O
    rng = np.random.default_rng(seed)
    Z = rng.normal(size=(k, f.n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]
    if k == 0 and case_rate == 0.2:
        y = f.y.copy()  # rare_codes' own phenotype, which its enriched rows follow
        y[rng.random(f.n) < 0.03] = NAN
    else:
        y = O.pheno(rng, f.n, Z, case_rate=case_rate)
    y[f.codes[lone] != 0] = NAN
    # the first het-majority row has few entries: without a case among them and without covariates its score can
    # cancel to 0.0 exactly, which is a state of its own (q == 0)
    y[np.flatnonzero(f.codes[HET_ROWS[0]] == 2)[0]] = 1.0
    return y, Z


def expected(f, forms, sets, weights, y, Z, mask=None):
    """The oracle's (row, eigenvalues) per set; y, Z over the output samples, mask: the subset over the raw samples."""
    K = _oracle()
    codes = f.codes if mask is None else f.codes[:, mask]
    nul = K.Null(y, Z)
    out, pos = [], 0
    for members in sets:
        w = np.ones(len(members)) if weights is None else weights[pos:pos + len(members)]
        pos += len(members)
        out.append(K.oracle_row(codes, forms, members, w, nul))
    return out


def _close(got, want, scale, ctx):
    assert abs(got - want) <= REL * scale + 1e-300, ctx


def check(L, rows, lam, exp, off, ctx=None):
    assert len(rows) == len(exp)
    for s, (e, elam) in enumerate(exp):
        g = rows[s]
        c = (ctx, s, e, g)
        assert L.GLM_ERRCODES[g["errcode"]] == e["errcode"], c
        assert g["obs_ct"] == e["obs_ct"] and g["n_carriers"] == e["n_carriers"], c
        assert g["p_state"] == e["p_state"] and g["n_lambda"] == e["n_lambda"], c
        assert not g["pad"].any(), c
        se = 0.0 if math.isnan(e["se"]) else e["se"]
        for key in ("q", "beta", "se", "stat", "p", "lambda_sum", "lambda_max"):
            if math.isnan(e[key]):
                assert math.isnan(g[key]), (key, c)
            else:
                # check_rows' scale: beta relative to |beta| + SE, the statistic to |stat| + 1, the others to the value
                _close(g[key], e[key], abs(e[key]) + (se if key == "beta" else 1.0 if key == "stat" else 0.0), (key, c))
        mine = lam[int(off[s]):int(off[s + 1])]
        if elam is None:
            assert np.isnan(mine).all() and math.isnan(g["p_skat"]), c
            continue
        assert np.abs(mine - elam).max() <= 1e-9 * elam[0], c
        assert g["lambda_max"] == mine[0], c
        # the p-value is the exported function's, of the returned numbers; and the oracle's to 1e-6
        p, state = L.skat_p_from_lambda(g["q"], mine[:g["n_lambda"]], return_state=True)
        assert state == g["p_state"], c
        if math.isnan(e["p_skat"]):
            assert math.isnan(g["p_skat"]) and math.isnan(p), c
        else:
            assert g["p_skat"] == p, c
            assert abs(g["p_skat"] - e["p_skat"]) <= 1e-6 * e["p_skat"], c


PARITY = [(0, 0.2, False), (2, 0.2, True), (20, 0.2, True), (2, 0.02, True), (0, 0.02, False), (2, 0.2, False)]


def _parity(L, f, k, case_rate, weighted, shape="all", max_minors=None):
    sets, lone = set_list(f.codes, f.n)
    off, vidx = _csr(sets)
    w = set_weights(sets, 100 * f.n + k) if weighted else None
    y_raw, z_raw = phenotype(f, lone, k, case_rate, 37 * f.n + k + int(1000 * case_rate))
    mask = SS.shapes(f.n)[shape]
    y, Z = y_raw[mask], np.ascontiguousarray(z_raw[:, mask])
    decided = 0
    for max_minor in max_minors or (0, f.n):
        sp, forms = f.sparse(max_minor)
        if max_minor == 0:
            assert forms.dense[sets[8]].any()  # the all-linked set holds a dense-form member
        ss = None if shape == "all" else sp.subset(mask)
        try:
            rows, lam = sp.skat_sparse(y, off, vidx, w, Z if k else None, subset=ss, return_lambda=True)
        finally:
            if ss is not None:
                ss.close()
        exp = expected(f, forms, sets, w, y, Z, None if shape == "all" else mask)
        check(L, rows, lam, exp, off, ctx=(f.n, k, case_rate, weighted, shape, max_minor))
        codes = [e["errcode"] for e, _ in exp]
        assert codes[13] == "CONST_ALLELE" and codes[14] == codes[15] == "CONST_ALLELE"
        assert codes[10] == codes[11] == codes[12] == "CONST_ALLELE"
        if weighted and codes[0] is None:
            assert codes[ZERO_SET] == "ZERO_VARIANCE"
        decided += sum(c is None for c in codes)
    return decided


# ---- on the GPU --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k,case_rate,weighted", PARITY)
def test_parity_with_the_oracle(gpu_lib, files, k, case_rate, weighted):
    decided = _parity(gpu_lib, files(SS.N_SMALL), k, case_rate, weighted)
    assert decided >= 2 * 9


@pytest.mark.gpu
def test_parity_with_the_oracle_at_a_wide_sample_count(gpu_lib, files):
    assert _parity(gpu_lib, files(SS.N_WIDE), 2, 0.2, True, max_minors=(0,)) >= 9


# every padded covariate width of kGlmWidths at its exact value and one above the bucket below it
# (test_glm_widths_chunks.WIDTHS: no case above has k = 1)
WIDTHS = [1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 20]
WIDTHS_N = 4099
# 12 of set_list's sets: singletons of a hom-ref, a het, a missing and a hom-alt majority, the repeat, the skip path,
# all linked, the mixed majorities, all missing, no carrier in S, the largest, (zero weights)
WIDTH_SETS = (0, 2, 4, 5, 6, 7, 8, 9, 10, 14, 16, 17)


def width_case(codes, n, k):
    """(sets, weights) of the width cases: set_list's and set_weights' draws, the 12 sets of WIDTH_SETS."""
    all_sets, lone = set_list(codes, n)
    w_all = set_weights(all_sets, 100 * n + k)
    off_all, _ = _csr(all_sets)
    sets = [all_sets[i] for i in WIDTH_SETS]
    w = np.concatenate([w_all[int(off_all[i]):int(off_all[i + 1])] for i in WIDTH_SETS])
    return sets, w, lone


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_instantiated_width(gpu_lib, files, k):
    """The kernel's template <int KP> for every width GlmPadCovar returns, at k = KP and one above the width below:
    the parity test's oracle and check on 12 weighted sets, every row held sparse."""
    f = files(WIDTHS_N)
    sets, w, lone = width_case(f.codes, f.n, k)
    off, vidx = _csr(sets)
    y, Z = phenotype(f, lone, k, 0.2, 37 * f.n + k + 200)
    sp, forms = f.sparse(f.n)
    rows, lam = sp.skat_sparse(y, off, vidx, w, Z, return_lambda=True)
    exp = expected(f, forms, sets, w, y, Z)
    check(gpu_lib, rows, lam, exp, off, ctx=k)
    codes = [e["errcode"] for e, _ in exp]
    print(f"k={k}: {codes}")
    assert codes[8] == codes[9] == "CONST_ALLELE" and codes[11] == "ZERO_VARIANCE"
    assert sum(c is None for c in codes) >= 8 and codes[7] is None  # the mixed-majority set is decided


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["word_block", "stride4"])
def test_parity_under_a_sample_subset(gpu_lib, files, shape):
    assert _parity(gpu_lib, files(SS.N_SMALL), 2, 0.2, True, shape=shape) >= 2 * 5


@pytest.mark.gpu
@pytest.mark.parametrize("shape,text", [("first", "no cases or no controls"), ("empty", "subset is empty")])
def test_subsets_without_a_case_and_a_control_are_refused(gpu_lib, files, shape, text):
    f = files(SS.N_SMALL)
    sets, lone = set_list(f.codes, f.n)
    off, vidx = _csr(sets)
    mask = SS.shapes(f.n)[shape]
    sp, _ = f.sparse(0)
    ss = sp.subset(mask)
    with pytest.raises(ValueError, match=text):
        sp.skat_sparse(np.ones(int(mask.sum())), off, vidx, subset=ss)
    ss.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2])
def test_one_variant_sets_are_score_test_rows(gpu_lib, files, k):
    L = gpu_lib
    f = files(SS.N_SMALL)
    y, Z = phenotype(f, set_list(f.codes, f.n)[1], k, 0.2, 5 + k)
    no_missing = np.flatnonzero(~((f.codes == 3) & ~np.isnan(y)[None, :]).any(axis=1))
    assert len(no_missing) > 20
    off, vidx = _csr([np.array([v], dtype=np.uint32) for v in no_missing])
    fitted = 0
    for max_minor in (0, f.n):
        sp, _ = f.sparse(max_minor)
        want = sp.glm_score_sparse(y, Z if k else None)
        for weights in (None, np.ones(len(vidx))):
            rows = sp.skat_sparse(y, off, vidx, weights, Z if k else None)
            for s, v in enumerate(no_missing):
                g, c = rows[s], (k, max_minor, v)
                if want["errcode"][v] is not None:
                    # no missing call: the score test's "every called value equal" is "no entry in S"
                    assert want["errcode"][v] != "CONST_ALLELE" or L.GLM_ERRCODES[g["errcode"]] == "CONST_ALLELE", c
                    continue
                assert g["errcode"] == 0 and g["p_state"] == L.SKAT_P_EXACT and g["n_lambda"] == 1, c
                se = want["se"][v]
                _close(g["beta"], want["beta"][v], abs(want["beta"][v]) + se, c)
                _close(g["se"], se, se, c)
                _close(g["stat"], want["stat"][v], abs(want["stat"][v]) + 1.0, c)
                _close(g["p_skat"], want["p"][v], want["p"][v], c)
                fitted += 1
    assert fitted >= 4 * 5  # (two forms, weights None and 1.0) x at least five fitted variants


def _bytes(rows, lam, off):
    return [rows[s].tobytes() + lam[int(off[s]):int(off[s + 1])].tobytes() for s in range(len(rows))]


@pytest.mark.gpu
def test_a_set_does_not_depend_on_the_call_the_budget_or_the_window(gpu_lib, files):
    L = gpu_lib
    f = files(SS.N_SMALL)
    k = 2
    sets, lone = set_list(f.codes, f.n)
    off, vidx = _csr(sets)
    w = set_weights(sets, 9)
    y, Z = phenotype(f, lone, k, 0.2, 44)
    r_off, r_vidx = _csr(sets[::-1])
    r_w = np.concatenate([w[int(off[s]):int(off[s + 1])] for s in range(len(sets))][::-1])
    results = {}
    for max_minor in (0, f.n):
        sp, _ = f.sparse(max_minor)
        rows, lam = sp.skat_sparse(y, off, vidx, w, Z, return_lambda=True)
        results[max_minor] = (rows, lam)
        want = _bytes(rows, lam, off)
        assert len(set(want)) >= 12
        for budget in (None, "1"):  # the default: every set in one launch; the minimum: one vector, a set per launch
            with pytest.MonkeyPatch.context() as mp:
                if budget:
                    mp.setenv(SCRATCH_ENV, budget)
                assert _bytes(*sp.skat_sparse(y, off, vidx, w, Z, return_lambda=True), off) == want, (max_minor, budget)
                rev = _bytes(*sp.skat_sparse(y, r_off, r_vidx, r_w, Z, return_lambda=True), r_off)
                assert rev == want[::-1], (max_minor, budget, "reversed")
                for s in range(len(sets)):
                    ws = w[int(off[s]):int(off[s + 1])]
                    o1 = np.array([0, len(sets[s])])
                    alone = _bytes(*sp.skat_sparse(y, o1, sets[s], ws, Z, return_lambda=True), o1)
                    assert alone == want[s:s + 1], (max_minor, budget, s)
        other, _ = f.sparse(max_minor, window=41)
        assert _bytes(*other.skat_sparse(y, off, vidx, w, Z, return_lambda=True), off) == want, (max_minor, "window")
        # without lambda_out the rows are the same
        assert [r.tobytes() for r in sp.skat_sparse(y, off, vidx, w, Z)] == [r.tobytes() for r in rows]
    # other base codes: to rounding
    (ra, la), (rb, lb) = results[0], results[f.n]
    for s in range(len(sets)):
        a, b, c = ra[s], rb[s], (s, ra[s], rb[s])
        for key in ("errcode", "obs_ct", "n_lambda", "p_state"):
            assert a[key] == b[key], (key, c)
        if a["errcode"]:
            continue
        se = 0.0 if math.isnan(a["se"]) else a["se"]
        for key in ("q", "p_skat", "beta", "se", "stat", "p", "lambda_sum", "lambda_max"):
            if math.isnan(a[key]):
                assert math.isnan(b[key]), (key, c)
            else:
                _close(b[key], a[key], abs(a[key]) + (se if key == "beta" else 1.0 if key == "stat" else 0.0), (key, c))
        la_s, lb_s = la[int(off[s]):int(off[s + 1])], lb[int(off[s]):int(off[s + 1])]
        assert np.abs(la_s - lb_s).max() <= 1e-9 * la_s[0], c


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched_and_the_library_usable(gpu_lib):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    group = L.Dataset.open_sharded(path, [0, 0])
    sp = L.Dataset.open(path, sparse=True)
    n, m = sp.n_samples, sp.v_end - sp.v_begin
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    good_off = np.array([0, 2, 3], dtype=np.uint64)
    good_vidx = np.array([1, 0, 2], dtype=np.uint32)
    good_w = np.array([1.0, 2.0, 0.5])
    big_off = np.array([0, 257], dtype=np.uint64)
    big_vidx = (np.arange(257) % m).astype(np.uint32)
    y_two = y.copy()
    y_two[1] = 2.0

    def call(ds, off, vidx, w, pheno=y):
        out = np.full(80 * (len(off) - 1), 0xAB, dtype=np.uint8)
        lam = np.full(8 * max(1, len(vidx)), 0xAB, dtype=np.uint8)
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = L.raw().pgh_skat_sparse(ds._h, None, p(pheno), 0, None, len(off) - 1, p(off), p(vidx), p(w), p(out), p(lam), eb)
        return rc, eb.value.decode(), bool((out == 0xAB).all() and (lam == 0xAB).all())

    cases = [
        ("set larger than PGH_SKAT_MAX_SET", (sp, big_off, big_vidx, None)),
        ("weight 2 is not finite", (sp, good_off, good_vidx, np.array([1.0, 2.0, np.inf]))),
        ("set_off[0] must be 0, got 1", (sp, np.array([1, 2, 3], dtype=np.uint64), good_vidx, good_w)),
        ("set_off decreases at set 1", (sp, np.array([0, 2, 1], dtype=np.uint64), good_vidx, good_w)),
        (f"set_vidx[1] = {m} is not below", (sp, good_off, np.array([1, m, 2], dtype=np.uint32), good_w)),
        ("phenotype must be 0 or 1", (sp, good_off, good_vidx, good_w, y_two)),
        ("no cases or no controls", (sp, good_off, good_vidx, good_w, np.zeros(n))),
        ("sparse-resident", (dense, good_off, good_vidx, good_w)),
        ("one device's dataset", (group, good_off, good_vidx, good_w)),
    ]
    for text, args in cases:
        rc, msg, untouched = call(*args)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
        rc, msg, untouched = call(sp, good_off, good_vidx, good_w)  # the next call is served
        assert rc == L.PGH_OK and not untouched, (text, rc, msg)
    # a set of exactly PGH_SKAT_MAX_SET memberships is served
    rc, msg, untouched = call(sp, np.array([0, 256], dtype=np.uint64), big_vidx[:256], None)
    assert rc == L.PGH_OK and not untouched, msg
    with pytest.raises(ValueError, match="PGH_SKAT_MAX_SET"):
        sp.skat_sparse(y, big_off, big_vidx)
    rows, lam = sp.skat_sparse(y, good_off, good_vidx, good_w, return_lambda=True)
    assert rows.dtype == L.SKAT_ROW_DTYPE and rows.shape == (2,) and lam.shape == (3,) and rows["obs_ct"].tolist() == [n, n]
    for d in (sp, group, dense):
        d.close()
