"""pgh_burden_sparse / Dataset.burden_sparse: per variant set, the linear fit of the phenotype on the weighted burden
B_i = c_s + d_i of the set's variants, from the entries of a sparse-resident dataset.

The oracle is numpy: d_i by sequential float64 adds in set order over the resident form of each member (base code and
entries; a dense-form member as base 0 with an entry per sample whose code is 1 or 2), which is bit-exact; the
CONST_ALLELE rule, n_nonzero and obs_ct from that d; the estimates from glm_oracle.oracle_row(c_s + d, y, Z, "linear").
errcode, obs_ct and n_nonzero are equal, beta / se / stat / p / mean within 1e-9 relative (the tolerance
tests/test_glm_sparse.py applies to the same solve).  A set's row does not depend on the other sets, on their order,
on the scratch budget or on the window: bit for bit."""

import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, data_path

import pgen_writer as W

NAN = float("nan")
NEW_SYMBOLS = ["pgh_burden_sparse"]
VAL = np.array([0, 1, 2, 0], dtype=np.int64)  # val(code): a missing call contributes nothing
SCRATCH_ENV = "PGH_BURDEN_SCRATCH_BYTES"


def _oracle():
    # glm_oracle needs scipy: only the device tests, which compare against it, skip without it
    return pytest.importorskip("glm_oracle")


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_burden_sparse(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert "} pgh_burden_row;" in header
    assert hasattr(lib.Dataset, "burden_sparse")
    # the struct of the header, field for field: 4 + 1 doubles, two uint32, errcode, 7 bytes of padding
    assert C.sizeof(lib.PghBurdenRow) == 56 == lib.BURDEN_ROW_DTYPE.itemsize
    assert [f[0] for f in lib.PghBurdenRow._fields_] == list(lib.BURDEN_ROW_DTYPE.names)
    for name in lib.BURDEN_ROW_DTYPE.names:
        assert getattr(lib.PghBurdenRow, name).offset == lib.BURDEN_ROW_DTYPE.fields[name][1], name


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
            lib.Dataset.burden_sparse(fake, **kw)


def test_a_null_dataset_is_refused_without_a_device(lib):
    out = np.full(56, 0xAB, dtype=np.uint8)
    eb = C.create_string_buffer(lib.ERRBUF_LEN)
    off = np.array([0, 0], dtype=np.uint64)
    rc = lib.raw().pgh_burden_sparse(None, None, None, 0, None, 1, off.ctypes.data_as(C.c_void_p), None, None,
                                     out.ctypes.data_as(C.c_void_p), eb)
    assert rc == lib.PGH_ERR_ARG and b"null dataset" in eb.value and (out == 0xAB).all()


# ---- the oracle --------------------------------------------------------------------------------------------------

def _csr(sets):
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.uint64)
    vidx = np.concatenate([np.asarray(s, dtype=np.uint32) for s in sets] + [np.zeros(0, np.uint32)])
    return off, vidx.astype(np.uint32)


class _Forms:
    """The resident form of every variant of geno: the base code (the majority, ties to the lower code) and whether
    the row is held in the dense form (4 m >= pitch, or m > max_minor when max_minor > 0)."""

    def __init__(self, geno, max_minor, pitch):
        counts = np.stack([(geno == c).sum(axis=1) for c in range(4)], axis=1)
        self.major = counts.argmax(axis=1)
        self.minor = geno.shape[1] - counts.max(axis=1)
        self.dense = self.minor > max_minor if max_minor else 4 * self.minor >= pitch


def _set_d(geno, forms, members, weights, in_s):
    """c_s and d (one value per raw sample; 0.0 outside in_s) of one set."""
    d = np.zeros(geno.shape[1], dtype=np.float64)
    cs = 0.0
    for v, w in zip(members, weights):
        g = geno[v]
        if forms.dense[v]:
            b, hit = 0, ((g == 1) | (g == 2)) & in_s
        else:
            b = int(forms.major[v])
            hit = (g != b) & in_s
        vb = int(VAL[b])
        cs = cs + float(w) * float(vb)
        d[hit] = d[hit] + float(w) * (VAL[g[hit]] - vb).astype(np.float64)  # one multiply, one add
    return cs, d


def _expected(geno, forms, sets, weights, y, Z, keep=None):
    """One dict per set.  y, Z: per output sample; keep: the subset's mask over the raw samples (None = all)."""
    orc = _oracle()
    n_raw = geno.shape[1]
    keep = np.ones(n_raw, dtype=bool) if keep is None else keep
    in_s = np.zeros(n_raw, dtype=bool)
    in_s[np.flatnonzero(keep)[~np.isnan(y)]] = True
    has_y = ~np.isnan(y)
    n_y, k = int(has_y.sum()), Z.shape[0]
    rows, pos = [], 0
    for members in sets:
        w = np.ones(len(members)) if weights is None else weights[pos:pos + len(members)]
        pos += len(members)
        cs, d_raw = _set_d(geno, forms, members, w, in_s)
        d = d_raw[keep]
        ds = d[has_y]
        row = dict(beta=NAN, se=NAN, stat=NAN, p=NAN, errcode=None, obs_ct=n_y, n_nonzero=int((ds != 0.0).sum()),
                   mean=cs + ds.sum() / n_y if n_y else NAN)
        if n_y < k + 3:
            row["errcode"] = "TOO_FEW_SAMPLES"
        elif ds.min() == ds.max():
            row["errcode"] = "CONST_ALLELE"
        else:
            B = cs + d
            assert not (B[has_y] == -9.0).any()  # the oracle's missing value
            o = orc.oracle_row(B, y, Z, "linear")
            assert o["obs_ct"] == n_y
            for key in ("beta", "se", "stat", "p", "errcode"):
                row[key] = o[key]
        rows.append(row)
    return rows


def _check(L, got, exp, rel=1e-9, ctx=None):
    assert len(got) == len(exp)
    for s, e in enumerate(exp):
        g = got[s]
        c = (ctx, s, e, g)
        assert L.GLM_ERRCODES[g["errcode"]] == e["errcode"], c
        assert g["obs_ct"] == e["obs_ct"] and g["n_nonzero"] == e["n_nonzero"], c
        assert not g["pad"].any(), c
        se = 0.0 if np.isnan(e["se"]) else e["se"]
        for key in ("beta", "se", "stat", "p", "mean"):
            if np.isnan(e[key]):
                assert np.isnan(g[key]), (key, c)
            else:
                # check_rows' scale: beta relative to |beta| + SE, the statistic to |t| + 1, the others to the value
                scale = abs(e[key]) + (se if key == "beta" else 1.0 if key == "stat" else 0.0)
                assert abs(g[key] - e[key]) <= rel * scale + 1e-300, (key, c)


def _covariates(rng, k, n):
    return rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]


def _weights(rng, count):
    w = rng.uniform(0.25, 25.0, count)
    w[rng.random(count) < 0.2] *= -1.0
    return w


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
    """A .pgen of every record type and its calls; sparse() opens it in several windows."""

    def __init__(self, L, tmp, m, n, seed):
        self.L, self.m, self.n = L, m, n
        self.geno, self.kinds = _matrix(m, n, seed)
        self.path = str(tmp / f"rare_{n}.pgen")
        W.write_pgen(self.path, self.geno, self.kinds)
        dense = L.Dataset.open(self.path)
        self.pitch = dense.info.pitch_bytes
        dense.close()

    def sparse(self, max_minor, **kw):
        # several windows per open, so that parts are concatenated and windows start after LD bases
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(97 * self.pitch))
            sp = self.L.Dataset.open(self.path, sparse=True, max_minor=max_minor, **kw)
        return sp, _Forms(self.geno, max_minor, self.pitch)


M_R = 600


@pytest.fixture(scope="module")
def rare_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("burden_sparse")
    return {n: _File(gpu_lib, tmp, M_R, n, n) for n in (257, 4099)}


def _random_sets(rng, count, lo, hi, sizes=(1, 60)):
    """Variants of [lo, hi) in any order, about one membership in six a repeat of an earlier one of its set."""
    sets = []
    for s in range(count):
        size = sizes[0] + s * (sizes[1] - sizes[0]) // max(1, count - 1)
        members = rng.integers(lo, hi, size)
        for j in np.flatnonzero(rng.random(size) < 1 / 6):
            members[j] = members[rng.integers(0, j + 1)]
        sets.append(members.astype(np.uint32))
    return sets


# ---- on the GPU --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("n", [257, 4099])
def test_parity_with_the_oracle_for_every_base_code_and_both_forms(gpu_lib, rare_files, n, k):
    f = rare_files[n]
    rng = np.random.default_rng(1000 * n + k)
    Z = _covariates(rng, k, n)
    y = _oracle()._pheno(rng, n, "linear", Z)
    sets = _random_sets(rng, 40, 0, M_R)
    major = _Forms(f.geno, n, f.pitch).major
    # one set holds het-, hom-alt- and missing-majority rows (and a hom-ref one) together
    mixed = [HET_ROWS[0], int(np.flatnonzero(major == 2)[0]), int(np.flatnonzero(major == 3)[0]), HET_ROWS[1],
             int(np.flatnonzero(major == 0)[5])]
    assert sorted(major[mixed].tolist()) == [0, 1, 1, 2, 3]
    sets[11] = np.array(mixed + mixed[:2], dtype=np.uint32)
    off, vidx = _csr(sets)
    w = _weights(rng, len(vidx))
    for max_minor in (0, 1, n):
        sp, forms = f.sparse(max_minor)
        info = sp.sparse_info()
        assert info.dense_variant_ct == int(forms.dense.sum())
        if max_minor == n:
            assert info.dense_variant_ct == 0 and all(info.base_hist[b] > 0 for b in (1, 2, 3))
        else:
            assert info.dense_variant_ct > 0 and info.sparse_variant_ct > 0
        got = sp.burden_sparse(y, off, vidx, w, Z if k else None)
        _check(gpu_lib, got, _expected(f.geno, forms, sets, w, y, Z), ctx=(n, k, max_minor))
        if max_minor == 1:  # and unweighted
            got = sp.burden_sparse(y, off, vidx, None, Z if k else None)
            _check(gpu_lib, got, _expected(f.geno, forms, sets, None, y, Z), ctx=(n, k, "unweighted"))
        sp.close()


# every padded covariate width of kGlmWidths at its exact value and one above the bucket below it
# (test_glm_widths_chunks.WIDTHS without the k = 1 of the parity test)
WIDTHS = [2, 4, 5, 8, 9, 12, 13, 16, 17, 20]


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_instantiated_width(gpu_lib, rare_files, k):
    """The kernel's template <int KP> for every width GlmPadCovar returns, at k = KP and one above the width below:
    the parity test's draw with 12 sets, its mixed-majority set among them, every row held sparse."""
    n = 4099
    f = rare_files[n]
    rng = np.random.default_rng(1000 * n + k)
    Z = _covariates(rng, k, n)
    y = _oracle()._pheno(rng, n, "linear", Z)
    sets = _random_sets(rng, 12, 0, M_R)
    major = _Forms(f.geno, n, f.pitch).major
    mixed = [HET_ROWS[0], int(np.flatnonzero(major == 2)[0]), int(np.flatnonzero(major == 3)[0]), HET_ROWS[1],
             int(np.flatnonzero(major == 0)[5])]
    assert sorted(major[mixed].tolist()) == [0, 1, 1, 2, 3]
    sets[11] = np.array(mixed + mixed[:2], dtype=np.uint32)
    off, vidx = _csr(sets)
    w = _weights(rng, len(vidx))
    sp, forms = f.sparse(n)
    assert sp.sparse_info().dense_variant_ct == 0
    exp = _expected(f.geno, forms, sets, w, y, Z)
    assert sum(e["errcode"] is None for e in exp) >= 10 and exp[11]["errcode"] is None
    _check(gpu_lib, sp.burden_sparse(y, off, vidx, w, Z), exp, ctx=k)
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 3])
def test_one_variant_sets_are_glm_sparse_rows(gpu_lib, rare_files, k):
    f = rare_files[4099]
    rng = np.random.default_rng(31 + k)
    Z = _covariates(rng, k, f.n)
    y = _oracle()._pheno(rng, f.n, "linear", Z)
    no_missing = np.flatnonzero(~((f.geno == 3) & ~np.isnan(y)[None, :]).any(axis=1))
    assert len(no_missing) > 100 and set(_Forms(f.geno, f.n, f.pitch).major[no_missing]) >= {0, 2}
    sets = [np.array([v], dtype=np.uint32) for v in no_missing]
    off, vidx = _csr(sets)
    for max_minor in (0, f.n):
        sp, forms = f.sparse(max_minor)
        want = sp.glm_sparse(y, Z if k else None)
        for weights in (None, np.ones(len(vidx))):
            got = sp.burden_sparse(y, off, vidx, weights, Z if k else None)
            exp = []
            for s, v in enumerate(no_missing):
                exp.append(dict(beta=want["beta"][v], se=want["se"][v], stat=want["stat"][v], p=want["p"][v],
                                errcode=want["errcode"][v], obs_ct=int(want["obs_ct"][v]),
                                n_nonzero=int(got[s]["n_nonzero"]), mean=2.0 * want["a1_freq"][v]))
            _check(gpu_lib, got, exp, ctx=(k, max_minor))
        assert {None, "CONST_ALLELE"} <= set(want["errcode"][no_missing])
        _check(gpu_lib, got, _expected(f.geno, forms, sets, None, y, Z), ctx=(k, max_minor, "oracle"))
        sp.close()


@pytest.mark.gpu
def test_collisions_and_long_rows(gpu_lib, rare_files, tmp_path):
    n, k = 4099, 3
    f = rare_files[n]
    rng = np.random.default_rng(77)
    # a hom-ref-majority row with about 30 % carriers, beside the file's own rows
    geno = f.geno[:200].copy()
    geno[199] = 0
    carriers = rng.random(n) < 0.3
    geno[199, carriers] = rng.integers(1, 3, carriers.sum(), dtype=np.uint8)
    path = str(tmp_path / "long.pgen")
    W.write_pgen(path, geno, [0] * len(geno))
    sp = gpu_lib.Dataset.open(path, sparse=True, max_minor=n)
    forms = _Forms(geno, n, f.pitch)
    assert sp.sparse_info().dense_variant_ct == 0
    assert forms.major[199] == 0 and forms.minor[199] > 1024
    Z = _covariates(rng, k, n)
    y = _oracle()._pheno(rng, n, "linear", Z)
    entry = geno != forms.major[:, None]
    i0 = int(np.argmax(np.where(np.isnan(y), 0, entry.sum(axis=0))))
    everywhere = np.flatnonzero(entry[:, i0]).astype(np.uint32)
    assert len(everywhere) >= 8
    sets = [everywhere,                                          # one sample carried by every member
            rng.integers(0, 200, 1100).astype(np.uint32),        # more than 1,024 memberships
            np.array([199, 3, 199], dtype=np.uint32),            # a row of more than 1,024 entries, twice
            np.array([HET_ROWS[1]] * 5, dtype=np.uint32),        # the same variant five times
            np.array([199], dtype=np.uint32)]
    off, vidx = _csr(sets)
    w = _weights(rng, len(vidx))
    exp = _expected(geno, forms, sets, w, y, Z)
    assert all(e["errcode"] is None for e in exp)
    for budget in (None, "1"):
        with pytest.MonkeyPatch.context() as mp:
            if budget:
                mp.setenv(SCRATCH_ENV, budget)
            _check(gpu_lib, sp.burden_sparse(y, off, vidx, w, Z), exp, ctx=budget)
    sp.close()


@pytest.mark.gpu
def test_subset_and_missing_phenotypes(gpu_lib, rare_files):
    f = rare_files[4099]
    rng = np.random.default_rng(12)
    keep = np.arange(f.n) % 3 != 2  # every third sample is out
    n, k = int(keep.sum()), 3
    Z = _covariates(rng, k, n)
    y = 0.3 * Z.sum(axis=0) + rng.normal(size=n)
    y[rng.random(n) < 0.1] = NAN
    # a hom-ref-majority variant with a few carriers in the subset: they lose their phenotype
    forms_all = _Forms(f.geno, f.n, f.pitch)
    carried = ((f.geno != 0) & keep[None, :]).sum(axis=1)
    lone = int(np.flatnonzero((forms_all.major == 0) & (carried >= 1) & (carried <= 6))[0])
    raw_of = np.flatnonzero(keep)
    y[np.isin(raw_of, np.flatnonzero(f.geno[lone] != 0))] = NAN
    sets = _random_sets(rng, 24, 0, M_R)
    sets[5] = np.array([lone], dtype=np.uint32)
    sets[6] = np.array([lone, lone], dtype=np.uint32)
    off, vidx = _csr(sets)
    w = _weights(rng, len(vidx))
    for max_minor in (0, f.n):
        sp, forms = f.sparse(max_minor)
        ss = sp.subset(keep)
        got = sp.burden_sparse(y, off, vidx, w, Z, subset=ss)
        exp = _expected(f.geno, forms, sets, w, y, Z, keep=keep)
        _check(gpu_lib, got, exp, ctx=max_minor)
        for s in (5, 6):
            assert exp[s]["errcode"] == "CONST_ALLELE" and exp[s]["n_nonzero"] == 0
        assert sum(e["errcode"] is None for e in exp) >= 20
        other, _ = f.sparse(max_minor)
        with pytest.raises(ValueError, match="different dataset"):
            other.burden_sparse(y, off, vidx, w, Z, subset=ss)
        other.close()
        ss.close()
        sp.close()


def _bytes(rows):
    return [r.tobytes() for r in rows]


@pytest.mark.gpu
def test_a_set_does_not_depend_on_the_call_the_budget_or_the_window(gpu_lib, rare_files):
    f = rare_files[4099]
    rng = np.random.default_rng(44)
    k = 3
    Z = _covariates(rng, k, f.n)
    y = _oracle()._pheno(rng, f.n, "linear", Z)
    v0 = next(v for v in range(150, M_R) if f.kinds[v] in (2, 3))  # a window that starts after an LD base
    v1 = min(M_R, v0 + 150)
    sets = _random_sets(rng, 40, v0, v1)
    off, vidx = _csr(sets)
    w = _weights(rng, len(vidx))
    r_off, r_vidx = _csr(sets[::-1])
    r_w = np.concatenate([w[int(off[s]):int(off[s + 1])] for s in range(len(sets))][::-1])
    for max_minor in (0, f.n):
        sp, forms = f.sparse(max_minor)
        whole = sp.burden_sparse(y, off, vidx, w, Z)
        _check(gpu_lib, whole, _expected(f.geno, forms, sets, w, y, Z), ctx=max_minor)
        want = _bytes(whole)
        assert len(set(want)) > 30
        for budget in (None, "1"):  # the default: a workgroup per set; the minimum: every set through one vector
            with pytest.MonkeyPatch.context() as mp:
                if budget:
                    mp.setenv(SCRATCH_ENV, budget)
                assert _bytes(sp.burden_sparse(y, off, vidx, w, Z)) == want, (max_minor, budget, "again")
                assert _bytes(sp.burden_sparse(y, r_off, r_vidx, r_w, Z)) == want[::-1], (max_minor, budget, "reversed")
                for s in range(len(sets)):
                    ws = w[int(off[s]):int(off[s + 1])]
                    alone = sp.burden_sparse(y, np.array([0, len(sets[s])]), sets[s], ws, Z)
                    assert _bytes(alone) == want[s:s + 1], (max_minor, budget, s)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(41 * f.pitch))
            part = gpu_lib.Dataset.open(f.path, sparse=True, max_minor=max_minor, variant_begin=v0, variant_end=v1)
        assert _bytes(part.burden_sparse(y, off, vidx - np.uint32(v0), w, Z)) == want, (max_minor, "sub-range")
        part.close()
        sp.close()


@pytest.mark.gpu
def test_decisions(gpu_lib, tmp_path):
    L = gpu_lib
    n = 64
    rng = np.random.default_rng(5)
    y = rng.normal(size=n)
    no_pheno = np.array([3, 17, 40])
    y[no_pheno] = NAN
    geno = np.zeros((6, n), dtype=np.uint8)
    geno[0] = rng.binomial(2, 0.2, n)
    geno[1] = 2
    geno[1, no_pheno[:2]] = [0, 1]               # a hom-alt base whose entries have no phenotype
    geno[2] = rng.binomial(2, 0.3, n)
    geno[2, rng.random(n) < 0.1] = 3
    geno[3, no_pheno] = [1, 2, 3]                # carriers without a phenotype only
    geno[4] = rng.binomial(2, 0.1, n)
    geno[5] = 3
    geno[5, rng.random(n) < 0.2] = 1             # a missing-majority row
    path = str(tmp_path / "decisions.pgen")
    W.write_pgen(path, geno, [0] * len(geno))
    sp = L.Dataset.open(path, sparse=True, max_minor=n)
    forms = _Forms(geno, n, 16)
    assert sp.sparse_info().dense_variant_ct == 0 and forms.major.tolist() == [0, 2, 0, 0, 0, 3]
    sets = [np.array([], dtype=np.uint32),       # empty
            np.array([1], dtype=np.uint32),      # base 2, no entry in S: mean = 2 w
            np.array([2, 2], dtype=np.uint32),   # +1 and -1 on the same variant: d == 0 everywhere
            np.array([3], dtype=np.uint32),
            np.array([0, 4], dtype=np.uint32),   # B is the covariate below
            np.array([2, 5, 0], dtype=np.uint32),
            np.array([5], dtype=np.uint32)]
    off, vidx = _csr(sets)
    w = np.array([3.5, 1.0, -1.0, 2.0, 1.0, 2.0, 1.5, -0.75, 4.0, 1.0])
    in_s = ~np.isnan(y)
    cs, d = _set_d(geno, forms, sets[4], [1.0, 2.0], in_s)
    Z = np.stack([cs + d, rng.normal(size=n)])
    got = sp.burden_sparse(y, off, vidx, w, Z)
    assert [L.GLM_ERRCODES[c] for c in got["errcode"]] == ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE",
                                                          "CONST_ALLELE", "SINGULAR_MATRIX", None, None]
    assert got["n_nonzero"][:4].tolist() == [0, 0, 0, 0] and got["obs_ct"].tolist() == [61] * 7
    assert got["mean"][0] == 0.0 and got["mean"][1] == 7.0 and got["mean"][2] == 0.0
    _check(L, got, _expected(geno, forms, sets, w, y, Z))
    # and without covariates
    got0 = sp.burden_sparse(y, off, vidx, w)
    assert [L.GLM_ERRCODES[c] for c in got0["errcode"]] == ["CONST_ALLELE"] * 4 + [None] * 3
    _check(L, got0, _expected(geno, forms, sets, w, y, np.zeros((0, n))))
    # n_y = k + 2: every row is TOO_FEW_SAMPLES, whatever its set
    few = np.full(n, NAN)
    few[[1, 2, 5, 9]] = [0.5, -1.0, 2.0, 0.25]
    got = sp.burden_sparse(few, off, vidx, w, Z)
    assert [L.GLM_ERRCODES[c] for c in got["errcode"]] == ["TOO_FEW_SAMPLES"] * 7 and got["obs_ct"].tolist() == [4] * 7
    _check(L, got, _expected(geno, forms, sets, w, few, Z))
    few[12] = 1.0  # k + 3: enough to decide
    got = sp.burden_sparse(few, off, vidx, w, Z)
    assert "TOO_FEW_SAMPLES" not in [L.GLM_ERRCODES[c] for c in got["errcode"]] and got["obs_ct"].tolist() == [5] * 7
    # no phenotype at all: the mean is undefined too
    got = sp.burden_sparse(np.full(n, NAN), off, vidx, w, Z)
    assert [L.GLM_ERRCODES[c] for c in got["errcode"]] == ["TOO_FEW_SAMPLES"] * 7 and np.isnan(got["mean"]).all()
    sp.close()


@pytest.mark.gpu
def test_refusals_leave_out_untouched_and_the_library_usable(gpu_lib):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    group = L.Dataset.open_sharded(path, [0, 0])
    sp = L.Dataset.open(path, sparse=True)
    other = L.Dataset.open(path, sparse=True)
    ss_other = other.subset(np.ones(other.n_samples, dtype=bool))
    n, m = sp.n_samples, sp.v_end - sp.v_begin
    y = np.arange(n, dtype=np.float64) % 3
    good_off = np.array([0, 2, 3], dtype=np.uint64)
    good_vidx = np.array([1, 0, 2], dtype=np.uint32)
    good_w = np.array([1.0, 2.0, 0.5])
    bad_z = np.zeros((2, n))
    bad_z[1, 5] = np.inf

    def call(ds, off, vidx, w, z=None, n_sets=None, subset=None):
        out = np.full(4, 0xAB, dtype=np.uint8).repeat(14 * 4).view(L.BURDEN_ROW_DTYPE)
        before = out.tobytes()
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = L.raw().pgh_burden_sparse(ds._h, subset._h if subset else None, p(y), 0 if z is None else z.shape[0], p(z),
                                       len(off) - 1 if n_sets is None else n_sets, p(off), p(vidx), p(w), p(out), eb)
        return rc, eb.value.decode(), out.tobytes() == before

    cases = [
        ("sparse-resident", (dense, good_off, good_vidx, good_w), {}),
        ("one device's dataset", (group, good_off, good_vidx, good_w), {}),
        ("at least one set", (sp, good_off, good_vidx, good_w), dict(n_sets=0)),
        ("set_off[0] must be 0, got 1", (sp, np.array([1, 2, 3], dtype=np.uint64), good_vidx, good_w), {}),
        ("set_off decreases at set 1", (sp, np.array([0, 2, 1], dtype=np.uint64), good_vidx, good_w), {}),
        (f"set_vidx[1] = {m} is not below", (sp, good_off, np.array([1, m, 2], dtype=np.uint32), good_w), {}),
        ("weight 2 is not finite", (sp, good_off, good_vidx, np.array([1.0, 2.0, np.inf])), {}),
        ("weight 0 is not finite", (sp, good_off, good_vidx, np.array([NAN, 2.0, 1.0])), {}),
        ("at most 20 covariates", (sp, good_off, good_vidx, good_w), dict(z=np.zeros((21, n)))),
        ("covariate 1 is not finite at sample 5", (sp, good_off, good_vidx, good_w), dict(z=bad_z)),
        ("different dataset", (sp, good_off, good_vidx, good_w), dict(subset=ss_other)),
    ]
    for text, args, kw in cases:
        rc, msg, untouched = call(*args, **kw)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
        # the next call is served
        rc, msg, untouched = call(sp, good_off, good_vidx, good_w)
        assert rc == L.PGH_OK and not untouched, (text, rc, msg)
    # the wrapper raises what the library says, and checks the shapes it has to
    with pytest.raises(ValueError, match="sparse-resident"):
        dense.burden_sparse(y, good_off, good_vidx)
    with pytest.raises(ValueError, match="is not below"):
        sp.burden_sparse(y, good_off, np.array([1, m, 2]))
    with pytest.raises(ValueError, match="at least one set"):
        sp.burden_sparse(y, np.array([0]), np.array([], dtype=np.uint32))
    with pytest.raises(ValueError, match="phenotype"):
        sp.burden_sparse(y[:-1], good_off, good_vidx)
    with pytest.raises(ValueError, match="memberships"):
        sp.burden_sparse(y, good_off, good_vidx[:2])
    with pytest.raises(ValueError, match="weights"):
        sp.burden_sparse(y, good_off, good_vidx, good_w[:2])
    rows = sp.burden_sparse(y, good_off, good_vidx, good_w)
    assert rows.dtype == L.BURDEN_ROW_DTYPE and rows.shape == (2,) and rows["obs_ct"].tolist() == [n, n]
    ss_other.close()
    for d in (other, sp, group, dense):
        d.close()
