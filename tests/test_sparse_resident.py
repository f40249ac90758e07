"""Sparse-resident datasets (pgh_open_sparse) and the plinking_sample_counts_sparse route of read_pfile: rows, counts
and per-sample tallies equal the dense dataset's and the oracle's on every record type; entry points that need rows
refuse such a dataset; the shell gives the same rows with the setting on and off."""

import os
import shutil

import numpy as np
import pytest

from conftest import ROOT, data_path

import pgen_writer as W
from tools.sparse_bench import carrier_rows, write_carrier_pfile

NEW_SYMBOLS = ["pgh_open_sparse", "pgh_get_sparse_info", "pgh_sparse_opens_started"]
SPARSE = {"plinking_sample_counts_sparse": True}


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_sparse_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert "pgh_sparse_info" in header and hasattr(lib, "PghSparseInfo")


# ---- C ABI on the device -----------------------------------------------------------------------------------------

def _mask(n, seed):
    return np.random.default_rng(seed).random(n) < 0.6


@pytest.mark.gpu
def test_rare_small_counts_equal_the_oracle(gpu_lib, oracle):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    pg = oracle.Pgen(path)
    for max_minor in (0, pg.N):
        ds = L.Dataset.open(path, sparse=True, max_minor=max_minor)
        sc = ds.sample_counts()
        assert np.array_equal(sc, pg.sample_counts())
        assert sc.sum(0).tolist() == [99217, 1947, 224, 1012]
        assert np.array_equal(ds.counts_range(), pg.counts_range())
        info = ds.sparse_info()
        assert info.sparse_variant_ct + info.dense_variant_ct == pg.M
        assert info.resident_bytes < info.dense_bytes
        if max_minor:
            assert info.dense_variant_ct == 0 and sum(info.base_hist) == pg.M  # every row sparse
        else:
            # the default rule: sparse iff the entries are smaller than the dense row
            minor = np.array([pg.N - np.bincount(pg.raw(v), minlength=4).max() for v in range(pg.M)])
            assert info.sparse_variant_ct == int((4 * minor < ds.info.pitch_bytes).sum())
        assert ds.device_rows is None
        ds.close()


@pytest.mark.gpu
def test_rare_small_through_the_shell_with_one_and_four_threads(gpu_lib, oracle):
    F = pytest.importorskip("plinking_duck_amd.functions")
    pg = oracle.Pgen(data_path("rare_small.pgen"))
    want = pg.sample_counts()
    for threads in (1, 4):
        r = F.query("read_pfile", data_path("rare_small"), orient="sample", genotypes="counts", threads=threads,
                    columns=["IID", "genotypes"], settings=SPARSE)
        got = {iid: (g["hom_ref"], g["het"], g["hom_alt"], g["missing"]) for iid, g in r.rows}
        assert [got[f"S{i}"] for i in range(pg.N)] == [tuple(int(x) for x in row) for row in want]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 4099, 70_000])
def test_every_record_type(gpu_lib, oracle, tmp_path, monkeypatch, n):
    L = gpu_lib
    rng = np.random.default_rng(n)
    m = 600
    geno = W.rare_matrix(m, n, rng)
    kinds = W.choose_kinds(geno, rng)
    path = str(tmp_path / "rare.pgen")
    W.write_pgen(path, geno, kinds)
    pg = oracle.Pgen(path)
    dense = L.Dataset.open(path)
    rows = dense.copy_rows_to_host(0, m)
    mask = _mask(n, n + 1)
    want_sc = pg.sample_counts()
    assert np.array_equal(dense.sample_counts(), want_sc)
    # several windows per open, so that parts are concatenated and windows start after LD bases
    monkeypatch.setenv("PGH_SPARSE_WINDOW_BYTES", str(97 * dense.info.pitch_bytes))
    lists = np.sort(rng.choice(m, 77, replace=False)).astype(np.uint32)
    for max_minor in (0, 1, n):
        ds = L.Dataset.open(path, sparse=True, max_minor=max_minor)
        info = ds.sparse_info()
        assert info.sparse_variant_ct + info.dense_variant_ct == m
        if max_minor == n:
            assert info.dense_variant_ct == 0
            assert info.base_hist[2] > 0 and info.base_hist[3] > 0  # hom-alt- and missing-majority rows
        if max_minor == 0:
            assert info.resident_bytes <= info.dense_bytes + 12 * m + 8
        assert np.array_equal(ds.copy_rows_to_host(0, m), rows)
        assert np.array_equal(ds.counts_range(), pg.counts_range())
        assert np.array_equal(ds.counts_range(123, 456), dense.counts_range(123, 456))
        assert np.array_equal(ds.sample_counts(), want_sc)
        assert np.array_equal(ds.sample_counts(vidx=lists), dense.sample_counts(vidx=lists))
        assert np.array_equal(ds.sample_counts(40, 333), dense.sample_counts(40, 333))
        ss, ss_d = ds.subset(mask), dense.subset(mask)
        assert np.array_equal(ds.counts_range(subset=ss), dense.counts_range(subset=ss_d))
        assert np.array_equal(ds.counts_range(subset=ss), pg.counts_range(include=mask))
        assert np.array_equal(ds.sample_counts(subset=ss), pg.sample_counts(include=mask))
        assert np.array_equal(ds.sample_counts(vidx=lists, subset=ss), dense.sample_counts(vidx=lists, subset=ss_d))
        ss.close()
        ss_d.close()
        ds.close()
    # a range that starts after an LD base
    v0 = next(v for v in range(150, m) if kinds[v] in (2, 3))
    part = L.Dataset.open(path, sparse=True, variant_begin=v0, variant_end=min(m, v0 + 150))
    assert np.array_equal(part.copy_rows_to_host(v0, part.v_end), rows[v0:part.v_end])
    assert np.array_equal(part.sample_counts(), dense.sample_counts(v0, part.v_end))
    assert np.array_equal(part.counts_range(), pg.counts_range(v0, part.v_end))
    part.close()
    dense.close()


@pytest.mark.gpu
def test_wide_rare_rows(gpu_lib, tmp_path):
    L = gpu_lib
    m, n = 2_000, 500_000
    prefix = str(tmp_path / "wide")
    write_carrier_pfile(prefix, m, n, carrier_rows(m, n, 0.001, 5))
    dense = L.Dataset.open(prefix + ".pgen")
    sp = L.Dataset.open(prefix + ".pgen", sparse=True)
    info = sp.sparse_info()
    assert info.dense_variant_ct == 0 and info.resident_bytes <= info.dense_bytes
    assert np.array_equal(sp.sample_counts(), dense.sample_counts())
    assert np.array_equal(sp.counts_range(), dense.counts_range())
    mask = _mask(n, 9)
    ss, ss_d = sp.subset(mask), dense.subset(mask)
    assert np.array_equal(sp.sample_counts(100, 1500, subset=ss), dense.sample_counts(100, 1500, subset=ss_d))
    ss.close()
    ss_d.close()
    sp.close()
    dense.close()


@pytest.mark.gpu
def test_entry_points_that_need_rows_refuse_a_sparse_dataset(gpu_lib):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    ds = L.Dataset.open(path, sparse=True)
    n, m = ds.n_samples, ds.info.variant_end
    vidx = np.arange(8, dtype=np.uint32)
    calls = [lambda: ds.unpack_range(0, 8),
             lambda: ds.score(vidx, np.ones(8)),
             lambda: ds.ld_pairs(vidx[:4], vidx[4:]),
             lambda: ds.missing_per_sample(),
             lambda: ds.unpack_samples(vidx),
             lambda: ds.dosage_sums(0, 8),
             lambda: ds.pca(vidx, np.zeros(8), np.ones(8), 2, np.ones((n, 4)) / n),
             lambda: L.TallyPass(ds),
             lambda: ds.glm(np.arange(n, dtype=np.float64) % 2, model="linear", v_begin=0, v_end=8),
             lambda: ds.reader()]
    for call in calls:
        with pytest.raises(ValueError, match="dense-resident"):
            call()
    with pytest.raises(ValueError, match="dense-resident"):
        L.Dataset.group([ds])
    assert ds._h  # the refused group did not take the dataset over
    assert np.array_equal(ds.counts_range(0, m)[:, 0] + ds.counts_range(0, m)[:, 1:].sum(1), np.full(m, n))
    with pytest.raises(ValueError):
        L.Dataset.open(path).sparse_info()
    ds.close()


# ---- the shell ---------------------------------------------------------------------------------------------------

def _copy_pfile(src_prefix, dst_prefix):
    for ext in (".pgen", ".pvar", ".psam"):
        shutil.copy(src_prefix + ext, dst_prefix + ext)


@pytest.mark.gpu
def test_shell_rows_equal_with_and_without_the_setting(gpu_lib, tmp_path):
    L = gpu_lib
    F = pytest.importorskip("plinking_duck_amd.functions")
    rs = str(tmp_path / "rare_small")
    _copy_pfile(data_path("rare_small"), rs)
    cases = [dict(), dict(af_range={"min": 0.0, "max": 0.01}), dict(variants=["v3", "v77", "v200", "v399"]),
             dict(region="1:50-250"), dict(samples=["S3", "S100", "S7", "S255"]), dict(include_genotypes=["hom_alt"]),
             dict(ac_range={"min": 1}, samples=list(range(0, 256, 3)))]
    before = L.sparse_opens_started()
    for i, kw in enumerate(cases):
        for g in ("counts", "stats"):
            a = F.query("read_pfile", rs, orient="sample", genotypes=g, columns=["IID", "genotypes"], threads=3, **kw)
            b = F.query("read_pfile", rs, orient="sample", genotypes=g, columns=["IID", "genotypes"], threads=3,
                        settings=SPARSE, **kw)
            assert len(a) > 0 or "include_genotypes" in kw
            assert sorted(a.rows, key=str) == sorted(b.rows, key=str), (kw, g)
            # opened once for this file, cached after that; never without the setting
            assert L.sparse_opens_started() == before + 1
    shards = []
    for k in (1, 2, 3):
        shards.append(str(tmp_path / f"shard{k}"))
        _copy_pfile(data_path(f"shard{k}"), shards[-1])
    a = F.query("read_pfile", shards, orient="sample", genotypes="counts", columns=["IID", "genotypes"])
    assert L.sparse_opens_started() == before + 1
    b = F.query("read_pfile", shards, orient="sample", genotypes="counts", columns=["IID", "genotypes"], settings=SPARSE)
    assert L.sparse_opens_started() == before + 4  # one per source
    assert sorted(a.rows, key=str) == sorted(b.rows, key=str)
    # other orients and modes do not take the route
    F.query("read_pfile", rs, orient="sample", genotypes="array", columns=["IID", "genotypes"], settings=SPARSE,
            samples=["S1"])
    F.query("read_pfile", rs, columns=["ID"], settings=SPARSE)
    assert L.sparse_opens_started() == before + 4


@pytest.mark.gpu
def test_shell_serves_from_the_sparse_form_when_the_dense_form_streams(gpu_lib, tmp_path, monkeypatch):
    L = gpu_lib
    F = pytest.importorskip("plinking_duck_amd.functions")
    m, n = 600, 4_099
    prefix = str(tmp_path / "rare_budget")
    write_carrier_pfile(prefix, m, n, carrier_rows(m, n, 0.002, 7))
    # 200 KB: the dense rows (600 x 1,152 B) stream window by window, the carriers (a few tens of KB) fit
    monkeypatch.setenv("PLINKING_HBM_CACHE_GB", "0.0002")
    want = F.query("read_pfile", prefix, orient="sample", genotypes="counts", columns=["IID", "genotypes"],
                   region="1:20-580", samples=list(range(0, n, 7)), threads=3)
    before = L.sparse_opens_started()
    got = F.query("read_pfile", prefix, orient="sample", genotypes="counts", columns=["IID", "genotypes"],
                  region="1:20-580", samples=list(range(0, n, 7)), threads=3, settings=SPARSE)
    assert L.sparse_opens_started() == before + 1
    assert sorted(got.rows, key=str) == sorted(want.rows, key=str)
