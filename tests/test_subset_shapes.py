"""Every entry point that takes a pgh_subset, under the structured masks of tests/subset_shapes.py.

One test function per family, parametrised over (N, mask).  The reference of every output is the operation in NumPy
on the physically subsetted matrix (subset_shapes.py and the yardsticks it borrows from the family's own test file);
integer outputs are compared with np.array_equal, floating outputs with the tolerance the family's own test uses
against the same reference (each is named where it is used).  Under `all` the integer outputs must also equal the
call without a subset bit for bit; under `empty` every entry point answers as include/pgenhip.h states next to
pgh_subset_create; a fit on five samples or fewer is pinned to the status the GLM oracles give it.

Exclusions, and nothing else: the pair matrices at N = 16,451 run only under masks of at most 300 samples (the full
square is gigabytes); plink_pca runs only under masks of at least 127 samples (and is refused under `empty`)."""

import ctypes as C
import math

import numpy as np
import pytest

import subset_shapes as SS

CASES = SS.cases()
IDS = [f"{n}-{name}" for n, name in CASES]
GROUP_SHAPES = ("first", "last_word", "word_block", "stride64", "empty")
PAIR_MAX_WIDE = 300   # pair matrices at N_WIDE: masks of at most this many samples
PCA_MIN = 127         # plink_pca: masks of at least this many samples
DEGENERATE_MAX = 5    # a fit with two covariates on this many samples or fewer is pinned to its refusal
EMPTY_MESSAGE = "sample subset is empty"


# ---- the catalogue itself (no GPU) -------------------------------------------------------------------------------

def _catalogue(n):
    """name -> (n_out, non-zero include words, full include words), written out independently of shapes()."""
    w = (n + 63) // 64
    every = list(range(w))
    odd = n // 128  # the word of all_but_one's dropped sample 64 (n // 128) + 31
    out = {
        "all": (n, every, every),
        "first": (1, [0], []),
        "last": (1, [w - 1], []),
        "ends": (2, [0, w - 1], []),
        "all_but_one": (n - 1, every, [i for i in every if i != odd]),
        "last_word": (n % 64, [w - 1], [w - 1]),
        "word_block": (128, [1, 2], [1, 2]),
        "tile_plus_one": (129, [0, 1, 2], [1]),
        "tile_minus_one": (127, [0, 1, 2], [1]),
        "stride64": (n // 64, list(range(n // 64)), []),
        "empty": (0, [], []),
    }
    if n == SS.N_SMALL:
        out["stride4"] = (250, every, [])
    else:
        out["stride4"] = (4112, every[:-1], [])  # samples 16448..16450 hold no s % 4 == 3
        out["tile_edges"] = (5, [127, 128, 255, 256, 257], [])
        out["third_tile"] = (67, [256, 257], [256, 257])
    return out


WIDE_EMPTY_TILES = {
    "all": [], "first": [1, 2], "last": [0, 1], "ends": [1], "all_but_one": [], "last_word": [0, 1],
    "word_block": [1, 2], "tile_plus_one": [1, 2], "tile_minus_one": [1, 2], "stride64": [], "stride4": [],
    "tile_edges": [], "third_tile": [0, 1], "empty": [0, 1, 2],
}


def test_the_catalogue_is_what_the_kernels_are_meant_to_see():
    """n_out, the zero and the full include words of every mask at both N, and at the wide N the empty 8192-sample
    tiles: a later edit cannot quietly turn word_block back into a mixed mask."""
    assert (SS.N_SMALL, SS.N_WIDE, SS.M) == (1003, 16451, 130)
    assert SS.N_SMALL == 4 * 250 + 3 == 64 * 15 + 43 and SS.N_WIDE == 64 * 257 + 3 > 2 * SS.SPARSE_TILE
    assert (SS.N_WIDE + 3) // 4 > 4096  # the workgroup forms of pgh_ld_pairs and the long-row paths
    for n in SS.SAMPLE_COUNTS:
        masks = SS.shapes(n)
        want = _catalogue(n)
        assert list(masks) == [name for name in SS.SHAPE_NAMES if name in want]
        assert ("tile_edges" in masks) == ("third_tile" in masks) == (n == SS.N_WIDE)
        n_words = (n + 63) // 64
        for name, mask in masks.items():
            n_out, nonzero, full = want[name]
            assert mask.dtype == bool and mask.shape == (n,)
            assert int(mask.sum()) == n_out, (n, name)
            zero_got, full_got = SS.word_classes(mask)
            assert zero_got == [i for i in range(n_words) if i not in nonzero], (n, name)
            assert full_got == full, (n, name)
            words = SS.include_words(mask)
            assert sum(bin(int(x)).count("1") for x in words) == n_out and len(words) == n_words
            if n == SS.N_WIDE:
                assert SS.empty_tiles(mask) == WIDE_EMPTY_TILES[name], name
        # the masks that sit at a pair tile and next to it, in the ragged last byte, and the dropped mid-word sample
        assert {int(masks[k].sum()) - SS.PAIR_TILE for k in ("word_block", "tile_plus_one", "tile_minus_one")} == {0, 1, -1}
        assert np.flatnonzero(masks["tile_plus_one"])[0] % 4 == 1 and np.flatnonzero(masks["tile_minus_one"])[0] == 3
        assert np.flatnonzero(masks["last_word"])[0] == 64 * (n // 64) and masks["last_word"][-1]
        dropped = int(np.flatnonzero(~masks["all_but_one"])[0])
        assert dropped % 64 == 31 and dropped == 64 * (n // 128) + 31
        assert (np.flatnonzero(masks["stride64"]) % 64 == 63).all() and (np.flatnonzero(masks["stride4"]) % 4 == 3).all()
    assert np.flatnonzero(SS.shapes(SS.N_WIDE)["tile_edges"]).tolist() == [8191, 8192, 16383, 16384, 16450]


# sha256 (first 16 hex digits) of hard_codes(n) and of rare_codes(n)'s codes + phenotype, taken before the generators
# got their m= keyword: the default must go on giving these bytes
MATRIX_DIGESTS = {SS.N_SMALL: ("01f3507bee0546b2", "1e90c5aacda0af4c"), SS.N_WIDE: ("1aa071641715fa01", "7c3fbf90b6e9ac83")}


def test_the_matrices_hold_the_made_rows():
    import hashlib

    for n in SS.SAMPLE_COUNTS:
        codes = SS.hard_codes(n)
        assert codes.shape == (SS.M, n) and codes.max() == 3
        rare_bytes = b"".join(a.tobytes() for a in SS.rare_codes(n))
        assert (hashlib.sha256(codes.tobytes()).hexdigest()[:16],
                hashlib.sha256(rare_bytes).hexdigest()[:16]) == MATRIX_DIGESTS[n], n
        assert (codes[SS.ROW_ALL_MISSING] == 3).all() and (codes[SS.ROW_MONO] == 0).all()
        block = SS.shapes(n)["word_block"]
        assert (codes[SS.ROW_BLOCK][block] == 0).all() and (codes[SS.ROW_BLOCK][~block] != 0).sum() > 100
        rest = np.delete(codes, [SS.ROW_ALL_MISSING, SS.ROW_MONO, SS.ROW_BLOCK], axis=0)
        assert 0.07 < (rest == 3).mean() < 0.09
        gone = SS.nan_samples(n)
        for name, mask in SS.shapes(n).items():
            if mask.sum() <= DEGENERATE_MAX:
                assert (mask & ~gone).sum() < 2 + 2 + 1, name  # fewer observations than parameters + 1
        if n == SS.N_SMALL:  # the BLAS planes are test_ld_prune's and test_ld_scores' integer ones
            from test_ld_prune import brute_prune, brute_sums, windows
            from test_ld_scores import brute_scores

            sub = codes[:, SS.shapes(n)["tile_plus_one"]]
            planes = SS.ld_planes(sub)
            assert planes.dtype == np.int64 and np.array_equal(planes, brute_sums(sub))
            win_end = windows(SS.M, 50)
            assert np.array_equal(SS.ld_prune_ref(planes, sub, win_end, 0.2137, 1e-12), brute_prune(sub, win_end, 0.2137))
            for a, b in zip(SS.ld_scores_ref(planes, sub, win_end, True), brute_scores(sub, win_end, True)):
                assert np.array_equal(a, b)
        rare, y = SS.rare_codes(n)
        assert rare.shape == (SS.M, n) and set(np.unique(y)) == {0.0, 1.0}
        assert {int(np.bincount(r, minlength=4).argmax()) for r in rare} == {0, 1, 2, 3}


# ---- datasets and references, built once per module ---------------------------------------------------------------

class _Hard:
    """The hardcall matrix of one N as a .pgen of every record type, resident."""

    def __init__(self, L, tmp, n):
        self.L, self.n = L, n
        self.codes = SS.hard_codes(n)
        self.path = str(tmp / f"hard_{n}.pgen")
        SS.W.write_pgen(self.path, self.codes, SS.W.choose_kinds(self.codes, np.random.default_rng(n)))
        self.ds = L.Dataset.open(self.path)
        self.masks = SS.shapes(n)
        self.z = SS.covariates(n)
        self.y_lin = SS.linear_phenotypes(n, self.z)
        self.y_bin = SS.binary_phenotypes(n, self.z)
        self._subsets, self._group = {}, None

    def subset(self, name, ds=None):
        ds = self.ds if ds is None else ds
        key = (id(ds), name)
        if key not in self._subsets:
            self._subsets[key] = ds.subset(self.masks[name])
        return self._subsets[key]

    def group(self):
        if self._group is None:
            cut = 57
            self._group = self.L.Dataset.group([self.L.Dataset.open(self.path, variant_begin=0, variant_end=cut),
                                                self.L.Dataset.open(self.path, variant_begin=cut, variant_end=SS.M)])
            assert self._group.shard_count == 2
        return self._group


class _Dose:
    """A dosage- and phase-bearing file from the writer (tests/test_dosage_tracks.py's generator)."""

    def __init__(self, L, orc, tmp, n):
        from test_dosage_tracks import make_dosage_file

        self.n = n
        self.path = str(tmp / f"dose_{n}.pgen")
        self.codes, self.dos, self.dkinds, self.want = make_dosage_file(self.path, SS.M, n, 300 + n, True)
        self.ds = L.Dataset.open(self.path)
        self.pg = orc.Pgen(self.path)  # the phase tracks are random bits of the writer's: the oracle reads them back
        assert self.pg.has_dosage and self.pg.has_phase and {0, 0x20, 0x40, 0x60} == set(self.dkinds)
        self.masks = SS.shapes(n)
        self._subsets = {}

    def subset(self, name):
        if name not in self._subsets:
            self._subsets[name] = self.ds.subset(self.masks[name])
        return self._subsets[name]


class _Rare:
    """pgen_writer.rare_matrix rows, opened dense and sparse (the default rule, and every row held sparse)."""

    def __init__(self, L, tmp, n):
        self.L, self.n = L, n
        self.codes, y = SS.rare_codes(n)
        self.path = str(tmp / f"rare_{n}.pgen")
        SS.W.write_pgen(self.path, self.codes, SS.W.choose_kinds(self.codes, np.random.default_rng(7 * n)))
        self.dense = L.Dataset.open(self.path)
        self.pitch = self.dense.info.pitch_bytes
        self.forms = {}
        for mm in (0, n):
            with pytest.MonkeyPatch.context() as mp:  # several windows per open, as the sparse tests do
                mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(97 * self.pitch))
                self.forms[mm] = L.Dataset.open(self.path, sparse=True, max_minor=mm)
        info = {mm: sp.sparse_info() for mm, sp in self.forms.items()}
        assert info[n].dense_variant_ct == 0 and all(info[n].base_hist[b] > 0 for b in range(4))
        assert info[0].dense_variant_ct > 0 and info[0].sparse_variant_ct > 0
        self.masks = SS.shapes(n)
        self.z = SS.covariates(n, seed=9)
        self.y_lin = SS.linear_phenotypes(n, self.z)[0]
        self.y_bin = np.where(SS.nan_samples(n), np.nan, y)
        self.x = SS.values(self.codes)
        self._subsets = {}

    def subset(self, name, ds):
        key = (id(ds), name)
        if key not in self._subsets:
            self._subsets[key] = ds.subset(self.masks[name])
        return self._subsets[key]


class _World:
    def __init__(self, L, orc, tmp):
        self.L, self.orc, self.tmp = L, orc, tmp
        self._made = {}

    def _get(self, kind, n, make):
        if (kind, n) not in self._made:
            self._made[(kind, n)] = make()
        return self._made[(kind, n)]

    def hard(self, n):
        return self._get("hard", n, lambda: _Hard(self.L, self.tmp, n))

    def dose(self, n):
        return self._get("dose", n, lambda: _Dose(self.L, self.orc, self.tmp, n))

    def rare(self, n):
        return self._get("rare", n, lambda: _Rare(self.L, self.tmp, n))


@pytest.fixture(scope="module")
def world(gpu_lib, oracle, tmp_path_factory):
    return _World(gpu_lib, oracle, tmp_path_factory.mktemp("subset_shapes"))


def _refused_as_empty(L, call):
    with pytest.raises(L.PghArgError, match=EMPTY_MESSAGE) as info:
        call()
    assert info.value.code == L.PGH_ERR_ARG


def _same_ints(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


# ---- counts and tallies ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", CASES, ids=IDS)
def test_counts_and_tallies(gpu_lib, world, n, shape):
    L = gpu_lib
    h = world.hard(n)
    mask, ss = h.masks[shape], h.subset(shape)
    n_out = int(mask.sum())
    assert ss.size == n_out
    sub = h.codes[:, mask]
    counts, per_sample = SS.counts_ref(sub), SS.sample_counts_ref(sub)
    a, b = 17, 101
    assert _same_ints(h.ds.counts_range(subset=ss), counts)
    assert _same_ints(h.ds.counts_range(a, b, subset=ss), counts[a:b])
    assert _same_ints(h.ds.missing_per_sample(subset=ss), per_sample[:, 3])
    assert _same_ints(h.ds.missing_per_sample(a, b, subset=ss), SS.sample_counts_ref(sub[a:b])[:, 3])
    t = L.TallyPass(h.ds, products=L.TALLY_COUNTS | L.TALLY_SAMPLE_MISSING | L.TALLY_HWE, subset=ss)
    assert _same_ints(t.counts(), counts)
    assert _same_ints(t.sample_missing(), per_sample[:, 3])
    # test_tally_pass.py's bound between the pass's exact test and hwe_lnp_batch of the same counts
    assert np.allclose(t.hwe_lnp(False), L.hwe_lnp_batch(counts, False), rtol=0, atol=1e-12)
    t.close()
    assert _same_ints(h.ds.sample_counts(subset=ss), per_sample)
    assert _same_ints(h.ds.sample_counts(a, b, subset=ss), SS.sample_counts_ref(sub[a:b]))
    pick = np.array([129, 0, 5, 64, 3, 4, 96, 97, 31], dtype=np.uint32)
    assert _same_ints(h.ds.sample_counts(vidx=pick, subset=ss), SS.sample_counts_ref(sub[pick]))
    if shape == "all":
        assert _same_ints(h.ds.counts_range(subset=ss), h.ds.counts_range())
        assert _same_ints(h.ds.missing_per_sample(subset=ss), h.ds.missing_per_sample())
        assert _same_ints(h.ds.sample_counts(subset=ss), h.ds.sample_counts())
    if shape == "empty":
        assert not counts.any() and per_sample.shape == (0, 4)


# ---- unpack ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", CASES, ids=IDS)
def test_unpack_and_reader(gpu_lib, world, n, shape):
    h = world.hard(n)
    mask, ss = h.masks[shape], h.subset(shape)
    n_out = int(mask.sum())
    sub = h.codes[:, mask]
    want, valid = SS.calls(sub), SS.validity_ref(sub)
    out, val = h.ds.unpack_range(subset=ss)
    assert _same_ints(out, want) and _same_ints(val, valid)
    out, val = h.ds.unpack_range(40, 99, subset=ss, missing_code=0)
    assert _same_ints(out, np.where(sub[40:99] == 3, 0, sub[40:99]).astype(np.int8)) and _same_ints(val, valid[40:99])
    pick = np.array([129, 0, 5, 64, 65, 3, 4, 96, 97, 31] + list(range(10, 80)), dtype=np.uint32)  # two 64-variant tiles
    assert _same_ints(h.ds.unpack_samples(pick, subset=ss), np.ascontiguousarray(want[pick].T))
    if shape == "all":
        plain_out, plain_val = h.ds.unpack_range()
        assert _same_ints(plain_out, want) and _same_ints(plain_val, valid)
        assert _same_ints(h.ds.unpack_samples(pick), np.ascontiguousarray(want[pick].T))
    # the reader, over the file with dosage and phase tracks
    d = world.dose(n)
    dss = d.subset(shape)
    inc = mask.astype(np.uint8)
    dsub = d.codes[:, mask]
    dcounts = SS.counts_ref(dsub)
    rd = d.ds.reader(dss)
    assert rd.n_out == n_out
    for v in list(range(0, SS.M, 9)) + [SS.M - 1]:
        assert _same_ints(rd.get_counts(v), dcounts[v])
        assert _same_ints(rd.get_2bit(v), SS.packed_2bit_ref(dsub[v]))
        assert _same_ints(rd.get_int8(v), SS.calls(dsub[v]))
        assert _same_ints(rd.get_missingness(v), SS.bits_ref(dsub[v] == 3))
        assert np.array_equal(rd.get_dosage_f64(v), d.want[v][mask])
        g, pp, pi = rd.get_phased(v)
        eg, epp, epi = d.pg.phase(v, inc)
        assert np.array_equal(eg, SS.calls(dsub[v]))  # the oracle's include= form is the physical subset
        assert _same_ints(g, SS.packed_2bit_ref(dsub[v]))
        assert np.array_equal(_bits(pp, n_out), epp != 0)
        assert np.array_equal(_bits(pi, n_out) & _bits(pp, n_out), (epi != 0) & (epp != 0))
    rd.close()


# ---- dosage ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", CASES, ids=IDS)
def test_dosage_entry_points(gpu_lib, world, n, shape):
    d = world.dose(n)
    mask, ss = d.masks[shape], d.subset(shape)
    want = d.want[:, mask]
    moments = SS.dosage_moments_ref(want)
    pick = np.array([129, 0, 5, 64, 65, 3, 4, 96, 97, 31] + list(range(10, 80)), dtype=np.uint32)
    assert _same_ints(d.ds.dosage_sums(subset=ss), moments)
    assert _same_ints(d.ds.dosage_sums(17, 101, subset=ss), moments[17:101])
    assert _same_ints(d.ds.dosage_sums(vidx=pick, subset=ss), moments[pick])
    assert np.array_equal(d.ds.dosage_unpack(subset=ss), want)
    assert np.array_equal(d.ds.dosage_unpack(vidx=pick, subset=ss), want[pick])
    assert np.array_equal(d.ds.dosage_unpack_samples(pick, subset=ss), want[pick].T)
    if shape == "all":
        assert _same_ints(d.ds.dosage_sums(subset=ss), d.ds.dosage_sums())
        assert d.ds.dosage_unpack(subset=ss).tobytes() == d.ds.dosage_unpack().tobytes()
    if shape == "empty":
        assert not moments.any() and d.ds.dosage_unpack(subset=ss).shape == (SS.M, 0)


# ---- score -------------------------------------------------------------------------------------------------------

SCORE_REL = 1e-6  # test_gpu_parity.REL, as test_score_matches_oracle applies it below
SCORE_MODES = (("default", "SCORE_MEAN_IMPUTE"), ("no_mean_imputation", "SCORE_NO_MEAN_IMPUTATION"),
               ("center", "SCORE_CENTER"))


def _score_inputs(ncols):
    rng = np.random.default_rng(17 + ncols)
    vidx = np.union1d(np.sort(rng.choice(SS.M, size=100, replace=False)),
                      [SS.ROW_ALL_MISSING, SS.ROW_MONO, SS.ROW_BLOCK]).astype(np.uint32)
    w = rng.standard_normal((len(vidx), ncols))
    if ncols > 1:
        w[:, ncols - 1] = 1.0  # a unit column: it comes out as the dosage sum, bit for bit
    flip = (rng.random(len(vidx)) < 0.3).astype(np.uint8)
    return vidx, w, flip


def _check_score(got, want, w, dosage_sum=True):
    """test_gpu_parity.test_score_matches_oracle's comparison."""
    (s, d, ac), (es, ed, eac) = got, want
    assert s.shape == es.shape and _same_ints(ac, eac)
    scale = np.abs(w).sum(axis=0) * 2.0  # magnitude of the terms being summed
    assert np.all(np.abs(s - es) <= SCORE_REL * np.maximum(np.abs(es), 1e-9 * scale))
    if dosage_sum:
        assert d.shape == ed.shape and np.allclose(d, ed, rtol=SCORE_REL, atol=1e-9)
    else:
        assert d is None


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", CASES, ids=IDS)
def test_score(gpu_lib, world, n, shape):
    import torch

    L, orc = gpu_lib, world.orc
    h = world.hard(n)
    mask, ss = h.masks[shape], h.subset(shape)
    n_out = int(mask.sum())
    sub = h.codes[:, mask]
    pg = SS.MatrixPgen(SS.values(sub))
    counts = SS.counts_ref(sub)
    for ncols in (1, 16):
        vidx, w, flip = _score_inputs(ncols)
        for mode, const in SCORE_MODES:
            code = getattr(L, const)
            want = orc.score(pg, vidx, w, flip=flip, mode=mode)
            got = h.ds.score(vidx, w, flip=flip, mode=code, subset=ss)
            _check_score(got, want, w)
            _check_score(h.ds.score(vidx, w, flip=flip, mode=code, subset=ss, want_dosage_sum=False), want, w, False)
            _check_score(h.ds.score(vidx, w, flip=flip, mode=code, subset=ss, counts=counts[vidx]), want, w)
            if ncols > 1 and code != L.SCORE_CENTER:
                assert got[0][:, ncols - 1].tobytes() == got[1].tobytes()
            if shape == "all":
                plain = h.ds.score(vidx, w, flip=flip, mode=code)
                assert _same_ints(got[2], plain[2])
                if ncols > 1 and code != L.SCORE_CENTER:  # the unit-weight dosage sum is bit-reproducible
                    assert got[1].tobytes() == plain[1].tobytes()
            if shape == "empty":
                assert got[0].shape == (0, ncols) and got[1].shape == (0,) and got[2].shape == (0,)
        # a kept plan, run twice: its outputs are per raw sample, the kept ones are the subset's
        code = L.SCORE_MEAN_IMPUTE
        want = orc.score(pg, vidx, w, flip=flip, mode="default")
        plan = h.ds.score_plan(vidx, w, flip, code, ss)
        for _ in range(2):
            d_score = torch.full((n, ncols), 7.0, dtype=torch.float64, device="cuda")
            d_dos = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
            d_ac = torch.full((n,), 7, dtype=torch.int32, device="cuda")
            plan.run_dev(d_score.data_ptr(), d_dos.data_ptr(), d_ac.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            raw = (d_score.cpu().numpy(), d_dos.cpu().numpy(), d_ac.cpu().numpy().astype(np.uint32))
            _check_score(tuple(x[mask] for x in raw), want, w)
            if n_out == 0:
                assert not raw[0].any() and not raw[1].any() and not raw[2].any()
        plan.close()


# ---- LD ----------------------------------------------------------------------------------------------------------

LD_WINDOW, LD_R2 = 50, 0.2137  # no band pair of any mask sits on the threshold (the reference asserts it)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", CASES, ids=IDS)
def test_ld(gpu_lib, world, n, shape):
    from test_ld_prune import windows

    L = gpu_lib
    h = world.hard(n)
    mask, ss = h.masks[shape], h.subset(shape)
    sub = h.codes[:, mask]
    planes = SS.ld_planes(sub)  # (6, M, M) int64
    assert planes.max(initial=0) < 2 ** 32
    a, b = SS.ld_pair_list(n)
    pairs = h.ds.ld_pairs(a, b, subset=ss)
    assert _same_ints(pairs, np.stack([planes[p][a, b] for p in range(6)], axis=1).astype(np.uint32))
    if shape == "all":
        assert _same_ints(pairs, h.ds.ld_pairs(a, b))
    win_end = windows(SS.M, LD_WINDOW)
    if shape == "empty":
        assert not pairs.any()
        _refused_as_empty(L, lambda: h.ds.ld_window_sums(subset=ss))
        _refused_as_empty(L, lambda: h.ds.ld_prune(LD_R2, window=LD_WINDOW, subset=ss))
        _refused_as_empty(L, lambda: h.ds.ld_scores(window=LD_WINDOW, subset=ss))
        return
    assert _same_ints(h.ds.ld_window_sums(subset=ss), planes.astype(np.uint32))
    rect = h.ds.ld_window_sums(vidx=np.arange(2, SS.M, dtype=np.uint32), subset=ss, a_range=(90, 128), b_range=(1, 127))
    assert _same_ints(rect, planes[:, 92:130, 3:129].astype(np.uint32))
    keep = h.ds.ld_prune(LD_R2, window=LD_WINDOW, subset=ss)
    assert np.array_equal(keep, SS.ld_prune_ref(planes, sub, win_end, LD_R2, near=1e-12))
    for unbiased in (False, True):  # test_ld_scores.check_against_brute: partners equal, scores within its summation bound
        score, partners = h.ds.ld_scores(window=LD_WINDOW, unbiased=unbiased, want_counts=True, subset=ss)
        exp, bound, exp_n = SS.ld_scores_ref(planes, sub, win_end, unbiased)
        assert score.dtype == np.float64 and _same_ints(partners, exp_n)
        err = np.abs(score - exp)
        assert (err <= bound).all(), (unbiased, int(np.argmax(err - bound)), float(err.max()))
    if shape == "all":
        assert _same_ints(h.ds.ld_window_sums(subset=ss), h.ds.ld_window_sums())
        assert np.array_equal(keep, h.ds.ld_prune(LD_R2, window=LD_WINDOW))


# ---- pair matrices -----------------------------------------------------------------------------------------------

def _king_table_ref(counts):
    """The pairs i < j of brute_counts' planes with test_king.py_kinship's formula, vectorised: the integers are far
    below 2^53, so the float64 quotient is the correctly rounded int / int."""
    i, j = np.triu_indices(counts.shape[1], k=1)
    nsnp, hethet, ibs0, h1, h2 = (counts[p][i, j].astype(np.int64) for p in range(5))
    den = 4 * (hethet + np.minimum(h1, h2))
    with np.errstate(all="ignore"):
        kin = 0.5 - (4 * ibs0 + h1 + h2).astype(np.float64) / den.astype(np.float64)
    kin[den == 0] = np.nan
    return i, j, nsnp, hethet, ibs0, h1, h2, kin


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", CASES, ids=IDS)
def test_pair_matrices(gpu_lib, world, n, shape):
    from test_grm import Yardstick, check
    from test_king import brute_counts, brute_table, check_table

    L = gpu_lib
    h = world.hard(n)
    mask, ss = h.masks[shape], h.subset(shape)
    n_out = int(mask.sum())
    if n == SS.N_WIDE and n_out > PAIR_MAX_WIDE:
        assert shape in ("all", "all_but_one", "stride4")  # the stated exclusion: the full square is gigabytes
        return
    if shape == "empty":
        _refused_as_empty(L, lambda: h.ds.king_counts(subset=ss))
        _refused_as_empty(L, lambda: h.ds.king_table(subset=ss))
        _refused_as_empty(L, lambda: h.ds.king_table_capped(0.0, 0, subset=ss))
        for flag in (False, True):
            _refused_as_empty(L, lambda: h.ds.grm(subset=ss, meanimpute=flag))
        return
    sub = h.codes[:, mask]
    counts = brute_counts(sub)
    got = h.ds.king_counts(subset=ss)
    assert _same_ints(got, counts)
    if n_out > SS.PAIR_TILE:  # a rectangle that starts inside a tile and ends in the ragged last one
        rect = h.ds.king_counts(subset=ss, i_range=(5, n_out), j_range=(0, SS.PAIR_TILE))
        assert _same_ints(rect, counts[:, 5:, :SS.PAIR_TILE])
    pick = np.arange(1, SS.M, 2, dtype=np.uint32)
    assert _same_ints(h.ds.king_counts(vidx=pick, subset=ss), brute_counts(sub[pick]))
    table = h.ds.king_table(subset=ss)
    i, j, nsnp, hethet, ibs0, h1, h2, kin = _king_table_ref(counts)
    assert len(table) == len(i) == n_out * (n_out - 1) // 2
    for key, want in (("i", i), ("j", j), ("nsnp", nsnp), ("hethet", hethet), ("ibs0", ibs0), ("het1hom2", h1),
                      ("het2hom1", h2)):
        assert np.array_equal(table[key].astype(np.int64), want), key
    assert table["kinship"].tobytes() == kin.tobytes()
    cut = 0.0884
    filtered = h.ds.king_table(cut, subset=ss)
    with np.errstate(invalid="ignore"):
        passing = kin >= cut
    assert np.array_equal(filtered["i"], i[passing]) and np.array_equal(filtered["j"], j[passing])
    assert filtered["kinship"].tobytes() == kin[passing].tobytes()
    if n_out <= SS.PAIR_TILE + 1:  # and test_king's own loop in Python integers
        check_table(table, brute_table(sub, -math.inf))
    if shape == "all":
        assert _same_ints(got, h.ds.king_counts())
    y = Yardstick(sub)
    for flag in (False, True):
        rel, nobs, n_used = h.ds.grm(subset=ss, meanimpute=flag)
        check(rel, nobs, n_used, y, meanimpute=flag)  # test_grm's derived bound
        if shape == "all":
            assert _same_ints(nobs, h.ds.grm(meanimpute=flag)[1])
    if n_out > SS.PAIR_TILE:
        rows, cols = np.arange(5, n_out), np.arange(0, SS.PAIR_TILE)
        rel, nobs, n_used = h.ds.grm(subset=ss, i_range=(5, n_out), j_range=(0, SS.PAIR_TILE))
        check(rel, nobs, n_used, y, rows=rows, cols=cols)


# ---- plink_pca ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", CASES, ids=IDS)
def test_pca(gpu_lib, world, n, shape):
    L, orc = gpu_lib, world.orc
    h = world.hard(n)
    mask, ss = h.masks[shape], h.subset(shape)
    n_out = int(mask.sum())
    n_pcs = 2
    if shape == "empty":
        keep, center, inv = SS.freq_norm(SS.counts_ref(h.codes))
        _refused_as_empty(L, lambda: h.ds.pca(keep, center, inv, n_pcs, np.zeros((0, 2 * n_pcs)), subset=ss))
        return
    if n_out < PCA_MIN:
        assert shape in ("first", "last", "ends", "last_word", "tile_edges", "third_tile") or \
            (shape == "stride64" and n == SS.N_SMALL)  # the stated exclusion
        return
    sub = h.codes[:, mask]
    g1 = orc.fill_g1(n_out, 2 * n_pcs)
    ev, vecs, keep, spectrum = SS.pca_ref(sub, n_pcs, g1)
    assert len(keep) > 100 and spectrum[0] > 1.1 * spectrum[1] and spectrum[1] > 1.1 * spectrum[2]  # separated
    _, center, inv = SS.freq_norm(SS.counts_ref(sub))
    got_ev, got_vecs = h.ds.pca(keep, center, inv, n_pcs, g1, subset=ss)
    # test_gpu_parity.test_pca_matches_oracle_on_wide_rows: eigenvalues within 1e-6, an orthonormal basis within 1e-8,
    # the eigenvectors within 1e-5 (here each up to its sign: the two components are separated)
    assert np.allclose(got_ev, ev, rtol=1e-6)
    assert np.allclose(got_vecs.T @ got_vecs, np.eye(n_pcs), atol=1e-8)
    assert np.allclose(got_vecs @ got_vecs.T @ vecs, vecs, atol=1e-5)
    for c in range(n_pcs):
        sign = np.sign(np.dot(got_vecs[:, c], vecs[:, c]))
        assert np.allclose(got_vecs[:, c], sign * vecs[:, c], atol=1e-5), c
    if shape == "all":
        plain_ev, plain_vecs = h.ds.pca(keep, center, inv, n_pcs, g1)
        assert np.allclose(plain_ev, ev, rtol=1e-6)


# ---- GLM, dense --------------------------------------------------------------------------------------------------

def _rel_at_the_sample_count_boundary(rel):
    """test_glm_widths_chunks.test_sample_count_boundary's tolerance of SE, statistic and p for a fit with few
    residual degrees of freedom: rel grows with tss / rss."""
    return lambda e: rel * max(1.0, e.get("tss", 1.0) / max(e.get("rss", 1.0), 1e-300))


def _pinned_as_refused(out, n_rows):
    assert list(out["errcode"]) == ["TOO_FEW_SAMPLES"] * n_rows
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.isnan(out[key]).all(), key
    assert not out["firth"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", CASES, ids=IDS)
def test_glm_dense(gpu_lib, world, n, shape):
    orc = pytest.importorskip("glm_oracle")
    L = gpu_lib
    h = world.hard(n)
    mask, ss = h.masks[shape], h.subset(shape)
    n_out = int(mask.sum())
    z = np.ascontiguousarray(h.z[:, mask])
    y_lin, y_bin = np.ascontiguousarray(h.y_lin[:, mask]), np.ascontiguousarray(h.y_bin[:, mask])
    if shape == "empty":
        _refused_as_empty(L, lambda: h.ds.glm(y_lin[0], z, model="linear", subset=ss))
        _refused_as_empty(L, lambda: h.ds.glm(y_bin[0], z, model="logistic", subset=ss))
        _refused_as_empty(L, lambda: h.ds.glm_multi(y_lin, z, model="linear", subset=ss))
        return
    x = SS.values(h.codes[:, mask])
    lin = h.ds.glm(y_lin[0], z, model="linear", subset=ss)
    log = h.ds.glm(y_bin[0], z, model="logistic", subset=ss)
    multi = h.ds.glm_multi(y_lin, z, model="linear", subset=ss)
    multi_log = h.ds.glm_multi(y_bin, z, model="logistic", subset=ss)
    assert multi["beta"].shape == (SS.M, 3)
    # test_glm_gpu / test_glm_widths_chunks: 1e-9 for the linear fit, 1e-6 for the logistic one, on check_rows' scale;
    # below PCA_MIN samples a fit has few residual degrees of freedom, which test_sample_count_boundary allows for
    rel_of = _rel_at_the_sample_count_boundary(1e-9) if n_out < PCA_MIN else None
    # every row of the single calls; of glm_multi's columns every third row once the oracle costs (n_out > 2000)
    some = None if n_out <= 2000 else sorted(set(range(0, SS.M, 3)) | {SS.ROW_ALL_MISSING, SS.ROW_MONO, SS.ROW_BLOCK})
    fitted_lin = orc.check_rows(lin, x, y_lin[0], z, "linear", rel=1e-9, rel_of=rel_of)
    fitted_log = orc.check_rows(log, x, y_bin[0], z, "logistic", rel=1e-6)
    for p in range(3):
        col = {key: v[:, p] for key, v in multi.items()}
        orc.check_rows(col, x, y_lin[p], z, "linear", rel=1e-9, rel_of=rel_of, idx=some)
    orc.check_rows({key: v[:, 2] for key, v in multi_log.items()}, x, y_bin[2], z, "logistic", rel=1e-6, idx=some)
    if n_out <= DEGENERATE_MAX:  # first, last, ends, tile_edges, and the three samples of the wide N's last word
        _pinned_as_refused(lin, SS.M)
        _pinned_as_refused(log, SS.M)
        for p in range(3):
            _pinned_as_refused({key: v[:, p] for key, v in multi.items()}, SS.M)
    elif n_out >= PCA_MIN:  # the numeric comparison happened
        assert fitted_lin >= 100 and fitted_log >= 60, (fitted_lin, fitted_log)
    assert lin["errcode"][SS.ROW_ALL_MISSING] == "TOO_FEW_SAMPLES"
    if n_out > DEGENERATE_MAX + 3:
        assert lin["errcode"][SS.ROW_MONO] == "CONST_ALLELE"
    if shape == "word_block":
        assert lin["errcode"][SS.ROW_BLOCK] == "CONST_ALLELE"
    if shape == "all":
        plain = h.ds.glm(y_lin[0], z, model="linear")
        assert plain["obs_ct"].tolist() == lin["obs_ct"].tolist() and list(plain["errcode"]) == list(lin["errcode"])


# ---- sparse-resident ---------------------------------------------------------------------------------------------

def _burden_sets(rng, major):
    sets = [rng.integers(0, SS.M, size).astype(np.uint32) for size in (1, 2, 3, 5, 8, 13, 21, 34, 60)]
    mixed = [7, int(np.flatnonzero(major == 2)[0]), int(np.flatnonzero(major == 3)[0]), 8, int(np.flatnonzero(major == 0)[5])]
    sets.append(np.array(mixed + mixed[:2], dtype=np.uint32))  # every base code in one set, two members twice
    sets.append(np.array([7], dtype=np.uint32))
    return sets


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", CASES, ids=IDS)
def test_sparse_resident(gpu_lib, world, n, shape):
    glm = pytest.importorskip("glm_oracle")
    import glm_score_oracle as O
    import glm_spa_oracle as S
    from test_burden_sparse import _check as burden_check, _csr, _expected as burden_expected, _Forms
    from test_glm_score_sparse_spa import CUTOFF, TOL
    from test_score_sparse import _Case, _within

    L = gpu_lib
    r = world.rare(n)
    mask = r.masks[shape]
    n_out = int(mask.sum())
    sub = r.codes[:, mask]
    x = r.x[:, mask]
    z = np.ascontiguousarray(r.z[:, mask])
    y_lin, y_bin = np.ascontiguousarray(r.y_lin[mask]), np.ascontiguousarray(r.y_bin[mask])
    counts, per_sample = SS.counts_ref(sub), SS.sample_counts_ref(sub)
    pick = np.array([129, 0, 5, 64, 7, 8, 96, 97, 31], dtype=np.uint32)
    rng = np.random.default_rng(31)
    sets = _burden_sets(rng, _Forms(r.codes, n, r.pitch).major)
    off, set_vidx = _csr(sets)
    bw = rng.uniform(0.25, 25.0, len(set_vidx)) * np.where(rng.random(len(set_vidx)) < 0.2, -1.0, 1.0)
    s_vidx = np.union1d(np.arange(0, SS.M, 2), [7, 8]).astype(np.uint32)
    s_flip = (rng.random(len(s_vidx)) < 0.4).astype(np.uint8)
    s_w = rng.normal(size=(len(s_vidx), 3)) * np.array([1.0, 1e3, 1e-3])[None, :]
    have = ~np.isnan(y_bin)
    one_class = not ((y_bin[have] == 1.0).any() and (y_bin[have] == 0.0).any())
    nul = None if (n_out == 0 or one_class) else O.Null(y_bin, z)
    score_cases = {}
    if shape != "empty":
        for mode in (L.SCORE_MEAN_IMPUTE, L.SCORE_NO_MEAN_IMPUTATION, L.SCORE_CENTER):
            for cols in ((0,), (0, 1, 2)):
                score_cases[(mode, cols)] = _Case(L, r.codes, s_vidx, np.ascontiguousarray(s_w[:, list(cols)]), s_flip,
                                                  mode, mask)
    for mm, sp in r.forms.items():
        ss = r.subset(shape, sp)
        assert ss.size == n_out
        ctx = (n, shape, mm)
        # counts from the carrier lists
        assert _same_ints(sp.counts_range(subset=ss), counts), ctx
        assert _same_ints(sp.counts_range(17, 101, subset=ss), counts[17:101]), ctx
        assert _same_ints(sp.sample_counts(subset=ss), per_sample), ctx
        assert _same_ints(sp.sample_counts(17, 101, subset=ss), SS.sample_counts_ref(sub[17:101])), ctx
        assert _same_ints(sp.sample_counts(vidx=pick, subset=ss), SS.sample_counts_ref(sub[pick])), ctx
        if shape == "all":
            assert _same_ints(sp.counts_range(subset=ss), sp.counts_range())
            assert _same_ints(sp.sample_counts(subset=ss), sp.sample_counts())
        # plink_score from the carrier lists: test_score_sparse's oracle and its bound of 1e-12 A
        for mode in (L.SCORE_MEAN_IMPUTE, L.SCORE_NO_MEAN_IMPUTATION, L.SCORE_CENTER):
            for cols in ((0,), (0, 1, 2)):
                w = np.ascontiguousarray(s_w[:, list(cols)])
                score, dos, ac = sp.score_sparse(s_vidx, w, s_flip, mode, ss)
                if shape == "empty":
                    assert score.shape == (0, len(cols)) and dos.shape == (0,) and ac.shape == (0,)
                    continue
                case = score_cases[(mode, cols)]
                assert score.shape == case.score.shape and _same_ints(ac, case.allele), ctx
                _within(score, case.score, case.A[None, :], 1e-12, ctx + ("score", mode))
                _within(dos, case.dosage, np.float64(case.A_dos), 1e-12, ctx + ("dosage", mode))
                if shape == "all":  # bit-reproducible
                    plain = sp.score_sparse(s_vidx, w, s_flip, mode)
                    assert all(a.tobytes() == b.tobytes() for a, b in zip((score, dos, ac), plain)), ctx
        if shape == "empty":
            _refused_as_empty(L, lambda: sp.glm_sparse(y_lin, z, subset=ss))
            _refused_as_empty(L, lambda: sp.glm_score_sparse(y_bin, z, subset=ss))
            _refused_as_empty(L, lambda: sp.glm_score_sparse_spa(y_bin, z, subset=ss))
            _refused_as_empty(L, lambda: sp.burden_sparse(y_lin, off, set_vidx, bw, z, subset=ss))
            continue
        # the linear fit: test_glm_sparse's 1e-9 against glm_oracle
        lin = sp.glm_sparse(y_lin, z, subset=ss)
        rel_of = _rel_at_the_sample_count_boundary(1e-9) if n_out < PCA_MIN else None
        fitted = glm.check_rows(lin, x, y_lin, z, "linear", rel=1e-9, rel_of=rel_of)
        # the burden test: test_burden_sparse's oracle and 1e-9
        forms = _Forms(r.codes, mm, r.pitch)
        burden = sp.burden_sparse(y_lin, off, set_vidx, bw, z, subset=ss)
        expected = burden_expected(r.codes, forms, sets, bw, y_lin, z, keep=mask)
        burden_check(L, burden, expected, rel=1e-9, ctx=ctx)
        if n_out <= DEGENERATE_MAX:
            _pinned_as_refused(lin, SS.M)
            assert {e["errcode"] for e in expected} == {"TOO_FEW_SAMPLES"}
        elif n_out >= PCA_MIN:
            assert fitted >= 40 and sum(e["errcode"] is None for e in expected) >= 8, (fitted, ctx)
        # the score test and its saddlepoint: 1e-9 (test_glm_score_sparse.REL) and test_glm_score_sparse_spa.TOL
        if one_class:
            assert n_out <= DEGENERATE_MAX
            for call in (sp.glm_score_sparse, sp.glm_score_sparse_spa):
                with pytest.raises(L.PghArgError, match="no cases or no controls"):
                    call(y_bin, z, subset=ss)
            continue
        score_rows = sp.glm_score_sparse(y_bin, z, subset=ss)
        fitted, worst = O.check_rows(score_rows, x, nul, rel=1e-9)
        spa = sp.glm_score_sparse_spa(y_bin, z, cutoff=CUTOFF, subset=ss)
        for key in ("beta", "se", "stat", "p", "a1_freq"):
            assert np.array_equal(spa[key], score_rows[key], equal_nan=True), (key, ctx)
        assert list(spa["errcode"]) == list(score_rows["errcode"]) and spa["obs_ct"].tolist() == score_rows["obs_ct"].tolist()
        row_forms = [S.row_form(r.codes[i], mm) for i in range(SS.M)]  # the form comes from all raw samples
        seen = S.check_spa(spa, x, sub, nul, row_forms, CUTOFF, TOL)
        print(f"{ctx}: score test {fitted} fitted, worst {worst:.3g}; saddlepoint {seen['applied']} applied, "
              f"{seen['failed']} failed, worst {seen['worst']:.3g}")
        if n_out <= DEGENERATE_MAX:
            _pinned_as_refused(score_rows, SS.M)
            assert np.isnan(spa["p_spa"]).all() and not spa["spa_state"].any()
        elif n_out >= PCA_MIN:
            assert nul.status is None and fitted >= 30, (fitted, ctx)


# ---- a shard group of two shards ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", [(n, s) for n in SS.SAMPLE_COUNTS for s in GROUP_SHAPES],
                         ids=[f"{n}-{s}" for n in SS.SAMPLE_COUNTS for s in GROUP_SHAPES])
def test_shard_group(gpu_lib, world, n, shape):
    L, orc = gpu_lib, world.orc
    h = world.hard(n)
    grp = h.group()
    mask = h.masks[shape]
    ss = h.subset(shape, grp)
    n_out = int(mask.sum())
    assert ss.size == n_out
    sub = h.codes[:, mask]
    counts, per_sample = SS.counts_ref(sub), SS.sample_counts_ref(sub)
    a, b = 40, 99  # across the cut at 57
    assert _same_ints(grp.counts_range(subset=ss), counts)
    assert _same_ints(grp.counts_range(a, b, subset=ss), counts[a:b])
    assert _same_ints(grp.missing_per_sample(subset=ss), per_sample[:, 3])
    assert _same_ints(grp.missing_per_sample(a, b, subset=ss), SS.sample_counts_ref(sub[a:b])[:, 3])
    assert _same_ints(grp.sample_counts(subset=ss), per_sample)
    pick = np.array([129, 0, 56, 57, 3, 4, 96], dtype=np.uint32)
    assert _same_ints(grp.sample_counts(vidx=pick, subset=ss), SS.sample_counts_ref(sub[pick]))
    out, val = grp.unpack_range(a, b, subset=ss)
    assert _same_ints(out, SS.calls(sub[a:b])) and _same_ints(val, SS.validity_ref(sub[a:b]))
    t = L.TallyPass(grp, products=L.TALLY_SAMPLE_MISSING, subset=ss)
    assert _same_ints(t.counts(), counts) and _same_ints(t.sample_missing(), per_sample[:, 3])
    t.close()
    pg = SS.MatrixPgen(SS.values(sub))
    for ncols in (1, 16):
        vidx, w, flip = _score_inputs(ncols)
        for mode, const in SCORE_MODES:
            got = grp.score(vidx, w, flip=flip, mode=getattr(L, const), subset=ss)
            _check_score(got, orc.score(pg, vidx, w, flip=flip, mode=mode), w)
            if shape == "empty":
                assert got[0].shape == (0, ncols) and got[2].shape == (0,)


# ---- include bits at and above N ---------------------------------------------------------------------------------

def _raw_subset(L, ds, words):
    handle = C.c_void_p()
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    rc = L.raw().pgh_subset_create(ds._h, words.ctypes.data_as(C.c_void_p), C.byref(handle), eb)
    assert rc == L.PGH_OK, eb.value
    ss = L.Subset.__new__(L.Subset)
    ss._h, ss.ds, ss.size = handle, ds, L.raw().pgh_subset_size(handle)
    return ss


@pytest.mark.gpu
@pytest.mark.parametrize("n", SS.SAMPLE_COUNTS)
def test_include_bits_at_and_above_n_are_ignored(gpu_lib, world, n):
    """A caller who says "everyone" with all-ones words: the subset keeps N samples, and the kernels that walk the
    include words bit by bit (pgh_dosage_sums, the sparse family) give what they give without a subset."""
    L = gpu_lib
    words = np.full((n + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    assert n % 64 and not np.array_equal(words, SS.include_words(np.ones(n, dtype=bool)))
    h, d, r = world.hard(n), world.dose(n), world.rare(n)
    ss = _raw_subset(L, h.ds, words)
    assert ss.size == n
    assert _same_ints(h.ds.counts_range(subset=ss), h.ds.counts_range())
    assert _same_ints(h.ds.counts_range(subset=ss), SS.counts_ref(h.codes))
    ss = _raw_subset(L, d.ds, words)
    assert ss.size == n
    assert _same_ints(d.ds.dosage_sums(subset=ss), d.ds.dosage_sums())
    assert _same_ints(d.ds.dosage_sums(subset=ss), SS.dosage_moments_ref(d.want))
    for mm, sp in r.forms.items():
        ss = _raw_subset(L, sp, words)
        assert ss.size == n
        assert _same_ints(sp.sample_counts(subset=ss), sp.sample_counts()), mm
        assert _same_ints(sp.sample_counts(subset=ss), SS.sample_counts_ref(r.codes)), mm
        assert _same_ints(sp.counts_range(subset=ss), SS.counts_ref(r.codes)), mm
    ss = _raw_subset(L, h.group(), words)
    assert ss.size == n
    assert _same_ints(h.group().counts_range(subset=ss), SS.counts_ref(h.codes))
