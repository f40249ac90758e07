#!/usr/bin/env python3
"""One SHA-256 per case over the result bytes of the GLM family (pgh_glm, pgh_glm_multi, pgh_glm_sparse,
pgh_glm_score_sparse, pgh_glm_score_sparse_spa, pgh_glm_score_sparse_firth, pgh_glm_score_sparse_multi, pgh_glm_score_sparse_multi_spa, pgh_glm_score_sparse_multi_firth, pgh_glm_sparse_multi, pgh_glm_score_multi, pgh_glm_score_multi_dosage, pgh_glm_score_multi_dosage_firth, pgh_glm_score_multi_spa,
pgh_glm_score_multi_firth, pgh_burden_sparse), pgh_score_sparse, and the plink_ld pair sums and sparse counts that share their wave sums: the
paths a change to the family's kernels, host staging, scratch layout or chunk loops can touch.  Two builds of the library
compute the same rows bit for bit exactly when their outputs of this tool are equal line for line; PGENHIP_LIB names
the build (plinking_duck_amd/lib.py).  A case that differs between two runs of ONE build is not deterministic from
run to run and its line says nothing.

The inputs are small seeded files: every record type through tests/pgen_writer.py, carrier lists through
tools/sparse_bench.py, and the library's own synthetic rows for the two shapes that need many variants or samples (a
range past one 16384-variant chunk; 70,001 samples, where 512 MiB of dense dosages split a 2100-variant call).

usage: python tools/glm_family_digest.py [--dir DIR]"""
import argparse
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pgen_writer as W  # noqa: E402
import plinking_duck_amd.lib as L  # noqa: E402
from tools.sparse_bench import carrier_rows, write_carrier_pfile  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dir", default=None, help="where the input files go (default: a temporary directory)")
args = ap.parse_args()
tmp = tempfile.TemporaryDirectory() if args.dir is None else None
out_dir = args.dir or tmp.name
os.makedirs(out_dir, exist_ok=True)


def emit(name, *results, note=""):
    h = hashlib.sha256()
    for r in results:
        if isinstance(r, dict):
            r = [r[key] for key in sorted(r)]
        for a in r if isinstance(r, (list, tuple)) else [r]:
            if a is None:
                h.update(b"none")
            elif a.dtype == object:
                h.update(repr(a.tolist()).encode())
            else:
                h.update(np.ascontiguousarray(a).tobytes())
    print(f"{name} {h.hexdigest()}{note}", flush=True)


def pheno(rng, n, Z, kind="linear", missing=0.03):
    eta = (Z.sum(axis=0) * 0.2 if Z is not None and len(Z) else 0.0) + rng.standard_normal(n)
    y = eta if kind == "linear" else (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    y[rng.random(n) < missing] = np.nan
    return y


def covar(rng, k, n):
    return rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None] if k else None


# ---- dense: pgh_glm and pgh_glm_multi --------------------------------------------------------------------------
rng = np.random.default_rng(20261018)
M, N = 300, 517
geno = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=(M, N), p=[0.6, 0.27, 0.1, 0.03])
geno[5] = 0  # a constant row
dos16 = np.where(rng.random((M, N)) < 0.3, rng.integers(0, 32769, (M, N)), 0xFFFF).astype(np.uint16)
dos_kinds = [int(rng.choice([0, 0x20, 0x40, 0x60])) for _ in range(M)]
plain = os.path.join(out_dir, "plain.pgen")
tracks = os.path.join(out_dir, "tracks.pgen")
W.write_pgen(plain, geno, W.choose_kinds(geno, rng))
W.write_pgen(tracks, geno, W.choose_kinds(geno, rng), dosage=dos16, dosage_kinds=dos_kinds)
ds = L.Dataset.open(plain)
dt = L.Dataset.open(tracks)
assert dt.info.dosage_variant_ct > 0
keep = rng.random(N) < 0.7
ss, st = ds.subset(keep), dt.subset(keep)
n_keep = int(keep.sum())

for k in (0, 3, 20):
    Z = covar(rng, k, N)
    emit(f"glm linear k={k}", ds.glm(pheno(rng, N, Z), Z, model="linear"))
Z2 = covar(rng, 2, N)
emit("glm logistic k=2", ds.glm(pheno(rng, N, Z2, "logistic"), Z2, model="logistic"))
y_sep = (geno[0] > 0).astype(np.float64)  # separated by variant 0's genotype, with a few flips elsewhere
emit("glm firth separated", ds.glm(y_sep, None, model="logistic", firth=True),
     ds.glm(y_sep, None, model="logistic", firth=False))
Zs = covar(rng, 3, n_keep)
emit("glm subset linear k=3", ds.glm(pheno(rng, n_keep, Zs), Zs, model="linear", subset=ss))
emit("glm subset logistic k=3", ds.glm(pheno(rng, n_keep, Zs, "logistic"), Zs, model="logistic", subset=ss))
emit("glm dosage tracks", dt.glm(pheno(rng, N, Z2), Z2, model="linear"),
     dt.glm(pheno(rng, N, Z2, "logistic"), Z2, model="logistic"),
     dt.glm(pheno(rng, n_keep, Zs), Zs, model="linear", subset=st, v_begin=7, v_end=M - 3))


def phenos(rng, n, P, Z, patterns, kind="linear"):
    masks = [rng.random(n) < 0.05 for _ in range(patterns)]
    Y = np.stack([pheno(rng, n, Z, kind, missing=0.0) for _ in range(P)])
    for p in range(P):
        Y[p, masks[p % patterns]] = np.nan
    return Y


Z3 = covar(rng, 3, N)
emit("glm_multi P=7 two patterns", ds.glm_multi(phenos(rng, N, 7, Z3, 2), Z3))
emit("glm_multi P=65", ds.glm_multi(phenos(rng, N, 65, Z3, 1), Z3))
emit("glm_multi subset", ds.glm_multi(phenos(rng, n_keep, 5, Zs, 2), Zs, subset=ss))
emit("glm_multi logistic P=3", ds.glm_multi(phenos(rng, N, 3, Z2, 2, "logistic"), Z2, model="logistic", v_end=40))
emit("glm_multi dosage tracks", dt.glm_multi(phenos(rng, N, 7, Z3, 2), Z3),
     dt.glm_multi(phenos(rng, n_keep, 3, Zs, 1), Zs, subset=st))

# the plink_ld pair sums: a wave per pair on these rows, a workgroup per pair on the 70,001-sample rows below
a, b = rng.integers(0, M, 400), rng.integers(0, M, 400)
emit("ld_pairs short rows", ds.ld_pairs(a, b), ds.ld_pairs(a, b, subset=ss))

# a range past one chunk of 16384 variants, starting inside the resident range
N_L = 203
long_ds = L.Dataset.synth(100, 17100, N_L, 7, 0.02)
Zl = covar(rng, 2, N_L)
emit("glm range past a chunk", long_ds.glm(pheno(rng, N_L, Zl), Zl, model="linear", v_begin=150),
     long_ds.glm(pheno(rng, N_L, Zl, "logistic"), Zl, model="logistic", v_begin=150))
long_ds.close()

# dosage chunks that split: 958 variants of 70,001 samples per 512 MiB of dense dosages
M_D, N_D = 2100, 70001
L.synth_write_dosage_files(os.path.join(out_dir, "dos"), M_D, N_D, 21, 0.02, 0.3)
dd = L.Dataset.open(os.path.join(out_dir, "dos.pgen"))
assert dd.info.dosage_variant_ct > 0
Zd = covar(rng, 2, N_D)
emit("glm dosage chunks split", dd.glm(pheno(rng, N_D, Zd), Zd, model="linear"))
emit("glm_multi dosage chunks split", dd.glm_multi(phenos(rng, N_D, 3, Zd, 2), Zd))
a, b = rng.integers(0, M_D, 200), rng.integers(0, M_D, 200)
emit("ld_pairs long rows", dd.ld_pairs(a, b))
dd.close()

# pgh_glm_score_multi_dosage over the small files above, on draws of its own so that the lines around it keep theirs
rng_t = np.random.default_rng(20261020)
Zt, Zts = covar(rng_t, 3, N), covar(rng_t, 3, n_keep)
Yt = phenos(rng_t, N, 7, Zt, 2, "logistic")
emit("glm_score_multi_dosage tracks P=7 two patterns", dt.glm_score_multi_dosage(Yt, Zt), dt.glm_score_multi_dosage(Yt, None))
emit("glm_score_multi_dosage tracks subset", dt.glm_score_multi_dosage(phenos(rng_t, n_keep, 3, Zts, 1, "logistic"), Zts,
                                                                         subset=st, v_begin=7, v_end=M - 3))
emit("glm_score_multi_dosage no tracks", ds.glm_score_multi_dosage(Yt, Zt))
# pgh_glm_score_multi_dosage_firth on the same draws, at a cutoff low enough to apply rows of these small files
firth_t = dt.glm_score_multi_dosage_firth(Yt, Zt, firth_cutoff=1.0)
emit("glm_score_multi_dosage_firth tracks P=7", firth_t, note=f" ({int((firth_t['firth_state'] == 1).sum())} applied)")
emit("glm_score_multi_dosage_firth no tracks", ds.glm_score_multi_dosage_firth(Yt, Zt, firth_cutoff=1.0))
for d in (ss, st, ds, dt):
    d.close()

# ---- sparse-resident: pgh_glm_sparse, pgh_burden_sparse, pgh_score_sparse ----------------------------------------
M_R, N_R = 160, 4099
rare = W.rare_matrix(M_R, N_R, rng)
for v, rate in ((7, 0.01), (8, 0.3)):  # het-majority rows: rare_matrix draws none
    hit = rng.random(N_R) < rate
    rare[v] = 1
    rare[v, hit] = rng.integers(0, 4, hit.sum(), dtype=np.uint8)
rare[9] = 0  # a row past kGlmSparseLong entries
rare[9, rng.permutation(N_R)[:1500]] = rng.integers(1, 4, 1500, dtype=np.uint8)
rare[10] = 3  # a missing-majority row past kGlmSparseLong called entries: every one of them joins the list
rare[10, rng.permutation(N_R)[:1300]] = rng.integers(0, 3, 1300, dtype=np.uint8)
assert np.bincount(rare[10], minlength=4).argmax() == 3 and (rare[10] != 3).sum() > 1024
minor = N_R - np.array([np.bincount(r, minlength=4).max() for r in rare])
assert (minor > 1024).any() and ((minor > 0) & (minor <= 1024)).any()  # both sides of kGlmSparseLong
rare_path = os.path.join(out_dir, "rare.pgen")
W.write_pgen(rare_path, rare, W.choose_kinds(rare, rng))
keep_r = rng.random(N_R) < 0.7
n_keep_r = int(keep_r.sum())
Zr, Zrs = covar(rng, 3, N_R), covar(rng, 3, n_keep_r)
yr, yrs = pheno(rng, N_R, Zr), pheno(rng, n_keep_r, Zrs)
yb, ybs = pheno(rng, N_R, Zr, "logistic"), pheno(rng, n_keep_r, Zrs, "logistic")
WIDTHS = (1, 2, 4, 8, 12, 16, 20)  # the instantiated covariate widths past 0; k = kp - 1 at kp = 1 covers the width 0
set_off = np.concatenate([[0], np.cumsum(rng.integers(0, 12, 40))]).astype(np.uint64)
set_vidx = rng.integers(0, M_R, int(set_off[-1])).astype(np.uint32)
set_w = rng.normal(size=len(set_vidx))
scored = rng.permutation(M_R)[:120].astype(np.uint32)
flip = (rng.random(len(scored)) < 0.5).astype(np.uint8)
for max_minor, form in ((N_R, "entries only"), (1, "with dense-form rows")):
    sp = L.Dataset.open(rare_path, sparse=True, max_minor=max_minor)
    info = sp.sparse_info()
    if max_minor == N_R:
        assert info.dense_variant_ct == 0 and all(info.base_hist[c] > 0 for c in range(4))
    else:
        assert info.dense_variant_ct > 0 and info.sparse_variant_ct > 0
    sub = sp.subset(keep_r)
    emit(f"glm_sparse {form}", sp.glm_sparse(yr, Zr), sp.glm_sparse(yr, None))
    emit(f"glm_sparse {form}, subset", sp.glm_sparse(yrs, Zrs, subset=sub, v_begin=3, v_end=M_R - 2))
    emit(f"glm_score_sparse {form}", sp.glm_score_sparse(yb, Zr), sp.glm_score_sparse(yb, None))
    emit(f"glm_score_sparse {form}, subset", sp.glm_score_sparse(ybs, Zrs, subset=sub, v_begin=3, v_end=M_R - 2))
    if max_minor == N_R:
        for k in sorted({k for kp in WIDTHS for k in (kp, kp - 1)}):
            Zk = covar(rng, k, N_R)
            emit(f"glm_sparse {form}, k={k}", sp.glm_sparse(pheno(rng, N_R, Zk), Zk))
            emit(f"glm_score_sparse {form}, k={k}", sp.glm_score_sparse(pheno(rng, N_R, Zk, "logistic"), Zk))
    emit(f"burden_sparse {form}, weighted", sp.burden_sparse(yr, set_off, set_vidx, weights=set_w, covariates=Zr))
    emit(f"burden_sparse {form}, unweighted", sp.burden_sparse(yr, set_off, set_vidx, covariates=Zr))
    emit(f"burden_sparse {form}, subset", sp.burden_sparse(yrs, set_off, set_vidx, weights=set_w, covariates=Zrs,
                                                              subset=sub))
    emit(f"skat_sparse {form}, weighted", *sp.skat_sparse(yb, set_off, set_vidx, weights=set_w, covariates=Zr,
                                                          return_lambda=True))
    for n_cols in (1, 9):
        w = rng.normal(size=(len(scored), n_cols))
        for mode in (L.SCORE_MEAN_IMPUTE, L.SCORE_CENTER, L.SCORE_NO_MEAN_IMPUTATION):
            emit(f"score_sparse {form}, n_cols={n_cols} mode={mode}", sp.score_sparse(scored, w, mode=mode),
                 sp.score_sparse(scored, w, flip=flip, mode=mode), sp.score_sparse(scored, w, flip=flip, mode=mode, subset=sub))
    emit(f"sparse counts and sample classes {form}", sp.counts_range(), sp.counts_range(subset=sub), sp.sample_counts(),
         sp.sample_counts(vidx=scored, subset=sub))
    sub.close()
    sp.close()

# carrier lists across a chunk boundary of pgh_glm_sparse and pgh_glm_score_sparse (16384 variants)
M_C, N_C = 17000, 311
prefix = os.path.join(out_dir, "carriers")
write_carrier_pfile(prefix, M_C, N_C, carrier_rows(M_C, N_C, 0.02, 5))
sp = L.Dataset.open(prefix + ".pgen", sparse=True)
Zc = covar(rng, 2, N_C)
emit("glm_sparse across a chunk", sp.glm_sparse(pheno(rng, N_C, Zc), Zc))
emit("glm_score_sparse across a chunk", sp.glm_score_sparse(pheno(rng, N_C, Zc, "logistic"), Zc))
sp.close()

# ---- the score tests that share the ranked row walk and the budget plan: pgh_glm_score_multi, _multi_spa, _multi_firth
# and pgh_glm_score_sparse_spa, on the inputs of their tests; and pgh_glm_score_sparse_firth beside the latter -----------
import subset_shapes as SS  # noqa: E402
import test_glm_score_multi as GM  # noqa: E402
import test_glm_score_multi_spa as MS  # noqa: E402

SCRATCH_ENV = "PGH_GLM_SCORE_SCRATCH_BYTES"
CUT = 0.1  # the lowest cutoff the entry points take: the saddlepoint and Firth are tried in most fitted rows
STEP = 4096  # samples of one step of the walk


def share(res, key):
    """The share of the rows in which the follow-up was applied, next to the share of the fitted rows."""
    return f"  applied {np.mean(res[key] == 1):.3f} of {np.mean(res['errcode'] == None):.3f} fitted"  # noqa: E711


def score_family(tag, dense, Y, Z, **kw):
    emit(f"glm_score_multi {tag}", dense.glm_score_multi(Y, Z, **kw))
    spa = dense.glm_score_multi_spa(Y, Z, spa_cutoff=CUT, **kw)
    emit(f"glm_score_multi_spa {tag}", spa, note=share(spa, "spa_state"))
    firth = dense.glm_score_multi_firth(Y, Z, firth_cutoff=CUT, **kw)
    emit(f"glm_score_multi_firth {tag}", firth, note=share(firth, "firth_state"))


for n in (4096, 4099, 8209):  # one full step of the walk, a second step of three samples, a third step
    case = MS.inputs(n)
    path = os.path.join(out_dir, f"score_walk_{n}.pgen")
    W.write_pgen(path, case.geno, case.kinds)
    # test_glm_score_multi_spa's three phenotypes and one with a missing-majority pattern
    sparse_y = case.y.copy()
    sparse_y[np.random.default_rng(n).random(n) < 0.6] = np.nan
    Y = np.vstack([MS.phenotypes(case), sparse_y])
    assert np.isnan(sparse_y).mean() > 0.5
    # a step in which the correction kernel ranks more than 256 missing calls and the follow-ups more than 256 entries
    in_s = ~np.isnan(Y[0][:STEP])
    assert ((case.geno[:, :STEP] == 3) & in_s).sum(axis=1).max() > 256
    assert (((case.geno[:, :STEP] == 1) | (case.geno[:, :STEP] == 2)) & in_s).sum(axis=1).max() > 256
    dense = L.Dataset.open(path)
    forms = [("entries only", L.Dataset.open(path, sparse=True, max_minor=n)),
             ("with dense-form rows", L.Dataset.open(path, sparse=True, max_minor=1))]
    for k in (0, 4, 5, 20):
        Zk = case.covariates(k) if k else None
        score_family(f"n={n} k={k}", dense, Y, Zk)
        for form, sp in forms:
            res = sp.glm_score_sparse_spa(case.y, Zk, cutoff=CUT)
            emit(f"glm_score_sparse_spa {form}, n={n} k={k}", res, note=share(res, "spa_state"))
            res = sp.glm_score_sparse_firth(case.y, Zk, firth_cutoff=CUT)
            emit(f"glm_score_sparse_firth {form}, n={n} k={k}", res, note=share(res, "firth_state"))
    if n == 4099:
        # a subset that cuts every 16-code word
        keep_w = SS.shapes(n)["stride4"]
        Zs4 = np.ascontiguousarray(case.covariates(4)[:, keep_w])
        sub = dense.subset(keep_w)
        score_family(f"n={n} k=4 subset", dense, np.ascontiguousarray(Y[:, keep_w]), Zs4, subset=sub)
        sub.close()
        for form, sp in forms:
            sub = sp.subset(keep_w)
            res = sp.glm_score_sparse_spa(case.y[keep_w], Zs4, cutoff=CUT, subset=sub)
            emit(f"glm_score_sparse_spa {form}, n={n} k=4 subset", res, note=share(res, "spa_state"))
            res = sp.glm_score_sparse_firth(case.y[keep_w], Zs4, firth_cutoff=CUT, subset=sub)
            emit(f"glm_score_sparse_firth {form}, n={n} k=4 subset", res, note=share(res, "firth_state"))
            sub.close()
        # Scratch budgets (k = 4).  The block of one phenotype and its mask are 2,129,920 + 1,040 = 2,130,960 bytes,
        # more than three quarters of either budget: one phenotype per block.  2,400,960 leaves 270,000: 270,000 / 4 * 3 /
        # 65,584 = 3 stashes, and the 73,248 bytes after them a chunk of 214 variants (341 bytes each with the
        # saddlepoint) or 237 (308 with Firth); without a follow-up, 270,000 / 276 = 978 variants, the whole range.
        # 2,200,960 leaves 70,000: one stash and a chunk of 12 or 14 variants, or 253 without a follow-up.
        for budget in (2_400_960, 2_200_960):
            before = os.environ.get(SCRATCH_ENV)
            os.environ[SCRATCH_ENV] = str(budget)
            score_family(f"n={n} k=4 budget={budget}", dense, Y, case.covariates(4))
            if before is None:
                del os.environ[SCRATCH_ENV]
            else:
                os.environ[SCRATCH_ENV] = before
        # 17 phenotypes at k = 13: every phenotype after the first straddles a 16-column block edge
        Zl, Yl = GM.layout_inputs(13)
        assert Yl.shape == (17, n)
        score_family(f"n={n} k=13 P=17", dense, Yl, Zl)
    for d in [dense] + [sp for _, sp in forms]:
        d.close()

# ---- pgh_glm_score_sparse_multi, on the inputs of its tests.  These cases come last and draw from generators of their
# own, so that the lines above are those of a build without the entry point ---------------------------------------------
import test_glm_score_sparse_multi as SM  # noqa: E402

n = 4099
geno, kinds = SM._matrix(SM.M_R, n, n)
path = os.path.join(out_dir, f"score_sparse_multi_{n}.pgen")
W.write_pgen(path, geno, kinds)
keep_m = np.random.default_rng(12).random(n) < 0.5
for max_minor, form in ((n, "entries only"), (1, "with dense-form rows")):
    sp = L.Dataset.open(path, sparse=True, max_minor=max_minor)
    for k in (0, 3):
        Zk, Yk, _ = SM.parity_inputs(n, k)
        emit(f"glm_score_sparse_multi {form}, k={k} P=6", sp.glm_score_sparse_multi(Yk, Zk if k else None))
    Z3, Y3, _ = SM.parity_inputs(n, 3)
    emit(f"glm_score_sparse_multi {form}, k=3 P=65",
         sp.glm_score_sparse_multi(np.stack([Y3[i % len(Y3)] for i in range(65)]), Z3))
    sub = sp.subset(keep_m)
    emit(f"glm_score_sparse_multi {form}, k=3 subset",
         sp.glm_score_sparse_multi(np.ascontiguousarray(Y3[:, keep_m]), np.ascontiguousarray(Z3[:, keep_m]), subset=sub))
    sub.close()
    if max_minor == n:
        for k in (4, 20):
            rng_k = np.random.default_rng(3000 + k)
            Zk = SM._covariates(rng_k, k, n)
            Yk = np.stack([SM.O.pheno(rng_k, n, Zk), SM.O.pheno(rng_k, n, Zk, case_rate=0.35, missing=0.1)])
            emit(f"glm_score_sparse_multi {form}, k={k} P=2", sp.glm_score_sparse_multi(Yk, Zk))
    sp.close()

# ---- pgh_glm_score_sparse_multi_spa, on the same files and inputs at the lowest cutoff.  Again last, after every line of
# a build without the entry point -----------------------------------------------------------------------------------------
for max_minor, form in ((n, "entries only"), (1, "with dense-form rows")):
    sp = L.Dataset.open(path, sparse=True, max_minor=max_minor)
    for k in (0, 3):
        Zk, Yk, _ = SM.parity_inputs(n, k)
        res = sp.glm_score_sparse_multi_spa(Yk, Zk if k else None, spa_cutoff=CUT)
        emit(f"glm_score_sparse_multi_spa {form}, k={k} P=6", res, note=share(res, "spa_state"))
    res = sp.glm_score_sparse_multi_spa(np.stack([Y3[i % len(Y3)] for i in range(65)]), Z3, spa_cutoff=CUT)
    emit(f"glm_score_sparse_multi_spa {form}, k=3 P=65", res, note=share(res, "spa_state"))
    sub = sp.subset(keep_m)
    res = sp.glm_score_sparse_multi_spa(np.ascontiguousarray(Y3[:, keep_m]), np.ascontiguousarray(Z3[:, keep_m]),
                                        spa_cutoff=CUT, subset=sub)
    emit(f"glm_score_sparse_multi_spa {form}, k=3 subset", res, note=share(res, "spa_state"))
    sub.close()
    if max_minor == n:
        for k in (4, 20):
            rng_k = np.random.default_rng(3000 + k)
            Zk = SM._covariates(rng_k, k, n)
            Yk = np.stack([SM.O.pheno(rng_k, n, Zk), SM.O.pheno(rng_k, n, Zk, case_rate=0.35, missing=0.1)])
            res = sp.glm_score_sparse_multi_spa(Yk, Zk, spa_cutoff=CUT)
            emit(f"glm_score_sparse_multi_spa {form}, k={k} P=2", res, note=share(res, "spa_state"))
    sp.close()

# ---- pgh_glm_score_sparse_multi_firth, on the same files and inputs at the lowest cutoff.  Again last, after every line
# of a build without the entry point -------------------------------------------------------------------------------------
for max_minor, form in ((n, "entries only"), (1, "with dense-form rows")):
    sp = L.Dataset.open(path, sparse=True, max_minor=max_minor)
    for k in (0, 3):
        Zk, Yk, _ = SM.parity_inputs(n, k)
        res = sp.glm_score_sparse_multi_firth(Yk, Zk if k else None, firth_cutoff=CUT)
        emit(f"glm_score_sparse_multi_firth {form}, k={k} P=6", res, note=share(res, "firth_state"))
    res = sp.glm_score_sparse_multi_firth(np.stack([Y3[i % len(Y3)] for i in range(65)]), Z3, firth_cutoff=CUT)
    emit(f"glm_score_sparse_multi_firth {form}, k=3 P=65", res, note=share(res, "firth_state"))
    sub = sp.subset(keep_m)
    res = sp.glm_score_sparse_multi_firth(np.ascontiguousarray(Y3[:, keep_m]), np.ascontiguousarray(Z3[:, keep_m]),
                                          firth_cutoff=CUT, subset=sub)
    emit(f"glm_score_sparse_multi_firth {form}, k=3 subset", res, note=share(res, "firth_state"))
    sub.close()
    if max_minor == n:
        for k in (4, 20):
            rng_k = np.random.default_rng(3000 + k)
            Zk = SM._covariates(rng_k, k, n)
            Yk = np.stack([SM.O.pheno(rng_k, n, Zk), SM.O.pheno(rng_k, n, Zk, case_rate=0.35, missing=0.1)])
            res = sp.glm_score_sparse_multi_firth(Yk, Zk, firth_cutoff=CUT)
            emit(f"glm_score_sparse_multi_firth {form}, k={k} P=2", res, note=share(res, "firth_state"))
    sp.close()

# ---- pgh_glm_sparse_multi, on the same file and the phenotypes of its tests' builders (fitted rows).  Again last, on
# generators of its own, after every line of a build without these cases ----------------------------------------------
import test_glm_sparse_multi as LM  # noqa: E402

x_l = LM._values(geno)
for max_minor, form in ((n, "entries only"), (1, "with dense-form rows")):
    sp = L.Dataset.open(path, sparse=True, max_minor=max_minor)
    for k in (0, 3):
        Zk, Yk = LM.parity_inputs(n, k)
        rng_k = np.random.default_rng(4000 + k)
        # the builder's five and a sixth with a missing pattern of its own
        Yk = np.vstack([Yk, LM._phenotype(rng_k, n, Zk, 1.0, rng_k.random(n) < 0.05, x_l)])
        emit(f"glm_sparse_multi {form}, k={k} P=6", sp.glm_sparse_multi(Yk, Zk if k else None))
    Z3, Y3 = LM.parity_inputs(n, 3)
    emit(f"glm_sparse_multi {form}, k=3 P=65", sp.glm_sparse_multi(np.stack([Y3[i % len(Y3)] for i in range(65)]), Z3))
    sub = sp.subset(keep_m)
    emit(f"glm_sparse_multi {form}, k=3 subset",
         sp.glm_sparse_multi(np.ascontiguousarray(Y3[:, keep_m]), np.ascontiguousarray(Z3[:, keep_m]), subset=sub))
    sub.close()
    if max_minor == n:
        for k in (4, 20):
            rng_k = np.random.default_rng(5000 + k)
            Zk = LM._covariates(rng_k, k, n)
            emit(f"glm_sparse_multi {form}, k={k} P=2", sp.glm_sparse_multi(LM._phenotypes(rng_k, n, Zk, 2, x=x_l), Zk))
    sp.close()
