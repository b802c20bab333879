"""The tiling boundaries of the five hypothesis-batch entry points on a real
MI355X: verify_pairs, essential_pairs, init_pairs, register_views and
register_views_p3p share one scaffold (csrc/hyp_batch.hpp) -- a flat grid over
(row, hypothesis tile), the row's correspondences staged through LDS in tiles
of 1024, and hypotheses per block halved from 1,024 correspondences and
quartered from 4,096.  The other GPU modules stop at 1,025 correspondences and
at hypothesis counts next to 64; here every row crosses a boundary.

One call per entry point: rows of SIZES correspondences -- either side of one
and of four LDS tiles -- with a row below every entry point's minimum in the
middle, so that the live rows come back in two runs; H = 70 hypotheses, a
multiple of no tile in use (64, 32, 16, 8), so that every row ends in a partial
hypothesis tile.  The scenes are the CPU modules': noise-free inliers and a
quarter of the correspondences displaced by 40-120 px.

Every expected value is numpy's.  A returned model's count lies between
numpy's counts at the threshold moved by 1e-9 either way; the winner is the
first maximum under the entry point's tie rule; the short row has info -1 and
the host's blank outputs; a row called alone gives the bits it gives in the
batch.  Where the rule breaks a tie on the count by the smaller cost
(essential_pairs, register_views_p3p), the costs of all-inlier models of exact
points are rounding alone -- a residual of some 1e-13 px, squared and summed
over 4,097 correspondences, below 1e-21 px^2 -- so which of them is smaller is
not numpy's to say: the winner must hold the best count, and numpy's cost of
it may exceed that of no other holder by more than COST_SLACK.  The last leg
of every rule, the earlier of equals, is checked where equals can be had: with
the second half of the table a copy of the first, every model comes twice with
the same bits, in another block of the grid, and the winner must come from the
first half.
"""
import functools

import numpy as np
import pytest

import sfm_synthetic as syn
import test_essential_pairs as ep
import test_init_pairs as ip
import test_register_views as rv
import test_verify_pairs as vp

pytestmark = pytest.mark.gpu

SIZES = (1023, 1024, 1025, 3, 4095, 4096, 4097)
DEAD = 3                 # the row below every minimum (4, 5, 6, 8, 8)
LIVE = tuple(r for r in range(len(SIZES)) if r != DEAD)
H = 70
SEED = 71
WRONG_SHARE = 0.25
K = syn.K_REF
THR_PAIR, THR_VIEW, THR_HOMOG = vp.THRESHOLD, 4.0, ip.H_THRESHOLD
COST_SLACK = 1e-18       # px^2: three orders above the rounding of an exact scene's cost (see above)
LO, HI = 1 - 1e-9, 1 + 1e-9


# ------------------------------------------------------------------ the scenes
@functools.lru_cache(maxsize=None)
def pair_rows():
    """row -> (x1, x2, true F): test_verify_pairs' pairs without noise, a quarter of the matches wrong"""
    made = [vp.make_pair([SEED, r], n, 0.0, WRONG_SHARE) for r, n in enumerate(SIZES)]
    return [(np.ascontiguousarray(m[0]), np.ascontiguousarray(m[1]), m[3]) for m in made]


@functools.lru_cache(maxsize=None)
def view_rows():
    """(X, row -> (pt_idx, xy)): test_register_views' views without noise, a quarter of the observations displaced"""
    p = syn.ba_problem(len(SIZES), 4200, 3, seed=SEED, dense=False)
    X = np.ascontiguousarray(p["X_true"])
    rows = []
    for v, n in enumerate(SIZES):
        rng = np.random.default_rng([SEED, v])
        idx = rng.choice(len(X), n, replace=False)
        h = (K @ (p["R_true"][v] @ (X[idx] - p["C_true"][v]).T)).T
        o = h[:, :2] / h[:, 2:]
        bad = rng.choice(n, int(round(WRONG_SHARE * n)), replace=False)
        ang, mag = rng.uniform(0, 2 * np.pi, len(bad)), rng.uniform(40, 120, len(bad))
        o[bad] += np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
        rows.append((idx.astype(np.int32), np.ascontiguousarray(o)))
    return X, rows


def csr(rows):
    return np.concatenate([[0], np.cumsum([SIZES[r] for r in rows])]).astype(np.int64)


def pair_args(rows):
    sc = pair_rows()
    return (csr(rows), np.concatenate([sc[r][0] for r in rows]), np.concatenate([sc[r][1] for r in rows]))


def view_args(rows):
    X, sc = view_rows()
    return (X, csr(rows), np.concatenate([sc[r][0] for r in rows]), np.concatenate([sc[r][1] for r in rows]))


@functools.lru_cache(maxsize=None)
def table(name, twice=False):
    """the sample table of the whole batch; a row keeps its samples when it is
    called alone.  ``twice``: hypotheses H / 2 .. H - 1 are hypotheses 0 .. H / 2 - 1 again"""
    import _sfmcore as core
    t = getattr(core, name)(np.array(SIZES), H, SEED)
    if twice:
        t[:, H // 2:] = t[:, :H // 2]
    return t


# ------------------------------------------------------------------ the five calls
# name -> (the call on ``rows`` of the batch, the outputs that hold one entry per correspondence)
def call_verify(core, rows, twice=False):
    return core.verify_pairs(*pair_args(rows), table("pair_samples", twice)[list(rows)], threshold=THR_PAIR,
                             want_counts=True, want_models=True)


def call_essential(core, rows, twice=False):
    return core.essential_pairs(K, *pair_args(rows), table("essential_samples", twice)[list(rows)],
                                threshold=THR_PAIR, want_counts=True, want_models=True)


def call_init(core, rows, twice=False):
    F = np.array([pair_rows()[r][2] for r in rows])
    return core.init_pairs(K, *pair_args(rows), F, table("homography_samples", twice)[list(rows)],
                           h_threshold=THR_HOMOG, want_cands=True, want_hcounts=True, want_hmodels=True)


def call_register(core, rows, twice=False):
    return core.register_views(K, *view_args(rows), table("register_samples", twice)[list(rows)],
                               threshold=THR_VIEW, want_counts=True, want_models=True)


def call_p3p(core, rows, twice=False):
    return core.register_views_p3p(K, *view_args(rows), table("p3p_samples", twice)[list(rows)],
                                   threshold=THR_VIEW, want_counts=True, want_models=True)


CALLS = {"verify_pairs": (call_verify, {3}), "essential_pairs": (call_essential, {3}),
         "init_pairs": (call_init, {10, 11, 12}), "register_views": (call_register, {4}),
         "register_views_p3p": (call_p3p, {4})}


def per_row(name, out, rows):
    """row -> its part of every output of a call on ``rows``"""
    st = csr(rows)
    return {r: tuple(a[st[k]:st[k + 1]] if i in CALLS[name][1] else a[k] for i, a in enumerate(out))
            for k, r in enumerate(rows)}


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def batch(core):
    """name -> row -> the row's outputs in the call on all seven rows, computed once"""
    rows = tuple(range(len(SIZES)))
    return {name: per_row(name, fn(core, rows), rows) for name, (fn, _) in CALLS.items()}


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ------------------------------------------------------------------ numpy's counts
def view_of(r):
    X, sc = view_rows()
    return X[sc[r][0]], sc[r][1]


def view_count_cost(P, X, xy, thr):
    m = rv.inlier_mask(P, X, xy, thr)
    return int(m.sum()), float(rv.errors2(P, X, xy)[0][m].sum())


@pytest.mark.parametrize("r", LIVE)
def test_verify_pairs_counts_and_winner(batch, r):
    x1, x2, _ = pair_rows()[r]
    F, cost, n_inl, inl, hyp, count, info, counts, models = batch["verify_pairs"][r]
    assert counts.shape == (H,) and models.shape == (H, 3, 3)
    finite = np.isfinite(models).all(axis=(1, 2))  # a model that is not finite counts 0
    lo = np.array([vp.inlier_mask(F, x1, x2, THR_PAIR * LO).sum() if f else 0 for F, f in zip(models, finite)])
    hi = np.array([vp.inlier_mask(F, x1, x2, THR_PAIR * HI).sum() if f else 0 for F, f in zip(models, finite)])
    assert np.all(lo <= counts) and np.all(counts <= hi)
    # most inliers, then the earliest
    assert counts.max() > 0 and hyp == int(np.argmax(counts)) and count == counts.max()
    assert info >= 0 and n_inl == inl.sum() >= count


@pytest.mark.parametrize("r", LIVE)
def test_essential_pairs_counts_and_winner(batch, r):
    x1, x2, _ = pair_rows()[r]
    F, cost, n_inl, inl, hyp, count, info, E, n_sol, counts, models = batch["essential_pairs"][r]
    assert counts.shape == (H, 10) and n_sol.min() >= 0 and n_sol.max() <= 10
    costs = np.full((H, 10), np.inf)
    for h in range(H):
        assert not counts[h, n_sol[h]:].any() and not models[h, n_sol[h]:].any()
        for s in range(n_sol[h]):
            lo = ep.score(models[h, s], x1, x2, THR_PAIR * LO)[0]
            hi, c, _ = ep.score(models[h, s], x1, x2, THR_PAIR * HI)
            assert lo <= counts[h, s] <= hi, (h, s, lo, counts[h, s], hi)
            costs[h, s] = c
    # most inliers, then the smaller cost, then the earliest hypothesis
    best = counts.max()
    assert best > 0 and count == best and counts[hyp].max() == best
    tied = counts == best
    assert costs[hyp][tied[hyp]].min() <= costs[tied].min() + COST_SLACK
    assert info >= 0 and n_inl == inl.sum() >= count


@pytest.mark.parametrize("r", LIVE)
def test_init_pairs_counts_and_winner(batch, r):
    x1, x2, _ = pair_rows()[r]
    d = dict(zip(("R", "C", "counts", "best", "n_good", "median", "h_count", "h_best", "Hbest", "info", "X", "good",
                  "angle", "cands", "hcounts", "hmodels"), batch["init_pairs"][r]))
    assert d["hmodels"].shape == (H, 3, 3) and np.isfinite(d["hmodels"]).all()
    lo = ip.h_counts(d["hmodels"], x1, x2, THR_HOMOG * LO)
    hi = ip.h_counts(d["hmodels"], x1, x2, THR_HOMOG * HI)
    assert np.all(lo <= d["hcounts"]) and np.all(d["hcounts"] <= hi)
    # most inliers, then the earliest
    assert d["hcounts"].max() > 0 and d["h_best"] == int(np.argmax(d["hcounts"]))
    assert d["h_count"] == d["hcounts"].max() and np.array_equal(d["Hbest"], d["hmodels"][d["h_best"]])
    # the pose kernel under the true F: the winning candidate sees the points that are not wrong matches
    assert d["info"] == 0 and d["best"] == int(np.argmax(d["counts"]))
    assert d["counts"].max() >= 0.74 * len(x1) and d["n_good"] == d["good"].sum()


@pytest.mark.parametrize("r", LIVE)
def test_register_views_counts_and_winner(batch, r):
    X, xy = view_of(r)
    C, R, cost, n_inl, inl, hyp, count, info, counts, models = batch["register_views"][r]
    assert counts.shape == (H,) and models.shape == (H, 3, 4)
    for h in range(H):
        lo = rv.inlier_mask(models[h], X, xy, THR_VIEW * LO).sum()
        hi = rv.inlier_mask(models[h], X, xy, THR_VIEW * HI).sum()
        assert lo <= counts[h] <= hi, (h, lo, counts[h], hi)
    # most inliers, then the earliest
    assert counts.max() > 0 and hyp == int(np.argmax(counts)) and count == counts.max()
    assert info >= 0 and n_inl == inl.sum() >= count


@pytest.mark.parametrize("r", LIVE)
def test_register_views_p3p_counts_and_winner(batch, r):
    X, xy = view_of(r)
    C, R, cost, n_inl, inl, hyp, count, info, n_sol, counts, models = batch["register_views_p3p"][r]
    assert counts.shape == (H, 4) and n_sol.min() >= 0 and n_sol.max() <= 4
    costs = np.full((H, 4), np.inf)
    for h in range(H):
        assert not counts[h, n_sol[h]:].any() and not models[h, n_sol[h]:].any()
        for k in range(n_sol[h]):
            lo = view_count_cost(models[h, k], X, xy, THR_VIEW * LO)[0]
            hi, costs[h, k] = view_count_cost(models[h, k], X, xy, THR_VIEW * HI)
            assert lo <= counts[h, k] <= hi, (h, k, lo, counts[h, k], hi)
    # most inliers, then the smaller cost, then the earlier slot
    best = counts.max()
    assert best > 0 and count == best and counts[hyp].max() == best
    tied = counts == best
    assert costs[hyp][tied[hyp]].min() <= costs[tied].min() + COST_SLACK
    assert info >= 0 and n_inl == inl.sum() >= count


# ------------------------------------------------------------------ the earlier of equals
# name -> (where the winning hypothesis stands in the outputs, where the per-hypothesis tables begin)
WINNER = {"verify_pairs": (4, 7), "essential_pairs": (4, 8), "init_pairs": (7, 14), "register_views": (5, 8),
          "register_views_p3p": (5, 8)}


@pytest.mark.parametrize("name", list(CALLS))
def test_of_two_equal_hypotheses_the_earlier_wins(core, name):
    """hypothesis h + H / 2 is hypothesis h again (35 is a multiple of no tile, so the copy sits at another
    place of another block): the same model, count and cost, and the winner is one of the first H / 2"""
    rows = tuple(range(len(SIZES)))
    out = per_row(name, CALLS[name][0](core, rows, twice=True), rows)
    half = H // 2
    for r in LIVE:
        hyp, tables = out[r][WINNER[name][0]], out[r][WINNER[name][1]:]
        for a in tables:  # counts, models and, where there is one, n_sol
            assert np.array_equal(a[:half], a[half:], equal_nan=True), (name, r)
        assert 0 <= hyp < half, (name, r, hyp)


# ------------------------------------------------------------------ the short row
def test_the_short_row_is_the_hosts(batch):
    eye = np.eye(3)
    for name in ("verify_pairs", "essential_pairs"):
        out = batch[name][DEAD]
        F, cost, n_inl, inl, hyp, count, info = out[:7]
        assert info == -1 and not F.any() and cost == 0 and n_inl == 0 and not inl.any() and hyp == -1 and count == 0
        assert all(not a.any() for a in out[7:]), name
    for name in ("register_views", "register_views_p3p"):
        out = batch[name][DEAD]
        C, R, cost, n_inl, inl, hyp, count, info = out[:8]
        assert info == -1 and not C.any() and np.array_equal(R, eye) and cost == 0 and n_inl == 0 and not inl.any()
        assert hyp == -1 and count == 0 and all(not a.any() for a in out[8:]), name
    R, C, counts, best, n_good, median, h_count, h_best, Hbest, info, X, good, angle, cands, hcounts, hmodels = \
        batch["init_pairs"][DEAD]
    assert info == -1 and np.array_equal(R, eye) and h_best == -1
    assert not any(np.any(a) for a in (C, counts, best, n_good, median, h_count, Hbest, X, good, angle, cands,
                                       hcounts, hmodels))


# ------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("name", list(CALLS))
def test_a_row_alone_gives_the_bits_of_the_batch(core, batch, name):
    for r in range(len(SIZES)):
        alone = per_row(name, CALLS[name][0](core, (r,)), (r,))[r]
        assert same(alone, batch[name][r]), (name, r)
