"""Batched view registration on a real MI355X (sfm_register_views) against
numpy at its own hypotheses, against tests/golden/register_views.npz and
against itself alone, permuted and with one hypothesis more.

The scene, the sample tables and the numpy pieces of the rule come from
tests/test_register_views.py; the fixture's generator asserts the margins
(every final error a pixel from the threshold) that make the masks exact.
"""
import os

import numpy as np
import pytest

import test_register_views as rv
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
K = rv.K

# Distance of the returned pose from the fixture's converged minimum, over every
# view of 63 and more correspondences and H in 64, 65, 256.  Levenberg-Marquardt
# stops by MINPACK's rules at 1e-8, short of the minimum; measured on the MI355X
# the largest rotation angle is 1.26e-9 rad and the largest |C - C_min| 7.46e-9
# (view registration).  The bounds are ten times those.
POSE_ANGLE_BOUND = 1.26e-8
POSE_CENTRE_BOUND = 7.46e-8


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "register_views.npz"))


@pytest.fixture(scope="module")
def scene():
    return rv.load_scene()


def run(core, sc, samples, thr, views=None, **kw):
    """the call on the whole scene, or on ``views`` of it in that order"""
    if views is None:
        vs, pt, xy = sc["view_start"], sc["pt_idx"], sc["xy"]
    else:
        sel = np.concatenate([np.arange(sc["view_start"][v], sc["view_start"][v + 1]) for v in views])
        vs = np.concatenate([[0], np.cumsum(sc["n_v"][list(views)])])
        pt, xy, samples = sc["pt_idx"][sel], sc["xy"][sel], samples[list(views)]
    return core.register_views(K, sc["X"], vs, pt, xy, samples, threshold=thr, want_counts=True, want_models=True,
                               **kw)


@pytest.fixture(scope="module")
def results(core, scene, gold):
    """H -> the call's outputs on the whole scene, computed once"""
    thr = float(gold["threshold"])
    return {H: run(core, scene, rv.sample_table(H), thr) for H in rv.HS}


def per_view(out, sc, v, views=None):
    """view v's part of every output (v: position in the call)"""
    n_v = sc["n_v"] if views is None else sc["n_v"][list(views)]
    vs = np.concatenate([[0], np.cumsum(n_v)])
    C, R, cost, n_inl, inl, hyp, count, info, counts, models = out
    return (C[v], R[v], cost[v], n_inl[v], inl[vs[v]:vs[v + 1]], hyp[v], count[v], info[v], counts[v], models[v])


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [64, 65, 1025])
def test_fit_is_the_least_singular_vector(scene, results, n):
    Ki = np.linalg.inv(K)
    worst = 0.0
    for v in np.where(scene["n_v"] == n)[0]:
        X, xy = rv.view(scene, v)
        for H in (65, 256):
            models = results[H][9][v]
            for h, s in enumerate(rv.sample_table(H)[v]):
                A = rv.dlt_rows(X[s], xy[s])
                p = (Ki @ models[h]).reshape(12)
                sv = np.linalg.svd(A, compute_uv=False)
                res = np.linalg.norm(A @ p) / np.linalg.norm(p)
                bound = sv[-1] * (1 + 1e-6) + 1e-12 * sv[0]
                worst = max(worst, (res - sv[-1]) / sv[0])
                assert res <= bound, (v, H, h, res, sv[-1], sv[0])
    print(f"n {n}: largest (residual - sigma_min) / |A| {worst:.3g}")


@pytest.mark.parametrize("H", rv.HS)
def test_counts_are_numpys_at_the_returned_models(scene, results, gold, H):
    thr = float(gold["threshold"])
    _, _, _, _, _, hyp, count, info, counts, models = results[H]
    for v in range(scene["V"]):
        X, xy = rv.view(scene, v)
        if len(X) < 6:
            assert not counts[v].any() and not models[v].any()
            continue
        for h in range(H):
            lo = rv.inlier_mask(models[v, h], X, xy, thr * (1 - 1e-9)).sum()
            hi = rv.inlier_mask(models[v, h], X, xy, thr * (1 + 1e-9)).sum()
            assert lo <= counts[v, h] <= hi, (v, h, lo, counts[v, h], hi)
        assert hyp[v] == np.argmax(counts[v]) and count[v] == counts[v].max()  # first maximum


@pytest.mark.parametrize("H", rv.HS[1:])
def test_result_is_the_truth_at_the_converged_minimum(scene, results, gold, H):
    C, R, cost, n_inl, inl, hyp, count, info, _, _ = results[H]
    worst_a = worst_c = worst_cost = 0.0
    for v in scene["checked"]:
        s, e = scene["view_start"][v], scene["view_start"][v + 1]
        truth = scene["truth"][s:e]
        assert 1 <= info[v] <= 5
        assert np.array_equal(inl[s:e], truth), (v, int(inl[s:e].sum()), int(truth.sum()))
        assert n_inl[v] == truth.sum() and n_inl[v] >= count[v]
        X, xy = rv.view(scene, v)
        e2 = rv.errors2(rv.projection(C[v], R[v]), X, xy)[0]
        assert np.isclose(e2[truth].sum(), cost[v], rtol=1e-12, atol=0)  # cost is the final inliers' own
        a, c = rv.rot_angle(R[v], gold["R_min"][v]), np.linalg.norm(C[v] - gold["C_min"][v])
        rel = cost[v] / gold["cost_min"][v] - 1.0
        worst_a, worst_c, worst_cost = max(worst_a, a), max(worst_c, c), max(worst_cost, rel)
        print(f"H {H} view {v}: info {info[v]} angle {a:.3g} |dC| {c:.3g} cost / cost_min - 1 {rel:.3g}")
        assert cost[v] <= gold["cost_min"][v] * (1 + 1e-7), (v, rel)
        assert a <= POSE_ANGLE_BOUND and c <= POSE_CENTRE_BOUND, (v, a, c)
    print(f"H {H}: largest angle {worst_a:.3g} |dC| {worst_c:.3g} cost excess {worst_cost:.3g}")


def test_small_views(scene, results):
    for H in rv.HS:
        C, R, cost, n_inl, inl, hyp, count, info, counts, models = results[H]
        # five correspondences: not attempted
        assert info[0] == -1 and not C[0].any() and np.array_equal(R[0], np.eye(3)) and not inl[:5].any()
        assert n_inl[0] == 0 and hyp[0] == -1 and count[0] == 0
        for v in (1, 2):  # six and seven, noise-free: the true pose
            s, e = scene["view_start"][v], scene["view_start"][v + 1]
            assert info[v] >= 1 and inl[s:e].all() and n_inl[v] == e - s
            Ct, Rt = scene["C_true"][v], scene["R_true"][v]
            print(f"H {H} view {v}: |dC| / |C| {np.linalg.norm(C[v] - Ct) / np.linalg.norm(Ct):.3g} "
                  f"|dR| {np.abs(R[v] - Rt).max():.3g}")
            assert np.linalg.norm(C[v] - Ct) <= 1e-8 * np.linalg.norm(Ct)
            assert np.abs(R[v] - Rt).max() <= 1e-8


def test_a_view_alone_and_permuted_views_give_the_same_bits(core, scene, results, gold):
    thr = float(gold["threshold"])
    whole = results[64]
    for v in (2, 5, 10, 12):
        alone = run(core, scene, rv.sample_table(64), thr, views=[v])
        assert same(per_view(alone, scene, 0, [v]), per_view(whole, scene, v)), v
    order = [12, 3, 0, 9, 1, 7, 11, 5, 2, 10, 4, 8, 6]
    perm = run(core, scene, rv.sample_table(64), thr, views=order)
    for k, v in enumerate(order):
        assert same(per_view(perm, scene, k, order), per_view(whole, scene, v)), v


def test_one_hypothesis_more_that_cannot_win_changes_nothing(core, scene, results, gold):
    thr = float(gold["threshold"])
    t65 = rv.sample_table(65)
    full = results[65]
    first = run(core, scene, np.ascontiguousarray(t65[:, :64]), thr)
    counts = full[8]
    quiet = [v for v in range(scene["V"]) if scene["n_v"][v] >= 6 and counts[v, 64] < counts[v, :64].max()]
    assert quiet, "every view's 65th hypothesis ties or wins: reseed"
    for v in quiet:
        a, b = per_view(first, scene, v), per_view(full, scene, v)
        assert same(a[:8], b[:8]), v
        assert np.array_equal(a[8], b[8][:64]) and np.array_equal(a[9], b[9][:64])


def test_too_few_inliers_returns_the_winning_hypothesis(core, scene, results, gold):
    thr = float(gold["threshold"])
    v = 10  # 65 correspondences, contaminated
    base = per_view(results[64], scene, v)
    C, R, cost, n_inl, inl, hyp, count, info, counts, models = per_view(
        run(core, scene, rv.sample_table(64), thr, views=[v], min_inliers=66), scene, 0, [v])
    assert info == -3 and hyp == base[5] and count == base[6] and np.array_equal(counts, base[8])
    X, xy = rv.view(scene, v)
    m = rv.inlier_mask(models[hyp], X, xy, thr)
    assert np.array_equal(inl, m) and n_inl == count == m.sum()
    assert np.isclose(cost, rv.errors2(models[hyp], X, xy)[0][m].sum(), rtol=1e-12)
    # the pose is the hypothesis's own: the one its null vector gives
    s = rv.sample_table(64)[v][hyp]
    Cn, Rn, _ = rv.pose_from_null((np.linalg.inv(K) @ models[hyp]).reshape(12))
    assert np.allclose(C, Cn, rtol=0, atol=1e-9) and np.allclose(R, Rn, rtol=0, atol=1e-9) and len(set(s)) == 6


def small_batch(sc):
    """Three views cut from the scene, for the shared branches below: view 0's
    five correspondences (below the minimum: dead), the first 40 of view 4
    (inside one tile) and view 7's 1,025 followed by view 0's five, which are
    outliers to it (1,030: past the tile edge at 1,024).  Returns (view_start,
    pt_idx, xy)."""
    vs = sc["view_start"]
    sel = np.concatenate([np.arange(vs[0], vs[1]), np.arange(vs[4], vs[4] + 40), np.arange(vs[7], vs[8]),
                          np.arange(vs[0], vs[1])])
    return np.array([0, 5, 45, 1075]), sc["pt_idx"][sel], sc["xy"][sel]


def test_every_count_zero_returns_the_earliest_finite_hypothesis(core, scene):
    """threshold 1e-200: its square underflows to 0 and no squared error is
    below 0, so every count of every view is 0.  The winner is then the first
    hypothesis whose model is finite, returned unrefitted (info -3) with an
    empty mask; C, R are that hypothesis's own pose (pose_from_null of its
    model, to the 1e-9 of test_too_few_inliers_returns_the_winning_hypothesis)."""
    vs, pt, xy = small_batch(scene)
    t = core.register_samples(np.diff(vs), 5, rv.SAMPLE_SEED)
    C, R, cost, n_inl, inl, hyp, count, info, counts, models = core.register_views(
        K, scene["X"], vs, pt, xy, t, threshold=1e-200, want_counts=True, want_models=True)
    assert not counts.any() and not count.any() and not n_inl.any() and not inl.any() and not cost.any()
    assert info[0] == -1 and hyp[0] == -1 and not C[0].any() and np.array_equal(R[0], np.eye(3))
    for v in (1, 2):
        finite = np.isfinite(models[v]).all(axis=(1, 2))
        assert info[v] == -3 and finite.any() and hyp[v] == np.argmax(finite), (v, info[v], hyp[v], finite)
        Cn, Rn, _ = rv.pose_from_null((np.linalg.inv(K) @ models[v, hyp[v]]).reshape(12))
        print(f"view {v}: best_hyp {hyp[v]} |dC| {np.abs(C[v] - Cn).max():.3g} |dR| {np.abs(R[v] - Rn).max():.3g}")
        assert np.allclose(C[v], Cn, rtol=0, atol=1e-9) and np.allclose(R[v], Rn, rtol=0, atol=1e-9)


def test_store_round_trip(core):
    """sfm_multiview.register_views on a small synthetic store: three candidate
    images, the middle one with 30 % wrong observations"""
    import sfm_synthetic as syn
    from sfm_io import MatchStore
    from sfm_multiview import register_views
    p = syn.ba_problem(4, 160, 4, seed=5, dense=False)
    X = p["X_true"]
    rng = np.random.default_rng(8)
    feat, img = np.repeat(np.arange(160), 4), np.tile(np.arange(4), 160)
    h = np.einsum("ij,njk,nk->ni", K, p["R_true"][img], X[feat] - p["C_true"][img])
    xy = h[:, :2] / h[:, 2:] + rng.normal(0, 0.5, (len(feat), 2))
    wrong = np.zeros(len(feat), dtype=bool)
    wrong[np.where(img == 2)[0][rng.choice(160, 48, replace=False)]] = True
    wrong[np.where(img == 3)[0][rng.choice(160, 16, replace=False)]] = True
    ang = rng.uniform(0, 2 * np.pi, wrong.sum())
    xy[wrong] += rng.uniform(40, 120, wrong.sum())[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])
    st = MatchStore(160, 4, feat.astype(np.int32), img.astype(np.int32), xy[:, 0].copy(), xy[:, 1].copy())
    st.flag[:] = 1
    rows = np.arange(0, 160, 2)  # the features that have a point
    cand = np.array([2, 1, 3])
    order, out, index = register_views(st, K, rows, X[rows], cand, H=64, seed=1, update_flags=True)
    n_inl, inl, info = out[3], out[4], out[7]
    assert np.all(info >= 1)
    assert np.array_equal(order, np.argsort(-n_inl, kind="stable")) and cand[order[0]] == 1
    assert np.array_equal(inl, ~wrong[index])
    in_call = np.zeros(len(feat), dtype=bool)
    in_call[index] = True
    assert np.array_equal(st.flag == 0, in_call & wrong)  # exactly the outliers of the registered views
