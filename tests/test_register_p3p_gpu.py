"""Calibrated batched view registration on a real MI355X
(sfm_register_views_p3p) against the restatement of tests/test_register_p3p.py
(Grunert's quartic through np.roots), against numpy at its own models, against
tests/golden/register_p3p.npz and against itself alone, permuted and with one
hypothesis more.  The fixture's generator asserts the margins (every final
error a pixel from the threshold) that make the masks exact.
"""
import os

import numpy as np
import pytest

import test_register_p3p as p3
import test_register_views as rv
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
K = p3.K
THR = p3.THRESHOLD

# Device solutions against the restatement's, over every comparable hypothesis
# of the checked views at H = 64 and 256: measured on the MI355X the largest
# distance of a device solution from its bearings is 5.36e-13 and the largest
# distance from the restatement's matching pose 5.32e-10 (max over |dR| entries
# and |dC|; the poses of a nearly degenerate sample are that sensitive to
# rounding).  The bounds are ten times those (calibrated view
# registration).
BEARING_BOUND = 5.36e-12
SOLUTION_BOUND = 5.32e-9
# Distance of the returned pose from the fixture's converged minimum over the
# checked views and H in 64, 65, 256: measured 1.22e-9 rad and 7.5e-9; ten times.
POSE_ANGLE_BOUND = 1.22e-8
POSE_CENTRE_BOUND = 7.5e-8
# The returned cost over the fixture's cost_min, relative: measured 7.93e-14 at
# most; ten times.  One-sided: a cost below cost_min passes.
COST_EXCESS_BOUND = 7.93e-13
# The noise-free views of 4 and 5 correspondences against the true pose:
# measured |dC| / |C| 3.25e-15 and |dR| 3.54e-16; ten times.
SMALL_CENTRE_BOUND = 3.25e-14
SMALL_ROTATION_BOUND = 3.54e-15


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "register_p3p.npz"))


@pytest.fixture(scope="module")
def scene():
    return p3.load_scene()


def run(core, sc, samples, views=None, **kw):
    """the call on the whole scene, or on ``views`` of it in that order"""
    if views is None:
        vs, pt, xy = sc["view_start"], sc["pt_idx"], sc["xy"]
    else:
        sel = np.concatenate([np.arange(sc["view_start"][v], sc["view_start"][v + 1]) for v in views])
        vs = np.concatenate([[0], np.cumsum(sc["n_v"][list(views)])])
        pt, xy, samples = sc["pt_idx"][sel], sc["xy"][sel], samples[list(views)]
    return core.register_views_p3p(K, sc["X"], vs, pt, xy, samples, threshold=THR, want_counts=True,
                                   want_models=True, **kw)


@pytest.fixture(scope="module")
def results(core, scene):
    """H -> the call's outputs on the whole scene, computed once"""
    return {H: run(core, scene, p3.sample_table(H)) for H in p3.HS}


def per_view(out, sc, v, views=None):
    """view v's part of every output (v: position in the call)"""
    n_v = sc["n_v"] if views is None else sc["n_v"][list(views)]
    vs = np.concatenate([[0], np.cumsum(n_v)])
    C, R, cost, n_inl, inl, hyp, count, info, n_sol, counts, models = out
    return (C[v], R[v], cost[v], n_inl[v], inl[vs[v]:vs[v + 1]], hyp[v], count[v], info[v], n_sol[v], counts[v],
            models[v])


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def pose_of(P):
    """(R, C) of a projection K [R | -R C]"""
    B = np.linalg.inv(K) @ P
    return B[:, :3], -B[:, :3].T @ B[:, 3]


@pytest.mark.parametrize("H", [64, 256])
def test_solutions_are_the_restatements_set(scene, results, gold, H):
    n_sol, models = results[H][8], results[H][10]
    worst_b = worst_s = 0.0
    compared = 0
    for v in scene["checked"]:
        X, xy = p3.view(scene, v)
        b = p3.bearings(xy)
        hyps = p3.restated_hypotheses(int(v), H)
        excluded = gold[f"excluded_H{H}"][v, :H]
        assert np.array_equal(excluded, [ill for _, ill in hyps])
        for h, smp in enumerate(p3.sample_table(H)[v]):
            dev = [pose_of(models[v, h, k]) for k in range(n_sol[v, h])]
            assert not models[v, h, n_sol[v, h]:].any()
            for R, C in dev:  # every device solution is one, comparable or not
                worst_b = max(worst_b, p3.property_error(R, C, X[smp], b[smp]))
            if excluded[h]:
                continue
            ref = [(R, C) for R, C, _, _, _ in hyps[h][0]]
            assert len(dev) == len(ref), (v, h, len(dev), len(ref))
            left = list(range(len(ref)))
            for R, C in dev:  # one to one: each device pose takes the nearest restated pose still free
                d = [max(np.abs(R - ref[j][0]).max(), np.abs(C - ref[j][1]).max()) for j in left]
                worst_s = max(worst_s, min(d))
                left.pop(int(np.argmin(d)))
            compared += 1
    print(f"H {H}: {compared} hypotheses compared, largest bearing miss {worst_b:.3g}, largest pose distance "
          f"{worst_s:.3g}")
    assert worst_b <= BEARING_BOUND and worst_s <= SOLUTION_BOUND


@pytest.mark.parametrize("H", p3.HS)
def test_counts_are_numpys_at_the_returned_models(scene, results, H):
    _, _, _, _, _, hyp, count, info, n_sol, counts, models = results[H]
    for v in range(scene["V"]):
        X, xy = p3.view(scene, v)
        if len(X) < 4:
            assert not n_sol[v].any() and not counts[v].any() and not models[v].any()
            continue
        assert n_sol[v].min() >= 0 and n_sol[v].max() <= 4
        for h in range(H):
            assert not counts[v, h, n_sol[v, h]:].any()
            for k in range(n_sol[v, h]):
                P = models[v, h, k]
                lo = rv.inlier_mask(P, X, xy, THR * (1 - 1e-9)).sum()
                hi = rv.inlier_mask(P, X, xy, THR * (1 + 1e-9)).sum()
                assert lo <= counts[v, h, k] <= hi, (v, h, k, lo, counts[v, h, k], hi)
        assert count[v] == counts[v].max()
        assert counts[v, hyp[v]].max() == count[v]  # the winner's hypothesis holds the best count


@pytest.mark.parametrize("H", p3.HS)
def test_winner_is_the_restatements(scene, results, gold, H):
    """most inliers, then the smaller cost: best_hyp and best_count against the
    restatement's winner on every checked view where that winner is clear -- no
    other slot of its count has a cost within 1e-9 relative, and no excluded
    hypothesis reaches its count"""
    hyp, count = results[H][5], results[H][6]
    compared = 0
    for v in scene["checked"]:
        hyps = p3.restated_hypotheses(int(v), H)
        bc, bcost, bh, bk = p3.restated_winner(int(v), H)[:4]
        clear = True
        for h, (sols, ill) in enumerate(hyps):
            for k, (_, _, _, m, cost) in enumerate(sols):
                if (h, k) != (bh, bk) and m.sum() == bc and (ill or cost <= bcost * (1 + 1e-9)):
                    clear = False
        if hyps[bh][1] or not clear:
            continue
        assert hyp[v] == bh and count[v] == bc, (v, hyp[v], bh, count[v], bc)
        compared += 1
    print(f"H {H}: winner compared on {compared} of {len(scene['checked'])} views")
    assert compared >= 1


def test_equal_count_and_cost_go_to_the_earlier_hypothesis(core, scene, results):
    """a hypothesis repeated under a later index cannot win; repeated under an
    earlier index it wins with the same pose, bit for bit"""
    v = 5
    base = per_view(results[64], scene, v)
    w = int(base[5])
    later, earlier = (63 if w != 63 else 62), (0 if w != 0 else 1)
    t = p3.sample_table(64).copy()
    t[v, later] = t[v, w]
    if later > w:
        out = per_view(run(core, scene, t, views=[v]), scene, 0, [v])
        assert out[5] == w and same(out[:5], base[:5]) and same(out[6:8], base[6:8])
    t = p3.sample_table(64).copy()
    t[v, earlier] = t[v, w]
    if earlier < w:
        out = per_view(run(core, scene, t, views=[v]), scene, 0, [v])
        assert out[5] == earlier and same(out[:5], base[:5]) and same(out[6:8], base[6:8])
    assert later > w or earlier < w


@pytest.mark.parametrize("H", p3.HS)
def test_result_is_the_truth_at_the_converged_minimum(scene, results, gold, H):
    C, R, cost, n_inl, inl, hyp, count, info = results[H][:8]
    worst_a = worst_c = worst_cost = 0.0
    for v in scene["checked"]:
        s, e = scene["view_start"][v], scene["view_start"][v + 1]
        truth = scene["truth"][s:e]
        assert 1 <= info[v] <= 5
        assert np.array_equal(inl[s:e], truth), (v, int(inl[s:e].sum()), int(truth.sum()))
        assert n_inl[v] == truth.sum() and n_inl[v] >= count[v]
        X, xy = p3.view(scene, v)
        e2 = rv.errors2(rv.projection(C[v], R[v]), X, xy)[0]
        assert np.isclose(e2[truth].sum(), cost[v], rtol=1e-12, atol=0)  # cost is the final inliers' own
        a, c = rv.rot_angle(R[v], gold["R_min"][v]), np.linalg.norm(C[v] - gold["C_min"][v])
        rel = cost[v] / gold["cost_min"][v] - 1.0
        worst_a, worst_c, worst_cost = max(worst_a, a), max(worst_c, c), max(worst_cost, rel)
        print(f"H {H} view {v}: info {info[v]} angle {a:.3g} |dC| {c:.3g} cost / cost_min - 1 {rel:.3g}")
        assert cost[v] <= gold["cost_min"][v] * (1 + COST_EXCESS_BOUND), (v, rel)
        assert a <= POSE_ANGLE_BOUND and c <= POSE_CENTRE_BOUND, (v, a, c)
    print(f"H {H}: largest angle {worst_a:.3g} |dC| {worst_c:.3g} cost excess {worst_cost:.3g}")


def test_planar_views_register_where_the_six_point_entry_point_cannot(core, scene, results, gold):
    """the capability: points on one plane.  register_views on the same views
    and seed finds no consensus (info -3)."""
    C, R, cost, n_inl, inl, hyp, count, info = results[256][:8]
    for v in p3.PLANAR:
        s, e = scene["view_start"][v], scene["view_start"][v + 1]
        assert info[v] >= 1 and np.array_equal(inl[s:e], scene["truth"][s:e])
        assert rv.rot_angle(R[v], gold["R_min"][v]) <= POSE_ANGLE_BOUND
        assert np.linalg.norm(C[v] - gold["C_min"][v]) <= POSE_CENTRE_BOUND
    views = list(p3.PLANAR)
    sel = np.concatenate([np.arange(scene["view_start"][v], scene["view_start"][v + 1]) for v in views])
    vs = np.concatenate([[0], np.cumsum(scene["n_v"][views])])
    t6 = core.register_samples(scene["n_v"], 256, p3.SAMPLE_SEED)[views]
    out6 = core.register_views(K, scene["X"], vs, scene["pt_idx"][sel], scene["xy"][sel], t6, threshold=THR)
    assert np.all(out6[7] == -3), out6[7]


def test_the_sixty_percent_view_registers_at_64_hypotheses(scene, results):
    C, R, cost, n_inl, inl, hyp, count, info = results[64][:8]
    v = p3.HARD
    s, e = scene["view_start"][v], scene["view_start"][v + 1]
    assert info[v] >= 1 and np.array_equal(inl[s:e], scene["truth"][s:e])


def test_degenerate_samples_have_no_solution_and_change_nothing_else(core, scene, results):
    v = p3.DEGENERATE
    for H in p3.HS:
        out = per_view(results[H], scene, v)
        n_sol, counts, models = out[8:]
        assert n_sol[0] == 0 and n_sol[1] == 0 and not counts[:2].any() and not models[:2].any()
        assert n_sol[2:].min() >= 1
        assert out[7] >= 1 and out[4].all() and out[3] == scene["n_v"][v]  # noise-free: everything an inlier
        assert np.abs(out[1] - scene["R_true"][v]).max() <= 1e-8
    # the other hypotheses do not depend on the two: with ordinary samples in their place
    t = p3.sample_table(64).copy()
    t[v, 0], t[v, 1] = t[v, 2], t[v, 3]
    other = per_view(run(core, scene, t, views=[v]), scene, 0, [v])
    base = per_view(results[64], scene, v)
    assert np.array_equal(other[8][2:], base[8][2:]) and np.array_equal(other[9][2:], base[9][2:])
    assert np.array_equal(other[10][2:], base[10][2:])


def small_batch(core, sc):
    """Three views cut from the scene, for the shared branches below: view 2's
    five correspondences, the degenerate view's 40 (inside one tile) and view
    7's 1,025 followed by view 2's five, which are outliers to it (1,030: past
    the tile edge at 1,024).  Returns (view_start, pt_idx, xy, samples): the
    table at H = 5, the degenerate view's first two samples degenerate as in
    sample_table."""
    vs, d = sc["view_start"], p3.DEGENERATE
    sel = np.concatenate([np.arange(vs[2], vs[3]), np.arange(vs[d], vs[d + 1]), np.arange(vs[7], vs[8]),
                          np.arange(vs[2], vs[3])])
    start = np.array([0, 5, 45, 1075])
    t = core.p3p_samples(np.diff(start), 5, p3.SAMPLE_SEED)
    t[1, 0], t[1, 1] = (0, 1, 2), (3, 4, 5)
    return start, sc["pt_idx"][sel], sc["xy"][sel], t


def test_every_count_zero_returns_the_earliest_solution(core, scene):
    """threshold 1e-200: its square underflows to 0 and no squared error is
    below 0, so every count of every view is 0.  The winner is then slot 0 of
    the first hypothesis with a solution, returned unrefitted (info -3) with an
    empty mask; C, R are that model's pose, to the 1e-9 of
    test_too_few_inliers_returns_the_winning_solution."""
    vs, pt, xy, t = small_batch(core, scene)
    C, R, cost, n_inl, inl, hyp, count, info, n_sol, counts, models = core.register_views_p3p(
        K, scene["X"], vs, pt, xy, t, threshold=1e-200, want_counts=True, want_models=True)
    assert not counts.any() and not count.any() and not n_inl.any() and not inl.any() and not cost.any()
    assert not n_sol[1, :2].any()
    for v in range(3):
        assert info[v] == -3 and n_sol[v].any() and hyp[v] == np.argmax(n_sol[v] > 0), (v, info[v], hyp[v], n_sol[v])
        Rk, Ck = pose_of(models[v, hyp[v], 0])
        print(f"view {v}: best_hyp {hyp[v]} |dC| {np.abs(C[v] - Ck).max():.3g} |dR| {np.abs(R[v] - Rk).max():.3g}")
        assert np.allclose(C[v], Ck, rtol=0, atol=1e-9) and np.allclose(R[v], Rk, rtol=0, atol=1e-9)


def test_a_view_without_a_usable_hypothesis_is_refused_and_changes_nothing_else(core, scene):
    """every sample of one view degenerate (three collinear points, or one 3-D
    point under two indices): no solution, no winner (info -2), and the other
    views' outputs bit for bit those of the call with the ordinary table"""
    vs, pt, xy, t = small_batch(core, scene)
    bad = t.copy()
    bad[1] = [(0, 1, 2), (3, 4, 5), (2, 0, 1), (4, 3, 6), (3, 4, 7)]
    n_v = np.diff(vs)

    def call(tab):
        out = core.register_views_p3p(K, scene["X"], vs, pt, xy, tab, threshold=THR, want_counts=True,
                                      want_models=True)
        C, R, cost, n_inl, inl, hyp, count, info, n_sol, counts, models = out
        return [(C[v], R[v], cost[v], n_inl[v], inl[vs[v]:vs[v + 1]], hyp[v], count[v], info[v], n_sol[v], counts[v],
                 models[v]) for v in range(3)]
    base, out = call(t), call(bad)
    C, R, cost, n_inl, inl, hyp, count, info, n_sol, counts, models = out[1]
    assert not n_sol.any() and not counts.any() and not models.any()
    assert hyp == -1 and info == -2 and count == 0 and n_inl == 0 and cost == 0
    assert np.array_equal(R, np.eye(3)) and not C.any() and len(inl) == n_v[1] and not inl.any()
    assert base[1][7] != -2  # the ordinary table has solutions for this view
    for v in (0, 2):
        assert same(out[v], base[v]), v


def test_small_views(scene, results):
    for H in p3.HS:
        C, R, cost, n_inl, inl, hyp, count, info, n_sol, counts, models = results[H]
        # three correspondences: not attempted
        assert info[0] == -1 and not C[0].any() and np.array_equal(R[0], np.eye(3)) and not inl[:3].any()
        assert n_inl[0] == 0 and hyp[0] == -1 and count[0] == 0
        assert not n_sol[0].any() and not counts[0].any() and not models[0].any()
        for v in (1, 2):  # four and five, noise-free: the true pose
            s, e = scene["view_start"][v], scene["view_start"][v + 1]
            assert info[v] >= 1 and inl[s:e].all() and n_inl[v] == e - s
            Ct, Rt = scene["C_true"][v], scene["R_true"][v]
            dc, dr = np.linalg.norm(C[v] - Ct) / np.linalg.norm(Ct), np.abs(R[v] - Rt).max()
            print(f"H {H} view {v}: |dC| / |C| {dc:.3g} |dR| {dr:.3g}")
            assert dc <= SMALL_CENTRE_BOUND and dr <= SMALL_ROTATION_BOUND


def test_a_view_alone_and_permuted_views_give_the_same_bits(core, scene, results):
    whole = results[64]
    for v in (1, 5, 9, 12, 14):
        alone = run(core, scene, p3.sample_table(64), views=[v])
        assert same(per_view(alone, scene, 0, [v]), per_view(whole, scene, v)), v
    order = [12, 3, 0, 9, 1, 14, 7, 11, 5, 13, 2, 10, 4, 8, 6]
    perm = run(core, scene, p3.sample_table(64), views=order)
    for k, v in enumerate(order):
        assert same(per_view(perm, scene, k, order), per_view(whole, scene, v)), v


def test_one_hypothesis_more_that_cannot_win_changes_nothing(core, scene, results):
    t65 = p3.sample_table(65)
    full = results[65]
    first = run(core, scene, np.ascontiguousarray(t65[:, :64]))
    counts = full[9]
    quiet = [v for v in range(scene["V"]) if scene["n_v"][v] >= 4 and counts[v, 64].max() < counts[v, :64].max()]
    assert quiet, "every view's 65th hypothesis ties or wins: reseed"
    for v in range(scene["V"]):
        a, b = per_view(first, scene, v), per_view(full, scene, v)
        if v in quiet:
            assert same(a[:8], b[:8]), v
        # a hypothesis's n_sol, counts and models do not depend on H
        assert np.array_equal(a[8], b[8][:64]) and np.array_equal(a[9], b[9][:64])
        assert np.array_equal(a[10], b[10][:64])


def test_too_few_inliers_returns_the_winning_solution(core, scene, results):
    v = 8  # 65 correspondences, contaminated
    base = per_view(results[64], scene, v)
    C, R, cost, n_inl, inl, hyp, count, info, n_sol, counts, models = per_view(
        run(core, scene, p3.sample_table(64), views=[v], min_inliers=66), scene, 0, [v])
    assert info == -3 and hyp == base[5] and count == base[6] and np.array_equal(counts, base[9])
    X, xy = p3.view(scene, v)
    k = int(np.argmin([np.abs(pose_of(models[hyp, j])[1] - C).max() for j in range(n_sol[hyp])]))
    m = rv.inlier_mask(models[hyp, k], X, xy, THR)
    assert np.array_equal(inl, m) and n_inl == count == m.sum() == counts[hyp, k]
    assert np.isclose(cost, rv.errors2(models[hyp, k], X, xy)[0][m].sum(), rtol=1e-12)
    Rk, Ck = pose_of(models[hyp, k])
    assert np.allclose(C, Ck, rtol=0, atol=1e-9) and np.allclose(R, Rk, rtol=0, atol=1e-9)
    # no other solution has more inliers, none of as many a smaller cost
    for h in range(64):
        for j in range(n_sol[h]):
            assert counts[h, j] <= count
            if counts[h, j] == count and (h, j) != (hyp, k):
                mj = rv.inlier_mask(models[h, j], X, xy, THR)
                assert rv.errors2(models[h, j], X, xy)[0][mj].sum() >= cost * (1 - 1e-12)


def test_last_timings_holds_the_four_intervals(core, scene):
    """the call's four intervals: upload, both kernels, download and the
    fit-and-score kernel alone, from events around the two launches"""
    core.set_call_timing(True)
    try:
        run(core, scene, p3.sample_table(64))
        t = core.last_timings()
    finally:
        core.set_call_timing(False)
    assert len(t) == 4 and (t > 0).all() and t[3] <= t[1]


def test_store_round_trip(core):
    """sfm_multiview.register_views_p3p on the P3Data matching files: the points
    are synthetic (every feature gets one), the observations of four images are
    replaced by their projections with noise, a share of them displaced"""
    from sfm_io import read_matching
    from sfm_multiview import register_views_p3p
    import sfm_synthetic as syn
    st = read_matching(os.path.join(GOLDEN, "P3Data"), 5)
    rng = np.random.default_rng(4)
    p = syn.ba_problem(st.n_images, st.n_features, 3, seed=7, dense=False)
    X = p["X_true"]
    h = np.einsum("ij,njk,nk->ni", K, p["R_true"][st.image], X[st.feature] - p["C_true"][st.image])
    xy = h[:, :2] / h[:, 2:] + rng.normal(0, 0.5, (len(st), 2))
    wrong = np.zeros(len(st), dtype=bool)
    share = {1: 0.0, 2: 0.3, 3: 0.1}
    for im, sh in share.items():
        idx = np.where(st.image == im)[0]
        wrong[rng.choice(idx, int(round(sh * len(idx))), replace=False)] = True
    ang = rng.uniform(0, 2 * np.pi, wrong.sum())
    xy[wrong] += rng.uniform(40, 120, wrong.sum())[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])
    st.x[:], st.y[:] = xy[:, 0], xy[:, 1]
    st.flag[:] = 1
    rows = np.arange(0, st.n_features, 2)  # the features that have a point
    cand = np.array([2, 1, 3])
    order, out, index = register_views_p3p(st, K, rows, X[rows], cand, H=64, seed=1, update_flags=True)
    n_inl, inl, info = out[3], out[4], out[7]
    assert len(out) == 8 and np.all(info >= 1)
    assert np.array_equal(order, np.argsort(-n_inl, kind="stable"))
    assert np.array_equal(inl, ~wrong[index])
    in_call = np.zeros(len(st), dtype=bool)
    in_call[index] = True
    assert np.array_equal(st.flag == 0, in_call & wrong)  # exactly the outliers of the registered views
