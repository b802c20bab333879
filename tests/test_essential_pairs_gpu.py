"""sfm_essential_pairs on the MI355X against the numpy restatement
(tests/test_essential_pairs.py) and its fixture (tests/golden/essential_pairs.npz).

Every bound is about ten times what was measured once on the MI355X against the
restatement (measured -> bound); the device runs Householder, Gauss-Jordan and
Aberth where numpy runs LAPACK's SVD, solve and companion-matrix eigenvalues:

    solution set, nearest neighbour up to sign   7.5e-6 -> 7.5e-5
    | |E|_F - 1 |, |F - F(E)|_F                  3.3e-16 -> 4e-15
    |2 E E^T E - tr(E E^T) E|_F                  3.8e-7 -> 4e-6
    |det E|                                      1.1e-7 -> 1.1e-6
    |x^2^T E x^1| on the five sample points      3.6e-16 -> 4e-15
    |E - E_gold|_F per pair                      9.9e-6 (H = 1), 2.5e-6 (H = 64, 65) -> 1e-4
    cost, relative                               3.4e-6 (H = 1), 8.4e-11 (H = 64, 65) -> 3.5e-5
    |E - E_true|_F on the noise-free pairs       5.4e-15 -> 6e-14
    round trip, calibrated over uncalibrated     0.61 (rotation), 0.24 (direction) -> 6

The larger figures are conditioning, not arithmetic: the roots of a degree-10
polynomial from its coefficients (the solution set and the cubic residuals, on
the worst of 768 hypotheses) and a refit that both sides stop at MINPACK's 1e-8
(E and cost per pair).  The round trip's factor is measured against verify_pairs
-> init_pairs on the same store in the same run, which this change does not touch:
calibrated (0, 2) 0.182 deg / 0.445 deg and (1, 2) 0.056 / 0.254 against 0.297 /
2.16 and 0.403 / 1.07; the plane pair (3, 4) 0.164 / 1.30 against 5.79 / 62.6.
"""
import functools

import numpy as np
import pytest

import test_essential_pairs as ep
import test_init_pairs as ip
import test_verify_pairs as vp

pytestmark = pytest.mark.gpu

TOL_SOL = 7.5e-5
TOL_NORM = 4e-15
TOL_CUBIC = 4e-6
TOL_DET = 1.1e-6
TOL_EPI = 4e-15
TOL_E = 1e-4
TOL_COST = 3.5e-5
TOL_TRUE = 6e-14
FACTOR = 6.0
SOLS_H = 64


@functools.lru_cache(maxsize=None)
def device(H):
    import _sfmcore as core
    sc = ep.load_scene()
    return core.essential_pairs(ep.K, sc["pair_start"], sc["x1"], sc["x2"], ep.sample_table(H), want_counts=True,
                                want_models=True)


def live(sc):
    return [p for p in range(sc["P"]) if sc["n_p"][p] >= 5]


def test_every_comparable_hypothesis_has_the_restatements_solutions():
    g, sc = ep.fixture(), ep.load_scene()
    F, cost, n_inl, inl, hyp, count, info, E, n_sol, counts, models = device(SOLS_H)
    comp = g[f"comparable_H{SOLS_H}"]
    worst = dict(sol=0.0, norm=0.0, cubic=0.0, det=0.0, epi=0.0)
    tab = ep.sample_table(SOLS_H)
    for p in live(sc):
        assert comp[p].mean() >= 0.95
        x1, x2 = ep.pair(sc, p)
        for h in np.where(comp[p])[0]:
            n = int(g[f"n_sol_H{SOLS_H}"][p, h])
            assert n_sol[p, h] == n, (p, h)
            ref, got = g["sols"][p, h, :n], models[p, h, :n]
            assert not models[p, h, n:].any() and not counts[p, h, n:].any()
            a, b = ep.normalise(x1[tab[p, h]]), ep.normalise(x2[tab[p, h]])
            a, b = np.column_stack([a, np.ones(5)]), np.column_stack([b, np.ones(5)])
            for Eg in got:
                worst["norm"] = max(worst["norm"], abs(np.linalg.norm(Eg) - 1.0))
                worst["cubic"] = max(worst["cubic"], np.linalg.norm(2 * Eg @ Eg.T @ Eg - np.trace(Eg @ Eg.T) * Eg))
                worst["det"] = max(worst["det"], abs(np.linalg.det(Eg)))
                worst["epi"] = max(worst["epi"], np.abs(((b @ Eg) * a).sum(axis=1)).max())
                worst["sol"] = max(worst["sol"], ep.nearest(ref, Eg))
            for Er in ref:
                worst["sol"] = max(worst["sol"], ep.nearest(got, Er))
    print("measured:", worst)
    assert worst["sol"] <= TOL_SOL and worst["norm"] <= TOL_NORM and worst["cubic"] <= TOL_CUBIC
    assert worst["det"] <= TOL_DET and worst["epi"] <= TOL_EPI


def test_counts_lie_between_numpys_at_the_threshold_moved_by_1e_9():
    sc = ep.load_scene()
    n_sol, counts, models = device(65)[8:11]
    for p in live(sc):
        x1, x2 = ep.pair(sc, p)
        for h in range(65):
            for s in range(n_sol[p, h]):
                lo = ep.score(models[p, h, s], x1, x2, ep.THRESHOLD * (1 - 1e-9))[0]
                hi = ep.score(models[p, h, s], x1, x2, ep.THRESHOLD * (1 + 1e-9))[0]
                assert lo <= counts[p, h, s] <= hi, (p, h, s)


@pytest.mark.parametrize("H", ep.HS)
def test_every_pair_agrees_with_the_restatement(H):
    g, sc = ep.fixture(), ep.load_scene()
    F, cost, n_inl, inl, hyp, count, info, E = device(H)[:8]
    # exact points leave the winner to rounding (the fixture's ``decided``): there the
    # counts and the mask are compared, not which of the equal solutions won
    dec = [p for p in live(sc) if g[f"decided_H{H}"][p]]
    assert set(live(sc)) - set(dec) <= {1, 2}
    assert np.array_equal(inl, g[f"mask_H{H}"])
    assert np.array_equal(info[dec], g[f"info_H{H}"][dec]) and np.array_equal(hyp[dec], g[f"best_hyp_H{H}"][dec])
    assert np.array_equal(count, g[f"best_count_H{H}"]) and np.array_equal(n_inl, g[f"n_inliers_H{H}"])
    assert (n_inl >= count).all() and (info[live(sc)] >= 1).all()
    dE = max(np.linalg.norm(ep.align(E[p], g[f"E_H{H}"][p]) - g[f"E_H{H}"][p]) for p in dec)
    dF = max(np.linalg.norm(ep.align(F[p], ep.F_of(E[p])) - ep.F_of(E[p])) for p in live(sc))
    ref = g[f"cost_H{H}"]
    dc = max(abs(cost[p] - ref[p]) / max(ref[p], 1e-12) for p in live(sc) if sc["n_p"][p] >= 63)
    print(f"measured: H {H} |E - E_gold| {dE:.3g} |F - F(E)| {dF:.3g} cost rel {dc:.3g}")
    assert dE <= TOL_E and dF <= TOL_NORM and dc <= TOL_COST
    for p in live(sc):
        if ep.KINDS[p] == "wrong" and H >= 64:
            s, e = sc["pair_start"][p], sc["pair_start"][p + 1]
            assert np.array_equal(inl[s:e], sc["truth"][s:e])
    # n_p = 4
    assert info[0] == -1 and not E[0].any() and not F[0].any() and hyp[0] == -1 and not inl[:4].any()


def test_the_documented_paths():
    import _sfmcore as core
    sc = ep.load_scene()
    p = ep.SIZES.index(63)
    x1, x2 = ep.pair(sc, p)
    tab = ep.sample_table(64)[p:p + 1]
    # no finite solution in any hypothesis
    out = core.essential_pairs(ep.K, [0, 63], np.full_like(x1, np.nan), x2, tab, want_counts=True, want_models=True)
    F, cost, n_inl, inl, hyp, count, info, E, n_sol, counts, models = out
    assert info[0] == -2 and not E.any() and not F.any() and not inl.any() and hyp[0] == -1 and count[0] == 0
    assert cost[0] == 0 and n_inl[0] == 0 and not n_sol.any() and not counts.any() and not models.any()
    # best_count < min_inliers: the winning solution as it is
    out = core.essential_pairs(ep.K, [0, 63], x1, x2, tab, min_inliers=64, want_counts=True, want_models=True)
    F, cost, n_inl, inl, hyp, count, info, E, n_sol, counts, models = out
    assert info[0] == -3 and count[0] == n_inl[0] == inl.sum() == counts[0].max()
    assert any(np.array_equal(E[0], m) for m in models[0, hyp[0]])
    assert np.array_equal(inl, ep.score(E[0], x1, x2, ep.THRESHOLD)[2])
    # refit_rounds = 0
    out0 = core.essential_pairs(ep.K, [0, 63], x1, x2, tab, refit_rounds=0)
    assert out0[6][0] == 0 and np.array_equal(out0[7], E) and np.array_equal(out0[3], inl)
    # a K with a NaN
    Kb = ep.K.copy()
    Kb[0, 0] = np.nan
    with pytest.raises(core.SfmCoreError, match="argument"):
        core.essential_pairs(Kb, [0, 63], x1, x2, tab)


def test_poses():
    import _sfmcore as core
    sc = ep.load_scene()
    F, cost, n_inl, inl, hyp, count, info, E, n_sol, counts, models = device(64)
    # six exact points: the true matrix.  Five hold every one of their solutions, so the
    # true matrix is one of the winning hypothesis's, and the one returned holds all five
    worst = max(np.linalg.norm(ep.align(E[2], sc["E_true"][2]) - sc["E_true"][2]),
                ep.nearest(models[1, hyp[1], :n_sol[1, hyp[1]]], sc["E_true"][1]))
    print(f"measured: |E - E_true| on the noise-free pairs {worst:.3g}, cost {cost[1]:.3g} {cost[2]:.3g}")
    assert worst <= TOL_TRUE and n_inl[1] == 5 and n_inl[2] == 6
    p = ep.PLANE
    s, e = sc["pair_start"][p], sc["pair_start"][p + 1]
    x1, x2 = ep.pair(sc, p)
    m = inl[s:e]
    out = core.init_pairs(ep.K, [0, int(m.sum())], x1[m], x2[m], F[p:p + 1])
    rot, dirn = ip.pose_errors(out[0][0], out[1][0], sc["R_true"][p], sc["C_true"][p])
    print(f"measured: plane pose rotation {np.rad2deg(rot):.3g} deg, direction {np.rad2deg(dirn):.3g} deg")
    assert out[9][0] == 0 and rot < ep.PLANE_ROT_BOUND and dirn < ep.PLANE_DIR_BOUND


def test_a_pairs_outputs_do_not_depend_on_the_batch():
    import _sfmcore as core
    sc = ep.load_scene()
    H = 64
    tab = ep.sample_table(H)
    full = device(H)
    P = sc["P"]

    def same(p, out, q, a, b):
        s, e = sc["pair_start"][p], sc["pair_start"][p + 1]
        for k in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10):
            assert np.array_equal(full[k][p], out[k][q], equal_nan=True), (p, k)
        assert np.array_equal(full[3][s:e], out[3][a:b])
    for p in range(P):
        x1, x2 = ep.pair(sc, p)
        out = core.essential_pairs(ep.K, [0, len(x1)], x1, x2, tab[p:p + 1], want_counts=True, want_models=True)
        same(p, out, 0, 0, len(x1))
    perm = np.random.default_rng(1).permutation(P)
    n_p = sc["n_p"][perm]
    start = np.concatenate([[0], np.cumsum(n_p)]).astype(np.int64)
    out = core.essential_pairs(ep.K, start, np.concatenate([ep.pair(sc, p)[0] for p in perm]),
                               np.concatenate([ep.pair(sc, p)[1] for p in perm]), tab[perm], want_counts=True,
                               want_models=True)
    for q, p in enumerate(perm):
        same(p, out, q, start[q], start[q + 1])
    # one hypothesis more: the first H columns stay
    more = np.concatenate([tab, ep.sample_table(65)[:, :1]], axis=1)
    out = core.essential_pairs(ep.K, sc["pair_start"], sc["x1"], sc["x2"], more, want_counts=True, want_models=True)
    for k in (8, 9, 10):
        assert np.array_equal(full[k], out[k][:, :H])


def test_launches_and_timings():
    import _sfmcore as core
    sc = ep.load_scene()
    core.set_call_timing(True)
    try:
        core.essential_pairs(ep.K, sc["pair_start"], sc["x1"], sc["x2"], ep.sample_table(64))
        t = core.last_timings()
    finally:
        core.set_call_timing(False)
    assert len(t) == 4 and (t > 0).all() and t[3] <= t[1]


def test_store_round_trip():
    """verify_pairs_calibrated -> init_pairs on a store whose pair (3, 4) sees one plane at
    a wide baseline: that pair gets its pose, which verify_pairs -> init_pairs cannot give
    it, and the general wide pairs lose nothing"""
    from sfm_multiview import init_pairs, verify_pairs, verify_pairs_calibrated
    sc = ep.store_scene()
    st = sc["store"]
    cal = verify_pairs_calibrated(st, ep.K, H=256, seed=0)
    unc = verify_pairs(st, H=256, seed=0)
    assert len(cal[2]) == 8 and cal[2][7].shape == cal[2][0].shape
    pc, pu = init_pairs(st, ep.K, cal), init_pairs(st, ep.K, unc)
    pairs = [tuple(q) for q in cal[1].tolist()]
    err = {}
    for name, out in (("calibrated", pc[2]), ("uncalibrated", pu[2])):
        for q, (i, j) in enumerate(pairs):
            Rt, Ct = vp.relative_pose(sc, i, j)
            err[name, (i, j)] = ip.pose_errors(out[0][q], out[1][q], Rt, Ct)
    for k, v in err.items():
        print("measured:", k, "rotation %.3g deg, direction %.3g deg" % tuple(np.rad2deg(v)))
    rot, dirn = err["calibrated", (3, 4)]
    assert rot < ep.PLANE_ROT_BOUND and dirn < ep.PLANE_DIR_BOUND
    for ij in ((0, 2), (1, 2)):
        for k in range(2):
            assert err["calibrated", ij][k] <= FACTOR * err["uncalibrated", ij][k], (ij, k)


def test_every_output_keeps_the_bits_recorded_before_the_shared_driver():
    import _sfmcore as core
    import test_verify_pairs_gpu as vpg
    vpg.check_stages_keep_their_bits(core, "E")
