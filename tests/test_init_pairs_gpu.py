"""Batched initial-pair selection on a real MI355X (sfm_init_pairs) against the
rule restated in numpy at the device's own candidates and models, against
tests/golden/init_pairs.npz and against itself alone, permuted, without the
homography table and with one hypothesis more.

The scene, the sample table and the restatement come from
tests/test_init_pairs.py; the fixture's generator asserts the margins (under 1 %
of a pair within 1e-9 relative of a cheirality or threshold limit, the winning
candidate clear of the next by more than that) and the conditioning (E, the
sampled homography systems) that make the comparisons below exact.
"""
import numpy as np
import pytest

import test_init_pairs as ip

pytestmark = pytest.mark.gpu
NAMES = ("R", "C", "counts", "best", "n_good", "median", "h_count", "h_best", "Hbest", "info", "X", "good", "angle",
         "cands", "hcounts", "hmodels")
PER_CORR = ("X", "good", "angle")


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def scene():
    return ip.load_scene()


def run(core, sc, samples, pairs=None, **kw):
    """the call on the whole scene, or on ``pairs`` of it in that order: a dict of its outputs"""
    pairs = list(range(sc["P"])) if pairs is None else list(pairs)
    sel = np.concatenate([np.arange(sc["pair_start"][p], sc["pair_start"][p + 1]) for p in pairs])
    ps = np.concatenate([[0], np.cumsum(sc["n_p"][pairs])])
    hs = None if samples is None else samples[pairs]
    out = core.init_pairs(ip.K, ps, sc["x1"][sel], sc["x2"][sel], sc["F"][pairs], hs, h_threshold=ip.H_THRESHOLD,
                          max_reproj=ip.MAX_REPROJ, want_cands=True, want_hcounts=True, want_hmodels=True, **kw)
    return dict(zip(NAMES, out), pair_start=ps)


def per_pair(out, k):
    """the part of every output that belongs to the pair at place k of the call"""
    s, e = out["pair_start"][k], out["pair_start"][k + 1]
    return {name: (out[name][s:e] if name in PER_CORR else out[name][k]) for name in NAMES}


def same(a, b, names=NAMES):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in names)


@pytest.fixture(scope="module")
def whole(core, scene):
    return run(core, scene, ip.sample_table())


def live(sc):
    return [p for p in range(sc["P"]) if ip.fixture()["info"][p] == 0]


def test_candidates_are_numpys_as_a_set(scene, whole):
    worst = worst_rot = 0.0
    for p in live(scene):
        d = per_pair(whole, p)
        assert d["info"] == 0
        ref = np.array([np.concatenate([R.reshape(-1), t]) for R, t in ip.candidates(scene["F"][p])])
        dist = np.abs(d["cands"][:, None, :] - ref[None, :, :]).max(axis=2)       # device x numpy
        match = dist.argmin(axis=1)
        assert sorted(match.tolist()) == [0, 1, 2, 3]                              # a bijection
        worst = max(worst, dist.min(axis=1).max())
        assert dist.min(axis=1).max() <= 1e-9
        for c in d["cands"]:
            R, t = c[:9].reshape(3, 3), c[9:]
            err = max(np.abs(R @ R.T - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0), abs(np.linalg.norm(t) - 1.0))
            worst_rot = max(worst_rot, err)
            assert err <= 1e-12
        assert np.array_equal(d["R"], d["cands"][d["best"], :9].reshape(3, 3))
        t = d["cands"][d["best"], 9:]
        assert np.abs(d["C"] + d["R"].T @ t).max() <= 1e-14 and abs(np.linalg.norm(d["C"]) - 1.0) <= 1e-12
    print(f"candidates against numpy's <= {worst:.3g}; R^T R - I, det R - 1, |t| - 1 <= {worst_rot:.3g}")


def test_counts_are_numpys_at_the_returned_candidates(scene, whole):
    for p in live(scene):
        x1, x2 = ip.pair(scene, p)
        d = per_pair(whole, p)
        for m, c in enumerate(d["cands"]):
            R, t = c[:9].reshape(3, 3), c[9:]
            fr, near = ip.front(R, t, ip.triangulate(ip.proj2(R, t), x1, x2))
            assert near.sum() <= 0.01 * len(x1)
            assert (fr & ~near).sum() <= d["counts"][m] <= (fr | near).sum()
        assert d["counts"].dtype == np.int64 and d["best"] == int(np.argmax(d["counts"]))


def test_points_good_and_angles_are_numpys_under_the_winner(scene, whole):
    worst_X = worst_a = 0.0
    for p in live(scene):
        x1, x2 = ip.pair(scene, p)
        d = per_pair(whole, p)
        t = d["cands"][d["best"], 9:]
        X, good, ang, near = ip.points_under(d["R"], t, x1, x2)
        assert near.sum() <= 0.01 * len(x1)
        assert np.array_equal(d["good"][~near], good[~near])
        both = d["good"] & good
        rel = np.linalg.norm(d["X"][both] - X[both], axis=1) / np.linalg.norm(X[both], axis=1)
        if both.any():
            worst_X = max(worst_X, rel.max())
            worst_a = max(worst_a, np.abs(d["angle"][both] - ang[both]).max())
            assert rel.max() <= 1e-7 and np.abs(d["angle"][both] - ang[both]).max() <= 1e-9
        assert not d["angle"][~d["good"]].any()
        assert d["n_good"] == d["good"].sum()
        assert abs(int(d["n_good"]) - int(ip.fixture()["n_good"][p])) <= near.sum()
    print(f"X against numpy's DLT <= {worst_X:.3g} relative, angle <= {worst_a:.3g} rad")


def test_median_angle_is_the_lower_median_of_the_devices_own_angles_as_bits(scene, whole):
    some = 0
    for p in range(scene["P"]):
        d = per_pair(whole, p)
        v = d["angle"][d["good"]]
        n = len(v)
        want = np.partition(v, (n - 1) // 2)[(n - 1) // 2] if n else 0.0
        assert np.float64(d["median"]).tobytes() == np.float64(want).tobytes()
        some += n > 0
    assert some >= 8
    g = ip.fixture()
    limit = np.deg2rad(ip.MIN_ANGLE_DEG)
    assert whole["median"][ip.PB] < limit < whole["median"][ip.PA]
    assert np.allclose(whole["median"], g["median"], rtol=0, atol=1e-9)


def test_homography_hypotheses_map_their_samples_and_counts_are_numpys(scene, whole):
    tab = ip.sample_table()
    worst = 0.0
    for p in range(scene["P"]):
        x1, x2 = ip.pair(scene, p)
        d = per_pair(whole, p)
        if len(x1) < 8:
            assert not d["hcounts"].any() and not d["hmodels"].any() and d["h_best"] == -1 and d["h_count"] == 0
            assert not d["Hbest"].any()
            continue
        assert d["hmodels"].shape == (ip.HH, 3, 3) and np.isfinite(d["hmodels"]).all()
        for s, H in zip(tab[p], d["hmodels"]):
            e, ok = ip.h_transfer2(H, x1[s], x2[s])
            assert ok.all()
            worst = max(worst, np.sqrt(e.max()))
            assert np.sqrt(e.max()) <= 1e-6
            g = H.reshape(-1)
            assert abs(np.linalg.norm(g) - 1.0) <= 4e-16 * 9 and g[np.argmax(np.abs(g))] > 0
        lo = ip.h_counts(d["hmodels"], x1, x2, ip.H_THRESHOLD * (1 - ip.MARGIN))
        hi = ip.h_counts(d["hmodels"], x1, x2, ip.H_THRESHOLD * (1 + ip.MARGIN))
        assert np.all(hi - lo <= 0.01 * len(x1))
        assert np.all(lo <= d["hcounts"]) and np.all(d["hcounts"] <= hi)
        assert d["hcounts"].max() > 0 and d["h_best"] == int(np.argmax(d["hcounts"]))
        assert d["h_count"] == d["hcounts"].max() and np.array_equal(d["Hbest"], d["hmodels"][d["h_best"]])
    print(f"a hypothesis maps its own sample to <= {worst:.3g} px")
    n_p = scene["n_p"]
    assert whole["h_count"][ip.PC] >= 0.95 * n_p[ip.PC] and whole["h_count"][ip.PA] <= 0.5 * n_p[ip.PA]


def test_winner_is_as_near_the_true_pose_as_the_restatement(scene, whole):
    g = ip.fixture()
    for p in live(scene):
        d = per_pair(whole, p)
        e = ip.pose_errors(d["R"], d["C"], scene["R_true"][p], scene["C_true"][p])
        assert e[0] <= g["pose_errors"][p][0] + 1e-6 and e[1] <= g["pose_errors"][p][1] + 1e-6
    # pair f: the moved points are exactly the ones not good
    assert np.array_equal(per_pair(whole, ip.PF)["good"], ~scene["moved"])
    assert per_pair(whole, ip.PA)["good"].all()


def blank(d, n, info):
    return (d["info"] == info and np.array_equal(d["R"], np.eye(3)) and not d["C"].any() and not d["counts"].any()
            and d["best"] == 0 and d["n_good"] == 0 and d["median"] == 0 and d["X"].shape == (n, 3)
            and not d["X"].any() and not d["good"].any() and not d["angle"].any() and not d["cands"].any())


def test_too_few_and_degenerate_pairs(scene, whole):
    d = per_pair(whole, ip.PD)
    assert blank(d, 7, -1) and d["h_count"] == 0 and d["h_best"] == -1 and not d["Hbest"].any()
    assert not d["hcounts"].any() and not d["hmodels"].any()
    for p in (ip.PE0, ip.PE1):
        d = per_pair(whole, p)
        assert blank(d, scene["n_p"][p], -2)
        # the homography stage still runs
        assert d["h_best"] >= 0 and d["h_count"] >= 4 and d["h_count"] == d["hcounts"].max()


def test_a_pair_alone_and_all_pairs_permuted_give_the_same_bits(core, scene, whole):
    tab = ip.sample_table()
    for p in (ip.PA, ip.PC, ip.PE0, 7, 10):
        alone = run(core, scene, tab, pairs=[p])
        assert same(per_pair(alone, 0), per_pair(whole, p))
    perm = list(np.random.default_rng(3).permutation(scene["P"]))
    out = run(core, scene, tab, pairs=perm)
    for k, p in enumerate(perm):
        assert same(per_pair(out, k), per_pair(whole, p))


def test_no_homography_table_gives_the_same_pose_outputs(core, scene, whole):
    out = run(core, scene, None)
    pose = [n for n in NAMES if n not in ("h_count", "h_best", "Hbest", "hcounts", "hmodels")]
    for p in range(scene["P"]):
        a = per_pair(out, p)
        assert same(a, per_pair(whole, p), pose)
        assert a["h_count"] == 0 and a["h_best"] == -1 and not a["Hbest"].any()
    assert out["hcounts"].shape == (scene["P"], 0) and out["hmodels"].shape == (scene["P"], 0, 3, 3)


def test_an_appended_hypothesis_that_cannot_win_changes_nothing(core, scene, whole):
    tab = ip.sample_table()
    # hypothesis 0 again, at the end: it ties with the first at best, and the earliest wins
    more = run(core, scene, np.concatenate([tab, tab[:, :1]], axis=1))
    rest = [n for n in NAMES if n not in ("hcounts", "hmodels")]
    for p in range(scene["P"]):
        a, b = per_pair(more, p), per_pair(whole, p)
        assert same(a, b, rest)
        assert np.array_equal(a["hcounts"][:ip.HH], b["hcounts"]) and np.array_equal(a["hmodels"][:ip.HH], b["hmodels"])
        assert a["hcounts"][ip.HH] == a["hcounts"][0] and np.array_equal(a["hmodels"][ip.HH], a["hmodels"][0])


def test_timings_follow_the_layout_of_verify_pairs(core, scene):
    core.set_call_timing(True)
    try:
        run(core, scene, ip.sample_table())
        t = core.last_timings()
    finally:
        core.set_call_timing(False)
    assert len(t) == 4 and np.all(t > 0) and t[3] <= t[1]


def test_store_round_trip_chooses_a_wide_baseline_pair(core):
    import sfm_multiview as mv
    sc = ip.store_scene()
    st = sc["store"]
    st.flag[:] = 0
    verified = mv.verify_pairs(st, H=256, seed=0)
    vorder, pair_ij, vout, i1, i2 = verified
    assert [tuple(q) for q in pair_ij] == [(0, 1), (0, 2), (1, 2), (3, 4)] and np.all(vout[6] >= 0)
    assert tuple(pair_ij[vorder[0]]) == (0, 1)          # the most inliers: the pair without a baseline
    order, eligible, out, pair_start, index1, index2 = mv.init_pairs(st, ip.K, verified, max_reproj=ip.MAX_REPROJ)
    R, C, counts, best, n_good, median, h_count, h_best, Hbest, info, X, good, angle = out
    assert np.array_equal(np.diff(pair_start), vout[2])
    b = int(order[0])
    assert tuple(pair_ij[b]) in ((0, 2), (1, 2)) and eligible[b]
    assert eligible.tolist() == [False, True, True, False]
    assert median[0] < np.deg2rad(4.0) and h_count[0] > 0.8 * vout[2][0] and h_count[3] > 0.8 * vout[2][3]
    print(f"verify order {[tuple(pair_ij[k]) for k in vorder]}, initial-pair order {[tuple(pair_ij[k]) for k in order]}; "
          f"median angles {np.rad2deg(median).round(2).tolist()} deg, h_count / n {(h_count / vout[2]).round(2).tolist()}")
    i, j = pair_ij[b]
    Rt, Ct = sc["R"][j] @ sc["R"][i].T, sc["R"][i] @ (sc["C"][j] - sc["C"][i])
    e_rot, e_dir = ip.pose_errors(R[b], C[b], Rt, Ct)
    print(f"chosen pair {(i, j)}: rotation error {e_rot:.3g} rad, direction error {e_dir:.3g} rad")
    # the chosen pair's good points seed the triangulation of the store
    s, e = pair_start[b], pair_start[b + 1]
    g = good[s:e]
    assert g.sum() >= 30
    st.flag[index1[s:e][g]] = 1
    st.flag[index2[s:e][g]] = 1
    rows, Xt, cost, front, tinfo = mv.triangulate_store(st, ip.K, [np.zeros(3), C[b]], [np.eye(3), R[b]], images=[i, j])
    assert np.array_equal(rows, st.feature[index1[s:e][g]]) and front.all()
    P2 = ip.K @ np.column_stack([R[b], -R[b] @ C[b]])
    x1 = np.column_stack([st.x[index1[s:e][g]], st.y[index1[s:e][g]]])
    x2 = np.column_stack([st.x[index2[s:e][g]], st.y[index2[s:e][g]]])
    assert np.sqrt(ip.reproj2(ip.P1, Xt, x1).max()) < ip.MAX_REPROJ
    assert np.sqrt(ip.reproj2(P2, Xt, x2).max()) < ip.MAX_REPROJ
    st.flag[:] = 0
