"""Robust track triangulation on a real MI355X (sfm_triangulate_tracks_robust)
against sfm_triangulate_tracks on the cleaned tracks, against
tests/golden/robust_tracks.npz and against itself under every mapping.

Everything here is equality, bit for bit, except where a quantity is
recomputed in numpy at the returned X: the angle, and the cost of a track
without consensus, both at the project's bound for that, 1e-12 relative.  The
fixture's generator asserts the margins that keep every count away from
rounding.
"""
import os
import re

import numpy as np
import pytest

import test_multiview as tm
import test_robust_tracks as tr
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu
K = tm.K


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "robust_tracks.npz"))


@pytest.fixture(scope="module")
def cases():
    return {name: tr.load_case(name) for name in tr.CASES}


def run(core, c, **kw):
    kw.setdefault("centres", c["C"])
    return core.triangulate_tracks_robust(c["P"], c["track_start"], c["obs_cam"], c["obs_xy"], **kw)


@pytest.fixture(scope="module")
def results(core, cases):
    """name -> the robust call's outputs at the defaults, computed once"""
    return {name: run(core, c) for name, c in cases.items()}


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["v2", "v3", "v5", "v8"])
def test_clean_tracks_are_the_plain_calls_bits(core, name):
    c = tm.load_problem(name)
    Xp, cp, _, ip = core.triangulate_tracks(c["P"], c["track_start"], c["obs_cam"], c["obs_xy"])
    X, cst, n_inl, inl, pair, count, info, angle = run(core, c)
    assert inl.all() and np.all(n_inl == c["k"]) and np.all(count == c["k"]) and np.all(pair >= 0)
    assert np.array_equal(X, Xp) and np.array_equal(info, ip) and np.array_equal(cst, cp)


@pytest.mark.parametrize("name", list(tr.CASES))
def test_contaminated_tracks_equal_the_cleaned_call(core, cases, gold, results, name):
    c = cases[name]
    kept = gold[f"{name}_kept"]
    X, cst, n_inl, inl, _, _, info, _ = results[name]
    k = c["k"]
    obs_kept = np.repeat(kept, k)
    assert np.array_equal(inl[obs_kept], c["truth"][obs_kept])
    assert np.all(n_inl[kept] == k - c["n_out"])
    start, cam, xy = tr.cleaned(c, c["truth"])
    Xc, cc, _, ic = core.triangulate_tracks(c["P"], start, cam, xy)
    assert np.array_equal(X[kept], Xc[kept]) and np.array_equal(cst[kept], cc[kept])
    assert np.array_equal(info[kept], ic[kept]) and np.all(info[kept] >= 1)


@pytest.mark.parametrize("name", list(tr.CASES))
def test_winner(core, cases, gold, results, name):
    c = cases[name]
    _, _, _, _, pair, count, _, _ = results[name]
    assert np.array_equal(count, gold[f"{name}_best_count"])
    table = core.track_pairs(c["k"], tr.MAX_PAIRS)
    assert np.all((pair >= 0) & (pair < len(table)))
    cam, xy = c["obs_cam"].reshape(-1, c["k"]), c["obs_xy"].reshape(-1, c["k"], 2)
    for i, j in sorted({tuple(p) for p in table[pair]}):
        sel = np.where((table[pair][:, 0] == i) & (table[pair][:, 1] == j))[0]
        for a, b in sorted({(cam[t, i], cam[t, j]) for t in sel}):
            s2 = sel[(cam[sel, i] == a) & (cam[sel, j] == b)]
            Xh = core.triangulate(c["P"][a], c["P"][b], np.ascontiguousarray(xy[s2, i]),
                                  np.ascontiguousarray(xy[s2, j]))
            for t, X in zip(s2, Xh):
                assert tr.inlier_mask(c["P"], cam[t], xy[t], X).sum() == count[t], t


def test_bits_do_not_depend_on_the_lanes_per_track(core, cases, results):
    for name in ("r3o1", "r8o3", "r20o6"):
        for lanes in (1, 4, 16, 64):
            assert same(run(core, cases[name], lanes_per_track=lanes), results[name]), (name, lanes)


def test_projections_in_lds_and_in_global_memory_agree(core, cases, results):
    cap = int(re.search(r"#define SFM_TRACKS_LDS_CAMS (\d+)", open(os.path.join(REPO, "include", "sfmcore.h")).read())[1])
    rng = np.random.default_rng(2)
    for name in ("r5o2", "r8o3"):
        c = cases[name]
        spread = cap // 8  # the case's cameras spread over the staged rows, the last row included
        idx = np.arange(len(c["P"])) * spread + (spread - 1)
        outs = []
        for n_cams in (cap, cap + 1):
            P, C = rng.normal(0, 1, (n_cams, 3, 4)), rng.normal(0, 1, (n_cams, 3))
            P[idx], C[idx] = c["P"], c["C"]
            outs.append(core.triangulate_tracks_robust(P, c["track_start"], idx[c["obs_cam"]], c["obs_xy"], centres=C))
        assert same(outs[0], outs[1]) and same(outs[0], results[name])


def track_outputs(out, c, t):
    s, e = c["track_start"][t], c["track_start"][t + 1]
    return [a[s:e] if i == 3 else a[t:t + 1] for i, a in enumerate(out)]


def test_alone_in_the_batch_and_permuted(core, cases, results):
    c, out = cases["r8o3"], results["r8o3"]
    k = c["k"]
    for t in (0, 63, 64, 256):
        s, e = c["track_start"][t], c["track_start"][t + 1]
        one = core.triangulate_tracks_robust(c["P"], [0, e - s], c["obs_cam"][s:e], c["obs_xy"][s:e], centres=c["C"])
        assert same(one, track_outputs(out, c, t)), t
    perm = np.random.default_rng(3).permutation(c["T"])
    obs = (perm[:, None] * k + np.arange(k)).reshape(-1)
    got = core.triangulate_tracks_robust(c["P"], c["track_start"], c["obs_cam"][obs], c["obs_xy"][obs], centres=c["C"])
    assert same(got, [a[obs] if i == 3 else a[perm] for i, a in enumerate(out)])


def ragged_batch(cases):
    """Tracks of 0, 1, 2, 3, 16, 17, 20 and 70 views cut from (or, for 70,
    repeated out of) the 20-view case's clean observations, plus one track of
    three mutually inconsistent observations"""
    c = cases["r20o6"]
    cams, xys, lens = [], [], []
    for t, n in enumerate((0, 1, 2, 3, 16, 17, 20, 70, 3, 0, 20, 2)):
        cam, _ = tm.track(c, t)
        xy = c["clean_xy"][c["track_start"][t]:c["track_start"][t + 1]]
        reps = -(-n // len(cam)) if n else 1
        cam, xy = np.tile(cam, reps)[:n], np.tile(xy, (reps, 1))[:n]
        if t == 8:
            xy = xy + np.array([[0.0, 0.0], [300.0, -200.0], [-250.0, 400.0]])
        cams.append(cam)
        xys.append(xy)
        lens.append(n)
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return c, start, np.concatenate(cams).astype(np.int32), np.concatenate(xys), np.array(lens)


def test_ragged_and_edge_shapes(core, cases):
    c, start, cam, xy, lens = ragged_batch(cases)
    outs = {lanes: core.triangulate_tracks_robust(c["P"], start, cam, xy, min_inliers=3, centres=c["C"],
                                                  lanes_per_track=lanes) for lanes in (0, 1, 8, 64)}
    for lanes in (1, 8, 64):
        assert same(outs[lanes], outs[0]), lanes
    X, cst, n_inl, inl, pair, count, info, angle = outs[0]
    short = lens < 2
    assert np.all(info[short] == -2) and np.all(pair[short] == -1) and np.all(count[short] == 0)
    assert np.all(X[short] == 0) and np.all(cst[short] == 0) and np.all(n_inl[short] == 0) and np.all(angle[short] == 0)
    assert not inl[start[1]:start[2]].any()
    # two views cannot reach min_inliers = 3
    two = lens == 2
    assert np.all(info[two] == -3) and np.all(count[two] == 2) and np.all(pair[two] == 0)
    # clean tracks of 3 to 70 views: every observation an inlier, the plain call's bits
    clean = (lens >= 3) & (np.arange(len(lens)) != 8)
    Xp, cp, _, ip = core.triangulate_tracks(c["P"], start, cam, xy)
    assert np.all(n_inl[clean] == lens[clean]) and np.all(count[clean] == lens[clean]) and np.all(info[clean] >= 1)
    assert np.array_equal(X[clean], Xp[clean]) and np.array_equal(cst[clean], cp[clean])
    assert np.array_equal(info[clean], ip[clean])
    assert inl[np.repeat(clean, lens)].all()
    # the cap: 17, 20 and 70 views have more than 120 pairs, and the winner is among the first 120
    assert np.all(pair[clean] >= 0) and np.all(pair[clean] < np.minimum(lens[clean] * (lens[clean] - 1) // 2, 120))
    capped = core.triangulate_tracks_robust(c["P"], start, cam, xy, min_inliers=3, centres=c["C"], max_pairs=1)
    assert np.all(capped[4][~short] == 0) and np.all(capped[5] <= count)
    # three mutually inconsistent observations: no consensus, the documented outputs
    t = 8
    s, e = start[t], start[t + 1]
    assert info[t] == -3 and count[t] < 3 and n_inl[t] == count[t] == inl[s:e].sum()
    i, j = core.track_pairs(3)[pair[t]]
    Xh = core.triangulate(c["P"][cam[s + i]], c["P"][cam[s + j]], xy[s + i:s + i + 1], xy[s + j:s + j + 1])[0]
    assert np.array_equal(X[t], Xh)
    assert np.array_equal(inl[s:e], tr.inlier_mask(c["P"], cam[s:e], xy[s:e], Xh))
    e2 = tr.errors2(c["P"], cam[s:e], xy[s:e], Xh)[0][inl[s:e]]
    assert abs(cst[t] - e2.sum()) <= 1e-12 * e2.sum()


def test_two_view_winner_returns_the_two_view_kernels_bits(core, cases, gold, results):
    c = cases["r3o1"]
    kept = gold["r3o1_kept"]
    X, _, n_inl, inl, _, _, info, _ = results["r3o1"]
    cam, xy = c["obs_cam"].reshape(-1, 3), c["obs_xy"].reshape(-1, 3, 2)
    m = inl.reshape(-1, 3)
    seen = 0
    for t in np.where(kept)[0]:
        assert n_inl[t] == 2
        a, b = np.where(m[t])[0]
        x1, x2 = xy[t, a][None], xy[t, b][None]
        X0 = core.triangulate(c["P"][cam[t, a]], c["P"][cam[t, b]], x1, x2)
        Xn, i2 = core.triangulate_nonlinear(c["P"][cam[t, a]], c["P"][cam[t, b]], x1, x2, X0)
        assert np.array_equal(X[t], Xn[0]) and info[t] == i2[0], t
        seen += 1
    assert seen >= 250


def test_angle(core, cases, results):
    for name in ("r3o1", "r8o3"):
        c = cases[name]
        X, _, _, inl, _, _, _, angle = results[name]
        for t in range(c["T"]):
            cams, _ = tm.track(c, t)
            m = inl[c["track_start"][t]:c["track_start"][t + 1]]
            want = tr.max_angle(c["C"], cams[m], X[t])
            assert abs(angle[t] - want) <= 1e-12 * want, (t, angle[t], want)
        out = run(core, c, centres=None)
        assert out[7] is None and same(out[:7], results[name][:7])


def test_store_round_trip(core, cases, results):
    from sfm_multiview import triangulate_store, triangulate_store_robust
    c = cases["r5o1"]
    store = tr.contaminated_store(c)
    rows, out, keep = triangulate_store_robust(store, K, c["C"], c["R"], update_flags=True)
    assert np.array_equal(rows, np.arange(c["T"])) and keep.all()
    want = core.triangulate_tracks_robust(c["P"], c["track_start"], c["obs_cam"], c["obs_xy"], min_inliers=3,
                                          centres=c["C"])
    assert same(out, want) and np.array_equal(out[3], c["truth"])
    rows2, start2, cam2, xy2 = store.tracks(range(len(c["P"])))
    start, cam, xy = tr.cleaned(c, c["truth"])
    assert np.array_equal(rows2, rows) and np.array_equal(start2, start)
    assert np.array_equal(cam2, cam) and np.array_equal(xy2, xy)
    assert np.array_equal(triangulate_store(store, K, c["C"], c["R"])[1], out[0])
