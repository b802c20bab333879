"""Multi-view track triangulation on a real MI355X (sfm_triangulate_tracks)
against tests/golden/multiview.npz and against the two-view entry points.

Bounds: two-view tracks are sfm_triangulate_dlt's and
sfm_triangulate_nonlinear's bits, within 1e-9 of the reference's linear
points and equal to its refined ones (the existing bounds of
test_gpu_parity.py); the N-view DLT within the project's DLT bound (relative
error <= 1e-9, `rel` as in test_gpu_parity.py) of numpy's SVD; the refined
cost never above the linear point's (exact: only decreasing steps are
accepted) and at most 1e-7 relative above the converged minimum's (ten units
of the ftol = 1e-8 stop rule); front and cost against numpy at the returned X
(exactly, and to 1e-12 relative).  The fixture's generator asserts the
conditioning and the margins that make these comparisons cover every track.
"""
import os
import re

import numpy as np
import pytest

import test_multiview as tm
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu
K = tm.K
# Distance of the refined X from the converged minimum: LM's stop rules leave
# the iterate short of it by an amount that depends on curvature.  Measured
# on the MI355X over the fixture's 771 tracks of 3 / 5 / 8 views: 6.02e-7
# (largest |X - X_min|: v3 6.02e-7, v5 2.32e-7, v8 4.76e-7; scene extent ~8).
# The bound is ten times that.
DIST_MEASURED = 6.02e-7
DIST_BOUND = 10 * DIST_MEASURED


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "multiview.npz"))


@pytest.fixture(scope="module")
def cases():
    return {name: tm.load_problem(name) for name in tm.CASES}


def run(core, c, **kw):
    return core.triangulate_tracks(c["P"], c["track_start"], c["obs_cam"], c["obs_xy"], **kw)


@pytest.fixture(scope="module")
def results(core, cases):
    """name -> (linear outputs, linear-then-refined outputs), computed once"""
    return {name: (run(core, c, refine=False), run(core, c)) for name, c in cases.items()}


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def pairs(c):
    cam = c["obs_cam"].reshape(-1, 2)
    xy = c["obs_xy"].reshape(-1, 2, 2)
    for a, b in sorted({tuple(p) for p in cam}):
        sel = np.where((cam[:, 0] == a) & (cam[:, 1] == b))[0]
        yield a, b, sel, np.ascontiguousarray(xy[sel, 0]), np.ascontiguousarray(xy[sel, 1])


def test_two_view_tracks_are_the_two_view_kernels_bits(core, cases, gold, results):
    c = cases["v2"]
    (Xl, _, _, il), (Xr, _, _, ir) = results["v2"]
    seen = 0
    for a, b, sel, x1, x2 in pairs(c):
        X0 = core.triangulate(c["P"][a], c["P"][b], x1, x2)
        assert np.array_equal(Xl[sel], X0), (a, b)
        Xn, info = core.triangulate_nonlinear(c["P"][a], c["P"][b], x1, x2, X0)
        assert np.array_equal(Xr[sel], Xn) and np.array_equal(ir[sel], info), (a, b)
        seen += len(sel)
    assert seen == c["T"] and np.all(il == 0) and np.all(ir >= 1)
    r = tm.rel(Xl, gold["v2_X_lin"])
    print(f"v2 linear vs reference: rel {r:.3g}")
    assert r <= 1e-9
    # from the reference's linear points: the reference's refined points
    Xo, _, _, io = run(core, c, X0=gold["v2_X_lin"], refine="only")
    assert np.array_equal(Xo, gold["v2_X_nl"]) and np.all(io >= 1)


@pytest.mark.parametrize("name", tm.NVIEW)
def test_linear_matches_numpy_svd(gold, results, name):
    X, _, _, info = results[name][0]
    r = tm.rel(X, gold[f"{name}_X_lin"])
    print(f"{name} linear vs numpy SVD: rel {r:.3g}")
    assert r <= 1e-9
    assert np.all(info == 0)


@pytest.mark.parametrize("name", tm.NVIEW)
def test_refined_cost(gold, results, name):
    (_, cl, _, _), (_, cr, _, info) = results[name]
    assert np.all(cr <= cl)  # exact: only decreasing steps are accepted
    excess = (cr - gold[f"{name}_cost_min"]) / gold[f"{name}_cost_min"]
    print(f"{name} refined cost over the converged minimum: max relative {excess.max():.3g}, stop codes "
          f"{np.bincount(info, minlength=6)[1:]}")
    assert np.all(cr <= gold[f"{name}_cost_min"] * (1 + 1e-7))
    assert np.all((info >= 1) & (info <= 4))  # none ran out of evaluations


def refined_distance(gold, results):
    return {name: float(np.abs(results[name][1][0] - gold[f"{name}_X_min"]).max()) for name in tm.NVIEW}


def test_refined_point_distance(gold, results):
    """Largest |X - X_min| over the fixture, measured on the MI355X: 6.02e-7;
    the bound is ten times that, 6.02e-6 (see DIST_BOUND above)."""
    d = refined_distance(gold, results)
    print("refined X from the converged minimum:", {k: f"{v:.3g}" for k, v in d.items()})
    assert max(d.values()) <= DIST_BOUND


@pytest.mark.parametrize("name", list(tm.CASES))
def test_front_and_cost_against_numpy(core, cases, results, name):
    c = cases[name]
    Pn = c["P"].copy()
    Pn[0] = -Pn[0]  # the same image points, camera 0 looking away: h2 < 0 for its views
    flipped = core.triangulate_tracks(Pn, c["track_start"], c["obs_cam"], c["obs_xy"])
    n_back = 0
    for P, outs in ((c["P"], results[name][0]), (c["P"], results[name][1]), (Pn, flipped)):
        X, cst, front, _ = outs
        assert front.dtype == bool
        for t in range(c["T"]):
            cams, xy = tm.track(c, t)
            assert front[t] == bool(np.all(tm.depths(P, cams, X[t]) > 0)), t
            want = tm.cost(P, cams, xy, X[t])
            assert abs(cst[t] - want) <= 1e-12 * want, (t, cst[t], want)
        n_back += int((~front).sum())
    assert np.all(results[name][1][2]) and n_back > 0  # both values of the bit occur


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_track_counts_around_the_wave_and_block(core, cases, results, T):
    for name in ("v2", "v5"):
        c = cases[name]
        n = c["track_start"][T]
        for k, kw in enumerate((dict(refine=False), dict())):
            out = core.triangulate_tracks(c["P"], c["track_start"][:T + 1], c["obs_cam"][:n], c["obs_xy"][:n], **kw)
            assert same(out, [a[:T] for a in results[name][k]])


def mixed_launch(cases):
    """65 tracks of 0, 1, 2, 3 and 8 views in turn over one camera set (the
    three cases' cameras side by side), so every wave holds every kind."""
    P = np.concatenate([cases[n]["P"] for n in ("v2", "v3", "v8")])
    off = {"v2": 0, "v3": len(cases["v2"]["P"]), "v8": len(cases["v2"]["P"]) + len(cases["v3"]["P"])}
    cams, xys, lens = [], [], []
    for i in range(65):
        kind = i % 5
        if kind == 0:
            lens.append(0)
            continue
        name = {1: "v3", 2: "v2", 3: "v3", 4: "v8"}[kind]
        cam, xy = tm.track(cases[name], i)
        if kind == 1:
            cam, xy = cam[:1], xy[:1]
        cams.append(cam + off[name])
        xys.append(xy)
        lens.append(len(cam))
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return P, start, np.concatenate(cams).astype(np.int32), np.concatenate(xys), np.array(lens)


def test_mixed_track_lengths_equal_single_launches(core, cases):
    P, start, cam, xy, lens = mixed_launch(cases)
    rng = np.random.default_rng(1)
    X0 = rng.normal(0, 1, (len(lens), 3)) + [0, 0, 6]
    for kw in (dict(refine=False), dict(), dict(X0=X0, refine="only"), dict(X0=X0, refine=False)):
        X, cst, front, info = core.triangulate_tracks(P, start, cam, xy, **kw)
        short = lens < 2
        assert np.all(info[short] == -2) and np.all(info[~short] >= (0 if kw.get("refine") is False else 1))
        assert np.all(cst[short] == 0) and not front[short].any()
        assert np.array_equal(X[short], X0[short] if "X0" in kw else np.zeros((short.sum(), 3)))
        for t in range(len(lens)):
            s, e = start[t], start[t + 1]
            alone = dict(kw)
            if "X0" in kw:
                alone["X0"] = X0[t:t + 1]
            one = core.triangulate_tracks(P, [0, e - s], cam[s:e], xy[s:e], **alone)
            assert same(one, (X[t:t + 1], cst[t:t + 1], front[t:t + 1], info[t:t + 1])), (kw.get("refine"), t)


def test_projections_in_lds_and_in_global_memory_agree(core, cases, results):
    cap = int(re.search(r"#define SFM_TRACKS_LDS_CAMS (\d+)", open(os.path.join(REPO, "include", "sfmcore.h")).read())[1])
    assert cap % 8 == 0
    rng = np.random.default_rng(2)
    for name in ("v2", "v8"):
        c = cases[name]
        spread = cap // 8  # the case's cameras spread over the staged rows, the last row included
        idx = np.arange(len(c["P"])) * spread + (spread - 1)
        outs = []
        for n_cams in (cap, cap + 1):
            P = rng.normal(0, 1, (n_cams, 3, 4))
            P[idx] = c["P"]
            outs.append([core.triangulate_tracks(P, c["track_start"], idx[c["obs_cam"]], c["obs_xy"], **kw)
                         for kw in (dict(refine=False), dict())])
        for k in range(2):
            assert same(outs[0][k], outs[1][k]) and same(outs[0][k], results[name][k])


def test_nan_start_is_kept(core, cases):
    for name in ("v2", "v3"):
        c = cases[name]
        T = 70
        n = c["track_start"][T]
        X0 = run(core, c, refine=False)[0][:T].copy()
        X0[[3, 64, 69], [0, 1, 2]] = np.nan
        X, cst, front, info = core.triangulate_tracks(c["P"], c["track_start"][:T + 1], c["obs_cam"][:n],
                                                      c["obs_xy"][:n], X0=X0, refine="only")
        bad = np.isnan(X0).any(1)
        assert bad.sum() == 3 and np.all(info[bad] == -1) and np.all(info[~bad] >= 1)
        assert np.array_equal(X[bad], X0[bad], equal_nan=True) and np.isfinite(X[~bad]).all()
        assert not front[bad].any()


def test_store_path_equals_raw_call(core):
    import sfm_synthetic as syn
    from sfm_io import MatchStore
    from sfm_multiview import triangulate_store
    n_cams, n_pts, k = syn.BA_CONFIGS["cfg3"]
    p = syn.ba_problem(n_cams, n_pts, k, seed=3, dense=False)
    feat = p["pt_idx"].astype(np.int32)
    store = MatchStore(n_pts, n_cams, feat, p["cam_idx"], p["obs"][:, 0].copy(), p["obs"][:, 1].copy())
    store.flag[:] = 1
    store.flag[store._row_start[7]] = 0      # feature 7 keeps 4 views
    store.flag[store._row_start[9]:store._row_start[10] - 1] = 0  # feature 9 keeps one: no track
    P = np.stack([tm.projection(K, C, R) for C, R in zip(p["C_true"], p["R_true"])])
    rows, start, cam, xy = store.tracks(range(n_cams))
    assert len(rows) == n_pts - 1 and 9 not in rows and start[8] - start[7] == 4
    for refine in (False, True):
        got = triangulate_store(store, K, p["C_true"], p["R_true"], refine=refine)
        assert np.array_equal(got[0], rows)
        assert same(got[1:], core.triangulate_tracks(P, start, cam, xy, refine=refine))
    # a subset of the images, cameras given for those images only
    sub = [1, 2, 4, 5]
    got = triangulate_store(store, K, p["C_true"][sub], p["R_true"][sub], images=sub)
    rows, start, cam, xy = store.tracks(sub)
    assert np.array_equal(got[0], rows) and len(rows) > 0
    assert same(got[1:], core.triangulate_tracks(P[sub], start, cam, xy))
    assert np.median(np.abs(got[1] - p["X_true"][rows]).max(1)) < 0.1  # the points are the scene's
