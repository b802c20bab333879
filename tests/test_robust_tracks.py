"""Robust track triangulation, CPU half: the pair enumeration, the numpy
restatement of the algorithm (tests/golden/make_golden_robust_tracks.py)
against tests/golden/robust_tracks.npz, the C-ABI's argument checks, the
store index of MatchStore.tracks and the flag update of
sfm_multiview.triangulate_store_robust.  The GPU half is
tests/test_robust_tracks_gpu.py; it shares the helpers here.
"""
import os
import re
import sys

import numpy as np
import pytest

import sfm_synthetic as syn
import test_multiview as tm
from conftest import GOLDEN, REPO

K = tm.K
THRESHOLD = 4.0
MAX_PAIRS = 120
N_TRACKS = 257
# name: (n_cams, views per track, displaced observations per track, seed)
CASES = {"r3o1": (6, 3, 1, 21), "r5o1": (7, 5, 1, 22), "r5o2": (7, 5, 2, 23), "r8o3": (8, 8, 3, 24),
         "r20o6": (24, 20, 6, 25)}


def load_case(name):
    """The contaminated tracks of one case, regenerated from its seed: the
    clean observations of sfm_synthetic.ba_problem under the true cameras,
    n_out of every track's observations displaced by 40-120 px in a random
    direction (default_rng(seed)); ``truth`` marks the untouched ones."""
    n_cams, k, n_out, seed = CASES[name]
    p = syn.ba_problem(n_cams, N_TRACKS, k, seed=seed, dense=False)
    P = np.stack([tm.projection(K, C, R) for C, R in zip(p["C_true"], p["R_true"])])
    rng = np.random.default_rng(seed)
    pos = np.argsort(rng.random((N_TRACKS, k)), axis=1)[:, :n_out]
    mag = rng.uniform(40.0, 120.0, (N_TRACKS, n_out))
    ang = rng.uniform(0.0, 2.0 * np.pi, (N_TRACKS, n_out))
    truth = np.ones((N_TRACKS, k), dtype=bool)
    truth[np.arange(N_TRACKS)[:, None], pos] = False
    xy = p["obs"].reshape(N_TRACKS, k, 2).copy()
    xy[np.arange(N_TRACKS)[:, None], pos] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=-1)
    return dict(P=P, C=p["C_true"], R=p["R_true"], track_start=np.arange(N_TRACKS + 1, dtype=np.int64) * k,
                obs_cam=p["cam_idx"].astype(np.int32), obs_xy=np.ascontiguousarray(xy.reshape(-1, 2)),
                clean_xy=p["obs"], truth=truth.reshape(-1), k=k, n_out=n_out, T=N_TRACKS, X_true=p["X_true"])


def pairs(n, max_pairs=MAX_PAIRS):
    """View pairs by decreasing index gap, i ascending within a gap, cut off"""
    out = []
    for g in range(n - 1, 0, -1):
        for i in range(n - g):
            out.append((i, i + g))
    return out[:max_pairs]


def errors2(P, cams, xy, X):
    """Per observation the squared reprojection error of X and the depth h2"""
    h = np.einsum("nij,j->ni", P[cams], np.append(X, 1.0))
    with np.errstate(all="ignore"):
        e2 = (xy[:, 0] - h[:, 0] / h[:, 2]) ** 2 + (xy[:, 1] - h[:, 1] / h[:, 2]) ** 2
    return e2, h[:, 2]


def inlier_mask(P, cams, xy, X, threshold=THRESHOLD):
    if not np.all(np.isfinite(X)):
        return np.zeros(len(cams), dtype=bool)
    e2, h2 = errors2(P, cams, xy, X)
    return (h2 > 0) & ~(np.abs(h2) < 1e-8) & (e2 < threshold * threshold)


def cleaned(c, mask):
    """The case's CSR with the observations outside ``mask`` removed"""
    per = np.add.reduceat(mask.astype(np.int64), c["track_start"][:-1])
    start = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    return start, c["obs_cam"][mask], c["obs_xy"][mask]


def max_angle(C, cams, X):
    """Largest angle between the rays X - C_i, X - C_j, by atan2"""
    best = 0.0
    for a in range(len(cams)):
        for b in range(a + 1, len(cams)):
            ra, rb = X - C[cams[a]], X - C[cams[b]]
            best = max(best, float(np.arctan2(np.linalg.norm(np.cross(ra, rb)), ra @ rb)))
    return best


def generator():
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden_robust_tracks
    return make_golden_robust_tracks


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "robust_tracks.npz"))


@pytest.mark.parametrize("n", [2, 3, 16, 17, 20])
def test_pair_enumeration(n):
    import _sfmcore as core
    got = core.track_pairs(n, MAX_PAIRS)
    total = n * (n - 1) // 2
    assert got.shape == (min(total, MAX_PAIRS), 2) and got.dtype == np.int64
    assert np.array_equal(got, np.array(pairs(n), dtype=np.int64).reshape(-1, 2))
    i, j = got[:, 0], got[:, 1]
    assert np.all(i < j) and np.all(i >= 0) and np.all(j < n) and tuple(got[0]) == (0, n - 1)
    gap = j - i
    assert np.all(np.diff(gap) <= 0)  # widest first
    same = np.diff(gap) == 0
    assert np.all(np.diff(i)[same] == 1) and np.all(i[1:][~same] == 0)  # i ascending from 0 within a gap
    assert len({(a, b) for a, b in got}) == len(got)
    # the kernel's decoding of a pair's number k: level m holds the m pairs of gap n - m
    for k, (a, b) in enumerate(got):
        m = 1
        while m * (m + 1) // 2 <= k:
            m += 1
        assert (a, b) == (k - m * (m - 1) // 2, k - m * (m - 1) // 2 + n - m)
    if n == 20:
        assert total == 190 and len(got) == 120 and len(core.track_pairs(n, 1000)) == 190
    if n == 17:
        assert total == 136 and len(got) == 120
    if n == 16:
        assert total == len(got) == 120  # the default cap tries every pair up to 16 views


def test_fixture_conditions(gold):
    for name, (_, k, n_out, _) in CASES.items():
        c = load_case(name)
        kept = gold[f"{name}_kept"]
        mask, truth = gold[f"{name}_mask"].reshape(N_TRACKS, k), c["truth"].reshape(N_TRACKS, k)
        assert np.array_equal(gold[f"{name}_truth"], c["truth"])
        assert np.array_equal(mask[kept], truth[kept])
        assert len(kept) == N_TRACKS and (kept.sum() >= 250 if name == "r3o1" else kept.all())
        assert float(gold[f"{name}_final_margin"]) >= 1.0
        assert float(gold[f"{name}_hyp_margin"]) >= 1e-6
        assert np.all(gold[f"{name}_best_count"][kept] >= k - n_out)
        disp = np.linalg.norm(c["obs_xy"] - c["clean_xy"], axis=1)
        assert np.all(disp[c["truth"]] == 0) and np.all((disp[~c["truth"]] >= 40 - 1e-9) & (disp[~c["truth"]] <= 120 + 1e-9))
        assert np.all((~truth).sum(1) == n_out)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_against_fixture(gold, name):
    """The numpy restatement, run again on a spread of tracks: the final
    mask and the largest hypothesis count are the fixture's; and the kernel's
    linear stage restated in numpy (streamed Givens, one-sided Jacobi) on the
    final inliers is within the project's DLT bound, 1e-9 relative, of the
    restatement's SVD point, the fixture's and this run's."""
    g = generator()
    c = load_case(name)
    k = c["k"]
    worst = 0.0
    for t in range(0, N_TRACKS, 16):
        cams, xy = tm.track(c, t)
        r = g.restate_track(c["P"], cams, xy, THRESHOLD, MAX_PAIRS, 2)
        assert np.array_equal(r["mask"], gold[f"{name}_mask"][t * k:(t + 1) * k]), t
        assert r["best_count"] == gold[f"{name}_best_count"][t]
        if r["mask"].sum() >= 3:
            X = tm.givens_dlt(c["P"], cams[r["mask"]], xy[r["mask"]])
            worst = max(worst, np.abs(X - gold[f"{name}_X_lin"][t]).max(), np.abs(r["X_lin"] - X).max())
    assert worst / np.abs(gold[f"{name}_X_lin"]).max() <= 1e-9


def test_symbol_declared_in_header():
    txt = open(os.path.join(REPO, "include", "sfmcore.h")).read()
    assert re.search(r"\bint sfm_triangulate_tracks_robust\s*\(", txt)
    import _sfmcore
    assert hasattr(_sfmcore._lib, "sfm_triangulate_tracks_robust") and _sfmcore.version() == 1


def small_problem():
    c = load_case("r5o1")
    return c["P"], c["C"], c["track_start"][:5], c["obs_cam"][:20], c["obs_xy"][:20]


def test_bad_arguments_raise():
    import _sfmcore as core
    P, C, ts, cam, xy = small_problem()
    call = core.triangulate_tracks_robust
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(core.SfmCoreError, match="argument: threshold"):
            call(P, ts, cam, xy, threshold=thr)
    with pytest.raises(core.SfmCoreError, match="argument: max_pairs"):
        call(P, ts, cam, xy, max_pairs=0)
    with pytest.raises(core.SfmCoreError, match="argument: min_inliers"):
        call(P, ts, cam, xy, min_inliers=1)
    with pytest.raises(core.SfmCoreError, match="argument: max_nfev"):
        call(P, ts, cam, xy, max_nfev=0)
    for lanes in (3, 6, 128, -1):
        with pytest.raises(core.SfmCoreError, match="argument: lanes_per_track"):
            call(P, ts, cam, xy, lanes_per_track=lanes)
    bad = {"starts at 0": ts + 1, "decreases": np.array([0, 10, 5, 15, 20]), "end": np.array([0, 5, 10, 15, 19])}
    for what, t in bad.items():
        with pytest.raises(core.SfmCoreError, match="argument: track_start"):
            call(P, t, cam, xy)
    for v in (-1, len(P), 2 ** 31 - 1):
        cb = cam.copy()
        cb[7] = v
        with pytest.raises(core.SfmCoreError, match="argument: camera index"):
            call(P, ts, cb, xy, centres=C)
    with pytest.raises(ValueError):
        call(P, ts, cam, xy[:5])
    with pytest.raises(ValueError):
        call(P, ts, cam, xy, centres=C[:3])


def raw_call(core, P, C, ts, cam, xy, angle, threshold=4.0, lanes=0):
    T = len(ts) - 1
    return core._lib.sfm_triangulate_tracks_robust(
        core._p(P.reshape(-1, 12)), len(P), core._p(C) if C is not None else None, core._p(ts, core._i64), T,
        core._p(cam, core._i32), core._p(xy), len(cam), threshold, 120, 2, 50, lanes, None, None, None, None, None,
        None, None, core._p(angle) if angle is not None else None, 0)


def test_raw_abi_rejects_before_any_device_work():
    """The C entry itself, with every output null: SFM_ERR_ARG (-1)"""
    import _sfmcore as core
    P, C, ts, cam, xy = small_problem()
    C = np.ascontiguousarray(C, dtype=np.float64)
    # angle without centres: the binding cannot express it
    assert raw_call(core, P, None, ts, cam, xy, np.zeros(4)) == -1
    assert b"angle needs centres" in core._lib.sfm_last_error()
    assert raw_call(core, P, C, ts + 1, cam, xy, None) == -1 and b"track_start" in core._lib.sfm_last_error()
    cb = cam.copy()
    cb[3] = len(P)
    assert raw_call(core, P, C, ts, cb, xy, None) == -1 and b"camera index" in core._lib.sfm_last_error()
    assert raw_call(core, P, C, ts, cam, xy, None, lanes=12) == -1 and b"lanes_per_track" in core._lib.sfm_last_error()
    assert raw_call(core, P, C, ts, cam, xy, None, threshold=float("nan")) == -1


def test_no_tracks_returns_empty_without_device(monkeypatch):
    import _sfmcore as core
    monkeypatch.setattr(core, "_DEVICE_SEEN", False)
    monkeypatch.setattr(core._lib, "sfm_device_count", lambda: 0)
    for centres in (None, np.zeros((0, 3))):
        out = core.triangulate_tracks_robust(np.zeros((0, 3, 4)), [0], [], np.zeros((0, 2)), centres=centres)
        X, cst, n_inl, inl, pair, count, info, angle = out
        assert X.shape == (0, 3) and cst.shape == (0,) and inl.shape == (0,) and inl.dtype == bool
        for a in (n_inl, pair, count, info):
            assert a.shape == (0,) and a.dtype == np.int32
        assert angle is None if centres is None else angle.shape == (0,)


def test_device_step_fails_loudly_without_gpu(monkeypatch):
    import _sfmcore as core
    monkeypatch.setattr(core, "_DEVICE_SEEN", False)
    monkeypatch.setattr(core._lib, "sfm_device_count", lambda: 0)
    P, C, ts, cam, xy = small_problem()
    with pytest.raises(core.SfmCoreError):
        core.triangulate_tracks_robust(P, ts, cam, xy)


@pytest.mark.parametrize("images", [[0, 1], [0, 1, 2, 3, 4], [1, 3]])
def test_tracks_index_equals_dense_where(images):
    """return_index against np.where on P3Data's dense flags"""
    from sfm_io import read_matching
    store = read_matching(os.path.join(GOLDEN, "P3Data"), 5)
    rng = np.random.default_rng(6)
    store.flag[:] = rng.random(len(store)) < 0.6
    ff = np.zeros((store.n_features, store.n_images), dtype=int)
    ff[store.feature, store.image] = store.flag
    where = np.full((store.n_features, store.n_images), -1, dtype=np.int64)
    where[store.feature, store.image] = np.arange(len(store))
    for use_flags, dense in ((True, ff), (False, store.dense()[2])):
        rows, start, cam, xy, index = store.tracks(images, use_flags=use_flags, return_index=True)
        assert store.tracks(images, use_flags=use_flags)[3].shape == xy.shape  # the four-tuple is unchanged
        sub = dense[:, images]
        drows = np.where(sub.sum(1) >= 2)[0]
        r, col = np.where(sub[drows] == 1)
        assert np.array_equal(rows, drows)
        assert np.array_equal(index, where[drows[r], np.asarray(images)[col]])
        assert index.dtype == np.int64 and len(index) == len(cam) == start[-1]
        assert np.array_equal(store.image[index], np.asarray(images)[cam])
        assert np.array_equal(store.feature[index], np.repeat(rows, np.diff(start)))
        assert np.array_equal(np.column_stack([store.x[index], store.y[index]]), xy)


def contaminated_store(c):
    """The case's observations as a MatchStore with every flag set"""
    from sfm_io import MatchStore
    feat = np.repeat(np.arange(c["T"], dtype=np.int32), c["k"])
    store = MatchStore(c["T"], len(c["P"]), feat, c["obs_cam"], c["obs_xy"][:, 0].copy(), c["obs_xy"][:, 1].copy())
    store.flag[:] = 1
    return store


def test_update_flags_clears_the_expected_entries(gold, monkeypatch):
    """triangulate_store_robust's flag update, the device call stood in by
    the restatement's mask: outliers of kept tracks and whole dropped tracks
    lose their flag, nothing else does."""
    import sfm_multiview as mv
    name = "r5o2"
    c = load_case(name)
    k, T = c["k"], c["T"]
    mask = gold[f"{name}_mask"].astype(bool)
    n_inl = mask.reshape(T, k).sum(1).astype(np.int32)
    info = np.ones(T, dtype=np.int32)
    info[[4, 100]] = -3                      # dropped: no consensus
    angle = np.full(T, 0.2)
    angle[[7, 200]] = np.deg2rad(0.5)        # dropped: rays too close to parallel
    seen = {}

    def stand_in(P, track_start, obs_cam, obs_xy, **kw):
        seen.update(kw, n=len(obs_cam))
        z = np.zeros(T, dtype=np.int32)
        return np.zeros((T, 3)), np.zeros(T), n_inl, mask, z, z, info, angle

    monkeypatch.setattr(mv._core, "triangulate_tracks_robust", stand_in)
    store = contaminated_store(c)
    store.flag[3 * k] = 0                    # an observation already unflagged stays out of the tracks
    rows, out, keep = mv.triangulate_store_robust(store, K, c["C"], c["R"], min_angle_deg=1.0)
    assert seen["n"] == T * k - 1 and seen["min_inliers"] == 3 and seen["threshold"] == 4.0
    assert seen["centres"].shape == (len(c["P"]), 3) and np.array_equal(rows, np.arange(T))
    assert np.array_equal(np.where(~keep)[0], [4, 7, 100, 200])
    assert store.flag.sum() == T * k - 1    # update_flags is off by default
    # run again on a full store with the update on
    store = contaminated_store(c)
    rows, out, keep = mv.triangulate_store_robust(store, K, c["C"], c["R"], min_angle_deg=1.0, update_flags=True)
    want = mask.reshape(T, k).copy()
    want[[4, 7, 100, 200]] = False
    assert np.array_equal(store.flag.reshape(T, k) == 1, want)
    rows2, start2, cam2, xy2 = store.tracks(range(len(c["P"])))
    assert np.array_equal(rows2, np.setdiff1d(np.arange(T), [4, 7, 100, 200]))
    assert np.array_equal(xy2, c["obs_xy"][want.reshape(-1)])
