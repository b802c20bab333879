"""Calibrated view registration without a GPU: the sample tables, the argument
checks of sfm_register_views_p3p (all made on the host before a device is
looked for), the restatement's own P3P, and the fixture's assertions,
recomputed.

The scene of tests/golden/register_p3p.npz is not stored: load_scene
regenerates it from seeds.  p3p_restate below is the minimal solver written
independently of csrc/p3p.hpp: the resultant in u = d2 / d1 of the two conics
in (u, v = d3 / d1) is a quartic in v (Grunert's), built with numpy's polynomial
arithmetic and solved by np.roots; a candidate is kept by the property that
defines a solution, and the pose comes from an SVD alignment.  The inlier rule
and the 6-point pieces are tests/test_register_views.py's.
"""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO

import sfm_synthetic as syn
import test_register_views as rv

K = syn.K_REF
SEED = 5
SAMPLE_SEED = 21
HS = (64, 65, 256)
THRESHOLD = 4.0
# (kind, n_v, noise px, share of observations displaced by 40-120 px)
VIEWS = (("general", 3, 0.0, 0.0), ("general", 4, 0.0, 0.0), ("general", 5, 0.0, 0.0),
         ("general", 63, 0.5, 0.0), ("general", 64, 0.5, 0.0), ("general", 65, 0.5, 0.0),
         ("general", 257, 0.5, 0.0), ("general", 1025, 0.5, 0.0),
         ("general", 65, 0.5, 0.3), ("general", 1025, 0.5, 0.3),
         ("planar", 64, 0.5, 0.0), ("planar", 257, 0.5, 0.0), ("planar", 257, 0.5, 0.3),
         ("general", 257, 0.5, 0.6),
         ("degenerate", 40, 0.0, 0.0))
SMALL, PLANAR, HARD, DEGENERATE = (0, 1, 2), (10, 11, 12), 13, 14
N_GENERAL, N_PLANE = 1100, 300
PROPERTY_TOL = 1e-9       # a solution reproduces its bearings and det R = 1 to this
ROOT_GAP = 1e-5           # a hypothesis is ill-conditioned below this relative gap between quartic roots
IMAG_BAND = (1e-10, 1e-4)  # ... or with a root whose |Im| / max(1, |Re|) lies in this band
MAX_EXCLUDED = 0.05


@functools.lru_cache(maxsize=None)
def load_scene():
    """One batch of views (VIEWS).  The points: sfm_synthetic.ba_problem's, then
    N_PLANE points on the tilted plane z = 6 + 0.5 x + 0.3 y, then three
    collinear points.  View v looks through camera v.  The degenerate view's
    first three correspondences are the collinear points and its positions 3
    and 4 are one 3-D point under two indices."""
    V = len(VIEWS)
    p = syn.ba_problem(V, N_GENERAL, 3, seed=SEED, dense=False)
    rng = np.random.default_rng([SEED, 1000])
    s, t = rng.uniform(-2, 2, N_PLANE), rng.uniform(-2, 2, N_PLANE)
    plane = np.column_stack([s, t, 6.0 + 0.5 * s + 0.3 * t])
    line = np.array([[-1.0, -0.5, 5.0], [0.0, 0.0, 6.0], [1.0, 0.5, 7.0]])
    X = np.ascontiguousarray(np.concatenate([p["X_true"], plane, line]))
    pt, xy, truth = [], [], []
    for v, (kind, n, noise, share) in enumerate(VIEWS):
        rng = np.random.default_rng([SEED, v])
        if kind == "planar":
            idx = N_GENERAL + rng.choice(N_PLANE, n, replace=False)
        elif kind == "degenerate":
            rest = rng.choice(N_GENERAL, n - 4, replace=False)
            idx = np.concatenate([N_GENERAL + N_PLANE + np.arange(3), rest[:1], rest])
        else:
            idx = rng.choice(N_GENERAL, n, replace=False)
        h = (K @ (p["R_true"][v] @ (X[idx] - p["C_true"][v]).T)).T
        o = h[:, :2] / h[:, 2:]
        if noise:
            o = o + rng.normal(0, noise, o.shape)
        good = np.ones(n, dtype=bool)
        if share:
            bad = rng.choice(n, int(round(share * n)), replace=False)
            ang, mag = rng.uniform(0, 2 * np.pi, len(bad)), rng.uniform(40, 120, len(bad))
            o[bad] += np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
            good[bad] = False
        pt.append(idx)
        xy.append(o)
        truth.append(good)
    n_v = np.array([n for _, n, _, _ in VIEWS], dtype=np.int64)
    return dict(K=K, X=X, n_v=n_v, view_start=np.concatenate([[0], np.cumsum(n_v)]),
                pt_idx=np.concatenate(pt).astype(np.int32), xy=np.ascontiguousarray(np.concatenate(xy)),
                truth=np.concatenate(truth), R_true=p["R_true"], C_true=p["C_true"], V=V,
                checked=np.where((n_v >= 63))[0])


def view(sc, v):
    s, e = sc["view_start"][v], sc["view_start"][v + 1]
    return sc["X"][sc["pt_idx"][s:e]], sc["xy"][s:e]


@functools.lru_cache(maxsize=None)
def sample_table(H):
    """p3p_samples over the scene; the degenerate view's first sample is its
    three collinear points and its second holds positions 3 and 4"""
    import _sfmcore
    t = _sfmcore.p3p_samples(load_scene()["n_v"], H, SAMPLE_SEED)
    t[DEGENERATE, 0] = (0, 1, 2)
    if H > 1:
        t[DEGENERATE, 1] = (3, 4, 5)
    return t


def bearings(xy):
    b = (np.linalg.inv(K) @ np.column_stack([xy, np.ones(len(xy))]).T).T
    return b / np.linalg.norm(b, axis=1, keepdims=True)


# ------------------------------------------------------------------ the restatement's P3P
def property_error(R, C, Xs, bs):
    """how far (R, C) is from being a solution: |det R - 1|, |R R^T - I| and the
    distance of each normalised R (X_i - C) from b_i (inf behind the camera)"""
    y = (R @ (Xs - C).T).T
    yn = y / np.linalg.norm(y, axis=1, keepdims=True)
    if not np.all(np.isfinite(yn)) or ((yn * bs).sum(axis=1) <= 0).any():
        return np.inf
    return max(abs(np.linalg.det(R) - 1.0), np.abs(R @ R.T - np.eye(3)).max(), np.abs(yn - bs).max())


def align(Xs, Ys):
    """the rotation and centre with Y_i = R (X_i - C), by SVD of the covariance"""
    mx, my = Xs.mean(axis=0), Ys.mean(axis=0)
    U, _, Vt = np.linalg.svd((Ys - my).T @ (Xs - mx))
    R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    return R, mx - R.T @ my


def p3p_restate(Xs, bs):
    """Every pose that puts the three points Xs on the unit bearings bs at
    positive depth: ([(R, C), ...], ill).  ``ill``: the hypothesis is
    ill-conditioned (two quartic roots within ROOT_GAP, or one whose imaginary
    part lies in IMAG_BAND), so that the number of solutions hangs on rounding."""
    a12, a13, a23 = (np.sum((Xs[i] - Xs[j]) ** 2) for i, j in ((0, 1), (0, 2), (1, 2)))
    ext2 = max(a12, a13, a23)
    area = np.linalg.norm(np.cross(Xs[1] - Xs[0], Xs[2] - Xs[0]))
    if not ext2 > 0 or min(a12, a13, a23) <= 1e-24 * ext2 or not area > 1e-10 * ext2:
        return [], False
    a12, a13, a23 = a12 / ext2, a13 / ext2, a23 / ext2
    c12, c13, c23 = bs[0] @ bs[1], bs[0] @ bs[2], bs[1] @ bs[2]
    # E1 = a13 (1 + u^2 - 2 c12 u) - a12 (1 + v^2 - 2 c13 v), E2 = a23 (1 + u^2 - 2 c12 u) - a12 (u^2 + v^2 - 2 c23 u v)
    # as quadratics in u whose coefficients are polynomials in v (highest power first)
    p2, p1, p0 = np.array([a13]), np.array([-2 * a13 * c12]), np.array([-a12, 2 * a12 * c13, a13 - a12])
    q2, q1, q0 = np.array([a23 - a12]), np.array([2 * a12 * c23, -2 * a23 * c12]), np.array([-a12, 0.0, a23])
    m, s = np.polymul, np.polysub
    r20, r21, r10 = s(m(p2, q0), m(p0, q2)), s(m(p2, q1), m(p1, q2)), s(m(p1, q0), m(p0, q1))
    quartic = s(m(r20, r20), m(r21, r10))
    roots = np.roots(quartic)
    rel = np.abs(roots.imag) / np.maximum(1.0, np.abs(roots.real))
    ill = len(roots) < 4 or bool(((rel > IMAG_BAND[0]) & (rel < IMAG_BAND[1])).any())
    for i in range(len(roots)):
        for j in range(i):
            if abs(roots[i] - roots[j]) < ROOT_GAP * max(1.0, abs(roots[i])):
                ill = True
    out = []
    for v in roots[rel <= IMAG_BAND[0]].real:
        with np.errstate(all="ignore"):
            u = -np.polyval(r20, v) / np.polyval(r21, v)
            d1 = np.sqrt(a12 / (1 + u * u - 2 * c12 * u))
        d = np.array([d1, u * d1, v * d1])
        if not (np.all(np.isfinite(d)) and np.all(d > 0)):
            continue
        for _ in range(4):  # Newton on the three distance constraints
            f = np.array([d[0] ** 2 + d[1] ** 2 - 2 * c12 * d[0] * d[1] - a12,
                          d[0] ** 2 + d[2] ** 2 - 2 * c13 * d[0] * d[2] - a13,
                          d[1] ** 2 + d[2] ** 2 - 2 * c23 * d[1] * d[2] - a23])
            J = 2 * np.array([[d[0] - c12 * d[1], d[1] - c12 * d[0], 0.0],
                              [d[0] - c13 * d[2], 0.0, d[2] - c13 * d[0]],
                              [0.0, d[1] - c23 * d[2], d[2] - c23 * d[1]]])
            try:
                d = d - np.linalg.solve(J, f)
            except np.linalg.LinAlgError:
                break
        if not (np.all(np.isfinite(d)) and np.all(d > 0)):
            continue
        R, C = align(Xs, np.sqrt(ext2) * d[:, None] * bs)
        if np.all(np.isfinite(R)) and np.all(np.isfinite(C)) and property_error(R, C, Xs, bs) <= PROPERTY_TOL:
            out.append((R, C))
    return out, ill


def near_threshold(P, X, xy, thr):
    """some error within 1e-9 relative of the threshold: the count hangs on rounding"""
    e2, h2 = rv.errors2(P, X, xy)
    with np.errstate(invalid="ignore"):
        return bool((np.abs(np.sqrt(e2[h2 > 0]) - thr) <= 1e-9 * thr).any())


@functools.lru_cache(maxsize=None)
def restated_hypotheses(v, H):
    """per hypothesis of view v: (solutions [(R, C, P, mask, cost)], excluded)"""
    sc = load_scene()
    X, xy = view(sc, v)
    b = bearings(xy)
    out = []
    for smp in sample_table(H)[v]:
        sols, ill = p3p_restate(X[smp], b[smp])
        full = []
        for R, C in sols:
            P = rv.projection(C, R)
            m = rv.inlier_mask(P, X, xy, THRESHOLD)
            ill = ill or near_threshold(P, X, xy, THRESHOLD)
            full.append((R, C, P, m, float(rv.errors2(P, X, xy)[0][m].sum())))
        out.append((full, ill))
    return out


def restated_winner(v, H):
    """most inliers, then the smaller cost, then the earlier hypothesis, then the earlier solution"""
    best = None
    for h, (sols, _) in enumerate(restated_hypotheses(v, H)):
        for k, (R, C, P, m, cost) in enumerate(sols):
            if best is None or m.sum() > best[0] or (m.sum() == best[0] and cost < best[1]):
                best = (int(m.sum()), cost, h, k, R, C, m)
    return best


def write_host_check_samples(path):
    """the fixture's samples for tools/p3p_host_check.cpp: the degenerate view's
    (its two degenerate samples first), then every other view's at H = 64"""
    sc = load_scene()
    rows = []
    for v in [DEGENERATE] + [v for v in range(sc["V"]) if v != DEGENERATE and sc["n_v"][v] >= 4]:
        X, xy = view(sc, v)
        b = bearings(xy)
        for smp in sample_table(64)[v]:
            rows.append(np.concatenate([X[smp].reshape(-1), b[smp].reshape(-1)]))
    np.savetxt(path, np.array(rows), fmt="%.17g")


# ------------------------------------------------------------------ samples
def test_p3p_samples():
    import _sfmcore as core
    counts = [2, 3, 4, 40, 0, 1025]
    t = core.p3p_samples(counts, 65, 9)
    assert t.shape == (6, 65, 3) and t.dtype == np.int32
    assert not t[0].any() and not t[4].any()          # n_v < 3: zeros
    for v in (1, 2, 3, 5):
        assert t[v].min() >= 0 and t[v].max() < counts[v]
        assert all(len(set(row)) == 3 for row in t[v].tolist())
    assert np.array_equal(t, core.p3p_samples(counts, 65, 9))          # reproducible by seed
    assert not np.array_equal(t, core.p3p_samples(counts, 65, 10))
    # a view's table depends on its place and size alone, not on the others
    other = core.p3p_samples([900, 3, 1, 40], 65, 9)
    assert np.array_equal(other[1], t[1]) and np.array_equal(other[3], t[3])
    with pytest.raises(ValueError):
        core.p3p_samples(counts, 0, 9)


# ------------------------------------------------------------------ the checks on the host
def small_call():
    sc = load_scene()
    V = 5
    e = int(sc["view_start"][V])
    return dict(K=K, X=sc["X"], view_start=sc["view_start"][:V + 1].copy(), pt_idx=sc["pt_idx"][:e].copy(),
                xy=sc["xy"][:e].copy(), samples=sample_table(64)[:V].copy())


def test_library_exports_the_symbol():
    import _sfmcore as core
    assert hasattr(core._lib, "sfm_register_views_p3p")
    assert "sfm_register_views_p3p" in {n for n, _, _ in core.SIGNATURES}
    assert "sfm_register_views_p3p" in open(os.path.join(REPO, "include", "sfmcore.h")).read()


def test_no_views_returns_empty_outputs_without_a_device():
    import _sfmcore as core
    out = core.register_views_p3p(K, np.zeros((3, 3)), [0], [], np.zeros((0, 2)), np.zeros((0, 8, 3), dtype=np.int32),
                                  want_counts=True, want_models=True)
    C, R, cost, n_inl, inl, hyp, count, info, n_sol, counts, models = out
    assert C.shape == (0, 3) and R.shape == (0, 3, 3) and inl.shape == (0,) and info.shape == (0,)
    assert n_sol.shape == (0, 8) and counts.shape == (0, 8, 4) and models.shape == (0, 8, 4, 3, 4)


def test_views_of_fewer_than_four_need_no_device(monkeypatch):
    import _sfmcore as core
    monkeypatch.setattr(core, "require_device", lambda: (_ for _ in ()).throw(AssertionError("device")))
    a = small_call()
    C, R, cost, n_inl, inl, hyp, count, info, n_sol, counts, models = core.register_views_p3p(
        K, a["X"], a["view_start"][:2], a["pt_idx"][:3], a["xy"][:3], a["samples"][:1], want_counts=True,
        want_models=True)
    assert info[0] == -1 and not C.any() and np.array_equal(R[0], np.eye(3)) and not inl.any()
    assert n_inl[0] == 0 and hyp[0] == -1 and count[0] == 0 and cost[0] == 0
    assert not n_sol.any() and not counts.any() and not models.any()


def _edit(a, key, fn):
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    fn(b[key])
    return b


VIOLATIONS = {
    "view_start not from 0": lambda a: _edit(a, "view_start", lambda x: x.__setitem__(0, 1)),
    "view_start decreases": lambda a: _edit(a, "view_start", lambda x: x.__setitem__(2, 2)),
    "view_start ends early": lambda a: _edit(a, "view_start", lambda x: x.__setitem__(-1, x[-1] - 1)),
    "pt_idx negative": lambda a: _edit(a, "pt_idx", lambda x: x.__setitem__(7, -1)),
    "pt_idx past X": lambda a: _edit(a, "pt_idx", lambda x: x.__setitem__(7, len(load_scene()["X"]))),
    "sample negative": lambda a: _edit(a, "samples", lambda x: x.__setitem__((1, 3, 2), -1)),
    "sample past its view": lambda a: _edit(a, "samples", lambda x: x.__setitem__((1, 3, 2), 4)),
    "sample repeated": lambda a: _edit(a, "samples", lambda x: x.__setitem__((4, 63, 2), x[4, 63, 0])),
}


@pytest.mark.parametrize("name", list(VIOLATIONS))
def test_argument_violations_raise_before_a_device_is_needed(name, monkeypatch):
    import _sfmcore as core

    def no_device():
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(core, "require_device", no_device)
    a = VIOLATIONS[name](small_call())
    with pytest.raises(core.SfmCoreError, match="argument"):
        core.register_views_p3p(**a)


@pytest.mark.parametrize("kw", [dict(threshold=0.0), dict(threshold=np.nan), dict(threshold=np.inf),
                                dict(min_inliers=3), dict(refit_rounds=-1), dict(max_nfev=0)])
def test_option_violations_raise_before_a_device_is_needed(kw, monkeypatch):
    import _sfmcore as core
    monkeypatch.setattr(core, "require_device", lambda: (_ for _ in ()).throw(AssertionError("device")))
    with pytest.raises(core.SfmCoreError, match="argument"):
        core.register_views_p3p(**small_call(), **kw)


def test_a_bad_sample_in_a_view_of_fewer_than_four_is_ignored():
    import _sfmcore as core
    a = small_call()
    a["samples"][0] = 99
    out = core.register_views_p3p(K, a["X"], a["view_start"][:2], a["pt_idx"][:3], a["xy"][:3], a["samples"][:1])
    assert out[7][0] == -1


# ------------------------------------------------------------------ the restatement's P3P
@pytest.mark.parametrize("v", [6, 7])
def test_restated_p3p_solutions_have_the_property_and_hold_the_truth(v):
    """noise-free samples of a general view: every solution is one by the
    defining property, and the true pose is among them"""
    sc = load_scene()
    s, e = sc["view_start"][v], sc["view_start"][v + 1]
    X = sc["X"][sc["pt_idx"][s:e]]
    Rt, Ct = sc["R_true"][v], sc["C_true"][v]
    y = (Rt @ (X - Ct).T).T
    b = y / np.linalg.norm(y, axis=1, keepdims=True)
    n_sols = []
    for smp in sample_table(64)[v]:
        sols, ill = p3p_restate(X[smp], b[smp])
        assert len(sols) <= 4 and (ill or len(sols) >= 1)
        for R, C in sols:
            assert property_error(R, C, X[smp], b[smp]) <= PROPERTY_TOL
        if not ill:
            assert min(max(np.abs(R - Rt).max(), np.abs(C - Ct).max()) for R, C in sols) <= 1e-7
        n_sols.append(len(sols))
    assert max(n_sols) >= 2  # the scene has samples of more than one solution


def test_restated_p3p_has_no_solution_for_the_degenerate_samples():
    sc = load_scene()
    X, xy = view(sc, DEGENERATE)
    b = bearings(xy)
    t = sample_table(64)[DEGENERATE]
    assert p3p_restate(X[t[0]], b[t[0]])[0] == [] and p3p_restate(X[t[1]], b[t[1]])[0] == []
    assert np.array_equal(X[3], X[4]) and len(p3p_restate(X[t[2]], b[t[2]])[0]) >= 1


# ------------------------------------------------------------------ the fixture
def test_fixture_assertions_hold_when_recomputed():
    g = np.load(os.path.join(GOLDEN, "register_p3p.npz"))
    sc = load_scene()
    thr = float(g["threshold"])
    assert thr == THRESHOLD
    assert np.array_equal(g["truth"], sc["truth"]) and np.array_equal(g["n_v"], sc["n_v"])
    assert set(sc["checked"]) == set(np.where(sc["n_v"] >= 63)[0])  # no view left out
    for v in sc["checked"]:
        X, xy = view(sc, v)
        s, e = sc["view_start"][v], sc["view_start"][v + 1]
        truth = sc["truth"][s:e]
        P = rv.projection(g["C_min"][v], g["R_min"][v])
        e2, h2 = rv.errors2(P, X, xy)
        # the converged minimum on the true inliers separates them from the rest by a pixel
        assert np.array_equal(rv.inlier_mask(P, X, xy, thr), truth)
        assert np.abs(np.sqrt(e2) - thr).min() >= 1.0 and h2.min() > 1.0
        assert np.isclose(e2[truth].sum(), g["cost_min"][v], rtol=1e-9)
        for H in HS:
            assert g[f"final_margin_H{H}"][v] >= 1.0
            assert np.array_equal(g[f"mask_H{H}"][s:e], truth)
            ex = g[f"excluded_H{H}"][v, :H]
            assert ex.mean() <= MAX_EXCLUDED
    # the capability gap: the 6-point restatement finds no consensus on the planar views
    import _sfmcore
    t6 = _sfmcore.register_samples(sc["n_v"], 256, SAMPLE_SEED)
    for v in PLANAR:
        X, xy = view(sc, v)
        assert six_point_best_count(X, xy, t6[v], thr) < 6
        assert g["six_point_best_count"][v] < 6
    # the 60 % view at H = 64: no clean 6-point sample, at least three clean 3-point samples
    s = sc["view_start"][HARD]
    truth = sc["truth"][s:sc["view_start"][HARD + 1]]
    assert not truth[_sfmcore.register_samples(sc["n_v"], 64, SAMPLE_SEED)[HARD]].all(axis=1).any()
    assert truth[sample_table(64)[HARD]].all(axis=1).sum() >= 3


def six_point_best_count(X, xy, samples, thr):
    """the best inlier count of tests/test_register_views.py's 6-point restatement"""
    best = 0
    for smp in samples:
        p = np.linalg.svd(rv.dlt_rows(X[smp], xy[smp]))[2][-1]
        C, R, P = rv.pose_from_null(p)
        if np.all(np.isfinite(C)) and np.all(np.isfinite(P)):
            best = max(best, int(rv.inlier_mask(P, X, xy, thr).sum()))
    return best
