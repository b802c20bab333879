"""Global position averaging on a real MI355X (sfm_average_positions,
sfm_multiview.average_positions) against the stored dense-solve restatement of
tests/test_position_averaging.py.  info, n_solved and edge_inlier are compared
for equality (the fixture keeps every angle 1e-6 rad from the threshold); C,
edge_angle and edge_length within pa.tolerance(name): 100 x the gap the numpy
PCG leaves to the dense solve on that graph, at least 1e-12 -- C and
edge_length relative to the largest |C|, edge_angle in radians.
"""
import numpy as np
import pytest

import test_position_averaging as pa

pytestmark = pytest.mark.gpu
NAMES = ("C", "edge_angle", "edge_inlier", "edge_length", "info", "cg_iters", "cg_residual", "n_solved", "path_used")


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


def call(core, g, path, **change):
    args = {**pa.DEFAULTS, **change}
    return dict(zip(NAMES, core.average_positions(g["N"], g["ij"], g["dir"], g["weight"], path=path, **args)))


def compare(got, ref, tol, what):
    assert got["n_solved"] == int(ref["n_solved"]) and np.array_equal(got["info"], ref["info"]), what
    assert np.array_equal(got["edge_inlier"], ref["edge_inlier"]), what
    gap = pa.gaps(got, ref)
    print(f"{what}: gap {gap:.3g} (allowed {tol:.3g}), CG iterations {got['cg_iters'].tolist()}")
    assert gap <= tol, (what, gap, tol)


# (graph, path asked for, path that must run)
PARITY = [("a", 1, 1), ("a", 2, 2), ("b", 1, 1), ("b", 2, 2), ("c", 1, 1), ("c", 2, 2), ("e", 1, 1), ("e", 2, 2),
          ("d", 2, 2), ("d", 0, 2), ("a", 0, 1)]


@pytest.mark.parametrize("name,path,used", PARITY)
def test_parity_with_the_restatement(core, name, path, used):
    got = call(core, pa.stored_graph(name), path)
    assert got["path_used"] == used
    compare(got, pa.stored_out(name), pa.tolerance(name), f"graph {name} path {path}")
    assert np.all(got["cg_iters"] < pa.DEFAULTS["cg_max_iters"]) and np.all(got["cg_residual"] <= pa.DEFAULTS["cg_tol"])


@pytest.mark.parametrize("path", [1, 2])
def test_leaves_and_the_small_component_are_left_out(core, path):
    g = pa.stored_graph("e")
    got = call(core, g, path)
    solved = np.arange(g["N"]) < 8
    assert np.array_equal(got["info"] >= 0, solved) and (got["info"] == 1).sum() == 1 and got["n_solved"] == 8
    assert not got["C"][~solved].any() and not got["C"][got["info"] == 1].any()
    dead = ~(solved[g["ij"][:, 0]] & solved[g["ij"][:, 1]])
    assert dead.sum() == 13
    assert not got["edge_angle"][dead].any() and not got["edge_length"][dead].any() and not got["edge_inlier"][dead].any()
    assert got["edge_inlier"][~dead].all()


@pytest.mark.parametrize("name,path", [("c", 1), ("c", 2), ("d", 2)])
def test_two_calls_give_identical_bytes(core, name, path):
    g = pa.stored_graph(name)
    a, b = call(core, g, path), call(core, g, path)
    for n in NAMES:
        assert np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes(), n


@pytest.mark.parametrize("name,path", [("b", 1), ("b", 2), ("d", 2)])
def test_the_iteration_cap_is_reported_not_raised(core, name, path):
    got = call(core, pa.stored_graph(name), path, cg_max_iters=3)
    assert np.array_equal(got["cg_iters"], np.full(pa.DEFAULTS["rounds"], 3))
    assert np.all(got["cg_residual"] > pa.DEFAULTS["cg_tol"]) and np.all(np.isfinite(got["C"]))


def test_path_1_refuses_a_graph_past_its_bound(core):
    g = pa.stored_graph("d")
    rc, untouched = pa.raw_call(g["N"], g["ij"], g["dir"], path=1)
    assert rc == -1 and untouched
    with pytest.raises(core.SfmCoreError):
        call(core, g, 1)


def test_timings_have_four_slots(core):
    g = pa.stored_graph("b")
    core.set_call_timing(True)
    try:
        for path in (1, 2):
            call(core, g, path)
            t = core.last_timings()
            assert len(t) == 4 and np.all(t >= 0) and t[1] > 0 and 0 < t[3] <= t[1] * 1.05
    finally:
        core.set_call_timing(False)


def test_a_scene_from_verify_pairs_to_centres(core):
    """8 cameras on an arc around a cloud of points, through verify_pairs, init_pairs, pair_rotations,
    average_rotations, pair_directions and average_positions.  The device's centres equal the restatement's on the
    same directions; the error against the true centres after a similarity alignment is printed, not asserted."""
    import sfm_multiview as mv
    import sfm_synthetic as syn
    import test_verify_pairs as vp
    from sfm_io import MatchStore
    rng = np.random.default_rng(6)
    n_img, n_pts = 8, 150
    X = np.column_stack([rng.uniform(-2, 2, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(6, 10, n_pts)])
    ang = np.linspace(-0.35, 0.35, n_img)
    Cw = np.column_stack([8.0 * np.sin(ang), rng.uniform(-0.6, 0.6, n_img), 8.0 - 8.0 * np.cos(ang)])
    R = np.stack([syn.rotvec_to_matrix(np.array([0.02 * rng.normal(), a, 0.02 * rng.normal()]))[0] for a in ang])
    feat = np.repeat(np.arange(n_pts), n_img)
    img = np.tile(np.arange(n_img), n_pts)
    xs = np.stack([vp.project(R[i], Cw[i], X) for i in range(n_img)], axis=1).reshape(-1, 2)
    xs = xs + rng.normal(0, 0.3, xs.shape)
    st = MatchStore(n_pts, n_img, feat.astype(np.int32), img.astype(np.int32), np.ascontiguousarray(xs[:, 0]),
                    np.ascontiguousarray(xs[:, 1]))
    verified = mv.verify_pairs(st, H=256, seed=0)
    init = mv.init_pairs(st, vp.K, verified)
    e_ij, e_R, e_w = mv.pair_rotations(verified, init)
    rotations = mv.average_rotations(e_ij, e_R, n_img, weight=e_w)
    ij, dirs, w, keep = mv.pair_directions(verified, init, rotations)
    assert len(ij) >= 2 * n_img
    solved, out = mv.average_positions(ij, dirs, n_img, weight=w)
    got = dict(zip(NAMES, out))
    ref = pa.restate(n_img, ij, dirs, w, **pa.DEFAULTS)
    pcg = pa.restate(n_img, ij, dirs, w, solver="pcg", **pa.DEFAULTS)
    assert ref["margin"] > pa.MASK_MARGIN
    compare(got, ref, max(100.0 * pa.gaps(pcg, ref), 1e-12), "scene")
    assert got["path_used"] == 1 and np.array_equal(solved, np.flatnonzero(ref["info"] >= 0)) and len(solved) >= 6
    # similarity alignment: the centres live in the frame of the averaged rotations (root at I)
    A, B = got["C"][solved], Cw[solved]
    a, b = A - A.mean(axis=0), B - B.mean(axis=0)
    U, S, Vt = np.linalg.svd(b.T @ a)
    Q = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    err = np.linalg.norm((S.sum() / (a * a).sum()) * a @ Q.T - b, axis=1)
    print(f"scene: {len(ij)} edges, {len(solved)} of {n_img} cameras solved, inlier edges {int(got['edge_inlier'].sum())}; "
          f"centre error after similarity alignment: worst {err.max():.3g}, median {np.median(err):.3g} "
          f"(camera spacing {np.linalg.norm(np.diff(Cw, axis=0), axis=1).mean():.3g})")
