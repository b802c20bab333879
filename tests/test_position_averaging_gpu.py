"""Global position averaging on a real MI355X (sfm_average_positions,
sfm_multiview.average_positions) against the stored dense-solve restatement of
tests/test_position_averaging.py.  info, n_solved and edge_inlier are compared
for equality (the fixture keeps every angle 1e-6 rad from the threshold); C,
edge_angle and edge_length within pa.tolerance(name): 100 x the gap the numpy
PCG leaves to the dense solve on that graph, at least 1e-12 -- C and
edge_length relative to the largest |C|, edge_angle in radians.  The lane-width graphs (pa.LANE_GRAPHS) run
the same comparison at the plans asserted in tests/test_position_plan.py; the
iteration counts are held to the numpy PCG's (check_iterations), and solves
ended by cg_max_iters to the numpy PCG ended at the same count.
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


def check_iterations(name, got, what):
    """every round within pa.iteration_bound() of the numpy PCG's count, on the graphs where that bound tells a
    useless preconditioner from the right one (pa.iterations_tell); printed on all"""
    pcg, ident = pa.iteration_counts(name)
    print(f"{what}: CG iterations, device {got['cg_iters'].tolist()}, numpy PCG {pcg.tolist()}, "
          f"numpy CG without a preconditioner {ident.tolist()}")
    if pa.iterations_tell(name):
        assert np.all(got["cg_iters"] <= pa.iteration_bound(pcg)), (what, got["cg_iters"].tolist(), pcg.tolist())


@pytest.mark.parametrize("name,path,used", PARITY)
def test_parity_with_the_restatement(core, name, path, used):
    got = call(core, pa.stored_graph(name), path)
    assert got["path_used"] == used
    compare(got, pa.stored_out(name), pa.tolerance(name), f"graph {name} path {path}")
    assert np.all(got["cg_iters"] < pa.DEFAULTS["cg_max_iters"]) and np.all(got["cg_residual"] <= pa.DEFAULTS["cg_tol"])
    check_iterations(name, got, f"graph {name} path {path}")


# every lane-width graph on every path its plan was built for (tests/test_position_plan.py holds the plans)
LANE_PARITY = [(name, path, used) for name, (_, _, paths) in pa.LANE_GRAPHS.items() for path, used in paths]


@pytest.mark.parametrize("name,path,used", LANE_PARITY)
def test_parity_at_every_lane_width(core, name, path, used):
    """G from 1 to 64 on both paths, path 1 at its clamp and at its LDS bound, path 2 with more group workgroups
    than node workgroups and with more partials than a workgroup has threads: against the stored dense
    restatement, the edge references recomputed from its centres"""
    g, rounds = pa.lane_graph(name), pa.LANE_GRAPHS[name][1]
    got = call(core, g, path, rounds=rounds)
    assert got["path_used"] == used
    compare(got, pa.lane_reference(name), pa.lane_tolerance(name), f"graph {name} path {path}")
    assert np.all(got["cg_iters"] < pa.DEFAULTS["cg_max_iters"]) and np.all(got["cg_residual"] <= pa.DEFAULTS["cg_tol"])
    check_iterations(name, got, f"graph {name} path {path}")


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


@pytest.mark.parametrize("name,path", [("k8x37", 1), ("k8x37", 2), ("k200", 2), ("dense1100", 2)])
def test_two_calls_give_identical_bytes_at_wide_groups(core, name, path):
    """a group that is a whole wave, on both paths; 32 lanes over 25 workgroups; pa_resum past one trip"""
    g, rounds = pa.lane_graph(name), pa.LANE_GRAPHS[name][1]
    a, b = call(core, g, path, rounds=rounds), call(core, g, path, rounds=rounds)
    for n in NAMES:
        assert np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes(), n


_capped = {}


def capped_reference(name, cap, rounds):
    """the float64 numpy PCG ended at `cap` iterations in every round, computed once"""
    if (name, cap, rounds) not in _capped:
        g = pa.stored_graph(name)
        args = {**pa.DEFAULTS, "rounds": rounds, "cg_max_iters": cap}
        ref = pa.restate(g["N"], g["ij"], g["dir"], g["weight"], solver="pcg", **args)
        assert ref["margin"] > pa.MASK_MARGIN and np.all(ref["cg_iters"] == cap)
        _capped[name, cap, rounds] = ref
    return _capped[name, cap, rounds]


def compare_capped(got, ref, stored_gap, cap, what):
    """A solve ended by the cap is no solution of the system, so the dense solve is no reference: the device must
    have made exactly `cap` iterations of the header's PCG.  Allowed: 100 x the gap between that PCG in float64
    and in long double (stored), at least 1e-12.  The residual that is reported is the one after the last
    iteration: within 1e-9 of the numpy PCG's, relatively -- the recurrence carries it to some 1e-13, and one
    iteration more or less moves it by tens of per cent."""
    assert np.array_equal(got["cg_iters"], np.full(len(got["cg_iters"]), cap)), what
    compare(got, ref, max(100.0 * float(stored_gap), 1e-12), what)
    print(f"{what}: residuals {got['cg_residual'].tolist()}, numpy PCG {ref['cg_residual'].tolist()}")
    assert np.all(got["cg_residual"] > pa.DEFAULTS["cg_tol"]) and np.all(np.isfinite(got["C"]))
    assert np.all(np.abs(got["cg_residual"] - ref["cg_residual"]) <= 1e-9 * ref["cg_residual"]), what


@pytest.mark.parametrize("name,path", [("b", 1), ("b", 2), ("d", 2)])
def test_the_iteration_cap_is_reported_not_raised(core, name, path):
    got = call(core, pa.stored_graph(name), path, cg_max_iters=3)
    assert len(got["cg_iters"]) == pa.DEFAULTS["rounds"]
    compare_capped(got, capped_reference(name, 3, pa.DEFAULTS["rounds"]), pa.lanes_fixture()[f"cap3_{name}_gap"], 3,
                   f"graph {name} path {path} cap 3")


@pytest.mark.parametrize("cap", pa.CAPS)
@pytest.mark.parametrize("path", [1, 2])
def test_the_cap_around_the_batch_of_eight(core, path, cap):
    """path 2 launches 8 iterations between two looks at the stop word and ends a solve that nothing else ended
    with one k_pa_apply alone: caps below, at, one past and at twice the batch, and a cap of 1, two rounds each"""
    got = call(core, pa.stored_graph("b"), path, rounds=pa.CAP_ROUNDS, cg_max_iters=cap)
    assert len(got["cg_iters"]) == pa.CAP_ROUNDS
    compare_capped(got, capped_reference("b", cap, pa.CAP_ROUNDS), pa.lanes_fixture()[f"cap{cap}_gap"], cap,
                   f"graph b path {path} cap {cap}")


def test_path_1_refuses_a_graph_past_its_bound(core):
    g = pa.stored_graph("d")
    rc, untouched = pa.raw_call(g["N"], g["ij"], g["dir"], path=1)
    assert rc == -1 and untouched
    with pytest.raises(core.SfmCoreError):
        call(core, g, 1)


def test_path_1_refuses_one_node_past_its_bound(core):
    """513 solved nodes (512 run on path 1 in the parity test above): refused before anything is written"""
    g = pa.lane_graph("bound513")
    assert pa.lane_reference("bound513")["n_solved"] == pa.PATH1_MAX_NODES + 1
    rc, untouched = pa.raw_call(g["N"], g["ij"], g["dir"], path=1)
    assert rc == -1 and untouched
    with pytest.raises(core.SfmCoreError):
        call(core, g, 1)


@pytest.mark.parametrize("path", [1, 2])
def test_an_overflowing_weight_sum_is_a_numeric_error(core, path):
    """every weight 1e308 is finite and passes the argument check; their sum is not, so c of round 0 is not
    finite: SFM_ERR_NUMERIC from the error word of path 1 and from PaState.error of path 2.  (Every loop of both
    paths ends on NaN: the stops are `rn > tol * bn` and `!(rn > ..)`, and the host's loop over k is bounded by
    cg_max_iters.)  The call after it is the call before it."""
    g = pa.stored_graph("e")
    before = call(core, g, path)
    with pytest.raises(core.SfmCoreError, match=r"error -7: numeric"):
        call(core, {**g, "weight": np.full(len(g["ij"]), 1e308)}, path)
    after = call(core, g, path)
    for n in NAMES:
        assert np.asarray(before[n]).tobytes() == np.asarray(after[n]).tobytes(), n


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
