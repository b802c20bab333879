"""The Gauss-Newton CG refit of rotation averaging on a real MI355X
(sfm_average_rotations_cg, average_rotations(refit="cg")) against the numpy PCG
restatement of tests/test_rotation_cg.py.  The integer outputs and the rounds
run are compared for equality (every stored run keeps its trace tests 1e-9 from
tau and its steps 5 % from tol); R and edge_angle within rc.tolerance(name):
100 x the gap the numpy PCG leaves to the dense minimum-norm solve on that
graph, at least 1e-12; the CG iterations of a round within max(2, 10 %) of the
numpy PCG's.
"""
import ctypes

import numpy as np
import pytest

import test_rotation_averaging as ra
import test_rotation_cg as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


def call(core, g, **args):
    out = core.average_rotations(g["N"], g["ij"], g["R_rel"], g["weight"], refit="cg", **args)
    assert len(out) == len(rc.CG_OUTPUTS)
    return dict(zip(rc.CG_OUTPUTS, out))


def compare(got, ref, tol, what, nodes=None):
    """`nodes`: the nodes R is compared on (all by default); edge_angle on the edges between them"""
    assert ref["margin"] > ra.MARGIN, what
    for n in ra.INTEGER_OUTPUTS:
        assert np.array_equal(got[n], ref[n]), (what, n)
    nodes = np.ones(len(ref["R"]), bool) if nodes is None else nodes
    edges = nodes[got["ij"][:, 0]] & nodes[got["ij"][:, 1]] if len(got["ij"]) else np.zeros(0, bool)
    gap = max(float(np.abs(got["R"][nodes] - ref["R"][nodes]).max()) if nodes.any() else 0.0,
              float(np.abs(got["edge_angle"][edges] - ref["edge_angle"][edges]).max()) if edges.any() else 0.0)
    print(f"{what}: gap {gap:.3g} (allowed {tol:.3g}), rounds {got['sweeps']}, CG iterations "
          f"{got['cg_iters'].tolist()} (numpy PCG {np.asarray(ref['cg_iters']).tolist()}), steps "
          f"{['%.3g' % s for s in got['step']]}")
    assert gap <= tol, (what, gap, tol)
    want = np.asarray(ref["cg_iters"], dtype=np.int64)
    assert np.all(np.abs(got["cg_iters"] - want) <= np.maximum(2, np.ceil(0.1 * want))), what
    assert np.all(got["cg_iters"][got["sweeps"]:] == 0) and np.all(got["step"][got["sweeps"]:] == 0), what
    assert np.all(got["cg_residual"][got["sweeps"]:] == 0), what
    assert np.allclose(got["step"], ref["step"], rtol=1e-6, atol=tol), what


def check_stored(core, name, nodes=None, **change):
    g = rc.graph(name)
    got = call(core, g, **rc.run_args(name, **change))
    got["ij"] = g["ij"]
    ref = rc.pcg_run(name, **change) if change else rc.stored_pcg(name)
    compare(got, ref, rc.tolerance(name), name + (f" {change}" if change else ""), nodes)
    return got, ref


def check_live(core, g, what, **args):
    """against the restatement computed here, at the floor of the tolerance: graphs of a few nodes"""
    got = call(core, g, **args)
    got["ij"] = np.asarray(g["ij"]).reshape(-1, 2)
    compare(got, rc.restate_cg(g["N"], g["ij"], g["R_rel"], g["weight"], **args), 1e-12, what)
    return got


# ------------------------------------------------------------------ trivial sizes
def test_trivial_sizes(core):
    none = dict(ij=np.zeros((0, 2), np.int32), R_rel=np.zeros((0, 3, 3)), weight=None)
    check_live(core, dict(N=0, **none), "N = 0")
    got = check_live(core, dict(N=3, **none), "E = 0", rounds=4)
    assert np.array_equal(got["info"], [-1, -1, -1]) and got["sweeps"] == 0 and len(got["step"]) == 4
    R_true = ra.random_rotations(np.random.default_rng(1), 2)
    ij = np.array([[1, 0]], np.int32)
    R_rel = ra.measure(R_true, ij, 1.0, np.zeros(1, bool), np.random.default_rng(2))[0]
    got = check_live(core, dict(N=2, ij=ij, R_rel=R_rel, weight=None), "one edge")
    assert got["sweeps"] == 1 and got["cg_iters"][0] == 0 and got["edge_inlier"].all()


# ------------------------------------------------------------------ trees and high degree
def test_path_of_70_nodes(core):
    """68 levels below the root, past one batch of the tree's launches; b = 0, so no CG iteration and one round"""
    got, ref = check_stored(core, "path70")
    assert got["level"].max() == 68 and got["sweeps"] == 1 and got["cg_iters"][0] == 0 and got["step"][0] == 0.0
    g = rc.graph("path70")
    tree = core.average_rotations(g["N"], g["ij"], g["R_rel"], seed=rc.RUN["seed"], consensus_sweeps=0, max_sweeps=0)
    assert got["R"].tobytes() == tree[0].tobytes() == ref["R"].tobytes()  # R is the tree's, bit for bit


@pytest.mark.parametrize("name", ["star", "double_star"])
def test_stars_of_degree_300(core, name):
    """one node's 300 entries walked by a single lane (G = 1)"""
    got, _ = check_stored(core, name)
    assert got["info"][0] == 1
    if name == "double_star":
        assert got["info"][301] == 0 and got["edge_inlier"].sum() == 502 and got["sweeps"] > 1


# ------------------------------------------------------------------ every lane width, grids past one workgroup
@pytest.mark.parametrize("name", ["sparse2", "sparse", "medium", "dense100", "k64", "k32x3", "k16x9", "k8x37"])
def test_parity_at_every_lane_width(core, name):
    """G = 2, 4, 4, 4, 8, 16, 32 and 64 lanes per node (G = 1: the stars, the path, the components)"""
    got, _ = check_stored(core, name)
    assert got["sweeps"] < rc.CG_DEFAULTS["rounds"] and got["step"][got["sweeps"] - 1] <= rc.CG_DEFAULTS["tol"]


def test_a_second_workgroup_of_the_node_grid(core):
    check_stored(core, "n257")


def test_the_partials_are_resummed_in_two_trips(core):
    """275 workgroups of 64-lane groups leave 275 partials for workgroups of 256 threads; no consensus sweep and
    two rounds keep the restatement cheap"""
    got, _ = check_stored(core, "dense1100")
    assert got["sweeps"] == 2 and np.all(got["cg_iters"] > 0)


# ------------------------------------------------------------------ components, weights, a detached group
def test_components_duplicates_orientations_and_weights(core):
    got, _ = check_stored(core, "components")
    roots = np.flatnonzero(got["info"] == 1)
    assert len(roots) == 2 and roots[0] < 12 <= roots[1]
    assert np.array_equal(got["R"][roots], np.tile(np.eye(3), (2, 1, 1)))  # the gauge, bit for bit
    assert got["info"][20] == -1 and np.array_equal(got["R"][20], np.eye(3))
    check_stored(core, "weighted")


def test_groups_detached_from_their_root(core):
    """the second cluster ends as two groups without a root, singular blocks of the normal equations: integer
    outputs equal, R compared on the root's group"""
    g = rc.graph("detached")
    ref = rc.stored_pcg("detached")
    got, _ = check_stored(core, "detached", nodes=rc.rooted(g["N"], g["ij"], ref["group"]))
    assert len(np.unique(got["group"])) == 3 and np.all(np.isfinite(got["R"]))
    assert np.all(got["cg_iters"][:got["sweeps"]] < rc.CG_DEFAULTS["cg_max_iters"])


# ------------------------------------------------------------------ capped solves, exact rounds
@pytest.mark.parametrize("cap", rc.CAPS)
def test_the_cap_around_the_batch_of_eight(core, cap):
    """the host launches 8 iterations between two looks at the stop word and ends a solve that nothing else ended
    with one apply launch alone: against the numpy PCG ended at the same count"""
    got, ref = check_stored(core, "medium", cg_max_iters=cap, **rc.CAP_ARGS)
    assert np.array_equal(got["cg_iters"], [cap, cap]) and np.array_equal(ref["cg_iters"], [cap, cap])
    assert np.all(np.abs(got["cg_residual"] - ref["cg_residual"]) <= 1e-9 * ref["cg_residual"])


@pytest.mark.parametrize("cap", [60, 500])
def test_cg_tol_zero_never_divides_zero_by_zero(core, cap):
    """cg_tol = 0 leaves the end of a solve to the cap, on 27 unknowns.  At 60 iterations r is at 1e-71 |b|; at the
    default 500 the squares underflow near iteration 130, p.q is 0 and the iteration that would divide by it is
    not made (the numpy PCG ends the same way, within a few iterations).  R is finite and within 1e-12 of the
    numpy PCG's under the same arguments, with the same rounds run"""
    g = rc.graph("dense")
    args = rc.run_args("dense", cg_tol=0.0, cg_max_iters=cap)
    got = call(core, g, **args)
    with np.errstate(all="ignore"):
        ref = rc.restate_cg(g["N"], g["ij"], g["R_rel"], g["weight"], **args)
    print(f"dense, cg_tol 0, cap {cap}: CG iterations {got['cg_iters'].tolist()} (numpy PCG "
          f"{ref['cg_iters'].tolist()}), residuals {got['cg_residual'].tolist()}, steps {got['step'].tolist()}")
    assert np.all(np.isfinite(got["R"])) and np.all(np.isfinite(got["step"])) and np.all(np.isfinite(got["cg_residual"]))
    assert ref["margin"] > ra.MARGIN and ref["step_margin"] > rc.STEP_MARGIN and got["sweeps"] == ref["sweeps"]
    n = got["sweeps"]
    assert np.all(got["cg_iters"][:n] == 60) if cap == 60 else np.all((got["cg_iters"][:n] > 60) & (got["cg_iters"][:n] < 500))
    assert np.abs(got["R"] - ref["R"]).max() <= 1e-12 and np.array_equal(got["edge_inlier"], ref["edge_inlier"])


def test_exact_rounds_and_no_round(core):
    """tol = 0 runs all 4 rounds; tol = 1e-5 ends after the third, whose step is 1.8e-6; no round leaves stage 2's
    rotations bit for bit"""
    got, _ = check_stored(core, "medium", rounds=4, tol=0.0)
    assert got["sweeps"] == 4 and len(got["step"]) == 4 and np.all(got["step"] > 1e-5 * np.array([1, 1, 0, 0]))
    got, ref = check_stored(core, "medium", rounds=4, tol=1e-5)
    assert got["sweeps"] == 3 and got["step"][3] == 0.0 and ref["step_margin"] > rc.STEP_MARGIN
    g = rc.graph("medium")
    none = call(core, g, **rc.run_args("medium", rounds=0))
    stage2 = core.average_rotations(g["N"], g["ij"], g["R_rel"], max_sweeps=0, **rc.RUN)
    assert none["sweeps"] == 0 and len(none["cg_iters"]) == 0
    for k, n in enumerate(ra.OUTPUTS):
        assert np.asarray(none[n]).tobytes() == np.asarray(stage2[k]).tobytes(), n


# ------------------------------------------------------------------ what the refit is for
def test_convergence_at_the_defaults(core):
    """on `medium` the Jacobi refit's defaults end at max_sweeps 1.7e-4 rad from its fixed point; this refit at
    its defaults ends by tol before `rounds`, within 1e-8 rad of that fixed point (stored: the Jacobi restatement
    run to tol = 1e-12)"""
    g = rc.graph("medium")
    got = call(core, g, seed=rc.RUN["seed"])
    assert got["sweeps"] < rc.CG_DEFAULTS["rounds"] and got["step"][got["sweeps"] - 1] <= 1e-9
    fixed = rc.fixture()["medium_jacobi_R"]
    dist = ra.angle_between(got["R"], fixed).max()
    jacobi = core.average_rotations(g["N"], g["ij"], g["R_rel"], seed=rc.RUN["seed"])
    print(f"medium: {got['sweeps']} rounds, {dist:.3g} rad from the Jacobi fixed point; the Jacobi refit at its defaults "
          f"({jacobi[7]} sweeps): {ra.angle_between(jacobi[0], fixed).max():.3g} rad")
    assert dist <= 1e-8
    assert np.array_equal(got["edge_inlier"], jacobi[2])


def test_two_calls_give_identical_bytes(core):
    for name in ("weighted", "k8x37", "n257"):
        g = rc.graph(name)
        a, b = (call(core, g, **rc.run_args(name)) for _ in range(2))
        for n in rc.CG_OUTPUTS:
            assert np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes(), (name, n)


def test_the_default_refit_is_untouched(core):
    """refit="jacobi" is the default, returns the eight outputs it returned and equals the Jacobi restatement"""
    g = ra.stored_graph("medium")
    args = dict(seed=ra.FIXTURE_ARGS["seed"], threshold=ra.FIXTURE_ARGS["threshold"], consensus_sweeps=3,
                max_sweeps=30, tol=0.0)
    plain = core.average_rotations(g["N"], g["ij"], g["R_rel"], g["weight"], **args)
    named = core.average_rotations(g["N"], g["ij"], g["R_rel"], g["weight"], refit="jacobi", rounds=2, **args)
    assert len(plain) == len(named) == len(ra.OUTPUTS)
    ref = ra.stored_run("medium", 3, 30, 0.0)
    for k, n in enumerate(ra.OUTPUTS):
        assert np.asarray(plain[k]).tobytes() == np.asarray(named[k]).tobytes(), n
        if n in ra.INTEGER_OUTPUTS:
            assert np.array_equal(plain[k], ref[n]), n
    assert np.abs(plain[0] - ref["R"]).max() <= 1e-9 and np.abs(plain[1] - ref["edge_angle"]).max() <= 1e-9
    with pytest.raises(ValueError):
        core.average_rotations(g["N"], g["ij"], g["R_rel"], refit="gauss")


# ------------------------------------------------------------------ arguments
def raw_call(core, N, ij, R_rel, weight, threshold=0.1, cs=3, rounds=3, tol=0.0, cg_tol=1e-10, cg_max_iters=20,
             null=()):
    """the C entry itself on sentinel-filled outputs: (return code, outputs untouched); `null` lists the positions
    of the outputs passed as null pointers"""
    ij = np.ascontiguousarray(ij, dtype=np.int32).reshape(-1, 2)
    R_rel = np.ascontiguousarray(R_rel, dtype=np.float64)
    E, nr, n = len(ij), max(rounds, 1), max(N, 1)
    outs = [np.full((n, 9), 7.0), np.full(E, 7.0), np.full(E, 7, np.uint8)] + \
        [np.full(n, 7, np.int32) for _ in range(4)] + [np.full(1, 7, np.int32)] + \
        [np.full(nr, 7, np.int32), np.full(nr, 7.0), np.full(nr, 7.0)]
    P = core._p
    types = [core._d, core._d, core._u8] + [core._i32] * 6 + [core._d, core._d]
    ptrs = [None if k in null else P(o, t) for k, (o, t) in enumerate(zip(outs, types))]
    rc_ = core._lib.sfm_average_rotations_cg(N, P(ij, core._i32), P(R_rel), P(weight) if weight is not None else None,
                                             E, ctypes.c_uint64(0), threshold, cs, rounds, tol, cg_tol, cg_max_iters,
                                             *ptrs, core.DEVICE)
    return rc_, all(np.all(o == 7) for o in outs)


def test_argument_errors_leave_the_outputs_untouched(core):
    g = rc.graph("dense")
    N, ij, R_rel = g["N"], g["ij"], g["R_rel"]
    w = np.ones(len(ij))

    def edit(a, at, value):
        a = a.copy()
        a[at] = value
        return a
    cases = {
        "image out of range": dict(ij=edit(ij, (3, 1), N)),
        "negative image": dict(ij=edit(ij, (0, 0), -1)),
        "i == j": dict(ij=edit(ij, (2, 0), ij[2, 1])),
        "NaN in R_rel": dict(R_rel=edit(R_rel, (4, 1, 1), np.nan)),
        "inf in R_rel": dict(R_rel=edit(R_rel, (len(ij) - 1, 2, 2), np.inf)),
        "zero weight": dict(weight=edit(w, 5, 0.0)),
        "NaN weight": dict(weight=edit(w, 5, np.nan)),
        "threshold 0": dict(threshold=0.0),
        "threshold pi": dict(threshold=np.pi),
        "threshold NaN": dict(threshold=np.nan),
        "consensus_sweeps < 0": dict(cs=-1),
        "rounds < 0": dict(rounds=-1),
        "tol < 0": dict(tol=-1e-9),
        "tol NaN": dict(tol=np.nan),
        "cg_tol < 0": dict(cg_tol=-1e-12),
        "cg_tol NaN": dict(cg_tol=np.nan),
        "cg_tol inf": dict(cg_tol=np.inf),
        "cg_max_iters 0": dict(cg_max_iters=0),
        "n_images < 0": dict(N=-1, ij=np.zeros((0, 2), np.int32), R_rel=np.zeros((0, 3, 3))),
        "R null": dict(null=(0,)),
        "edge_angle null": dict(null=(1,)),
        "edge_inlier null": dict(null=(2,)),
        "group null": dict(null=(4,)),
        "sweeps null": dict(null=(7,)),
        "cg_iters null": dict(null=(8,)),
        "cg_residual null": dict(null=(9,)),
        "step null": dict(null=(10,)),
    }
    for name, change in cases.items():
        args = dict(N=N, ij=ij, R_rel=R_rel, weight=None)
        args.update(change)
        code, untouched = raw_call(core, **args)
        assert code == -1 and untouched, name
        assert core._lib.sfm_last_error().startswith(b"argument:"), name
    assert raw_call(core, N, ij, R_rel, w)[0] == 0
    # no round asks for none of the three new outputs, and cg_max_iters may be the largest int32
    code, untouched = raw_call(core, N, ij, R_rel, w, rounds=0, null=(8, 9, 10))
    assert code == 0 and not untouched
    assert raw_call(core, N, ij, R_rel, w, cg_max_iters=2 ** 31 - 1)[0] == 0
    for bad in (dict(cg_max_iters=0), dict(rounds=-1), dict(cg_tol=-1.0), dict(threshold=4.0)):
        with pytest.raises(core.SfmCoreError):
            core.average_rotations(N, ij, R_rel, refit="cg", **bad)


def test_timings_have_four_slots(core):
    g = rc.graph("medium")
    core.set_call_timing(True)
    try:
        call(core, g, **rc.run_args("medium"))
        t = core.last_timings()
        assert len(t) == 4 and np.all(t >= 0) and t[1] > 0 and 0 < t[3] <= t[1] * 1.05
    finally:
        core.set_call_timing(False)


# ------------------------------------------------------------------ the chain
def test_a_scene_from_verify_pairs_to_centres(core):
    """8 cameras on an arc around a cloud of points through verify_pairs, init_pairs, pair_rotations,
    average_rotations(refit="cg"), pair_directions and average_positions: all 8 cameras solved, and the same
    edge_inlier as with the Jacobi refit"""
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
    jacobi = mv.average_rotations(e_ij, e_R, n_img, weight=e_w)
    rotations = mv.average_rotations(e_ij, e_R, n_img, weight=e_w, refit="cg")
    order, out = rotations
    assert len(out) == len(rc.CG_OUTPUTS) and out[7] < rc.CG_DEFAULTS["rounds"] and out[10][out[7] - 1] <= 1e-9
    assert np.array_equal(out[2], jacobi[1][2]) and np.array_equal(order, jacobi[0])
    ref = rc.restate_cg(n_img, e_ij, e_R, e_w)
    assert ref["margin"] > ra.MARGIN and np.abs(out[0] - ref["R"]).max() <= 1e-12
    ij, dirs, w, keep = mv.pair_directions(verified, init, rotations)
    assert len(ij) >= 2 * n_img
    solved, pos = mv.average_positions(ij, dirs, n_img, weight=w)
    assert np.array_equal(solved, np.arange(n_img)) and pos[7] == n_img
    print(f"scene: {len(e_ij)} edges, {out[7]} rounds, CG iterations {out[8].tolist()}, steps {out[10].tolist()}; "
          f"largest angle to the Jacobi refit's rotations {ra.angle_between(out[0], jacobi[1][0]).max():.3g} rad")
