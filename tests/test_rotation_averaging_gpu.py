"""Global rotation averaging on a real MI355X (sfm_average_rotations,
sfm_multiview.average_rotations) against the numpy restatement of
tests/test_rotation_averaging.py.  Integer outputs are compared for equality; R
and edge_angle within 1e-9, the project's fp64 parity bound, with tol = 0 and
max_sweeps = 30 so that both sides run the same sweeps.  Every graph's
restatement also reports its least distance of a trace sum from tau, which must
exceed 1e-9: no decision then turns on the device's last bits.
"""
import ctypes

import numpy as np
import pytest

import test_rotation_averaging as ra

pytestmark = pytest.mark.gpu
SAME_SWEEPS = dict(max_sweeps=30, tol=0.0)


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


def compare(out, ref, bound=1e-9):
    assert ref["margin"] > ra.MARGIN
    got = dict(zip(ra.OUTPUTS, out))
    for n in ra.INTEGER_OUTPUTS:
        assert np.array_equal(got[n], ref[n]), n
    assert got["R"].shape == ref["R"].shape and got["edge_angle"].shape == ref["edge_angle"].shape
    for n in ("R", "edge_angle"):
        assert got[n].size == 0 or np.abs(got[n] - ref[n]).max() <= bound, n
    return got


def check(core, N, ij, R_rel, weight=None, **args):
    """the device call against the restatement under the same arguments; returns (device outputs, restatement)"""
    args = {**SAME_SWEEPS, **args}
    ref = ra.restate(N, ij, R_rel, weight, **args)
    return compare(core.average_rotations(N, ij, R_rel, weight, **args), ref), ref


def graph_on(R_true, ij, wrong, seed, noise_deg=1.0):
    """(ij, R_rel) measured on the edges ij, those listed in `wrong` replaced by random rotations -- each at least
    15 degrees from the truth, three thresholds: one drawn next to the truth would not be wrong"""
    ij = np.asarray(ij, dtype=np.int32).reshape(-1, 2)
    mask = np.zeros(len(ij), dtype=bool)
    mask[list(wrong)] = True
    R_rel = ra.measure(R_true, ij, noise_deg, mask, np.random.default_rng(seed))[0]
    truth = R_true[ij[:, 1]] @ np.swapaxes(R_true[ij[:, 0]], 1, 2)
    assert not mask.any() or np.rad2deg(ra.angle_between(R_rel[mask], truth[mask]).min()) > 15
    return ij, R_rel


# ------------------------------------------------------------------ trivial sizes
def test_trivial_sizes(core):
    rng = np.random.default_rng(1)
    none = np.zeros((0, 2), np.int32), np.zeros((0, 3, 3))
    check(core, 0, *none)
    got, _ = check(core, 3, *none)
    assert np.array_equal(got["info"], [-1, -1, -1]) and np.array_equal(got["group"], [0, 1, 2])
    R_true = ra.random_rotations(rng, 3)
    got, _ = check(core, 2, *graph_on(R_true, [[1, 0]], [], 2))
    assert np.array_equal(got["info"], [1, 0]) and np.array_equal(got["level"], [0, 1]) and got["edge_inlier"].all()
    # a triangle with one wrong edge: nodes 1 and 2 hold two predictions that disagree, each with support 1, and
    # take entry 0 -- for node 2 the wrong edge's; node 0 (the lowest of equal degree) is the root
    got, ref = check(core, 3, *graph_on(R_true, [[0, 2], [0, 1], [1, 2]], [0], 3), consensus_sweeps=1, max_sweeps=0)
    assert np.array_equal(got["info"], [1, 0, 0]) and np.array_equal(got["edge_inlier"], [True, True, False])


# ------------------------------------------------------------------ deep trees
def test_path_of_70_nodes(core):
    rng = np.random.default_rng(4)
    N = 70
    R_true = ra.random_rotations(rng, N)
    order = rng.permutation(N)  # the levels do not follow the node numbers
    ij = np.column_stack([order[:-1], order[1:]])
    got, _ = check(core, N, *graph_on(R_true, ij, [], 5))
    root = int(np.flatnonzero(got["info"] == 1)[0])
    assert got["level"].max() == max(np.flatnonzero(order == root)[0], N - 1 - np.flatnonzero(order == root)[0])
    ij2 = np.column_stack([np.arange(N - 1), np.arange(1, N)])  # root 1, 68 levels below it
    got, _ = check(core, N, *graph_on(R_true, ij2, [], 6))
    assert got["level"].max() == 68 and got["edge_inlier"].all() and np.all(got["group"] == 0)
    # the middle edge wrong.  A path has no loop, so nothing contradicts the wrong edge: the tree satisfies every
    # edge exactly, all of them are inliers in one group, and the wrong edge shows only against the truth, as the
    # offset of everything behind it.  Every node ends with an inlier edge or info -1.
    got, _ = check(core, N, *graph_on(R_true, ij2, [34], 7))
    assert got["edge_inlier"].all() and np.all(got["group"] == 0)
    assert np.all((got["n_inlier_edges"] > 0) | (got["info"] == -1))
    off = ra.angle_between(got["R"], ra.to_root_gauge(R_true, N, ij2))
    assert np.rad2deg(off[:35].max()) < 15 and np.rad2deg(off[35:].min()) > 15


# ------------------------------------------------------------------ high degree
def test_star_and_double_star_of_degree_300(core):
    rng = np.random.default_rng(8)
    R_true = ra.random_rotations(rng, 303)
    leaves = np.arange(1, 301)
    # the star: its centre, degree 300, is the root; every leaf has degree 1
    star = np.column_stack([np.zeros(300, np.int64), leaves])
    got, _ = check(core, 301, *graph_on(R_true, star, [], 9))
    assert got["info"][0] == 1 and np.all(got["level"][1:] == 1)
    # two hubs over the same leaves: hub 0 has one leaf more (302) and is the root, hub 301 moves with 301 entries,
    # more than one workgroup of 256; a third of its edges are wrong
    ij = np.vstack([star, np.column_stack([leaves, np.full(300, 301)]), [[301, 0]], [[0, 302]]])
    wrong = 300 + rng.choice(300, 100, replace=False)
    got, ref = check(core, 303, *graph_on(R_true, ij, wrong, 11))
    assert got["info"][0] == 1 and got["info"][301] == 0
    assert not got["edge_inlier"][wrong].any() and got["edge_inlier"].sum() == len(ij) - 100


@pytest.mark.parametrize("N", [65, 70, 130])
def test_complete_graphs(core, N):
    """degree 64 (a full wave), 69 (the 128-thread workgroup) and 129 (the 256-thread one)"""
    ij, R_rel, _, clean = ra.random_graph(N, 1.0, 1.0, 0.3, 30 + N)
    got, _ = check(core, N, ij, R_rel, max_sweeps=5)
    assert np.array_equal(got["edge_inlier"], clean)


# ------------------------------------------------------------------ mixed components
def test_components_duplicates_and_orientations(core):
    rng = np.random.default_rng(12)
    N = 21
    R_true = ra.random_rotations(rng, N)
    a, b = ra.random_graph(12, 0.6, 0.0, 0.0, 13)[0], ra.random_graph(8, 0.8, 0.0, 0.0, 14)[0] + 12
    dup = np.array([a[0], a[0], a[1][::-1], b[0][::-1], b[0]])  # the same pair twice, and both orientations
    ij = np.vstack([a, b, dup])
    ij, R_rel = graph_on(R_true, ij, [3, len(a) + 2, len(a) + len(b) + 1], 15)
    ij = np.vstack([ij, [[12, 13]]])  # a pendant edge's node keeps degree >= 1; node 20 stays isolated
    R_rel = np.concatenate([R_rel, (R_true[13] @ R_true[12].T)[None]])
    got, ref = check(core, N, ij, R_rel)
    roots = np.flatnonzero(got["info"] == 1)
    assert len(roots) == 2 and roots[0] < 12 <= roots[1]
    assert np.array_equal(got["R"][roots], np.tile(np.eye(3), (2, 1, 1)))  # the gauge, bit for bit
    assert got["info"][20] == -1 and got["group"][20] == 20 and got["level"][20] == 0
    assert np.array_equal(got["R"][20], np.eye(3))
    truth = ra.to_root_gauge(R_true, N, ij)
    assert np.rad2deg(ra.angle_between(got["R"][:20], truth[:20]).max()) < 2.0


# ------------------------------------------------------------------ the fixture graphs
@pytest.mark.parametrize("cs,ms,tol", ra.FIXTURE_RUNS[:4])
@pytest.mark.parametrize("name", sorted(ra.FIXTURE_GRAPHS))
def test_fixture_graphs(core, name, cs, ms, tol):
    g = ra.stored_graph(name)
    out = core.average_rotations(g["N"], g["ij"], g["R_rel"], g["weight"], seed=ra.FIXTURE_ARGS["seed"],
                                 threshold=ra.FIXTURE_ARGS["threshold"], consensus_sweeps=cs, max_sweeps=ms, tol=tol)
    got = compare(out, ra.stored_run(name, cs, ms, tol))
    assert got["sweeps"] == ms


def test_convergence_at_the_defaults(core):
    """the default tol ends the refit before max_sweeps on the dense fixture; the two sides may stop one sweep
    apart, and agree to 1e-6 rad: three orders above tol, five below the noise"""
    g = ra.stored_graph("dense")
    ref = ra.stored_run("dense", 3, 200, 1e-9)
    out = core.average_rotations(g["N"], g["ij"], g["R_rel"], seed=ra.FIXTURE_ARGS["seed"])
    got = dict(zip(ra.OUTPUTS, out))
    assert 1 <= got["sweeps"] < 200 and abs(got["sweeps"] - ref["sweeps"]) <= 1
    assert ra.angle_between(got["R"], ref["R"]).max() <= 1e-6
    assert np.array_equal(got["edge_inlier"], ref["edge_inlier"])


# ------------------------------------------------------------------ weights, determinism, arguments
def test_weights_move_a_node_toward_the_heavy_edge(core):
    rng = np.random.default_rng(16)
    R_true = ra.random_rotations(rng, 3)
    ij, R_rel = graph_on(R_true, [[0, 1], [0, 2], [1, 2], [1, 2]], [], 17, noise_deg=1.0)
    # node 2 hears edges 1, 2 and 3; edge 3 weighs 1,000
    heavy = np.array([1.0, 1.0, 1.0, 1000.0])
    plain, _ = check(core, 3, ij, R_rel)
    got, ref = check(core, 3, ij, R_rel, heavy)
    assert got["edge_angle"][3] < 0.1 * plain["edge_angle"][3]
    assert np.abs(got["R"] - plain["R"]).max() > 1e-6


def test_two_calls_give_identical_bytes(core):
    g = ra.stored_graph("weighted")
    outs = [core.average_rotations(g["N"], g["ij"], g["R_rel"], g["weight"], seed=3) for _ in range(2)]
    for a, b in zip(*outs):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def raw_call(core, N, ij, R_rel, weight, threshold=0.1, cs=3, ms=5, tol=0.0):
    """the C entry itself on sentinel-filled outputs: (return code, outputs untouched)"""
    ij = np.ascontiguousarray(ij, dtype=np.int32).reshape(-1, 2)
    R_rel = np.ascontiguousarray(R_rel, dtype=np.float64)
    E = len(ij)
    outs = [np.full((N, 9), 7.0), np.full(E, 7.0), np.full(E, 7, np.uint8)] + \
        [np.full(N, 7, np.int32) for _ in range(4)] + [np.full(1, 7, np.int32)]
    P = core._p
    types = [core._d, core._d, core._u8] + [core._i32] * 5
    rc = core._lib.sfm_average_rotations(N, P(ij, core._i32), P(R_rel), P(weight) if weight is not None else None, E,
                                         ctypes.c_uint64(0), threshold, cs, ms, tol,
                                         *[P(o, t) for o, t in zip(outs, types)], core.DEVICE)
    return rc, all(np.all(o == 7) for o in outs)


def test_argument_errors_leave_the_outputs_untouched(core):
    g = ra.stored_graph("dense")
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
        "max_sweeps < 0": dict(ms=-1),
        "tol < 0": dict(tol=-1e-9),
        "tol NaN": dict(tol=np.nan),
    }
    for name, change in cases.items():
        args = dict(N=N, ij=ij, R_rel=R_rel, weight=None)
        args.update(change)
        rc, untouched = raw_call(core, **args)
        assert rc == -1 and untouched, name
        assert core._lib.sfm_last_error().startswith(b"argument:"), name
    assert raw_call(core, N, ij, R_rel, w)[0] == 0
    with pytest.raises(core.SfmCoreError):
        core.average_rotations(N, ij, R_rel, threshold=4.0)


# ------------------------------------------------------------------ the chain
def test_pair_rotations_to_average_rotations(core):
    """sfm_multiview end to end from hand-built verify_pairs / init_pairs tuples of the documented shapes"""
    from sfm_multiview import average_rotations, pair_rotations
    N = 30
    ij, R_rel, R_true, clean = ra.random_graph(N, 0.4, 1.0, 0.3, 18)
    rng = np.random.default_rng(19)
    P = len(ij)
    n_good = rng.integers(30, 300, P).astype(np.int32)
    info = np.zeros(P, dtype=np.int32)
    drop = rng.choice(P, 10, replace=False)
    n_good[drop[:5]] = 12
    info[drop[5:]] = -2
    zeros = np.zeros(P)
    init_out = (R_rel, np.zeros((P, 3)), np.zeros((P, 4), np.int64), zeros, n_good, zeros, zeros, zeros,
                np.zeros((P, 3, 3)), info, np.zeros((0, 3)), np.zeros(0, bool), np.zeros(0))
    verified = (np.arange(P), ij, (np.zeros((P, 3, 3)),) + (zeros,) * 6, np.zeros(0, np.int64), np.zeros(0, np.int64))
    init = (np.arange(P), np.ones(P, bool), init_out, np.zeros(P + 1, np.int64), np.zeros(0, np.int64),
            np.zeros(0, np.int64))
    e_ij, e_R, e_w = pair_rotations(verified, init)
    keep = np.setdiff1d(np.arange(P), drop)
    assert np.array_equal(e_ij, ij[keep]) and np.array_equal(e_w, n_good[keep])
    order, out = average_rotations(e_ij, e_R, N, weight=e_w, seed=5, **SAME_SWEEPS)
    got = compare(out, ra.restate(N, e_ij, e_R, e_w, seed=5, **SAME_SWEEPS))
    assert np.array_equal(got["edge_inlier"], clean[keep])
    assert sorted(order) == list(range(N))
    size = np.bincount(got["group"], minlength=N)[got["group"]]
    assert np.all(np.diff(size[order]) <= 0) and size[order[0]] == size.max()
    k = int(size.max())
    assert np.array_equal(order[:k], np.flatnonzero(got["group"] == got["group"][order[0]]))
    truth = ra.to_root_gauge(R_true, N, e_ij)
    assert np.rad2deg(ra.angle_between(got["R"][order[:k]], truth[order[:k]]).max()) < 2.0
