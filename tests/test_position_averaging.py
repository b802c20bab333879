"""Global position averaging (sfm_average_positions): the plain-numpy
restatement of its rounds, the synthetic view graphs, and the CPU tests that
pin the algorithm.  No GPU: the device call is compared with the stored
restatement in tests/test_position_averaging_gpu.py.

The restatement follows include/sfmcore.h: leaf pruning, the largest component
and its root, then per round the 3 (M - 1) system assembled densely and solved
with np.linalg.solve (`solver="dense"`), or solved by the preconditioned
conjugate gradients of the header in vectorised numpy (`solver="pcg"`), the
division by c and the new weights and targets.  The gap between the two solvers
at the device tests' cg_tol is stored per graph as `cg_gap`; it sets the
device's tolerance (see tolerance()).

Graphs a to e are stored with their restatement in position_averaging.npz.  The
lane-width graphs (LANE_GRAPHS), built so that the host's plan reaches every
group width, the clamp and the bound of path 1 and grids past one workgroup's
worth of partials, are regenerated from their seeds and checked by hash;
position_averaging_lanes.npz stores their dense restatement's centres alone
(tests/golden/make_golden_position_lanes.py).
"""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN

DEFAULTS = dict(mu=0.01, sigma=np.deg2rad(3), threshold=np.deg2rad(5), rounds=12, cg_tol=1e-12, cg_max_iters=2000)
FLOOR = 1e-3
MASK_MARGIN = 1e-6  # every stored graph's final angles keep this far from the threshold
PATH1_MAX_NODES = 512


# ------------------------------------------------------------------ the graph that is solved
def unit(d):
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    d = d / np.abs(d).max(axis=1, keepdims=True)
    return d / np.sqrt((d * d).sum(axis=1, keepdims=True))


def select(N, ij):
    """(solved (N,) bool, root): leaf pruning, the largest component (the lowest node on ties), its node with the
    most entries among the edges between solved nodes (the lowest on ties); root = -1 where nothing is left"""
    ij = np.asarray(ij, dtype=np.int64).reshape(-1, 2)
    alive = np.zeros(N, dtype=bool)
    alive[np.unique(ij)] = True
    while True:
        e = ij[alive[ij[:, 0]] & alive[ij[:, 1]]]
        lo, hi = np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1])
        simple = np.unique(np.column_stack([lo, hi]), axis=0) if len(e) else np.zeros((0, 2), np.int64)
        distinct = np.bincount(simple.ravel(), minlength=N)
        drop = alive & (distinct < 2)
        if not drop.any():
            break
        alive &= ~drop
    if not alive.any():
        return alive, -1
    label = np.arange(N)
    e = ij[alive[ij[:, 0]] & alive[ij[:, 1]]]
    while True:
        m = np.minimum(label[e[:, 0]], label[e[:, 1]])
        new = label.copy()
        np.minimum.at(new, e[:, 0], m)
        np.minimum.at(new, e[:, 1], m)
        if np.array_equal(new, label):
            break
        label = new
    size = np.bincount(label[alive], minlength=N)
    solved = alive & (label == int(np.argmax(size)))  # argmax: the first (lowest label) of equals
    inner = ij[solved[ij[:, 0]] & solved[ij[:, 1]]]
    entries = np.bincount(inner.ravel(), minlength=N)
    return solved, int(np.argmax(np.where(solved, entries, -1)))


# ------------------------------------------------------------------ the two solvers
def edge_blocks(d, w, mu):
    return w[:, None, None] * (np.eye(3) - (1.0 - mu) * d[:, :, None] * d[:, None, :])


def rhs(M, i, j, d, w, s, mu):
    b = np.zeros((M, 3))
    np.add.at(b, j, (mu * w * s)[:, None] * d)
    np.add.at(b, i, -(mu * w * s)[:, None] * d)
    return b


def solve_dense(M, root, i, j, d, w, s, mu):
    B = edge_blocks(d, w, mu)
    A = np.zeros((M, 3, M, 3))
    np.add.at(A, (i, slice(None), i), B)   # two index arrays around a slice address (E, 3, 3): [edge, row, column]
    np.add.at(A, (j, slice(None), j), B)
    np.add.at(A, (i, slice(None), j), -B)
    np.add.at(A, (j, slice(None), i), -B)
    b = rhs(M, i, j, d, w, s, mu)
    free = np.flatnonzero(np.arange(M) != root)
    idx = (3 * free[:, None] + np.arange(3)).ravel()
    x = np.zeros((M, 3))
    x[free] = np.linalg.solve(A.reshape(3 * M, 3 * M)[np.ix_(idx, idx)], b.reshape(-1)[idx]).reshape(-1, 3)
    return x, 0, 0.0


def inv3(D):
    """the inverses of symmetric 3 x 3 blocks (M, 3, 3) by cofactors, in the blocks' own number format"""
    a, b, c, d, e, f = D[:, 0, 0], D[:, 0, 1], D[:, 0, 2], D[:, 1, 1], D[:, 1, 2], D[:, 2, 2]
    A, B, C = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * A + b * B + c * C
    rows = [[A, B, C], [B, a * f - c * c, b * c - a * e], [C, b * c - a * e, a * d - b * b]]
    return np.stack([np.stack(row, axis=1) for row in rows], axis=1) / det[:, None, None]


def solve_pcg(M, root, i, j, d, w, s, mu, x0, cg_tol, cg_max_iters, dtype=np.float64, precond="blocks"):
    """the header's PCG carried in `dtype`; precond "blocks": the 3 x 3 diagonal blocks' inverses, "identity": none
    (the count it needs is what a solver with a useless preconditioner would report)"""
    one = np.eye(3, dtype=dtype)
    B = w[:, None, None] * (one - (1.0 - mu) * d[:, :, None] * d[:, None, :])
    D = np.zeros((M, 3, 3), dtype=dtype)
    np.add.at(D, i, B)
    np.add.at(D, j, B)
    D[root] = one
    Dinv = inv3(D) if precond == "blocks" else np.broadcast_to(one, (M, 3, 3))
    free = (np.arange(M) != root).astype(dtype)

    def op(p):
        u = p[i] - p[j]
        f = w[:, None] * (u - (1.0 - mu) * d * (d * u).sum(axis=1, keepdims=True))
        q = np.zeros((M, 3), dtype=dtype)
        np.add.at(q, i, f)
        np.add.at(q, j, -f)
        return q * free[:, None]

    def prec(r):
        return (Dinv * r[:, None, :]).sum(axis=2) * free[:, None]

    ws = (mu * w * s)[:, None] * d
    b = np.zeros((M, 3), dtype=dtype)
    np.add.at(b, j, ws)
    np.add.at(b, i, -ws)
    b = b * free[:, None]
    x = x0.copy()
    r = b - op(x)
    z = prec(r)
    p = z.copy()
    rho = (r * z).sum()
    bn, k = np.sqrt((b * b).sum()), 0
    rn = np.sqrt((r * r).sum())
    while k < cg_max_iters and rn > cg_tol * bn:
        q = op(p)
        alpha = rho / (p * q).sum()
        x += alpha * p
        r -= alpha * q
        z = prec(r)
        rho_new = (r * z).sum()
        p = z + (rho_new / rho) * p
        rho = rho_new
        rn = np.sqrt((r * r).sum())
        k += 1
    return x, k, (float(rn / bn) if bn > 0 else 0.0)


def edge_geometry(d, v):
    """(theta, d.v, |v|) of the unit directions d against the baselines v = C_j - C_i"""
    proj = (d * v).sum(axis=1)
    cr = np.cross(d, v)
    return np.arctan2(np.sqrt((cr * cr).sum(axis=1)), proj), proj, np.sqrt((v * v).sum(axis=1))


def edge_outputs(pair_ij, dir, C, info, threshold=DEFAULTS["threshold"]):
    """(edge_angle, edge_length, edge_inlier, margin) that belong to the centres C: the one formula of the call's
    three edge outputs, on the edges between solved nodes (info >= 0), zero on the others; margin is the least
    |theta - threshold| over the former"""
    ij = np.asarray(pair_ij, dtype=np.int64).reshape(-1, 2)
    solved = np.asarray(info) >= 0
    edges = np.flatnonzero(solved[ij[:, 0]] & solved[ij[:, 1]])
    C = np.asarray(C)
    theta, proj, _ = edge_geometry(unit(dir)[edges].astype(C.dtype), C[ij[edges, 1]] - C[ij[edges, 0]])
    angle, length, inlier = np.zeros(len(ij), C.dtype), np.zeros(len(ij), C.dtype), np.zeros(len(ij), bool)
    angle[edges], length[edges], inlier[edges] = theta, proj, theta <= threshold
    return angle, length, inlier, (float(np.abs(theta - threshold).min()) if len(edges) else np.inf)


def restate(n_images, pair_ij, dir, weight=None, mu=0.01, sigma=np.deg2rad(3), threshold=np.deg2rad(5), rounds=12,
            cg_tol=1e-12, cg_max_iters=2000, solver="dense", dtype=np.float64, precond="blocks"):
    """sfm_average_positions in numpy.  Returns a dict of its outputs, plus `c` (rounds,) and `margin`, the least
    |theta - threshold| over the solved edges.  `dtype` is the number format the PCG, the normalisation and the
    reweighting are carried in (the inputs are the same doubles); C and the edge outputs come back in it."""
    N = int(n_images)
    ij = np.asarray(pair_ij, dtype=np.int64).reshape(-1, 2)
    E = len(ij)
    out = dict(C=np.zeros((N, 3), dtype), edge_angle=np.zeros(E, dtype), edge_inlier=np.zeros(E, bool),
               edge_length=np.zeros(E, dtype), info=np.full(N, -1, np.int32), cg_iters=np.zeros(rounds, np.int32),
               cg_residual=np.zeros(rounds), n_solved=0, c=np.zeros(rounds), margin=np.inf)
    if N == 0 or E == 0:
        return out
    solved, root_g = select(N, ij)
    if root_g < 0:
        return out
    nodes = np.flatnonzero(solved)
    local = np.full(N, -1)
    local[nodes] = np.arange(len(nodes))
    edges = np.flatnonzero(solved[ij[:, 0]] & solved[ij[:, 1]])
    i, j = local[ij[edges, 0]], local[ij[edges, 1]]
    assert solver == "pcg" or dtype == np.float64, "the dense solve is LAPACK's, in float64"
    d = unit(dir)[edges].astype(dtype)
    w0 = (np.ones(len(edges)) if weight is None else np.asarray(weight, dtype=np.float64)[edges]).astype(dtype)
    M, root = len(nodes), int(local[root_g])
    w, s, x = w0.copy(), np.ones(len(edges), dtype), np.zeros((M, 3), dtype)
    for rnd in range(rounds):
        if solver == "dense":
            x, k, res = solve_dense(M, root, i, j, d, w, s, mu)
        else:
            x, k, res = solve_pcg(M, root, i, j, d, w, s, mu, x, cg_tol, cg_max_iters, dtype, precond)
        out["cg_iters"][rnd], out["cg_residual"][rnd] = k, res
        c = (w * (d * (x[j] - x[i])).sum(axis=1)).sum() / w.sum()
        out["c"][rnd] = float(c)
        assert np.isfinite(c) and c > 0, "SFM_ERR_NUMERIC"
        x = x / c
        theta, proj, length = edge_geometry(d, x[j] - x[i])
        s = np.maximum(proj, FLOOR)
        w = w0 / ((1.0 + (theta / sigma) ** 2) * np.maximum(length, FLOOR) ** 2)
    out["C"][nodes] = x
    out["info"][nodes] = 0
    out["info"][root_g] = 1
    out["n_solved"] = M
    out["edge_angle"], out["edge_length"], out["edge_inlier"], out["margin"] = edge_outputs(
        ij, dir, out["C"], out["info"], threshold)
    return out


def align(C, truth):
    """the largest distance of s C + t from the truth over the best scale s and translation t (least squares)"""
    a, b = C - C.mean(axis=0), truth - truth.mean(axis=0)
    scale = float((a * b).sum() / (a * a).sum())
    return float(np.linalg.norm(scale * a - b, axis=1).max())


# ------------------------------------------------------------------ the graphs
def random_unit(rng, n):
    return unit(rng.normal(size=(n, 3)))


def measure(centres, ij, noise_deg, wrong, rng):
    """directions C_j - C_i with a rotation of noise_deg RMS about a random axis, the `wrong` ones uniform"""
    ij = np.asarray(ij, dtype=np.int64).reshape(-1, 2)
    d = unit(centres[ij[:, 1]] - centres[ij[:, 0]])
    if noise_deg > 0:
        t = rng.normal(0, np.deg2rad(noise_deg) / np.sqrt(2), (len(d), 3))
        t -= d * (d * t).sum(axis=1, keepdims=True)  # a tangent offset: two free components
        d = unit(d + t)
    wrong = np.asarray(wrong, dtype=bool)
    d[wrong] = random_unit(rng, int(wrong.sum()))
    return np.ascontiguousarray(d)


def orient(rng, i, j):
    flip = rng.random(len(i)) < 0.5
    return np.column_stack([np.where(flip, j, i), np.where(flip, i, j)]).astype(np.int32)


def pick_wrong(rng, E, frac):
    wrong = np.zeros(E, dtype=bool)
    wrong[rng.choice(E, int(round(frac * E)), replace=False)] = True
    return wrong


def box_graph(seed, noise_deg, wrong_frac, N=30, density=0.44):
    """N cameras in a 10 x 10 x 2 box, every pair an edge with probability `density`"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, (N, 3)) * [10.0, 10.0, 2.0]
    a, b = np.triu_indices(N, 1)
    keep = rng.random(len(a)) < density
    ij = orient(rng, a[keep], b[keep])
    rng2 = np.random.default_rng(seed + 1000)  # the same graph for every noise setting
    wrong = pick_wrong(rng2, len(ij), wrong_frac)
    return dict(N=N, ij=ij, dir=measure(centres, ij, noise_deg, wrong, rng2), weight=None, truth=centres, clean=~wrong)


def hub_graph(seed, N=300):
    """node 0 joined to every other node (degree N - 1), the others on a ring with chords"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, (N, 3)) * [10.0, 10.0, 4.0]
    others = np.arange(1, N)
    ring = np.column_stack([others, np.roll(others, -1)])
    chords = np.vstack([np.column_stack([others, np.roll(others, -7)]), np.column_stack([others, np.roll(others, -31)])])
    pairs = np.vstack([np.column_stack([np.zeros(N - 1, np.int64), others]), ring, chords])
    ij = orient(rng, pairs[:, 0], pairs[:, 1])
    assert len(ij) % 64 != 0
    wrong = pick_wrong(rng, len(ij), 0.02)
    weight = rng.integers(30, 400, len(ij)).astype(np.float64)
    return dict(N=N, ij=ij, dir=measure(centres, ij, 1.0, wrong, rng), weight=weight, truth=centres, clean=~wrong)


def sparse_graph(seed, N=1100, per_node=5):
    """every node draws per_node partners: about 2 per_node entries a node, past path 1's bound"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, (N, 3)) * [20.0, 20.0, 5.0]
    a = np.repeat(np.arange(N), per_node)
    b = rng.integers(0, N, len(a))
    ok = a != b
    lo, hi = np.minimum(a[ok], b[ok]), np.maximum(a[ok], b[ok])
    pairs = np.unique(np.column_stack([lo, hi]), axis=0)
    ij = orient(rng, pairs[:, 0], pairs[:, 1])
    wrong = pick_wrong(rng, len(ij), 0.05)
    return dict(N=N, ij=ij, dir=measure(centres, ij, 1.0, wrong, rng), weight=None, truth=centres, clean=~wrong)


def hand_graph(seed):
    """nodes 0-7 a complete core; 3 - 8 - 9 a chain of two leaves; 10-14 a complete second component; 15 alone.
    One pair twice and one in both orientations."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, (16, 3)) * [6.0, 6.0, 3.0]
    a, b = np.triu_indices(8, 1)
    core = np.column_stack([a, b])
    a, b = np.triu_indices(5, 1)
    second = np.column_stack([a, b]) + 10
    pairs = np.vstack([core[:10], [[3, 8], [8, 9]], second, core[10:], [[0, 1], [2, 1], [9, 8]]])
    ij = pairs.astype(np.int32)
    return dict(N=16, ij=ij, dir=measure(centres, ij, 0.5, np.zeros(len(ij), bool), rng), weight=None, truth=centres,
                clean=np.ones(len(ij), bool))


# The graphs below are built for the plan they make the host choose (csrc/position_plan.hpp): the lanes G per node
# double at 8, 16, .. 256 mean entries a node, path 1 clamps G to 512 / M.  1 degree of noise, 3 % wrong edges.
def measured_graph(rng, centres, pairs, weighted=False, wrong_frac=0.03):
    ij = orient(rng, pairs[:, 0], pairs[:, 1])
    wrong = pick_wrong(rng, len(ij), wrong_frac)
    weight = rng.integers(30, 400, len(ij)).astype(np.float64) if weighted else None
    return dict(N=len(centres), ij=ij, dir=measure(centres, ij, 1.0, wrong, rng), weight=weight, truth=centres,
                clean=~wrong)


def complete_graph(seed, N, copies=1, weighted=False):
    """every pair of N nodes `copies` times; a copy is a second measurement: its own noise and orientation"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, (N, 3)) * [10.0, 10.0, 4.0]
    a, b = np.triu_indices(N, 1)
    return measured_graph(rng, centres, np.tile(np.column_stack([a, b]), (copies, 1)), weighted)


def random_graph(seed, N, degree):
    """every pair of N nodes an edge with probability degree / (N - 1)"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, (N, 3)) * [10.0, 10.0, 4.0]
    a, b = np.triu_indices(N, 1)
    keep = rng.random(len(a)) < degree / (N - 1)
    return measured_graph(rng, centres, np.column_stack([a[keep], b[keep]]))


def core_graph(seed, core=120, outer=120):
    """a complete core, and outer nodes with 2 or 3 edges each into it: half the nodes have fewer entries than a
    group sized by the mean has lanes"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 1, (core + outer, 3)) * [10.0, 10.0, 4.0]
    a, b = np.triu_indices(core, 1)
    spokes = []
    for n in range(core, core + outer):
        inner = rng.choice(core, int(rng.integers(2, 4)), replace=False)
        spokes.append(np.column_stack([inner, np.full(len(inner), n)]))
    return measured_graph(rng, centres, np.vstack([np.column_stack([a, b])] + spokes))


# name: (generator, rounds, ((path asked for, path that must run), ..))
LANE_GRAPHS = {
    "dense100": (lambda: random_graph(51, 100, 24), 12, ((1, 1), (2, 2))),
    "k64": (lambda: complete_graph(52, 64), 12, ((1, 1), (2, 2))),
    "k32x3": (lambda: complete_graph(53, 32, 3), 12, ((1, 1), (2, 2))),
    "k16x9": (lambda: complete_graph(54, 16, 9, weighted=True), 12, ((1, 1), (2, 2))),
    "k8x37": (lambda: complete_graph(55, 8, 37), 12, ((1, 1), (2, 2))),
    "k200": (lambda: complete_graph(56, 200), 12, ((1, 1), (2, 2))),
    "core120": (lambda: core_graph(57), 12, ((1, 1), (2, 2))),
    "clamp256": (lambda: random_graph(58, 256, 20), 12, ((1, 1), (2, 2))),
    "clamp257": (lambda: random_graph(59, 257, 20), 12, ((1, 1), (2, 2))),
    "bound512": (lambda: sparse_graph(60, N=512), 12, ((0, 1), (1, 1), (2, 2))),
    "bound513": (lambda: sparse_graph(61, N=513), 12, ((0, 2),)),
    "dense300": (lambda: random_graph(62, 300, 280), 12, ((2, 2),)),
    "dense1100": (lambda: random_graph(63, 1100, 290), 2, ((2, 2),)),
}
ITERATIONS_NOT_ASSERTED = ("e", "k8x37")  # 8 nodes, 21 unknowns: CG ends there with any preconditioner (iterations_tell)
CAPS = (1, 7, 8, 9, 16)  # cg_max_iters around path 2's batch of 8 launches, on graph b at two rounds
CAP_ROUNDS = 2

FIXTURE_GRAPHS = {"a": lambda: box_graph(41, 0.0, 0.0), "b": lambda: box_graph(41, 1.0, 0.10),
                  "c": lambda: hub_graph(42), "d": lambda: sparse_graph(43), "e": lambda: hand_graph(44)}
OUTPUTS = ("C", "edge_angle", "edge_inlier", "edge_length", "info", "cg_iters", "cg_residual", "n_solved")

_fixture = {}


def fixture():
    if not _fixture:
        _fixture.update(np.load(os.path.join(GOLDEN, "position_averaging.npz")))
    return _fixture


def stored_graph(name):
    fx = fixture()
    weight = fx[name + "_weight"] if name + "_weight" in fx else None
    return dict(N=int(fx[name + "_N"]), ij=fx[name + "_ij"], dir=fx[name + "_dir"], weight=weight,
                truth=fx[name + "_truth"], clean=fx[name + "_clean"])


def stored_out(name):
    fx = fixture()
    return {k: fx[f"{name}_out_{k}"] for k in ("C", "edge_angle", "edge_inlier", "edge_length", "info", "n_solved")}


def gaps(a, b):
    """the gap between two results: C and edge_length relative to the largest |C|, edge_angle in radians"""
    scale = np.abs(b["C"]).max()
    return max(np.abs(a["C"] - b["C"]).max() / scale, np.abs(a["edge_length"] - b["edge_length"]).max() / scale,
               np.abs(a["edge_angle"] - b["edge_angle"]).max())


def tolerance(name):
    """What the device may differ by from the dense restatement on a stored graph: 100 x the gap that the numpy
    PCG at the same cg_tol leaves to the dense solve (a different summation order, amplified by a condition
    number of about 1e3), and no less than 1e-12.  The gap is the largest of three: C and edge_length relative to
    the largest |C|, edge_angle in radians."""
    return max(100.0 * float(fixture()[name + "_cg_gap"]), 1e-12)


_runs = {}


def run(name):
    """the dense restatement on a stored graph at the defaults, computed once and shared"""
    if name not in _runs:
        g = stored_graph(name)
        _runs[name] = restate(g["N"], g["ij"], g["dir"], g["weight"], **DEFAULTS)
    return _runs[name]


# ------------------------------------------------------------------ the lane-width graphs: regenerated, not stored
_lanes, _lane_graphs, _lane_refs = {}, {}, {}


def lanes_fixture():
    """position_averaging_lanes.npz: per graph of LANE_GRAPHS the dense restatement's C, info and n_solved, its
    margin, cg_gap, the numpy PCG's iteration counts with the block preconditioner and with none, and the SHA-256 of
    the generated ij and dir; the two iteration counts for graphs a to e as well; the capped solves' gaps"""
    if not _lanes:
        _lanes.update(np.load(os.path.join(GOLDEN, "position_averaging_lanes.npz")))
    return _lanes


def graph_hash(g):
    ij, d = np.ascontiguousarray(g["ij"], dtype=np.int32), np.ascontiguousarray(g["dir"], dtype=np.float64)
    return hashlib.sha256(ij.tobytes() + d.tobytes()).hexdigest()


def lane_graph(name):
    """the graph regenerated from its seed, once; refused if its bytes are not the ones the fixture was made from"""
    if name not in _lane_graphs:
        g = LANE_GRAPHS[name][0]()
        assert graph_hash(g) == str(lanes_fixture()[name + "_sha256"]), f"{name}: the generator's stream has changed"
        _lane_graphs[name] = g
    return _lane_graphs[name]


def lane_reference(name):
    """the stored dense restatement of a lane-width graph, its edge outputs recomputed from the stored C"""
    if name not in _lane_refs:
        fx, g = lanes_fixture(), lane_graph(name)
        C, info = fx[name + "_C"], fx[name + "_info"]
        angle, length, inlier, margin = edge_outputs(g["ij"], g["dir"], C, info)
        assert margin > MASK_MARGIN
        _lane_refs[name] = dict(C=C, info=info, n_solved=int(fx[name + "_n_solved"]), edge_angle=angle,
                                edge_length=length, edge_inlier=inlier)
    return _lane_refs[name]


def lane_tolerance(name):
    """tolerance()'s rule on a lane-width graph"""
    return max(100.0 * float(lanes_fixture()[name + "_cg_gap"]), 1e-12)


def iteration_bound(pcg_iters):
    """The most CG iterations a round may take on the device: the numpy PCG's count and max(2, 10 %) more.  The stop
    compares a residual that falls by a roughly constant factor per iteration, so another summation order moves the
    crossing by an iteration or two; a wrong D^-1 is still a positive definite preconditioner, converges to the same
    answer and costs a multiple."""
    pcg_iters = np.asarray(pcg_iters, dtype=np.int64)
    return pcg_iters + np.maximum(2, pcg_iters // 10)


def iteration_counts(name):
    """(the numpy PCG's counts per round, the same without a preconditioner) of a stored or a lane-width graph"""
    fx = lanes_fixture()
    pcg = fixture()[name + "_pcg_iters"] if name in FIXTURE_GRAPHS else fx[name + "_pcg_iters"]
    return pcg, fx[name + "_ident_iters"]


def iterations_tell(name):
    """does the bound on the iteration count tell a useless preconditioner from the right one on this graph?  Only
    where the unpreconditioned count passes the bound in every round; elsewhere the assertion is not made."""
    pcg, ident = iteration_counts(name)
    return bool(np.all(ident > iteration_bound(pcg)))


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", sorted(LANE_GRAPHS))
def test_lane_graphs_regenerate_to_the_stored_hash(name):
    fx, g = lanes_fixture(), lane_graph(name)  # lane_graph asserts the hash
    solved, _ = select(g["N"], g["ij"])
    assert int(solved.sum()) == int(fx[name + "_n_solved"]) and np.array_equal(solved, fx[name + "_info"] >= 0)
    assert float(fx[name + "_margin"]) > MASK_MARGIN and len(fx[name + "_pcg_iters"]) == LANE_GRAPHS[name][1]
    assert np.all(fx[name + "_pcg_iters"] < DEFAULTS["cg_max_iters"])
    assert (g["weight"] is not None) == (name == "k16x9")  # the one weighted case
    if name.startswith("bound"):
        assert int(fx[name + "_n_solved"]) == g["N"]  # every node solved: the two sides of path 1's bound


@pytest.mark.parametrize("name", sorted(FIXTURE_GRAPHS))
def test_edge_outputs_from_the_stored_centres(name):
    """the helper that turns stored centres into edge references, on graphs a to e against their stored edge
    outputs: the same formula on the same doubles, so only libm's last bits of atan2 and sqrt may differ"""
    g, ref = stored_graph(name), stored_out(name)
    angle, length, inlier, margin = edge_outputs(g["ij"], g["dir"], ref["C"], ref["info"])
    assert np.array_equal(inlier, ref["edge_inlier"]) and margin > MASK_MARGIN
    assert np.abs(angle - ref["edge_angle"]).max() <= 1e-14 and np.abs(length - ref["edge_length"]).max() <= 1e-13
    dead = ~((ref["info"] >= 0)[g["ij"][:, 0]] & (ref["info"] >= 0)[g["ij"][:, 1]])
    assert not angle[dead].any() and not length[dead].any() and not inlier[dead].any()


def test_the_long_double_restatement_is_wider_than_double():
    """the capped solves are compared with a PCG carried in np.longdouble: it must be the 80-bit format, and at
    the defaults it must land on the float64 PCG's answer"""
    assert np.finfo(np.longdouble).eps < 1e-18
    g = stored_graph("e")
    wide = restate(g["N"], g["ij"], g["dir"], g["weight"], solver="pcg", dtype=np.longdouble, **DEFAULTS)
    assert wide["C"].dtype == np.longdouble and gaps(wide, run("e")) <= 1e-12
    assert np.array_equal(wide["edge_inlier"], run("e")["edge_inlier"])


def test_which_graphs_carry_the_iteration_count_assertion():
    """the graphs on which the device's cg_iters is held to iteration_bound() are those where the numpy PCG
    without a preconditioner passes it in every round; the others are named here and in DESIGN.md"""
    dropped = {n for n in list(FIXTURE_GRAPHS) + list(LANE_GRAPHS) if not iterations_tell(n)}
    assert dropped == set(ITERATIONS_NOT_ASSERTED)


@pytest.mark.parametrize("name", sorted(FIXTURE_GRAPHS))
def test_generator_reproduces_the_stored_graphs(name):
    g, s = FIXTURE_GRAPHS[name](), stored_graph(name)
    assert g["N"] == s["N"] and np.array_equal(g["ij"], s["ij"]) and np.array_equal(g["clean"], s["clean"])
    assert np.abs(g["dir"] - s["dir"]).max() < 1e-14 and np.abs(g["truth"] - s["truth"]).max() < 1e-12
    assert (g["weight"] is None) == (s["weight"] is None)
    if g["weight"] is not None:
        assert np.array_equal(g["weight"], s["weight"])


@pytest.mark.parametrize("name", sorted(FIXTURE_GRAPHS))
def test_restatement_against_the_fixture(name):
    """Integers exactly; the rest within 1e-9 of the largest |C| (radians for the angles): LAPACK builds differ in
    the last bits of a solve of condition 1e3 and twelve rounds carry that along, far below any mask margin"""
    out, ref = run(name), stored_out(name)
    assert out["n_solved"] == int(ref["n_solved"]) and np.array_equal(out["info"], ref["info"])
    assert np.array_equal(out["edge_inlier"], ref["edge_inlier"])
    assert gaps(out, ref) < 1e-9
    assert out["margin"] > MASK_MARGIN and np.all(out["c"] > 0)


def test_exact_directions_recover_the_truth():
    """graph (a): the error after aligning scale and translation, against 10 x what it was when the fixture was
    written (the factor covers BLAS differences between hosts)"""
    g, out = stored_graph("a"), run("a")
    assert out["n_solved"] == g["N"]
    assert align(out["C"], g["truth"]) <= 10.0 * float(fixture()["a_truth_error"])


def test_noisy_graph_keeps_exactly_the_clean_edges():
    g, out = stored_graph("b"), run("b")
    assert out["n_solved"] == g["N"] and np.array_equal(out["edge_inlier"], g["clean"])


def test_pruning_components_and_root_of_the_hand_graph():
    g = stored_graph("e")
    solved, root = select(g["N"], g["ij"])
    assert np.array_equal(np.flatnonzero(solved), np.arange(8))
    deg = np.bincount(g["ij"][np.all(g["ij"] < 8, axis=1)].ravel(), minlength=8)
    assert root == int(np.argmax(deg)) and deg[root] == deg.max()
    out = run("e")
    assert np.array_equal(out["info"] >= 0, solved) and out["info"][root] == 1 and out["n_solved"] == 8
    dead = ~(solved[g["ij"][:, 0]] & solved[g["ij"][:, 1]])
    assert dead.sum() == 2 + 10 + 1 and not out["edge_angle"][dead].any() and not out["C"][8:].any()
    # ties: two triangles, the one with the lower nodes is solved; the root the lowest node of equal degree
    two = np.array([[3, 4], [4, 5], [5, 3], [0, 1], [1, 2], [2, 0]])
    solved, root = select(6, two)
    assert solved.tolist() == [True] * 3 + [False] * 3 and root == 0
    assert select(4, np.array([[0, 1], [1, 2], [2, 3]]))[1] == -1  # a path prunes away entirely


def test_the_two_solvers_agree_to_the_stored_gap():
    """the numpy PCG of the header against the dense solve, on the small graphs: within 10 x the stored gap"""
    for name in ("a", "b", "e"):
        g = stored_graph(name)
        pcg = restate(g["N"], g["ij"], g["dir"], g["weight"], solver="pcg", **DEFAULTS)
        assert gaps(pcg, run(name)) <= max(10.0 * float(fixture()[name + "_cg_gap"]), 1e-12), name
        assert np.all(pcg["cg_iters"] < DEFAULTS["cg_max_iters"]) and np.all(pcg["cg_residual"] <= 1e-12)


def test_pair_directions_convention():
    """R_i^T C_rel is the unit vector from C_i to C_j for cameras x_cam = R (X - C); the pairs kept are
    pair_rotations' with edge_inlier set and both images in the first group"""
    import sfm_synthetic as syn
    from sfm_multiview import pair_directions, pair_rotations
    rng = np.random.default_rng(5)
    n = 6
    R = syn.rotvec_to_matrix(rng.normal(0, 0.4, (n, 3)))
    Cw = rng.uniform(-3, 3, (n, 3))
    a, b = np.triu_indices(n, 1)
    pair_ij = np.column_stack([a, b]).astype(np.int32)
    P = len(pair_ij)
    C_rel = unit(np.einsum("eij,ej->ei", R[pair_ij[:, 0]], Cw[pair_ij[:, 1]] - Cw[pair_ij[:, 0]]))
    R_rel = R[pair_ij[:, 1]] @ np.swapaxes(R[pair_ij[:, 0]], 1, 2)
    n_good = np.full(P, 100, dtype=np.int32)
    n_good[4] = 10
    info = np.zeros(P, dtype=np.int32)
    info[7] = -2
    init = (None, None, (R_rel, C_rel, None, None, n_good, None, None, None, None, info, None, None, None), None, None,
            None)
    verified = (None, pair_ij, None, None, None)
    e_ij, _, _ = pair_rotations(verified, init)
    usable = np.setdiff1d(np.arange(P), [4, 7])
    assert np.array_equal(e_ij, pair_ij[usable])
    inlier = np.ones(len(usable), dtype=bool)
    inlier[2] = False
    group = np.array([0, 0, 0, 0, 0, 5], dtype=np.int32)  # image 5 lost its inlier connection
    rot_out = (R, np.zeros(len(usable)), inlier, None, group, None, None, 0)
    ij, dirs, w, keep = pair_directions(verified, init, (np.arange(n), rot_out))
    want = np.zeros(P, dtype=bool)
    want[usable] = inlier & (pair_ij[usable] != 5).all(axis=1)
    assert np.array_equal(keep, want) and np.array_equal(ij, pair_ij[want]) and ij.dtype == np.int32
    assert np.array_equal(w, n_good[want]) and w.dtype == np.float64
    assert np.abs(dirs - unit(Cw[ij[:, 1]] - Cw[ij[:, 0]])).max() < 1e-14


# ------------------------------------------------------------------ the library without a device
def raw_call(N, ij, d, weight=None, mu=0.01, sigma=0.05, threshold=0.09, rounds=2, cg_tol=1e-12, cg_max_iters=50,
             path=0):
    """the C entry itself on sentinel-filled outputs: (return code, outputs untouched)"""
    import _sfmcore as core
    ij = np.ascontiguousarray(ij, dtype=np.int32).reshape(-1, 2)
    d = np.ascontiguousarray(d, dtype=np.float64)
    E, nr = len(ij), max(int(rounds), 1)
    outs = [np.full((N, 3), 7.0), np.full(E, 7.0), np.full(E, 7, np.uint8), np.full(E, 7.0), np.full(N, 7, np.int32),
            np.full(nr, 7, np.int32), np.full(nr, 7.0), np.full(1, 7, np.int32), np.full(1, 7, np.int32)]
    types = [core._d, core._d, core._u8, core._d, core._i32, core._i32, core._d, core._i32, core._i32]
    P = core._p
    rc = core._lib.sfm_average_positions(N, P(ij, core._i32), P(d), P(weight) if weight is not None else None, E, mu,
                                         sigma, threshold, rounds, cg_tol, cg_max_iters, path,
                                         *[P(o, t) for o, t in zip(outs, types)], core.DEVICE)
    return rc, all(np.all(o == 7) for o in outs)


def _edit(a, at, value):
    a = np.array(a, dtype=np.float64 if np.asarray(a).dtype.kind == "f" else None)
    a[at] = value
    return a


def violations():
    g = stored_graph("a")
    ij, d, w = g["ij"], g["dir"], np.ones(len(g["ij"]))
    big = stored_graph("d")
    return {
        "mu 0": dict(mu=0.0), "mu above 1": dict(mu=1.5), "mu NaN": dict(mu=np.nan),
        "sigma 0": dict(sigma=0.0), "sigma inf": dict(sigma=np.inf),
        "threshold 0": dict(threshold=0.0), "threshold pi": dict(threshold=np.pi), "threshold NaN": dict(threshold=np.nan),
        "rounds 0": dict(rounds=0), "rounds < 0": dict(rounds=-3),
        "cg_tol < 0": dict(cg_tol=-1e-9), "cg_tol NaN": dict(cg_tol=np.nan), "cg_max_iters 0": dict(cg_max_iters=0),
        "path 3": dict(path=3), "path -1": dict(path=-1),
        "zero direction": dict(d=_edit(d, 3, 0.0)), "NaN direction": dict(d=_edit(d, (5, 1), np.nan)),
        "inf direction": dict(d=_edit(d, (0, 2), np.inf)),
        "i == j": dict(ij=_edit(ij, (2, 0), ij[2, 1])), "image out of range": dict(ij=_edit(ij, (3, 1), g["N"])),
        "negative image": dict(ij=_edit(ij, (0, 0), -1)),
        "zero weight": dict(weight=_edit(w, 5, 0.0)), "NaN weight": dict(weight=_edit(w, 5, np.nan)),
        "path 1 past its bound": dict(N=big["N"], ij=big["ij"], d=big["dir"], path=1),
    }


def test_argument_violations_are_found_without_a_device():
    """SFM_ERR_ARG with nothing written, on a host without a GPU as on one with: the checks, the pruning and the
    path bound come before a device is looked for"""
    import _sfmcore as core
    g = stored_graph("a")
    for name, change in violations().items():
        args = dict(N=g["N"], ij=g["ij"], d=g["dir"])
        args.update(change)
        rc, untouched = raw_call(**args)
        assert rc == -1 and untouched, name
        assert core._lib.sfm_last_error().startswith(b"argument:"), name
    with pytest.raises(core.SfmCoreError):
        core.average_positions(g["N"], g["ij"], g["dir"], mu=0.0)
    with pytest.raises(ValueError):
        core.average_positions(g["N"], g["ij"], g["dir"][:-1])


def test_nothing_to_solve_needs_no_device():
    """N = 0, E = 0 and a graph that prunes away entirely: answered on the host, as the restatement answers"""
    import _sfmcore as core
    from sfm_multiview import average_positions
    path = np.array([[0, 1], [1, 2], [2, 3], [1, 2]], np.int32)  # a path with a doubled edge: all leaves in turn
    d = np.ones((4, 3))
    for N, ij, dd in ((0, np.zeros((0, 2), np.int32), np.zeros((0, 3))), (3, np.zeros((0, 2), np.int32), np.zeros((0, 3))),
                      (5, path, d)):
        out = core.average_positions(N, ij, dd, rounds=3)
        ref = restate(N, ij, dd, rounds=3)
        for k, n in enumerate(OUTPUTS):
            assert np.array_equal(out[k], ref[n]), n
        assert out[8] == 0 and out[0].shape == (N, 3) and out[4].dtype == np.int32 and out[5].dtype == np.int32
        solved, out2 = average_positions(ij, dd, N, rounds=3)
        assert len(solved) == 0 and out2[7] == 0


def test_the_header_and_the_binding_name_the_same_bound():
    import _sfmcore as core
    from conftest import REPO
    txt = open(os.path.join(REPO, "include", "sfmcore.h")).read()
    assert f"#define SFM_POSITIONS_PATH1_MAX_NODES {PATH1_MAX_NODES}\n" in txt
    assert core.POSITIONS_PATH1_MAX_NODES == PATH1_MAX_NODES
    assert "sfm_average_positions" in {n for n, _, _ in core.SIGNATURES} and hasattr(core._lib, "sfm_average_positions")
    assert stored_out("d")["n_solved"] > PATH1_MAX_NODES
