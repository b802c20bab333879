"""Global rotation averaging (sfm_average_rotations): the plain-numpy
restatement of its three stages, the synthetic view graphs, and the CPU tests
that pin the algorithm.  No GPU: the device call is compared with `restate` in
tests/test_rotation_averaging_gpu.py.

The restatement follows include/sfmcore.h definition by definition: the CSR
order of a node's entries, the 64-bit priority, the trace test with its nine
products added left to right, the refit's sums in entry order.  Every
comparison of a trace sum with tau = 1 + 2 cos(threshold) is recorded, and the
fixture graphs are chosen so that none lies within 1e-9 of tau (`margin`): no
decision can then turn on the last bits of the device's arithmetic.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

MARGIN = 1e-9
U64 = np.uint64


# ------------------------------------------------------------------ rotations
def rotvec_to_matrix(w):
    """Rodrigues, (n, 3) -> (n, 3, 3)"""
    w = np.asarray(w, dtype=np.float64).reshape(-1, 3)
    th = np.linalg.norm(w, axis=1)
    small = th < 1e-12
    k = w / np.where(small, 1.0, th)[:, None]
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    s, c = np.sin(th)[:, None, None], np.cos(th)[:, None, None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def random_rotations(rng, n):
    """uniform over SO(3): unit quaternions"""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a, b, c, d = q.T
    return np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], -1),
                     np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], -1),
                     np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], -1)], 1)


def angle_between(A, B):
    """the angle of A B^T, accurate near 0"""
    M = A @ np.swapaxes(B, -1, -2)
    v = 0.5 * np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], -1)
    return np.arctan2(np.linalg.norm(v, axis=-1), 0.5 * (np.trace(M, axis1=-2, axis2=-1) - 1))


# ------------------------------------------------------------------ the graphs
def measure(R_true, ij, noise_deg, wrong, rng):
    """(R_rel, clean) for the edges ij: R_rel = noise R_j R_i^T, a `wrong` edge a uniform random rotation.  The
    noise is a rotation vector of independent normal components with an RMS angle of noise_deg."""
    ij = np.asarray(ij, dtype=np.int32).reshape(-1, 2)
    E = len(ij)
    rel = R_true[ij[:, 1]] @ np.swapaxes(R_true[ij[:, 0]], 1, 2)
    if noise_deg > 0:
        rel = rotvec_to_matrix(rng.normal(0, np.deg2rad(noise_deg) / np.sqrt(3), (E, 3))) @ rel
    wrong = np.asarray(wrong, dtype=bool)
    rel[wrong] = random_rotations(rng, int(wrong.sum()))
    return np.ascontiguousarray(rel), ~wrong


def random_graph(N, density, noise_deg, wrong_frac, seed):
    """N cameras, every pair an edge with probability `density` in a random orientation, a share wrong_frac of
    the edges wrong.  Returns (ij, R_rel, R_true, clean)."""
    rng = np.random.default_rng(seed)
    R_true = random_rotations(rng, N)
    i, j = np.triu_indices(N, 1)
    keep = rng.random(len(i)) < density
    i, j = i[keep], j[keep]
    flip = rng.random(len(i)) < 0.5
    ij = np.column_stack([np.where(flip, j, i), np.where(flip, i, j)]).astype(np.int32)
    wrong = np.zeros(len(ij), dtype=bool)
    wrong[rng.choice(len(ij), int(round(wrong_frac * len(ij))), replace=False)] = True
    R_rel, clean = measure(R_true, ij, noise_deg, wrong, rng)
    return ij, R_rel, R_true, clean


# ------------------------------------------------------------------ the restatement
def priority(seed, e):
    """the 64-bit mix of include/sfmcore.h, modulo 2^64"""
    e = np.atleast_1d(np.asarray(e)).astype(U64)
    z = np.full(e.shape, int(seed) & (2 ** 64 - 1), dtype=U64) + (e + U64(1)) * U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def adjacency(N, ij):
    """CSR over the nodes: (adj_start, ent_edge, ent_nbr, ent_rev, ent_node, ent_pos), entries by ascending edge"""
    ij = np.asarray(ij, dtype=np.int64).reshape(-1, 2)
    E = len(ij)
    node = np.concatenate([ij[:, 0], ij[:, 1]])
    nbr = np.concatenate([ij[:, 1], ij[:, 0]])
    edge = np.concatenate([np.arange(E), np.arange(E)])
    rev = np.concatenate([np.zeros(E, bool), np.ones(E, bool)])
    o = np.lexsort((edge, node))
    node, nbr, edge, rev = node[o], nbr[o], edge[o], rev[o]
    adj_start = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=N))]).astype(np.int64)
    pos = np.arange(2 * E) - adj_start[node]
    return adj_start, edge, nbr, rev, node, pos


def components(N, ij):
    """label of every node: the lowest node of its connected component"""
    label = np.arange(N)
    ij = np.asarray(ij, dtype=np.int64).reshape(-1, 2)
    while len(ij):
        m = np.minimum(label[ij[:, 0]], label[ij[:, 1]])
        new = label.copy()
        np.minimum.at(new, ij[:, 0], m)
        np.minimum.at(new, ij[:, 1], m)
        if np.array_equal(new, label):
            break
        label = new
    return label


def find_roots(N, ij, adj_start):
    """is_root (N,): per component the node of highest degree, the lowest index on ties"""
    label = components(N, ij)
    deg = np.diff(adj_start)
    is_root = np.zeros(N, dtype=bool)
    for c in np.unique(label):
        members = np.flatnonzero(label == c)
        is_root[members[np.argmax(deg[members])]] = True  # argmax: the first of equals
    return is_root


def product(A, B):
    """(A B)[r][c] = (A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c], batched"""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) \
        + A[..., :, 2, None] * B[..., None, 2, :]


def predict(R_rel, edge, nbr, rev, R):
    """the predictions of the entries: R_rel R_nbr (rev) or R_rel^T R_nbr (fwd)"""
    A = R_rel[edge]
    A = np.where(rev[:, None, None], A, np.swapaxes(A, 1, 2))
    return product(A, R[nbr])


def trace_sum(P, Q):
    """the nine products of tr(P Q^T), added left to right"""
    p = P.reshape(P.shape[:-2] + (9,))
    q = Q.reshape(Q.shape[:-2] + (9,))
    t = p[..., 0] * q[..., 0]
    for k in range(1, 9):
        t = t + p[..., k] * q[..., k]
    return t


def axis_part(P, R):
    """v and s of M = P R^T"""
    M = product(P, np.swapaxes(R, -1, -2))
    v = np.stack([(M[..., 2, 1] - M[..., 1, 2]) / 2.0, (M[..., 0, 2] - M[..., 2, 0]) / 2.0,
                  (M[..., 1, 0] - M[..., 0, 1]) / 2.0], -1)
    return v, np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


class Margin:
    def __init__(self, tau):
        self.tau, self.least = tau, np.inf

    def test(self, t):
        if t.size:
            self.least = min(self.least, float(np.abs(t - self.tau).min()))
        return t >= self.tau


def restate(n_images, pair_ij, R_rel, weight=None, seed=0, threshold=np.deg2rad(5), consensus_sweeps=3,
            max_sweeps=200, tol=1e-9):
    """sfm_average_rotations in numpy.  Returns a dict of its outputs and `margin`, the least |t - tau| over every
    trace test made."""
    N = int(n_images)
    ij = np.asarray(pair_ij, dtype=np.int32).reshape(-1, 2)
    E = len(ij)
    R_rel = np.asarray(R_rel, dtype=np.float64).reshape(E, 3, 3)
    w_edge = np.ones(E) if weight is None else np.asarray(weight, dtype=np.float64)
    tau = 1.0 + 2.0 * np.cos(threshold)
    mg = Margin(tau)
    R = np.tile(np.eye(3), (N, 1, 1))
    if N == 0 or E == 0:
        return dict(R=R, edge_angle=np.zeros(E), edge_inlier=np.zeros(E, bool), n_inlier_edges=np.zeros(N, np.int32),
                    group=np.arange(N, dtype=np.int32), info=np.full(N, -1, np.int32), level=np.zeros(N, np.int32),
                    sweeps=0, margin=np.inf)
    adj_start, edge, nbr, rev, node, pos = adjacency(N, ij)
    deg = np.diff(adj_start)
    is_root = find_roots(N, ij, adj_start)
    # stage 1
    level = np.where(is_root, 0, -1).astype(np.int32)
    prio = priority(seed, edge)
    for l in range(N - 1):
        cand = np.flatnonzero((level[node] < 0) & (level[nbr] == l))
        if not len(cand):
            break
        o = cand[np.lexsort((edge[cand], prio[cand], node[cand]))]
        first = o[np.concatenate([[True], np.diff(node[o]) != 0])]
        R[node[first]] = predict(R_rel, edge[first], nbr[first], rev[first], R)
        level[node[first]] = l + 1
    # stage 2
    moving = np.flatnonzero(~is_root)
    for _ in range(consensus_sweeps):
        P = predict(R_rel, edge, nbr, rev, R)
        Rn = R.copy()
        for n in moving:
            Pn = P[adj_start[n]:adj_start[n + 1]]
            support = mg.test(trace_sum(Pn[:, None], Pn[None, :])).sum(axis=1)
            Rn[n] = Pn[np.argmax(support)]  # the lowest a of the greatest support
        R = Rn
    # stage 3
    by_pos = [np.flatnonzero((pos == k) & ~is_root[node]) for k in range(int(deg[moving].max()) if len(moving) else 0)]
    sweeps = 0
    for _ in range(max_sweeps):
        P = predict(R_rel, edge, nbr, rev, R)
        t = trace_sum(P, R[node])
        ok = np.zeros(2 * E, dtype=bool)
        live = ~is_root[node]
        ok[live] = mg.test(t[live])
        v, s = axis_part(P, R[node])
        theta = np.arctan2(s, (t - 1.0) / 2.0)
        f = np.where(s > 0.0, theta / np.where(s > 0.0, s, 1.0), 1.0)
        term = w_edge[edge][:, None] * (v * f[:, None])
        num, den = np.zeros((N, 3)), np.zeros(N)
        for idx in by_pos:  # a node's entries in their order; one entry per node and position
            idx = idx[ok[idx]]
            num[node[idx]] = num[node[idx]] + term[idx]
            den[node[idx]] = den[node[idx]] + w_edge[edge[idx]]
        has = den > 0.0
        om = np.zeros((N, 3))
        om[has] = num[has] / den[has][:, None]
        th2 = (om[:, 0] * om[:, 0] + om[:, 1] * om[:, 1]) + om[:, 2] * om[:, 2]
        th = np.sqrt(th2)
        series = th < 1e-4
        safe = np.where(series, 1.0, th)
        sh = np.sin(safe / 2.0)
        A = np.where(series, 1.0 - th2 / 6.0, np.sin(safe) / safe)
        B = np.where(series, 0.5 - th2 / 24.0, (2.0 * sh * sh) / np.where(series, 1.0, th2))
        Ex = B[:, None, None] * (om[:, :, None] * om[:, None, :])
        for k in range(3):
            Ex[:, k, k] = Ex[:, k, k] + (1.0 - B * th2)
        Ex[:, 0, 1] = Ex[:, 0, 1] - A * om[:, 2]
        Ex[:, 0, 2] = Ex[:, 0, 2] + A * om[:, 1]
        Ex[:, 1, 0] = Ex[:, 1, 0] + A * om[:, 2]
        Ex[:, 1, 2] = Ex[:, 1, 2] - A * om[:, 0]
        Ex[:, 2, 0] = Ex[:, 2, 0] - A * om[:, 1]
        Ex[:, 2, 1] = Ex[:, 2, 1] + A * om[:, 0]
        Rn = R.copy()
        Rn[has] = product(Ex[has], R[has])
        R = Rn
        sweeps += 1
        if tol > 0.0 and th.max() <= tol:
            break
    # the edges on the final rotations
    P = product(R_rel, R[ij[:, 0]])
    Rj = R[ij[:, 1]]
    t = trace_sum(P, Rj)
    inlier = mg.test(t)
    _, s = axis_part(P, Rj)
    angle = np.arctan2(s, (t - 1.0) / 2.0)
    n_inl = (np.bincount(ij[inlier, 0], minlength=N) + np.bincount(ij[inlier, 1], minlength=N)).astype(np.int32)
    group = components(N, ij[inlier]).astype(np.int32)
    info = np.where(is_root & (deg > 0), 1, np.where(n_inl > 0, 0, -1)).astype(np.int32)
    return dict(R=R, edge_angle=angle, edge_inlier=inlier, n_inlier_edges=n_inl, group=group, info=info, level=level,
                sweeps=sweeps, margin=mg.least)


OUTPUTS = ("R", "edge_angle", "edge_inlier", "n_inlier_edges", "group", "info", "level", "sweeps")
INTEGER_OUTPUTS = ("edge_inlier", "n_inlier_edges", "group", "info", "level", "sweeps")


def to_root_gauge(R_true, N, ij):
    """the truth with every component's root at I: R_true[n] R_true[root of n]^T"""
    ij = np.asarray(ij, dtype=np.int64).reshape(-1, 2)
    adj_start = adjacency(N, ij)[0]
    is_root = find_roots(N, ij, adj_start)
    label = components(N, ij)
    root_of = np.zeros(N, dtype=np.int64)
    root_of[label[is_root]] = np.flatnonzero(is_root)
    return R_true @ np.swapaxes(R_true[root_of[label]], 1, 2)


# ------------------------------------------------------------------ the fixture graphs
# name -> (N, density, seed, weighted); 1 degree of noise and 30 % wrong edges, what the device tests run.
# "dense" is a complete graph of 10 nodes, and small for a reason.  The refit is a Jacobi iteration with the root
# held at I: a rotation common to all other nodes is pulled back only through the entries that point at the root,
# about one in N - 1 of them, so each sweep removes about 1 / (N - 1) of it.  It starts near the noise over sqrt(N)
# (5e-3 rad) and the sweeps stop when the update, 1 / (N - 1) of what is left, is below tol = 1e-9: about
# (N - 1) ln(5e-3 / ((N - 1) 1e-9)) sweeps, 120 at N = 10 and 640 at N = 60.  So the default max_sweeps = 200
# reaches tol on graphs of about a dozen nodes; on the larger fixtures the refit ends at max_sweeps, with the same
# inlier mask and rotations that still move by 1e-4 rad a sweep (DESIGN.md records this).
FIXTURE_GRAPHS = {"dense": (10, 1.0, 11, False), "medium": (60, 0.5, 11, False), "sparse": (120, 0.15, 12, False),
                  "weighted": (80, 0.25, 13, True)}
FIXTURE_ARGS = dict(seed=7, threshold=np.deg2rad(5), consensus_sweeps=3, max_sweeps=30, tol=0.0)
# every setting the device tests run a fixture graph at: (consensus_sweeps, max_sweeps, tol)
FIXTURE_RUNS = ((0, 30, 0.0), (1, 30, 0.0), (3, 30, 0.0), (3, 0, 0.0), (3, 200, 1e-9))


def fixture_graph(name):
    N, density, seed, weighted = FIXTURE_GRAPHS[name]
    ij, R_rel, R_true, clean = random_graph(N, density, 1.0, 0.3, seed)
    weight = np.random.default_rng(seed + 100).integers(30, 400, len(ij)).astype(np.float64) if weighted else None
    return dict(N=N, ij=ij, R_rel=R_rel, weight=weight, R_true=R_true, clean=clean)


_fixture = {}


def fixture():
    if not _fixture:
        _fixture.update(np.load(os.path.join(GOLDEN, "rotation_averaging.npz")))
    return _fixture


def stored_graph(name):
    fx = fixture()
    weight = fx[name + "_weight"] if name + "_weight" in fx else None
    return dict(N=int(fx[name + "_N"]), ij=fx[name + "_ij"], R_rel=fx[name + "_R_rel"], weight=weight,
                R_true=fx[name + "_R_true"], clean=fx[name + "_clean"])


_runs = {}


def stored_run(name, consensus_sweeps, max_sweeps, tol):
    """the restatement on a stored graph at one of FIXTURE_RUNS, computed once and shared"""
    key = (name, consensus_sweeps, max_sweeps, tol)
    if key not in _runs:
        g = stored_graph(name)
        _runs[key] = restate(g["N"], g["ij"], g["R_rel"], g["weight"], seed=FIXTURE_ARGS["seed"],
                             threshold=FIXTURE_ARGS["threshold"], consensus_sweeps=consensus_sweeps,
                             max_sweeps=max_sweeps, tol=tol)
    return _runs[key]


# ------------------------------------------------------------------ tests
def test_priority_is_the_documented_mix():
    """two values worked by hand with Python integers"""
    def mix(seed, e):
        m = 2 ** 64 - 1
        z = (seed + (e + 1) * 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)
    for seed in (0, 7, 2 ** 64 - 1):
        got = priority(seed, np.arange(5))
        assert got.dtype == np.uint64 and [int(x) for x in got] == [mix(seed, e) for e in range(5)]


@pytest.mark.parametrize("name", sorted(FIXTURE_GRAPHS))
def test_generator_reproduces_the_stored_graphs(name):
    """the stored inputs are the generator's (integers exactly; the rotations to rounding, since sin and cos
    may differ in the last bit between numpy builds)"""
    g, s = fixture_graph(name), stored_graph(name)
    assert g["N"] == s["N"] and np.array_equal(g["ij"], s["ij"]) and np.array_equal(g["clean"], s["clean"])
    assert np.abs(g["R_rel"] - s["R_rel"]).max() < 1e-14 and np.abs(g["R_true"] - s["R_true"]).max() < 1e-14
    assert (g["weight"] is None) == (s["weight"] is None)
    if g["weight"] is not None:
        assert np.array_equal(g["weight"], s["weight"])


@pytest.mark.parametrize("name", sorted(FIXTURE_GRAPHS))
def test_restatement_against_the_fixture(name):
    """Integer outputs exactly; R and edge_angle within 1e-12: numpy's sin, cos and arctan2 may differ by an ulp
    (1e-16) between builds and 30 sweeps compound that, three orders below the device bound of 1e-9."""
    fx = fixture()
    out = stored_run(name, FIXTURE_ARGS["consensus_sweeps"], FIXTURE_ARGS["max_sweeps"], FIXTURE_ARGS["tol"])
    for n in INTEGER_OUTPUTS:
        assert np.array_equal(out[n], fx[f"{name}_out_{n}"]), n
    assert np.abs(out["R"] - fx[name + "_out_R"]).max() < 1e-12
    assert np.abs(out["edge_angle"] - fx[name + "_out_edge_angle"]).max() < 1e-12


@pytest.mark.parametrize("name", sorted(FIXTURE_GRAPHS))
def test_no_fixture_decision_is_within_the_margin(name):
    """every trace test of every run the device tests make on the stored graphs keeps 1e-9 from tau"""
    for cs, ms, tol in FIXTURE_RUNS:
        assert stored_run(name, cs, ms, tol)["margin"] > MARGIN, (cs, ms, tol)


@pytest.mark.parametrize("N,density,seed", [(60, 0.5, 21), (120, 0.15, 22), (200, 0.2, 23)])
def test_exact_graphs_are_recovered(N, density, seed):
    """no noise, 30 % wrong edges: exact data is an exact fixed point, so R is the truth in the root's gauge to
    1e-9 rad (the project's fp64 parity bound) and the inliers are the clean edges"""
    ij, R_rel, R_true, clean = random_graph(N, density, 0.0, 0.3, seed)
    out = restate(N, ij, R_rel, seed=seed)
    assert angle_between(out["R"], to_root_gauge(R_true, N, ij)).max() < 1e-9
    assert np.array_equal(out["edge_inlier"], clean)
    assert out["sweeps"] == 1 and np.all(out["group"] == 0) and (out["info"] == 1).sum() == 1


@pytest.mark.parametrize("name", sorted(FIXTURE_GRAPHS))
def test_noisy_graphs_keep_exactly_the_clean_edges(name):
    """1 degree of noise, 30 % wrong edges, the defaults: the inlier mask is the clean-edge mask, and every node
    lies within 2 degrees of the truth"""
    g = stored_graph(name)
    out = stored_run(name, 3, 200, 1e-9)
    assert np.array_equal(out["edge_inlier"], g["clean"])
    assert np.rad2deg(angle_between(out["R"], to_root_gauge(g["R_true"], g["N"], g["ij"])).max()) < 2.0


def test_the_refit_reaches_tol_on_the_dense_fixture():
    """the default tol and max_sweeps on the 10-node complete graph: see FIXTURE_GRAPHS for the sweep count"""
    assert 1 <= stored_run("dense", 3, 200, 1e-9)["sweeps"] < 200


def test_the_tree_alone_is_not_enough():
    """why the consensus sweeps exist: with none, the tree leaves nodes wrong that the sweeps repair"""
    g = stored_graph("medium")
    truth = to_root_gauge(g["R_true"], g["N"], g["ij"])
    tree = restate(g["N"], g["ij"], g["R_rel"], seed=7, consensus_sweeps=0, max_sweeps=0)
    assert (np.rad2deg(angle_between(tree["R"], truth)) > 5).sum() >= g["N"] // 10
    assert np.rad2deg(angle_between(stored_run("medium", 3, 200, 1e-9)["R"], truth)).max() < 2.0


def test_empty_graphs_need_no_device():
    """N = 0, and E = 0 with N = 3: the library answers on the host, as the restatement does"""
    import _sfmcore
    for N in (0, 3):
        out = _sfmcore.average_rotations(N, np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)))
        ref = restate(N, np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)))
        for k, n in enumerate(OUTPUTS):
            assert np.array_equal(out[k], ref[n]), n
        assert out[0].shape == (N, 3, 3) and out[4].dtype == np.int32


def test_pair_rotations_keeps_the_usable_pairs_in_order():
    from sfm_multiview import pair_rotations
    rng = np.random.default_rng(3)
    P = 12
    pair_ij = np.column_stack([np.arange(P), np.arange(P) + 1]).astype(np.int32)
    R = random_rotations(rng, P)
    n_good = np.array([50, 10, 30, 29, 200, 80, 31, 0, 45, 45, 30, 90], dtype=np.int32)
    info = np.array([0, 0, 0, 0, -1, 0, -2, 0, 0, 0, 0, 0], dtype=np.int32)
    init_out = (R, None, None, None, n_good, None, None, None, None, info, None, None, None)
    verified = (None, pair_ij, None, None, None)
    init = (None, None, init_out, None, None, None)
    ij, R_rel, w = pair_rotations(verified, init)
    keep = np.array([0, 2, 5, 8, 9, 10, 11])
    assert ij.dtype == np.int32 and np.array_equal(ij, pair_ij[keep]) and np.array_equal(R_rel, R[keep])
    assert w.dtype == np.float64 and np.array_equal(w, n_good[keep])
    assert len(pair_rotations(verified, init, min_points=81)[0]) == 1
