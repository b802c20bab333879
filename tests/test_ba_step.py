"""One Levenberg-Marquardt step of the bundle adjustment from first principles,
on ragged problems.  CPU only: the generators, the reference and the pins of
the C oracle that tests/test_ba_step_gpu.py builds on.

The problems.  sfm_synthetic.ba_problem's scene (points in its box, cameras on
its yaw arc, its perturbed start and pixel noise) with an explicit track table
per case (CASES below): points without observations and with one, tracks over
every camera, cameras without observations, one camera that sees everything,
odd camera counts and the first camera counts at which the Schur sweep splits a
row.  In ragged7* and odd33_skew camera 1 is rolled 3.0 rad about its optical
axis and camera 2 has a rotation vector of exactly zero; the *_skew cases have
K[0, 1] = 1.7.

The reference carries no hand-derived Jacobian.  The residual of one
observation is written as a function of (dtheta, dt, dX) at zero,
    R = matrix_exp(hat(dtheta)) R0,  u = K (R (X + dX) + t + dt),
    r = obs - u[:2] / (u[2] + 1e-8),
and torch.func.vmap(jacrev(.)) in float64 gives its 2x6 and 2x3 blocks.  From
them g = J^T r, D = clamp(diag J^T J, 1e-6, 1e32) and the product
(J^T J + lambda D) delta are formed block by block (no dense J).

A solver's step delta is recovered from its output after one iteration:
dX = X1 - X0, dt = t1 - t0, dtheta = log(R(rotvec1) R0^T).  Its norm-wise
backward error is
    eta = |(J^T J + lambda D) delta + g|_2 / | |J^T J + lambda D| |delta| + |g| |_2;
the largest row-wise eta is reported for camera rows and point rows apart, and
rows without an observation must not move (dt, dX exactly zero; dtheta goes
through two rotation-vector conversions, so at most ZERO_ROT).

The oracle's eta is bounded by RATIO_BOUND * eps * (1 + max|x0| / max|delta|):
the second term is the cancellation in recovering delta by subtraction.
Measured here on orc_ba_lm (eta at lambda = 1e-4 / 1 / 1e4, the ratio eta over
that scale, and rho of the first step, accepted everywhere):

    case           eta 1e-4        1      1e4 | ratio             |  rho
    ragged7        1.6e-14    7e-16    3e-12 |  6.72  0.21  0.37 |  1.000  1.004  1.000
    ragged7_skew   1.8e-14  1.4e-15  3.2e-12 |  7.18  0.41  0.39 |  1.000  1.004  1.000
    one            1.1e-13  2.8e-15  2.5e-12 | 21.28  0.37  0.11 |  0.999  1.001  1.000
    two            1.4e-13  2.7e-15  1.3e-12 | 20.68  0.29  0.06 |  1.000  0.996  1.000
    odd33_skew     1.2e-15  1.2e-15  8.5e-12 |  0.61  0.27  0.84 |  1.000  0.998  1.000
    full12         8.2e-16  1.2e-15  4.5e-12 |  0.07  0.13  0.21 |  1.000  0.998  1.000
    hub            7.4e-16    1e-15  5.4e-12 |  0.39  0.42  0.65 |  1.000  1.000  1.000
    split288       4.4e-15  1.4e-15  5.2e-12 |  2.83  0.37  0.56 |  1.000  0.999  1.000
    split289       4.5e-15  1.4e-15  5.6e-12 |  6.93  0.39  0.61 |  0.999  1.000  1.000

cost0 matched 0.5 |r|^2 of the reference to 4e-15 relative, and the blocks
matched the central differences of oracle.ba_residuals to 9.4e-9 of a block's
largest entry.  The largest ratio is 21.3 (one and two at lambda = 1e-4, where
the undamped system is singular: 16 residuals for 30 parameters); RATIO_BOUND
is ten times it.

The rejected-step input (REJECTED): a ragged7-sized problem started 0.2 rad /
0.2 in pose and 0.3 in the points from the truth.  By the reference's own
dense solve its step at lambda = 1e-4 has rho = -0.59 and the step at 2e-4,
from the same linearisation, rho = 0.96; the oracle rejects the first and
accepts the second.  Sixteen such inputs turned up among 240 starts (pose
noise 0.05 - 0.3, point noise 0.05 / 0.3, lambda 1e-12 - 1e3); this one has
the widest margins.
"""
import functools

import numpy as np
import pytest
import torch

import oracle as O
import sfm_synthetic as syn

EPS = float(np.finfo(np.float64).eps)
LAMBDAS = (1e-4, 1.0, 1e4)
ZERO_ROT = 16 * EPS
# name: (n_cams, n_pts, skewed K, cameras 1 and 2 special, seed)
CASES = {
    "ragged7": (7, 60, False, True, 11),
    "ragged7_skew": (7, 60, True, True, 11),
    "one": (1, 8, False, False, 12),
    "two": (2, 9, False, False, 13),
    "odd33_skew": (33, 400, True, True, 14),
    "full12": (12, 40, False, False, 15),
    "hub": (6, 1500, False, False, 16),
    "split288": (288, 600, False, False, 17),
    "split289": (289, 600, False, False, 18),
}
RATIO_BOUND = 213.0  # ten times the largest measured eta / (eps (1 + max|x0| / max|delta|)), see the docstring
REJECTED = dict(seed=129, pose_noise=0.2, pt_noise=0.3, lam=1e-4)


# ------------------------------------------------------------------ rotations
def hat(w):
    w = np.asarray(w, dtype=np.float64)
    H = np.zeros(w.shape[:-1] + (3, 3))
    H[..., 0, 1], H[..., 0, 2] = -w[..., 2], w[..., 1]
    H[..., 1, 0], H[..., 1, 2] = w[..., 2], -w[..., 0]
    H[..., 2, 0], H[..., 2, 1] = -w[..., 1], w[..., 0]
    return H


def expm(w):
    """exp(hat(w)), (n, 3) -> (n, 3, 3), by the matrix exponential (no rotation-vector branch)"""
    return torch.linalg.matrix_exp(torch.from_numpy(hat(w))).numpy()


def logm(R):
    """the rotation vector of R, (n, 3, 3) -> (n, 3), for angles below pi; accurate at zero"""
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    s = np.linalg.norm(v, axis=-1)
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    th = np.arctan2(s, c)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(s < 1e-8, 1.0 + th * th / 6.0, th / s)
    return v * f[..., None]


# ------------------------------------------------------------------ problems
def _tracks(name, nc, n_pts, rng):
    """per point, the ascending cameras that observe it"""
    out = []
    for p in range(n_pts):
        if name.startswith("ragged7"):      # lengths 0..6 over cameras 0..5; camera 6 sees nothing
            L = p % 7
            if L == 6:
                cams = np.arange(6)
            elif L and p % 3 == 0:
                cams = np.concatenate([[0], rng.choice(np.arange(1, 6), L - 1, replace=False)])
            else:
                cams = rng.choice(np.arange(1, 6), L, replace=False)
        elif name == "one":
            cams = np.array([0])
        elif name == "two":                 # the second camera sees nothing
            cams = np.array([0])
        elif name == "odd33_skew":          # lengths 1..33
            cams = rng.choice(nc, 1 + p % 33, replace=False)
        elif name == "full12":
            cams = np.arange(nc)
        elif name == "hub":                 # camera 0 and one or two others
            cams = np.concatenate([[0], rng.choice(np.arange(1, nc), 1 + p % 2, replace=False)])
        else:                               # split288 / split289: lengths 2..6
            cams = rng.choice(nc, 2 + p % 5, replace=False)
        out.append(np.sort(cams).astype(np.int32))
    return out


def make_problem(name, nc, n_pts, skew, special, seed, pose_noise=0.01, pt_noise=0.05, noise=0.5):
    rng = np.random.default_rng(seed)
    K = syn.K_REF.copy()
    if skew:
        K[0, 1] = 1.7
    X = np.column_stack([rng.uniform(-2, 2, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(4, 8, n_pts)])
    yaw = np.linspace(-0.15, 0.15, nc) if nc > 1 else np.zeros(1)
    C = np.column_stack([3.0 * np.sin(yaw), rng.normal(0, 0.05, nc), rng.normal(0, 0.05, nc)])
    rv = np.column_stack([rng.normal(0, 0.01, nc), -yaw + rng.normal(0, 0.01, nc), rng.normal(0, 0.01, nc)])
    R = syn.rotvec_to_matrix(rv)
    if special:
        R[1] = expm(np.array([[0.0, 0.0, 3.0]]))[0] @ R[1]
        R[2] = np.eye(3)
    tr = _tracks(name, nc, n_pts, rng)
    cam_idx = np.concatenate(tr).astype(np.int32) if n_pts else np.zeros(0, np.int32)
    pt_idx = np.repeat(np.arange(n_pts, dtype=np.int32), [len(t) for t in tr])
    xc = np.einsum("nij,nj->ni", R[cam_idx], X[pt_idx] - C[cam_idx])
    u = xc @ K.T
    obs = u[:, :2] / u[:, 2:3] + rng.normal(0, noise, (len(cam_idx), 2))
    R0 = expm(rng.normal(0, pose_noise, (nc, 3))) @ R
    if special:
        R0[2] = np.eye(3)
    rv0 = logm(R0)
    C0 = C + rng.normal(0, pose_noise, C.shape)
    X0 = X + rng.normal(0, pt_noise, X.shape)
    R0 = syn.rotvec_to_matrix(rv0)          # the rotation the solvers start from
    cams0 = np.column_stack([rv0, np.einsum("nij,nj->ni", -R0, C0)])
    if special:
        assert not cams0[2, :3].any() and 2.0 < np.linalg.norm(cams0[1, :3]) < np.pi
    return dict(name=name, n_cams=nc, n_pts=n_pts, K=K, cams0=cams0, R0=R0, X0=np.ascontiguousarray(X0),
                cam_idx=cam_idx, pt_idx=pt_idx, obs=np.ascontiguousarray(obs))


@functools.lru_cache(maxsize=None)
def problem(name):
    nc, n_pts, skew, special, seed = CASES[name]
    return make_problem(name, nc, n_pts, skew, special, seed)


@functools.lru_cache(maxsize=None)
def rejected_problem():
    r = REJECTED
    return make_problem("ragged7", 7, 60, False, True, r["seed"], pose_noise=r["pose_noise"], pt_noise=r["pt_noise"])


def args(p):
    return p["cams0"], p["X0"], p["cam_idx"], p["pt_idx"], p["obs"], p["K"]


# ------------------------------------------------------------------ reference
def _hat_t(w):
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def _residual(dth, dt, dX, R0, t, X, ob, K):
    R = torch.linalg.matrix_exp(_hat_t(dth)) @ R0
    u = K @ (R @ (X + dX) + t + dt)
    return ob - u[:2] / (u[2] + 1e-8)


class Lin:
    """the linearisation of a problem at (cams, pts): the blocks of vmap(jacrev) and what follows from them"""

    def __init__(self, p, cams=None, pts=None):
        cams = p["cams0"] if cams is None else cams
        pts = p["X0"] if pts is None else pts
        ci, pi = p["cam_idx"].astype(np.int64), p["pt_idx"].astype(np.int64)
        self.ci, self.pi, self.nc, self.np = ci, pi, p["n_cams"], p["n_pts"]
        T = torch.from_numpy
        R = syn.rotvec_to_matrix(cams[:, :3])
        z = torch.zeros(3, dtype=torch.float64)
        a = (z, z, z, T(R[ci]), T(np.ascontiguousarray(cams[ci, 3:])), T(pts[pi]), T(p["obs"]), T(p["K"]))
        dims = (None, None, None, 0, 0, 0, 0, None)
        if len(ci):
            self.r = torch.func.vmap(_residual, in_dims=dims)(*a).numpy()
            Jth, Jt, Jx = torch.func.vmap(torch.func.jacrev(_residual, argnums=(0, 1, 2)), in_dims=dims)(*a)
            self.Jc, self.Jp = torch.cat([Jth, Jt], dim=2).numpy(), Jx.numpy()
        else:
            self.r, self.Jc, self.Jp = np.zeros((0, 2)), np.zeros((0, 2, 6)), np.zeros((0, 2, 3))
        self.cost = 0.5 * float((self.r * self.r).sum())
        self.U, self.V = np.zeros((self.nc, 6, 6)), np.zeros((self.np, 3, 3))
        np.add.at(self.U, ci, np.einsum("oai,oaj->oij", self.Jc, self.Jc))
        np.add.at(self.V, pi, np.einsum("oai,oaj->oij", self.Jp, self.Jp))
        self.W = np.einsum("oai,oaj->oij", self.Jc, self.Jp)
        self.gc, self.gp = np.zeros((self.nc, 6)), np.zeros((self.np, 3))
        np.add.at(self.gc, ci, np.einsum("oai,oa->oi", self.Jc, self.r))
        np.add.at(self.gp, pi, np.einsum("oai,oa->oi", self.Jp, self.r))
        self.Dc = np.clip(np.einsum("cii->ci", self.U), 1e-6, 1e32)
        self.Dp = np.clip(np.einsum("pii->pi", self.V), 1e-6, 1e32)
        self.cam_seen = np.bincount(ci, minlength=self.nc) > 0
        self.pt_seen = np.bincount(pi, minlength=self.np) > 0

    def product(self, lam, dc, dp, absolute=False):
        """(J^T J + lam D) (dc, dp), or |J^T J + lam D| (|dc|, |dp|): each (camera, point) pair is one W block"""
        f = np.abs if absolute else (lambda x: x)
        U, V, W, dc, dp = f(self.U), f(self.V), f(self.W), f(dc), f(dp)
        hc = np.einsum("cij,cj->ci", U, dc) + lam * self.Dc * dc
        hp = np.einsum("pij,pj->pi", V, dp) + lam * self.Dp * dp
        np.add.at(hc, self.ci, np.einsum("oij,oj->oi", W, dp[self.pi]))
        np.add.at(hp, self.pi, np.einsum("oij,oi->oj", W, dc[self.ci]))
        return hc, hp

    def model(self, lam, dc, dp):
        """the model decrease 0.5 delta^T (lam D delta - g)"""
        return 0.5 * float((dc * (lam * self.Dc * dc - self.gc)).sum() + (dp * (lam * self.Dp * dp - self.gp)).sum())

    def dense_step(self, lam):
        """the step by a dense solve (small problems only)"""
        n, m = 6 * self.nc, 3 * self.np
        H = np.zeros((n + m, n + m))
        for c in range(self.nc):
            H[6 * c:6 * c + 6, 6 * c:6 * c + 6] = self.U[c]
        for q in range(self.np):
            H[n + 3 * q:n + 3 * q + 3, n + 3 * q:n + 3 * q + 3] = self.V[q]
        for o, (c, q) in enumerate(zip(self.ci, self.pi)):
            H[6 * c:6 * c + 6, n + 3 * q:n + 3 * q + 3] = self.W[o]
            H[n + 3 * q:n + 3 * q + 3, 6 * c:6 * c + 6] = self.W[o].T
        H[np.diag_indices(n + m)] += lam * np.concatenate([self.Dc.ravel(), self.Dp.ravel()])
        d = np.linalg.solve(H, -np.concatenate([self.gc.ravel(), self.gp.ravel()]))
        return d[:n].reshape(-1, 6), d[n:].reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def lin0(name):
    return Lin(rejected_problem() if name == "rejected" else problem(name))


def step_of(p, cams1, pts1):
    """the step (dc, dp) that takes the problem's start to (cams1, pts1)"""
    dth = logm(syn.rotvec_to_matrix(cams1[:, :3]) @ np.transpose(p["R0"], (0, 2, 1)))
    return np.column_stack([dth, cams1[:, 3:] - p["cams0"][:, 3:]]), pts1 - p["X0"]


def moved(p, dc, dp):
    """the step applied to the problem's start, in the solvers' parameters"""
    R = expm(dc[:, :3]) @ p["R0"]
    return np.column_stack([logm(R), p["cams0"][:, 3:] + dc[:, 3:]]), p["X0"] + dp


def measures(L, lam, dc, dp):
    """eta, the largest row-wise eta of the camera rows and of the point rows, whether the rows without an
    observation stayed, and the scale eps (1 + max|x0| / max|delta|) is the caller's"""
    hc, hp = L.product(lam, dc, dp)
    ac, ap = L.product(lam, dc, dp, absolute=True)
    rc, rp = hc + L.gc, hp + L.gp
    sc, sp = ac + np.abs(L.gc), ap + np.abs(L.gp)
    eta = np.sqrt((rc * rc).sum() + (rp * rp).sum()) / np.sqrt((sc * sc).sum() + (sp * sp).sum())

    def rows(r, s, seen):
        r, s = r[seen], s[seen]
        return float(np.max(r[s > 0] / s[s > 0], initial=0.0)) if r.size else 0.0
    stay = (not dc[~L.cam_seen, 3:].any() and not dp[~L.pt_seen].any() and
            np.abs(dc[~L.cam_seen, :3]).max(initial=0.0) <= ZERO_ROT)
    return dict(eta=float(eta), eta_cam=rows(np.abs(rc), sc, L.cam_seen), eta_pt=rows(np.abs(rp), sp, L.pt_seen),
                stay=bool(stay))


def cancellation(p, dc, dp):
    """eps max|x0| / max|delta|: what recovering delta by subtraction loses"""
    x0 = max(np.abs(p["cams0"]).max(), np.abs(p["X0"]).max(initial=0.0))
    return EPS * x0 / max(np.abs(dc).max(), np.abs(dp).max(initial=0.0))


def rho_of(p, L, lam, dc, dp, cost1=None):
    """the gain ratio of the step, with the reference's residual at the moved parameters unless cost1 is given"""
    if cost1 is None:
        cost1 = Lin(p, *moved(p, dc, dp)).cost
    return (L.cost - cost1) / L.model(lam, dc, dp)


@functools.lru_cache(maxsize=None)
def oracle_step(name, lam, iterations=1):
    """orc_ba_lm's output after `iterations` from the problem's start, its step and the step's measures"""
    p = rejected_problem() if name == "rejected" else problem(name)
    cams1, pts1, rep = O.ba_lm(*args(p), max_iterations=iterations, ftol=0.0, gtol=0.0, xtol=0.0, initial_lambda=lam)
    dc, dp = step_of(p, cams1, pts1)
    return dict(cams=cams1, pts=pts1, rep=rep, dc=dc, dp=dp)


def oracle_eta(name, lam, lam_step=None, iterations=1):
    o = oracle_step(name, lam, iterations)
    p = rejected_problem() if name == "rejected" else problem(name)
    m = measures(lin0(name), lam if lam_step is None else lam_step, o["dc"], o["dp"])
    m["scale"] = EPS + cancellation(p, o["dc"], o["dp"])
    return m


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", list(CASES))
def test_the_cases_are_what_they_claim(name):
    p, L = problem(name), lin0(name)
    nc, n_pts = CASES[name][:2]
    n = np.bincount(p["pt_idx"], minlength=n_pts)
    assert np.all(np.diff(p["pt_idx"]) >= 0) and len(set(zip(p["cam_idx"], p["pt_idx"]))) == len(p["cam_idx"])
    want = {"ragged7": (0, 6), "ragged7_skew": (0, 6), "one": (1, 1), "two": (1, 1), "odd33_skew": (1, 33),
            "full12": (12, 12), "hub": (2, 3), "split288": (2, 6), "split289": (2, 6)}[name]
    assert (n.min(), n.max()) == want
    if name.startswith("ragged7"):
        assert not L.cam_seen[6] and L.cam_seen[:6].all() and 18 <= (p["cam_idx"] == 0).sum() <= 24
    if name == "two":
        assert not L.cam_seen[1]
    if name == "hub":
        assert (p["cam_idx"] == 0).sum() == 1500 > 512
    if name.startswith("split"):
        assert nc + 1 > 288 and 6 * nc == {"split288": 1728, "split289": 1734}[name]
    assert (p["K"][0, 1] == 1.7) == name.endswith("_skew")


@pytest.mark.parametrize("name", list(CASES))
def test_blocks_are_central_differences_of_the_oracles_residual(name):
    """every observation's 2x9 block against (r(+h) - r(-h)) / 2h of oracle.ba_residuals along each of the nine
    directions, all cameras (or points) moved at once: each observation has one camera and one point.  h = 1e-4:
    truncation h^2 f''' / 6 f' ~ 1e-8, rounding eps |u| / h ~ 1e-9 of a block's largest entry."""
    p, L = problem(name), lin0(name)
    h = 1e-4
    r0 = O.ba_residuals(*args(p)).reshape(-1, 2)
    assert np.abs(r0 - L.r).max() <= 1e-10
    fd = np.zeros((len(p["cam_idx"]), 2, 9))
    for k in range(9):
        r = []
        for s in (h, -h):
            dc, dp = np.zeros((p["n_cams"], 6)), np.zeros((p["n_pts"], 3))
            if k < 6:
                dc[:, k] = s
            else:
                dp[:, k - 6] = s
            cams, pts = moved(p, dc, dp)
            r.append(O.ba_residuals(cams, pts, p["cam_idx"], p["pt_idx"], p["obs"], p["K"]).reshape(-1, 2))
        fd[:, :, k] = (r[0] - r[1]) / (2 * h)
    J = np.concatenate([L.Jc, L.Jp], axis=2)
    err = np.abs(fd - J).max(axis=(1, 2)) / np.abs(J).max(axis=(1, 2))
    print(f"{name}: blocks against central differences <= {err.max():.3g} of a block's largest entry")
    assert err.max() <= 1e-6


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_step_is_accepted_and_backward_stable(name, lam):
    p, L = problem(name), lin0(name)
    o = oracle_step(name, lam)
    m = oracle_eta(name, lam)
    rho = rho_of(p, L, lam, o["dc"], o["dp"], o["rep"]["cost"])
    print(f"{name} lambda {lam:g}: eta {m['eta']:.3g} (camera rows {m['eta_cam']:.3g}, point rows {m['eta_pt']:.3g}), "
          f"ratio {m['eta'] / m['scale']:.3g}, rho {rho:.4f}")
    assert o["rep"]["accepted"] == 1 and o["rep"]["iterations"] == 1
    assert abs(o["rep"]["cost0"] - L.cost) <= 1e-12 * L.cost
    assert m["stay"]
    assert m["eta"] <= RATIO_BOUND * m["scale"]


def test_rejected_step_input():
    """the committed input: the oracle rejects the step at lam and accepts the one at 2 lam from the same
    linearisation; the reference's own gain ratios say so with a margin"""
    p, L, lam = rejected_problem(), lin0("rejected"), REJECTED["lam"]
    rho = [rho_of(p, L, l, *L.dense_step(l)) for l in (lam, 2 * lam)]
    print(f"rejected input: rho {rho[0]:.4f} at lambda {lam:g}, {rho[1]:.4f} at {2 * lam:g}")
    assert rho[0] < 1e-3 - 0.02 and rho[1] > 1e-3 + 0.02
    o1, o2 = oracle_step("rejected", lam, 1), oracle_step("rejected", lam, 2)
    assert (o1["rep"]["iterations"], o1["rep"]["accepted"]) == (1, 0)
    assert np.array_equal(o1["pts"], p["X0"]) and np.array_equal(o1["cams"][:, 3:], p["cams0"][:, 3:])
    assert (o2["rep"]["iterations"], o2["rep"]["accepted"]) == (2, 1)
    m = oracle_eta("rejected", lam, lam_step=2 * lam, iterations=2)
    assert m["stay"] and m["eta"] <= RATIO_BOUND * m["scale"]
