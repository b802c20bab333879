"""Generate tests/golden/multiview.npz: expected results of the multi-view
track triangulation (sfm_triangulate_tracks).

Runs only where make_golden.py runs: the two-view expectations come from
calling the reference's own linear_triangulation and nonlinear_triangulation
(imported from the place make_golden.py names); nothing of its source is
stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_multiview.py

The inputs are not stored: tests/test_multiview.py regenerates them from
sfm_synthetic.ba_problem's seeds (CASES, load_problem), cameras at their true
poses, 0.5 px noise.  Cases (key prefix):
  v2          257 two-view tracks over 6 cameras.  X_lin, X_nl: the
              reference's linear_triangulation on each camera pair's tracks
              and its nonlinear_triangulation from that.
  v3, v5, v8  257 tracks of 3 / 5 / 8 views over 6 / 7 / 8 cameras.  X_lin:
              numpy's SVD of the stacked 2n x 4 matrix; cost_lin: the sum of
              squared residuals there; X_min, cost_min: the converged minimum
              of the generalised loss, scipy least_squares(method='lm') with
              ftol = xtol = gtol = 1e-15 from X_lin, restarted until the cost
              no longer falls.
Asserted here, relied on by the tests:
  cond_eps    per track sigma_1 / (sigma_3 - sigma_4) of the stacked matrix
              times 2.2e-16 is at most 1e-10 (the largest is stored): rounding
              cannot move the singular vector by a tenth of the 1e-9 bound.
  margin      every |h3| is at least 1e-6 from the 1e-8 dehomogenisation
              threshold, and every depth at every stored point at least 1e-6
              of max(1, |X|_inf) from 0 and from +-1e-8 (the smallest such
              distance is stored): no branch and no front bit is within
              rounding of flipping, and no track is left out of a comparison.
"""
import os
import sys

import numpy as np
from scipy.optimize import least_squares

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import test_multiview as tm  # noqa: E402

K = tm.K


def depth_margin(c, Xs):
    """Smallest distance of a depth from 0 / +-1e-8 over the scene's scale"""
    m = np.inf
    for t in range(c["T"]):
        cams, _ = tm.track(c, t)
        for X in Xs:
            z = np.abs(tm.depths(c["P"], cams, X[t]))
            m = min(m, (z - 1e-8).min() / max(1.0, np.abs(X[t]).max()))
    return m


def two_view(ref, out):
    c = tm.load_problem("v2")
    cam = c["obs_cam"].reshape(-1, 2)
    xy = c["obs_xy"].reshape(-1, 2, 2)
    X_lin, X_nl = np.full((c["T"], 3), np.nan), np.full((c["T"], 3), np.nan)
    for a, b in sorted({tuple(p) for p in cam}):
        sel = np.where((cam[:, 0] == a) & (cam[:, 1] == b))[0]
        args = (K, c["C"][a], c["R"][a], c["C"][b], c["R"][b], xy[sel, 0], xy[sel, 1])
        X_lin[sel] = ref.t.linear_triangulation(*args)
        X_nl[sel] = ref.nt.nonlinear_triangulation(*args, X_lin[sel])
    assert np.isfinite(X_lin).all() and np.isfinite(X_nl).all()  # every track in a pair, none left out
    h3 = min(abs(tm.dlt_svd(c["P"], *tm.track(c, t))[1][3]) for t in range(c["T"]))
    margin = min(depth_margin(c, (X_lin, X_nl)), h3 - 1e-8)
    assert margin >= 1e-6, margin
    out.update(v2_X_lin=X_lin, v2_X_nl=X_nl, v2_margin=np.array(margin))
    print("v2", c["T"], f"margin {margin:.3g}")


def n_view(name, out):
    c = tm.load_problem(name)
    T = c["T"]
    X_lin, X_min = np.zeros((T, 3)), np.zeros((T, 3))
    cost_lin, cost_min = np.zeros(T), np.zeros(T)
    cond, h3 = 0.0, np.inf
    for t in range(T):
        cams, xy = tm.track(c, t)
        X_lin[t], h, s = tm.dlt_svd(c["P"], cams, xy)
        cond = max(cond, s[0] / (s[2] - s[3]) * 2.2e-16)
        h3 = min(h3, abs(h[3]))
        cost_lin[t] = tm.cost(c["P"], cams, xy, X_lin[t])
        x, best = X_lin[t], cost_lin[t]
        for _ in range(10):
            r = least_squares(lambda X: tm.residuals(c["P"], cams, xy, X), x, method="lm", ftol=1e-15, xtol=1e-15,
                              gtol=1e-15)
            cnew = tm.cost(c["P"], cams, xy, r.x)
            if not cnew < best:
                break
            x, best = r.x, cnew
        X_min[t], cost_min[t] = x, best
    assert cond <= 1e-10, cond
    margin = min(depth_margin(c, (X_lin, X_min)), h3 - 1e-8)
    assert margin >= 1e-6, margin
    assert np.all(cost_min <= cost_lin)
    out.update({f"{name}_X_lin": X_lin, f"{name}_X_min": X_min, f"{name}_cost_lin": cost_lin,
                f"{name}_cost_min": cost_min, f"{name}_cond_eps": np.array(cond), f"{name}_margin": np.array(margin)})
    print(name, T, f"cond*eps {cond:.3g} margin {margin:.3g} cost_lin/cost_min max "
          f"{(cost_lin / cost_min).max():.4g} |X_lin - X_min| max {np.abs(X_lin - X_min).max():.3g}")


def main():
    ref = mg._import_reference()
    assert os.path.dirname(os.path.abspath(ref.t.__file__)) == mg.REF
    out = {}
    two_view(ref, out)
    for name in tm.NVIEW:
        n_view(name, out)
    path = os.path.join(HERE, "multiview.npz")
    np.savez_compressed(path, **out)
    print("multiview.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
