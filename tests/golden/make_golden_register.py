"""Generate tests/golden/register_views.npz: expected results of the batched
view registration (sfm_register_views).  numpy and scipy only: the reference
has no counterpart.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_register.py

The inputs are not stored: tests/test_register_views.py regenerates them from
seeds (load_scene, sample_table).  restate_view below is the whole rule in
numpy: per 6-point sample the SVD null vector of the 12 x 12 system and its
pose, the inlier rule, the winner (most inliers, then the earliest), and the
rounds of refit (scipy least_squares on the six pose parameters over the
current inliers), re-score and not-worse test.
Stored: threshold, n_v, truth (the untouched observations); per view of 63
correspondences and more (zeros elsewhere) C_min, R_min, cost_min -- the
converged minimum of the squared reprojection error over the true inliers
(scipy lm, tolerances 1e-15, restarted until the cost stops falling) -- and per
H in 64, 65, 256 the restatement's final mask and the distance of its nearest
final error from the threshold.
Asserted here for every such view and H, relied on by the tests: the final mask
is the truth, and every final error is at least 1 px from the threshold.
"""
import os
import sys

import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_register_views as rv  # noqa: E402

THRESHOLD = 4.0


def residuals(w, R0, C0, X, xy):
    """left-multiplied rotation increment w[:3], additive centre w[3:]"""
    R = Rotation.from_rotvec(w[:3]).as_matrix() @ R0
    h = (rv.K @ (R @ (X - (C0 + w[3:])).T)).T
    return (xy - h[:, :2] / h[:, 2:3]).reshape(-1)


def refit(C, R, X, xy, **kw):
    r = least_squares(residuals, np.zeros(6), args=(R, C, X, xy), method="lm", **kw)
    return C + r.x[3:], Rotation.from_rotvec(r.x[:3]).as_matrix() @ R


def score(C, R, X, xy, thr):
    P = rv.projection(C, R)
    m = rv.inlier_mask(P, X, xy, thr)
    return m, float(rv.errors2(P, X, xy)[0][m].sum())


def restate_view(X, xy, samples, thr, min_inliers=6, rounds=3):
    best = None
    for h, s in enumerate(samples):
        p = np.linalg.svd(rv.dlt_rows(X[s], xy[s]))[2][-1]
        C, R, P = rv.pose_from_null(p)
        if not (np.all(np.isfinite(C)) and np.all(np.isfinite(P))):
            continue
        # a hypothesis is scored under its own 11-parameter projection
        m = rv.inlier_mask(P, X, xy, thr)
        cost = float(rv.errors2(P, X, xy)[0][m].sum())
        if best is None or m.sum() > best[0]:
            best = (int(m.sum()), h, C, R, m, cost)
    if best is None:
        return dict(info=-2, mask=np.zeros(len(X), dtype=bool))
    count, h, C, R, m, cost = best
    out = dict(info=-3, best_hyp=h, best_count=count)
    if count >= min_inliers:
        for _ in range(rounds):
            Cn, Rn = refit(C, R, X[m], xy[m], ftol=1e-8, xtol=1e-8, gtol=1e-8)
            m2, cost2 = score(Cn, Rn, X, xy, thr)
            if not (m2.sum() > m.sum() or (m2.sum() == m.sum() and cost2 <= cost)):
                break
            changed = not np.array_equal(m, m2)
            C, R, m, cost = Cn, Rn, m2, cost2
            if not changed:
                break
        out["info"] = 1
    out.update(C=C, R=R, mask=m, cost=cost)
    return out


def converged(C, R, X, xy):
    cost = np.inf
    for _ in range(20):
        C, R = refit(C, R, X, xy, ftol=1e-15, xtol=1e-15, gtol=1e-15)
        c = float((residuals(np.zeros(6), R, C, X, xy) ** 2).sum())
        if not c < cost:
            break
        cost = c
    return C, R, cost


def main():
    sc = rv.load_scene()
    V, n_corr = sc["V"], len(sc["xy"])
    out = dict(threshold=np.array(THRESHOLD), n_v=sc["n_v"], truth=sc["truth"], C_min=np.zeros((V, 3)),
               R_min=np.zeros((V, 3, 3)), cost_min=np.zeros(V))
    for H in rv.HS[1:]:
        out[f"mask_H{H}"] = np.zeros(n_corr, dtype=bool)
        out[f"final_margin_H{H}"] = np.zeros(V)
    for v in sc["checked"]:
        X, xy = rv.view(sc, v)
        s, e = sc["view_start"][v], sc["view_start"][v + 1]
        truth = sc["truth"][s:e]
        C, R, cost = converged(sc["C_true"][v], sc["R_true"][v], X[truth], xy[truth])
        out["C_min"][v], out["R_min"][v], out["cost_min"][v] = C, R, cost
        for H in rv.HS[1:]:
            r = restate_view(X, xy, rv.sample_table(H)[v], THRESHOLD)
            assert r["info"] == 1, (v, H, r["info"])
            assert np.array_equal(r["mask"], truth), (v, H, int(r["mask"].sum()), int(truth.sum()), "reseed")
            e2 = rv.errors2(rv.projection(r["C"], r["R"]), X, xy)[0]
            margin = np.abs(np.sqrt(e2) - THRESHOLD).min()
            assert margin >= 1.0, (v, H, margin)
            out[f"mask_H{H}"][s:e] = r["mask"]
            out[f"final_margin_H{H}"][v] = margin
            print(f"view {v} n {e - s} H {H}: best_count {r['best_count']} of {int(truth.sum())}, margin "
                  f"{margin:.3g} px, |C - C_min| {np.linalg.norm(r['C'] - C):.3g}, angle "
                  f"{rv.rot_angle(r['R'], R):.3g}, cost / cost_min - 1 {r['cost'] / cost - 1:.3g}")
    path = os.path.join(HERE, "register_views.npz")
    np.savez_compressed(path, **out)
    print("register_views.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
