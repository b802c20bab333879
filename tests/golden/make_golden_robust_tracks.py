"""Generate tests/golden/robust_tracks.npz: expected results of the robust
track triangulation (sfm_triangulate_tracks_robust).  numpy and scipy only:
the reference has no counterpart.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_robust_tracks.py

The inputs are not stored: tests/test_robust_tracks.py regenerates them from
seeds (CASES, load_case): the clean observations of sfm_synthetic.ba_problem
under the true cameras (0.5 px noise), n_out observations of every track
displaced by 40-120 px.  restate_track below is the algorithm in numpy: the
two-view hypotheses by SVD, the kernel's enumeration, inlier rule and
tie-break, a refit of the winner's inliers (SVD DLT, then scipy's lm from it)
and one re-score.  Stored per case (key prefix): truth (the untouched
observations), mask (the restatement's final mask), best_count (the largest
hypothesis count per track), X_lin (the refit's linear point), X (its refined
point), kept (the tracks the comparisons cover: all of them but in r3o1, where
two views of three cannot always outvote the third).
Asserted here, relied on by the tests:
  the final mask is the truth on every kept track, and every track is kept
  (r3o1: at least 250 of 257);
  final_margin  every final error is at least 1 px from the 4-px threshold;
  hyp_margin    every (hypothesis, observation) error that enters a count is
                at least 1e-6 px from the threshold and every such depth at
                least 1e-6 from 0 and from 1e-8, so that no count depends on
                rounding (the smallest distance is stored).
"""
import os
import sys

import numpy as np
from scipy.optimize import least_squares

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_multiview as tm  # noqa: E402
import test_robust_tracks as tr  # noqa: E402


def restate_track(P, cams, xy, threshold, max_pairs, min_inliers):
    """One track.  Returns mask (final), best_count, best_pair, info (1
    refined, -2, -3), X_lin, X, final_margin and hyp_margin in pixels."""
    n = len(cams)
    out = dict(mask=np.zeros(n, dtype=bool), best_count=0, best_pair=-1, info=-2, X_lin=np.zeros(3), X=np.zeros(3),
               final_margin=np.inf, hyp_margin=np.inf)
    if n < 2:
        return out
    best = None
    for k, (i, j) in enumerate(tr.pairs(n, max_pairs)):
        X = tm.dlt_svd(P, cams[[i, j]], xy[[i, j]])[0]
        m = tr.inlier_mask(P, cams, xy, X, threshold)
        if np.all(np.isfinite(X)):
            e2, h2 = tr.errors2(P, cams, xy, X)
            front = h2 > 1e-8
            margin = min(np.abs(h2).min(), np.abs(np.abs(h2) - 1e-8).min())
            if front.any():
                margin = min(margin, np.abs(np.sqrt(e2[front]) - threshold).min())
            out["hyp_margin"] = min(out["hyp_margin"], margin)
        e2 = tr.errors2(P, cams, xy, X)[0] if m.any() else np.zeros(n)
        sse = 0.0
        for v in e2[m]:  # added in observation order
            sse += v
        key = (-int(m.sum()), sse, k)
        if best is None or key < best[0]:
            best = (key, X, m)
    (neg_count, _, k), X, m = best
    out.update(best_count=-neg_count, best_pair=k, mask=m, X_lin=X, X=X, info=-3)
    if -neg_count < min_inliers:
        return out
    X_lin = tm.dlt_svd(P, cams[m], xy[m])[0]
    r = least_squares(lambda x: tm.residuals(P, cams[m], xy[m], x), X_lin, method="lm", ftol=1e-8, xtol=1e-8,
                      gtol=1e-8, max_nfev=50 * 4)
    e2, h2 = tr.errors2(P, cams, xy, r.x)
    out.update(info=1, X_lin=X_lin, X=r.x, mask=tr.inlier_mask(P, cams, xy, r.x, threshold),
               final_margin=np.abs(np.sqrt(e2) - threshold).min())
    return out


def case(name, out):
    c = tr.load_case(name)
    T, k = c["T"], c["k"]
    mask = np.zeros(T * k, dtype=bool)
    best_count = np.zeros(T, dtype=np.int32)
    X_lin, X = np.zeros((T, 3)), np.zeros((T, 3))
    kept = np.zeros(T, dtype=bool)
    final_margin, hyp_margin, worst_inlier = np.inf, np.inf, 0.0
    for t in range(T):
        cams, xy = tm.track(c, t)
        r = restate_track(c["P"], cams, xy, tr.THRESHOLD, tr.MAX_PAIRS, 2)
        mask[t * k:(t + 1) * k], best_count[t], X_lin[t], X[t] = r["mask"], r["best_count"], r["X_lin"], r["X"]
        kept[t] = r["info"] == 1 and np.array_equal(r["mask"], c["truth"][t * k:(t + 1) * k])
        hyp_margin = min(hyp_margin, r["hyp_margin"])
        if kept[t]:
            final_margin = min(final_margin, r["final_margin"])
            worst_inlier = max(worst_inlier, np.sqrt(tr.errors2(c["P"], cams, xy, r["X"])[0][r["mask"]]).max())
    if name == "r3o1":
        assert kept.sum() >= 250, kept.sum()
    else:
        assert kept.all(), (name, np.where(~kept)[0])
    assert final_margin >= 1.0, final_margin
    assert hyp_margin >= 1e-6, (name, hyp_margin, "reseed the case")
    out.update({f"{name}_truth": c["truth"], f"{name}_mask": mask, f"{name}_best_count": best_count,
                f"{name}_X_lin": X_lin, f"{name}_X": X, f"{name}_kept": kept,
                f"{name}_final_margin": np.array(final_margin), f"{name}_hyp_margin": np.array(hyp_margin)})
    print(name, f"kept {kept.sum()} of {T}, final margin {final_margin:.3g} px, hypothesis margin {hyp_margin:.3g}, "
          f"largest inlier error {worst_inlier:.3g} px")


def main():
    out = {}
    for name in tr.CASES:
        case(name, out)
    path = os.path.join(HERE, "robust_tracks.npz")
    np.savez_compressed(path, **out)
    print("robust_tracks.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
