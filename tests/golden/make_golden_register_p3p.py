"""Generate tests/golden/register_p3p.npz: expected results of the calibrated
batched view registration (sfm_register_views_p3p).  numpy and scipy only: the
reference has no counterpart.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_register_p3p.py

The inputs are not stored: tests/test_register_p3p.py regenerates them from
seeds (load_scene, sample_table).  The restatement is that module's P3P
(Grunert's quartic through np.roots, solutions kept by the defining property),
the inlier rule, the winner (most inliers, then the smaller cost, then the
earlier hypothesis, then the earlier solution) and make_golden_register.py's
rounds of refit, re-score and not-worse test.
Stored: threshold, n_v, truth (the untouched observations); per view of 63
correspondences and more (zeros elsewhere) C_min, R_min, cost_min -- the
converged minimum of the squared reprojection error over the true inliers, as
make_golden_register.py computes it -- and per H in 64, 65, 256 the
restatement's final mask, the distance of its nearest final error from the
threshold and the hypotheses left out of per-hypothesis comparisons
(excluded_H*: ill-conditioned by test_register_p3p.ROOT_GAP / IMAG_BAND, or a
solution with an error within 1e-9 relative of the threshold); per planar view
the best count of the 6-point restatement at H = 256.
Asserted here, relied on by the tests:
  - for every such view and H the final mask is the truth and every final error
    is at least 1 px from the threshold;
  - at most 5 % of a view's hypotheses are excluded;
  - on the three planar views the 6-point restatement over register_samples at
    H = 256 has best_count < 6 (the capability gap);
  - on the 60 % view at H = 64 the 6-point table holds no all-inlier sample and
    the 3-point table at least three.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import conftest  # noqa: E402,F401  (puts the package on the path)
import make_golden_register as g6  # noqa: E402
import test_register_p3p as p3  # noqa: E402
import test_register_views as rv  # noqa: E402

THRESHOLD = p3.THRESHOLD


def restate_view(v, H, min_inliers=4, rounds=3):
    sc = p3.load_scene()
    X, xy = p3.view(sc, v)
    best = p3.restated_winner(v, H)
    if best is None:
        return dict(info=-2, mask=np.zeros(len(X), dtype=bool))
    count, cost, h, k, R, C, m = best
    out = dict(info=-3, best_hyp=h, best_count=count)
    if count >= min_inliers:
        for _ in range(rounds):
            Cn, Rn = g6.refit(C, R, X[m], xy[m], ftol=1e-8, xtol=1e-8, gtol=1e-8)
            m2, cost2 = g6.score(Cn, Rn, X, xy, THRESHOLD)
            if not (m2.sum() > m.sum() or (m2.sum() == m.sum() and cost2 <= cost)):
                break
            changed = not np.array_equal(m, m2)
            C, R, m, cost = Cn, Rn, m2, cost2
            if not changed:
                break
        out["info"] = 1
    out.update(C=C, R=R, mask=m, cost=cost)
    return out


def main():
    import _sfmcore
    sc = p3.load_scene()
    V, n_corr = sc["V"], len(sc["xy"])
    out = dict(threshold=np.array(THRESHOLD), n_v=sc["n_v"], truth=sc["truth"], C_min=np.zeros((V, 3)),
               R_min=np.zeros((V, 3, 3)), cost_min=np.zeros(V), six_point_best_count=np.zeros(V, dtype=np.int64))
    for H in p3.HS:
        out[f"mask_H{H}"] = np.zeros(n_corr, dtype=bool)
        out[f"final_margin_H{H}"] = np.zeros(V)
        out[f"excluded_H{H}"] = np.zeros((V, H), dtype=bool)
    for v in sc["checked"]:
        X, xy = p3.view(sc, v)
        s, e = sc["view_start"][v], sc["view_start"][v + 1]
        truth = sc["truth"][s:e]
        C, R, cost = g6.converged(sc["C_true"][v], sc["R_true"][v], X[truth], xy[truth])
        out["C_min"][v], out["R_min"][v], out["cost_min"][v] = C, R, cost
        for H in p3.HS:
            r = restate_view(v, H)
            assert r["info"] == 1, (v, H, r["info"])
            assert np.array_equal(r["mask"], truth), (v, H, int(r["mask"].sum()), int(truth.sum()), "reseed")
            e2 = rv.errors2(rv.projection(r["C"], r["R"]), X, xy)[0]
            margin = np.abs(np.sqrt(e2) - THRESHOLD).min()
            assert margin >= 1.0, (v, H, margin)
            ex = np.array([ill for _, ill in p3.restated_hypotheses(v, H)])
            assert ex.mean() <= p3.MAX_EXCLUDED, (v, H, ex.mean())
            out[f"mask_H{H}"][s:e] = r["mask"]
            out[f"final_margin_H{H}"][v] = margin
            out[f"excluded_H{H}"][v] = ex
            n_sol = [len(sols) for sols, _ in p3.restated_hypotheses(v, H)]
            print(f"view {v} n {e - s} H {H}: best_count {r['best_count']} of {int(truth.sum())}, margin "
                  f"{margin:.3g} px, |C - C_min| {np.linalg.norm(r['C'] - C):.3g}, angle "
                  f"{rv.rot_angle(r['R'], R):.3g}, cost / cost_min - 1 {r['cost'] / cost - 1:.3g}, mean n_sol "
                  f"{np.mean(n_sol):.2f}, excluded {int(ex.sum())}")
    t6 = _sfmcore.register_samples(sc["n_v"], 256, p3.SAMPLE_SEED)
    for v in p3.PLANAR:
        X, xy = p3.view(sc, v)
        out["six_point_best_count"][v] = p3.six_point_best_count(X, xy, t6[v], THRESHOLD)
        print(f"planar view {v}: 6-point best_count {out['six_point_best_count'][v]} of {len(X)}")
        assert out["six_point_best_count"][v] < 6, v
    s, e = sc["view_start"][p3.HARD], sc["view_start"][p3.HARD + 1]
    truth = sc["truth"][s:e]
    clean6 = truth[_sfmcore.register_samples(sc["n_v"], 64, p3.SAMPLE_SEED)[p3.HARD]].all(axis=1).sum()
    clean3 = truth[p3.sample_table(64)[p3.HARD]].all(axis=1).sum()
    print(f"60 % view at H = 64: {clean6} clean 6-point samples, {clean3} clean 3-point samples")
    assert clean6 == 0 and clean3 >= 3, "reseed"
    path = os.path.join(HERE, "register_p3p.npz")
    np.savez_compressed(path, **out)
    print("register_p3p.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
