"""Generates tests/golden/essential_pairs.npz: the numpy restatement
(tests/test_essential_pairs.py) of sfm_essential_pairs over the scene of that
module, for H in HS, with the margins the GPU tests rely on asserted here.  The
scene and the sample tables are regenerated from seeds and not stored.

    python tests/golden/make_golden_essential_pairs.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_essential_pairs as ep  # noqa: E402
import test_verify_pairs as vp  # noqa: E402

COND_BAR = 1e8          # the refit's scaled 5 x 5 normal equations
COST_FLOOR = 1e-9       # px^2
SOLS_H = 64             # the solutions of every hypothesis are stored for this H


def main():
    sc = ep.load_scene()
    P = sc["P"]
    out = dict(threshold=ep.THRESHOLD, n_p=sc["n_p"], truth=sc["truth"], E_true=sc["E_true"])
    for H in ep.HS:
        E, F = np.zeros((P, 3, 3)), np.zeros((P, 3, 3))
        cost, cond = np.zeros(P), np.zeros(P)
        n_inl, hyp, count, info = (np.zeros(P, dtype=np.int32) for _ in range(4))
        mask = np.zeros(len(sc["x1"]), dtype=bool)
        comp = np.zeros((P, H), dtype=bool)
        n_sol = np.zeros((P, H), dtype=np.int32)
        decided = np.zeros(P, dtype=bool)
        sols = np.zeros((P, H, 10, 3, 3))
        for p in range(P):
            x1, x2 = ep.pair(sc, p)
            s, e = sc["pair_start"][p], sc["pair_start"][p + 1]
            r = ep.restate_pair(x1, x2, ep.sample_table(H)[p])
            E[p], F[p], cost[p], cond[p] = r["E"], r["F"], r["cost"], r["cond"]
            n_inl[p], hyp[p], count[p], info[p] = r["n_inliers"], r["best_hyp"], r["best_count"], r["info"]
            mask[s:e] = r["mask"]
            if r["info"] == -1:
                continue
            comp[p] = [ep.comparable(i) for i in r["infos"]]
            assert comp[p].mean() >= 0.95, f"reseed: pair {p}, H {H}: {comp[p].mean():.3f} of the hypotheses comparable"
            for h, Es in enumerate(r["sols"]):
                n_sol[p, h] = len(Es)
                sols[p, h, :len(Es)] = Es
            assert r["info"] >= 1, f"reseed: pair {p}, H {H}: info {r['info']}"
            # no final distance at the threshold
            d = vp.distances(r["F"], x1, x2)
            assert np.abs(d - ep.THRESHOLD).min() > 1e-9 * ep.THRESHOLD, f"reseed: pair {p}, H {H}: a distance at the threshold"
            # the winner ahead of the runner-up: by one inlier, or by 1e-6 relative in cost and by
            # COST_FLOOR px^2, far above what rounding moves a cost by.  Exact points leave every
            # solution that holds them at a cost of rounding size (and five points hold all ten):
            # such a pair is recorded as not decided, and its winner is not compared
            t = sorted(r["table"], key=lambda q: (-q[1], q[2]))
            decided[p] = len(t) == 1 or t[0][1] > t[1][1] or t[1][2] - t[0][2] > max(1e-6 * t[0][2], COST_FLOOR)
            assert decided[p] or ep.KINDS[p] == "clean", f"reseed: pair {p}, H {H}: the winner is not ahead"
            assert r["cond"] < COND_BAR, f"reseed: pair {p}, H {H}: refit conditioned {r['cond']:.3g}"
            # with outliers among general points, the mask is the truth (on the plane the twin
            # pose takes a few of the moved matches with it, which is what the fixture records)
            if ep.KINDS[p] == "wrong" and H >= 64:
                assert np.array_equal(r["mask"], sc["truth"][s:e]), f"reseed: pair {p}, H {H}: mask is not the truth"
            print(f"H {H:3d} pair {p:2d} n {len(x1):5d} info {r['info']} inliers {r['n_inliers']:5d} "
                  f"best {r['best_hyp']:3d}/{r['best_count']:5d} cond {r['cond']:.3g} comparable {comp[p].mean():.3f}")
        out.update({f"E_H{H}": E, f"F_H{H}": F, f"cost_H{H}": cost, f"cond_H{H}": cond, f"n_inliers_H{H}": n_inl,
                    f"best_hyp_H{H}": hyp, f"best_count_H{H}": count, f"info_H{H}": info, f"mask_H{H}": mask,
                    f"comparable_H{H}": comp, f"n_sol_H{H}": n_sol, f"decided_H{H}": decided})
        if H == SOLS_H:
            out["sols"] = sols
    np.savez_compressed(os.path.join(HERE, "essential_pairs.npz"), **out)
    print("wrote essential_pairs.npz", os.path.getsize(os.path.join(HERE, "essential_pairs.npz")), "bytes")


if __name__ == "__main__":
    main()
