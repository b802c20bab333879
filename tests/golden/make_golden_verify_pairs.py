"""Generate tests/golden/verify_pairs.npz: expected results of the batched pair
verification (sfm_verify_pairs).  numpy only: the reference's pair loop has no
counterpart of the consistent convention.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_verify_pairs.py

The inputs are not stored: tests/test_verify_pairs.py regenerates them from
seeds (load_scene, sample_table, store_scene) and holds the rule in numpy
(restate_pair).
Stored: threshold, n_p, truth (the matches that were not displaced); per pair of
nine correspondences and more (zeros elsewhere) and per H in 64, 65, 256 the
restatement's final F and the distance of its nearest final Sampson distance
from the threshold; the restatement's pose errors on the store scene; and a
table of _sfmcore.register_samples as recorded when pair_samples joined it.
Asserted here, relied on by the tests, for every such pair and H: the
restatement's final mask is the truth; every final distance is at least 0.5 px
from the threshold; the inlier design matrix of the final fit has sigma_8 /
sigma_1 >= 1e-4; at most 5 % of all sampled 8 x 9 design matrices have sigma_8 /
sigma_1 < 1e-6.  For the pairs of 8 and 9 noise-free correspondences: every
correspondence an inlier and the true F to 1e-8.  For the store scene: the best
pair's restated F gives the true relative rotation within 0.01 rad and the
direction of C within 0.025 rad, half of what the GPU test allows.
Reseed (SEED, STORE_SEED in the test module) if one fails.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_verify_pairs as vp  # noqa: E402


def pose_from_F(F, x1, x2):
    """two_view_init in numpy: E = K^T F K, the four candidates, the one with
    the most points in front of both cameras (the first maximum)"""
    from EssentialMatrixFromFundamentalMatrix import EssentialMatrixFromFundamentalMatrix
    from ExtractCameraPose import ExtractCameraPose
    Cset, Rset = ExtractCameraPose(EssentialMatrixFromFundamentalMatrix(F, vp.K))
    P1 = vp.K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    counts = []
    for C, R in zip(Cset, Rset):
        P2 = vp.K @ np.hstack([R, -R @ C.reshape(3, 1)])
        n = 0
        for (u1, v1), (u2, v2) in zip(x1, x2):
            A = np.array([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]])
            X = np.linalg.svd(A)[2][-1]
            X = X[:3] / X[3]
            n += X[2] > 0 and (R[2] @ (X - C)) > 0
        counts.append(n)
    best = int(np.argmax(counts))
    return Cset[best], Rset[best]


def store_errors():
    sc = vp.store_scene()
    st = sc["store"]
    pair_ij, pair_start, i1, i2 = st.pairs()
    x1 = np.column_stack([st.x[i1], st.y[i1]])
    x2 = np.column_stack([st.x[i2], st.y[i2]])
    import _sfmcore
    samples = _sfmcore.pair_samples(np.diff(pair_start), 256, 0)
    res = [vp.restate_pair(x1[s:e], x2[s:e], samples[p], vp.THRESHOLD)
           for p, (s, e) in enumerate(zip(pair_start[:-1], pair_start[1:]))]
    n_inl = np.array([int(r["mask"].sum()) for r in res])
    order = np.argsort(-n_inl, kind="stable")
    b = int(order[0])
    i, j = pair_ij[b]
    s, e = pair_start[b], pair_start[b + 1]
    m = res[b]["mask"]
    C, R = pose_from_F(res[b]["F"], x1[s:e][m], x2[s:e][m])
    Rt, Ct = vp.relative_pose(sc, i, j)
    # the wrong matches against image 0 are outliers of their pairs, everything else of them an inlier
    for p, (a, c) in enumerate(pair_ij):
        if a != 0:
            continue
        feat = st.feature[i1[pair_start[p]:pair_start[p + 1]]]
        assert np.array_equal(res[p]["mask"], ~sc["wrong"][feat, c]), (a, c)
    return (i, j), n_inl, vp.rot_angle(R, Rt), vp.direction_angle(C, Ct)


def main():
    sc = vp.load_scene()
    P = sc["P"]
    out = dict(threshold=np.array(vp.THRESHOLD), n_p=sc["n_p"], truth=sc["truth"])
    weak = total = 0
    for H in vp.HS:
        out[f"F_H{H}"] = np.zeros((P, 3, 3))
        out[f"margin_H{H}"] = np.zeros(P)
        tab = vp.sample_table(H)
        for p in range(P):
            x1, x2 = vp.pair(sc, p)
            n = len(x1)
            if n < 8:
                continue
            s, e = sc["pair_start"][p], sc["pair_start"][p + 1]
            truth = sc["truth"][s:e]
            r = vp.restate_pair(x1, x2, tab[p], vp.THRESHOLD)
            if n < vp.NOISY_FROM:  # noise-free: everything an inlier, the true F
                err = np.linalg.norm(vp.align(r["F"], sc["F_true"][p]) - sc["F_true"][p])
                assert r["mask"].all() and err <= 1e-8, (p, H, err)
            if n < 9:
                continue
            ratios = np.array([vp.sv_ratio(vp.design(x1[q], x2[q])[0]) for q in tab[p]])
            weak += int((ratios < 1e-6).sum())
            total += len(ratios)
            assert r["info"] in (1, 2), (p, H, r["info"])
            assert np.array_equal(r["mask"], truth), (p, H, int(r["mask"].sum()), int(truth.sum()), "reseed")
            margin = np.abs(vp.distances(r["F"], x1, x2) - vp.THRESHOLD).min()
            assert margin >= 0.5, (p, H, margin, "reseed")
            cond = vp.sv_ratio(vp.design(x1[truth], x2[truth])[0])
            assert cond >= 1e-4, (p, H, cond)
            out[f"F_H{H}"][p] = r["F"]
            out[f"margin_H{H}"][p] = margin
            print(f"pair {p} n {n} H {H}: best_count {r['best_count']} of {int(truth.sum())}, info {r['info']}, "
                  f"margin {margin:.3g} px, sigma_8 / sigma_1 {cond:.3g}, weakest sample "
                  f"{ratios.min():.3g}")
    assert weak <= 0.05 * total, (weak, total)
    print(f"sampled design matrices under 1e-6: {weak} of {total}")
    pair_b, n_inl, e_rot, e_dir = store_errors()
    print(f"store scene: best pair {tuple(pair_b)}, inliers {n_inl.tolist()}, rotation error {e_rot:.3g} rad, "
          f"direction error {e_dir:.3g} rad")
    assert e_rot < 0.01 and e_dir < 0.025, (e_rot, e_dir, "reseed")
    out["store_errors"] = np.array([e_rot, e_dir])
    out["store_best_pair"] = np.array(pair_b)
    import _sfmcore
    out["register_table"] = _sfmcore.register_samples([5, 6, 7, 40, 0, 1025], 65, 9)
    path = os.path.join(HERE, "verify_pairs.npz")
    np.savez_compressed(path, **out)
    print("verify_pairs.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
