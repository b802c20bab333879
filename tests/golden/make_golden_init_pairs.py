"""Generate tests/golden/init_pairs.npz: what the tests of the batched
initial-pair selection (sfm_init_pairs) rely on.  numpy only: the rule is
restated in tests/test_init_pairs.py (restate_pair), which also regenerates the
scene from seeds.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_init_pairs.py

Stored: n_p, Hh, h_threshold, max_reproj; F (P x 3 x 3), the numpy least-squares
F of every pair's correspondences (pair f: pair a's; pairs e: zeros, and pair
a's with one NaN); f_shift, pair f's displacements along the epipolar lines of
F[a] (0 for the points that stay); per pair the restatement's info, counts,
n_good, median angle, h_count and the winner's rotation and direction errors
against the true relative pose.
Asserted here, relied on by the tests: pair b has the most correspondences, its
median angle lies below the eligibility limit (4 degrees) and pair a's above;
pair c has h_count >= 0.95 n and pair a h_count <= 0.5 n; in every pair the
share of correspondences whose cheirality depth or reprojection threshold lies
within 1e-9 relative of its limit is below 1 %; the winning candidate has more
than 1 % of the pair more points than the next; E has sigma_2 / sigma_1 >=
1e-3; every sampled 8 x 9 homography system has sigma_8 / sigma_1 >= 1e-5, so a
hypothesis maps its own sample to 1e-6 px; every moved point of pair f, and no
other, is not good.  Reseed (SEED, SAMPLE_SEED in the test module) if one fails.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_init_pairs as ip  # noqa: E402
import test_verify_pairs as vp  # noqa: E402
import _sfmcore  # noqa: E402


def displacements(x1, x2, F):
    """per chosen point of pair f, the first shift along its epipolar line that
    the restatement calls not good, clear of every limit"""
    cands = ip.candidates(F)
    counts = [ip.front(R, t, ip.triangulate(ip.proj2(R, t), x1, x2))[0].sum() for R, t in cands]
    R, t = cands[int(np.argmax(counts))]
    d = ip.epipolar_direction(F, x1)
    shift = np.zeros(len(x1))
    for i in ip.moved_indices():
        for s in [k * sg for k in (60, 120, 240, 480, 960, 1920) for sg in (1.0, -1.0)]:
            q = x2[i:i + 1] + s * d[i:i + 1]
            X, good, _, near = ip.points_under(R, t, x1[i:i + 1], q)
            z1, z2, _ = ip.depths(R, t, X)
            clear = (min(z1[0], z2[0]) < -1e-3 * np.linalg.norm(X[0])) or \
                max(ip.reproj2(ip.P1, X, x1[i:i + 1])[0], ip.reproj2(ip.proj2(R, t), X, q)[0]) > 4 * ip.MAX_REPROJ ** 2
            if not good[0] and not near[0] and clear:
                shift[i] = s
                break
        assert shift[i] != 0, (i, "no displacement found")
    return shift


def main():
    raw = ip.raw_pairs()
    P = len(ip.SIZES)
    F = np.zeros((P, 3, 3))
    for p, (x1, x2, _, _) in enumerate(raw):
        if len(x1) >= 8 and ip.KINDS[p] not in ("e0", "e1", "f"):
            F[p] = vp.fit(x1, x2)
    F[ip.PF] = F[ip.PA]
    F[ip.PE1] = F[ip.PA]
    F[ip.PE1][1, 2] = np.nan
    f_shift = displacements(raw[ip.PF][0], raw[ip.PF][1], F[ip.PA])
    sc = ip.assemble(raw, F, f_shift)
    n_p = sc["n_p"]
    tab = _sfmcore.homography_samples(n_p, ip.HH, ip.SAMPLE_SEED)
    out = dict(n_p=n_p, Hh=np.array(ip.HH), h_threshold=np.array(ip.H_THRESHOLD), max_reproj=np.array(ip.MAX_REPROJ),
               F=F, f_shift=f_shift, info=np.zeros(P, dtype=np.int32), counts=np.zeros((P, 4), dtype=np.int64),
               n_good=np.zeros(P, dtype=np.int32), median=np.zeros(P), h_count=np.zeros(P, dtype=np.int32),
               pose_errors=np.zeros((P, 2)))
    res = []
    for p in range(P):
        x1, x2 = ip.pair(sc, p)
        r = ip.restate_pair(x1, x2, F[p], tab[p])
        res.append(r)
        out["info"][p], out["h_count"][p] = r["info"], r["h_count"]
        if len(x1) >= 8:
            weakest = min(vp.sv_ratio(ip.h_fit(x1[s], x2[s])[1]) for s in tab[p])
            assert weakest >= 1e-5, (p, weakest, "reseed")
        if r["info"] != 0:
            print(f"pair {p} ({ip.KINDS[p]}) n {len(x1)}: info {r['info']}, h_count {r['h_count']}")
            continue
        S = np.linalg.svd(ip.K.T @ F[p] @ ip.K, compute_uv=False)
        assert S[1] >= 1e-3 * S[0], (p, S, "reseed")
        share = r["near"].sum() / len(x1)
        assert share < 0.01, (p, share, "reseed")
        c = np.sort(r["counts"])
        assert c[3] - c[2] > 0.01 * len(x1), (p, r["counts"], "reseed")
        e = ip.pose_errors(r["R"], r["C"], sc["R_true"][p], sc["C_true"][p])
        out["counts"][p], out["n_good"][p], out["median"][p], out["pose_errors"][p] = \
            r["counts"], r["n_good"], r["median"], e
        print(f"pair {p} ({ip.KINDS[p]}) n {len(x1)}: counts {r['counts'].tolist()}, good {r['n_good']}, median angle "
              f"{np.rad2deg(r['median']):.3g} deg, h_count {r['h_count']}, rotation error {e[0]:.3g} rad, direction "
              f"error {e[1]:.3g} rad, sigma_2 / sigma_1 {S[1] / S[0]:.3g}, weakest sample {weakest:.3g}")
    limit = np.deg2rad(ip.MIN_ANGLE_DEG)
    assert n_p[ip.PB] == n_p.max() and (n_p == n_p.max()).sum() == 1
    assert res[ip.PB]["median"] < limit < res[ip.PA]["median"], "reseed"
    assert res[ip.PC]["h_count"] >= 0.95 * n_p[ip.PC] and res[ip.PA]["h_count"] <= 0.5 * n_p[ip.PA], "reseed"
    assert res[ip.PD]["info"] == -1 and res[ip.PE0]["info"] == -2 and res[ip.PE1]["info"] == -2
    assert res[ip.PE0]["h_count"] > 0 and res[ip.PE1]["h_count"] > 0
    assert np.array_equal(res[ip.PF]["good"], ~sc["moved"]), "reseed"
    assert res[ip.PA]["good"].all(), "reseed"       # so that pair f's other points are all good
    path = os.path.join(HERE, "init_pairs.npz")
    np.savez_compressed(path, **out)
    print("init_pairs.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
