"""Batched initial-pair selection, timed: sfm_init_pairs (every verified pair in
one call) against the only route there was before it -- two_view_init looped
per pair (E and the candidates by numpy on the host, one sfm_two_view_select
call per pair; no reprojection check, no parallax, no homography), timed over
the first --loop-pairs pairs.  The loop is a time to set beside the call's, not
the same result.

Shape: 4,950 pairs (100 images) x 2,000 correspondences x Hh = 128, cfg2's
two-view geometry with 0.5 px noise and its true F for every pair.  Per round:
the median over --reps calls after a warm-up of the whole call (host clock
around a call that ends in a stream synchronise), of the kernels (HIP events,
sfm_last_timings, in calls of their own) and of the loop.

    python tools/init_pairs_once.py [--pairs 4950] [--n 2000] [--Hh 128] [--rounds 3] [--reps 5] [--loop-pairs 100] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "structure-from-motion-_amd"))
import _sfmcore as core  # noqa: E402
import sfm_synthetic as syn  # noqa: E402
from sfm_two_view import two_view_init  # noqa: E402

K = syn.K_REF


def scene(P, n, seed=3):
    """P pairs of n correspondences of cfg2's geometry, each pair with its own points; the true F"""
    rng = np.random.default_rng(seed)
    N = P * n
    X = np.column_stack([rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(5, 12, N)])
    R2 = syn.rotvec_to_matrix([0.02, -0.15, 0.01])[0]
    C2 = np.array([1.0, 0.05, 0.1])

    def proj(R, C):
        u = (K @ (R @ (X - C).T)).T
        return u[:, :2] / u[:, 2:3]
    x1 = proj(np.eye(3), np.zeros(3)) + rng.normal(0, 0.5, (N, 2))
    x2 = proj(R2, C2) + rng.normal(0, 0.5, (N, 2))
    t = -R2 @ C2
    Ki = np.linalg.inv(K)
    F = Ki.T @ np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R2 @ Ki
    F = np.tile(F / np.linalg.norm(F), (P, 1, 1))
    return np.arange(P + 1, dtype=np.int64) * n, np.ascontiguousarray(x1), np.ascontiguousarray(x2), F


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4950)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--Hh", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-pairs", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    P, n = a.pairs, a.n
    ps, x1, x2, F = scene(P, n)
    hs = core.homography_samples(np.diff(ps), a.Hh, 0) if a.Hh else None
    L = min(a.loop_pairs, P)
    per_pair = [(F[p], np.ascontiguousarray(x1[ps[p]:ps[p + 1]]), np.ascontiguousarray(x2[ps[p]:ps[p + 1]]))
                for p in range(L)]

    def call():
        return core.init_pairs(K, ps, x1, x2, F, hs)

    def timings():
        call()
        return core.last_timings()

    def loop():
        for Fp, p1, p2 in per_pair:
            two_view_init(Fp, K, p1, p2)

    out = call()
    row = dict(pairs=P, correspondences=n, Hh=a.Hh, info_counts=np.bincount(out[9] + 2, minlength=3).tolist(),
               median_good_share=float(np.median(out[4] / n)), median_angle_deg=float(np.rad2deg(np.median(out[5]))),
               median_h_share=float(np.median(out[6] / n)), loop_pairs=L, rounds=[])
    for _ in range(a.rounds):
        whole = median_ms(call, a.reps)
        core.set_call_timing(True)
        k = np.median(np.array([timings() for _ in range(a.reps + 1)][1:]), axis=0)
        core.set_call_timing(False)
        lp = median_ms(loop, 3)
        row["rounds"].append(dict(call_ms=whole, upload_ms=float(k[0]), kernels_ms=float(k[1]), download_ms=float(k[2]),
                                  homography_ms=float(k[3]), loop_ms=lp))
        print(f"call {whole:.2f} ms; sfm_last_timings: upload {k[0]:.2f}, kernels {k[1]:.2f} (homography {k[3]:.2f}), "
              f"download {k[2]:.2f} ms; two_view_init looped over {L} pairs {lp:.1f} ms "
              f"({lp / L * P:.0f} ms for {P} at that rate)", flush=True)
    print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
