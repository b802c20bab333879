"""Batched pair verification, timed: sfm_verify_pairs (every image pair in one
call) against the only route the drop-ins give -- per pair one sfm_ransac_f8
over the same H x 8 table (the reference's convention and symmetric epipolar
distance, no refit; Wrapper_dev.py:69-123); the per-pair arrays are built
outside the timed region.  The loop is a time to set beside the call's, not the
same result: its F misses its own sample points.

Shapes: "p3" 10 pairs x 500 correspondences (P3Data scale) and "full" 4,950
pairs (100 images) x 2,000; a quarter of the matches displaced by 40-120 px
along the normal of their epipolar line, 0.5 px noise on the rest.  Per shape
and round: the median over --reps calls after a warm-up of the whole call (host
clock around a call that ends in a stream synchronise), of the kernels (HIP
events, sfm_last_timings, in calls of their own) and of the per-pair loop.  The
share of the FP64 VALU peak uses the flop model below.

    python tools/verify_pairs_once.py [--shape p3 full] [--H 256] [--rounds 3] [--reps 20] [--loop-reps 3] [--out FILE]
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

FP64_PEAK = 78.6e12  # MI355X vector FP64, flop/s
SHAPES = {"p3": (10, 500), "full": (4950, 2000)}
K = syn.K_REF


def flop_model(P, n, H, rounds=2.0, sweeps=8.0):
    """Fit, per hypothesis: the Householder LQ of the 8 x 9 design over 8 lanes
    (8 reflectors x 8 lanes x ~40 and the back-substitution 8 x 8 x 36) ~4,900,
    the two normalisations and the rank-2 / denormalise / scale step on every
    lane 8 x ~250 = 2,000: 6,900.  Score, per hypothesis and correspondence: two
    lines 20, e 5, den 7, the test 3 = 35.  Refit, per pair and round (``rounds``
    ASSUMED): over 0.75 n inliers the Hartley sums 14 and a Givens absorption
    of one row, 9 rotations of ~6 + 6 (9 - j) = 330; the tree merge 7 levels x 9
    rows x 330 on the longest path, counted once per thread, 128 x 9 x 330; one
    lane's Jacobi, ``sweeps`` ASSUMED x 36 pairs x ~200; a re-score of n at 40."""
    fit = P * H * 6900.0
    score = P * H * n * 35.0
    refit = P * rounds * (0.75 * n * 344 + 128 * 9 * 330 + sweeps * 36 * 200 + n * 40)
    return fit, score, refit


def scene(P, n, seed=3):
    """P pairs of n correspondences of cfg2's geometry, each pair with its own points"""
    rng = np.random.default_rng(seed)
    N = P * n
    X = np.column_stack([rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(5, 12, N)])
    R2 = syn.rotvec_to_matrix([0.02, -0.15, 0.01])[0]
    C2 = np.array([1.0, 0.05, 0.1])

    def proj(R, C):
        u = (K @ (R @ (X - C).T)).T
        return u[:, :2] / u[:, 2:3]
    c1 = proj(np.eye(3), np.zeros(3))
    x1 = c1 + rng.normal(0, 0.5, (N, 2))
    x2 = proj(R2, C2) + rng.normal(0, 0.5, (N, 2))
    t = -R2 @ C2
    Ki = np.linalg.inv(K)
    F = Ki.T @ np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R2 @ Ki
    bad = rng.random(N) < 0.25
    l = np.column_stack([c1[bad], np.ones(bad.sum())]) @ F.T
    nrm = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
    x2[bad] += (rng.uniform(40, 120, bad.sum()) * rng.choice([-1.0, 1.0], bad.sum()))[:, None] * nrm
    return np.arange(P + 1, dtype=np.int64) * n, np.ascontiguousarray(x1), np.ascontiguousarray(x2), ~bad


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
    ap.add_argument("--shape", nargs="+", default=["p3", "full"])
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=2.5)
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    res = []
    for name in a.shape:
        P, n = SHAPES[name]
        ps, x1, x2, good = scene(P, n)
        samples = core.pair_samples(np.diff(ps), a.H, 0)
        per_pair = [(np.ascontiguousarray(x1[ps[p]:ps[p + 1]]), np.ascontiguousarray(x2[ps[p]:ps[p + 1]]),
                     np.ascontiguousarray(samples[p])) for p in range(P)]

        def call():
            return core.verify_pairs(ps, x1, x2, samples, threshold=a.threshold)

        def kernels():
            call()
            return core.last_timings()[[1, 3]]

        def loop():
            for p1, p2, s8 in per_pair:
                core.ransac_f8(p1, p2, s8, 0.06)

        out = call()
        row = dict(shape=name, pairs=P, correspondences=n, H=a.H, info_counts=np.bincount(out[6] + 3).tolist(),
                   median_inlier_share=float(np.median(out[2] / n)),
                   masks_equal_truth=int(sum(np.array_equal(out[3][ps[p]:ps[p + 1]], good[ps[p]:ps[p + 1]])
                                             for p in range(P))), rounds=[])
        for _ in range(a.rounds):
            whole = median_ms(call, a.reps)
            core.set_call_timing(True)
            k = np.median(np.array([kernels() for _ in range(a.reps + 1)][1:]), axis=0)
            core.set_call_timing(False)
            lp = median_ms(loop, a.loop_reps)
            row["rounds"].append(dict(call_ms=whole, kernels_ms=float(k[0]), fit_score_ms=float(k[1]), loop_ms=lp))
            print(f"{name}: call {whole:.3f} ms, kernels {k[0]:.3f} ms (fit and score {k[1]:.3f}), per-pair loop "
                  f"({P} calls) {lp:.1f} ms", flush=True)
        fit, score, refit = flop_model(P, n, a.H)
        kern = float(np.median([r["kernels_ms"] for r in row["rounds"]])) * 1e-3
        row.update(model_flops=dict(fit=fit, score=score, refit=refit), fp64_share=(fit + score + refit) / FP64_PEAK / kern)
        print(f"{name}: model {fit / 1e9:.2f} + {score / 1e9:.2f} + {refit / 1e9:.2f} GFLOP (fit + score + refit) -> "
              f"{100 * row['fp64_share']:.2f} % of FP64 VALU peak; median inlier share "
              f"{row['median_inlier_share']:.3f}; masks equal to the truth {row['masks_equal_truth']} of {P}",
              flush=True)
        res.append(row)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
