"""Batched view registration, timed: sfm_register_views (every candidate view in
one call) against the only route the 4-point drop-ins give -- per view one
sfm_pnp_ransac over an H x 4 table and one sfm_nonlinear_pnp on all of the
view's points (Wrapper_dev.py:241-249), with the same H; the per-view index
lists and arrays are built outside the timed region.

Shapes: "p3" 4 views x 500 correspondences (P3Data scale) and "cfg5" 198 views
x 20,000 (4M observations over 200 cameras); 30 % of the observations displaced
by 40-120 px, 0.5 px noise on the rest.  Per shape and round: the median over
--reps calls after a warm-up of the whole call (host clock around a call that
ends in a stream synchronise), of the kernels (HIP events, sfm_last_timings, in
calls of their own) and of the per-view loop.  The share of the FP64 VALU peak
uses the flop model below.

    python tools/register_once.py [--shape p3 cfg5] [--H 256] [--rounds 3] [--reps 20] [--loop-reps 3] [--out FILE]
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
SHAPES = {"p3": (4, 500), "cfg5": (198, 20000)}
K = syn.K_REF


def flop_model(V, n, H, sweeps=8.0, evals=12.0):
    """Fit, per hypothesis: ``sweeps`` Jacobi sweeps ASSUMED, 66 column pairs
    each, a pair 16 lanes x (6 for the three products, 12 for the butterflies,
    ~40 for the rotation with its three divisions and two square roots at one
    flop each, 12 for the four updates) = 1120.  Score, per hypothesis and
    correspondence: h 21, the scaled test 16 = 37.  Refit, per view: ``evals``
    cost evaluations ASSUMED over 0.7 n inliers at 330 flops (pose 33, six
    Jacobian columns 6 x 23, J^T J and J^T r 159), plus 4 re-scores of n at 45."""
    fit = V * H * sweeps * 66 * 1120
    score = V * H * n * 37
    refit = V * (evals * 0.7 * n * 330 + 4 * n * 45)
    return fit, score, refit


def scene(V, n, seed=3):
    p = syn.ba_problem(max(V, 2), max(2 * n, 1000), 2, seed=seed, dense=False)
    X = p["X_true"]
    rng = np.random.default_rng(seed + 1)
    pt, xy = [], []
    for v in range(V):
        idx = rng.choice(len(X), n, replace=False)
        h = (K @ (p["R_true"][v] @ (X[idx] - p["C_true"][v]).T)).T
        o = h[:, :2] / h[:, 2:] + rng.normal(0, 0.5, (n, 2))
        bad = rng.choice(n, int(0.3 * n), replace=False)
        ang, mag = rng.uniform(0, 2 * np.pi, len(bad)), rng.uniform(40, 120, len(bad))
        o[bad] += np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
        pt.append(idx)
        xy.append(o)
    return (np.ascontiguousarray(X), np.arange(V + 1, dtype=np.int64) * n, np.concatenate(pt).astype(np.int32),
            np.ascontiguousarray(np.concatenate(xy)))


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
    ap.add_argument("--shape", nargs="+", default=["p3", "cfg5"])
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=4.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    res = []
    for name in a.shape:
        V, n = SHAPES[name]
        X, vs, pt, xy = scene(V, n)
        samples = core.register_samples(np.diff(vs), a.H, 0)
        per_view = [(np.ascontiguousarray(X[pt[vs[v]:vs[v + 1]]]), np.ascontiguousarray(xy[vs[v]:vs[v + 1]]),
                     np.ascontiguousarray(samples[v][:, :4])) for v in range(V)]

        def call():
            return core.register_views(K, X, vs, pt, xy, samples, threshold=a.threshold)

        def kernels():
            call()
            return core.last_timings()[[1, 3]]

        def loop():
            for Xv, xv, s4 in per_view:
                _, _, C, R, _, _ = core.pnp_ransac(Xv, xv, K, s4, a.threshold)
                core.nonlinear_pnp(Xv, xv, K, C, R)

        out = call()
        row = dict(shape=name, views=V, correspondences=n, H=a.H, info_counts=np.bincount(out[7] + 4).tolist(),
                   median_inlier_share=float(np.median(out[3] / n)), rounds=[])
        for _ in range(a.rounds):
            whole = median_ms(call, a.reps)
            core.set_call_timing(True)
            k = np.median(np.array([kernels() for _ in range(a.reps + 1)][1:]), axis=0)
            core.set_call_timing(False)
            lp = median_ms(loop, a.loop_reps)
            row["rounds"].append(dict(call_ms=whole, kernels_ms=float(k[0]), fit_score_ms=float(k[1]), loop_ms=lp))
            print(f"{name}: call {whole:.3f} ms, kernels {k[0]:.3f} ms (fit and score {k[1]:.3f}), per-view loop "
                  f"({2 * V} calls) {lp:.1f} ms", flush=True)
        fit, score, refit = flop_model(V, n, a.H)
        kern = float(np.median([r["kernels_ms"] for r in row["rounds"]])) * 1e-3
        row.update(model_flops=dict(fit=fit, score=score, refit=refit), fp64_share=(fit + score + refit) / FP64_PEAK / kern)
        print(f"{name}: model {fit / 1e9:.2f} + {score / 1e9:.2f} + {refit / 1e9:.2f} GFLOP (fit + score + refit) -> "
              f"{100 * row['fp64_share']:.2f} % of FP64 VALU peak; median inlier share "
              f"{row['median_inlier_share']:.3f}", flush=True)
        res.append(row)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
