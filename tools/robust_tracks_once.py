"""Robust track triangulation, timed: sfm_triangulate_tracks_robust against
sfm_triangulate_tracks on the same tracks -- the non-robust floor: one fit,
no hypotheses -- with one observation of every track displaced by 40-120 px.

Per problem (cfg4-shaped: 100k x 10 views over 50 cameras, staged in LDS;
cfg5-shaped: 500k x 8 over 200, read from global memory) and per round: the
median over --reps calls after a warm-up of the whole call (host clock around
a call that ends in a stream synchronise) and of the kernel alone (HIP events
around the launch, from sfm_last_timings, in calls of their own), for the
robust call at the lanes per track the library chooses and at each of
--lanes, and for the plain call.  The kernel's share of peak uses a flop
model from the shapes (below) with --evals cost evaluations per refit
ASSUMED.  Also printed: the median and the largest |X - X_true| of both calls
on the contaminated tracks, and how many masks equal the truth.

    python tools/robust_tracks_once.py [--cfg cfg4 cfg5] [--rounds 3] [--reps 20] [--lanes 1 4 8] [--out FILE]
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
from sfm_two_view import projection  # noqa: E402

FP64_PEAK = 78.6e12  # MI355X vector FP64, flop/s


def flop_model(n_tracks, views, inliers, max_pairs, evals):
    """Per hypothesis: the two-view DLT, ~2,600 flops (32 for the rows, ~7
    Jacobi sweeps of 6 column pairs at ~60), and 32 per observation scored
    (h 18, two divisions, error 5, compare and add).  Per track: two more
    scores (the winner's mask, the re-score), and the refit of the inliers
    as tools/multiview_once.py models it."""
    pairs = min(views * (views - 1) // 2, max_pairs)
    hyp = pairs * (2600 + 32 * views) + 2 * 32 * views
    refit = inliers * 136 + 6 * 6 * 72 + evals * (inliers * 81 + 60)
    return n_tracks * (hyp + refit), n_tracks * refit


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def kernel_ms(fn, reps):
    core.set_call_timing(True)
    t = []
    for _ in range(reps + 1):
        fn()
        t.append(core.last_timings()[1])
    core.set_call_timing(False)
    return float(np.median(t[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", nargs="+", default=["cfg4", "cfg5"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lanes", type=int, nargs="*", default=[])
    ap.add_argument("--evals", type=float, default=5.0)
    ap.add_argument("--threshold", type=float, default=4.0)
    ap.add_argument("--max-pairs", type=int, default=120)
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    res = []
    for cfg in a.cfg:
        p = syn.ba_problem_cfg(cfg, dense=False)
        T, k = p["n_pts"], p["k"]
        P = np.stack([projection(syn.K_REF, C, R) for C, R in zip(p["C_true"], p["R_true"])])
        start = np.arange(T + 1, dtype=np.int64) * k
        cam = p["cam_idx"].astype(np.int32)
        rng = np.random.default_rng(7)
        bad = rng.integers(0, k, T) + np.arange(T) * k  # one displaced observation per track
        mag, ang = rng.uniform(40.0, 120.0, T), rng.uniform(0.0, 2.0 * np.pi, T)
        xy = p["obs"].copy()
        xy[bad] += np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
        truth = np.ones(T * k, dtype=bool)
        truth[bad] = False

        def robust(lanes=0):
            return core.triangulate_tracks_robust(P, start, cam, xy, threshold=a.threshold, max_pairs=a.max_pairs,
                                                  min_inliers=3, centres=p["C_true"], lanes_per_track=lanes)

        def plain():
            return core.triangulate_tracks(P, start, cam, xy)

        out = robust()
        Xp = plain()[0]
        for lanes in a.lanes:
            o = robust(lanes)
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(o, out)), lanes
        err_r = np.linalg.norm(out[0] - p["X_true"], axis=1)
        err_p = np.linalg.norm(Xp - p["X_true"], axis=1)
        exact = int((out[3] == truth).reshape(T, k).all(1).sum())
        flops, refit_flops = flop_model(T, k, k - 1, a.max_pairs, a.evals)
        row = dict(cfg=cfg, tracks=T, views=k, n_cams=p["n_cams"], masks_equal_truth=exact,
                   info_counts=np.bincount(out[6] + 3, minlength=9).tolist(),
                   err_robust_median=float(np.median(err_r)), err_robust_max=float(err_r.max()),
                   err_plain_median=float(np.median(err_p)), err_plain_max=float(err_p.max()),
                   model_flops=flops, model_refit_flops=refit_flops, evals_assumed=a.evals, rounds=[])
        print(f"{cfg}: {exact} of {T} masks equal the truth; |X - X_true| median / max: robust "
              f"{row['err_robust_median']:.4f} / {row['err_robust_max']:.4f}, plain {row['err_plain_median']:.4f} / "
              f"{row['err_plain_max']:.4f}", flush=True)
        for _ in range(a.rounds):
            r = dict(plain_call_ms=median_ms(plain, a.reps), plain_kernel_ms=kernel_ms(plain, a.reps))
            for lanes in [0] + list(a.lanes):
                r[f"robust_call_ms_lanes{lanes}"] = median_ms(lambda: robust(lanes), a.reps)
                r[f"robust_kernel_ms_lanes{lanes}"] = kernel_ms(lambda: robust(lanes), a.reps)
            row["rounds"].append(r)
            print(f"{cfg}: " + ", ".join(f"{key} {v:.3f}" for key, v in r.items()), flush=True)
        kern = float(np.median([r["robust_kernel_ms_lanes0"] for r in row["rounds"]])) * 1e-3
        kplain = float(np.median([r["plain_kernel_ms"] for r in row["rounds"]])) * 1e-3
        row.update(fp64_share=flops / FP64_PEAK / kern, kernel_ratio=kern / kplain)
        print(f"{cfg}: model {flops / 1e9:.2f} GFLOP ({a.evals:g} evaluations per refit assumed) -> "
              f"{100 * row['fp64_share']:.2f} % of FP64 VALU peak; robust / plain kernel time {row['kernel_ratio']:.1f}",
              flush=True)
        res.append(row)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
