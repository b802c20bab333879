"""Multi-view track triangulation, timed: sfm_triangulate_tracks (linear then
refined, all views) against the only route to a point per track that the
two-view entry points give -- the reference's registration loop
(Wrapper_dev.py:262-291): for every image, every earlier image, one
sfm_triangulate_dlt and one sfm_triangulate_nonlinear on the features the
pair shares (pairs sharing fewer than 8 are skipped, as there), the later
pair's points overwriting the earlier's.

Per problem (cfg4: 100k x 10 views over 50 cameras, staged in LDS; cfg5:
500k x 8 over 200, read from global memory) and per round: the median over
--reps calls after a warm-up of the whole call (host clock around a call that
ends in a stream synchronise), of the kernel alone (HIP events around the
launch, from sfm_last_timings, in calls of their own), and of the pair loop
(--loop-reps passes; the pairs' index lists and coordinate arrays are built
outside the timed region).  The kernel's share of peak uses a flop model
from the shapes (below) with --evals cost evaluations per track ASSUMED, and
the bytes the kernel must move.

    python tools/multiview_once.py [--cfg cfg4 cfg5] [--rounds 3] [--reps 20] [--loop-reps 20] [--out FILE]
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
HBM_PEAK = 8.0e12    # B/s


def flop_model(n_tracks, n_obs, evals):
    """Linear stage: per observation 16 flops for the two rows and 2 x 60 for
    their Givens rotations; per track ~6 Jacobi sweeps of 6 column pairs at
    ~72 flops.  Refinement: per observation and evaluation 81 flops (h 18,
    residuals and cost 8, Jacobian rows 19, J^T J and J^T r 36), per
    evaluation ~60 for the 3 x 3 solve and the stop tests."""
    return n_obs * 136 + n_tracks * 6 * 6 * 72 + evals * (n_obs * 81 + n_tracks * 60)


def byte_model(n_tracks, n_obs):
    return n_obs * 20 + n_tracks * (8 + 24 + 8 + 4 + 1)


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def pair_lists(p, P):
    """(P_a, P_b, x_a, x_b, rows) per image pair a < b in the loop's order"""
    n_cams, k = p["n_cams"], p["k"]
    cam = p["cam_idx"].reshape(-1, k)
    obs = p["obs"].reshape(-1, k, 2)
    slot = np.full((n_cams, len(cam)), -1, dtype=np.int8)  # camera-major: a pair reads two contiguous rows
    slot[cam, np.arange(len(cam))[:, None]] = np.arange(k, dtype=np.int8)
    seen = slot >= 0
    out = []
    for b in range(1, n_cams):
        for a in range(b):
            rows = np.where(seen[a] & seen[b])[0]
            if len(rows) < 8:
                continue
            out.append((P[a], P[b], np.ascontiguousarray(obs[rows, slot[a, rows]]),
                        np.ascontiguousarray(obs[rows, slot[b, rows]]), rows))
    return out


def pair_loop(pairs, X):
    for Pa, Pb, xa, xb, rows in pairs:
        X0 = core.triangulate(Pa, Pb, xa, xb)
        X[rows] = core.triangulate_nonlinear(Pa, Pb, xa, xb, X0)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", nargs="+", default=["cfg4", "cfg5"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=20)
    ap.add_argument("--evals", type=float, default=5.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    res = []
    for cfg in a.cfg:
        p = syn.ba_problem_cfg(cfg, dense=False)
        T, k, n_obs = p["n_pts"], p["k"], len(p["cam_idx"])
        P = np.stack([projection(syn.K_REF, C, R) for C, R in zip(p["C_true"], p["R_true"])])
        start = np.arange(T + 1, dtype=np.int64) * k
        cam, xy = p["cam_idx"].astype(np.int32), p["obs"]
        pairs = pair_lists(p, P)
        Xloop = np.full((T, 3), np.nan)

        def call():
            return core.triangulate_tracks(P, start, cam, xy)

        def kernel():
            call()
            return core.last_timings()[1]

        X, cost, front, info = call()
        pair_loop(pairs, Xloop)
        err_all = np.linalg.norm(X - p["X_true"], axis=1)
        err_loop = np.linalg.norm(Xloop - p["X_true"], axis=1)
        row = dict(cfg=cfg, tracks=T, views=k, n_cams=p["n_cams"], pairs=len(pairs),
                   pair_calls=2 * len(pairs), info_counts=np.bincount(info + 2, minlength=8).tolist(),
                   front=int(front.sum()), median_err_all_views=float(np.median(err_all)),
                   median_err_last_pair=float(np.nanmedian(err_loop)), rounds=[])
        flops, nbytes = flop_model(T, n_obs, a.evals), byte_model(T, n_obs)
        for _ in range(a.rounds):
            whole = median_ms(call, a.reps)
            core.set_call_timing(True)
            kern = float(np.median([kernel() for _ in range(a.reps + 1)][1:]))
            core.set_call_timing(False)
            loop = median_ms(lambda: pair_loop(pairs, Xloop), a.loop_reps)
            row["rounds"].append(dict(call_ms=whole, kernel_ms=kern, pair_loop_ms=loop))
            print(f"{cfg}: call {whole:.3f} ms, kernel {kern:.3f} ms, pair loop ({len(pairs)} pairs) {loop:.1f} ms",
                  flush=True)
        kern = float(np.median([r["kernel_ms"] for r in row["rounds"]])) * 1e-3
        row.update(model_flops=flops, model_bytes=nbytes, evals_assumed=a.evals,
                   fp64_share=flops / FP64_PEAK / kern, hbm_share=nbytes / HBM_PEAK / kern)
        print(f"{cfg}: model {flops / 1e9:.2f} GFLOP ({a.evals:g} evaluations per track assumed) -> "
              f"{100 * row['fp64_share']:.2f} % of FP64 VALU peak; {nbytes / 1e6:.1f} MB -> "
              f"{100 * row['hbm_share']:.2f} % of HBM peak; median |X - X_true|: all views "
              f"{row['median_err_all_views']:.4f}, last pair {row['median_err_last_pair']:.4f}", flush=True)
        res.append(row)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
