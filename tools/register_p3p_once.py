"""Calibrated batched view registration, timed: sfm_register_views_p3p against
sfm_register_views on the same scenes in the same session, at the same H and
at the H that gives each sampler the same confidence (99 % of one clean sample
at 30 % outliers: 37 six-point samples, 11 three-point samples).

Shapes and scene are tools/register_once.py's: "p3" 4 views x 500
correspondences and "cfg5" 198 views x 20,000; 30 % of the observations
displaced by 40-120 px, 0.5 px noise on the rest.  Per shape, H and round: the
median over --reps calls after a warm-up of the whole call (host clock around a
call that ends in a stream synchronise) and of the kernels (HIP events,
sfm_last_timings, in calls of their own).

    python tools/register_p3p_once.py [--shape p3 cfg5] [--H 256] [--rounds 3] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "structure-from-motion-_amd"))
sys.path.insert(0, os.path.dirname(__file__))
import _sfmcore as core  # noqa: E402
from register_once import K, SHAPES, median_ms, scene  # noqa: E402

EQUAL_CONFIDENCE = {"dlt6": 37, "p3p": 11}


def measure(name, fn, reps, rounds):
    out = fn()
    rows = []
    for _ in range(rounds):
        whole = median_ms(fn, reps)
        core.set_call_timing(True)
        try:
            ks = []
            for _ in range(reps + 1):
                fn()
                ks.append(core.last_timings()[[1, 3]])
        finally:
            core.set_call_timing(False)
        k = np.median(np.array(ks[1:]), axis=0)
        rows.append(dict(call_ms=whole, kernels_ms=float(k[0]), fit_score_ms=float(k[1])))
        print(f"{name}: call {whole:.3f} ms, kernels {k[0]:.3f} ms (fit and score {k[1]:.3f})", flush=True)
    return out, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=["p3", "cfg5"])
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threshold", type=float, default=4.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    res = []
    for shape in a.shape:
        V, n = SHAPES[shape]
        X, vs, pt, xy = scene(V, n)
        for label, H6, H3 in (("same H", a.H, a.H), ("equal confidence", EQUAL_CONFIDENCE["dlt6"],
                                                   EQUAL_CONFIDENCE["p3p"])):
            s6 = core.register_samples(np.diff(vs), H6, 0)
            s3 = core.p3p_samples(np.diff(vs), H3, 0)
            o6, r6 = measure(f"{shape} {label} dlt6 H {H6}",
                             lambda: core.register_views(K, X, vs, pt, xy, s6, threshold=a.threshold), a.reps, a.rounds)
            o3, r3 = measure(f"{shape} {label} p3p H {H3}",
                             lambda: core.register_views_p3p(K, X, vs, pt, xy, s3, threshold=a.threshold), a.reps,
                             a.rounds)
            n_sol = core.register_views_p3p(K, X, vs, pt, xy, s3, threshold=a.threshold, want_counts=True)[8]
            row = dict(shape=shape, views=V, correspondences=n, setting=label, H_dlt6=H6, H_p3p=H3, dlt6=r6, p3p=r3,
                       mean_n_sol=float(n_sol.mean()),
                       registered=dict(dlt6=int((o6[7] >= 1).sum()), p3p=int((o3[7] >= 1).sum())),
                       median_inlier_share=dict(dlt6=float(np.median(o6[3] / n)), p3p=float(np.median(o3[3] / n))))
            print(f"{shape} {label}: mean n_sol {row['mean_n_sol']:.2f}, registered {row['registered']}, median "
                  f"inlier share {row['median_inlier_share']}", flush=True)
            res.append(row)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
