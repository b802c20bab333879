"""Batched calibrated pair verification, timed: sfm_essential_pairs beside
sfm_verify_pairs at the same shapes, on the same scene and in the same session
(tools/verify_pairs_once.py: "p3" 10 pairs x 500 correspondences, "full" 4,950 x
2,000; a quarter of the matches wrong).  Per shape and round: the median over
--reps calls after a warm-up of the whole call (host clock around a call that
ends in a stream synchronise) and of the kernels (HIP events, sfm_last_timings,
in calls of their own), for both entry points.

    python tools/essential_pairs_once.py [--shape p3 full] [--H 256] [--rounds 3] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from verify_pairs_once import K, SHAPES, core, median_ms, scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=["p3", "full"])
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threshold", type=float, default=2.5)
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    res = []
    for name in a.shape:
        P, n = SHAPES[name]
        ps, x1, x2, good = scene(P, n)
        s5 = core.essential_samples(np.diff(ps), a.H, 0)
        s8 = core.pair_samples(np.diff(ps), a.H, 0)
        calls = dict(essential=lambda: core.essential_pairs(K, ps, x1, x2, s5, threshold=a.threshold),
                     verify=lambda: core.verify_pairs(ps, x1, x2, s8, threshold=a.threshold))
        out = calls["essential"]()
        row = dict(shape=name, pairs=P, correspondences=n, H=a.H, info_counts=np.bincount(out[6] + 4).tolist(),
                   median_inlier_share=float(np.median(out[2] / n)),
                   masks_equal_truth=int(sum(np.array_equal(out[3][ps[p]:ps[p + 1]], good[ps[p]:ps[p + 1]])
                                             for p in range(P))), rounds=[])
        for _ in range(a.rounds):
            r = {}
            for which, call in calls.items():
                whole = median_ms(call, a.reps)
                core.set_call_timing(True)
                t = []
                for _ in range(a.reps + 1):
                    call()
                    t.append(core.last_timings()[:4])
                core.set_call_timing(False)
                k = np.median(np.array(t[1:]), axis=0)
                r[which] = dict(call_ms=whole, upload_ms=float(k[0]), kernels_ms=float(k[1]), download_ms=float(k[2]),
                                fit_score_ms=float(k[3]))
                print(f"{name} {which}: call {whole:.3f} ms, upload {k[0]:.3f}, kernels {k[1]:.3f} (fit and score "
                      f"{k[3]:.3f}), download {k[2]:.3f}", flush=True)
            row["rounds"].append(r)
        print(f"{name}: median inlier share {row['median_inlier_share']:.3f}; masks equal to the truth "
              f"{row['masks_equal_truth']} of {P}; info {row['info_counts']}", flush=True)
        res.append(row)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
