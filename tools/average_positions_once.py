"""Global position averaging, timed: sfm_average_positions (every camera's
centre from all pairs in one call) on both of its paths, against the numpy
restatement of the same rounds (tests/test_position_averaging.py) on the same
host: the dense solve where it fits, two rounds of the numpy PCG where it does
not (the device is then compared with it at two rounds as well).

Shapes: 200 images x 4,950 pairs and 10,000 images x about 500,000 pairs,
cameras in a box, 1 degree of direction noise and 10 % uniformly random
directions.  Per shape and path: the median over --reps calls after a warm-up
of the whole call (host clock around a call that ends in a stream synchronise)
and of sfm_last_timings' split (HIP events, in calls of their own): upload,
kernels, download and the CG iterations alone; the CG iterations per round.
The restatement runs once per shape.

    python tools/average_positions_once.py [--reps 5] [--skip-large] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "structure-from-motion-_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import _sfmcore as core  # noqa: E402
import test_position_averaging as pa  # noqa: E402


def graph(N, E, seed):
    """N cameras in a box, E distinct random pairs, 1 degree of noise, 10 % wrong"""
    rng = np.random.default_rng(seed)
    side = 10.0 * (N / 30.0) ** (1.0 / 3.0)
    centres = rng.uniform(0, 1, (N, 3)) * [side, side, side / 5.0]
    i = rng.integers(0, N, 2 * E + 1000)
    j = rng.integers(0, N, 2 * E + 1000)
    ok = i != j
    lo, hi = np.minimum(i[ok], j[ok]), np.maximum(i[ok], j[ok])
    _, first = np.unique(lo.astype(np.int64) * N + hi, return_index=True)
    first = np.sort(first)[:E]
    ij = np.column_stack([i[ok][first], j[ok][first]]).astype(np.int32)
    wrong = rng.random(len(ij)) < 0.10
    return ij, pa.measure(centres, ij, 1.0, wrong, rng), centres, ~wrong


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    rows = []
    for N, E in [(200, 4950)] + ([] if a.skip_large else [(10000, 500000)]):
        ij, d, centres, clean = graph(N, E, 3)
        solver = "dense" if N <= 2000 else "pcg"
        # the numpy PCG scatters with np.add.at, seconds an iteration at 500,000 pairs: two rounds of it
        ref_args = dict(pa.DEFAULTS, rounds=pa.DEFAULTS["rounds"] if solver == "dense" else 2)
        t0 = time.perf_counter()
        ref = pa.restate(N, ij, d, solver=solver, **ref_args)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        for path in ([1, 2] if N <= core.POSITIONS_PATH1_MAX_NODES else [2]):
            def call():
                return core.average_positions(N, ij, d, path=path, **pa.DEFAULTS)

            def timings():
                call()
                return core.last_timings()

            out = dict(zip(pa.OUTPUTS, call()))
            same = dict(zip(pa.OUTPUTS, core.average_positions(N, ij, d, path=path, **ref_args)))
            whole = median_ms(call, a.reps)
            core.set_call_timing(True)
            k = np.median(np.array([timings() for _ in range(a.reps + 1)][1:]), axis=0)
            core.set_call_timing(False)
            s = out["info"] >= 0
            row = dict(images=N, pairs=len(ij), path=path, solved=out["n_solved"], call_ms=whole, upload_ms=float(k[0]),
                       kernels_ms=float(k[1]), download_ms=float(k[2]), cg_ms=float(k[3]),
                       cg_iters=out["cg_iters"].tolist(), cg_residual_max=float(out["cg_residual"].max()),
                       numpy_solver=solver, numpy_rounds=ref_args["rounds"], numpy_ms=numpy_ms,
                       gap_to_numpy=float(pa.gaps(same, ref)),
                       mask_differs_from_clean=int((out["edge_inlier"] != clean).sum()),
                       mask_differs_from_numpy=int((same["edge_inlier"] != ref["edge_inlier"]).sum()),
                       worst_camera=pa.align(out["C"][s], centres[s]))
            rows.append(row)
            print(f"{N} images x {len(ij)} pairs, path {path}: call {whole:.2f} ms; sfm_last_timings: upload {k[0]:.2f}, "
                  f"kernels {k[1]:.2f} (CG {k[3]:.2f}), download {k[2]:.2f} ms; CG iterations {row['cg_iters']}; numpy "
                  f"({solver}, {ref_args['rounds']} rounds) {numpy_ms:.0f} ms, gap to it {row['gap_to_numpy']:.2e}; mask differs from the clean edges "
                  f"on {row['mask_differs_from_clean']}; worst camera {row['worst_camera']:.3g}", flush=True)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
