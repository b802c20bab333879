"""Global rotation averaging, timed: sfm_average_rotations (every camera's
rotation from all pairs in one call) against the vectorised numpy restatement
of the same three stages (tests/test_rotation_averaging.py) on the same host.
The restatement is the only other implementation there is; it is a time to set
beside the call's and, at tol = 0, the same result.

Shapes: 200 images x 4,950 pairs (a quarter of all pairs of 200, what 100
images' worth of verified pairs gives) and 10,000 images x about 500,000 pairs
(every image with about 100 neighbours), 30 % wrong edges and 1 degree of noise.
Per shape: the median over --reps calls after a warm-up of the whole call (host
clock around a call that ends in a stream synchronise) and of sfm_last_timings'
split (HIP events, in calls of their own): upload, kernels, download and the
consensus kernels alone.  The restatement runs once per shape.

--refit cg times the Gauss-Newton CG refit at its defaults (rounds 10, tol
1e-9, cg_tol 1e-10, cg_max_iters 500) and reports its rounds, CG iterations
and steps; sfm_last_timings' fourth slot is then the CG launches alone, and
the numpy restatement is left out (tests/test_rotation_cg.py holds it).
--refit jacobi with --max-sweeps 200 --tol 1e-9 is the Jacobi refit at its
defaults.  Both report the largest and the median angle of the result to the
truth in the root's gauge.

    python tools/average_rotations_once.py [--reps 5] [--refit jacobi|cg] [--max-sweeps 30] [--tol 0]
                                           [--skip-large] [--skip-numpy] [--out FILE]
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
import test_rotation_averaging as ra  # noqa: E402


def graph(N, E, seed):
    """N images, E distinct random pairs, 1 degree of noise, 30 % wrong"""
    rng = np.random.default_rng(seed)
    R_true = ra.random_rotations(rng, N)
    i = rng.integers(0, N, 2 * E + 1000)
    j = rng.integers(0, N, 2 * E + 1000)
    ok = i != j
    lo, hi = np.minimum(i[ok], j[ok]), np.maximum(i[ok], j[ok])
    _, first = np.unique(lo.astype(np.int64) * N + hi, return_index=True)
    first = np.sort(first)[:E]
    ij = np.column_stack([i[ok][first], j[ok][first]]).astype(np.int32)
    wrong = rng.random(len(ij)) < 0.3
    R_rel, clean = ra.measure(R_true, ij, 1.0, wrong, rng)
    return ij, R_rel, R_true, clean


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
    ap.add_argument("--max-sweeps", type=int, default=30)
    ap.add_argument("--tol", type=float, default=0.0, help="the Jacobi refit's tol")
    ap.add_argument("--refit", choices=("jacobi", "cg"), default="jacobi")
    ap.add_argument("--skip-numpy", action="store_true", help="leave out the numpy restatement of the Jacobi refit")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    rows = []
    for N, E in [(200, 4950)] + ([] if a.skip_large else [(10000, 500000)]):
        ij, R_rel, R_true, clean = graph(N, E, 3)
        cg = a.refit == "cg"
        args = dict(seed=1, consensus_sweeps=3, refit="cg") if cg else \
            dict(seed=1, consensus_sweeps=3, max_sweeps=a.max_sweeps, tol=a.tol)

        def call():
            return core.average_rotations(N, ij, R_rel, **args)

        def timings():
            call()
            return core.last_timings()

        out = call()
        whole = median_ms(call, a.reps)
        core.set_call_timing(True)
        k = np.median(np.array([timings() for _ in range(a.reps + 1)][1:]), axis=0)
        core.set_call_timing(False)
        err = np.rad2deg(ra.angle_between(out[0], ra.to_root_gauge(R_true, N, ij)))
        # a random "wrong" rotation lands within the threshold of the truth with probability 3.5e-5
        truth = R_true[ij[:, 1]] @ np.swapaxes(R_true[ij[:, 0]], 1, 2)
        chance = int((ra.angle_between(R_rel[~clean], truth[~clean]) < np.deg2rad(5)).sum())
        row = dict(images=N, pairs=len(ij), refit=a.refit, max_degree=int(np.bincount(ij.ravel()).max()),
                   levels=int(out[6].max()), refit_sweeps=out[7], call_ms=whole, upload_ms=float(k[0]),
                   kernels_ms=float(k[1]), download_ms=float(k[2]), mask_differs_from_clean=int((out[2] != clean).sum()),
                   wrong_within_threshold=chance, worst_node_deg=float(err.max()), median_node_deg=float(np.median(err)))
        if cg:
            n = out[7]
            row.update(cg_ms=float(k[3]), cg_iters=out[8][:n].tolist(), cg_residual=out[9][:n].tolist(),
                       step=out[10][:n].tolist())
            fourth = f"CG launches {k[3]:.2f}"
        else:
            row.update(consensus_ms=float(k[3]))
            fourth = f"consensus {k[3]:.2f}"
        numpy_ms = None
        if not cg and not a.skip_numpy:
            t0 = time.perf_counter()
            ref = ra.restate(N, ij, R_rel, **args)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            row.update(numpy_ms=numpy_ms,
                       same_integers_as_numpy=bool(all(np.array_equal(out[ra.OUTPUTS.index(n)], ref[n])
                                                       for n in ra.INTEGER_OUTPUTS)),
                       max_R_difference=float(np.abs(out[0] - ref["R"]).max()), numpy_margin=ref["margin"])
        rows.append(row)
        print(f"{N} images x {len(ij)} pairs, refit {a.refit}: call {whole:.2f} ms; sfm_last_timings: upload {k[0]:.2f}, "
              f"kernels {k[1]:.2f} ({fourth}), download {k[2]:.2f} ms; "
              + (f"numpy restatement {numpy_ms:.0f} ms; " if numpy_ms is not None else "")
              + f"refit sweeps or rounds {out[7]}"
              + (f", CG iterations {row['cg_iters']}, steps {['%.2g' % x for x in row['step']]}" if cg else "")
              + f"; mask differs from the clean edges on {row['mask_differs_from_clean']} ({chance} wrong edges lie "
              f"within the threshold of the truth by chance), worst node {err.max():.3f} deg, median "
              f"{np.median(err):.3f} deg", flush=True)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
