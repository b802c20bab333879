"""Guided descriptor matching, timed beside the unguided call on the same data in
the same session: sfm_match_descriptors_guided and sfm_match_descriptors, every
pair in one call each.

Shape: that of tools/match_descriptors_once.py, 200 images x 8,192 keypoints x
128 bytes, every image against its 20 successors: 3,790 pairs.  The scene has
a known F per pair: cameras on a line, one baseline step per image, each turned
a little further about the vertical axis, in front of a pool of 4 x 8,192 scene
points with uniform random base descriptors.  Half of an image's keypoints are
the projections of randomly chosen pool points (4,000 x 3,000 pixel frame, focal
length 3,000; projections are not clipped to the frame) with the base
descriptor plus integer noise in [-2, 2]; half are uniform random positions with
uniform random descriptors.  F of the pair (i, j) follows from the two poses,
x_j^T F x_i = 0, scaled to unit Frobenius norm.
Per round: the median over --reps calls after a warm-up of the whole call (host
clock) and of upload, kernels and download (HIP events, sfm_last_timings, in
calls of their own), for both entry points, and the ratio of the kernel times.

    python tools/match_guided_once.py [--images 200] [--keypoints 8192] [--dim 128] [--successors 20] [--gate 4.0] [--rounds 3] [--reps 3] [--no-cross-check] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "structure-from-motion-_amd"))

K = np.array([[3000.0, 0.0, 2000.0], [0.0, 3000.0, 1500.0], [0.0, 0.0, 1.0]])


def pose(k):
    a = 0.002 * k
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return R, np.array([0.05 * k, 0.0, 0.0])


def fundamental(i, j):
    (Ri, Ci), (Rj, Cj) = pose(i), pose(j)
    R, t = Rj @ Ri.T, Rj @ (Ci - Cj)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return F / np.linalg.norm(F)


def scene(n_images, n_kp, dim, seed=3):
    rng = np.random.default_rng(seed)
    n_pool, half = 4 * n_kp, n_kp // 2
    X = np.column_stack([rng.uniform(-3, 3 + 0.05 * n_images, n_pool), rng.uniform(-2.5, 2.5, n_pool),
                         rng.uniform(5, 9, n_pool)])
    pool = rng.integers(0, 256, (n_pool, dim), dtype=np.uint8)
    desc = rng.integers(0, 256, (n_images * n_kp, dim), dtype=np.uint8)
    xy = rng.random((n_images * n_kp, 2)) * np.array([4000.0, 3000.0])
    for k in range(n_images):
        seen = rng.choice(n_pool, half, replace=False)
        noisy = pool[seen].astype(np.int16) + rng.integers(-2, 3, (half, dim), dtype=np.int16)
        desc[k * n_kp:k * n_kp + half] = np.clip(noisy, 0, 255).astype(np.uint8)
        R, C = pose(k)
        x = (K @ (R @ (X[seen] - C).T)).T
        xy[k * n_kp:k * n_kp + half] = x[:, :2] / x[:, 2:]
    return desc, xy, np.arange(n_images + 1, dtype=np.int64) * n_kp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--keypoints", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--successors", type=int, default=20)
    ap.add_argument("--gate", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cross-check", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    desc, xy, img_start = scene(a.images, a.keypoints, a.dim)
    pairs = np.array([(i, j) for i in range(a.images) for j in range(i + 1, min(i + 1 + a.successors, a.images))],
                     dtype=np.int32)
    F = np.array([fundamental(i, j) for i, j in pairs])
    import _sfmcore as core
    core.require_device()
    cross = not a.no_cross_check
    n = np.diff(img_start)
    products = int((n[pairs[:, 0]] * n[pairs[:, 1]]).sum())

    calls = dict(unguided=lambda: core.match_descriptors(desc, img_start, pairs, 0.8, core.INT32_MAX, cross),
                 guided=lambda: core.match_descriptors_guided(desc, xy, img_start, pairs, F, a.gate, 0.8,
                                                              core.INT32_MAX, cross))
    row = dict(images=a.images, keypoints=a.keypoints, dim=a.dim, pairs=len(pairs), cross_check=cross, gate=a.gate,
               distance_products=products, rounds=[])
    for name, call in calls.items():
        row[f"{name}_matches"] = int(call()["match_start"][-1])
    small = core.match_descriptors_guided(desc, xy, img_start, pairs[:4], F[:4], a.gate, 0.8, core.INT32_MAX, cross,
                                          want_diagnostics=True)
    row["candidates_per_keypoint_first_pairs"] = float(small["n_cand"].mean())
    print(json.dumps({k: v for k, v in row.items() if k != "rounds"}), flush=True)
    for _ in range(a.rounds):
        r = {}
        for name, call in calls.items():
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                t.append((time.perf_counter() - t0) * 1e3)
            core.set_call_timing(True)
            k = []
            for _ in range(a.reps):
                call()
                k.append(core.last_timings())
            core.set_call_timing(False)
            k = np.median(np.array(k), axis=0)
            r[name] = dict(call_ms=float(np.median(t)), upload_ms=float(k[0]), kernels_ms=float(k[1]),
                           download_ms=float(k[2]))
        r["guided_to_unguided_kernels"] = r["guided"]["kernels_ms"] / r["unguided"]["kernels_ms"]
        row["rounds"].append(r)
        print(f"kernels: unguided {r['unguided']['kernels_ms']:.1f} ms, guided {r['guided']['kernels_ms']:.1f} ms, "
              f"ratio {r['guided_to_unguided_kernels']:.2f}; calls {r['unguided']['call_ms']:.1f} / "
              f"{r['guided']['call_ms']:.1f} ms", flush=True)
    print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
