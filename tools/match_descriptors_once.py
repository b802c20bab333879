"""Descriptor matching, timed: sfm_match_descriptors (every pair in one call)
beside a plain torch baseline on the same data and device -- the descriptors
biased to int8 and held as fp16 on the device, then per pair one fp16 matmul,
the distances from it and topk(2, largest=False) per row (and the column argmin
the cross-check needs, timed separately).  The baseline materialises every
N_i x N_j matrix; it is approximate (fp16) and only its time is used.  It runs
in a child process of its own (--baseline-only), after the library's calls:
torch brings its own HIP runtime and finds no device in a process where the
library's has already opened it.

Shape: 200 images x 8,192 keypoints x 128 bytes, every image against its 20
successors: 3,790 pairs.  Half of an image's keypoints are noisy views of a
common pool of scene descriptors, half uniform random.  Per round: the median
over --reps calls after a warm-up of the whole call (host clock) and of upload,
kernels and download (HIP events, sfm_last_timings, in calls of their own).
The i8 MFMA throughput is 2 * sum(N_i N_j) * dim operations (twice that with
the reverse pass of the cross-check, reported as issued) per kernel second,
beside the dense i8 peak: the micro-architecture guide's matrix-core table
gives "I8 | 32x32x32 / 16x16x64: the cycles of the BF16 form of the same MxN at
2x the K, so 2x BF16 per clock" and BF16 as ~2.5 PF dense, so ~5 POPS.

    python tools/match_descriptors_once.py [--images 200] [--keypoints 8192] [--dim 128] [--successors 20] [--rounds 3] [--reps 3] [--no-cross-check] [--no-baseline] [--baseline-only] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "structure-from-motion-_amd"))

I8_PEAK_OPS = 5.0e15  # 2 x the ~2.5 PF dense BF16 peak


def scene(n_images, n_kp, dim, seed=3):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (4 * n_kp, dim), dtype=np.uint8)
    desc = rng.integers(0, 256, (n_images * n_kp, dim), dtype=np.uint8)
    half = n_kp // 2
    for k in range(n_images):
        seen = rng.choice(len(pool), half, replace=False)
        noisy = pool[seen].astype(np.int16) + rng.integers(-2, 3, (half, dim), dtype=np.int16)
        desc[k * n_kp:k * n_kp + half] = np.clip(noisy, 0, 255).astype(np.uint8)
    return desc, np.arange(n_images + 1, dtype=np.int64) * n_kp


def torch_baseline(desc, img_start, pairs):
    """seconds of (matmul + topk(2)) and of (the same + the column argmin) over all pairs; the data is on the
    device before the clock starts"""
    import torch
    dev = torch.device("cuda")
    d8 = torch.from_numpy((desc.astype(np.int16) - 128).astype(np.int8)).to(dev)
    d16 = d8.half() / 16  # exact; keeps every product sum inside fp16's range
    norm = (d16.float() ** 2).sum(1).half()
    st = img_start.tolist()
    out = []
    for with_columns in (False, True):
        for p in range(min(3, len(pairs))):  # warm-up
            i, j = pairs[p]
            (norm[st[j]:st[j + 1]][None, :] - 2 * (d16[st[i]:st[i + 1]] @ d16[st[j]:st[j + 1]].T)).topk(2, dim=1, largest=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, j in pairs:
            w = norm[st[j]:st[j + 1]][None, :] - 2 * (d16[st[i]:st[i + 1]] @ d16[st[j]:st[j + 1]].T)
            w.topk(2, dim=1, largest=False)
            if with_columns:
                (w + norm[st[i]:st[i + 1]][:, None]).argmin(dim=0)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--keypoints", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--successors", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cross-check", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    desc, img_start = scene(a.images, a.keypoints, a.dim)
    pairs = np.array([(i, j) for i in range(a.images) for j in range(i + 1, min(i + 1 + a.successors, a.images))],
                     dtype=np.int32)
    if a.baseline_only:
        print(json.dumps(torch_baseline(desc, img_start, pairs.tolist())))
        return
    import _sfmcore as core
    core.require_device()
    cross = not a.no_cross_check
    n = np.diff(img_start)
    products = int((n[pairs[:, 0]] * n[pairs[:, 1]]).sum())
    ops = 2 * products * a.dim * (2 if cross else 1)  # the reverse pass computes every product again

    def call():
        return core.match_descriptors(desc, img_start, pairs, 0.8, core.INT32_MAX, cross)

    def timings():
        call()
        return core.last_timings()

    out = call()
    row = dict(images=a.images, keypoints=a.keypoints, dim=a.dim, pairs=len(pairs), cross_check=cross,
               matches=int(out["match_start"][-1]), distance_products=products, i8_ops_issued=ops, rounds=[])
    print(json.dumps({k: v for k, v in row.items() if k != "rounds"}), flush=True)
    for _ in range(a.rounds):
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
        whole = float(np.median(t))
        core.set_call_timing(True)
        k = np.median(np.array([timings() for _ in range(a.reps)]), axis=0)
        core.set_call_timing(False)
        rate = ops / (k[1] * 1e-3)
        row["rounds"].append(dict(call_ms=whole, upload_ms=float(k[0]), kernels_ms=float(k[1]), download_ms=float(k[2]),
                                  i8_ops_per_s=rate, i8_peak_fraction=rate / I8_PEAK_OPS))
        print(f"call {whole:.1f} ms; sfm_last_timings: upload {k[0]:.1f}, kernels {k[1]:.1f}, download {k[2]:.1f} ms; "
              f"i8 MFMA {rate / 1e12:.0f} TOPS = {100 * rate / I8_PEAK_OPS:.1f} % of ~5 POPS dense", flush=True)
    if not a.no_baseline:
        import subprocess
        shape = ["--images", a.images, "--keypoints", a.keypoints, "--dim", a.dim, "--successors", a.successors]
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only"] + [str(v) for v in shape],
                               capture_output=True, text=True, check=True)
        fwd, both = json.loads(child.stdout.strip().splitlines()[-1])
        row["torch_matmul_topk2_ms"], row["torch_with_column_argmin_ms"] = fwd * 1e3, both * 1e3
        print(f"torch fp16 matmul + topk(2) per pair: {fwd * 1e3:.0f} ms; with the column argmin: {both * 1e3:.0f} ms",
              flush=True)
    print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
