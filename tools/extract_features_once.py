"""Feature extraction, timed: sfm_extract_features on synthetic textured images
in one call with max_keypoints=8192.  Prints the keypoint counts and, per round,
the median over --reps calls after a warm-up of the whole call (host clock) and
of upload, kernels and download (HIP events, sfm_last_timings, in calls of their
own).  The blur kernels must move, per image, every layer read once and written
once: 4 bytes x 2 x the floats of the pyramid (the first layer reads bytes); the
script states that figure over the time of the pyramid kernels alone, the
fourth entry of sfm_last_timings.

    python tools/extract_features_once.py [--images 200] [--height 1200] [--width 1600] [--max-keypoints 8192] [--rounds 3] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "structure-from-motion-_amd"))


def textures(n, H, W, seed=5):
    """smooth random textures: a few base fields of random blobs at several scales, mixed per image"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, H, W), dtype=np.uint8)
    fields = []
    for s in (1.5, 3.0, 6.0, 12.0):
        f = rng.standard_normal((H, W)).astype(np.float32)
        k = np.exp(-np.arange(-int(4 * s), int(4 * s) + 1) ** 2 / (2 * s * s)).astype(np.float32)
        k /= k.sum()
        f = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, f)
        f = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, f)
        fields.append(f / f.std())
    for i in range(n):
        img = sum(w * np.roll(f, (int(rng.integers(H)), int(rng.integers(W))), axis=(0, 1))
                  for w, f in zip(rng.uniform(0.5, 1.5, len(fields)), fields))
        img = (img - img.min()) / (img.max() - img.min())
        out[i] = np.floor(img * 255.0 + 0.5).astype(np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--max-keypoints", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import _sfmcore as core
    core.require_device()
    images = textures(a.images, a.height, a.width)
    per_image, h, w = 0, a.height, a.width
    for _ in range(core.extract_octaves(a.height, a.width)):
        per_image += 6 * h * w
        h, w = (h + 1) // 2, (w + 1) // 2
    blur_bytes = a.images * (2 * 4 * per_image)

    def call():
        return core.extract_features(images, max_keypoints=a.max_keypoints)

    def timings():
        call()
        return core.last_timings()

    out = call()
    counts = np.diff(out["kp_start"])
    row = dict(images=a.images, height=a.height, width=a.width, max_keypoints=a.max_keypoints,
               keypoints=int(counts.sum()), keypoints_min=int(counts.min()), keypoints_max=int(counts.max()),
               pyramid_floats_per_image=per_image, blur_bytes=blur_bytes, rounds=[])
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
        rate = blur_bytes / (k[3] * 1e-3)
        row["rounds"].append(dict(call_ms=whole, upload_ms=float(k[0]), kernels_ms=float(k[1]), download_ms=float(k[2]),
                                  pyramid_ms=float(k[3]), pyramid_bytes_per_s=rate))
        print(f"call {whole:.1f} ms; sfm_last_timings: upload {k[0]:.1f}, kernels {k[1]:.1f}, download {k[2]:.1f}, "
              f"pyramid kernels alone {k[3]:.1f} ms: {blur_bytes / 1e9:.1f} GB in that time is {rate / 1e9:.0f} GB/s",
              flush=True)
    print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
