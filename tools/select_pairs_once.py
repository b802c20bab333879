"""Pair selection by retrieval, timed: sfm_vocab_train (training, and the
quantisation alone) and sfm_select_pairs, beside a plain torch baseline of the
retrieval on the same device -- the dense fp32 tf-idf matrix V (n_images x
n_words, built on the host from the same words), one V @ V.T, the cosine and
topk per row.  Only the baseline's time is used.  It runs in a child process of
its own (--baseline-only), after the library's calls: torch brings its own HIP
runtime and finds no device in a process where the library's has already
opened it.

Shape: 200 images x 8,192 keypoints x 128 bytes, 4,096 words, 10 iterations,
top_k 20; half of an image's keypoints are noisy views of a common pool of
scene descriptors, half uniform random (tools/match_descriptors_once.py's
scene).  Per round: the median over --reps calls after a warm-up of each whole
call (host clock) and of upload, kernels and download (HIP events,
sfm_last_timings, in calls of their own).  The i8 MFMA throughput of the
assignment is 2 n n_words dim operations per pass: for the quantisation over
its kernel time (norms, one pass and the tally), for the training (T + 1
passes, or T after an early stop) over its kernel time, which also holds the
sorts, the sums and the updates.  tools/match_descriptors_once.py reports the
matcher's rate on the same kernel.

    python tools/select_pairs_once.py [--images 200] [--keypoints 8192] [--dim 128] [--words 4096] [--iterations 10] [--top-k 20] [--rounds 3] [--reps 3] [--no-baseline] [--baseline-only FILE] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "structure-from-motion-_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

I8_PEAK_OPS = 5.0e15  # 2 x the ~2.5 PF dense BF16 peak


def torch_baseline(word, img_start, n_words, top_k, reps):
    """median seconds of V @ V.T, the cosine and topk; V is on the device before the clock starts"""
    import torch
    n = len(img_start) - 1
    h = np.zeros((n, n_words), dtype=np.float32)
    for i in range(n):
        h[i] = np.bincount(word[img_start[i]:img_start[i + 1]], minlength=n_words)
    df = (h > 0).sum(axis=0)
    q = np.floor(256.0 * np.log(n / np.maximum(df, 1)) + 0.5).astype(np.float32)
    V = torch.from_numpy(h * q[None, :]).to("cuda")
    t = []
    for r in range(reps + 2):  # two warm-up runs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G = V @ V.T
        norm = G.diagonal().clamp_min(1.0).sqrt()
        S = G / (norm[:, None] * norm[None, :])
        S.fill_diagonal_(-1.0)
        S.topk(min(top_k, n), dim=1)
        torch.cuda.synchronize()
        if r >= 2:
            t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--keypoints", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--words", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--top-k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-only", metavar="FILE", help="an .npz of word and img_start: time the baseline alone")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.baseline_only:
        z = np.load(a.baseline_only)
        print(json.dumps(torch_baseline(z["word"], z["img_start"], a.words, a.top_k, a.reps)))
        return
    from match_descriptors_once import scene
    import _sfmcore as core
    core.require_device()
    desc, img_start = scene(a.images, a.keypoints, a.dim)
    n = len(desc)
    first = np.sort(np.random.default_rng(0).choice(n, a.words, replace=False))
    c0 = desc[first]
    pass_ops = 2 * n * a.words * a.dim

    trained = core.vocab_train(desc, c0, a.iterations)
    centres, word, T = trained["centres"], trained["word"], trained["iterations"]
    inertia = trained["inertia"]
    passes = T if T > 0 and T < a.iterations and inertia[T] == inertia[T - 1] else T + 1  # no pass after an early stop
    sel = core.select_pairs(word, img_start, a.words, a.top_k)
    nb = sel["neighbour"]
    i, k = np.nonzero(nb >= 0)
    pairs = np.unique(np.stack([np.minimum(i, nb[i, k]), np.maximum(i, nb[i, k])], axis=1), axis=0)
    row = dict(images=a.images, keypoints=a.keypoints, dim=a.dim, words=a.words, max_iterations=a.iterations,
               iterations=T, assignment_passes=passes, inertia=[int(v) for v in trained["inertia"]],
               empty_clusters=int((trained["count"] == 0).sum()), top_k=a.top_k, pairs=len(pairs),
               i8_ops_per_pass=pass_ops, rounds=[])
    print(json.dumps({k: v for k, v in row.items() if k != "rounds"}), flush=True)
    calls = dict(train=lambda: core.vocab_train(desc, c0, a.iterations),
                 quantize=lambda: core.vocab_train(desc, centres, 0),
                 select=lambda: core.select_pairs(word, img_start, a.words, a.top_k))

    def timings(call):
        call()
        return core.last_timings()

    for _ in range(a.rounds):
        r = {}
        for name, call in calls.items():
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                t.append((time.perf_counter() - t0) * 1e3)
            core.set_call_timing(True)
            k = np.median(np.array([timings(call) for _ in range(a.reps)]), axis=0)
            core.set_call_timing(False)
            r[name] = dict(call_ms=float(np.median(t)), upload_ms=float(k[0]), kernels_ms=float(k[1]),
                           download_ms=float(k[2]))
            print(f"{name}: call {r[name]['call_ms']:.2f} ms; sfm_last_timings: upload {k[0]:.2f}, kernels {k[1]:.2f}, "
                  f"download {k[2]:.2f} ms", flush=True)
        for name, p in (("train", passes), ("quantize", 1)):
            rate = p * pass_ops / (r[name]["kernels_ms"] * 1e-3)
            r[name].update(i8_ops_per_s=rate, i8_peak_fraction=rate / I8_PEAK_OPS)
            print(f"{name}: i8 MFMA {rate / 1e12:.0f} TOPS over the kernel phase = {100 * rate / I8_PEAK_OPS:.1f} % of "
                  "~5 POPS dense", flush=True)
        row["rounds"].append(r)
    if not a.no_baseline:
        import subprocess
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "words.npz")
            np.savez(path, word=word, img_start=img_start)
            shape = ["--words", a.words, "--top-k", a.top_k, "--reps", a.reps]
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only", path] +
                                   [str(v) for v in shape], capture_output=True, text=True, check=True)
        row["torch_dense_matmul_topk_ms"] = json.loads(child.stdout.strip().splitlines()[-1]) * 1e3
        print(f"torch dense fp32 V @ V.T + cosine + topk: {row['torch_dense_matmul_topk_ms']:.2f} ms (V on the device)",
              flush=True)
    print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
