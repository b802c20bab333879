"""Track merging, timed: sfm_merge_tracks (every row of a store in one call)
beside the two host routes there are without it -- the plain-Python restatement
of tests/test_merge_tracks.py (a dictionary of keys and a union-find) and a
vectorised numpy version (np.unique on the keys, then label propagation over
the row-keypoint incidences until nothing changes).  Both baselines run on the
host that drives the device, once each (they take seconds); their components
and conflicts are compared with the call's.

Shape: cfg5's, 500,000 rows and about 4 M observations over 200 images.  The
rows are cut from longer ground-truth tracks (--track-rows rows a track on
average, each row a random subset of the track's keypoints), so merging has
work to do; --conflicts of the rows take one keypoint of another track.  Per
round: the median over --reps calls after a warm-up of the whole call (host
clock around a call that ends in a stream synchronise) and of upload, kernels
and download (HIP events, sfm_last_timings, in calls of their own).

    python tools/merge_tracks_once.py [--rows 500000] [--row-len 8] [--images 200] [--track-rows 4] [--conflicts 0.01] [--rounds 3] [--reps 5] [--no-baselines] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "structure-from-motion-_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import _sfmcore as core  # noqa: E402


def scene(n_rows, row_len, n_images, track_rows, conflicts, seed=3):
    """CSR rows (row_start, image, x, y): ground-truth tracks of 2 row_len keypoints in distinct images, each cut
    into rows of row_len of them, images ascending inside a row; the rows shuffled"""
    rng = np.random.default_rng(seed)
    n_tracks = max(n_rows // track_rows, 1)
    L = min(2 * row_len, n_images)
    # a track's images: L distinct ones (a random start and stride pattern), its keypoints random pixels
    t_img = np.sort(np.argsort(rng.random((n_tracks, n_images)), axis=1)[:, :L].astype(np.int32), axis=1)
    t_x, t_y = rng.uniform(0, 4000, (n_tracks, L)), rng.uniform(0, 3000, (n_tracks, L))
    track = rng.integers(0, n_tracks, n_rows)
    pick = np.sort(np.argsort(rng.random((n_rows, L)), axis=1)[:, :row_len], axis=1)
    image = t_img[track[:, None], pick]
    x, y = t_x[track[:, None], pick], t_y[track[:, None], pick]
    # a share of the rows takes its first keypoint from another track (its smallest image, so the row stays sorted)
    bad = np.where(rng.random(n_rows) < conflicts)[0]
    other = rng.integers(0, n_tracks, len(bad))
    ok = t_img[other, 0] <= image[bad, 1]
    bad, other = bad[ok], other[ok]
    image[bad, 0], x[bad, 0], y[bad, 0] = t_img[other, 0], t_x[other, 0], t_y[other, 0]
    row_start = np.arange(n_rows + 1, dtype=np.int64) * row_len
    return row_start, np.ascontiguousarray(image.reshape(-1)), x.reshape(-1).copy(), y.reshape(-1).copy()


def numpy_merge(row_start, image, x, y):
    """keypoint, component and conflict by numpy alone: np.unique on the keys, then the smallest row index
    propagated over the (row, keypoint) incidences until it stops changing"""
    n_rows, n_obs = len(row_start) - 1, len(image)
    row = np.repeat(np.arange(n_rows), np.diff(row_start))
    keys = np.column_stack([image.astype(np.float64), x + 0.0, y + 0.0])  # + 0.0: -0.0 becomes 0.0
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    keypoint = first[inverse]  # np.unique's return_index is the first occurrence
    lab = np.arange(n_rows)
    sweeps = 0
    while True:
        sweeps += 1
        kp_lab = np.full(len(first), n_rows)
        np.minimum.at(kp_lab, inverse, lab[row])
        new = lab.copy()
        np.minimum.at(new, row, kp_lab[inverse])
        new = new[new]  # pointer jumping: a label is a row, take that row's label
        if np.array_equal(new, lab):
            break
        lab = new
    # conflicting: a (component, image) with more than one keypoint
    ck = np.unique(np.column_stack([lab[row], image, keypoint]), axis=0)
    twice = (ck[1:, 0] == ck[:-1, 0]) & (ck[1:, 1] == ck[:-1, 1])
    bad = np.zeros(n_rows, dtype=bool)
    bad[ck[1:, 0][twice]] = True
    return keypoint.astype(np.int32), lab.astype(np.int32), bad[lab], sweeps


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
    ap.add_argument("--rows", type=int, default=500000)
    ap.add_argument("--row-len", type=int, default=8)
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--track-rows", type=int, default=4)
    ap.add_argument("--conflicts", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    core.require_device()
    rs, im, x, y = scene(a.rows, a.row_len, a.images, a.track_rows, a.conflicts)

    def call():
        return core.merge_tracks(rs, im, x, y, a.images, core.MERGE_DROP)

    def timings():
        call()
        return core.last_timings()

    out = call()
    comps, size = np.unique(out["component"], return_counts=True)
    row = dict(rows=a.rows, observations=len(im), images=a.images, keypoints=int(np.sum(out["keypoint"] == np.arange(len(im)))),
               components=len(comps), largest_component=int(size.max()),
               conflicting_components=int(len(np.unique(out["component"][out["conflict"]]))),
               tracks=len(out["track_label"]), track_observations=len(out["track_obs"]), rounds=[])
    print(json.dumps({k: v for k, v in row.items() if k != "rounds"}), flush=True)
    for _ in range(a.rounds):
        whole = median_ms(call, a.reps)
        core.set_call_timing(True)
        k = np.median(np.array([timings() for _ in range(a.reps + 1)][1:]), axis=0)
        core.set_call_timing(False)
        row["rounds"].append(dict(call_ms=whole, upload_ms=float(k[0]), kernels_ms=float(k[1]), download_ms=float(k[2])))
        print(f"call {whole:.2f} ms; sfm_last_timings: upload {k[0]:.2f}, kernels {k[1]:.2f}, download {k[2]:.2f} ms",
              flush=True)
    if not a.no_baselines:
        t0 = time.perf_counter()
        kp, comp, cf, sweeps = numpy_merge(rs, im, x, y)
        row["numpy_ms"] = (time.perf_counter() - t0) * 1e3
        row["numpy_sweeps"] = sweeps
        row["numpy_agrees"] = bool(np.array_equal(kp, out["keypoint"]) and np.array_equal(comp, out["component"])
                                   and np.array_equal(cf, out["conflict"]))
        print(f"numpy (np.unique + {sweeps} propagation sweeps) {row['numpy_ms']:.0f} ms, agrees: {row['numpy_agrees']}",
              flush=True)
        import test_merge_tracks as mt
        t0 = time.perf_counter()
        ref = mt.restate(rs, im, x, y, mt.DROP)
        row["python_ms"] = (time.perf_counter() - t0) * 1e3
        row["python_agrees"] = all(np.array_equal(ref[n], out[n]) for n in mt.OUTPUTS)
        print(f"plain-Python restatement {row['python_ms']:.0f} ms, agrees: {row['python_agrees']}", flush=True)
    print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
