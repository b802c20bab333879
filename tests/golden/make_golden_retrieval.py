"""Generate tests/golden/retrieval.npz: a visual vocabulary and tf-idf retrieval
on the grouped scene.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_retrieval.py

Everything comes from the plain-numpy restatement of tests/test_retrieval.py
with fixed seeds; nothing comes from the reference, which has no such stage.
Stored: the scene (grouped_desc, grouped_img_start, grouped_group: 3 groups of
4 images, 864 descriptors of 128 bytes) and grouped_first, the rows that are the
192 initial centres; trainN_{centres, word, count, inertia, iterations} for
max_iterations N = 1, 3, 10, the centres of N = 1 and 3 as trainN_centres_delta,
their uint8 difference (mod 256) from train10_centres, which is mostly zero;
selK_{neighbour, score, dot, norm2, df} over train10_word for top_k K = 1, 3,
11, 20; and the two edge scenes of test_retrieval.edge_scenes ({empty,
common}_{word, img_start} and their outputs at top_k 3).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_retrieval as rt  # noqa: E402


def main():
    descs, group = rt.grouped_scene()
    desc, img_start = rt.pack(descs)
    c0 = rt.initial_centres(desc, rt.N_WORDS)
    first = np.sort(np.random.default_rng(0).choice(len(desc), rt.N_WORDS, replace=False))
    assert np.array_equal(desc[first], c0)
    out = dict(grouped_desc=desc, grouped_img_start=img_start, grouped_group=group, grouped_first=first)
    for its in rt.TRAIN_ITERATIONS:
        ref = rt.restate_train(desc, c0, its)
        print(f"train{its}: iterations", int(ref["iterations"]), "inertia", ref["inertia"].tolist(), "empty clusters",
              int((ref["count"] == 0).sum()))
        out.update({f"train{its}_{k}": ref[k] for k in rt.TRAIN_OUTPUTS})
    for its in (1, 3):
        out[f"train{its}_centres_delta"] = out.pop(f"train{its}_centres") - out["train10_centres"]
    word = out["train10_word"]
    for k in rt.TOP_KS:
        ref = rt.restate_select(word, img_start, rt.N_WORDS, k)
        out.update({f"sel{k}_{n}": ref[n] for n in rt.SELECT_OUTPUTS})
    ref = rt.restate_select(word, img_start, rt.N_WORDS, 3)
    for i in range(len(group)):
        print("image", i, "group", int(group[i]), "neighbours", ref["neighbour"][i].tolist(),
              "their groups", group[ref["neighbour"][i]].tolist(), "scores", np.round(ref["score"][i], 4).tolist())
    for name, (w, st, nw) in rt.edge_scenes(word, img_start).items():
        ref = rt.restate_select(w, st, nw, 3)
        out.update({f"{name}_word": w, f"{name}_img_start": st})
        out.update({f"{name}_{n}": ref[n] for n in rt.SELECT_OUTPUTS})
    path = os.path.join(HERE, "retrieval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
