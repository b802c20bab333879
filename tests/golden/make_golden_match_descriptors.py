"""Generate tests/golden/match_descriptors.npz: descriptor matching on two scenes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_match_descriptors.py

Everything comes from the plain-numpy restatement of
tests/test_match_descriptors.py with fixed seeds; nothing comes from the
reference, which has no matcher.  Stored per scene ("synthetic": four images of
60 noisy scene points and 40 distractors each, all six pairs; "small": uniform
random 64-byte descriptors in images of 70, 0, 1 and 33 keypoints, eight
ordered pairs): desc, img_start, pairs and mid, the median finite d1.  Stored
per entry of test_match_descriptors.FIXTURE_CASES, with the prefix caseN_:
match_start, a, b, dsq, nn, d1, d2 and nn_rev.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_match_descriptors as md  # noqa: E402


def main():
    out = {}
    for scene in ("synthetic", "small"):
        desc, img_start, pairs = md.scene_inputs(scene)
        d1 = md.restate(desc, img_start, pairs, 1.0, md.INT32_MAX, False)["d1"]
        out.update({f"{scene}_desc": desc, f"{scene}_img_start": img_start, f"{scene}_pairs": pairs,
                    f"{scene}_mid": np.int32(np.median(d1[d1 < md.INT32_MAX]))})
    for n, (scene, ratio, max_dsq, cross) in enumerate(md.FIXTURE_CASES):
        desc, img_start, pairs = md.scene_inputs(scene)
        if max_dsq == "mid":
            max_dsq = int(out[f"{scene}_mid"])
        ref = md.restate(desc, img_start, pairs, ratio, max_dsq, cross)
        print(f"case{n}", scene, ratio, max_dsq, cross, "matches per pair", np.diff(ref["match_start"]).tolist())
        out.update({f"case{n}_{k}": ref[k] for k in md.OUTPUTS})
    path = os.path.join(HERE, "match_descriptors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
