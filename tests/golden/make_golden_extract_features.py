"""Generate tests/golden/extract_features.npz: feature extraction on three textures.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_extract_features.py

Everything comes from the plain-numpy restatement of
tests/test_extract_features.py with fixed seeds; nothing comes from the
reference, which has no extractor.  The images are smooth random textures
(sums of random Gaussian blobs of several scales) of 130 x 97, 97 x 130 and
80 x 64 pixels.  Stored per image k: imgK and the fp64 restatement's cands, xy,
scale, response, angle, desc, with the prefix imgK_.  Stored once: the
ambiguity budget of the fp32 against the fp64 restatement (budget_x, _y,
_scale, _response, _angle: the largest differences over keypoints accepted by
both; budget_dec_move, _contrast, _edge, _peak: per decision the largest fp64
margin at which the two runs disagree, 0 where they never do); budget1_* and
budget1_dec_*, the same with both precisions run stage by stage on one fp32
pyramid, which is what the device tests compare and allow 4 times; and
chain_matches, the matches of the fp64 restatement on the two crops of
test_extract_features.chain_crops at ratio 0.8 with the cross-check.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_extract_features as ef  # noqa: E402
import test_match_descriptors as md  # noqa: E402


def main():
    out = {}
    images = ef.fixture_images()
    for k, img in enumerate(images):
        r = ef.restate(img)
        print(f"img{k}", img.shape, "candidates", len(r["cands"]), "refined", int(r["refined"]["ok"].sum()),
              "keypoints", len(r["xy"]))
        out[f"img{k}"] = img
        out.update({f"img{k}_{n}": r[n] for n in ("cands", "xy", "scale", "response", "angle", "desc")})
    val, dec = ef.budget(images)
    print("budget", val, dec)
    out.update({"budget_" + n: np.float64(v) for n, v in val.items()})
    out.update({"budget_dec_" + n: np.float64(v) for n, v in dec.items()})
    val1, dec1 = ef.budget_one_pyramid(images)
    print("budget on one pyramid", val1, dec1)
    out.update({"budget1_" + n: np.float64(v) for n, v in val1.items()})
    out.update({"budget1_dec_" + n: np.float64(v) for n, v in dec1.items()})
    a, b = ef.chain_crops()
    ra, rb = ef.restate(a), ef.restate(b)
    desc, st = md.pack([ra["desc"], rb["desc"]])
    m = md.restate(desc, st, [(0, 1)])
    d = rb["xy"][m["b"]] - ra["xy"][m["a"]]
    print("chain: keypoints", len(ra["xy"]), len(rb["xy"]), "matches", len(m["a"]), "largest deviation",
          np.abs(d - np.array(ef.CHAIN_SHIFT, dtype=np.float64)).max())
    out["chain_matches"] = np.int64(len(m["a"]))
    path = os.path.join(HERE, "extract_features.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
