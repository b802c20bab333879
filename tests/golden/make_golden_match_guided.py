"""Generate tests/golden/match_guided.npz: guided descriptor matching on two scenes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_match_guided.py

The inputs are the scenes of tests/test_match_guided.py with fixed seeds; the
outputs come from the loop-written restatement below, which shares nothing with
the numpy one of that file: the gate is evaluated one pair of keypoints at a
time on Python floats (IEEE doubles, one rounding per operation, never fused),
the candidates are walked in index order with a running first and second, and
the reverse direction is a loop of its own.  Nothing comes from the reference,
which has no matcher.  Stored: small_* ("small": uniform random 64-byte
descriptors and keypoints in images of 70, 0, 1 and 33 keypoints, nine ordered
pairs, one F with a NaN) and border_* (one pair, 200 x 1,200 keypoints, every row
with six columns stepped ulp by ulp across the threshold curve): desc, xy,
img_start, pairs, F; small_mid, the median finite d1 of the small scene;
border_gate, border_rows, border_cols; and per entry (case0.. as
test_match_guided.FIXTURE_CASES, and border) match_start, a, b, dsq, nn, d1, d2,
nn_rev and n_cand.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_match_guided as mg  # noqa: E402

INT32_MAX = 2 ** 31 - 1


def inside(F, x, y, u, v, thr2):
    """vp_inlier on Python floats, one operation per line of the header's definition"""
    l0 = (F[0] * x + F[1] * y) + F[2]
    l1 = (F[3] * x + F[4] * y) + F[5]
    l2 = (F[6] * x + F[7] * y) + F[8]
    m0 = (F[0] * u + F[3] * v) + F[6]
    m1 = (F[1] * u + F[4] * v) + F[7]
    e = (u * l0 + v * l1) + l2
    den = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1)
    return den > 0.0 and e * e < thr2 * den


def product(a, b):
    try:
        return a * b
    except OverflowError:
        return float("inf")


def loop_restate(desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross_check):
    desc = np.asarray(desc).astype(np.int64)
    xy = [(float(x), float(y)) for x, y in xy]
    thr2 = product(float(gate), float(gate))
    r2 = float(ratio) * float(ratio)
    out = {k: [] for k in mg.OUTPUTS}
    out["match_start"].append(0)
    for p, (i, j) in enumerate(pairs):
        Fp = [float(f) for f in np.asarray(F[p]).reshape(9)]
        i0, j0 = int(img_start[i]), int(img_start[j])
        ni, nj = int(img_start[i + 1]) - i0, int(img_start[j + 1]) - j0
        dsq = [[int(((desc[i0 + a] - desc[j0 + b]) ** 2).sum()) for b in range(nj)] for a in range(ni)]
        cand = [[inside(Fp, *xy[i0 + a], *xy[j0 + b], thr2) for b in range(nj)] for a in range(ni)]
        nn, d1, d2, n_cand = [], [], [], []
        for a in range(ni):
            best, first, second, count = -1, INT32_MAX, INT32_MAX, 0
            for b in range(nj):
                if not cand[a][b]:
                    continue
                count += 1
                if best < 0 or dsq[a][b] < first:      # ascending b: a tie keeps the smaller index
                    best, first, second = b, dsq[a][b], (first if best >= 0 else INT32_MAX)
                elif count == 2 or dsq[a][b] < second:
                    second = dsq[a][b]
            nn.append(best)
            d1.append(first)
            d2.append(second)
            n_cand.append(count)
        nn_rev = []
        for b in range(nj):
            best = -1
            for a in range(ni):
                if cand[a][b] and (best < 0 or dsq[a][b] < dsq[best][b]):
                    best = a
            nn_rev.append(best)
        n = 0
        for a in range(ni):
            if nn[a] < 0 or d1[a] > max_dsq:
                continue
            if d2[a] != INT32_MAX and not float(d1[a]) < r2 * float(d2[a]):
                continue
            if cross_check and nn_rev[nn[a]] != a:
                continue
            out["a"].append(a)
            out["b"].append(nn[a])
            out["dsq"].append(d1[a])
            n += 1
        out["match_start"].append(out["match_start"][-1] + n)
        for k, v in (("nn", nn), ("d1", d1), ("d2", d2), ("nn_rev", nn_rev), ("n_cand", n_cand)):
            out[k].extend(v)
    return {k: np.array(v, dtype=np.int64 if k == "match_start" else np.int32) for k, v in out.items()}


def main():
    out = {}
    small = mg.small_scene()
    out.update({f"small_{k}": v for k, v in zip(("desc", "xy", "img_start", "pairs", "F"), small)})
    d1 = loop_restate(*small, mg.SMALL_GATE, 1.0, INT32_MAX, False)["d1"]
    out["small_mid"] = np.int32(np.median(d1[d1 < INT32_MAX]))
    for n, (ratio, max_dsq, cross) in enumerate(mg.FIXTURE_CASES):
        if max_dsq == "mid":
            max_dsq = int(out["small_mid"])
        ref = loop_restate(*small, mg.SMALL_GATE, ratio, max_dsq, cross)
        print(f"case{n}", ratio, max_dsq, cross, "matches per pair", np.diff(ref["match_start"]).tolist(),
              "candidates per row: none", int((ref["n_cand"] == 0).sum()), "one", int((ref["n_cand"] == 1).sum()),
              "more", int((ref["n_cand"] > 1).sum()))
        out.update({f"case{n}_{k}": ref[k] for k in mg.OUTPUTS})
    *border, gate, rows, cols = mg.border_scene()
    out.update({f"border_{k}": v for k, v in zip(("desc", "xy", "img_start", "pairs", "F"), border)})
    out.update(border_gate=np.float64(gate), border_rows=rows, border_cols=cols)
    ref = loop_restate(*border, gate, 1.0, INT32_MAX, True)
    print("border: matches", int(ref["match_start"][-1]), "candidates per row: min", int(ref["n_cand"].min()), "max",
          int(ref["n_cand"].max()))
    out.update({f"border_{k}": ref[k] for k in mg.OUTPUTS})
    path = os.path.join(HERE, "match_guided.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300_000


if __name__ == "__main__":
    main()
