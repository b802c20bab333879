"""Writes tests/golden/position_averaging.npz: the fixture view graphs of
tests/test_position_averaging.py, each with its truth, the dense-solve
restatement's outputs on them at the defaults, the gap `cg_gap` that the numpy
PCG restatement at the same cg_tol leaves to the dense solve (it sets the
device tests' tolerance), and for graph (a) the error against the truth.

Asserted before anything is written, and again by the CPU tests: every final
edge angle of every graph keeps 1e-6 rad from the threshold, so no mask bit
turns on last bits, and every round's c is positive.

    python tests/golden/make_golden_position_averaging.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_position_averaging as pa  # noqa: E402


def main():
    arrays = {}
    for name in sorted(pa.FIXTURE_GRAPHS):
        g = pa.FIXTURE_GRAPHS[name]()
        for k in ("ij", "dir", "truth", "clean"):
            arrays[f"{name}_{k}"] = g[k]
        arrays[name + "_N"] = np.int64(g["N"])
        if g["weight"] is not None:
            arrays[name + "_weight"] = g["weight"]
        out = pa.restate(g["N"], g["ij"], g["dir"], g["weight"], **pa.DEFAULTS)
        pcg = pa.restate(g["N"], g["ij"], g["dir"], g["weight"], solver="pcg", **pa.DEFAULTS)
        assert out["margin"] > pa.MASK_MARGIN and pcg["margin"] > pa.MASK_MARGIN, (name, out["margin"])
        assert np.all(out["c"] > 0) and np.all(pcg["c"] > 0), name
        assert np.array_equal(out["edge_inlier"], pcg["edge_inlier"]) and np.array_equal(out["info"], pcg["info"])
        assert np.all(pcg["cg_iters"] < pa.DEFAULTS["cg_max_iters"]), (name, pcg["cg_iters"])
        for k in ("C", "edge_angle", "edge_inlier", "edge_length", "info"):
            arrays[f"{name}_out_{k}"] = out[k]
        arrays[name + "_out_n_solved"] = np.int64(out["n_solved"])
        arrays[name + "_cg_gap"] = np.float64(pa.gaps(pcg, out))
        arrays[name + "_pcg_iters"] = pcg["cg_iters"]
        s = out["info"] >= 0
        e = s[g["ij"][:, 0]] & s[g["ij"][:, 1]]
        good, bad = g["clean"] & e, ~g["clean"] & e
        print(f"{name}: N {g['N']}, E {len(g['ij'])}, solved {out['n_solved']}, max entries "
              f"{int(np.bincount(g['ij'].ravel()).max())}; mask {int(out['edge_inlier'][good].sum())}/{int(good.sum())} "
              f"clean and {int(out['edge_inlier'][bad].sum())}/{int(bad.sum())} wrong edges; margin {out['margin']:.2e}; "
              f"cg_gap {float(arrays[name + '_cg_gap']):.2e}; PCG iterations {pcg['cg_iters'].tolist()}; "
              f"worst camera {pa.align(out['C'][s], g['truth'][s]):.3g}")
        if name == "a":
            arrays["a_truth_error"] = np.float64(pa.align(out["C"], g["truth"]))
            print("a: truth error", float(arrays["a_truth_error"]))
        if name == "b":
            assert np.array_equal(out["edge_inlier"], g["clean"])
    path = os.path.join(HERE, "position_averaging.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
