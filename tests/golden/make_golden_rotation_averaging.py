"""Writes tests/golden/rotation_averaging.npz: the fixture view graphs of
tests/test_rotation_averaging.py (1 degree of noise, 30 % wrong edges) with the
numpy restatement's outputs on them.  Small arrays only.

The seeds are chosen so that no trace test of any run the device tests make on
these graphs lies within 1e-9 of tau; that is asserted here before anything is
written, and again by the CPU tests.

    python tests/golden/make_golden_rotation_averaging.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_rotation_averaging as ra  # noqa: E402


def main():
    arrays = {}
    for name in sorted(ra.FIXTURE_GRAPHS):
        g = ra.fixture_graph(name)
        for k in ("ij", "R_rel", "R_true", "clean"):
            arrays[f"{name}_{k}"] = g[k]
        arrays[name + "_N"] = np.int64(g["N"])
        if g["weight"] is not None:
            arrays[name + "_weight"] = g["weight"]
        for cs, ms, tol in ra.FIXTURE_RUNS:
            out = ra.restate(g["N"], g["ij"], g["R_rel"], g["weight"], seed=ra.FIXTURE_ARGS["seed"],
                             threshold=ra.FIXTURE_ARGS["threshold"], consensus_sweeps=cs, max_sweeps=ms, tol=tol)
            assert out["margin"] > ra.MARGIN, (name, cs, ms, tol, out["margin"])
            print(f"{name}: consensus_sweeps {cs}, max_sweeps {ms}, tol {tol}: {out['sweeps']} sweeps, "
                  f"{int(out['edge_inlier'].sum())} / {len(g['ij'])} inlier edges ({int(g['clean'].sum())} clean), "
                  f"margin {out['margin']:.2e}")
            if (cs, ms, tol) == (ra.FIXTURE_ARGS["consensus_sweeps"], ra.FIXTURE_ARGS["max_sweeps"],
                                 ra.FIXTURE_ARGS["tol"]):
                for n in ra.OUTPUTS:
                    arrays[f"{name}_out_{n}"] = np.asarray(out[n])
    path = os.path.join(HERE, "rotation_averaging.npz")
    np.savez(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
