"""Writes tests/golden/rotation_cg.npz: results only, the graphs come from
their seeds (tests/test_rotation_cg.py) and are pinned by a SHA-256 of their ij
and R_rel.

Per fixed-point graph: the Jacobi restatement run to tol = 1e-12 (max_sweeps
20,000), 2 to 16 s each.  Per device graph: the PCG restatement's rotations,
levels, rounds, iteration counts, residuals and steps, its margins, and
`cg_gap`, its gap to the restatement with the dense minimum-norm solve (R on
the nodes whose group holds a root, edge_angle on the edges between them).

    python tests/golden/make_golden_rotation_cg.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import test_rotation_averaging as ra  # noqa: E402
import test_rotation_cg as rc  # noqa: E402


def main():
    fx = {}
    for name, make in rc.FIXED_POINT.items():
        g = make()
        fx[name + "_sha256"] = rc.graph_hash(g)
        t0 = time.perf_counter()
        out = ra.restate(g["N"], g["ij"], g["R_rel"], g["weight"], max_sweeps=20000, tol=1e-12, **rc.RUN)
        assert out["sweeps"] < 20000
        for n in ("R", "edge_inlier", "n_inlier_edges", "group", "info", "level", "sweeps", "margin"):
            fx[f"{name}_jacobi_{n}"] = out[n]
        print(f"{name}: Jacobi to 1e-12 in {out['sweeps']} sweeps, {time.perf_counter() - t0:.1f} s, margin "
              f"{out['margin']:.3g}", flush=True)
    for name, (make, _, G) in rc.DEVICE_GRAPHS.items():
        g = make()
        assert rc.lanes(g) == G, (name, rc.lanes(g))
        fx[name + "_sha256"] = rc.graph_hash(g)
        args = rc.run_args(name)
        t0 = time.perf_counter()
        pcg = rc.restate_cg(g["N"], g["ij"], g["R_rel"], g["weight"], **args)
        t1 = time.perf_counter()
        dense = rc.restate_cg(g["N"], g["ij"], g["R_rel"], g["weight"], **args, solver="dense")
        for n in ra.INTEGER_OUTPUTS:
            assert np.array_equal(pcg[n], dense[n]), (name, n)
        keep = rc.rooted(g["N"], g["ij"], pcg["group"])
        ek = keep[g["ij"][:, 0]] & keep[g["ij"][:, 1]]
        gap = max(float(np.abs(pcg["R"][keep] - dense["R"][keep]).max()),
                  float(np.abs(pcg["edge_angle"][ek] - dense["edge_angle"][ek]).max()) if ek.any() else 0.0)
        for n in ("R", "level", "sweeps", "cg_iters", "cg_residual", "step", "margin", "step_margin"):
            fx[f"{name}_pcg_{n}"] = pcg[n]
        fx[name + "_pcg_margin"] = min(pcg["margin"], dense["margin"])
        fx[name + "_cg_gap"] = gap
        print(f"{name}: N {g['N']}, E {len(g['ij'])}, G {G}, rounds {pcg['sweeps']}, CG iterations "
              f"{pcg['cg_iters'].tolist()}, steps {['%.2g' % s for s in pcg['step']]}, cg_gap {gap:.3g}, margins "
              f"{pcg['margin']:.3g} / {pcg['step_margin']:.3g}, rooted {int(keep.sum())}; PCG {t1 - t0:.1f} s, dense "
              f"{time.perf_counter() - t1:.1f} s", flush=True)
    np.savez_compressed(os.path.join(HERE, "rotation_cg.npz"), **fx)


if __name__ == "__main__":
    main()
