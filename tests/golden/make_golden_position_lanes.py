"""Writes tests/golden/position_averaging_lanes.npz for the lane-width graphs
of tests/test_position_averaging.py (LANE_GRAPHS).  The graphs themselves are
not stored: a test regenerates each from its seed and checks the SHA-256 of its
ij and dir bytes against the one kept here.  Per graph:

    <name>_C, _info, _n_solved   the dense-solve restatement at the defaults
    <name>_margin                its least |theta - threshold|
    <name>_cg_gap                the gap the numpy PCG at the same cg_tol leaves to it
    <name>_pcg_iters             that PCG's iterations per round
    <name>_ident_iters           the same PCG without a preconditioner
    <name>_sha256

and for graphs a to e of position_averaging.npz <name>_ident_iters alone.  For
the capped solves (graph b at CAP_ROUNDS rounds and every cap of CAPS; graphs b
and d at the defaults and a cap of 3): cap<cap>_gap and cap3_<name>_gap, the gap
between the float64 PCG at that cap and the same PCG carried in np.longdouble.

Asserted before anything is written: every round's c is positive, every final
angle keeps 1e-6 rad from the threshold (the capped solves' too), n_solved is
what the graph was built for.

    python tests/golden/make_golden_position_lanes.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_position_averaging as pa  # noqa: E402

N_SOLVED = {"dense100": 100, "k64": 64, "k32x3": 32, "k16x9": 16, "k8x37": 8, "k200": 200, "core120": 240,
            "clamp256": 256, "clamp257": 257, "bound512": 512, "bound513": 513, "dense300": 300, "dense1100": 1100}


def capped(g, cap, rounds):
    args = {**pa.DEFAULTS, "rounds": rounds, "cg_max_iters": cap}
    narrow = pa.restate(g["N"], g["ij"], g["dir"], g["weight"], solver="pcg", **args)
    wide = pa.restate(g["N"], g["ij"], g["dir"], g["weight"], solver="pcg", dtype=np.longdouble, **args)
    assert narrow["margin"] > pa.MASK_MARGIN and wide["margin"] > pa.MASK_MARGIN, (cap, narrow["margin"])
    assert np.array_equal(narrow["edge_inlier"], wide["edge_inlier"])
    assert np.all(narrow["cg_iters"] == cap) and np.all(wide["cg_iters"] == cap), (cap, narrow["cg_iters"])
    return np.float64(pa.gaps(narrow, wide))


def main():
    assert np.finfo(np.longdouble).eps < 1e-18
    arrays = {}
    for name, (make, rounds, _) in pa.LANE_GRAPHS.items():
        g = make()
        args = {**pa.DEFAULTS, "rounds": rounds}
        out = pa.restate(g["N"], g["ij"], g["dir"], g["weight"], **args)
        pcg = pa.restate(g["N"], g["ij"], g["dir"], g["weight"], solver="pcg", **args)
        ident = pa.restate(g["N"], g["ij"], g["dir"], g["weight"], solver="pcg", precond="identity", **args)
        assert out["n_solved"] == N_SOLVED[name], (name, out["n_solved"])
        assert out["margin"] > pa.MASK_MARGIN and pcg["margin"] > pa.MASK_MARGIN, (name, out["margin"])
        assert np.all(out["c"] > 0) and np.all(pcg["c"] > 0), name
        assert np.array_equal(out["edge_inlier"], pcg["edge_inlier"]) and np.array_equal(out["info"], pcg["info"])
        assert np.all(pcg["cg_iters"] < pa.DEFAULTS["cg_max_iters"]), (name, pcg["cg_iters"])
        arrays[name + "_C"], arrays[name + "_info"] = out["C"], out["info"]
        arrays[name + "_n_solved"] = np.int64(out["n_solved"])
        arrays[name + "_margin"] = np.float64(out["margin"])
        arrays[name + "_cg_gap"] = np.float64(pa.gaps(pcg, out))
        arrays[name + "_pcg_iters"], arrays[name + "_ident_iters"] = pcg["cg_iters"], ident["cg_iters"]
        arrays[name + "_sha256"] = np.array(pa.graph_hash(g))
        entries = np.bincount(g["ij"].ravel(), minlength=g["N"])
        print(f"{name}: N {g['N']}, E {len(g['ij'])}, entries a node {entries.min()}..{entries.max()} (mean "
              f"{entries.mean():.1f}); margin {out['margin']:.2e}; cg_gap {float(arrays[name + '_cg_gap']):.2e}; "
              f"PCG iterations {pcg['cg_iters'].tolist()}, without a preconditioner {ident['cg_iters'].tolist()}")
    for name in sorted(pa.FIXTURE_GRAPHS):
        g = pa.stored_graph(name)
        ident = pa.restate(g["N"], g["ij"], g["dir"], g["weight"], solver="pcg", precond="identity", **pa.DEFAULTS)
        arrays[name + "_ident_iters"] = ident["cg_iters"]
        print(f"{name}: PCG iterations {pa.fixture()[name + '_pcg_iters'].tolist()}, without a preconditioner "
              f"{ident['cg_iters'].tolist()}")
    for cap in pa.CAPS:
        arrays[f"cap{cap}_gap"] = capped(pa.stored_graph("b"), cap, pa.CAP_ROUNDS)
        print(f"b, {pa.CAP_ROUNDS} rounds, cap {cap}: float64 to long double {float(arrays[f'cap{cap}_gap']):.2e}")
    for name in ("b", "d"):
        arrays[f"cap3_{name}_gap"] = capped(pa.stored_graph(name), 3, pa.DEFAULTS["rounds"])
        print(f"{name}, cap 3: float64 to long double {float(arrays[f'cap3_{name}_gap']):.2e}")
    path = os.path.join(HERE, "position_averaging_lanes.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
