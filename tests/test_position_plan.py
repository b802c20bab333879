"""csrc/position_plan.hpp's host arithmetic without a device: builds
tests/position_plan_check.cpp host-only under AddressSanitizer and
UndefinedBehaviorSanitizer and runs it on the solved size of every graph the
position-averaging suites use.  What the device tests say about a graph ("this
one runs at G = 32", "this one re-sums more partials than a workgroup has
threads") is asserted here on the code's own arithmetic.
"""
import os
import subprocess

import numpy as np
import pytest

import test_position_averaging as pa
from conftest import PKG, REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
T2 = 256  # path 2's workgroup, pa_resum's stride

# graph: {path asked for: (path that runs, G) or "refused"}
PLANS = {
    "a": {1: (1, 2), 2: (2, 2), 0: (1, 2)}, "b": {1: (1, 2), 2: (2, 2)}, "c": {1: (1, 1), 2: (2, 1)},
    "d": {1: "refused", 2: (2, 2), 0: (2, 2)}, "e": {1: (1, 1), 2: (2, 1)},
    "dense100": {1: (1, 4), 2: (2, 4)}, "k64": {1: (1, 8), 2: (2, 8)}, "k32x3": {1: (1, 16), 2: (2, 16)},
    "k16x9": {1: (1, 32), 2: (2, 32)}, "k8x37": {1: (1, 64), 2: (2, 64)}, "k200": {1: (1, 2), 2: (2, 32)},
    "core120": {1: (1, 2), 2: (2, 8)}, "clamp256": {1: (1, 2), 2: (2, 4)}, "clamp257": {1: (1, 1), 2: (2, 4)},
    "bound512": {0: (1, 1), 1: (1, 1), 2: (2, 2)}, "bound513": {0: (2, 2), 1: "refused", 2: (2, 2)},
    "dense300": {2: (2, 64)}, "dense1100": {2: (2, 64)},
}
# (graph, path): the grids and the LDS request that the device tests lean on
GRIDS = {
    ("a", 2): dict(nb_group=1, nb_node=1, nb_edge=1), ("c", 2): dict(nb_group=2, nb_node=2, nb_edge=5),
    ("d", 2): dict(nb_group=9, nb_node=5, nb_edge=22), ("e", 2): dict(nb_group=1, nb_node=1, nb_edge=1),
    ("k8x37", 2): dict(nb_group=2, nb_node=1), ("dense300", 2): dict(nb_group=75),
    ("dense1100", 2): dict(nb_group=275), ("bound512", 1): dict(lds_bytes=86208),
}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("position_plan") / "position_plan_check")
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-x", "c++", "-I" + os.path.join(PKG, "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(REPO, "tests", "position_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(n_nodes, n_edges, path):
        r = subprocess.run([exe, str(n_nodes), str(n_edges), str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr  # no sanitizer report
        if r.stdout.strip() == "refused":
            return "refused"
        return dict(zip(("path_used", "G", "nb_group", "nb_node", "nb_edge", "lds_bytes"), map(int, r.stdout.split())))
    return run


def solved_size(name):
    """(solved nodes, edges between them) of a stored or a lane-width graph"""
    g = pa.stored_graph(name) if name in pa.FIXTURE_GRAPHS else pa.lane_graph(name)
    solved, _ = pa.select(g["N"], g["ij"])
    return int(solved.sum()), int((solved[g["ij"][:, 0]] & solved[g["ij"][:, 1]]).sum())


def test_every_graph_gets_the_plan_its_tests_rely_on(plan):
    reached = {1: set(), 2: set()}
    for name, by_path in PLANS.items():
        M, El = solved_size(name)
        for path, want in by_path.items():
            got = plan(M, El, path)
            if want == "refused":
                assert got == "refused" and M > pa.PATH1_MAX_NODES, (name, path, got)
                continue
            assert (got["path_used"], got["G"]) == want, (name, path, got)
            assert got["nb_group"] == -(-M * got["G"] // T2) and got["nb_node"] == -(-M // T2), (name, path, got)
            assert got["nb_edge"] == -(-El // T2), (name, path, got)
            assert got["lds_bytes"] == (168 * M + 192 if got["path_used"] == 1 else 0), (name, path, got)
            assert got["path_used"] == 2 or got["G"] * M <= 512, (name, path, got)
            for k, v in GRIDS.get((name, path), {}).items():
                assert got[k] == v, (name, path, k, got)
            reached[got["path_used"]].add(got["G"])
    assert reached[1] == {1, 2, 4, 8, 16, 32, 64} and reached[2] == {1, 2, 4, 8, 16, 32, 64}, reached


def test_the_edges_of_the_plan(plan):
    """the sides of every step the lane-width graphs were built around"""
    for name in ("k64", "k8x37"):  # path 1 filled exactly once: G M = 512
        M, El = solved_size(name)
        assert plan(M, El, 1)["G"] * M == 512
    M, El = solved_size("k8x37")  # a group is a whole wave; more group workgroups than node workgroups
    got = plan(M, El, 2)
    assert got["G"] == 64 and got["nb_group"] > got["nb_node"]
    M, El = solved_size("k200")  # the clamp: 32 lanes by the mean, 2 in one workgroup
    assert plan(M, El, 2)["G"] == 32 and plan(M, El, 1)["G"] == 2
    M, El = solved_size("dense1100")  # pa_resum takes more than one trip over the group and the edge partials
    got = plan(M, El, 2)
    assert got["nb_group"] > T2 and got["nb_edge"] > T2 and got["nb_node"] < got["nb_group"]
    M, El = solved_size("core120")  # half the nodes have fewer entries than their group has lanes
    g = pa.lane_graph("core120")
    entries = np.bincount(g["ij"].ravel(), minlength=g["N"])
    assert (entries < plan(M, El, 2)["G"]).sum() == g["N"] // 2
    # the width steps at 8 G mean entries a node, and the auto choice at the bound
    assert plan(300, 1200, 2)["G"] == 1 and plan(300, 1201, 2)["G"] == 2
    assert plan(8, 8 * 256 // 2, 2)["G"] == 32 and plan(8, 8 * 256 // 2 + 1, 2)["G"] == 64
    assert plan(8, 1 << 30, 2)["G"] == 64 and plan(1, 1 << 30, 1)["G"] == 64
    assert plan(256, 2560, 1)["G"] == 2 and plan(257, 2570, 1)["G"] == 1
    assert plan(512, 2532, 0)["path_used"] == 1 and plan(513, 2538, 0)["path_used"] == 2
    assert plan(513, 2538, 1) == "refused" and plan(0, 0, 0)["path_used"] == 0 and plan(0, 0, 1)["path_used"] == 0
