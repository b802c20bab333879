"""Speculation of the rejection branch's damped Schur system (DESIGN §4 "LM
control"): once a step of a solve has been rejected, the system at lambda * nu
is built beside every reduced solve, and a rejected step's successor takes it
instead of building its own.

The speculated system is the unspeculated one up to the order in which the
split (spec, range) items' partial slabs are summed, so a speculated solve
must count the same iterations and accepted steps and reach the same cost to
1e-9 relative, points to 1e-6 and cameras to 1e-8 (the bounds of the
multi-rank and split-plan comparisons), and be bitwise repeatable.  Before the
first rejection nothing differs: bitwise the unspeculated solve.

Cases: (a) cfg3, 6 cameras / 2000 points, no split (its items fit the free
CUs); (b) 33 cameras (17 specs, one of them a single camera) / 3000 points in
one range of several chunks, with 12 free CUs so that 9 of the 17 specs are
split (the whole items come in rounds of 8); (c) the same with no free CU,
every item split.
"""
import numpy as np
import pytest

import sfm_synthetic as syn

pytestmark = pytest.mark.gpu
K = syn.K_REF
ITERS = 24  # fixed iterations: past convergence, where the rejections are

CASES = {
    "cfg3": (dict(), lambda: syn.ba_problem_cfg("cfg3", dense=False)),
    "some_split": (dict(SFM_SWEEP_RANGES="1", SFM_SPEC_FREE_CUS="12"), lambda: syn.ba_problem(33, 3000, 12, seed=7, dense=False)),
    "all_split": (dict(SFM_SWEEP_RANGES="1", SFM_SPEC_FREE_CUS="0"), lambda: syn.ba_problem(33, 3000, 12, seed=7, dense=False)),
}


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


_problems = {}


def problem_args(case):
    gen = CASES[case][1]
    if gen not in _problems:
        p = gen()
        cams0 = np.column_stack([p["rotvec0"], np.einsum("nij,nj->ni", -p["R0"], p["C0"])])
        _problems[gen] = (cams0, p["X0"], p["cam_idx"], p["pt_idx"], p["obs"], K)
    return _problems[gen]


def solve(core, monkeypatch, case, speculate, args=None, **opts):
    """one solve of a fresh problem: (cameras, points, report, speculative plan)"""
    for k, v in CASES[case][0].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SFM_SPECULATE", "1" if speculate else "0")
    prob = core.BAProblem(*(args or problem_args(case)))
    try:
        rep = prob.solve(**opts)
        cams, pts = prob.download()
        return cams, pts, rep, prob.spec_plan()
    finally:
        prob.close()


_plain = {}


def plain(core, monkeypatch, case):
    """the unspeculated solve of a case, computed once"""
    if case not in _plain:
        _plain[case] = solve(core, monkeypatch, case, False, max_iterations=ITERS, fixed_iterations=True)
    return _plain[case]


def check_plan(case, plan):
    if case == "cfg3":
        assert plan["sub_ranges"] == 0 and plan["whole_items"] > 0, plan
    elif case == "some_split":
        assert plan["sub_ranges"] >= 2 and plan["whole_items"] > 0 and plan["split_specs"] > 0, plan
    else:
        assert plan["sub_ranges"] >= 2 and plan["whole_items"] == 0 and plan["split_specs"] == 17, plan


@pytest.mark.parametrize("case", list(CASES))
def test_speculated_solve_matches_unspeculated(core, monkeypatch, case):
    c0, x0, r0, _ = plain(core, monkeypatch, case)
    c1, x1, r1, plan = solve(core, monkeypatch, case, True, max_iterations=ITERS, fixed_iterations=True)
    print(case, plan, r0, r1, np.abs(c1 - c0).max(), np.abs(x1 - x0).max())
    check_plan(case, plan)
    assert 0 < r0["accepted"] < r0["iterations"] == ITERS  # rejections, so speculated systems were used
    assert (r1["iterations"], r1["accepted"], r1["status"]) == (r0["iterations"], r0["accepted"], r0["status"])
    assert abs(r1["cost"] - r0["cost"]) <= 1e-9 * r0["cost"]
    assert np.abs(c1 - c0).max() < 1e-8 and np.abs(x1 - x0).max() < 1e-6


@pytest.mark.parametrize("case", list(CASES))
def test_speculated_solve_is_repeatable(core, monkeypatch, case):
    for k, v in CASES[case][0].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SFM_SPECULATE", "1")
    ca, xa, ra, _ = solve(core, monkeypatch, case, True, max_iterations=ITERS, fixed_iterations=True)
    prob = core.BAProblem(*problem_args(case))
    try:
        rb = prob.solve(max_iterations=ITERS, fixed_iterations=True)
        cb, xb = prob.download()
        prob.reset()
        rc = prob.solve(max_iterations=ITERS, fixed_iterations=True)
        cc, xc = prob.download()
    finally:
        prob.close()
    for c, x, r in ((cb, xb, rb), (cc, xc, rc)):
        assert (r["iterations"], r["accepted"], r["status"], r["cost"], r["lambda_"]) == \
            (ra["iterations"], ra["accepted"], ra["status"], ra["cost"], ra["lambda_"])
        assert np.array_equal(c, ca) and np.array_equal(x, xa)


def test_all_accepted_solve_is_bitwise_unspeculated(core, monkeypatch):
    """up to the first rejection speculation queues nothing"""
    n = 0
    for m in range(1, ITERS):  # the iterations before the first rejected step
        r = solve(core, monkeypatch, "some_split", False, max_iterations=m, fixed_iterations=True)[2]
        if r["accepted"] < m:
            break
        n = m
    assert n >= 1
    c0, x0, r0, _ = solve(core, monkeypatch, "some_split", False, max_iterations=n, fixed_iterations=True)
    c1, x1, r1, _ = solve(core, monkeypatch, "some_split", True, max_iterations=n, fixed_iterations=True)
    assert r1["accepted"] == n and r1 == {**r0, "t_loop_ms": r1["t_loop_ms"]}
    assert np.array_equal(c1, c0) and np.array_equal(x1, x0)


def test_all_rejected_solve_returns_its_input(core, monkeypatch):
    """a converged start at a tiny damping: every step is rejected (the
    speculated system is used from the third iteration on), and the solve
    returns its input bit for bit"""
    c0, x0, r0, _ = plain(core, monkeypatch, "all_split")
    args = (c0, x0) + problem_args("all_split")[2:]
    c1, x1, r1, plan = solve(core, monkeypatch, "all_split", True, args=args, max_iterations=8,
                             fixed_iterations=True, initial_lambda=1e-30)
    print(r1)
    check_plan("all_split", plan)
    assert (r1["iterations"], r1["accepted"]) == (8, 0)
    assert r1["cost"] == r1["cost0"]
    assert np.array_equal(c1, c0) and np.array_equal(x1, x0)
