"""One LM step of the bundle adjustment on a real MI355X (sfm_ba_lm and the
device-resident session) against the first-principles reference of
tests/test_ba_step.py: the problems, the float64 autograd blocks, the step
recovered from a solver's output and its backward error eta all come from
there.

The step check: after max_iterations=1 the device's step must solve
(J^T J + lambda D) delta = -g as well as the C oracle's does,
    eta_gpu <= 16 max(eta_oracle, eps max|x0| / max|delta|),
both being backward-stable fp64 eliminations of one system that differ in
factorisation and summation order; a wrong Jacobian term, a dropped pair or a
misplaced damping term moves eta by many orders of magnitude.  The same bound
is asked of every solver, planner and kernel variant the library can switch
to, of the step after a rejected one, and of the session after a reset.
"""
import numpy as np
import pytest

import oracle as O
import test_ba_step as S

pytestmark = pytest.mark.gpu
FACTOR = 16.0
VARIANTS = [("SFM_SOLVE", "gj"), ("SFM_SOLVE", "chol"), ("SFM_PLAN_HOST", "0"), ("SFM_PLAN_HOST", "1"),
            ("SFM_SWEEP_RANGES", "1"), ("SFM_SWEEP_RANGES", "8")]
VARIANTS += [(e, v) for e in ("SFM_LINEARIZE_CAM_LDS", "SFM_BACKSUB_CAM_LDS", "SFM_CAMLIN_FUSED", "SFM_FINISH_FUSED",
                              "SFM_GJR_FOLD") for v in ("0", "1")]


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


_steps = {}


def gpu_step(core, name, lam):
    """the device's first step on a case from its start at damping lam, computed once"""
    if (name, lam) not in _steps:
        _steps[name, lam] = core.ba_lm(*S.args(S.problem(name)), max_iterations=1, fixed_iterations=True,
                                       initial_lambda=lam)
    return _steps[name, lam]


def check_step(name, lam, cams1, pts1, what="", lam_step=None, oracle_iterations=1):
    """the eta bound on the step from the case's start to (cams1, pts1); returns the step"""
    p = S.rejected_problem() if name == "rejected" else S.problem(name)
    lam_step = lam if lam_step is None else lam_step
    dc, dp = S.step_of(p, cams1, pts1)
    m = S.measures(S.lin0(name), lam_step, dc, dp)
    mo = S.oracle_eta(name, lam, lam_step=lam_step, iterations=oracle_iterations)
    floor = S.cancellation(p, dc, dp)
    print(f"{name} lambda {lam_step:g} {what}: eta gpu {m['eta']:.3g} (camera rows {m['eta_cam']:.3g}, point rows "
          f"{m['eta_pt']:.3g}), oracle {mo['eta']:.3g} (camera rows {mo['eta_cam']:.3g}, point rows "
          f"{mo['eta_pt']:.3g}), eps max|x0| / max|delta| {floor:.3g}")
    assert m["stay"], "a camera or point without observations moved"
    assert m["eta"] <= FACTOR * max(mo["eta"], floor), (m, mo["eta"], floor)
    return dc, dp


# ------------------------------------------------------------------ 1. the step
@pytest.mark.parametrize("lam", S.LAMBDAS)
@pytest.mark.parametrize("name", list(S.CASES))
def test_step_solves_the_damped_normal_equations(core, name, lam):
    cams1, pts1, rep = gpu_step(core, name, lam)
    assert rep["accepted"] == 1 and rep["iterations"] == 1
    check_step(name, lam, cams1, pts1)


# ------------------------------------------------------------------ 2. the report
@pytest.mark.parametrize("lam", S.LAMBDAS)
@pytest.mark.parametrize("name", list(S.CASES))
def test_report_is_the_references_cost_and_gain_ratio(core, name, lam):
    p, L = S.problem(name), S.lin0(name)
    cams1, pts1, rep = gpu_step(core, name, lam)
    dc, dp = S.step_of(p, cams1, pts1)
    cost1 = S.Lin(p, cams1, pts1).cost
    rho = (L.cost - cost1) / L.model(lam, dc, dp)
    f = 1.0 - (2.0 * rho - 1.0) ** 3
    want = lam * max(1.0 / 3.0, f)
    print(f"{name} lambda {lam:g}: cost0 off {abs(rep['cost0'] - L.cost) / L.cost:.3g}, cost off "
          f"{abs(rep['cost'] - cost1) / cost1:.3g}, rho {rho:.6f}, lambda_ off {abs(rep['lambda_'] - want) / want:.3g}")
    assert abs(rep["cost0"] - L.cost) <= 1e-12 * L.cost
    assert abs(rep["cost"] - cost1) <= 1e-12 * cost1
    assert abs(rep["lambda_"] - want) <= 1e-8 * want


# ------------------------------------------------------------------ 3. a rejected step
def test_rejected_step_leaves_the_input_and_doubles_lambda(core):
    p, lam = S.rejected_problem(), S.REJECTED["lam"]
    cams1, pts1, rep = core.ba_lm(*S.args(p), max_iterations=1, fixed_iterations=True, initial_lambda=lam)
    assert (rep["iterations"], rep["accepted"]) == (1, 0)
    assert rep["lambda_"] == 2 * lam and rep["cost"] == rep["cost0"]
    assert np.array_equal(pts1, p["X0"]) and np.array_equal(cams1, p["cams0"])


def test_step_after_a_rejected_one_is_the_step_at_twice_the_damping(core):
    p, lam = S.rejected_problem(), S.REJECTED["lam"]
    cams2, pts2, rep = core.ba_lm(*S.args(p), max_iterations=2, fixed_iterations=True, initial_lambda=lam)
    assert (rep["iterations"], rep["accepted"]) == (2, 1)
    check_step("rejected", lam, cams2, pts2, "after a rejected step", lam_step=2 * lam, oracle_iterations=2)


# ------------------------------------------------------------------ 4. every path
@pytest.mark.parametrize("env,value", VARIANTS)
@pytest.mark.parametrize("name", ["odd33_skew", "hub"])
def test_step_under_every_switch(core, monkeypatch, name, env, value):
    monkeypatch.setenv(env, value)
    for lam in S.LAMBDAS:
        cams1, pts1, rep = core.ba_lm(*S.args(S.problem(name)), max_iterations=1, fixed_iterations=True,
                                      initial_lambda=lam)
        assert rep["accepted"] == 1
        check_step(name, lam, cams1, pts1, f"{env}={value}")


@pytest.mark.parametrize("value", ["0", "1"])
def test_step_of_the_pinhole_and_the_general_sweep(core, monkeypatch, value):
    monkeypatch.setenv("SFM_SWEEP_PINHOLE", value)
    for lam in S.LAMBDAS:
        cams1, pts1, rep = core.ba_lm(*S.args(S.problem("ragged7")), max_iterations=1, fixed_iterations=True,
                                      initial_lambda=lam)
        assert rep["accepted"] == 1
        check_step("ragged7", lam, cams1, pts1, f"SFM_SWEEP_PINHOLE={value}")


@pytest.mark.parametrize("name", ["ragged7_skew", "odd33_skew", "hub"])
def test_step_of_the_session_after_reset(core, name):
    prob = core.BAProblem(*S.args(S.problem(name)))
    try:
        for lam in S.LAMBDAS:
            rep = prob.solve(max_iterations=1, fixed_iterations=True, initial_lambda=lam)
            assert rep["accepted"] == 1
            check_step(name, lam, *prob.download(), "session")
            prob.reset()
    finally:
        prob.close()


@pytest.mark.parametrize("name", ["ragged7_skew", "odd33_skew", "hub", "two"])
def test_step_of_three_ranks_on_one_device(core, name):
    """the point shards of three in-process ranks: in "two" and ragged7 a rank's shard leaves cameras unobserved"""
    for lam in S.LAMBDAS:
        cams1, pts1, rep = core.ba_lm_multi(*S.args(S.problem(name)), [0, 0, 0], max_iterations=1,
                                            fixed_iterations=True, initial_lambda=lam)
        assert rep["accepted"] == 1 and rep["n_ranks"] == 3
        check_step(name, lam, cams1, pts1, "three ranks")


# ------------------------------------------------------------------ 5. to convergence
@pytest.mark.parametrize("name", ["ragged7_skew", "odd33_skew", "hub"])
def test_converges_as_the_oracle_does_on_ragged_input(core, name):
    p = S.problem(name)
    _, _, ro = O.ba_lm(*S.args(p), max_iterations=30, gtol=0.0)
    cams1, pts1, rg = core.ba_lm(*S.args(p), max_iterations=30)
    cost1 = S.Lin(p, cams1, pts1).cost
    print(f"{name}: {rg['iterations']} iterations, {rg['accepted']} accepted, status {rg['status']}; cost off the "
          f"oracle's {abs(rg['cost'] - ro['cost']) / ro['cost']:.3g}, off the returned parameters' "
          f"{abs(rg['cost'] - cost1) / cost1:.3g}")
    assert (rg["iterations"], rg["accepted"], rg["status"]) == (ro["iterations"], ro["accepted"], ro["status"])
    assert abs(rg["cost"] - ro["cost"]) <= 1e-7 * ro["cost"]
    assert abs(rg["cost"] - cost1) <= 1e-8 * cost1


# ------------------------------------------------------------------ 6. rejections
def still_usable(core):
    cams1, pts1, rep = core.ba_lm(*S.args(S.problem("ragged7")), max_iterations=1, fixed_iterations=True,
                                  initial_lambda=1.0)
    old = gpu_step(core, "ragged7", 1.0)
    assert rep["accepted"] == 1 and np.array_equal(cams1, old[0]) and np.array_equal(pts1, old[1])


def test_create_rejects_bad_observation_lists(core, monkeypatch):
    p = S.problem("ragged7")
    cams0, X0, ci, pi, obs, K = S.args(p)

    def fails(message, ci=ci, pi=pi, cams=cams0, obs=obs, **opts):
        with pytest.raises(core.SfmCoreError, match=message):
            core.ba_lm(cams, X0, ci, pi, obs, K, max_iterations=1, **opts)
        still_usable(core)
    swapped = pi.copy()
    swapped[[0, -1]] = swapped[[-1, 0]]
    fails("point-major", pi=swapped)
    for bad in (-1, p["n_pts"]):
        q = pi.copy()
        q[-1 if bad > 0 else 0] = bad
        fails("observation index out of range", pi=q)
    for bad in (-1, p["n_cams"]):
        c = ci.copy()
        c[5] = bad
        fails("observation index out of range", ci=c)
    twice = ci.copy()
    k = int(np.flatnonzero(pi[1:] == pi[:-1])[0])
    twice[k + 1] = twice[k]
    for host in ("0", "1"):
        monkeypatch.setenv("SFM_PLAN_HOST", host)
        fails("observed twice by the same camera", ci=twice)
    monkeypatch.delenv("SFM_PLAN_HOST")
    fails("at most 682 cameras", cams=np.zeros((683, 6)))
    fails("gradient_tolerance < 0", gradient_tolerance=-1.0)


def test_an_empty_problem_is_an_argument_error(core):
    """sfmcore.h: n_pts == 0 or n_obs == 0 is SFM_ERR_ARG (nothing to adjust)"""
    p = S.problem("ragged7")
    cams0, X0, ci, pi, obs, K = S.args(p)
    for X, c, q, o in ((X0, ci[:0], pi[:0], obs[:0]), (X0[:0], ci[:0], pi[:0], obs[:0])):
        cams = cams0.copy()
        with pytest.raises(core.SfmCoreError, match="nothing to adjust"):
            core.ba_lm(cams, X, c, q, o, K, max_iterations=1)
        assert np.array_equal(cams, cams0)
    still_usable(core)
