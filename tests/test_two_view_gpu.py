"""Two-view initialisation on a real MI355X: the fused kernel
(sfm_two_view_select) and the counting kernel (sfm_cheirality_count) against
the reference's results in tests/golden/two_view.npz.

Tolerances: triangulated points within the project's DLT bound (relative
error <= 1e-9, `rel` as in test_gpu_parity.py) of the reference's and of
sfm_triangulate_dlt's on the same device; counts and the selected index
exactly -- the fixture's generator asserts that every depth is at least 1e-6
of the scene's scale from zero, so no point is excluded from any count.
"""
import numpy as np
import pytest

import sfm_synthetic as syn
from test_two_view import CASE_NAMES, load_cases, numpy_counts

pytestmark = pytest.mark.gpu
K = syn.K_REF


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def cases():
    return load_cases()


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def projections(c):
    from sfm_two_view import projection
    P1 = projection(K, np.zeros(3), np.eye(3))
    return P1, np.stack([projection(K, C, R) for C, R in zip(c["Cset"], c["Rset"])])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_two_view_init_matches_reference(core, cases, name):
    from sfm_two_view import two_view_init
    c = cases[name]
    C, R, X, counts, best, X_all = two_view_init(c["F"], K, c["x1"], c["x2"], return_all=True)
    P1, P2s = projections(c)
    assert X_all.shape == c["X"].shape
    for m in range(4):
        r_ref = rel(X_all[m], c["X"][m])
        r_dlt = rel(X_all[m], core.triangulate(P1, P2s[m], c["x1"], c["x2"]))
        print(f"{name} candidate {m}: rel vs reference {r_ref:.3g}, vs sfm_triangulate_dlt {r_dlt:.3g}")
        assert r_ref <= 1e-9
        assert r_dlt <= 1e-9
    print(f"{name}: counts {counts} best {best}")
    assert counts.dtype == np.int64 and np.array_equal(counts, c["counts"])
    assert best == c["sel"]
    assert np.array_equal(X, X_all[best])
    assert np.abs(C - c["Cset"][c["sel"]]).max() <= 1e-9 and np.abs(R - c["Rset"][c["sel"]]).max() <= 1e-9


def test_two_view_init_without_return_all(core, cases):
    from sfm_two_view import two_view_init
    c = cases["p3"]
    out = two_view_init(c["F"], K, c["x1"], c["x2"])
    assert len(out) == 5 and out[4] == 2 and list(out[3]) == [0, 0, 7, 7]  # the tie goes to the earlier index
    assert rel(out[2], c["X"][2]) <= 1e-9


def test_two_view_select_edges(core, cases):
    c = cases["syn0_N65"]
    P1, P2s = projections(c)
    R1, C1 = np.eye(3), np.zeros(3)
    x1, x2 = c["x1"], c["x2"]
    # M = 1
    counts, best, X, X_all = core.two_view_select(P1, P2s[:1], R1, C1, c["Rset"][:1], c["Cset"][:1], x1, x2, True)
    assert list(counts) == [c["counts"][0]] and best == 0 and np.array_equal(X, X_all[0])
    assert rel(X, c["X"][0]) <= 1e-9
    # M = 2 identical candidates: the tie goes to the first
    two = [0, 0]
    counts, best, X, X_all = core.two_view_select(P1, P2s[two], R1, C1, c["Rset"][two], c["Cset"][two], x1, x2, True)
    assert list(counts) == [c["counts"][0]] * 2 and best == 0 and np.array_equal(X_all[0], X_all[1])
    # M = 8: the four candidates in reverse, twice
    ids = [3, 2, 1, 0, 3, 2, 1, 0]
    counts, best, X, X_all = core.two_view_select(P1, P2s[ids], R1, C1, c["Rset"][ids], c["Cset"][ids], x1, x2, True)
    assert np.array_equal(counts, c["counts"][ids]) and best == 3  # candidate 0 sits at 3 and 7
    assert np.array_equal(X, X_all[3]) and np.array_equal(X_all[:4], X_all[4:])
    for k, m in enumerate(ids):
        assert rel(X_all[k], c["X"][m]) <= 1e-9
    # a camera 1 that is not at the origin: its depth enters the count
    counts, _, _, X_all = core.two_view_select(P1, P2s, R1, np.array([0.0, 0.0, 8.0]), c["Rset"], c["Cset"], x1, x2, True)
    want = [int(np.sum((Xm[:, 2] - 8.0 > 0) & (((Xm - Cm) @ Rm.T)[:, 2] > 0)))
            for Xm, Cm, Rm in zip(X_all, c["Cset"], c["Rset"])]
    assert list(counts) == want and want != list(c["counts"])
    # N = 0
    counts, best, X, X_all = core.two_view_select(P1, P2s, R1, C1, c["Rset"], c["Cset"], x1[:0], x2[:0], True)
    assert list(counts) == [0, 0, 0, 0] and best == 0 and X.shape == (0, 3) and X_all.shape == (4, 0, 3)
    # M outside 1..8
    for ids in ([], [0, 1, 2, 3, 0, 1, 2, 3, 0]):
        with pytest.raises(core.SfmCoreError, match="argument"):
            core.two_view_select(P1, P2s[ids], R1, C1, c["Rset"][ids], c["Cset"][ids], x1, x2)
        with pytest.raises(core.SfmCoreError, match="argument"):
            core.cheirality_count(R1, C1, c["Rset"][ids], c["Cset"][ids], c["X"][ids])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cheirality_count_matches_reference(core, cases, name):
    c = cases[name]
    counts, best = core.cheirality_count(np.eye(3), np.zeros(3), c["Rset"], c["Cset"], c["X"])
    assert np.array_equal(counts, c["counts"]) and best == c["sel"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_disambiguate_matches_reference(core, cases, name, capsys):
    from DisambiguateCameraPose import DisambiguateCameraPose
    c = cases[name]
    for Xset in (list(c["X"]), c["X"]):  # a list or an array
        C, R, X = DisambiguateCameraPose(c["Cset"], c["Rset"], Xset)
        assert capsys.readouterr().out == c["line"] + "\n"
        assert np.array_equal(C, c["Cset"][c["sel"]]) and np.array_equal(R, c["Rset"][c["sel"]])
        assert np.array_equal(X, c["X"][c["sel"]])
        assert not np.shares_memory(X, c["X"]) and not np.shares_memory(C, c["Cset"])


def test_disambiguate_skips_empty_and_mixed_lengths(core, cases, capsys):
    from DisambiguateCameraPose import DisambiguateCameraPose
    c = cases["syn0_N257"]
    msg = "Selected camera pose configuration {} with {} points in front of both cameras\n"
    # an empty first candidate is skipped
    Xset = [np.zeros((0, 3))] + list(c["X"][1:])
    C, R, X = DisambiguateCameraPose(c["Cset"], c["Rset"], Xset)
    counts, sel = numpy_counts(c["Cset"], c["Rset"], Xset)
    assert sel == 1 and counts[1] == c["counts"][1] > 0
    assert capsys.readouterr().out == msg.format(1, counts[1])
    assert np.array_equal(C, c["Cset"][1]) and np.array_equal(R, c["Rset"][1]) and np.array_equal(X, c["X"][1])
    # candidates of unequal length are counted in separate calls
    Xset = [c["X"][0][:20], c["X"][1], c["X"][2][:70], c["X"][3]]
    C, R, X = DisambiguateCameraPose(c["Cset"], c["Rset"], Xset)
    counts, sel = numpy_counts(c["Cset"], c["Rset"], Xset)
    assert capsys.readouterr().out == msg.format(sel, counts[sel])
    assert np.array_equal(C, c["Cset"][sel]) and np.array_equal(X, Xset[sel])
    # nothing to count: the reference's warning and candidate 0
    C, R, X = DisambiguateCameraPose(c["Cset"], c["Rset"], [[], [], [], []])
    assert capsys.readouterr().out == "Warning: No valid camera pose found, using first configuration\n"
    assert np.array_equal(C, c["Cset"][0]) and np.array_equal(R, c["Rset"][0]) and len(X) == 0


def test_two_view_select_is_deterministic(core, cases):
    c = cases["syn1_N1025"]
    P1, P2s = projections(c)
    runs = [core.two_view_select(P1, P2s, np.eye(3), np.zeros(3), c["Rset"], c["Cset"], c["x1"], c["x2"], True)
            for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert np.array_equal(runs[0][3], runs[1][3]) and np.array_equal(runs[0][2], runs[1][2])
