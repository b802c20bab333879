"""Guided descriptor matching on a real MI355X (sfm_match_descriptors_guided,
sfm_io.match_descriptors_guided, sfm_multiview.rematch_verified) against the
plain-numpy restatement of tests/test_match_guided.py and
tests/golden/match_guided.npz.  The distances are integers and the gate is
defined operation by operation in fp64, so every output is compared for
equality, dtype and shape included; there are no tolerances.  The last test
reaches the kernels' pair stride: the 65,535 + 600 pairs of tests/fast_refs.py
with an F of its own per pair and a finite gate, so that 600 workgroups reload
F, the row terms and the candidate counters for a second pair, against the
vectorised restatement there (equal to the plain one wherever
tests/test_fast_refs.py can afford the plain one).
"""
import numpy as np
import pytest

import fast_refs as fr
import test_match_descriptors as md
import test_match_guided as mg
from test_match_descriptors import INT32_MAX

pytestmark = pytest.mark.gpu
T = 64    # the kernel's column tile (MD_TN of csrc/match_common.hpp)
BM = 128  # the rows of one workgroup at dim 64 and 128 (md_bm); 64 at dim 256


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


def check(core, descs, kps, pairs, F, gate, ratio=0.8, max_dsq=INT32_MAX, cross_check=True):
    """the device call, at the capacity bound, against the restatement; returns the restatement"""
    desc, img_start = md.pack(descs)
    xy = np.concatenate([np.zeros((0, 2))] + list(kps))
    out = core.match_descriptors_guided(desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross_check,
                                        want_diagnostics=True)
    ref = mg.restate_guided(desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross_check)
    md.same(out, ref, mg.OUTPUTS)
    return ref


SIZES = [(1, 1), (1, 2), (2, 1), (17, 15), (64, 64), (65, 130), (130, 65), (300, 257)]


@pytest.mark.parametrize("dim", [64, 128, 256])
@pytest.mark.parametrize("ni,nj", SIZES)
def test_one_pair_of_random_descriptors(core, ni, nj, dim):
    rng = np.random.default_rng(1000 * ni + 10 * nj + dim)
    descs = [rng.integers(0, 256, (ni, dim)).astype(np.uint8), rng.integers(0, 256, (nj, dim)).astype(np.uint8)]
    kps = [mg.frame_points(rng, ni), mg.frame_points(rng, nj)]
    F = mg.random_rank2(rng)
    gate = mg.gate_with_all_three(F, kps[0], kps[1])
    if ni >= 17:
        assert gate is not None  # a condition on the inputs, decided by the restatement alone
    elif gate is None:
        gate = float(np.median(mg.sampson(F, kps[0], kps[1])))
    ref = check(core, descs, kps, [(0, 1)], [F], gate, ratio=1.0, cross_check=False)
    if ni >= 17:
        n = ref["n_cand"]
        assert (n == 0).any() and (n == 1).any() and (n >= 2).any()
    check(core, descs, kps, [(0, 1)], [F], gate, ratio=0.97, cross_check=True)


def on_line(line, u):
    """v with line . (u, v, 1) = 0"""
    return -(line[0] * u + line[2]) / line[1]


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_tile_and_workgroup_boundaries(core, dim):
    """one descriptor of j at columns 3, 3 + T and N_j - 1 (three column tiles) and a copy of it in row 5 of i, of
    which only the middle column lies inside row 5's band; the same on the i side for nn_rev (rows 3, 3 + BM and
    N_i - 1, three workgroups, only the middle row inside column 7's band)"""
    rng = np.random.default_rng(5 + dim)
    ni, nj, gate = 2 * BM + 9, 2 * T + 21, 4.0
    F = mg.fundamental(np.eye(3), np.zeros(3), mg.rot_y(0.1), np.array([1.0, 0.05, 0.1]))
    a, b = rng.integers(0, 256, (ni, dim)).astype(np.uint8), rng.integers(0, 256, (nj, dim)).astype(np.uint8)
    xa, xb = mg.frame_points(rng, ni), mg.frame_points(rng, nj)
    b[3 + T] = b[nj - 1] = b[3]
    a[5] = b[3]
    line = F @ np.array([xa[5, 0], xa[5, 1], 1.0])  # row 5's epipolar line in j
    xb[3 + T, 1] = on_line(line, xb[3 + T, 0])
    xb[10, 1] = on_line(line, xb[10, 0])            # a non-duplicate inside the band: row 5's d2
    for c in (3, nj - 1):
        xb[c, 1] = on_line(line, xb[c, 0]) + 60.0
    a[3 + BM] = a[ni - 1] = a[3]
    b[7] = a[3]
    back = F.T @ np.array([xb[7, 0], xb[7, 1], 1.0])  # column 7's epipolar line in i
    xa[3 + BM, 1] = on_line(back, xa[3 + BM, 0])
    for r in (3, ni - 1):
        xa[r, 1] = on_line(back, xa[r, 0]) - 60.0
    ref = check(core, [a, b], [xa, xb], [(0, 1)], [F], gate, ratio=1.0, cross_check=False)
    assert ref["nn"][5] == 3 + T and ref["d1"][5] == 0 and 0 < ref["d2"][5] < INT32_MAX
    assert ref["nn_rev"][7] == 3 + BM
    plain = md.restate(*md.pack([a, b]), [(0, 1)], 1.0, INT32_MAX, False)
    assert plain["nn"][5] == 3 and plain["d2"][5] == 0 and plain["nn_rev"][7] == 3
    check(core, [a, b], [xa, xb], [(0, 1), (1, 0)], [F, F.T], gate, ratio=1.0, cross_check=True)
    # columns past N_j and rows past N_i are never counted: with every pair admitted n_cand is N_j exactly
    ref = check(core, [a, b], [xa, xb], [(0, 1), (1, 0)], [F, F.T], 1e200, ratio=1.0, cross_check=False)
    assert ref["n_cand"].tolist() == [nj] * ni + [ni] * nj


def test_borderline_pairs_decision_for_decision(core):
    """the fixture's pairs on the threshold curve: a fused multiply-add, another grouping of den or a loose
    prefilter changes n_cand or nn here"""
    fx = mg.fixture()
    desc, xy, img_start, pairs, F = (fx[f"border_{k}"] for k in ("desc", "xy", "img_start", "pairs", "F"))
    gate = float(fx["border_gate"])
    out = core.match_descriptors_guided(desc, xy, img_start, pairs, F, gate, 1.0, INT32_MAX, True,
                                        want_diagnostics=True)
    md.same(out, {n: fx[f"border_{n}"] for n in mg.OUTPUTS}, mg.OUTPUTS)
    # the same pairs the other way round: the columns become the rows
    ref = mg.restate_guided(desc, xy, img_start, [(1, 0)], F.transpose(0, 2, 1), gate, 1.0, INT32_MAX, True)
    out = core.match_descriptors_guided(desc, xy, img_start, [(1, 0)], F.transpose(0, 2, 1), gate, 1.0, INT32_MAX,
                                        True, want_diagnostics=True)
    md.same(out, ref, mg.OUTPUTS)


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_all_admitting_gate_equals_the_unguided_call(core, dim):
    rng = np.random.default_rng(40 + dim)
    sizes = (150, 37, 0, 1, 260)
    descs = [rng.integers(0, 256, (n, dim)).astype(np.uint8) for n in sizes]
    kps = [mg.frame_points(rng, n) for n in sizes]
    pairs = [(0, 1), (1, 0), (0, 2), (3, 0), (4, 1), (0, 4)]
    F = np.array([mg.random_rank2(rng) for _ in pairs])
    desc, img_start = md.pack(descs)
    xy = np.concatenate(kps)
    n = np.diff(img_start)
    for cross in (False, True):
        out = core.match_descriptors_guided(desc, xy, img_start, pairs, F, 1e200, 0.9, INT32_MAX, cross,
                                            want_diagnostics=True)
        md.same(out, core.match_descriptors(desc, img_start, pairs, 0.9, INT32_MAX, cross, want_diagnostics=True))
        assert np.array_equal(out["n_cand"], np.concatenate([np.full(n[i], n[j], np.int32) for i, j in pairs]))


def unequal_scene(dim=128, sizes=(150, 37, 0, 1, 260), seed=3):
    rng = np.random.default_rng(seed)
    descs = [rng.integers(0, 256, (n, dim)).astype(np.uint8) for n in sizes]
    return descs, [mg.frame_points(rng, n) for n in sizes], rng


def test_multi_pair_call_is_pair_major_and_equals_single_pair_calls(core):
    descs, kps, rng = unequal_scene()
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (0, 3), (3, 4), (4, 0), (0, 4)]
    F = np.array([mg.random_epipolar(rng) for _ in pairs])
    F[6, 2, 0] = np.nan
    desc, img_start = md.pack(descs)
    xy = np.concatenate(kps)
    for cross in (False, True):
        whole = check(core, descs, kps, pairs, F, 15.0, 0.95, INT32_MAX, cross)
        assert whole["match_start"][6] == whole["match_start"][7]  # the NaN F: no match
        assert whole["match_start"][-1] > 0 and (whole["n_cand"] >= 2).any()
        lo = dict(m=0, i=0, j=0)
        for p, (i, j) in enumerate(pairs):
            one = core.match_descriptors_guided(desc, xy, img_start, [(i, j)], F[p:p + 1], 15.0, 0.95, INT32_MAX, cross,
                                                want_diagnostics=True)
            m, ni, nj = len(one["a"]), len(descs[i]), len(descs[j])
            assert whole["match_start"][p] == lo["m"] and whole["match_start"][p + 1] == lo["m"] + m
            for k in ("a", "b", "dsq"):
                assert np.array_equal(whole[k][lo["m"]:lo["m"] + m], one[k]), (p, k)
            for k in ("nn", "d1", "d2", "n_cand"):
                assert np.array_equal(whole[k][lo["i"]:lo["i"] + ni], one[k]), (p, k)
            assert np.array_equal(whole["nn_rev"][lo["j"]:lo["j"] + nj], one["nn_rev"]), p
            if cross:
                assert np.array_equal(one["nn_rev"][one["b"]], one["a"])
            assert np.all(np.diff(one["a"]) > 0)  # ascending a inside a pair
            lo = dict(m=lo["m"] + m, i=lo["i"] + ni, j=lo["j"] + nj)


def test_capacity_at_the_bound_null_diagnostics_and_repeat_calls(core):
    """identical images under an all-admitting gate: every keypoint matches itself, so the matches fill the bound"""
    rng = np.random.default_rng(9)
    d = rng.integers(0, 256, (140, 64)).astype(np.uint8)
    x = mg.frame_points(rng, 140)
    F = np.array([mg.random_rank2(rng), mg.random_rank2(rng)])
    for cross in (False, True):
        ref = check(core, [d, d.copy(), d[:60].copy()], [x, x, x[:60]], [(0, 1), (2, 0)], F, 1e200, 1.0, INT32_MAX, cross)
        assert ref["match_start"].tolist() == [0, 140, 200] and (ref["dsq"] == 0).all()
        assert ref["a"].tolist() == list(range(140)) + list(range(60)) and np.array_equal(ref["a"], ref["b"])
    rc, outs = mg.raw_call(core, np.concatenate([d[:30], d[:30]]), np.concatenate([x[:30], x[:30]]), [0, 30, 60],
                           [(0, 1)], F[:1], gate=1e200, ratio=1.0, capacity=30,
                           null=("nn", "d1", "d2", "nn_rev", "n_cand"))
    assert rc == 0 and outs["match_start"][:2].tolist() == [0, 30] and outs["a"][:30].tolist() == list(range(30))
    assert (outs["a"][30:] == -7).all()
    assert all((outs[k] == -7).all() for k in ("nn", "d1", "d2", "nn_rev", "n_cand"))
    # two calls, another one in between on the same buffers
    descs, kps, rng = unequal_scene(sizes=(300, 257, 129), seed=8)
    desc, img_start = md.pack(descs)
    xy = np.concatenate(kps)
    pairs = [(0, 1), (1, 2), (2, 0)]
    F = np.array([mg.random_epipolar(rng) for _ in pairs])
    first = core.match_descriptors_guided(desc, xy, img_start, pairs, F, 10.0, 0.9, INT32_MAX, True, want_diagnostics=True)
    core.match_descriptors_guided(desc[::-1].copy(), xy[::-1].copy(), img_start, pairs, F, 25.0, 0.9, INT32_MAX, True)
    again = core.match_descriptors_guided(desc, xy, img_start, pairs, F, 10.0, 0.9, INT32_MAX, True, want_diagnostics=True)
    md.same(first, again, mg.OUTPUTS)
    md.same(first, mg.restate_guided(desc, xy, img_start, pairs, F, 10.0, 0.9, INT32_MAX, True), mg.OUTPUTS)


def test_fixture_scenes(core):
    fx = mg.fixture()
    for tag, desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross in mg.fixture_cases():
        out = core.match_descriptors_guided(desc, xy, img_start, pairs, F, gate, ratio, max_dsq, bool(cross),
                                            want_diagnostics=True)
        md.same(out, {n: fx[f"{tag}_{n}"] for n in mg.OUTPUTS}, mg.OUTPUTS)


def test_a_workgroup_takes_a_second_pair_with_another_F(core):
    """gridDim.y is 65,535, so the workgroups of pairs 0 .. 599 go on to pairs 65,535 .. 66,134, of other shapes
    (tests/test_fast_refs.py asserts the table) and each with an F of its own under a finite gate: an F, row terms
    or candidate counters left over from the workgroup's first pair change n_cand, and with it nn, of the second"""
    s = fr.wrap_scene(64)
    ref = fr.match_guided(s["desc"], s["xy"], s["img_start"], s["pairs"], s["F"], fr.GUIDED_GATE, 0.8,
                          fr.wrap_limit(64), True)
    # conditions on the inputs, from the restatement alone
    ni, nj = s["shape"][:, 0], s["shape"][:, 1]
    pair = np.repeat(np.arange(len(ni)), ni)
    short = np.bincount(pair, weights=ref["n_cand"] < nj[pair], minlength=len(ni))  # rows with a candidate refused
    some = np.bincount(pair, weights=ref["n_cand"] > 0, minlength=len(ni))
    busy = (ni > 0) & (nj > 0)
    wrapped = np.arange(len(ni)) >= fr.WRAP
    assert (wrapped & busy & (short > 0) & (some > 0)).sum() > 100  # wrapped pairs with candidates refused ...
    assert (wrapped & busy & (short == 0)).sum() >= 5               # ... and with every candidate admitted
    per = np.diff(ref["match_start"])
    assert (per[fr.WRAP:] > 0).sum() > 50 and ((per[fr.WRAP:] == 0) & busy[fr.WRAP:]).sum() > 50
    assert 0 < ref["match_start"][fr.WRAP] < ref["match_start"][-1]
    lo = int(ni[:s["nan_pair"]].sum())
    assert ni[s["nan_pair"]] > 0 and (ref["n_cand"][lo:lo + ni[s["nan_pair"]]] == 0).all()  # the F with a NaN
    out = core.match_descriptors_guided(s["desc"], s["xy"], s["img_start"], s["pairs"], s["F"], fr.GUIDED_GATE, 0.8,
                                        fr.wrap_limit(64), True, want_diagnostics=True)
    md.same(out, ref, mg.OUTPUTS)


def test_twins_are_recovered_through_the_python_layer(core):
    """4 views of 60 points, five pairs of which share a descriptor: the unguided call loses the twins to the
    ratio test, rematch_verified with the scene's F finds every true match, and the tracks are the scene points
    (the counts are those of test_match_guided.test_twin_scene_counts)"""
    from sfm_io import match_descriptors
    from sfm_multiview import rematch_verified, verify_pairs
    s = mg.twin_reference()
    kps, descs, pairs, F = s["keypoints"], s["descriptors"], s["pairs"], s["F"]
    store, pair_ij, match_start, a, b, dsq = match_descriptors(kps, descs, ratio=s["ratio"])
    md.same(dict(match_start=match_start, a=a, b=b, dsq=dsq), s["plain"], ("match_start", "a", "b", "dsq"))
    plain = mg.matches_of(dict(match_start=match_start, a=a, b=b), pair_ij)
    twins = set(range(2 * mg.TWINS))
    assert len(plain) == 6 * 50 and not any(m[1] in twins for m in plain)
    # verify_pairs' tuple with the scene's own F: (order, pair_ij, (F, cost, n_inliers, ..., info), index1, index2)
    vout = (F, None, np.full(6, 50, np.int32), None, None, None, np.zeros(6, np.int32))
    verified = (np.arange(6), pairs, vout, None, None)
    gstore, gpair_ij, gms, ga, gb, gdsq = rematch_verified(kps, descs, verified, threshold=s["threshold"],
                                                            ratio=s["ratio"])
    assert np.array_equal(gpair_ij, pairs)
    md.same(dict(match_start=gms, a=ga, b=gb, dsq=gdsq), s["guided"], ("match_start", "a", "b", "dsq"))
    guided = mg.matches_of(dict(match_start=gms, a=ga, b=gb), gpair_ij)
    assert guided == {(int(i), n, int(j), n) for i, j in pairs for n in range(60)} and plain <= guided
    # one track per scene point, seen by all four views
    merged, row_track, obs_map = gstore.merge_tracks()
    assert merged.n_features == 60 and len(merged) == 240
    assert np.array_equal(merged.image.reshape(60, 4), np.tile(np.arange(4, dtype=np.int32), (60, 1)))
    where = {(k, float(x), float(y)): n for k in range(4) for n, (x, y) in enumerate(kps[k])}
    for t in range(60):
        pts = {where[(int(merged.image[o]), merged.x[o], merged.y[o])] for o in range(4 * t, 4 * t + 4)}
        assert len(pts) == 1
    short, _, _ = store.merge_tracks()
    assert short.n_features == 50
    # failed and weak pairs are left out, and verify_pairs accepts the guided store as it is
    vout = (F, None, np.array([50, 50, 3, 50, 50, 50], np.int32), None, None, None,
            np.array([0, -2, 0, 0, 1, 0], np.int32))
    part = rematch_verified(kps, descs, (np.arange(6), pairs, vout, None, None), threshold=s["threshold"], min_inliers=8)
    assert np.array_equal(part[1], pairs[[0, 3, 4, 5]]) and len(part[3]) == 4 * 60
    order, vp_ij, out, index1, index2 = verify_pairs(gstore, H=64)
    assert np.array_equal(vp_ij, pairs) and len(index1) == len(ga)
