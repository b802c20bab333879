"""Descriptor matching on a real MI355X (sfm_match_descriptors,
sfm_io.match_descriptors) against the plain-numpy restatement of
tests/test_match_descriptors.py and tests/golden/match_descriptors.npz.
Integer work with an exact answer: every output is compared for equality, dtype
and shape included; there are no tolerances.  Uniform random bytes are
asymmetric data, so a swapped row or column or a k order that differs between
the two MFMA operands cannot pass.  The last test reaches the kernels' pair
stride: 65,535 + 600 pairs, so that 600 workgroups of k_md_nn, k_md_accept and
k_md_write take a second pair of another shape than their first, against the
vectorised restatement of tests/fast_refs.py (equal to the plain one wherever
tests/test_fast_refs.py can afford the plain one).
"""
import functools

import numpy as np
import pytest

import fast_refs as fr
import test_match_descriptors as md
from test_match_descriptors import INT32_MAX

pytestmark = pytest.mark.gpu
T = 64    # the kernel's column tile (MD_TN of csrc/match_common.hpp)
BM = 128  # the rows of one workgroup (md_bm)


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


def check(core, descs, pairs, ratio=0.8, max_dsq=INT32_MAX, cross_check=True):
    """the device call, at the capacity bound, against the restatement; returns the restatement"""
    desc, img_start = md.pack(descs)
    out = core.match_descriptors(desc, img_start, pairs, ratio, max_dsq, cross_check, want_diagnostics=True)
    ref = md.restate(desc, img_start, pairs, ratio, max_dsq, cross_check)
    md.same(out, ref)
    return ref


SIZES = [(1, 1), (2, 1), (1, 2), (15, 17), (16, 16), (17, 15), (63, 65), (64, 64), (65, 130), (130, 65), (300, 257)]


@pytest.mark.parametrize("dim", [64, 128, 256])
@pytest.mark.parametrize("ni,nj", SIZES)
def test_one_pair_of_random_descriptors(core, ni, nj, dim):
    rng = np.random.default_rng(1000 * ni + 10 * nj + dim)
    descs = [rng.integers(0, 256, (ni, dim)).astype(np.uint8), rng.integers(0, 256, (nj, dim)).astype(np.uint8)]
    check(core, descs, [(0, 1)], ratio=1.0, cross_check=False)
    check(core, descs, [(0, 1)], ratio=0.97, cross_check=True)


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_bias_and_extremes(core, dim):
    rng = np.random.default_rng(dim)
    values = np.array([0, 127, 128, 255], dtype=np.uint8)
    descs = [values[rng.integers(0, 4, (n, dim))] for n in (70, 90)]
    ref = check(core, descs, [(0, 1), (1, 0)], ratio=1.0, cross_check=False)
    assert ref["d1"].max() > 255 * 255
    # all 0 against all 255: dim * 255^2 in every entry (16,646,400 at dim 256), ties everywhere
    far = [np.zeros((33, dim), np.uint8), np.full((20, dim), 255, np.uint8)]
    ref = check(core, far, [(0, 1), (1, 0)], ratio=1.0, cross_check=False)
    assert (ref["d1"] == dim * 255 * 255).all() and (ref["d2"] == dim * 255 * 255).all() and (ref["nn"] == 0).all()
    assert len(ref["a"]) == 0
    one = [np.zeros((33, dim), np.uint8), np.full((1, dim), 255, np.uint8)]
    ref = check(core, one, [(0, 1)], ratio=0.5, cross_check=True)
    assert ref["a"].tolist() == [0] and ref["dsq"].tolist() == [dim * 255 * 255]


@pytest.mark.parametrize("dim", [64, 128])
def test_ties_across_tile_boundaries(core, dim):
    """one descriptor of j at columns 3, 3 + T and N_j - 1 (three column tiles), and a copy of it in i: nn is 3
    and d2 == d1 == 0; the same on the i side (rows 3, 3 + BM and N_i - 1, three workgroups) for nn_rev"""
    rng = np.random.default_rng(5 + dim)
    ni, nj = 2 * BM + 9, 2 * T + 21
    a, b = rng.integers(0, 256, (ni, dim)).astype(np.uint8), rng.integers(0, 256, (nj, dim)).astype(np.uint8)
    b[3 + T] = b[nj - 1] = b[3]
    a[5] = b[3]
    a[3 + BM] = a[ni - 1] = a[3]
    b[7] = a[3]
    ref = check(core, [a, b], [(0, 1)], ratio=1.0, cross_check=False)
    assert ref["nn"][5] == 3 and ref["d1"][5] == 0 and ref["d2"][5] == 0
    assert ref["nn_rev"][7] == 3 and ref["nn"][3] == ref["nn"][3 + BM] == ref["nn"][ni - 1] == 7
    ref = check(core, [a, b], [(0, 1), (1, 0)], ratio=1.0, cross_check=True)
    assert 3 in ref["a"][:ref["match_start"][1]].tolist() and (3 + BM) not in ref["a"][:ref["match_start"][1]].tolist()
    # near ties: a second candidate one unit further in a later tile must stay second
    b2 = b.copy()
    b2[3 + T] = b2[3]
    b2[3 + T, 0] ^= 1
    b2[nj - 1, 1] ^= 1
    ref = check(core, [a, b2], [(0, 1)], ratio=1.0, cross_check=False)
    assert ref["nn"][5] == 3 and ref["d2"][5] == 1


def unequal_images(dim=128, sizes=(150, 37, 0, 1, 260), seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (n, dim)).astype(np.uint8) for n in sizes]


def test_empty_and_one_keypoint_images_inside_a_multi_pair_call(core):
    descs = unequal_images()
    pairs = [(0, 2), (2, 0), (0, 3), (3, 0), (2, 3), (3, 2), (4, 1), (3, 4)]
    ref = check(core, descs, pairs, ratio=0.9, cross_check=True)
    # (0, 3): one candidate, so the ratio test is passed and the cross-check keeps one of the 150; (3, 0) has a
    # second neighbour and is left to the ratio test
    per_pair = np.diff(ref["match_start"]).tolist()
    assert per_pair[:3] == [0, 0, 1] and per_pair[3] <= 1 and per_pair[4:6] == [0, 0]
    check(core, descs, pairs, ratio=1.0, cross_check=False)
    check(core, [descs[2], descs[2]], [(0, 1)], ratio=1.0, cross_check=True)  # nothing at all on either side


def test_multi_pair_call_is_pair_major_and_equals_single_pair_calls(core):
    descs = unequal_images(sizes=(150, 37, 90, 260))
    pairs = [(0, 1), (1, 0), (0, 2), (3, 1)]
    desc, img_start = md.pack(descs)
    for cross in (False, True):
        whole = core.match_descriptors(desc, img_start, pairs, 0.95, INT32_MAX, cross, want_diagnostics=True)
        md.same(whole, md.restate(desc, img_start, pairs, 0.95, INT32_MAX, cross))
        lo = dict(m=0, i=0, j=0)
        for p, (i, j) in enumerate(pairs):
            one = core.match_descriptors(desc, img_start, [(i, j)], 0.95, INT32_MAX, cross, want_diagnostics=True)
            m, ni, nj = len(one["a"]), len(descs[i]), len(descs[j])
            assert whole["match_start"][p] == lo["m"] and whole["match_start"][p + 1] == lo["m"] + m
            for k in ("a", "b", "dsq"):
                assert np.array_equal(whole[k][lo["m"]:lo["m"] + m], one[k]), (p, k)
            for k in ("nn", "d1", "d2"):
                assert np.array_equal(whole[k][lo["i"]:lo["i"] + ni], one[k]), (p, k)
            assert np.array_equal(whole["nn_rev"][lo["j"]:lo["j"] + nj], one["nn_rev"]), p
            lo = dict(m=lo["m"] + m, i=lo["i"] + ni, j=lo["j"] + nj)
        assert np.all(np.diff(whole["a"][:whole["match_start"][1]]) > 0)  # ascending a inside a pair


@pytest.mark.parametrize("cross_check", [0, 1])
@pytest.mark.parametrize("ratio", [1.0, 0.8])
def test_parameter_settings(core, cross_check, ratio):
    keypoints, descs, _ = md.synthetic_scene(seed=21)
    descs = descs + [np.random.default_rng(4).integers(0, 256, (50, 128)).astype(np.uint8)]
    pairs = [(0, 1), (2, 3), (3, 0), (1, 4), (4, 2)]
    desc, img_start = md.pack(descs)
    d1 = md.restate(desc, img_start, pairs, 1.0, INT32_MAX, False)["d1"]
    mid = int(np.median(d1))  # half of the nearest neighbours pass it
    counts = []
    for max_dsq in (0, mid, INT32_MAX):
        ref = check(core, descs, pairs, ratio, max_dsq, bool(cross_check))
        counts.append(len(ref["a"]))
    assert counts[0] == 0 and 0 < counts[1] <= counts[2]
    # the diagnostics are optional, and capacity may be larger than the bound
    plain = core.match_descriptors(desc, img_start, pairs, ratio, mid, bool(cross_check), capacity=5000)
    md.same(plain, md.restate(desc, img_start, pairs, ratio, mid, bool(cross_check)), ("match_start", "a", "b", "dsq"))


def test_capacity_exactly_at_the_bound_is_filled(core):
    """identical images: every keypoint matches itself, so the matches fill the bound exactly"""
    rng = np.random.default_rng(9)
    d = rng.integers(0, 256, (140, 64)).astype(np.uint8)
    for cross in (False, True):
        ref = check(core, [d, d.copy(), d[:60].copy()], [(0, 1), (2, 0)], ratio=1.0, cross_check=cross)
        assert ref["match_start"].tolist() == [0, 140, 200] and (ref["dsq"] == 0).all()
        assert ref["a"].tolist() == list(range(140)) + list(range(60)) and np.array_equal(ref["a"], ref["b"])
    rc, outs = md.raw_call(core, np.concatenate([d[:30], d[:30]]), [0, 30, 60], [(0, 1)], ratio=1.0, capacity=30,
                           null=("nn", "d1", "d2", "nn_rev"))
    assert rc == 0 and outs["match_start"][:2].tolist() == [0, 30] and outs["a"][:30].tolist() == list(range(30))
    assert (outs["a"][30:] == -7).all() and (outs["nn"] == -7).all()


def test_two_calls_give_identical_outputs(core):
    descs = unequal_images(sizes=(300, 257, 129), seed=8)
    desc, img_start = md.pack(descs)
    pairs = [(0, 1), (1, 2), (2, 0)]
    first = core.match_descriptors(desc, img_start, pairs, 0.9, INT32_MAX, True, want_diagnostics=True)
    other = core.match_descriptors(desc[::-1].copy(), img_start, pairs, 0.9, INT32_MAX, True)  # the buffers reused
    again = core.match_descriptors(desc, img_start, pairs, 0.9, INT32_MAX, True, want_diagnostics=True)
    md.same(first, again)
    assert len(other["a"]) <= 257 + 129 + 129


def test_synthetic_scene_through_the_python_layer(core):
    from sfm_io import match_descriptors
    from sfm_multiview import verify_pairs
    s = md.synthetic_reference()
    store, pair_ij, match_start, a, b, dsq = match_descriptors(s["keypoints"], s["descriptors"])
    assert np.array_equal(pair_ij, s["pairs"]) and pair_ij.dtype == np.int64
    md.same(dict(match_start=match_start, a=a, b=b, dsq=dsq), s["ref"], ("match_start", "a", "b", "dsq"))
    for n in ("feature", "image", "x", "y", "flag"):
        got, want = getattr(store, n), s["arrays"][n]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), n
    assert store.n_features == len(a) and store.n_images == 4 and np.array_equal(store._row_start, s["row_start"])
    merged, row_track, obs_map = store.merge_tracks()
    for n in ("feature", "image", "x", "y", "flag"):
        assert np.array_equal(getattr(merged, n), s["merged"][n]), n
    assert np.array_equal(row_track, s["merged"]["row_track"]) and np.array_equal(obs_map, s["merged"]["obs_map"])
    assert np.array_equal(merged._row_start, s["tracks"]["track_start"])
    # verify_pairs accepts either store
    for st in (store, merged):
        order, vp_ij, out, index1, index2 = verify_pairs(st, H=64)
        assert np.array_equal(vp_ij, s["pairs"]) and len(order) == 6 and out[0].shape == (6, 3, 3)
        assert st is merged or len(index1) == len(s["ref"]["a"])  # one correspondence per match


def test_fixture_scenes(core):
    fx = md.fixture()
    for tag, desc, img_start, pairs, ratio, max_dsq, cross in md.fixture_cases():
        out = core.match_descriptors(desc, img_start, pairs, ratio, max_dsq, bool(cross), want_diagnostics=True)
        md.same(out, {n: fx[f"{tag}_{n}"] for n in md.OUTPUTS})


@functools.lru_cache(maxsize=None)
def wrap_neighbours(dim):
    """the 66,135-pair scene of tests/fast_refs.py and what precedes the tests, once per dim"""
    s = fr.wrap_scene(dim)
    return s, fr.match_neighbours(s["desc"], s["img_start"], s["pairs"])


def wrap_conditions(s, ref):
    """what the scene must show for the comparison to mean something, from the restatement alone"""
    ms, shape = ref["match_start"], s["shape"]
    per = np.diff(ms)[fr.WRAP:]
    busy = (shape[fr.WRAP:] > 0).all(axis=1)
    assert (per > 0).sum() > 100 and ((per == 0) & busy).sum() > 10   # wrapped pairs with matches and with none
    assert (np.diff(ms)[:fr.PLACED] > 0).sum() > 100
    # match_start moves on each side of index 65,535: in the placed pairs, in the fillers and in the wrapped pairs
    assert 0 < ms[fr.PLACED] < ms[fr.WRAP] < ms[-1] and len(np.unique(ms[fr.WRAP - 300:fr.WRAP + 300])) > 100
    row = ref["row_off"][s["tie_pair"]] + 5
    assert (ref["nn"][row], ref["d1"][row], ref["d2"][row]) == (3, 0, 0)  # the copies at 3 + T and 129 do not win


@pytest.mark.parametrize("dim,cross_check", [(64, False), (64, True), (128, True)])
def test_a_workgroup_takes_a_second_pair(core, dim, cross_check):
    """gridDim.y is 65,535, so the workgroups of pairs 0 .. 599 go on to pairs 65,535 .. 66,134: every ordered
    pair of (0, 1, 17, 65, 130, 2 BM + 9) keypoints as the rows of the first and of the second pair and as their
    columns (tests/test_fast_refs.py asserts the table), a tie across column tiles in a second pair, and
    match_start across the wrap.  Results left over from the first pair, rows of the second never written or a
    barrier count that differs inside a workgroup cannot pass."""
    s, nb = wrap_neighbours(dim)
    ref = fr.match_accept(nb, 0.8, fr.wrap_limit(dim), cross_check)
    ref.update(row_off=nb["row_off"])
    wrap_conditions(s, ref)
    out = core.match_descriptors(s["desc"], s["img_start"], s["pairs"], 0.8, fr.wrap_limit(dim), cross_check,
                                 want_diagnostics=True)
    md.same(out, ref)
