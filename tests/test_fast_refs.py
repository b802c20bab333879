"""The vectorised restatements of tests/fast_refs.py against the plain ones, which
remain the definition: on the committed fixture scenes and on seeded samples of
the large scenes of the GPU tests, cut out so that the plain restatements finish
in seconds.  Equality of dtype, shape and every element.  The conditions the GPU
tests need of the large scenes' inputs that can be read off the inputs alone are
asserted here too.  No GPU needed.
"""
import numpy as np

import fast_refs as fr
import test_match_descriptors as md
import test_match_guided as mg
import test_retrieval as rt
from test_match_descriptors import INT32_MAX


# ------------------------------------------------------------------ matching
def test_match_equals_the_plain_restatement_on_the_fixture_scenes():
    fx = md.fixture()
    for tag, desc, img_start, pairs, ratio, max_dsq, cross in md.fixture_cases():
        out = fr.match(desc, img_start, pairs, ratio, max_dsq, cross)
        md.same(out, md.restate(desc, img_start, pairs, ratio, max_dsq, cross))
        md.same(out, {n: fx[f"{tag}_{n}"] for n in md.OUTPUTS})
    # no pair at all, and the hand-made tie: the smaller index wins and d2 == d1
    md.same(fr.match(np.zeros((3, 64), np.uint8), [0, 2, 3], [], 0.8, INT32_MAX, True),
            md.restate(np.zeros((3, 64), np.uint8), [0, 2, 3], [], 0.8, INT32_MAX, True))
    d = np.full((4, 64), 100, np.uint8)
    d[1:, 0] = (103, 104, 97)
    out = fr.match(d, [0, 1, 4], [(0, 1), (1, 0)], 1.0, INT32_MAX, False)
    md.same(out, md.restate(d, [0, 1, 4], [(0, 1), (1, 0)], 1.0, INT32_MAX, False))
    assert (out["nn"][0], out["d1"][0], out["d2"][0]) == (0, 9, 9)


def test_match_guided_equals_the_plain_restatement_on_the_fixture_scenes():
    fx = mg.fixture()
    for tag, desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross in mg.fixture_cases():
        out = fr.match_guided(desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross)
        md.same(out, mg.restate_guided(desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross), mg.OUTPUTS)
        md.same(out, {n: fx[f"{tag}_{n}"] for n in mg.OUTPUTS}, mg.OUTPUTS)
    desc, xy, img_start, pairs, F = mg.small_scene()
    for gate in (0.0, 1e200):  # nothing admitted, and thr2 = +inf
        md.same(fr.match_guided(desc, xy, img_start, pairs, F, gate, 0.9, INT32_MAX, True),
                mg.restate_guided(desc, xy, img_start, pairs, F, gate, 0.9, INT32_MAX, True), mg.OUTPUTS)


def placed(scene):
    """(first, wrapped): the (N_i, N_j) of pairs 0 .. 599 and of the pairs 65,535 later"""
    return scene["shape"][:fr.PLACED], scene["shape"][fr.WRAP:]


def test_wrap_scene_places_every_transition():
    """conditions on the inputs of the GPU tests' 66,135 pairs, from the pair table alone"""
    for dim in (64, 128):
        s = fr.wrap_scene(dim)
        assert len(s["pairs"]) == fr.WRAP + fr.PLACED == 66135 and s["desc"].shape[1] == dim
        assert (s["pairs"][:, 0] != s["pairs"][:, 1]).all() and s["shape"][:, 0].sum() < 1_100_000
        n = np.diff(s["img_start"])
        assert 300 <= len(n) <= 400 and ((n >= 1) & (n <= 3)).sum() > 0.9 * len(n)
        first, wrapped = placed(s)
        assert set(np.unique(s["shape"][fr.PLACED:fr.WRAP])) <= {1, 2, 3}
        for side in (0, 1):  # rows, then columns
            for k in fr.SHAPES:
                here = first[:, side] == k
                assert k == fr.SHAPES[0] or (here & (wrapped[:, side] < k)).any(), (side, k)
                assert k == fr.SHAPES[-1] or (here & (wrapped[:, side] > k)).any(), (side, k)
        assert ((first[:, 1] == 130) & (wrapped[:, 1] == 1)).any()           # three column tiles, then one column
        empty = (first[:, 0] == 0) | (first[:, 1] == 0)
        assert (empty & (wrapped[:, 0] == 2 * fr.BM + 9) & (wrapped[:, 1] > 0)).any()  # empty, then three row blocks
        inside = (first[:, 0] > 0) & (first[:, 0] < fr.BM) & (first[:, 1] > 0)
        assert (inside & (wrapped[:, 0] > 2 * fr.BM) & (wrapped[:, 1] > 0)).any()  # first row block, then the third
        assert s["tie_pair"] >= fr.WRAP and tuple(s["shape"][s["tie_pair"]]) == (17, 130)
        assert len(np.unique(s["F"][np.isfinite(s["F"]).all(axis=(1, 2))].reshape(-1, 9), axis=0)) == len(s["F"]) - 1


def test_match_and_match_guided_equal_the_plain_restatements_on_a_sample_of_the_wrap_scene():
    s = fr.wrap_scene(64)
    idx = fr.wrap_sample(s)
    assert 250 <= len(idx) <= 400 and s["tie_pair"] in idx and (idx >= fr.WRAP).sum() > 80
    pairs, F = s["pairs"][idx], s["F"][idx]
    shapes = {tuple(x) for x in s["shape"][idx]}
    assert {(a, b) for a, b in shapes if a in fr.SHAPES} >= {(265, 265), (0, 265), (130, 1), (17, 130)}
    for cross in (False, True):
        out = fr.match(s["desc"], s["img_start"], pairs, 0.8, fr.wrap_limit(64), cross)
        md.same(out, md.restate(s["desc"], s["img_start"], pairs, 0.8, fr.wrap_limit(64), cross))
    tie = int(np.flatnonzero(idx == s["tie_pair"])[0])
    row = int(np.diff(s["img_start"])[pairs[:tie, 0]].sum()) + 5  # row 5 of the tie pair, pair-major
    assert (out["nn"][row], out["d1"][row], out["d2"][row]) == (3, 0, 0)  # the copy in the late tiles does not win
    out = fr.match_guided(s["desc"], s["xy"], s["img_start"], pairs, F, fr.GUIDED_GATE, 0.8, fr.wrap_limit(64), True)
    md.same(out, mg.restate_guided(s["desc"], s["xy"], s["img_start"], pairs, F, fr.GUIDED_GATE, 0.8,
                                   fr.wrap_limit(64), True), mg.OUTPUTS)
    full = np.repeat(s["shape"][idx][:, 1], s["shape"][idx][:, 0])
    assert (out["n_cand"] < full).any() and (out["n_cand"] == full).any() and (out["n_cand"] == 0).any()


# ------------------------------------------------------------------ assignment and training
def test_train_equals_the_plain_restatement_on_the_fixture_scene():
    fx = rt.fixture()
    desc, c0 = fx["grouped_desc"], rt.fixture_centres0(fx)
    for its in (0,) + rt.TRAIN_ITERATIONS:
        out = fr.train(desc, c0, its, chunk=100)  # 864 rows: nine chunks, the last a short one
        rt.same(out, rt.restate_train(desc, c0, its), rt.TRAIN_OUTPUTS)
        if its:
            rt.same(out, rt.fixture_train(fx, its), rt.TRAIN_OUTPUTS)
    # an empty cluster keeps its bytes, a tie goes to the smaller index, the early stop
    d = np.full((3, 64), 7, np.uint8)
    d[:, 0] = (1, 2, 3)
    for its in (0, 1, 5):
        rt.same(fr.train(d, d[[0, 0]], its, chunk=2), rt.restate_train(d, d[[0, 0]], its), rt.TRAIN_OUTPUTS)
    assert fr.train(d, d[[0, 0]], 5)["iterations"] == 3


def test_train_equals_the_plain_restatement_on_a_sample_of_the_large_scene():
    desc, centres = fr.train_scene()
    assert desc.shape == (2 ** 20 + 300, 64) and centres.shape == (65, 64) and desc.dtype == centres.dtype == np.uint8
    rows = fr.train_sample(desc)
    assert len(rows) == 500 and np.array_equal(rows[-300:], desc[2 ** 20:])
    for its in (0, 1, 4):
        rt.same(fr.train(rows, centres, its, chunk=128), rt.restate_train(rows, centres, its), rt.TRAIN_OUTPUTS)
    # and one chunk across the end of the first block of 2^20 rows equals the same rows on their own
    word, _, _ = fr.assign(desc[2 ** 20 - 100:], centres, chunk=64)
    assert np.array_equal(word, rt.restate_train(desc[2 ** 20 - 100:], centres, 0)["word"])


# ------------------------------------------------------------------ retrieval
def test_select_equals_the_plain_restatement_on_the_fixture_scenes():
    fx = rt.fixture()
    word, img_start = fx["train10_word"], fx["grouped_img_start"]
    for k in rt.TOP_KS:
        out = fr.select(word, img_start, rt.N_WORDS, k, block=5)
        rt.same(out, rt.restate_select(word, img_start, rt.N_WORDS, k), rt.SELECT_OUTPUTS)
        rt.same(out, rt.fixture_select(fx, f"sel{k}"), rt.SELECT_OUTPUTS)
    for name, (w, st, nw) in rt.edge_scenes(word, img_start).items():
        rt.same(fr.select(w, st, nw, 3), rt.restate_select(w, st, nw, 3), rt.SELECT_OUTPUTS)
    # ties go to the smaller index; images without a keypoint; no image
    words = [[0, 1], [0], [0], [0], [2]]
    st = np.concatenate([[0], np.cumsum([len(w) for w in words])])
    out = fr.select(np.concatenate(words), st, 3, 2)
    rt.same(out, rt.restate_select(np.concatenate(words), st, 3, 2), rt.SELECT_OUTPUTS)
    assert out["neighbour"].tolist() == [[1, 2], [2, 3], [1, 3], [1, 2], [-1, -1]]
    for st in ([0, 0, 0], [0]):
        rt.same(fr.select(np.zeros(0, np.int32), st, 4, 2), rt.restate_select(np.zeros(0, np.int32), st, 4, 2),
                rt.SELECT_OUTPUTS)
    rng = np.random.default_rng(70)  # the scene of 70 short images of tests/test_retrieval_gpu.py
    word = rng.integers(0, 50, 350)
    for k in (6, 80):
        rt.same(fr.select(word, np.arange(0, 351, 5), 50, k, block=32),
                rt.restate_select(word, np.arange(0, 351, 5), 50, k), rt.SELECT_OUTPUTS)


def test_select_equals_the_plain_restatement_on_samples_of_the_large_scenes():
    for n in fr.SELECT_SIZES:
        word, img_start = fr.select_scene(n)
        assert len(img_start) == n + 1 and len(word) == 4 * (n - 1) and word.max() < fr.SELECT_WORDS
        assert img_start[n // 2] == img_start[n // 2 + 1]  # the empty image
        if n in (513, 16384):
            w, st = fr.select_sample(word, img_start)
            out = fr.select(w, st, fr.SELECT_WORDS, fr.SELECT_TOP_K, block=64)
            rt.same(out, rt.restate_select(w, st, fr.SELECT_WORDS, fr.SELECT_TOP_K), rt.SELECT_OUTPUTS)
            assert (out["neighbour"][300] == -1).all() and out["neighbour"][fr.SELECT_TWIN, 0] == 301
    # LDS bytes of the query kernel at the four sizes: 8 per image and 128 more
    lds = [8 * n + 128 for n in fr.SELECT_SIZES]
    assert lds[0] < 48 * 1024 < lds[1] < 64 * 1024 < lds[2] < lds[3] == 131200
