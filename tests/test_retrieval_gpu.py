"""Pair selection by retrieval on a real MI355X (sfm_vocab_train,
sfm_select_pairs, sfm_io.select_pairs) against the plain-numpy restatement of
tests/test_retrieval.py and tests/golden/retrieval.npz.  Integer work with an
exact answer, and a score of five IEEE operations: every output is compared
for equality, dtype and shape included; there are no tolerances.
"""
import numpy as np
import pytest

import test_retrieval as rt
from test_retrieval import N_WORDS, SELECT_OUTPUTS, TRAIN_OUTPUTS

pytestmark = pytest.mark.gpu
T = 64    # the nearest-centre kernel's column tile (MD_TN of csrc/match_common.hpp)
BM = 128  # the rows of one workgroup (md_bm)


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def fx():
    return rt.fixture()


def train(core, desc, centres, its):
    out = core.vocab_train(desc, centres, its)
    out["iterations"] = np.int32(out["iterations"])
    return out


def check_train(core, desc, centres, its):
    """the device call against the restatement; returns the restatement"""
    ref = rt.restate_train(desc, centres, its)
    rt.same(train(core, desc, centres, its), ref, TRAIN_OUTPUTS)
    return ref


def check_select(core, word, img_start, n_words, top_k):
    ref = rt.restate_select(word, img_start, n_words, top_k)
    rt.same(core.select_pairs(word, img_start, n_words, top_k), ref, SELECT_OUTPUTS)
    return ref


@pytest.mark.parametrize("dim", [64, 128, 256])
@pytest.mark.parametrize("n", [1, 17, 129, 300])
def test_assignment_of_random_descriptors(core, n, dim):
    rng = np.random.default_rng(1000 * n + dim)
    desc = rng.integers(0, 256, (n, dim)).astype(np.uint8)
    for n_words in (1, 2, 63, 64, 65, 130):
        if n_words <= n:
            ref = check_train(core, desc, rng.integers(0, 256, (n_words, dim)).astype(np.uint8), 0)
            assert ref["iterations"] == 0 and len(ref["inertia"]) == 1 and ref["count"].sum() == n


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_bias_and_extremes(core, dim):
    rng = np.random.default_rng(dim)
    values = np.array([0, 127, 128, 255], dtype=np.uint8)
    ref = check_train(core, values[rng.integers(0, 4, (90, dim))], values[rng.integers(0, 4, (70, dim))], 0)
    assert ref["inertia"][0] > 90 * 255 * 255
    n = 33
    ref = check_train(core, np.zeros((n, dim), np.uint8), np.full((20, dim), 255, np.uint8), 0)
    assert ref["inertia"][0] == n * dim * 255 * 255 and (ref["word"] == 0).all()


@pytest.mark.parametrize("dim", [64, 128])
def test_ties_across_column_tiles(core, dim):
    """identical centres at 3, 3 + T and n_words - 1 (three column tiles): a descriptor equal to them gets word 3,
    and a centre one unit further in a later tile does not win over an earlier tile's"""
    rng = np.random.default_rng(5 + dim)
    n_words = 2 * T + 21
    centres = rng.integers(0, 256, (n_words, dim)).astype(np.uint8)
    centres[:, 0] = np.clip(centres[:, 0], 2, 250)
    centres[[3 + T, n_words - 1]] = centres[3]
    desc = rng.integers(0, 256, (n_words + 11, dim)).astype(np.uint8)
    desc[7] = centres[3]
    desc[11] = centres[5]
    desc[11, 0] += 1                 # one unit from centre 5 ...
    centres[5 + T] = desc[11]
    centres[5 + T, 0] += 1           # ... and one unit from centre 5 + T, on the other side: a tie at dsq 1
    centres[2 * T + 9] = desc[11]
    centres[2 * T + 9, 1] ^= 2       # dsq 4 in the last tile
    ref = check_train(core, desc, centres, 0)
    assert ref["word"][7] == 3 and ref["word"][11] == 5
    assert ref["count"][3 + T] == 0 and ref["count"][n_words - 1] == 0


@pytest.mark.parametrize("its", rt.TRAIN_ITERATIONS)
def test_training_on_the_grouped_scene(core, fx, its):
    """max_iterations 1 and 3 end at the cap, 10 at the early stop"""
    ref = rt.fixture_train(fx, its)
    rt.same(train(core, fx["grouped_desc"], rt.fixture_centres0(fx), its), ref, TRAIN_OUTPUTS)
    assert int(ref["iterations"]) == min(its, 7)


def test_training_with_an_empty_cluster(core):
    """two identical initial centres: the second is empty at first and keeps its bytes through update 1"""
    rng = np.random.default_rng(8)
    desc = rng.integers(0, 256, (300, 64)).astype(np.uint8)
    c0 = desc[[5, 40, 41, 90, 150, 200, 250, 299]].copy()
    c0[6] = c0[2]
    ref = check_train(core, desc, c0, 1)
    assert np.array_equal(ref["centres"][6], c0[6]) and not np.array_equal(ref["centres"][2], c0[2])
    ref = check_train(core, desc, c0, 0)
    assert ref["count"][6] == 0 and ref["count"][2] > 0
    check_train(core, desc, c0, 4)


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_sums_over_three_row_blocks(core, dim):
    """2 BM + 9 descriptors span three workgroups of the assignment and several lane groups of the sums"""
    rng = np.random.default_rng(30 + dim)
    desc = rng.integers(0, 256, (2 * BM + 9, dim)).astype(np.uint8)
    ref = check_train(core, desc, desc[[0, 100, 128, 200, 264]], 1)
    assert ref["count"].sum() == len(desc) and ref["count"].min() > 0


@pytest.mark.parametrize("top_k", rt.TOP_KS)
def test_select_pairs_on_the_grouped_scene(core, fx, top_k):
    out = core.select_pairs(fx["train10_word"], fx["grouped_img_start"], N_WORDS, top_k)
    rt.same(out, rt.fixture_select(fx, f"sel{top_k}"), SELECT_OUTPUTS)


@pytest.mark.parametrize("name", ["empty", "common"])
def test_select_pairs_with_an_empty_image_and_with_common_words(core, fx, name):
    n_words = N_WORDS + (name == "common")
    out = core.select_pairs(fx[f"{name}_word"], fx[f"{name}_img_start"], n_words, 3)
    rt.same(out, rt.fixture_select(fx, name), SELECT_OUTPUTS)


def test_select_pairs_of_one_image_and_of_many_short_ones(core):
    ref = check_select(core, np.array([0, 1, 1, 3]), [0, 4], 4, 2)
    assert ref["neighbour"].tolist() == [[-1, -1]] and ref["norm2"].tolist() == [0]
    # 70 images of 5 random words each from 50: many queries with short postings, and ties in the score
    rng = np.random.default_rng(70)
    word = rng.integers(0, 50, 350)
    ref = check_select(core, word, np.arange(0, 351, 5), 50, 6)
    top = ref["score"][:, :-1]
    assert ((top == ref["score"][:, 1:]) & (top > 0)).any()  # a condition on the inputs: tied scores exist
    check_select(core, word, np.arange(0, 351, 5), 50, 80)   # top_k above the image count


def test_python_layer_returns_the_within_group_pairs(core, fx):
    from sfm_io import match_descriptors, quantize, select_pairs, train_vocabulary
    st, group = fx["grouped_img_start"], fx["grouped_group"]
    descs = [fx["grouped_desc"][st[k]:st[k + 1]] for k in range(len(st) - 1)]
    pairs, neighbour, score, centres = select_pairs(descs, n_words=N_WORDS, top_k=3)
    want = [(i, j) for i in range(12) for j in range(i + 1, 12) if group[i] == group[j]]
    assert pairs.dtype == np.int32 and pairs.tolist() == [list(p) for p in want] and len(want) == 18
    assert np.array_equal(neighbour, fx["sel3_neighbour"]) and np.array_equal(score, fx["sel3_score"])
    assert np.array_equal(centres, fx["train10_centres"])
    trained, report = train_vocabulary(descs, N_WORDS)
    assert np.array_equal(trained, centres) and report["iterations"] == 7
    assert np.array_equal(np.concatenate(quantize(descs, centres)), fx["train10_word"])
    # the deterministic subsample: every second row
    sub, _ = train_vocabulary(descs, 16, iterations=2, max_rows=432)
    rows = fx["grouped_desc"][::2]
    assert np.array_equal(sub, rt.restate_train(rows, rt.initial_centres(rows, 16), 2)["centres"])
    rng = np.random.default_rng(3)
    keypoints = [rng.random((len(d), 2)) * 1000.0 for d in descs]
    store, pair_ij, match_start, a, b, dsq = match_descriptors(keypoints, descs, pairs=pairs)
    assert np.array_equal(pair_ij, pairs) and len(match_start) == 19 and (np.diff(match_start) > 0).all()


def test_outputs_are_the_same_from_run_to_run(core, fx):
    rng = np.random.default_rng(9)
    other = rng.integers(0, 256, (500, 128)).astype(np.uint8)
    first = train(core, fx["grouped_desc"], rt.fixture_centres0(fx), 10)
    train(core, other, other[:40], 2)
    rt.same(train(core, fx["grouped_desc"], rt.fixture_centres0(fx), 10), first, TRAIN_OUTPUTS)
    word, st = fx["train10_word"], fx["grouped_img_start"]
    first = core.select_pairs(word, st, N_WORDS, 5)
    core.select_pairs(rng.integers(0, 30, 400), np.arange(0, 401, 20), 30, 4)
    rt.same(core.select_pairs(word, st, N_WORDS, 5), first, SELECT_OUTPUTS)
