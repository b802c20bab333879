"""Pair selection by retrieval on a real MI355X (sfm_vocab_train,
sfm_select_pairs, sfm_io.select_pairs) against the plain-numpy restatement of
tests/test_retrieval.py and tests/golden/retrieval.npz.  Integer work with an
exact answer, and a score of five IEEE operations: every output is compared
for equality, dtype and shape included; there are no tolerances.  The last two
tests reach the second regimes: training on 2^20 + 300 rows (two pseudo-images
of the nearest-centre pass, the tally's grid stride, the sort and the sums at a
million rows, an inertia above 2^32) and retrieval at 513, 6,145, 8,193 and
16,384 images (the top-k scan's stride, the dynamic-LDS attribute above 48 KiB,
a launch above 64 KiB and the documented limit), against the vectorised
restatements of tests/fast_refs.py (equal to the plain ones wherever
tests/test_fast_refs.py can afford the plain ones).
"""
import functools

import numpy as np
import pytest

import fast_refs as fr
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


@functools.lru_cache(maxsize=None)
def large_training():
    """the scene of 2^20 + 300 rows and its restatement after one update, which holds the quantisation too"""
    desc, centres = fr.train_scene()
    return desc, centres, fr.train(desc, centres, 1)


@pytest.mark.parametrize("its", [0, 1])
def test_training_past_one_pseudo_image(core, its):
    """2^20 + 300 descriptors at dim 64 against 65 centres: the nearest-centre pass takes the rows as a block of
    2^20 and a block of 300 whose results start at row 2^20, k_vt_tally strides its grid, and the sort, the byte
    sums and the u64 inertia see a million rows"""
    desc, centres, one = large_training()
    ref = one
    if its == 0:  # the state before the update: the assignment to the initial centres
        word, count, total = fr.assign(desc, centres)
        ref = dict(centres=centres, word=word.astype(np.int32), count=count, inertia=np.array([total], np.int64),
                   iterations=np.int32(0))
        assert total == one["inertia"][0]
    # conditions on the inputs, from the restatement alone
    tail, head = ref["word"][2 ** 20:], ref["word"][:300]
    assert len(tail) == 300 and len(np.unique(tail)) > 30 and (tail != head).sum() > 250
    assert (ref["inertia"] > 2 ** 32).all() and ref["count"].sum() == len(desc) and ref["count"].min() > 0
    assert int(ref["iterations"]) == its and len(ref["inertia"]) == its + 1
    assert its == 0 or (ref["inertia"][1] < ref["inertia"][0] and not np.array_equal(ref["centres"], centres))
    rt.same(train(core, desc, centres, its), ref, TRAIN_OUTPUTS)


@pytest.mark.parametrize("n_images", fr.SELECT_SIZES)
def test_select_pairs_at_the_four_lds_regimes(core, n_images):
    """one image more than the query workgroup has threads, then 49,288, 65,672 and 131,200 bytes of dynamic LDS:
    above 48 KiB, above 64 KiB and at the 16,384 images the header allows"""
    word, img_start = fr.select_scene(n_images)
    ref = fr.select(word, img_start, fr.SELECT_WORDS, fr.SELECT_TOP_K)
    # conditions on the inputs, from the restatement alone
    nb, sc = ref["neighbour"], ref["score"]
    assert ((sc[:, :-1] == sc[:, 1:]) & (sc[:, :-1] > 0)).any()                 # tied scores exist
    ahead = [(nb[:, a] >= fr.SP_THREADS) & (nb[:, b] >= 0) & (nb[:, b] < fr.SP_THREADS)
             for a in range(fr.SELECT_TOP_K) for b in range(a + 1, fr.SELECT_TOP_K)]
    assert np.any(ahead)  # an index that only the scan's stride reaches ranks ahead of one that its start reaches
    assert nb[fr.SELECT_TWIN, 0] == n_images - 1 and nb[fr.SELECT_TWIN, 1] >= 0
    assert (nb[n_images // 2] == -1).all() and (nb == -1).any(axis=1).sum() >= 1  # padded rows
    assert (nb >= 0).all(axis=1).sum() > n_images // 2
    rt.same(core.select_pairs(word, img_start, fr.SELECT_WORDS, fr.SELECT_TOP_K), ref, SELECT_OUTPUTS)


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
