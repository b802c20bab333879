"""Pair selection by retrieval (sfm_vocab_train, sfm_select_pairs) restated in
plain numpy from the definitions of include/sfmcore.h: an int64 distance
matrix with argmin for the (dsq, index) order, exact integer sums, math.log for
the idf table and math.sqrt on Python floats for the score -- not as the
kernels compute them.  Checked here against tests/golden/retrieval.npz
(generator: tests/golden/make_golden_retrieval.py; none of it comes from the
reference, which has no such stage) and against hand-made cases;
tests/test_retrieval_gpu.py compares the device calls with it for equality.
No GPU needed.
"""
import math
import os
import re

import numpy as np

from conftest import GOLDEN, REPO

TRAIN_OUTPUTS = ("centres", "word", "count", "inertia", "iterations")
SELECT_OUTPUTS = ("neighbour", "score", "dot", "norm2", "df")


def distances(desc, centres):
    """the int64 matrix of squared distances, exact"""
    a, c = np.asarray(desc).astype(np.int64), np.asarray(centres).astype(np.int64)
    return (a * a).sum(axis=1)[:, None] + (c * c).sum(axis=1)[None, :] - 2 * (a @ c.T)


def restate_train(desc, centres0, max_iterations):
    """the outputs of sfm_vocab_train as a dict"""
    desc = np.asarray(desc, dtype=np.uint8)
    centres = np.array(centres0, dtype=np.uint8)
    n_words = len(centres)
    rows = np.arange(len(desc))

    def assign(c):
        D = distances(desc, c)
        word = np.argmin(D, axis=1)  # the first minimum: the smaller index on a tie
        return word, np.bincount(word, minlength=n_words).astype(np.int64), int(D[rows, word].sum())
    word, count, total = assign(centres)
    inertia, T = [total], 0
    while T < max_iterations:
        new = centres.copy()
        for w in np.nonzero(count)[0]:
            s = desc[word == w].astype(np.int64).sum(axis=0)
            new[w] = (2 * s + count[w]) // (2 * count[w])
        T += 1
        changed = not np.array_equal(new, centres)
        centres = new
        word, count, total = assign(centres)
        inertia.append(total)
        if not changed:
            break
    return dict(centres=centres, word=word.astype(np.int32), count=count, inertia=np.array(inertia, dtype=np.int64),
                iterations=np.int32(T))


def restate_select(word, img_start, n_words, top_k):
    """the outputs of sfm_select_pairs as a dict"""
    word, img_start = np.asarray(word), np.asarray(img_start)
    n = len(img_start) - 1
    h = np.zeros((n, n_words), dtype=np.int64)
    for i in range(n):
        h[i] = np.bincount(word[img_start[i]:img_start[i + 1]], minlength=n_words)
    df = (h > 0).sum(axis=0)
    q = np.array([0] + [math.floor(256.0 * math.log(n / d) + 0.5) for d in range(1, n + 1)], dtype=np.int64)
    v = h * q[df][None, :]
    norm2 = (v * v).sum(axis=1)
    dots = v @ v.T
    neighbour = np.full((n, top_k), -1, dtype=np.int32)
    score = np.zeros((n, top_k), dtype=np.float64)
    dot = np.zeros((n, top_k), dtype=np.int64)
    for i in range(n):
        cand = []
        for j in range(n):
            if j != i and dots[i, j] > 0:
                s = float(int(dots[i, j])) / (math.sqrt(float(int(norm2[i]))) * math.sqrt(float(int(norm2[j]))))
                cand.append((-s, j))
        for k, (s, j) in enumerate(sorted(cand)[:top_k]):
            neighbour[i, k], score[i, k], dot[i, k] = j, -s, dots[i, j]
    return dict(neighbour=neighbour, score=score, dot=dot, norm2=norm2.astype(np.int64), df=df.astype(np.int32))


def same(out, ref, names):
    for n in names:
        a, b = np.asarray(out[n]), np.asarray(ref[n])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), n


# ------------------------------------------------------------------ scenes
SCENE_SEED, N_WORDS, TRAIN_ITERATIONS, TOP_KS = 5, 192, (1, 3, 10), (1, 3, 11, 20)


def grouped_scene(seed=SCENE_SEED, n_groups=3, per_group=4, n_points=60, n_seen=42, n_distractors=30, dim=128):
    """3 groups of 4 images; a group has 60 base descriptors of uniform random bytes, an image sees 42 of them with
    integer noise in [-2, 2] clipped, plus 30 uniform random distractors, shuffled; the images are permuted across
    the groups.  Returns (descriptors, group): group[k] is the group of image k."""
    rng = np.random.default_rng(seed)
    descriptors, group = [], []
    for g in range(n_groups):
        base = rng.integers(0, 256, (n_points, dim))
        for _ in range(per_group):
            seen = rng.permutation(n_points)[:n_seen]
            d = np.clip(base[seen] + rng.integers(-2, 3, (n_seen, dim)), 0, 255)
            d = np.concatenate([d, rng.integers(0, 256, (n_distractors, dim))])
            descriptors.append(d[rng.permutation(len(d))].astype(np.uint8))
            group.append(g)
    order = rng.permutation(len(descriptors))
    return [descriptors[k] for k in order], np.array(group)[order]


def pack(descs):
    desc = np.concatenate(descs)
    return desc, np.concatenate([[0], np.cumsum([len(d) for d in descs])]).astype(np.int64)


def initial_centres(desc, n_words, seed=0):
    """train_vocabulary's choice of the initial centres"""
    return desc[np.sort(np.random.default_rng(seed).choice(len(desc), n_words, replace=False))]


def edge_scenes(word, img_start):
    """Two variations of the grouped scene's words.  "empty": an image without keypoints in the middle.  "common":
    one more word (N_WORDS) that every image holds twice, and a last image of three keypoints that holds nothing
    else: df == n_images, weight 0, norm2 0.  Returns {name: (word, img_start, n_words)}."""
    per = [word[img_start[k]:img_start[k + 1]] for k in range(len(img_start) - 1)]
    empty = per[:5] + [np.zeros(0, np.int32)] + per[5:]
    extra = np.full(2, N_WORDS, np.int32)
    common = [np.concatenate([extra[:1], p, extra[1:]]) for p in per] + [np.full(3, N_WORDS, np.int32)]
    out = {}
    for name, images, nw in (("empty", empty, N_WORDS), ("common", common, N_WORDS + 1)):
        out[name] = (np.concatenate(images).astype(np.int32),
                     np.concatenate([[0], np.cumsum([len(p) for p in images])]).astype(np.int64), nw)
    return out


def fixture():
    return np.load(os.path.join(GOLDEN, "retrieval.npz"))


def fixture_train(fx, its):
    """the fixture's training outputs; the centres of the runs of 1 and 3 iterations are stored as their byte
    difference (mod 256) from the run of 10, which is mostly zero and keeps the file small"""
    out = {k: fx[f"train{its}_{k}"] for k in TRAIN_OUTPUTS if k != "centres"}
    out["centres"] = fx["train10_centres"] if its == 10 else fx["train10_centres"] + fx[f"train{its}_centres_delta"]
    return out


def fixture_centres0(fx):
    """the initial centres: rows grouped_first of the descriptors"""
    return fx["grouped_desc"][fx["grouped_first"]]


def fixture_select(fx, tag):
    return {k: fx[f"{tag}_{k}"] for k in SELECT_OUTPUTS}


# ------------------------------------------------------------------ the restatement
def test_restatement_matches_the_fixture():
    fx = fixture()
    descs, group = grouped_scene()
    desc, img_start = pack(descs)
    assert desc.shape == (864, 128) and desc.dtype == np.uint8
    c0 = initial_centres(desc, N_WORDS)
    for k, v in (("desc", desc), ("img_start", img_start), ("group", group)):
        assert fx[f"grouped_{k}"].dtype == v.dtype and np.array_equal(fx[f"grouped_{k}"], v), k
    assert np.array_equal(fixture_centres0(fx), c0)
    for its in TRAIN_ITERATIONS:
        same(fixture_train(fx, its), restate_train(desc, c0, its), TRAIN_OUTPUTS)
    word = fx["train10_word"]
    for k in TOP_KS:
        same(fixture_select(fx, f"sel{k}"), restate_select(word, img_start, N_WORDS, k), SELECT_OUTPUTS)
    for name, (w, st, nw) in edge_scenes(word, img_start).items():
        assert np.array_equal(fx[f"{name}_word"], w) and np.array_equal(fx[f"{name}_img_start"], st)
        same(fixture_select(fx, name), restate_select(w, st, nw, 3), SELECT_OUTPUTS)
    assert os.path.getsize(os.path.join(GOLDEN, "retrieval.npz")) < 200_000


def test_grouped_scene_stops_early_and_retrieves_the_groups():
    """conditions on the inputs, on the restatement alone"""
    fx = fixture()
    T = int(fx["train10_iterations"])
    inertia = fx["train10_inertia"]
    assert 0 < T < 10 and len(inertia) == T + 1 and inertia[T] == inertia[T - 1]
    assert (np.diff(inertia) <= 0).all() and inertia[0] > inertia[T]
    assert int(fx["train1_iterations"]) == 1 and int(fx["train3_iterations"]) == 3  # the cap, not the early stop
    group, nb = fx["grouped_group"], fx["sel3_neighbour"]
    for i in range(len(group)):
        others = [j for j in range(len(group)) if j != i and group[j] == group[i]]
        assert sorted(nb[i].tolist()) == others, i
    assert (fx["sel20_neighbour"][:, -1] == -1).all()  # fewer than 20 candidates: padding
    assert (fx["sel20_score"][fx["sel20_neighbour"] < 0] == 0.0).all()
    assert (fx["sel20_dot"][fx["sel20_neighbour"] < 0] == 0).all()
    # the edge scenes: an empty image and an image of common words only have norm2 0 and an all -1 row
    assert fx["empty_norm2"][5] == 0 and (fx["empty_neighbour"][5] == -1).all()
    assert not (fx["empty_neighbour"] == 5).any()
    assert fx["common_df"][N_WORDS] == 13 and fx["common_norm2"][12] == 0 and (fx["common_neighbour"][12] == -1).all()
    assert np.array_equal(fx["common_neighbour"][:12], fx["sel3_neighbour"])
    assert np.array_equal(fx["common_dot"][:12] > 0, fx["sel3_dot"] > 0)


def test_restatement_of_the_update_on_hand_made_cases():
    def rows(*first):
        d = np.full((len(first), 64), 7, dtype=np.uint8)
        d[:, 0] = first
        return d
    # members 1 and 2 give 2 (1.5 rounds up); members 0, 0, 1 give 0 (1/3 rounds down); all 255 stays 255
    desc = np.concatenate([rows(1, 2), rows(0, 0, 1) + np.uint8(100), np.full((3, 64), 255, np.uint8)])
    c0 = np.stack([rows(1)[0], rows(0)[0] + np.uint8(100), np.full(64, 254, np.uint8), np.full(64, 200, np.uint8)])
    out = restate_train(desc, c0, 1)
    assert out["word"].tolist() == [0, 0, 1, 1, 1, 2, 2, 2] and out["count"].tolist() == [2, 3, 3, 0]
    assert out["centres"][0, 0] == 2 and (out["centres"][0, 1:] == 7).all()
    assert out["centres"][1, 0] == 100 and (out["centres"][1, 1:] == 107).all()
    assert (out["centres"][2] == 255).all()
    assert np.array_equal(out["centres"][3], c0[3])  # an empty cluster keeps its bytes
    assert out["iterations"] == 1 and out["inertia"].tolist() == [1 + 1 + 3 * 64, 1 + 1]
    # two identical centres: the tie goes to the smaller index and the larger one is empty.  max_iterations = 0 is
    # quantisation: the initial centres, iterations == 0 and one inertia entry
    c0 = np.stack([rows(1)[0], rows(1)[0]])
    out = restate_train(rows(1, 2, 3), c0, 0)
    assert out["word"].tolist() == [0, 0, 0] and out["count"].tolist() == [3, 0]
    assert np.array_equal(out["centres"], c0) and out["iterations"] == 0 and out["inertia"].tolist() == [5]
    # update 1 moves centre 0 to 2 and keeps the empty centre 1 at 1, which then takes the first descriptor; update
    # 2 moves centre 0 to 3 (2.5 rounds up) and the descriptor 2, at distance 1 from both, goes to the smaller
    # index; update 3 changes nothing
    out = restate_train(rows(1, 2, 3), c0, 1)
    assert out["centres"][:, 0].tolist() == [2, 1] and out["word"].tolist() == [1, 0, 0]
    out = restate_train(rows(1, 2, 3), c0, 5)
    assert out["centres"][:, 0].tolist() == [3, 1] and out["word"].tolist() == [1, 0, 0]
    assert out["count"].tolist() == [2, 1] and out["iterations"] == 3 and out["inertia"].tolist() == [5, 1, 1, 1]


def test_restatement_of_the_retrieval_on_hand_made_cases():
    # four images over five words; word 4 is in every image (weight 0).  Images 0 and 1 share word 0, image 2 has
    # words 1 and 4, image 3 only word 4
    words = [[0, 0, 4], [0, 2, 4], [1, 4], [4, 4]]
    word = np.concatenate(words)
    st = np.concatenate([[0], np.cumsum([len(w) for w in words])])
    out = restate_select(word, st, 5, 2)
    q2, q4 = math.floor(256 * math.log(2) + 0.5), math.floor(256 * math.log(4) + 0.5)
    assert out["df"].tolist() == [2, 1, 1, 0, 4]
    assert out["norm2"].tolist() == [(2 * q2) ** 2, q2 ** 2 + q4 ** 2, q4 ** 2, 0]
    assert out["neighbour"].tolist() == [[1, -1], [0, -1], [-1, -1], [-1, -1]]  # padded rows
    assert out["dot"].tolist() == [[2 * q2 * q2, 0], [2 * q2 * q2, 0], [0, 0], [0, 0]]
    assert out["score"][0, 0] == out["score"][1, 0] and 0 < out["score"][0, 0] < 1 and out["score"][2, 0] == 0.0
    # images 2 and 3 share only the word of every image: dot 0, not neighbours; image 3 has norm2 0: an all -1 row
    # ties in the score go to the smaller j: images 1, 2, 3 are identical, image 0 shares a word with them
    words = [[0, 1], [0], [0], [0], [2]]
    word = np.concatenate(words)
    st = np.concatenate([[0], np.cumsum([len(w) for w in words])])
    out = restate_select(word, st, 3, 2)
    assert out["neighbour"].tolist() == [[1, 2], [2, 3], [1, 3], [1, 2], [-1, -1]]
    assert out["score"][1].tolist() == [1.0, 1.0] and out["score"][0, 0] == out["score"][0, 1] < 1.0
    assert restate_select(word, st, 3, 0)["neighbour"].shape == (5, 0)


# ------------------------------------------------------------------ header and bindings
TRAIN_ARGS = ["const uint8_t *desc", "int64_t n", "int32_t dim", "int32_t n_words", "int32_t max_iterations",
              "uint8_t *centres", "int32_t *word", "int64_t *count", "int64_t *inertia", "int32_t *iterations",
              "int device"]
SELECT_ARGS = ["const int32_t *word", "int64_t n_kp", "const int64_t *img_start", "int32_t n_images",
               "int32_t n_words", "int32_t top_k", "int32_t *neighbour", "double *score", "int64_t *dot",
               "int64_t *norm2", "int32_t *df", "int device"]


def test_header_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "sfmcore.h")).read()
    import _sfmcore
    for name, args in (("sfm_vocab_train", TRAIN_ARGS), ("sfm_select_pairs", SELECT_ARGS)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"include/sfmcore.h does not declare {name}"
        assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == args
        assert hasattr(_sfmcore._lib, name)
        assert len(dict((n, a) for n, _, a in _sfmcore.SIGNATURES)[name]) == len(args)
    assert "limits of this implementation" in txt and "rounded half up" in txt
    import sfm_io
    import sfm_multiview
    for name in ("train_vocabulary", "quantize", "select_pairs"):
        assert getattr(sfm_multiview, name) is getattr(sfm_io, name)


def raw_train(core, desc, centres, n=None, dim=None, n_words=None, its=1, null=()):
    """sfm_vocab_train with sentinel-filled outputs; returns (rc, outputs, centres as passed)"""
    desc = np.ascontiguousarray(desc, dtype=np.uint8)
    centres = np.array(centres, dtype=np.uint8)
    before = centres.copy()
    outs = dict(word=np.full(64, -7, np.int32), count=np.full(64, -7, np.int64), inertia=np.full(16, -7, np.int64),
                iterations=np.full(1, -7, np.int32))
    P = core._p
    types = dict(word=core._i32, count=core._i64, inertia=core._i64, iterations=core._i32)
    ptr = {k: (None if k in null else P(v, types[k])) for k, v in outs.items()}
    rc = core._lib.sfm_vocab_train(None if "desc" in null else P(desc, core._u8), len(desc) if n is None else n,
                                   desc.shape[1] if dim is None else dim, len(centres) if n_words is None else n_words,
                                   its, None if "centres" in null else P(centres, core._u8), ptr["word"],
                                   ptr["count"], ptr["inertia"], ptr["iterations"], 0)
    outs["centres_unchanged"] = np.full(1, -7 if np.array_equal(centres, before) else 0)
    return rc, outs


def raw_select(core, word, img_start, n_words=8, top_k=2, n_kp=None, n_images=None, null=()):
    """sfm_select_pairs with sentinel-filled outputs; returns (rc, outputs)"""
    word = np.ascontiguousarray(word, dtype=np.int32)
    img_start = np.ascontiguousarray(img_start, dtype=np.int64)
    outs = dict(neighbour=np.full(64, -7, np.int32), score=np.full(64, -7.0), dot=np.full(64, -7, np.int64),
                norm2=np.full(16, -7, np.int64), df=np.full(16, -7, np.int32))
    P = core._p
    types = dict(neighbour=core._i32, score=core._d, dot=core._i64, norm2=core._i64, df=core._i32)
    ptr = {k: (None if k in null else P(v, types[k])) for k, v in outs.items()}
    rc = core._lib.sfm_select_pairs(None if "word" in null else P(word, core._i32),
                                    len(word) if n_kp is None else n_kp,
                                    None if "img_start" in null else P(img_start, core._i64),
                                    len(img_start) - 1 if n_images is None else n_images, n_words, top_k,
                                    ptr["neighbour"], ptr["score"], ptr["dot"], ptr["norm2"], ptr["df"], 0)
    return rc, outs


def untouched(outs):
    return all((v == -7).all() for v in outs.values())


def test_train_arguments_are_refused_before_a_device_is_looked_for():
    """each SFM_ERR_ARG case through the C ABI: -1 and no output touched (no GPU: the checks come first)"""
    import _sfmcore as core
    rng = np.random.default_rng(0)
    desc = rng.integers(0, 256, (8, 64)).astype(np.uint8)
    centres = desc[:3]
    cases = {"null_desc": dict(null=("desc",)), "null_centres": dict(null=("centres",)),
             "null_iterations": dict(null=("iterations",)), "dim_96": dict(dim=96), "dim_0": dict(dim=0),
             "dim_512": dict(dim=512), "n_0": dict(n=0), "n_negative": dict(n=-1), "no_words": dict(n_words=0),
             "words_above_n": dict(n_words=9), "words_above_2_20": dict(n=2 ** 21, n_words=2 ** 20 + 1, its=0),
             "iterations_negative": dict(its=-1), "train_above_2_24": dict(n=2 ** 24 + 1, its=1)}
    for name, change in cases.items():
        rc, outs = raw_train(core, desc, centres, **change)
        assert rc == -1, name
        assert untouched(outs), name
        assert core._lib.sfm_last_error().startswith(b"argument:"), name
    # the limits themselves pass the argument checks: the call then looks for a device.  Nullable outputs are null.
    rc, _ = raw_train(core, desc, desc, its=0, null=("word", "count", "inertia"))
    assert rc == 0 or not core._lib.sfm_last_error().startswith(b"argument:")
    with np.testing.assert_raises(core.SfmCoreError):
        core.vocab_train(desc, centres, -1)
    with np.testing.assert_raises(ValueError):
        core.vocab_train(desc, centres[:, :32])


def test_select_arguments_are_refused_before_a_device_is_looked_for():
    import _sfmcore as core
    word, st = np.array([0, 1, 2, 3, 7, 0, 1, 2]), np.array([0, 5, 8])
    many = np.zeros(2 ** 18 + 1, dtype=np.int32)
    cases = {"null_word": dict(null=("word",)), "null_img_start": dict(null=("img_start",)),
             "null_neighbour": dict(null=("neighbour",)), "null_score": dict(null=("score",)),
             "start": dict(img_start=np.array([1, 5, 8])), "decreasing": dict(img_start=np.array([0, 9, 8])),
             "short": dict(img_start=np.array([0, 5, 7])), "word_high": dict(n_words=7),
             "word_negative": dict(word=np.array([0, 1, 2, -1, 7, 0, 1, 2])),
             "too_many_keypoints": dict(word=many, img_start=np.array([0, 2 ** 18 + 1])),
             "too_many_images": dict(img_start=np.concatenate([[0, 5], np.full(16384, 8)])),
             "no_words": dict(n_words=0), "words_above_2_20": dict(n_words=2 ** 20 + 1),
             "n_images_negative": dict(n_images=-1), "top_k_negative": dict(top_k=-1)}
    for name, change in cases.items():
        a = dict(word=word, img_start=st)
        a.update(change)
        rc, outs = raw_select(core, a.pop("word"), a.pop("img_start"), **a)
        assert rc == -1, name
        assert untouched(outs), name
        assert core._lib.sfm_last_error().startswith(b"argument:"), name
    # the limits pass: 2^18 keypoints in an image, 16,384 images (top_k == 0 ends the call before a device)
    rc, outs = raw_select(core, many[:-1], [0, 2 ** 18], top_k=0)
    assert rc == 0 and untouched(outs)
    rc, outs = raw_select(core, word, np.concatenate([[0, 5], np.full(16383, 8)]), top_k=0)
    assert rc == 0 and untouched(outs)
    with np.testing.assert_raises(core.SfmCoreError):
        core.select_pairs(word, st, 7)


def test_nothing_to_select_needs_no_device():
    import _sfmcore as core
    word, st = np.array([0, 1, 2, 3, 7, 0, 1, 2]), np.array([0, 5, 8])
    rc, outs = raw_select(core, word, st, top_k=0, null=("neighbour", "score", "dot", "norm2", "df"))
    assert rc == 0
    rc, outs = raw_select(core, np.zeros(0, np.int32), [0], null=("word",))
    assert rc == 0 and untouched(outs)
    out = core.select_pairs(word, st, 8, top_k=0)
    assert out["neighbour"].shape == (2, 0) and out["neighbour"].dtype == np.int32 and out["score"].shape == (2, 0)
    out = core.select_pairs(np.zeros(0, np.int32), [0], 8, top_k=3)
    assert out["neighbour"].shape == (0, 3) and out["norm2"].shape == (0,)
    # images without a single keypoint: every row is padding, on the host
    out = core.select_pairs(np.zeros(0, np.int32), [0, 0, 0], 4, top_k=2)
    same(out, restate_select(np.zeros(0, np.int32), [0, 0, 0], 4, 2), SELECT_OUTPUTS)


# ------------------------------------------------------------------ the Python layer
def test_python_layer_refuses_bad_inputs():
    from sfm_io import quantize, select_pairs, train_vocabulary
    rng = np.random.default_rng(2)
    d = [rng.integers(0, 256, (4, 128)).astype(np.uint8), rng.integers(0, 256, (3, 128)).astype(np.uint8)]
    ragged = [d[0], rng.integers(0, 256, (3, 64)).astype(np.uint8)]
    empty = [np.zeros((0, 128), np.uint8)] * 2
    for descs in ([d[0].astype(np.float32), d[1]], ragged, [], empty, [d[0][:, :32], d[1][:, :32]], [d[0][0], d[1]]):
        for call in (lambda x: train_vocabulary(x, 2), lambda x: quantize(x, d[0][:2]), lambda x: select_pairs(x)):
            with np.testing.assert_raises(ValueError):
                call(descs)
    bad = [lambda: train_vocabulary(d, 0), lambda: train_vocabulary(d, 2, iterations=-1),
           lambda: train_vocabulary(d, 2, max_rows=0), lambda: quantize(d, d[0][:2].astype(np.int32)),
           lambda: quantize(d, d[0][:2, :64]), lambda: quantize(d, np.zeros((8, 128), np.uint8)),
           lambda: select_pairs(d, centres=d[0][:2], top_k=-1), lambda: select_pairs(d, centres=d[0][:0])]
    for call in bad:
        with np.testing.assert_raises(ValueError):
            call()


def test_pairs_of_a_neighbour_array_are_unique_ordered_and_sorted():
    from sfm_io import neighbour_pairs
    nb = np.array([[2, 1, -1], [0, 2, 3], [0, 1, -1], [-1, -1, -1], [3, 0, 1]], dtype=np.int32)
    pairs = neighbour_pairs(nb)
    assert pairs.dtype == np.int32 and pairs.tolist() == [[0, 1], [0, 2], [0, 4], [1, 2], [1, 3], [1, 4], [3, 4]]
    assert (pairs[:, 0] < pairs[:, 1]).all() and len(np.unique(pairs, axis=0)) == len(pairs)
    for none in (np.full((3, 2), -1, np.int32), np.zeros((3, 0), np.int32), np.zeros((0, 4), np.int32)):
        assert neighbour_pairs(none).shape == (0, 2) and neighbour_pairs(none).dtype == np.int32
