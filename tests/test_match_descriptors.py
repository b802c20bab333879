"""Descriptor matching (sfm_match_descriptors) restated in plain numpy: an
int64 distance matrix, a lexsort for the (dsq, index) order and the tests as
include/sfmcore.h writes them, not as the kernels compute them.  Checked here
against tests/golden/match_descriptors.npz (generator:
tests/golden/make_golden_match_descriptors.py; none of it comes from the
reference, which has no matcher) and against hand-made cases;
tests/test_match_descriptors_gpu.py compares the device call with it for
equality.  No GPU needed.
"""
import itertools
import os
import re

import numpy as np

import test_merge_tracks as mt
from conftest import GOLDEN, REPO

INT32_MAX = 2 ** 31 - 1
OUTPUTS = ("match_start", "a", "b", "dsq", "nn", "d1", "d2", "nn_rev")


def first_two(D):
    """per row of the int64 distance matrix D: (nn, d1, d2) of the (dsq, index) order of its columns"""
    n, m = D.shape
    nn, d1, d2 = np.full(n, -1, np.int32), np.full(n, INT32_MAX, np.int32), np.full(n, INT32_MAX, np.int32)
    for r in range(n):
        order = np.lexsort((np.arange(m), D[r]))  # the last key is the primary one
        if m >= 1:
            nn[r], d1[r] = order[0], D[r, order[0]]
        if m >= 2:
            d2[r] = D[r, order[1]]
    return nn, d1, d2


def restate(desc, img_start, pairs, ratio=0.8, max_dsq=INT32_MAX, cross_check=True):
    """the outputs of sfm_match_descriptors as a dict of numpy arrays"""
    desc = np.asarray(desc).astype(np.int64)
    out = {k: [] for k in OUTPUTS[1:]}
    match_start = [0]
    r2 = np.float64(ratio) * np.float64(ratio)
    for i, j in np.asarray(pairs).reshape(-1, 2):
        A, B = desc[img_start[i]:img_start[i + 1]], desc[img_start[j]:img_start[j + 1]]
        D = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
        nn, d1, d2 = first_two(D)
        nn_rev = first_two(D.T)[0]
        count = 0
        for a in range(len(A)):
            ok = nn[a] >= 0 and d1[a] <= max_dsq
            ok = ok and (d2[a] == INT32_MAX or np.float64(d1[a]) < r2 * np.float64(d2[a]))
            ok = ok and (not cross_check or nn_rev[nn[a]] == a)
            if ok:
                out["a"].append(a)
                out["b"].append(nn[a])
                out["dsq"].append(d1[a])
                count += 1
        match_start.append(match_start[-1] + count)
        for k, v in (("nn", nn), ("d1", d1), ("d2", d2), ("nn_rev", nn_rev)):
            out[k].extend(v.tolist())
    res = {k: np.array(v, dtype=np.int32) for k, v in out.items()}
    res["match_start"] = np.array(match_start, dtype=np.int64)
    return res


def pack(descs):
    """(desc, img_start) of a list of per-image (N_k, dim) uint8 arrays"""
    dim = descs[0].shape[1]
    desc = np.concatenate([np.zeros((0, dim), np.uint8)] + [np.asarray(d, dtype=np.uint8) for d in descs])
    return desc, np.concatenate([[0], np.cumsum([len(d) for d in descs])]).astype(np.int64)


def store_arrays(keypoints, pairs, ref):
    """what sfm_io.match_descriptors builds from the outputs: the store's feature, image, x, y and flag"""
    feature, image, x, y = [], [], [], []
    pairs = np.asarray(pairs).reshape(-1, 2)
    for p, (i, j) in enumerate(pairs):
        for m in range(ref["match_start"][p], ref["match_start"][p + 1]):
            obs = sorted([(int(i), int(ref["a"][m])), (int(j), int(ref["b"][m]))])
            for im, k in obs:
                feature.append(m)
                image.append(im)
                x.append(keypoints[im][k][0])
                y.append(keypoints[im][k][1])
    return dict(feature=np.array(feature, dtype=np.int32), image=np.array(image, dtype=np.int32),
                x=np.array(x, dtype=np.float64), y=np.array(y, dtype=np.float64),
                flag=np.zeros(len(feature), dtype=np.uint8))


# ------------------------------------------------------------------ scenes
SCENE_SEED = 7


def synthetic_scene(seed=SCENE_SEED, n_images=4, n_points=60, n_distractors=40, dim=128):
    """Four images of 60 scene points with uniform random base descriptors: each image sees a random 70 % of the
    points, a descriptor is the base plus integer noise in [-2, 2] clipped, and 40 uniform random distractors per
    image follow.  Returns (keypoints, descriptors, point): point[k][n] is the scene point of keypoint n of image k
    or -1; keypoints are distinct random positions."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_points, dim))
    keypoints, descriptors, point = [], [], []
    for _ in range(n_images):
        seen = np.sort(rng.permutation(n_points)[:int(round(0.7 * n_points))])
        d = np.clip(base[seen] + rng.integers(-2, 3, (len(seen), dim)), 0, 255)
        d = np.concatenate([d, rng.integers(0, 256, (n_distractors, dim))])
        order = rng.permutation(len(d))  # scene points and distractors interleaved
        descriptors.append(d[order].astype(np.uint8))
        point.append(np.concatenate([seen, np.full(n_distractors, -1)])[order])
        keypoints.append(rng.random((len(d), 2)) * 1000.0)
    return keypoints, descriptors, point


def small_scene(seed=11, dim=64, sizes=(70, 0, 1, 33)):
    """uniform random descriptors with an empty and a one-keypoint image"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (n, dim)).astype(np.uint8) for n in sizes]


SMALL_PAIRS = [(0, 3), (3, 0), (0, 1), (1, 0), (0, 2), (2, 0), (2, 1), (3, 2)]
# (scene, ratio, max_dsq, cross_check) of every fixture entry; "mid" is the median d1 of the scene
FIXTURE_CASES = [("synthetic", 0.8, INT32_MAX, 1), ("synthetic", 1.0, INT32_MAX, 0), ("small", 0.8, INT32_MAX, 1),
                 ("small", 1.0, "mid", 0), ("small", 0.95, "mid", 1)]


def scene_inputs(name):
    if name == "synthetic":
        _, descs, _ = synthetic_scene()
        pairs = list(itertools.combinations(range(4), 2))
    else:
        descs, pairs = small_scene(), SMALL_PAIRS
    desc, img_start = pack(descs)
    return desc, img_start, np.array(pairs, dtype=np.int32)


def fixture():
    return np.load(os.path.join(GOLDEN, "match_descriptors.npz"))


def fixture_cases():
    """(tag, desc, img_start, pairs, ratio, max_dsq, cross_check) of every fixture entry, from the stored inputs"""
    fx = fixture()
    for n, (scene, ratio, max_dsq, cross) in enumerate(FIXTURE_CASES):
        desc, img_start, pairs = (fx[f"{scene}_{k}"] for k in ("desc", "img_start", "pairs"))
        if max_dsq == "mid":
            max_dsq = int(fx[f"{scene}_mid"])
        yield f"case{n}", desc, img_start, pairs, ratio, max_dsq, cross


def same(out, ref, names=OUTPUTS):
    for n in names:
        assert out[n].dtype == ref[n].dtype and out[n].shape == ref[n].shape and np.array_equal(out[n], ref[n]), n


# ------------------------------------------------------------------ the restatement
def test_restatement_matches_the_fixture():
    fx = fixture()
    for scene in ("synthetic", "small"):
        for k, v in zip(("desc", "img_start", "pairs"), scene_inputs(scene)):
            assert fx[f"{scene}_{k}"].dtype == v.dtype and np.array_equal(fx[f"{scene}_{k}"], v), (scene, k)
    for tag, desc, img_start, pairs, ratio, max_dsq, cross in fixture_cases():
        ref = restate(desc, img_start, pairs, ratio, max_dsq, cross)
        same({n: fx[f"{tag}_{n}"] for n in OUTPUTS}, ref)
    assert os.path.getsize(os.path.join(GOLDEN, "match_descriptors.npz")) < 200_000


def test_restatement_on_hand_made_cases():
    def img(*rows):
        d = np.full((len(rows), 64), 100, dtype=np.uint8)
        for r, first in enumerate(rows):
            d[r, :len(first)] = first
        return d
    # image 0: one keypoint, all 100.  Image 1: keypoints 0 and 2 differ from it by 3 in one byte (dsq 9), keypoint
    # 1 by 4 and 3 (dsq 25).  The minimum 9 is tied: nn is the smaller index 0 and the second of the order is the
    # other 9, so d2 == d1 and 9 < r^2 * 9 fails for every ratio in (0, 1]: refused.
    desc, st = pack([img([100]), img([103], [104, 103], [97])])
    for ratio in (1.0, 0.8, 0.01):
        ref = restate(desc, st, [(0, 1)], ratio, INT32_MAX, False)
        assert (ref["nn"].tolist(), ref["d1"].tolist(), ref["d2"].tolist()) == ([0], [9], [9])
        assert ref["match_start"].tolist() == [0, 0]
    # the other way round each keypoint of image 1 has a single candidate: d2 is INT32_MAX, the ratio test is
    # passed, and all three match keypoint 0; the cross-check (nn_rev[0] == 0) keeps only a = 0
    ref = restate(desc, st, [(1, 0)], 0.5, INT32_MAX, False)
    assert ref["nn"].tolist() == [0, 0, 0] and ref["d1"].tolist() == [9, 25, 9] and ref["d2"].tolist() == [INT32_MAX] * 3
    assert (ref["a"].tolist(), ref["b"].tolist(), ref["dsq"].tolist()) == ([0, 1, 2], [0, 0, 0], [9, 25, 9])
    assert ref["nn_rev"].tolist() == [0]
    ref = restate(desc, st, [(1, 0)], 0.5, INT32_MAX, True)
    assert (ref["a"].tolist(), ref["b"].tolist(), ref["match_start"].tolist()) == ([0], [0], [0, 1])
    # max_dsq: 9 passes at 9 and fails at 8
    assert restate(desc, st, [(1, 0)], 0.5, 9, True)["a"].tolist() == [0]
    assert restate(desc, st, [(1, 0)], 0.5, 8, True)["a"].tolist() == []
    # no keypoint in j: nn = -1, d1 = d2 = INT32_MAX, no match; and none in i: nothing at all
    desc, st = pack([img([100], [90]), np.zeros((0, 64), np.uint8)])
    ref = restate(desc, st, [(0, 1), (1, 0)], 1.0, INT32_MAX, False)
    assert ref["nn"].tolist() == [-1, -1] and ref["d1"].tolist() == [INT32_MAX] * 2 and ref["d2"].tolist() == [INT32_MAX] * 2
    assert ref["nn_rev"].tolist() == [-1, -1] and ref["match_start"].tolist() == [0, 0, 0] and len(ref["a"]) == 0
    # a cross-check that removes a forward match.  Image 0: p = 100.., q = 110 in byte 0.  Image 1: u = 108 in byte
    # 0 and v = 140.  dsq(p,u) = 64, dsq(q,u) = 4, dsq(p,v) = 1600, dsq(q,v) = 900: both p and q choose u
    # (64 < 0.81 * 1600 and 4 < 0.81 * 900) but u chooses q, so p -> u goes and q -> u stays.
    desc, st = pack([img([100], [110]), img([108], [140])])
    fwd = restate(desc, st, [(0, 1)], 0.9, INT32_MAX, False)
    assert (fwd["a"].tolist(), fwd["b"].tolist(), fwd["dsq"].tolist()) == ([0, 1], [0, 0], [64, 4])
    assert fwd["d2"].tolist() == [1600, 900] and fwd["nn_rev"].tolist() == [1, 1]
    chk = restate(desc, st, [(0, 1)], 0.9, INT32_MAX, True)
    assert (chk["a"].tolist(), chk["b"].tolist(), chk["dsq"].tolist()) == ([1], [0], [4])
    # the ratio test is one-directional: at ratio 0.3 the pair (1, 0) keeps u -> q (4 < 0.09 * 64) and drops v
    # (900 < 0.09 * 1600 is false), while (0, 1) keeps both p -> u (64 < 144) and q -> u (4 < 81)
    rev = restate(desc, st, [(1, 0)], 0.3, INT32_MAX, False)
    assert (rev["a"].tolist(), rev["b"].tolist()) == ([0], [1])
    assert restate(desc, st, [(0, 1)], 0.3, INT32_MAX, False)["a"].tolist() == [0, 1]
    assert restate(desc, st, [(0, 1)], 0.15, INT32_MAX, False)["a"].tolist() == [1]  # 64 < 0.0225 * 1600 is false


# ------------------------------------------------------------------ header and bindings
ARGS = ["const uint8_t *desc", "int64_t n_kp", "const int64_t *img_start", "int32_t n_images", "int32_t dim",
        "const int32_t *pairs", "int64_t P", "double ratio", "int32_t max_dsq", "int32_t cross_check",
        "int64_t capacity", "int64_t *match_start", "int32_t *match_a", "int32_t *match_b", "int32_t *match_dsq",
        "int32_t *nn", "int32_t *d1", "int32_t *d2", "int32_t *nn_rev", "int device"]


def test_header_declares_the_entry_point():
    txt = open(os.path.join(REPO, "include", "sfmcore.h")).read()
    m = re.search(r"\bint\s+sfm_match_descriptors\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/sfmcore.h does not declare sfm_match_descriptors"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ARGS
    assert "forward direction only" in txt
    import _sfmcore
    assert hasattr(_sfmcore._lib, "sfm_match_descriptors")
    assert len(dict((n, a) for n, _, a in _sfmcore.SIGNATURES)["sfm_match_descriptors"]) == len(ARGS)
    import sfm_io
    import sfm_multiview
    assert sfm_multiview.match_descriptors is sfm_io.match_descriptors


def raw_call(core, desc, img_start, pairs, dim=None, ratio=0.8, max_dsq=INT32_MAX, cross_check=1, capacity=64,
             null=()):
    """the C entry point with sentinel-filled outputs; returns (rc, outputs)"""
    desc = np.ascontiguousarray(desc, dtype=np.uint8)
    img_start = np.ascontiguousarray(img_start, dtype=np.int64)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    outs = dict(match_start=np.full(16, -7, dtype=np.int64))
    outs.update({k: np.full(64, -7, dtype=np.int32) for k in ("a", "b", "dsq", "nn", "d1", "d2", "nn_rev")})
    P, I32, I64 = core._p, core._i32, core._i64
    ptr = {k: (None if k in null else P(v, I64 if k == "match_start" else I32)) for k, v in outs.items()}
    rc = core._lib.sfm_match_descriptors(None if "desc" in null else P(desc, core._u8), len(desc),
                                         None if "img_start" in null else P(img_start, I64), len(img_start) - 1,
                                         desc.shape[1] if dim is None else dim,
                                         None if "pairs" in null else P(pairs, I32), len(pairs), ratio, max_dsq,
                                         cross_check, capacity, ptr["match_start"], ptr["a"], ptr["b"], ptr["dsq"],
                                         ptr["nn"], ptr["d1"], ptr["d2"], ptr["nn_rev"], 0)
    return rc, outs


def test_arguments_are_refused_before_a_device_is_looked_for():
    """each SFM_ERR_ARG case through the C ABI: -1 and no output touched (no GPU: the checks come first)"""
    import _sfmcore as core
    rng = np.random.default_rng(0)
    desc = rng.integers(0, 256, (8, 64)).astype(np.uint8)
    st, pairs = np.array([0, 5, 8]), [(0, 1)]  # images of 5 and 3 keypoints: the bound is 5, or 3 with cross_check
    big = np.zeros((2 ** 20 + 2, 64), dtype=np.uint8)
    cases = {"null_desc": dict(null=("desc",)), "null_img_start": dict(null=("img_start",)),
             "null_pairs": dict(null=("pairs",)), "null_match_start": dict(null=("match_start",)),
             "null_a": dict(null=("a",)), "null_b": dict(null=("b",)), "null_dsq": dict(null=("dsq",)),
             "dim_96": dict(dim=96), "dim_0": dict(dim=0), "dim_512": dict(dim=512),
             "start": dict(img_start=np.array([1, 5, 8])), "decreasing": dict(img_start=np.array([0, 9, 8])),
             "short": dict(img_start=np.array([0, 5, 7])), "image_high": dict(pairs=[(0, 2)]),
             "image_negative": dict(pairs=[(-1, 1)]), "same_image": dict(pairs=[(1, 1)]),
             "ratio_0": dict(ratio=0.0), "ratio_above_1": dict(ratio=1.0000001), "ratio_negative": dict(ratio=-0.5),
             "ratio_nan": dict(ratio=float("nan")), "ratio_inf": dict(ratio=float("inf")),
             "max_dsq_negative": dict(max_dsq=-1), "capacity_cross": dict(capacity=2),
             "capacity_forward": dict(capacity=4, cross_check=0),
             "too_many_keypoints": dict(desc=big, img_start=np.array([0, 2 ** 20 + 1, 2 ** 20 + 2]),
                                        capacity=2 ** 21)}
    for name, change in cases.items():
        a = dict(desc=desc, img_start=st, pairs=pairs)
        a.update(change)
        rc, outs = raw_call(core, a.pop("desc"), a.pop("img_start"), a.pop("pairs"), **a)
        assert rc == -1, name
        assert all((v == -7).all() for v in outs.values()), name
        assert core._lib.sfm_last_error().startswith(b"argument:"), name
    # the bound itself is accepted as far as the arguments go: the call then looks for a device
    for cross, cap in ((1, 3), (0, 5)):
        rc, _ = raw_call(core, desc, st, pairs, cross_check=cross, capacity=cap)
        assert rc == 0 or not core._lib.sfm_last_error().startswith(b"argument:")
    with np.testing.assert_raises(core.SfmCoreError):
        core.match_descriptors(desc, st, pairs, ratio=1.5)


def test_no_pairs_need_no_device():
    import _sfmcore as core
    rng = np.random.default_rng(1)
    desc = rng.integers(0, 256, (8, 128)).astype(np.uint8)
    rc, outs = raw_call(core, desc, [0, 5, 8], np.zeros((0, 2)), capacity=0, null=("pairs", "a", "b", "dsq"))
    assert rc == 0 and outs["match_start"][0] == 0 and (outs["match_start"][1:] == -7).all()
    out = core.match_descriptors(desc, [0, 5, 8], np.zeros((0, 2), np.int32), want_diagnostics=True)
    same(out, restate(desc, [0, 5, 8], [], 0.8, INT32_MAX, True))
    from sfm_io import match_descriptors
    kps = [rng.random((5, 2)), rng.random((3, 2))]
    store, pair_ij, ms, a, b, dsq = match_descriptors(kps, [desc[:5], desc[5:]], pairs=[])
    assert len(store) == 0 and store.n_features == 0 and store.n_images == 2 and pair_ij.shape == (0, 2)
    assert ms.tolist() == [0] and len(a) == len(b) == len(dsq) == 0
    assert store.feature.dtype == np.int32 and store.image.dtype == np.int32 and store.x.dtype == np.float64


def test_python_layer_refuses_bad_inputs():
    from sfm_io import match_descriptors
    rng = np.random.default_rng(2)
    d = [rng.integers(0, 256, (4, 128)).astype(np.uint8), rng.integers(0, 256, (3, 128)).astype(np.uint8)]
    k = [rng.random((4, 2)), rng.random((3, 2))]
    nan = [k[0].copy(), k[1]]
    nan[0][2, 1] = np.nan
    ragged = [d[0], rng.integers(0, 256, (3, 64)).astype(np.uint8)]
    bad = [dict(keypoints=k, descriptors=[d[0].astype(np.float32), d[1]]), dict(keypoints=k, descriptors=ragged),
           dict(keypoints=k[:1], descriptors=d), dict(keypoints=[k[0][:3], k[1]], descriptors=d),
           dict(keypoints=nan, descriptors=d), dict(keypoints=k, descriptors=d, pairs=[(0, 0)]),
           dict(keypoints=k, descriptors=d, pairs=[(0, 2)]), dict(keypoints=k, descriptors=d, ratio=0.0),
           dict(keypoints=k, descriptors=d, max_distance=-1.0),
           dict(keypoints=k, descriptors=[d[0][:, :32], d[1][:, :32]])]
    for kw in bad:
        with np.testing.assert_raises(ValueError):
            match_descriptors(**kw)


def test_store_of_matches_has_read_matchings_layout():
    """match_store alone (host code): rows of two observations, images ascending inside the row"""
    from sfm_io import match_store, read_matching
    kps = [np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([[5.0, 6.0]]), np.array([[7.0, 8.0], [9.0, 10.0]])]
    pairs = np.array([(0, 2), (2, 1)])
    ref = dict(match_start=np.array([0, 2, 3]), a=np.array([0, 1], np.int32).tolist() + [1], b=[1, 0, 0])
    st = match_store(kps, pairs, ref["match_start"], np.array(ref["a"], np.int32), np.array(ref["b"], np.int32))
    want = store_arrays(kps, pairs, {k: np.asarray(v) for k, v in ref.items()})
    assert st.feature.tolist() == [0, 0, 1, 1, 2, 2] and st.image.tolist() == [0, 2, 0, 2, 1, 2]
    assert st.x.tolist() == [1.0, 9.0, 3.0, 7.0, 5.0, 9.0] and st.y.tolist() == [2.0, 10.0, 4.0, 8.0, 6.0, 10.0]
    p3 = read_matching(os.path.join(GOLDEN, "P3Data"), 5)
    for n in ("feature", "image", "x", "y", "flag"):
        assert getattr(st, n).dtype == getattr(p3, n).dtype == want[n].dtype, n
        assert np.array_equal(getattr(st, n), want[n]), n
    assert st.n_features == 3 and st.n_images == 3 and st._row_start.tolist() == [0, 2, 4, 6]


# ------------------------------------------------------------------ the synthetic scene
def synthetic_reference():
    """the scene, its restatement at ratio 0.8 with the cross-check, the store's arrays and the merged tracks"""
    keypoints, descriptors, point = synthetic_scene()
    desc, img_start = pack(descriptors)
    pairs = np.array(list(itertools.combinations(range(4), 2)), dtype=np.int32)
    ref = restate(desc, img_start, pairs, 0.8, INT32_MAX, True)
    arrays = store_arrays(keypoints, pairs, ref)
    row_start = 2 * np.arange(len(ref["a"]) + 1, dtype=np.int64)
    tracks = mt.restate(row_start, arrays["image"], arrays["x"], arrays["y"], mt.DROP)
    merged = mt.merged_arrays(tracks, arrays["image"], arrays["x"], arrays["y"], arrays["flag"])
    return dict(keypoints=keypoints, descriptors=descriptors, point=point, pairs=pairs, ref=ref, arrays=arrays,
                row_start=row_start, tracks=tracks, merged=merged)


def test_synthetic_scene_finds_every_true_match_and_one_track_per_point():
    s = synthetic_reference()
    point, ref, pairs = s["point"], s["ref"], s["pairs"]
    found = set()
    for p, (i, j) in enumerate(pairs):
        for m in range(ref["match_start"][p], ref["match_start"][p + 1]):
            found.add((int(i), int(ref["a"][m]), int(j), int(ref["b"][m])))
    # a condition on the inputs: true distances are at most 128 * 16 = 2,048, random ones about 1.4 M
    n_true = 0
    for i, j in pairs:
        for a in np.where(point[i] >= 0)[0]:
            b = np.where(point[j] == point[i][a])[0]
            if len(b):
                n_true += 1
                assert (int(i), int(a), int(j), int(b[0])) in found
    assert n_true > 100 and ref["dsq"][ref["dsq"] <= 2048].size >= n_true
    # the merged rows: exactly one track per scene point seen by at least two images; whatever else there is
    # consists of distractors only
    tracks, arrays = s["tracks"], s["arrays"]
    assert not tracks["conflict"].any()
    start = np.concatenate([[0], np.cumsum([len(k) for k in s["keypoints"]])])
    xy_to_kp = {(k, float(x), float(y)): n for k in range(4) for n, (x, y) in enumerate(s["keypoints"][k])}
    per_point = {}
    for t in range(len(tracks["track_label"])):
        obs = tracks["track_obs"][tracks["track_start"][t]:tracks["track_start"][t + 1]]
        pts = {int(point[arrays["image"][o]][xy_to_kp[(int(arrays["image"][o]), arrays["x"][o], arrays["y"][o])]])
               for o in obs}
        assert len(pts) == 1  # a track never mixes scene points, nor a point with a distractor
        pt = pts.pop()
        if pt >= 0:
            per_point.setdefault(pt, []).append(t)
            seen_in = [k for k in range(4) if pt in point[k]]
            assert sorted(arrays["image"][obs].tolist()) == seen_in  # the whole track, every view of the point
    seen_twice = [pt for pt in range(60) if sum(pt in point[k] for k in range(4)) >= 2]
    assert sorted(per_point) == seen_twice and all(len(v) == 1 for v in per_point.values())
    assert start[-1] == sum(len(d) for d in s["descriptors"])
