"""Guided descriptor matching (sfm_match_descriptors_guided) restated in plain
numpy from the definitions of include/sfmcore.h: the gate as separate fp64
operations in vp_inlier's order (numpy never fuses a multiply and an add), the
(dsq, index) order of tests/test_match_descriptors.py over the candidates only,
and the tests as the header writes them.  Checked here against
tests/golden/match_guided.npz, which an independent loop-written restatement
produced (tests/golden/make_golden_match_guided.py; none of it comes from the
reference, which has no matcher), and against hand-made cases;
tests/test_match_guided_gpu.py compares the device call with it for equality.
No GPU needed.
"""
import functools
import itertools
import os
import re

import numpy as np

import test_match_descriptors as md
from conftest import GOLDEN, REPO
from test_match_descriptors import INT32_MAX, first_two, pack, same

OUTPUTS = md.OUTPUTS + ("n_cand",)
K_PIX = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])


def gate_terms(F, xa, xb):
    """e (n, m) and den (n, m) of vp_inlier for every keypoint (x, y) of xa against every (u, v) of xb"""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    xa, xb = np.asarray(xa, dtype=np.float64).reshape(-1, 2), np.asarray(xb, dtype=np.float64).reshape(-1, 2)
    x, y = xa[:, 0][:, None], xa[:, 1][:, None]
    u, v = xb[:, 0][None, :], xb[:, 1][None, :]
    with np.errstate(all="ignore"):
        l0 = (F[0] * x + F[1] * y) + F[2]
        l1 = (F[3] * x + F[4] * y) + F[5]
        l2 = (F[6] * x + F[7] * y) + F[8]
        m0 = (F[0] * u + F[3] * v) + F[6]
        m1 = (F[1] * u + F[4] * v) + F[7]
        e = (u * l0 + v * l1) + l2
        den = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1)
    return e, den


def gate_matrix(F, xa, xb, gate):
    """gate_p(a, b) as an (n, m) bool matrix"""
    e, den = gate_terms(F, xa, xb)
    with np.errstate(all="ignore"):
        thr2 = np.float64(gate) * np.float64(gate)
        return (den > 0.0) & (e * e < thr2 * den)


def first_two_over(D, G):
    """first_two of every row of D over the columns where G is set; indices are D's"""
    n = D.shape[0]
    nn, d1, d2 = np.full(n, -1, np.int32), np.full(n, INT32_MAX, np.int32), np.full(n, INT32_MAX, np.int32)
    for r in range(n):
        cols = np.flatnonzero(G[r])
        k, d1[r:r + 1], d2[r:r + 1] = first_two(D[r:r + 1, cols])
        if len(cols):
            nn[r] = cols[k[0]]
    return nn, d1, d2


def restate_guided(desc, xy, img_start, pairs, F, gate, ratio=0.8, max_dsq=INT32_MAX, cross_check=True):
    """the outputs of sfm_match_descriptors_guided as a dict of numpy arrays"""
    desc = np.asarray(desc).astype(np.int64)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    F = np.asarray(F, dtype=np.float64).reshape(-1, 9)
    out = {k: [] for k in OUTPUTS[1:]}
    match_start = [0]
    r2 = np.float64(ratio) * np.float64(ratio)
    for p, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        si, sj = slice(img_start[i], img_start[i + 1]), slice(img_start[j], img_start[j + 1])
        A, B = desc[si], desc[sj]
        D = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
        G = gate_matrix(F[p], xy[si], xy[sj], gate)
        nn, d1, d2 = first_two_over(D, G)
        nn_rev = first_two_over(D.T, G.T)[0]
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
        for k, v in (("nn", nn), ("d1", d1), ("d2", d2), ("nn_rev", nn_rev), ("n_cand", G.sum(axis=1))):
            out[k].extend(v.tolist())
    res = {k: np.array(v, dtype=np.int32) for k, v in out.items()}
    res["match_start"] = np.array(match_start, dtype=np.int64)
    return res


# ------------------------------------------------------------------ geometry and scenes
def rot_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def fundamental(R_i, C_i, R_j, C_j, K=K_PIX):
    """x_j^T F x_i = 0 for cameras x_cam = R (X - C), of unit Frobenius norm"""
    R, t = R_j @ R_i.T, R_j @ (C_i - C_j)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return F / np.linalg.norm(F)


def random_rank2(rng):
    """a random 3 x 3 matrix of rank 2 and unit Frobenius norm"""
    U, s, Vt = np.linalg.svd(rng.standard_normal((3, 3)))
    F = U @ np.diag([s[0], s[1], 0.0]) @ Vt
    return F / np.linalg.norm(F)


def random_epipolar(rng):
    """the F of a random second camera about one baseline away: epipolar lines that cross the frame"""
    t = rng.standard_normal(3)
    return fundamental(np.eye(3), np.zeros(3), rot_y(rng.uniform(-0.2, 0.2)), t / np.linalg.norm(t))


def frame_points(rng, n):
    """n uniform random keypoints in a 640 x 480 frame"""
    return rng.random((n, 2)) * np.array([640.0, 480.0])


def sampson(F, xa, xb):
    """the Sampson distances in pixels, for choosing inputs only (never for a decision)"""
    e, den = gate_terms(F, xa, xb)
    with np.errstate(all="ignore"):
        return np.sqrt(e * e / den)


def gate_with_all_three(F, xa, xb):
    """a gate at which some row has no candidate, some one and some two or more, or None: a condition on the
    inputs, looked for among the rows' two smallest Sampson distances"""
    s = np.sort(sampson(F, xa, xb), axis=1)[:, :2].reshape(-1)
    for g in np.sort(s[np.isfinite(s)]) * 1.0000001:
        n = gate_matrix(F, xa, xb, g).sum(axis=1)
        if (n == 0).any() and (n == 1).any() and (n >= 2).any():
            return float(g)
    return None


SMALL_SIZES = (70, 0, 1, 33)
SMALL_PAIRS = [(0, 3), (3, 0), (0, 1), (1, 0), (0, 2), (2, 0), (2, 1), (3, 2), (0, 3)]
NAN_PAIR = 8  # the second (0, 3) has an F with a NaN
SMALL_GATE = 12.0
# (ratio, max_dsq, cross_check) of every fixture entry on the small scene; "mid" is the median finite d1
FIXTURE_CASES = [(0.8, INT32_MAX, 1), (1.0, INT32_MAX, 0), (0.95, "mid", 1)]


def small_scene(seed=17, dim=64):
    """uniform random descriptors and keypoints with an empty and a one-keypoint image, the F of a random camera
    pair per pair and one F that holds a NaN"""
    rng = np.random.default_rng(seed)
    descs = [rng.integers(0, 256, (n, dim)).astype(np.uint8) for n in SMALL_SIZES]
    kps = [frame_points(rng, n) for n in SMALL_SIZES]
    F = np.array([random_epipolar(rng) for _ in SMALL_PAIRS])
    F[NAN_PAIR, 1, 2] = np.nan
    desc, img_start = pack(descs)
    return desc, np.concatenate(kps), img_start, np.array(SMALL_PAIRS, dtype=np.int32), F


BORDER_N = 200                 # rows of the borderline pair
BORDER_STEPS = (-2, -1, 0, 1, 2, 3)  # ulps of v, outwards, from the last double inside the band


def step(v, k):
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


@functools.lru_cache(maxsize=None)
def border_scene(seed=23, dim=64, gate=3.0):
    """One pair on the threshold curve.  Row k of image 0 is a random keypoint; for a random u the v with
    e^2 = thr2 den is bracketed by bisection on the fp64 predicate itself down to two neighbouring doubles, the
    last inside and the first outside, and image 1 holds (u, v) for v stepped BORDER_STEPS ulps from the last
    inside: columns 6 k .. 6 k + 5.  A fused multiply-add or a loose prefilter changes decisions exactly here.
    Returns (desc, xy, img_start, pairs, F, gate, rows, cols): (rows[n], cols[n]) are the designated pairs."""
    rng = np.random.default_rng(seed)
    F = fundamental(np.eye(3), np.zeros(3), rot_y(0.15), np.array([1.0, 0.1, 0.05]))
    xa = frame_points(rng, BORDER_N)
    xb = np.zeros((BORDER_N * len(BORDER_STEPS), 2))
    for k in range(BORDER_N):
        u = rng.random() * 640.0
        l = F @ np.array([xa[k, 0], xa[k, 1], 1.0])
        lo = -(u * l[0] + l[2]) / l[1]          # on the line: inside
        out = 1 if rng.random() < 0.5 else -1   # which way along v the band is left
        hi = lo + 40.0 * out                    # 40 pixels along v: outside a 3 pixel band
        assert gate_matrix(F, xa[k], [u, lo], gate)[0, 0] and not gate_matrix(F, xa[k], [u, hi], gate)[0, 0]
        while True:
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if gate_matrix(F, xa[k], [u, mid], gate)[0, 0]:
                lo = mid
            else:
                hi = mid
        for n, s in enumerate(BORDER_STEPS):
            xb[len(BORDER_STEPS) * k + n] = (u, step(lo, s * out))
    descs = [rng.integers(0, 256, (len(x), dim)).astype(np.uint8) for x in (xa, xb)]
    desc, img_start = pack(descs)
    rows = np.repeat(np.arange(BORDER_N), len(BORDER_STEPS))
    return (desc, np.concatenate([xa, xb]), img_start, np.array([(0, 1)], dtype=np.int32), F[None], gate, rows,
            np.arange(len(xb)))


def fixture():
    return np.load(os.path.join(GOLDEN, "match_guided.npz"))


def fixture_cases():
    """(tag, desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross_check) of every fixture entry, from the
    stored inputs: case0.. on the small scene, then "border" """
    fx = fixture()
    small = [fx[f"small_{k}"] for k in ("desc", "xy", "img_start", "pairs", "F")]
    for n, (ratio, max_dsq, cross) in enumerate(FIXTURE_CASES):
        if max_dsq == "mid":
            max_dsq = int(fx["small_mid"])
        yield (f"case{n}", *small, SMALL_GATE, ratio, max_dsq, cross)
    yield ("border", *(fx[f"border_{k}"] for k in ("desc", "xy", "img_start", "pairs", "F")), float(fx["border_gate"]),
           1.0, INT32_MAX, 1)


# ------------------------------------------------------------------ the restatement
def test_restatement_matches_the_fixture():
    fx = fixture()
    for name, scene in (("small", small_scene()), ("border", border_scene()[:5])):
        for k, v in zip(("desc", "xy", "img_start", "pairs", "F"), scene):
            assert fx[f"{name}_{k}"].dtype == v.dtype and np.array_equal(fx[f"{name}_{k}"], v, equal_nan=True), (name, k)
    for tag, desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross in fixture_cases():
        ref = restate_guided(desc, xy, img_start, pairs, F, gate, ratio, max_dsq, cross)
        same({n: fx[f"{tag}_{n}"] for n in OUTPUTS}, ref, OUTPUTS)
    assert os.path.getsize(os.path.join(GOLDEN, "match_guided.npz")) < 300_000


def test_small_scene_has_every_kind_of_row():
    desc, xy, img_start, pairs, F = small_scene()
    ref = restate_guided(desc, xy, img_start, pairs, F, SMALL_GATE, 1.0, INT32_MAX, False)
    n = ref["n_cand"][:70]  # pair (0, 3)
    assert (n == 0).any() and (n == 1).any() and (n >= 2).any()
    assert ((ref["nn"] == -1) == (ref["n_cand"] == 0)).all() and ((ref["d2"] == INT32_MAX) == (ref["n_cand"] < 2)).all()
    plain = md.restate(desc, img_start, pairs, 1.0, INT32_MAX, False)
    assert (ref["nn"] != plain["nn"]).any()
    # the pair whose F holds a NaN is empty
    assert (ref["n_cand"][-70:] == 0).all() and (ref["nn"][-70:] == -1).all() and (ref["nn_rev"][-33:] == -1).all()
    assert ref["match_start"][NAN_PAIR] == ref["match_start"][NAN_PAIR + 1]


def test_borderline_pairs_show_both_outcomes():
    desc, xy, img_start, pairs, F, gate, rows, cols = border_scene()
    assert len(rows) >= 200 * len(BORDER_STEPS)
    G = gate_matrix(F[0], xy[:BORDER_N], xy[BORDER_N:], gate)
    hit = G[rows, cols].reshape(BORDER_N, len(BORDER_STEPS))
    # step 0 is the last double inside and step 1 the first outside, for every one of the 200 rows
    assert hit[:, BORDER_STEPS.index(0)].all() and not hit[:, BORDER_STEPS.index(1)].any()
    assert hit.any() and not hit.all()
    # and they are borderline: e^2 and thr2 den agree to a few ulps
    e, den = gate_terms(F[0], xy[:BORDER_N], xy[BORDER_N:])
    lhs, rhs = (e * e)[rows, cols], (gate * gate * den)[rows, cols]
    assert (np.abs(lhs - rhs) <= 1e-9 * rhs).all()


def test_restatement_on_hand_made_cases():
    def img(*rows):
        d = np.full((len(rows), 64), 100, dtype=np.uint8)
        for r, first in enumerate(rows):
            d[r, :len(first)] = first
        return d
    # rectified stereo: l = (0, -1, y), m0 = 0, m1 = 1, so e = y - v and den = 2; at gate 1 a pair is a candidate
    # when (y - v)^2 < 2
    F = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    xa = np.array([[5.0, 10.0], [6.0, 50.0], [7.0, 100.0]])
    xb = np.array([[1.0, 10.0], [2.0, 50.0], [3.0, 51.0], [4.0, 200.0]])
    # a0 is b3's descriptor (dsq 0) but b3 is outside its band; its only candidate is b0 (dsq 9).  a1 has b1 and b2
    # inside, both at dsq 4.  a2 has no candidate.
    desc, st = pack([img([100], [110], [120]), img([103], [112], [108], [100])])
    xy = np.concatenate([xa, xb])
    plain = md.restate(desc, st, [(0, 1)], 1.0, INT32_MAX, False)
    ref = restate_guided(desc, xy, st, [(0, 1)], [F], 1.0, 1.0, INT32_MAX, False)
    assert ref["n_cand"].tolist() == [1, 2, 0]
    # a row with no candidate
    assert ref["nn"][2] == -1 and ref["d1"][2] == INT32_MAX and ref["d2"][2] == INT32_MAX
    # a row with one candidate: d2 == INT32_MAX and the ratio test is passed at any ratio
    assert (ref["nn"][0], ref["d1"][0], ref["d2"][0]) == (0, 9, INT32_MAX)
    assert restate_guided(desc, xy, st, [(0, 1)], [F], 1.0, 0.01, INT32_MAX, False)["a"].tolist() == [0]
    # the unguided nearest gated out
    assert plain["nn"][0] == 3 and plain["d1"][0] == 0 and ref["nn"][0] != plain["nn"][0]
    # a tie on dsq inside the band goes to the smaller index, and d2 == d1 refuses the match at every ratio
    assert (ref["nn"][1], ref["d1"][1], ref["d2"][1]) == (1, 4, 4)
    assert (ref["a"].tolist(), ref["b"].tolist(), ref["dsq"].tolist()) == ([0], [0], [9])
    # nn_rev over the same candidates: b2's only candidate is a1, b3 has none
    assert ref["nn_rev"].tolist() == [0, 1, 1, -1]
    assert restate_guided(desc, xy, st, [(0, 1)], [F], 1.0, 1.0, INT32_MAX, True)["a"].tolist() == [0]
    # at gate 0.5 thr2 den = 0.5: only v == y is left, and b2 (one pixel off) goes
    wide = restate_guided(desc, xy, st, [(0, 1)], [F], 0.5, 1.0, INT32_MAX, False)
    assert wide["n_cand"].tolist() == [1, 1, 0]
    # gate 0 admits nothing, not even e == 0
    assert restate_guided(desc, xy, st, [(0, 1)], [F], 0.0, 1.0, INT32_MAX, False)["n_cand"].tolist() == [0, 0, 0]
    # the pair listed the other way round takes F^T: the same candidates
    back = restate_guided(desc, xy, st, [(1, 0)], [F.T], 1.0, 1.0, INT32_MAX, False)
    assert back["n_cand"].tolist() == [1, 1, 1, 0] and back["nn"].tolist() == [0, 1, 1, -1]
    # a NaN F: the pair is empty
    bad = F.copy()
    bad[0, 0] = np.nan
    ref = restate_guided(desc, xy, st, [(0, 1), (0, 1)], [bad, F], 1.0, 1.0, INT32_MAX, True)
    assert ref["n_cand"].tolist() == [0, 0, 0, 1, 2, 0] and ref["nn"][:3].tolist() == [-1] * 3
    assert ref["nn_rev"][:4].tolist() == [-1] * 4 and ref["match_start"].tolist() == [0, 0, 1]


def test_all_admitting_gate_is_the_unguided_call():
    """gate = 1e200: thr2 is +inf and every pair with den > 0 passes"""
    desc, xy, img_start, pairs, F = small_scene()
    keep = [p for p in range(len(pairs)) if p != NAN_PAIR]
    pairs, F = pairs[keep], F[keep]
    n = np.diff(img_start)
    for p, (i, j) in enumerate(pairs):
        _, den = gate_terms(F[p], xy[img_start[i]:img_start[i + 1]], xy[img_start[j]:img_start[j + 1]])
        assert (den > 0).all()
    for ratio, cross in ((0.8, True), (1.0, False)):
        ref = restate_guided(desc, xy, img_start, pairs, F, 1e200, ratio, INT32_MAX, cross)
        same(ref, md.restate(desc, img_start, pairs, ratio, INT32_MAX, cross), md.OUTPUTS)
        assert np.array_equal(ref["n_cand"], np.repeat(n[pairs[:, 1]], n[pairs[:, 0]]))


# ------------------------------------------------------------------ header and bindings
ARGS = ["const uint8_t *desc", "const double *xy", "int64_t n_kp", "const int64_t *img_start", "int32_t n_images",
        "int32_t dim", "const int32_t *pairs", "const double *F", "int64_t P", "double gate", "double ratio",
        "int32_t max_dsq", "int32_t cross_check", "int64_t capacity", "int64_t *match_start", "int32_t *match_a",
        "int32_t *match_b", "int32_t *match_dsq", "int32_t *nn", "int32_t *d1", "int32_t *d2", "int32_t *nn_rev",
        "int32_t *n_cand", "int device"]


def test_header_declares_the_entry_point():
    txt = open(os.path.join(REPO, "include", "sfmcore.h")).read()
    m = re.search(r"\bint\s+sfm_match_descriptors_guided\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/sfmcore.h does not declare sfm_match_descriptors_guided"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ARGS
    assert "gate_p = den > 0 && e e < thr2 den" in txt
    import _sfmcore
    assert hasattr(_sfmcore._lib, "sfm_match_descriptors_guided")
    assert len(dict((n, a) for n, _, a in _sfmcore.SIGNATURES)["sfm_match_descriptors_guided"]) == len(ARGS)
    import sfm_io
    import sfm_multiview
    assert sfm_multiview.match_descriptors_guided is sfm_io.match_descriptors_guided
    assert callable(sfm_multiview.rematch_verified)


def raw_call(core, desc, xy, img_start, pairs, F, gate=4.0, dim=None, ratio=0.8, max_dsq=INT32_MAX, cross_check=1,
             capacity=64, null=(), size=64):
    """the C entry point with sentinel-filled outputs; returns (rc, outputs)"""
    desc = np.ascontiguousarray(desc, dtype=np.uint8)
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    img_start = np.ascontiguousarray(img_start, dtype=np.int64)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    F = np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9)
    outs = dict(match_start=np.full(16, -7, dtype=np.int64))
    outs.update({k: np.full(size, -7, dtype=np.int32) for k in ("a", "b", "dsq", "nn", "d1", "d2", "nn_rev", "n_cand")})
    P, I32, I64 = core._p, core._i32, core._i64
    ptr = {k: (None if k in null else P(v, I64 if k == "match_start" else I32)) for k, v in outs.items()}
    rc = core._lib.sfm_match_descriptors_guided(
        None if "desc" in null else P(desc, core._u8), None if "xy" in null else P(xy), len(desc),
        None if "img_start" in null else P(img_start, I64), len(img_start) - 1, desc.shape[1] if dim is None else dim,
        None if "pairs" in null else P(pairs, I32), None if "F" in null else P(F), len(pairs), gate, ratio, max_dsq,
        cross_check, capacity, ptr["match_start"], ptr["a"], ptr["b"], ptr["dsq"], ptr["nn"], ptr["d1"], ptr["d2"],
        ptr["nn_rev"], ptr["n_cand"], 0)
    return rc, outs


def test_arguments_are_refused_before_a_device_is_looked_for():
    """each SFM_ERR_ARG case through the C ABI: -1 and no output touched (no GPU: the checks come first)"""
    import _sfmcore as core
    rng = np.random.default_rng(0)
    desc = rng.integers(0, 256, (8, 64)).astype(np.uint8)
    xy = frame_points(rng, 8)
    st, pairs, F = np.array([0, 5, 8]), [(0, 1)], random_rank2(rng)[None]
    big = np.zeros((2 ** 20 + 2, 64), dtype=np.uint8)
    cases = {"null_desc": dict(null=("desc",)), "null_img_start": dict(null=("img_start",)),
             "null_pairs": dict(null=("pairs",)), "null_match_start": dict(null=("match_start",)),
             "null_a": dict(null=("a",)), "null_b": dict(null=("b",)), "null_dsq": dict(null=("dsq",)),
             "null_xy": dict(null=("xy",)), "null_F": dict(null=("F",)),
             "gate_negative": dict(gate=-1.0), "gate_nan": dict(gate=float("nan")), "gate_inf": dict(gate=float("inf")),
             "dim_96": dict(dim=96), "dim_0": dict(dim=0), "dim_512": dict(dim=512),
             "start": dict(img_start=np.array([1, 5, 8])), "decreasing": dict(img_start=np.array([0, 9, 8])),
             "short": dict(img_start=np.array([0, 5, 7])), "image_high": dict(pairs=[(0, 2)]),
             "image_negative": dict(pairs=[(-1, 1)]), "same_image": dict(pairs=[(1, 1)]),
             "ratio_0": dict(ratio=0.0), "ratio_above_1": dict(ratio=1.0000001), "ratio_negative": dict(ratio=-0.5),
             "ratio_nan": dict(ratio=float("nan")), "ratio_inf": dict(ratio=float("inf")),
             "max_dsq_negative": dict(max_dsq=-1), "capacity_cross": dict(capacity=2),
             "capacity_forward": dict(capacity=4, cross_check=0), "cross_check_2": dict(cross_check=2),
             "too_many_keypoints": dict(desc=big, xy=np.zeros((len(big), 2)),
                                        img_start=np.array([0, 2 ** 20 + 1, 2 ** 20 + 2]), capacity=2 ** 21)}
    for name, change in cases.items():
        a = dict(desc=desc, xy=xy, img_start=st, pairs=pairs, F=F)
        a.update(change)
        rc, outs = raw_call(core, a.pop("desc"), a.pop("xy"), a.pop("img_start"), a.pop("pairs"), a.pop("F"), **a)
        assert rc == -1, name
        assert all((v == -7).all() for v in outs.values()), name
        assert core._lib.sfm_last_error().startswith(b"argument:"), name
    # the bound itself, gate 0 and a gate whose square overflows are accepted as far as the arguments go: the call
    # then looks for a device
    for kw in (dict(cross_check=1, capacity=3), dict(cross_check=0, capacity=5), dict(gate=0.0), dict(gate=1e200)):
        rc, _ = raw_call(core, desc, xy, st, pairs, F, **kw)
        assert rc == 0 or not core._lib.sfm_last_error().startswith(b"argument:")
    with np.testing.assert_raises(core.SfmCoreError):
        core.match_descriptors_guided(desc, xy, st, pairs, F, gate=-2.0)
    with np.testing.assert_raises(ValueError):
        core.match_descriptors_guided(desc, xy[:7], st, pairs, F, gate=2.0)
    with np.testing.assert_raises(ValueError):
        core.match_descriptors_guided(desc, xy, st, pairs, np.zeros((2, 3, 3)), gate=2.0)


def test_no_pairs_need_no_device():
    import _sfmcore as core
    rng = np.random.default_rng(1)
    desc = rng.integers(0, 256, (8, 128)).astype(np.uint8)
    xy = frame_points(rng, 8)
    rc, outs = raw_call(core, desc, xy, [0, 5, 8], np.zeros((0, 2)), np.zeros((0, 9)), capacity=0,
                        null=("pairs", "F", "a", "b", "dsq"))
    assert rc == 0 and outs["match_start"][0] == 0 and (outs["match_start"][1:] == -7).all()
    out = core.match_descriptors_guided(desc, xy, [0, 5, 8], np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), 4.0,
                                        want_diagnostics=True)
    same(out, restate_guided(desc, xy, [0, 5, 8], [], [], 4.0), OUTPUTS)
    from sfm_io import match_descriptors_guided
    kps = [xy[:5], xy[5:]]
    store, pair_ij, ms, a, b, dsq = match_descriptors_guided(kps, [desc[:5], desc[5:]], [], np.zeros((0, 3, 3)))
    assert len(store) == 0 and store.n_features == 0 and store.n_images == 2 and pair_ij.shape == (0, 2)
    assert ms.tolist() == [0] and len(a) == len(b) == len(dsq) == 0
    from sfm_multiview import rematch_verified
    failed = (np.zeros(1, np.int64), np.array([[0, 1]]), (np.full((1, 3, 3), np.nan), None, np.zeros(1, np.int32), None,
                                                          None, None, np.full(1, -2, np.int32)), None, None)
    store, pair_ij, ms, a, b, dsq = rematch_verified(kps, [desc[:5], desc[5:]], failed)
    assert len(store) == 0 and pair_ij.shape == (0, 2) and ms.tolist() == [0]


def test_python_layer_refuses_bad_inputs():
    from sfm_io import match_descriptors_guided
    rng = np.random.default_rng(2)
    d = [rng.integers(0, 256, (4, 128)).astype(np.uint8), rng.integers(0, 256, (3, 128)).astype(np.uint8)]
    k = [frame_points(rng, 4), frame_points(rng, 3)]
    F = random_rank2(rng)[None]
    nan = [k[0].copy(), k[1]]
    nan[0][2, 1] = np.nan
    ok = dict(keypoints=k, descriptors=d, pairs=[(0, 1)], F=F)
    bad = [dict(F=F[0]), dict(F=np.zeros((2, 3, 3))), dict(F=np.zeros((1, 9))), dict(F=np.zeros((1, 3, 4))),
           dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")),
           dict(descriptors=[d[0].astype(np.float32), d[1]]), dict(keypoints=k[:1]), dict(keypoints=nan),
           dict(pairs=[(0, 0)]), dict(pairs=[(0, 2)]), dict(ratio=0.0), dict(max_distance=-1.0)]
    for change in bad:
        kw = dict(ok)
        kw.update(change)
        with np.testing.assert_raises((ValueError, TypeError)):
            match_descriptors_guided(**kw)


# ------------------------------------------------------------------ the scene with twins
TWINS = 5  # scene points 2 m and 2 m + 1, m < TWINS, share a base descriptor


def twin_scene(seed=31, n_views=4, n_points=60, dim=128):
    """Four views with known poses of 60 scene points, every point seen by every view; a descriptor is the point's
    base plus integer noise in [-2, 2], and the first five pairs of points share their base: repeated structure.
    Returns (keypoints, descriptors, pairs, F): pairs the six combinations, F[p] with x_j^T F x_i = 0."""
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-2, 2, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(6, 10, n_points)])
    base = rng.integers(0, 256, (n_points, dim))
    for m in range(TWINS):
        base[2 * m + 1] = base[2 * m]
    R = [rot_y(-0.04 * k) for k in range(n_views)]
    C = [np.array([0.7 * k, 0.1 * k, 0.05 * k]) for k in range(n_views)]
    keypoints, descriptors = [], []
    for k in range(n_views):
        x = (K_PIX @ (R[k] @ (X - C[k]).T)).T
        keypoints.append(x[:, :2] / x[:, 2:])
        descriptors.append(np.clip(base + rng.integers(-2, 3, base.shape), 0, 255).astype(np.uint8))
    pairs = np.array(list(itertools.combinations(range(n_views), 2)), dtype=np.int64)
    F = np.array([fundamental(R[i], C[i], R[j], C[j]) for i, j in pairs])
    return keypoints, descriptors, pairs, F


@functools.lru_cache(maxsize=None)
def twin_reference(threshold=4.0, ratio=0.8):
    """the scene with the unguided and the guided restatement at ratio 0.8 with the cross-check"""
    keypoints, descriptors, pairs, F = twin_scene()
    desc, img_start = pack(descriptors)
    xy = np.concatenate(keypoints)
    plain = md.restate(desc, img_start, pairs, ratio, INT32_MAX, True)
    guided = restate_guided(desc, xy, img_start, pairs, F, threshold, ratio, INT32_MAX, True)
    return dict(keypoints=keypoints, descriptors=descriptors, pairs=pairs, F=F, plain=plain, guided=guided,
                threshold=threshold, ratio=ratio)


def matches_of(ref, pairs):
    return {(int(i), int(ref["a"][m]), int(j), int(ref["b"][m])) for p, (i, j) in enumerate(pairs)
            for m in range(ref["match_start"][p], ref["match_start"][p + 1])}


def test_twin_scene_counts():
    """what the GPU test expects of the scene, from the restatement alone"""
    s = twin_reference()
    pairs, F, kps = s["pairs"], s["F"], s["keypoints"]
    twins = set(range(2 * TWINS))
    # conditions on the inputs: a true match lies on its epipolar line, a twin's other half well off it
    for p, (i, j) in enumerate(pairs):
        d = sampson(F[p], kps[i], kps[j])
        assert np.diag(d).max() < 1e-6
        for m in range(TWINS):
            assert d[2 * m, 2 * m + 1] > 2 * s["threshold"] and d[2 * m + 1, 2 * m] > 2 * s["threshold"]
    true = {(int(i), n, int(j), n) for i, j in pairs for n in range(60)}
    plain, guided = matches_of(s["plain"], pairs), matches_of(s["guided"], pairs)
    # the unguided call loses every twin to the ratio test and finds every other true match
    assert not any(m[1] in twins for m in plain) and plain == {m for m in true if m[1] not in twins}
    assert len(plain) == 6 * 50
    # the guided call finds every true match, the twins' among them, and nothing else
    assert guided == true and len(guided) == 6 * 60
