"""Feature extraction on a real MI355X (sfm_extract_features,
sfm_io.extract_features) against the plain-numpy restatement of
tests/test_extract_features.py, each stage from the device's own output of
the stage before: the pyramid against a bound derived from the tap counts, the
candidates for equality, the refinement, the orientations and the descriptors
against the fp64 restatement run on the device's pyramid, candidates, refined
list and keypoints, within the tolerances of tests/golden/extract_features.npz
(the fp32-against-fp64 budget of the restatement alone, both precisions on one
pyramid as here, times 4).  The shapes
straddle the kernels' tiles (blur 32 x 64, detection 8 x 32), not the workload's.
"""
import numpy as np
import pytest

import test_extract_features as ef

pytestmark = pytest.mark.gpu
TH, TW = 32, 64  # the blur tile (EF_TH, EF_TW of csrc/extract_features.hip)


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def tol():
    fx = ef.fixture()
    # the budget taken on one pyramid, as the comparisons here are; it is never above the chained budget
    val = {n: 4.0 * float(fx["budget1_" + n]) for n in ("x", "y", "scale", "response", "angle")}
    dec = {n: 4.0 * float(fx["budget1_dec_" + n]) for n in ("move", "contrast", "edge", "peak")}
    assert all(fx["budget1_" + n] <= fx["budget_" + n] for n in val)
    assert all(fx["budget1_dec_" + n] <= fx["budget_dec_" + n] for n in dec)
    return val, dec


_RUNS = {}


def run(core, key, images):
    """one device call with diagnostics per distinct input, shared among the tests"""
    if key not in _RUNS:
        _RUNS[key] = core.extract_features(np.stack(images), want_diagnostics=True)
    return _RUNS[key]


def image_slices(out, k):
    a, b = out["kp_start"][k], out["kp_start"][k + 1]
    c, d = out["cand_start"][k], out["cand_start"][k + 1]
    return slice(a, b), slice(c, d)


def check_stages(out, images, tol):
    val_tol, dec_tol = tol
    assert out["kp_start"][0] == 0 and np.all(np.diff(out["kp_start"]) >= 0) and out["kp_start"][-1] == len(out["xy"])
    assert out["cand_start"][0] == 0 and out["cand_start"][-1] == len(out["cand"])
    for k, img in enumerate(images):
        H, W = img.shape
        kp, cd = image_slices(out, k)
        # 1. the pyramid, against a bound derived from the tap counts
        want = ef.restate_pyramid(img)
        pyr = ef.unflatten_pyramid(out["pyramid"][k], H, W)
        bounds = ef.pyramid_error_bounds(H, W)
        assert len(pyr) == len(want) == ef.max_octaves(H, W)
        for o in range(len(want)):
            for l in range(ef.S + 3):
                err = np.abs(pyr[o][l].astype(np.float64) - want[o][l]).max()
                assert err <= bounds[o][l], (k, o, l, err, bounds[o][l])
        # 2. the candidates from the device's pyramid: equality, order included
        cands = ef.restate_candidates(pyr)
        assert np.all(out["cand"][cd, 0] == k)
        assert np.array_equal(out["cand"][cd, 1:], cands), (k, len(cands), cd)
        # 3. the refinement from the device's pyramid and candidates
        ref = ef.restate_refine(pyr, cands)
        ok, site, rv = out["ref_ok"][cd], out["ref_site"][cd], out["ref_val"][cd]
        amb = (ref["m_move"] <= dec_tol["move"]) | (ref["m_contrast"] <= dec_tol["contrast"]) | \
              (ref["m_edge"] <= dec_tol["edge"])
        assert np.array_equal(ok[~amb], ref["ok"][~amb]), (k, np.nonzero(ok != ref["ok"])[0])
        both = ok & ref["ok"] & ~amb
        assert np.array_equal(site[both], ref["site"][both])
        step = 2.0 ** cands[:, 0]
        x, y = (site[:, 2] + rv[:, 0].astype(np.float64)) * step, (site[:, 1] + rv[:, 1].astype(np.float64)) * step
        scale = 1.6 * step * 2.0 ** ((site[:, 0] + rv[:, 2].astype(np.float64)) / ef.S)
        print(f"image {k} {H}x{W}: {len(cands)} candidates, {int(ok.sum())} refined, {kp.stop - kp.start} keypoints")
        if both.any():
            dx, dy = np.abs(x - ref["x"])[both].max(), np.abs(y - ref["y"])[both].max()
            ds, dr = np.abs(scale - ref["scale"])[both].max(), np.abs(rv[:, 3] - ref["resp"])[both].max()
            print(f"  refinement: |dx| {dx:.3g} |dy| {dy:.3g} |dscale| {ds:.3g} |dresponse| {dr:.3g}")
            assert dx <= val_tol["x"] and dy <= val_tol["y"] and ds <= val_tol["scale"] and dr <= val_tol["response"]
        # 4. the orientations from the device's refined list
        idx = np.nonzero(ok)[0]
        peaks, m_peak = ef.restate_orient(pyr, cands[idx, 0], site[idx], rv[idx, :3])
        dxy, dsc, dan, dre = out["xy"][kp], out["scale"][kp], out["angle"][kp], out["response"][kp]
        dsite = out["kp_site"][kp]
        assert np.all((dxy[:, 0] >= 0) & (dxy[:, 0] <= W - 1) & (dxy[:, 1] >= 0) & (dxy[:, 1] <= H - 1))
        p, worst = 0, 0.0
        for i, found, m in zip(idx, peaks, m_peak):
            here = (int(cands[i, 0]),) + tuple(int(v) for v in site[i])
            n = len(found)
            if m <= dec_tol["peak"]:  # ambiguous: take the device's count at this location
                n = 0
                while p + n < len(dxy) and tuple(dsite[p + n]) == here and dxy[p + n, 0] == x[i] and n < ef.NBINS:
                    n += 1
            assert p + n <= len(dxy), (k, i)
            for q in range(n):
                assert tuple(dsite[p + q]) == here, (k, i, q)
                assert dxy[p + q, 0] == x[i] and dxy[p + q, 1] == y[i] and dre[p + q] == rv[i, 3]
                # the fp32 output against the fp64 formula on the same offsets: exp2f within 2 ulp, two products
                assert abs(float(dsc[p + q]) - scale[i]) <= 4 * 2.0 ** -23 * scale[i]
                if n == len(found):
                    d = abs(float(dan[p + q]) - float(found[q][1]))
                    worst = max(worst, min(d, ef.TWO_PI - d))
            p += n
        assert p == len(dxy), (k, p, len(dxy))
        print(f"  orientation: largest angle difference {worst:.3g} (tolerance {val_tol['angle']:.3g})")
        assert worst <= val_tol["angle"]
        assert np.all((dan >= 0) & (dan < np.float32(ef.TWO_PI) + 1e-6))
        # 5. the descriptors from the device's final keypoints
        raw = ef.describe_raw(pyr, dsite[:, 0], dsite[:, 1], dxy[:, 0], dxy[:, 1], dsc, dan)
        diff = np.abs(out["desc"][kp].astype(np.int64) - ef.to_bytes(raw).astype(np.int64))
        assert diff.max(initial=0) <= 1
        near = np.abs(raw - (np.floor(raw) + 0.5))
        print(f"  descriptors: {int((diff != 0).sum())} of {diff.size} bytes differ, "
              f"farthest from a rounding point {near[diff != 0].max(initial=0.0):.3g}")
        assert np.all(near[diff != 0] <= 2e-3)


SHAPES = [(16, 16), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (33, 257), (257, 33)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_one_image_stage_by_stage(core, tol, H, W):
    img = ef.texture(H, W, 1000 * H + W)
    check_stages(run(core, ("one", H, W), [img]), [img], tol)


def test_fixture_images_stage_by_stage(core, tol):
    imgs = ef.fixture_images()
    for k, img in enumerate(imgs):
        check_stages(run(core, ("fixture", k), [img]), [img], tol)
    # the fp64 restatement of the whole chain is close: the same candidates where the pyramids agree on every comparison
    fx = ef.fixture()
    out = run(core, ("fixture", 0), [imgs[0]])
    assert abs(len(out["xy"]) - len(fx["img0_xy"])) <= max(2, len(fx["img0_xy"]) // 10)


def batch_images():
    return [ef.texture(TH + 1, TW + 1, s) for s in (41, 42, 43)]


def test_batch_of_three_equals_three_calls_and_two_calls_agree(core, tol):
    imgs = batch_images()
    out = run(core, ("batch",), imgs)
    check_stages(out, imgs, tol)
    again = core.extract_features(np.stack(imgs), want_diagnostics=True)
    for n, v in out.items():
        assert v.tobytes() == again[n].tobytes(), n
    for k, img in enumerate(imgs):
        one = core.extract_features(img[None], want_diagnostics=True)
        kp, cd = image_slices(out, k)
        for n in ("xy", "scale", "angle", "response", "desc", "kp_site"):
            assert one[n].tobytes() == out[n][kp].tobytes(), (k, n)
        assert np.array_equal(one["cand"][:, 1:], out["cand"][cd, 1:])
        assert one["pyramid"][0].tobytes() == out["pyramid"][k].tobytes()
        for n in ("ref_ok", "ref_site", "ref_val"):
            assert one[n].tobytes() == out[n][cd].tobytes(), (k, n)


def test_cap_keeps_the_largest_responses_in_key_order(core):
    imgs = ef.fixture_images()[:2]  # 97 x 130 and 130 x 97: one call each
    for img in imgs:
        full = core.extract_features(img[None])
        n = len(full["xy"])
        m = n // 2
        assert m >= 5
        capped = core.extract_features(img[None], max_keypoints=m)
        order = np.lexsort((np.arange(n), -full["response"].astype(np.float64)))
        keep = np.sort(order[:m])
        assert capped["kp_start"].tolist() == [0, m]
        for name in ("xy", "scale", "angle", "response", "desc"):
            assert capped[name].tobytes() == full[name][keep].tobytes(), name
        # a cap above the count changes nothing
        loose = core.extract_features(img[None], max_keypoints=n + 3)
        assert all(loose[name].tobytes() == full[name].tobytes() for name in full)


def test_capacity_too_small_is_an_error_and_nothing_is_written_out_of_bounds(core):
    img = ef.fixture_images()[0]
    n = len(core.extract_features(img[None])["xy"])
    cap, guard = n - 1, 16
    outs = dict(kp_start=np.full(2 + guard, -7, np.int64), xy=np.full((cap + guard, 2), -7.0),
                scale=np.full(cap + guard, -7, np.float32), angle=np.full(cap + guard, -7, np.float32),
                response=np.full(cap + guard, -7, np.float32), desc=np.full((cap + guard, 128), 249, np.uint8))
    P = core._p
    rc = core._lib.sfm_extract_features(P(np.ascontiguousarray(img), core._u8), 1, img.shape[0], img.shape[1], 0, 0, 0.04,
                                        10.0, 1.6, cap, P(outs["kp_start"], core._i64), P(outs["xy"]),
                                        P(outs["scale"], core._f32), P(outs["angle"], core._f32),
                                        P(outs["response"], core._f32), P(outs["desc"], core._u8), None, None, 0, None,
                                        None, None, None, None, core.DEVICE)
    assert rc == -6 and b"capacity" in core._lib.sfm_last_error()  # SFM_ERR_CAPACITY
    assert (outs["kp_start"][2:] == -7).all()
    for name in ("xy", "scale", "angle", "response"):
        assert (outs[name][cap:] == -7).all(), name
    assert (outs["desc"][cap:] == 249).all()
    with pytest.raises(core.SfmCoreError):
        core.extract_features(img[None], capacity=cap)
    from sfm_io import extract_features
    with pytest.raises(core.SfmCoreError):
        extract_features([img], capacity=cap)
    assert len(extract_features([img], capacity=n)[0][0]) == n


def test_through_the_public_chain(core):
    from sfm_io import extract_features, match_descriptors
    from sfm_multiview import verify_pairs
    a, b = ef.chain_crops()
    kps, descs, scale, angle, response = extract_features([a, b])
    assert all(k.dtype == np.float64 and k.shape == (len(d), 2) and d.dtype == np.uint8 and d.shape[1] == 128
               for k, d in zip(kps, descs))
    assert all(len(s) == len(k) == len(t) == len(r) for s, t, r, k in zip(scale, angle, response, kps))
    store, pair_ij, ms, ma, mb, dsq = match_descriptors(kps, descs, ratio=0.8, cross_check=True)
    d = kps[1][mb] - kps[0][ma]
    print("chain: keypoints", len(kps[0]), len(kps[1]), "matches", len(ma))
    assert np.abs(d - np.array(ef.CHAIN_SHIFT, dtype=np.float64)).max() <= 1.0
    want = int(ef.fixture()["chain_matches"])
    assert want >= 30 and 2 * len(ma) >= want
    merged, row_track, obs_map = store.merge_tracks()
    # several orientations of one location share a keypoint, so their matches merge into one track or conflict
    assert 0 < merged.n_features <= len(ma) and len(row_track) == len(ma)
    for st in (store, merged):
        order, vp_ij, vout, index1, index2 = verify_pairs(st, H=64, seed=0)
        assert vp_ij.tolist() == [[0, 1]] and len(index1) == len(index2) == st.n_features
        assert vout[0].shape == (1, 3, 3) and len(vout[3]) == st.n_features
