"""Batched pair verification on a real MI355X (sfm_verify_pairs) against numpy
at its own hypotheses, against tests/golden/verify_pairs.npz and against itself
alone, permuted and with one hypothesis more.

The scene, the sample tables and the rule in numpy come from
tests/test_verify_pairs.py; the fixture's generator asserts the margins (every
final Sampson distance half a pixel from the threshold) and the conditioning
that make the masks exact and the refitted F comparable.

Measured on the MI355X (pair verification): sigma_3 / sigma_1 of a
returned model at most 1.12e-16, the sample residual over the restatement's at
most 1.43e-14 sigma_1, |F - F_gold|_F at most 8.14e-15, the noise-free pairs'
|F - F_true|_F at most 8.81e-15.
"""
import os

import numpy as np
import pytest

import test_verify_pairs as vp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
THR = vp.THRESHOLD


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "verify_pairs.npz"))


@pytest.fixture(scope="module")
def scene():
    return vp.load_scene()


def run(core, sc, samples, pairs=None, **kw):
    """the call on the whole scene, or on ``pairs`` of it in that order"""
    if pairs is None:
        ps, x1, x2 = sc["pair_start"], sc["x1"], sc["x2"]
    else:
        sel = np.concatenate([np.arange(sc["pair_start"][p], sc["pair_start"][p + 1]) for p in pairs])
        ps = np.concatenate([[0], np.cumsum(sc["n_p"][list(pairs)])])
        x1, x2, samples = sc["x1"][sel], sc["x2"][sel], samples[list(pairs)]
    return core.verify_pairs(ps, x1, x2, samples, threshold=THR, want_counts=True, want_models=True, **kw)


@pytest.fixture(scope="module")
def results(core, scene):
    """H -> the call's outputs on the whole scene, computed once"""
    return {H: run(core, scene, vp.sample_table(H)) for H in vp.HS}


def per_pair(out, sc, p, pairs=None):
    """pair p's part of every output (p: position in the call)"""
    n_p = sc["n_p"] if pairs is None else sc["n_p"][list(pairs)]
    ps = np.concatenate([[0], np.cumsum(n_p)])
    F, cost, n_inl, inl, hyp, count, info, counts, models = out
    return (F[p], cost[p], n_inl[p], inl[ps[p]:ps[p + 1]], hyp[p], count[p], info[p], counts[p], models[p])


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def counts_at(models, x1, x2, thr):
    """numpy's inlier count of every model (H, 3, 3) over the pair"""
    h1 = np.column_stack([x1, np.ones(len(x1))])
    h2 = np.column_stack([x2, np.ones(len(x2))])
    l = np.einsum("hij,nj->hni", models, h1)
    m = np.einsum("hji,nj->hni", models, h2)
    e = (h2[None] * l).sum(axis=2)
    den = l[..., 0] ** 2 + l[..., 1] ** 2 + m[..., 0] ** 2 + m[..., 1] ** 2
    with np.errstate(invalid="ignore"):
        return ((den > 0) & (e * e < thr * thr * den)).sum(axis=1)


def check_counts(x1, x2, counts, models, hyp, count):
    """numpy's count at the returned models brackets the device's; the winner is the first maximum"""
    finite = np.isfinite(models).all(axis=(1, 2))
    lo = np.where(finite, counts_at(np.nan_to_num(models), x1, x2, THR * (1 - 1e-9)), 0)
    hi = np.where(finite, counts_at(np.nan_to_num(models), x1, x2, THR * (1 + 1e-9)), 0)
    assert np.all(lo <= counts) and np.all(counts <= hi)
    assert counts.max() > 0 and hyp == int(np.argmax(counts)) and count == counts.max()


def test_counts_are_numpys_at_the_returned_models(scene, results):
    for H in vp.HS:
        for p in range(scene["P"]):
            x1, x2 = vp.pair(scene, p)
            F, cost, n_inl, inl, hyp, count, info, counts, models = per_pair(results[H], scene, p)
            if len(x1) < 8:
                assert not counts.any() and not models.any() and hyp == -1
                continue
            assert counts.shape == (H,) and models.shape == (H, 3, 3)
            check_counts(x1, x2, counts, models, hyp, count)


def test_fit_is_the_null_vector_of_its_sample_in_unit_norm_and_rank_two(scene, results):
    weak = total = 0
    worst_rank = worst_res = worst_norm = 0.0
    for H in vp.HS:
        tab = vp.sample_table(H)
        for p in range(scene["P"]):
            x1, x2 = vp.pair(scene, p)
            if len(x1) < 8:
                continue
            models = per_pair(results[H], scene, p)[8]
            for s, F in zip(tab[p], models):
                A, T1, T2 = vp.design(x1[s], x2[s])
                sv = np.linalg.svd(A, compute_uv=False)
                total += 1
                if sv[7] < 1e-6 * sv[0]:
                    weak += 1
                    continue
                g = F.reshape(-1)
                worst_norm = max(worst_norm, abs(np.linalg.norm(g) - 1.0))
                # nine quotients rounded once each, and numpy's own sum of nine squares
                assert abs(np.linalg.norm(g) - 1.0) <= 4e-16 * 9
                assert g[np.argmax(np.abs(g))] > 0
                s3 = np.linalg.svd(F, compute_uv=False)
                worst_rank = max(worst_rank, s3[2] / s3[0])
                assert s3[2] <= 1e-12 * s3[0]

                def residual(G):
                    f = np.linalg.inv(T2).T @ G @ np.linalg.inv(T1)
                    return np.linalg.norm(A @ (f / np.linalg.norm(f)).reshape(-1))
                excess = residual(F) - residual(vp.fit(x1[s], x2[s]))
                worst_res = max(worst_res, excess / sv[0])
                assert excess <= 1e-9 * sv[0]
    print(f"hypotheses under sigma_8 / sigma_1 = 1e-6: {weak} of {total}; | |F| - 1 | <= {worst_norm:.3g}, "
          f"sigma_3 / sigma_1 <= {worst_rank:.3g}, residual over the restatement's <= {worst_res:.3g} sigma_1")
    assert weak <= 0.05 * total


def test_result_is_the_truth_and_the_fixtures_fit(scene, results, gold):
    worst_F = worst_cost = 0.0
    for H in (65, 256):
        for p in scene["checked"]:
            x1, x2 = vp.pair(scene, p)
            s, e = scene["pair_start"][p], scene["pair_start"][p + 1]
            truth = scene["truth"][s:e]
            F, cost, n_inl, inl, hyp, count, info, counts, models = per_pair(results[H], scene, p)
            assert info in (1, 2)
            assert np.array_equal(inl, truth) and n_inl == truth.sum()
            assert n_inl >= count
            ref = vp.cost_of(F, x1, x2, truth)
            # the noise-free pair's cost is rounding alone (1e-25 px^2): nothing relative holds of it
            if ref > 1e-20:
                worst_cost = max(worst_cost, abs(cost - ref) / ref)
            assert np.isclose(cost, ref, rtol=1e-12, atol=0 if ref > 1e-20 else 1e-20)
            G = gold[f"F_H{H}"][p]
            d = np.linalg.norm(vp.align(F, G) - G)
            worst_F = max(worst_F, d)
            assert d <= 1e-9
    print(f"|F - F_gold|_F <= {worst_F:.3g}, cost relative to numpy's <= {worst_cost:.3g}")


def test_small_pairs(scene, results):
    worst = 0.0
    for H in vp.HS:
        F, cost, n_inl, inl, hyp, count, info, counts, models = per_pair(results[H], scene, 0)   # 7
        assert info == -1 and not F.any() and not inl.any() and n_inl == 0 and hyp == -1 and count == 0
        for p in (1, 2):                                                                       # 8 and 9, noise-free
            F, cost, n_inl, inl, hyp, count, info, counts, models = per_pair(results[H], scene, p)
            assert info >= 0 and inl.all() and n_inl == len(inl) == scene["n_p"][p]
            Ft = scene["F_true"][p]
            d = np.linalg.norm(vp.align(F, Ft) - Ft)
            worst = max(worst, d)
            assert abs(np.linalg.norm(F) - 1.0) <= 4e-15 and d <= 1e-8
    print(f"noise-free pairs: |F - F_true|_F <= {worst:.3g}")


def test_a_pair_alone_and_all_pairs_permuted_give_the_same_bits(core, scene, results):
    H = 65
    tab = vp.sample_table(H)
    whole = results[H]
    for p in (2, 9, 11):
        alone = run(core, scene, tab, pairs=[p])
        assert same(per_pair(alone, scene, 0, [p]), per_pair(whole, scene, p))
    perm = list(np.random.default_rng(3).permutation(scene["P"]))
    out = run(core, scene, tab, pairs=perm)
    for k, p in enumerate(perm):
        assert same(per_pair(out, scene, k, perm), per_pair(whole, scene, p))


def test_an_appended_hypothesis_that_cannot_win_changes_nothing(core, scene, results):
    tab = vp.sample_table(64)
    # hypothesis 0 again, at the end: it ties with the first at best, and the earliest wins
    more = run(core, scene, np.concatenate([tab, tab[:, :1]], axis=1))
    for p in range(scene["P"]):
        a, b = per_pair(more, scene, p), per_pair(results[64], scene, p)
        assert same(a[:7], b[:7])
        assert np.array_equal(a[7][:64], b[7]) and np.array_equal(a[8][:64], b[8], equal_nan=True)
        assert a[7][64] == a[7][0] and np.array_equal(a[8][64], a[8][0], equal_nan=True)


def test_min_inliers_above_the_winner_returns_the_winning_hypothesis(core, scene, results):
    H = 65
    out = run(core, scene, vp.sample_table(H), min_inliers=2000)
    for p in range(1, scene["P"]):
        x1, x2 = vp.pair(scene, p)
        F, cost, n_inl, inl, hyp, count, info, counts, models = per_pair(out, scene, p)
        w = per_pair(results[H], scene, p)
        assert info == -3 and hyp == w[4] and count == w[5]
        assert np.array_equal(F, models[hyp]) and np.array_equal(counts, w[7])
        assert n_inl == count == inl.sum()
        lo, hi = vp.inlier_mask(F, x1, x2, THR * (1 - 1e-9)), vp.inlier_mask(F, x1, x2, THR * (1 + 1e-9))
        assert np.all(lo <= inl) and np.all(inl <= hi)
        assert np.isclose(cost, vp.cost_of(F, x1, x2, inl), rtol=1e-12, atol=1e-20)


def test_refit_rounds_zero_returns_the_winner_with_info_zero(core, scene, results):
    H = 65
    out = run(core, scene, vp.sample_table(H), refit_rounds=0)
    for p in range(1, scene["P"]):
        F, cost, n_inl, inl, hyp, count, info, counts, models = per_pair(out, scene, p)
        assert info == 0 and np.array_equal(F, models[hyp]) and n_inl == count


def test_store_round_trip_into_two_view_init(core, gold):
    import sfm_multiview as mv
    from sfm_two_view import two_view_init
    sc = vp.store_scene()
    st = sc["store"]
    st.flag[:] = 0
    order, pair_ij, out, i1, i2 = mv.verify_pairs(st, H=256, seed=0, threshold=THR, update_flags=True)
    F, cost, n_inl, inl, hyp, count, info = out
    ps = st.pairs()[1]
    assert len(pair_ij) == 6 and np.all(info >= 0)
    # the flags: exactly the observations of inlier correspondences
    expect = np.zeros(len(st), dtype=np.uint8)
    expect[i1[inl]] = 1
    expect[i2[inl]] = 1
    assert np.array_equal(st.flag, expect) and 0 < expect.sum() < len(st)
    assert np.array_equal(order, np.argsort(-n_inl.astype(np.int64), kind="stable"))
    assert np.all(np.diff(n_inl[order]) <= 0)
    # the wrong matches against image 0 are the outliers of their pairs
    for p, (a, c) in enumerate(pair_ij):
        if a == 0:
            feat = st.feature[i1[ps[p]:ps[p + 1]]]
            assert np.array_equal(inl[ps[p]:ps[p + 1]], ~sc["wrong"][feat, c])
    b = int(order[0])
    assert tuple(pair_ij[b]) == tuple(gold["store_best_pair"])
    m = inl[ps[b]:ps[b + 1]]
    x1 = np.column_stack([st.x[i1], st.y[i1]])[ps[b]:ps[b + 1]][m]
    x2 = np.column_stack([st.x[i2], st.y[i2]])[ps[b]:ps[b + 1]][m]
    C, R, X, cnt, best = two_view_init(F[b], vp.K, x1, x2)
    Rt, Ct = vp.relative_pose(sc, *pair_ij[b])
    e_rot, e_dir = vp.rot_angle(R, Rt), vp.direction_angle(C, Ct)
    print(f"best pair {tuple(pair_ij[b])}: {n_inl[b]} inliers, rotation error {e_rot:.3g} rad, direction error "
          f"{e_dir:.3g} rad (restatement: {gold['store_errors'][0]:.3g}, {gold['store_errors'][1]:.3g})")
    assert e_rot <= 0.02 and e_dir <= 0.05
    st.flag[:] = 0


def test_p3data_counts_are_numpys(core):
    from sfm_io import read_matching
    st = read_matching(os.path.join(GOLDEN, "P3Data"), 5)
    pair_ij, ps, i1, i2 = st.pairs()
    x1 = np.column_stack([st.x[i1], st.y[i1]])
    x2 = np.column_stack([st.x[i2], st.y[i2]])
    samples = core.pair_samples(np.diff(ps), 256, 0)
    F, cost, n_inl, inl, hyp, count, info, counts, models = core.verify_pairs(
        ps, x1, x2, samples, threshold=THR, want_counts=True, want_models=True)
    assert len(pair_ij) > 0
    for p in range(len(pair_ij)):
        s, e = ps[p], ps[p + 1]
        check_counts(x1[s:e], x2[s:e], counts[p], models[p], hyp[p], count[p])
        assert n_inl[p] >= count[p] and inl[s:e].sum() == n_inl[p]
        print(f"P3Data pair {tuple(pair_ij[p] + 1)}: {n_inl[p]} inliers of {e - s} matches "
              f"(best hypothesis {count[p]}, info {info[p]})")


# ------------------------------------------------- the batch recorded before the stages shared a driver
# tests/golden/pair_stages_parent.npz (make_golden_pair_stages.py): every output of sfm_verify_pairs ("F") and
# sfm_essential_pairs ("E") on one batch, as the commit before pair_verify.hpp returned them.
STAGE_SIZES = (0, 8, 5, 9, 40, 4, 1025, 120, 300, 7)   # dead pairs first, in the middle and last
STAGE_H = 65
STAGE_CALLS = {"main": {}, "h1": {"H": 1}, "tight": {"threshold": 1e-9}, "none": {"threshold": 1e-170},
               "high": {"min_inliers": 100000}, "rounds0": {"refit_rounds": 0}}
STAGE_NAMES = {"F": ("F", "cost", "n_inliers", "inlier", "best_hyp", "best_count", "info", "counts", "models"),
               "E": ("F", "cost", "n_inliers", "inlier", "best_hyp", "best_count", "info", "E", "n_sol", "counts",
                     "models")}


def stages_batch(seed):
    """cfg2's two cameras: pairs of nine and more with 1 px noise and 30 % of their matches wrong"""
    made = [vp.make_pair([seed, p], n, 1.0 if n >= 9 else 0.2, 0.3 if n >= 9 else 0.0)
            for p, n in enumerate(STAGE_SIZES)]
    ps = np.concatenate([[0], np.cumsum(STAGE_SIZES)]).astype(np.int64)
    return ps, np.concatenate([m[0] for m in made]), np.concatenate([m[1] for m in made])


def stages_run(core, stage, seed, calls=STAGE_CALLS):
    """{"<stage>_<call>_<output>": array} over ``calls``"""
    ps, x1, x2 = stages_batch(seed)
    out = {}
    for call, kw in calls.items():
        kw = dict(kw)
        H = kw.pop("H", STAGE_H)
        if stage == "F":
            got = core.verify_pairs(ps, x1, x2, core.pair_samples(np.diff(ps), H, seed), want_counts=True,
                                    want_models=True, **kw)
        else:
            got = core.essential_pairs(vp.K, ps, x1, x2, core.essential_samples(np.diff(ps), H, seed),
                                       want_counts=True, want_models=True, **kw)
        out.update({f"{stage}_{call}_{name}": a for name, a in zip(STAGE_NAMES[stage], got)})
    return out


def check_stages_keep_their_bits(core, stage):
    gold = np.load(os.path.join(GOLDEN, "pair_stages_parent.npz"))
    got = stages_run(core, stage, int(gold["seed"]))
    assert len(got) == len(STAGE_CALLS) * len(STAGE_NAMES[stage])
    for key, a in got.items():
        # an array equal to the main call's is stored once
        ref = gold[key if key in gold.files else f"{stage}_main_" + key.split("_", 2)[2]]
        assert a.dtype == ref.dtype and np.array_equal(a, ref), key


def test_every_output_keeps_the_bits_recorded_before_the_shared_driver(core):
    check_stages_keep_their_bits(core, "F")
