"""Track merging on a real MI355X (sfm_merge_tracks, sfm_io.merge_tracks)
against the plain-Python restatement of tests/test_merge_tracks.py and
tests/golden/merge_tracks.npz.  Integer work with an exact answer: every output
is compared for equality, dtype included; there are no tolerances.
"""
import numpy as np
import pytest

import test_merge_tracks as mt

pytestmark = pytest.mark.gpu
POLICIES = ((mt.DROP, "drop"), (mt.KEEP_ROWS, "keep_rows"))


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


def make_store(rs, im, x, y, n_images):
    from sfm_io import MatchStore
    n_rows = len(rs) - 1
    return MatchStore(n_rows, n_images, np.repeat(np.arange(n_rows, dtype=np.int32), np.diff(rs)), im, x, y)


def same(out, ref, names=mt.OUTPUTS):
    for n in names:
        assert out[n].dtype == ref[n].dtype and out[n].shape == ref[n].shape and np.array_equal(out[n], ref[n]), n


def check_call(core, rs, im, x, y, n_images, policy):
    """the device call against the restatement; returns both"""
    out = core.merge_tracks(rs, im, x, y, n_images, policy)
    ref = mt.restate(rs, im, x, y, policy)
    same(out, ref)
    return out, ref


def check_store(st, conflicts, ref, flag=None):
    """sfm_io.merge_tracks on a store against merged_arrays of the restatement, the two maps against the arrays,
    the store untouched; returns (merged, row_track, obs_map)"""
    from sfm_io import merge_tracks
    if flag is not None:
        st.flag[:] = flag
    before = [a.copy() for a in (st.feature, st.image, st.x, st.y, st.flag, st._row_start)]
    merged, row_track, obs_map = merge_tracks(st, conflicts)
    for a, b in zip(before, (st.feature, st.image, st.x, st.y, st.flag, st._row_start)):
        assert np.array_equal(a, b)
    want = mt.merged_arrays(ref, st.image, st.x, st.y, st.flag)
    assert merged.n_features == len(ref["track_label"]) and merged.n_images == st.n_images
    for n in ("feature", "image", "x", "y", "flag"):
        assert np.array_equal(getattr(merged, n), want[n]), n
    assert np.array_equal(row_track, want["row_track"]) and np.array_equal(obs_map, want["obs_map"])
    assert np.array_equal(merged._row_start, ref["track_start"])
    # feature-major with images ascending
    assert np.all(np.diff(merged.feature) >= 0)
    assert np.all((np.diff(merged.image) >= 0) | (np.diff(merged.feature) > 0))
    # the maps against the arrays
    kept = obs_map >= 0
    assert np.array_equal(kept, row_track[st.feature] >= 0)
    assert np.array_equal(merged.feature[obs_map[kept]], row_track[st.feature[kept]])
    assert np.array_equal(merged.image[obs_map[kept]], st.image[kept])
    assert np.all(merged.x[obs_map[kept]] == st.x[kept]) and np.all(merged.y[obs_map[kept]] == st.y[kept])
    assert len(np.unique(obs_map[kept])) == len(merged)  # every merged observation is some observation's
    return merged, row_track, obs_map


# ------------------------------------------------------------------ 1. P3Data
@pytest.mark.parametrize("scene", ["", "_untruncated"])
@pytest.mark.parametrize("policy,conflicts", POLICIES)
def test_p3data_against_the_fixture(core, scene, policy, conflicts):
    st = mt.p3data() if scene == "" else mt.p3data_untruncated()
    fx = mt.fixture()
    tag = "drop" if policy == mt.DROP else "keep"
    ref = {n: fx[mt.fixture_key(n, tag, scene)] for n in mt.OUTPUTS}
    same(core.merge_tracks(st._row_start, st.image, st.x, st.y, st.n_images, policy), ref)
    flag = np.random.default_rng(5).integers(0, 4, len(st)).astype(np.uint8)
    merged, row_track, _ = check_store(st, conflicts, ref, flag)
    assert set(np.unique(merged.flag)) == {0, 1, 2, 3}
    m2, r2, o2 = st.merge_tracks(conflicts)  # the method is the function
    assert np.array_equal(m2.x, merged.x) and np.array_equal(r2, row_track)
    figures = mt.FIGURES if scene == "" else mt.FIGURES_UNTRUNCATED
    n_clean = figures["components"] - figures["conflicting"]
    if policy == mt.DROP:
        assert merged.n_features == n_clean
        assert np.bincount(np.diff(merged._row_start), minlength=6)[2:6].tolist() == figures["consistent_by_views"]


# ------------------------------------------------------------------ 2. chain
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_chain_is_one_component(core, order):
    n = 4096
    rng = np.random.default_rng(11)
    px, py = rng.uniform(0, 1000, n + 1), rng.uniform(0, 1000, n + 1)
    ks = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": rng.permutation(n)}[order]
    rows = [[(int(k), px[k], py[k]), (int(k) + 1, px[k + 1], py[k + 1])] for k in ks]  # keypoint k lies in image k
    rs, im, x, y = mt.rows_of(rows)
    out, _ = check_call(core, rs, im, x, y, n + 1, mt.DROP)
    assert np.all(out["component"] == 0) and not out["conflict"].any()
    assert len(out["track_label"]) == 1 and out["track_start"].tolist() == [0, n + 1]
    assert np.array_equal(im[out["track_obs"]], np.arange(n + 1))


# ------------------------------------------------------------------ 3. star
@pytest.mark.parametrize("clean", [False, True])
def test_star_contends_for_one_slot_and_one_root(core, clean):
    n = 10000
    rows = [[(0, 5.0, 5.0), (1 + j if clean else 1, float(j), 0.5 * j)] for j in range(n)]
    rs, im, x, y = mt.rows_of(rows)
    out, _ = check_call(core, rs, im, x, y, n + 1 if clean else 2, mt.DROP)
    assert np.all(out["component"] == 0) and np.all(out["keypoint"][0::2] == 0)
    assert out["conflict"].all() != clean
    assert len(out["track_label"]) == (1 if clean else 0)
    if clean:
        assert out["track_start"].tolist() == [0, n + 1]
    check_call(core, rs, im, x, y, n + 1 if clean else 2, mt.KEEP_ROWS)


# ------------------------------------------------------------------ 4. near-equal keys
def test_near_equal_keys_stay_apart(core):
    rng = np.random.default_rng(2)
    m = 13000
    bx, by = rng.uniform(1, 1000, m), rng.uniform(1, 1000, m)
    assert len(np.unique(np.column_stack([bx, by]), axis=0)) == m
    keys = ([(0, bx[k], by[k]) for k in range(m)] + [(0, bx[k], np.nextafter(by[k], np.inf)) for k in range(m)]
            + [(1, bx[k], by[k]) for k in range(m)] + [(0, -bx[k], by[k]) for k in range(m)] + [(0, 0.0, 7.0)])
    assert len(keys) == 4 * m + 1 >= 50000
    again = keys[:-1] + [(0, -0.0, 7.0)]  # every key a second time, the zero with the other sign
    obs = keys + again
    order = rng.permutation(len(obs))
    rows = [[obs[order[2 * r]], obs[order[2 * r + 1]]] for r in range(len(obs) // 2)]
    rs, im, x, y = mt.rows_of(rows)
    for policy, _ in POLICIES:
        out, _ = check_call(core, rs, im, x, y, 2, policy)
    kp = out["keypoint"]
    assert len(np.unique(kp)) == len(keys)  # no two of the near-equal keys share a keypoint
    assert np.array_equal(np.bincount(kp, minlength=len(kp))[np.unique(kp)], np.full(len(keys), 2))
    place = np.empty(len(obs), dtype=np.int64)
    place[order] = np.arange(len(obs))  # where each entry of `obs` went
    z0, z1 = place[len(keys) - 1], place[len(obs) - 1]
    assert kp[z0] == kp[z1] == min(z0, z1)  # 0.0 and -0.0 are one keypoint
    assert np.signbit(x[z1]) and not np.signbit(x[z0])
    for k in (0, 1, m - 1):  # the four variants of one base point are four keypoints
        assert len({int(kp[place[k + j * m]]) for j in range(4)}) == 4


# ------------------------------------------------------------------ 5. conflicts
CONFLICT_ROWS = [
    [(0, 1.0, 1.0), (1, 2.0, 2.0)], [(0, 1.0, 1.0), (1, 3.0, 3.0)],                  # a direct conflict in image 1
    [(0, 10.0, 1.0), (1, 11.0, 1.0)], [(1, 11.0, 1.0), (2, 12.0, 1.0)], [(0, 13.0, 1.0), (2, 12.0, 1.0)],  # across three rows
    [(0, 20.0, 1.0), (0, 21.0, 1.0), (1, 22.0, 1.0)],                                # conflicting on its own
    [(0, 30.0, 1.0), (1, 31.0, 1.0)], [(1, 31.0, 1.0), (2, 32.0, 1.0)],              # a clean neighbour
]


@pytest.mark.parametrize("policy,conflicts", POLICIES)
def test_conflicts(core, policy, conflicts):
    rs, im, x, y = mt.rows_of(CONFLICT_ROWS)
    out, ref = check_call(core, rs, im, x, y, 3, policy)
    assert out["component"].tolist() == [0, 0, 2, 2, 2, 5, 6, 6]
    assert out["conflict"].tolist() == [True] * 6 + [False] * 2
    st = make_store(rs, im, x, y, 3)
    merged, row_track, obs_map = check_store(st, conflicts, ref, np.arange(len(st), dtype=np.uint8) % 2)
    clean = row_track[6]
    assert row_track[7] == clean >= 0  # the neighbour is one track of three views under both policies
    s, e = merged._row_start[clean], merged._row_start[clean + 1]
    assert merged.image[s:e].tolist() == [0, 1, 2] and merged.x[s:e].tolist() == [30.0, 31.0, 32.0]
    if policy == mt.DROP:
        assert out["label"].tolist() == [-1] * 6 + [6, 6] and np.all(obs_map[:rs[6]] == -1)
        assert merged.n_features == 1
    else:
        assert out["label"].tolist() == [0, 1, 2, 3, 4, 5, 6, 6] and merged.n_features == 7
        for r in range(6):  # the conflicting rows come back exactly as they went in
            t = row_track[r]
            assert t == r
            for name in ("image", "x", "y", "flag"):
                got = getattr(merged, name)[merged._row_start[t]:merged._row_start[t + 1]]
                assert np.array_equal(got, getattr(st, name)[rs[r]:rs[r + 1]]), (r, name)
            assert np.array_equal(obs_map[rs[r]:rs[r + 1]], np.arange(merged._row_start[t], merged._row_start[t + 1]))


# ------------------------------------------------------------------ 6. edges
def test_edges(core):
    for policy, conflicts in POLICIES:
        # one row
        rs, im, x, y = mt.rows_of([[(0, 1.0, 2.0), (2, 3.0, 4.0)]])
        check_call(core, rs, im, x, y, 3, policy)
        # empty rows and rows of one observation, some of them the same keypoint
        rows = [[], [(1, 5.0, 5.0)], [], [(1, 5.0, 5.0)], [(0, 1.0, 1.0), (1, 6.0, 6.0)], [(2, 9.0, 9.0)], []]
        rs, im, x, y = mt.rows_of(rows)
        out, ref = check_call(core, rs, im, x, y, 3, policy)
        assert out["component"].tolist() == [0, 1, 2, 1, 4, 5, 6] and out["track_start"].tolist() == [0, 0, 1, 1, 3, 4, 4]
        check_store(make_store(rs, im, x, y, 3), conflicts, ref)
        # no observations at all
        rs, im, x, y = mt.rows_of([[], [], []])
        out, ref = check_call(core, rs, im, x, y, 3, policy)
        merged, row_track, obs_map = check_store(make_store(rs, im, x, y, 3), conflicts, ref)
        assert merged.n_features == 3 and len(merged) == 0 and len(obs_map) == 0
        # nothing shared: the merged store is the input
        rng = np.random.default_rng(4)
        rows = [[(int(i), float(rng.uniform(0, 100)), float(1000 * r + i)) for i in np.sort(rng.permutation(7)[:n])]
                for r, n in enumerate(rng.integers(2, 6, 700))]
        rs, im, x, y = mt.rows_of(rows)
        out, ref = check_call(core, rs, im, x, y, 7, policy)
        st = make_store(rs, im, x, y, 7)
        merged, row_track, obs_map = check_store(st, conflicts, ref, rng.integers(0, 2, len(st)).astype(np.uint8))
        for n in ("feature", "image", "x", "y", "flag", "_row_start"):
            assert np.array_equal(getattr(merged, n), getattr(st, n)), n
        assert np.array_equal(row_track, np.arange(700)) and np.array_equal(obs_map, np.arange(len(st)))
    # each SFM_ERR_ARG case leaves its outputs untouched, also once the device is in use
    mt.test_arguments_are_refused_before_a_device_is_looked_for()


# ------------------------------------------------------------------ 7. random
def random_scene(seed=7, n_rows=20000, n_images=8):
    """rows cut from scene points of one keypoint per image: about 50,000 observations whose keypoints come from a
    pool a third that size; 2 % of the rows take one keypoint of another point"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(2, 4, n_rows)  # 2 or 3 observations: 2.5 on average
    n_points = int(lengths.sum()) // 3 // 5  # five keypoints a point: the pool is n_obs / 3
    vis = np.array([np.sort(rng.permutation(n_images)[:5]) for _ in range(n_points)])
    px, py = rng.uniform(0, 2000, (n_points, n_images)), rng.uniform(0, 2000, (n_points, n_images))
    point = np.minimum((n_points * rng.random(n_rows) ** 3).astype(np.int64), n_points - 1)  # skewed: some points once
    rows = []
    for r in range(n_rows):
        p = point[r]
        imgs = np.sort(rng.permutation(vis[p])[:lengths[r]])
        row = [(int(i), px[p, i], py[p, i]) for i in imgs]
        if rng.random() < 0.02:
            q = int(rng.integers(n_points))
            i = int(vis[q][0])
            row[0] = (i, px[q, i], py[q, i])
            row.sort(key=lambda o: o[0])
        rows.append(row)
    return rows, n_images


def partition(out, rs):
    """track of every observation, -1 for none"""
    slot = out["obs_slot"]
    return np.where(slot >= 0, np.searchsorted(out["track_start"], slot, side="right") - 1, -1)


def test_random_rows(core):
    rows, n_images = random_scene()
    rs, im, x, y = mt.rows_of(rows)
    assert 45000 <= len(im) <= 55000
    out, ref = check_call(core, rs, im, x, y, n_images, mt.DROP)
    assert len(np.unique(out["keypoint"])) <= 0.4 * len(im)
    comps, size = np.unique(out["component"], return_counts=True)
    bad = np.zeros(len(rs) - 1, dtype=bool)
    bad[out["component"][out["conflict"]]] = True
    assert np.sum(size == 1) > 100 and np.sum((size > 1) & ~bad[comps]) > 100 and np.sum(bad[comps]) > 100
    for policy, conflicts in POLICIES:
        first = core.merge_tracks(rs, im, x, y, n_images, policy)
        second = core.merge_tracks(rs, im, x, y, n_images, policy)
        same(first, second)  # bit-identical from run to run
        same(first, mt.restate(rs, im, x, y, policy) if policy != mt.DROP else ref)
        # rows shuffled: the same partition of the observations into tracks
        order = np.random.default_rng(1).permutation(len(rows))
        rs2, im2, x2, y2 = mt.rows_of([rows[r] for r in order])
        shuffled = core.merge_tracks(rs2, im2, x2, y2, n_images, policy)
        back = np.concatenate([np.arange(rs2[k], rs2[k + 1]) for k in np.argsort(order)])  # old observation -> new
        assert np.array_equal(im2[back], im) and np.array_equal(x2[back], x)
        t1, t2 = partition(first, rs), partition(shuffled, rs2)[back]
        assert np.array_equal(t1 < 0, t2 < 0)
        pairs = np.unique(np.column_stack([t1, t2]), axis=0)
        assert len(pairs) == len(np.unique(t1)) == len(np.unique(t2))
        if policy == mt.KEEP_ROWS:
            check_store(make_store(rs, im, x, y, n_images), conflicts, first,
                        np.random.default_rng(3).integers(0, 2, len(im)).astype(np.uint8))


# ------------------------------------------------------------------ 8. round trip
def test_round_trip_from_ground_truth_tracks(core):
    rng = np.random.default_rng(9)
    G, n_images = 3000, 6
    vis = [np.sort(rng.permutation(n_images)[:rng.integers(2, n_images + 1)]) for _ in range(G)]
    px, py = rng.uniform(0, 3000, (G, n_images)), rng.uniform(0, 3000, (G, n_images))
    # a matcher's files: for every source image, a row per keypoint with its direct matches only -- the next one or
    # two images that see the point
    rows, track_of_row = [], []
    for s in range(n_images - 1):
        for g in range(G):
            later = vis[g][vis[g] > s]
            if s not in vis[g] or len(later) == 0:
                continue
            rows.append([(int(i), px[g, i], py[g, i]) for i in [s] + list(later[:rng.integers(1, 3)])])
            track_of_row.append(g)
    rs, im, x, y = mt.rows_of(rows)
    st = make_store(rs, im, x, y, n_images)
    assert len(st.tracks(np.arange(n_images), use_flags=False)[0]) == len(rows) > G  # the motivating fact
    # the store built from the ground truth, tracks in the order of their first row
    first_row = {}
    for r, g in enumerate(track_of_row):
        first_row.setdefault(g, r)
    truth = [[(int(i), px[g, i], py[g, i]) for i in vis[g]] for g in sorted(first_row, key=first_row.get)]
    assert len(truth) == G
    want = make_store(*mt.rows_of(truth), n_images)
    for policy, conflicts in POLICIES:
        out, ref = check_call(core, rs, im, x, y, n_images, policy)
        assert not out["conflict"].any()
        merged, row_track, _ = check_store(st, conflicts, ref)
        for n in ("n_features", "n_images"):
            assert getattr(merged, n) == getattr(want, n)
        for n in ("feature", "image", "x", "y", "_row_start"):
            assert np.array_equal(getattr(merged, n), getattr(want, n)), n
        order = {g: t for t, g in enumerate(sorted(first_row, key=first_row.get))}
        assert np.array_equal(row_track, [order[g] for g in track_of_row])
