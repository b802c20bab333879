"""Track merging (sfm_merge_tracks) restated in plain Python: a dictionary of
keypoint keys and a union-find over rows, written from the definitions in
include/sfmcore.h and not from the kernels.  Checked here against
tests/golden/merge_tracks.npz (P3Data through read_matching; generator:
tests/golden/make_golden_merge_tracks.py, which asserts the scene's figures);
tests/test_merge_tracks_gpu.py compares the device call with it for equality.
No GPU needed.
"""
import os
import re

import numpy as np

from conftest import GOLDEN, REPO

DROP, KEEP_ROWS = 0, 1
OUTPUTS = ("keypoint", "component", "conflict", "label", "track_label", "track_start", "track_obs", "obs_slot")
PER_POLICY = ("label", "track_label", "track_start", "track_obs", "obs_slot")


def restate(row_start, image, x, y, policy):
    """the outputs of sfm_merge_tracks as a dict of numpy arrays"""
    row_start = [int(v) for v in row_start]
    image = [int(v) for v in image]
    n_rows, n_obs = len(row_start) - 1, len(image)
    row = [r for r in range(n_rows) for _ in range(row_start[r], row_start[r + 1])]
    # keypoint: the smallest observation with the same image and coordinates (Python floats compare and hash
    # -0.0 as 0.0, and finite doubles are equal exactly when their bits are)
    first = {}
    keypoint = [first.setdefault((image[i], float(x[i]), float(y[i])), i) for i in range(n_obs)]
    # component: the smallest row of the set of rows joined through shared keypoints
    parent = list(range(n_rows))

    def find(r):
        while parent[r] != r:
            parent[r] = parent[parent[r]]
            r = parent[r]
        return r
    for i in range(n_obs):
        a, b = find(row[i]), find(row[keypoint[i]])
        if a != b:
            parent[a] = b
    smallest = {}
    for r in range(n_rows):
        smallest.setdefault(find(r), r)  # rows ascending: the first seen is the smallest
    component = [smallest[find(r)] for r in range(n_rows)]
    # conflicting: two different keypoints of one image
    kept, bad = {}, set()
    for i in range(n_obs):
        c = component[row[i]]
        if kept.setdefault((c, image[i]), keypoint[i]) != keypoint[i]:
            bad.add(c)
    conflict = [component[r] in bad for r in range(n_rows)]
    label = [component[r] if not conflict[r] else (-1 if policy == DROP else r) for r in range(n_rows)]
    # tracks: the distinct labels >= 0 ascending, each with its rows' distinct keypoints by (image, keypoint)
    members = {}
    for i in range(n_obs):
        if label[row[i]] >= 0:
            members.setdefault(label[row[i]], set()).add(keypoint[i])
    track_label = sorted({v for v in label if v >= 0})
    track_start, track_obs, place = [0], [], {}
    for v in track_label:
        for k in sorted(members.get(v, ()), key=lambda k: (image[k], k)):
            place[(v, k)] = len(track_obs)
            track_obs.append(k)
        track_start.append(len(track_obs))
    obs_slot = [place.get((label[row[i]], keypoint[i]), -1) for i in range(n_obs)]
    i32 = np.int32
    return dict(keypoint=np.array(keypoint, dtype=i32), component=np.array(component, dtype=i32),
                conflict=np.array(conflict, dtype=bool), label=np.array(label, dtype=i32),
                track_label=np.array(track_label, dtype=i32), track_start=np.array(track_start, dtype=np.int64),
                track_obs=np.array(track_obs, dtype=i32), obs_slot=np.array(obs_slot, dtype=i32))


def merged_arrays(ref, image, x, y, flag):
    """what sfm_io.merge_tracks builds from the outputs: the merged store's feature, image, x, y and flag, then
    row_track and obs_map"""
    n_tracks = len(ref["track_label"])
    feature = np.repeat(np.arange(n_tracks), np.diff(ref["track_start"]))
    mflag = np.zeros(len(ref["track_obs"]), dtype=np.uint8)
    for i, s in enumerate(ref["obs_slot"]):
        if s >= 0:
            mflag[s] |= flag[i]
    number = {int(v): t for t, v in enumerate(ref["track_label"])}
    row_track = np.array([number.get(int(v), -1) for v in ref["label"]], dtype=np.int64)
    k = ref["track_obs"]
    return dict(feature=feature, image=np.asarray(image)[k], x=np.asarray(x)[k], y=np.asarray(y)[k], flag=mflag,
                row_track=row_track, obs_map=ref["obs_slot"].astype(np.int64))


def rows_of(rows):
    """CSR arrays of a list of rows, each a list of (image, x, y)"""
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = [o for r in rows for o in r]
    image = np.array([o[0] for o in flat], dtype=np.int32)
    x = np.array([o[1] for o in flat], dtype=np.float64)
    y = np.array([o[2] for o in flat], dtype=np.float64)
    return row_start, image, x, y


def p3data():
    from sfm_io import read_matching
    return read_matching(os.path.join(GOLDEN, "P3Data"), 5)


def p3data_untruncated():
    """P3Data with every coordinate as the float the file holds.  read_matching keeps get_data's semantics: a
    line's own keypoint as floats, its matches' coordinates int()-truncated -- so a keypoint met as a match
    (49, 166) is rarely the keypoint met as its own line's source (49.0748, 166.783), and fewer rows join.  This
    parse shows what the files hold: (feature, image, x, y) in read_matching's order."""
    from sfm_io import MatchStore
    feature, image, x, y = [], [], [], []
    n_rows = 0
    for k in range(1, 5):
        with open(os.path.join(GOLDEN, "P3Data", f"matching{k}.txt")) as f:
            lines = f.read().split("\n")[1:]
        for line in lines:
            t = line.split()
            if not t:
                continue
            row = {k - 1: (float(t[4]), float(t[5]))}
            for j in range(int(t[0]) - 1):
                row[int(t[6 + 3 * j]) - 1] = (float(t[7 + 3 * j]), float(t[8 + 3 * j]))
            for im in sorted(row):
                feature.append(n_rows)
                image.append(im)
                x.append(row[im][0])
                y.append(row[im][1])
            n_rows += 1
    return MatchStore(n_rows, 5, np.array(feature, dtype=np.int32), np.array(image, dtype=np.int32), np.array(x),
                      np.array(y))


# the scene's figures (scene_figures) through read_matching and from the untruncated parse
FIGURES = dict(rows=3833, observations=9226, keypoints=6792, shared_keypoints=1532, components=2039,
               largest_component=27, conflicting=633, consistent_by_views=[1257, 133, 15, 1],
               rows_by_views=[2596, 955, 241, 41])
FIGURES_UNTRUNCATED = dict(rows=3833, observations=9226, keypoints=5562, shared_keypoints=2192, components=1739,
                           largest_component=29, conflicting=230, consistent_by_views=[931, 310, 178, 90],
                           rows_by_views=[2596, 955, 241, 41])


def fixture():
    return np.load(os.path.join(GOLDEN, "merge_tracks.npz"))


def scene_figures(st, ref):
    """the figures of DESIGN.md's table from the restatement (policy DROP) of a store"""
    kp, comp, conflict = ref["keypoint"], ref["component"], ref["conflict"]
    row = np.repeat(np.arange(st.n_features), np.diff(st._row_start))
    pairs = np.unique(np.column_stack([kp, row]), axis=0)  # (keypoint, row) once each
    rows_per_kp = np.bincount(pairs[:, 0], minlength=len(kp))
    comps, rows_per_comp = np.unique(comp, return_counts=True)
    views = np.diff(ref["track_start"])
    return dict(rows=st.n_features, observations=len(st), keypoints=int(np.sum(kp == np.arange(len(kp)))),
                shared_keypoints=int(np.sum(rows_per_kp > 1)), components=len(comps),
                largest_component=int(rows_per_comp.max()), conflicting=int(len(np.unique(comp[conflict]))),
                consistent_by_views=[int(np.sum(views == v)) for v in (2, 3, 4, 5)],
                rows_by_views=[int(np.sum(np.diff(st._row_start) == v)) for v in (2, 3, 4, 5)])


def fixture_key(name, tag, scene=""):
    return (f"{name}_{tag}" if name in PER_POLICY else name) + scene


def test_restatement_matches_the_fixture_on_p3data():
    fx = fixture()
    for st, scene in ((p3data(), ""), (p3data_untruncated(), "_untruncated")):
        for policy, tag in ((DROP, "drop"), (KEEP_ROWS, "keep")):
            ref = restate(st._row_start, st.image, st.x, st.y, policy)
            for name in OUTPUTS:
                stored = fx[fixture_key(name, tag, scene)]
                assert ref[name].dtype == stored.dtype and np.array_equal(ref[name], stored), (scene, tag, name)
        # under KEEP_ROWS a conflicting row is the track it was
        assert np.array_equal(ref["label"][ref["conflict"]], np.where(ref["conflict"])[0])


def test_p3data_figures():
    for st, figures in ((p3data(), FIGURES), (p3data_untruncated(), FIGURES_UNTRUNCATED)):
        assert scene_figures(st, restate(st._row_start, st.image, st.x, st.y, DROP)) == figures


def test_untruncated_parse_differs_from_read_matching_only_in_match_coordinates():
    a, b = p3data(), p3data_untruncated()
    assert np.array_equal(a.feature, b.feature) and np.array_equal(a.image, b.image)
    assert np.array_equal(np.trunc(b.x)[a.x != b.x], a.x[a.x != b.x])
    assert np.array_equal(np.trunc(b.y)[a.y != b.y], a.y[a.y != b.y])


def test_restatement_on_hand_made_rows():
    a, b, c, d = (0, 1.0, 2.0), (1, 3.0, 4.0), (1, 3.0, 5.0), (2, 7.0, 8.0)
    # rows 0 and 1 share a and disagree in image 1; row 2 is clean and shares nothing; row 3 repeats row 2's keypoint
    rows = [[a, b], [a, c], [d, (3, 1.0, 1.0)], [(0, -0.0, 9.0), d], [(0, 0.0, 9.0)]]
    rs, im, x, y = rows_of(rows)
    ref = restate(rs, im, x, y, DROP)
    assert ref["keypoint"].tolist() == [0, 1, 0, 3, 4, 5, 6, 4, 6]
    assert ref["component"].tolist() == [0, 0, 2, 2, 2]
    assert ref["conflict"].tolist() == [True, True, False, False, False]
    assert ref["label"].tolist() == [-1, -1, 2, 2, 2]
    assert ref["track_label"].tolist() == [2] and ref["track_start"].tolist() == [0, 3]
    assert ref["track_obs"].tolist() == [6, 4, 5]  # images 0, 2, 3
    assert ref["obs_slot"].tolist() == [-1, -1, -1, -1, 1, 2, 0, 1, 0]
    keep = restate(rs, im, x, y, KEEP_ROWS)
    assert keep["label"].tolist() == [0, 1, 2, 2, 2] and keep["track_label"].tolist() == [0, 1, 2]
    assert keep["track_obs"].tolist() == [0, 1, 0, 3, 6, 4, 5]
    assert keep["obs_slot"].tolist() == [0, 1, 2, 3, 5, 6, 4, 5, 4]


def test_header_declares_the_entry_point():
    txt = open(os.path.join(REPO, "include", "sfmcore.h")).read()
    m = re.search(r"\bint\s+sfm_merge_tracks\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/sfmcore.h does not declare sfm_merge_tracks"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["const int64_t *row_start", "int64_t n_rows", "const int32_t *image", "const double *x",
                    "const double *y", "int64_t n_obs", "int32_t n_images", "int32_t policy", "int32_t *keypoint",
                    "int32_t *component", "uint8_t *conflict", "int32_t *label", "int64_t *n_tracks",
                    "int32_t *track_label", "int64_t *track_start", "int32_t *track_obs", "int32_t *obs_slot",
                    "int device"]
    assert re.search(r"SFM_MERGE_DROP\s*=\s*0\s*,\s*SFM_MERGE_KEEP_ROWS\s*=\s*1", txt)
    import _sfmcore
    assert hasattr(_sfmcore._lib, "sfm_merge_tracks")
    assert len(dict((n, a) for n, _, a in _sfmcore.SIGNATURES)["sfm_merge_tracks"]) == len(args)
    assert (_sfmcore.MERGE_DROP, _sfmcore.MERGE_KEEP_ROWS) == (DROP, KEEP_ROWS)


def test_arguments_are_refused_before_a_device_is_looked_for():
    """each SFM_ERR_ARG case through the C ABI: -1 and no output touched (no GPU: the checks come first)"""
    import ctypes
    import _sfmcore as core
    rs, im, x, y = rows_of([[(0, 1.0, 2.0), (1, 3.0, 4.0)], [(0, 1.0, 2.0)]])
    cases = {"decreasing": dict(rs=np.array([0, 3, 2, 3])), "short": dict(rs=np.array([0, 2, 2])),
             "start": dict(rs=np.array([1, 2, 3])), "image_high": dict(im=np.array([0, 2, 0])),
             "image_negative": dict(im=np.array([0, -1, 0])), "nan": dict(x=np.array([1.0, np.nan, 1.0])),
             "inf": dict(y=np.array([2.0, 4.0, -np.inf])), "policy": dict(policy=2)}
    for name, change in cases.items():
        a = dict(rs=rs, im=im, x=x, y=y, policy=DROP)
        a.update(change)
        rs_, im_ = np.ascontiguousarray(a["rs"], dtype=np.int64), np.ascontiguousarray(a["im"], dtype=np.int32)
        n_rows = len(rs_) - 1
        i32 = [np.full(8, -7, dtype=np.int32) for _ in range(6)]
        cf, ts, nt = np.full(8, 9, dtype=np.uint8), np.full(8, -7, dtype=np.int64), np.full(1, -7, dtype=np.int64)
        P, I32, I64 = core._p, core._i32, core._i64
        rc = core._lib.sfm_merge_tracks(P(rs_, I64), n_rows, P(im_, I32), P(a["x"]), P(a["y"]), 3, 2, a["policy"],
                                        P(i32[0], I32), P(i32[1], I32), P(cf, core._u8), P(i32[2], I32), P(nt, I64),
                                        P(i32[3], I32), P(ts, I64), P(i32[4], I32), P(i32[5], I32), 0)
        assert rc == -1, name
        assert all((v == -7).all() for v in i32) and (cf == 9).all() and (ts == -7).all() and nt[0] == -7, name
        assert core._lib.sfm_last_error().startswith(b"argument:"), name
    assert ctypes.sizeof(ctypes.c_int32) == 4


def test_empty_inputs_need_no_device():
    import _sfmcore as core
    out = core.merge_tracks(np.zeros(1, dtype=np.int64), [], [], [], 3)
    assert all(len(out[n]) == 0 for n in OUTPUTS if n != "track_start") and out["track_start"].tolist() == [0]
    out = core.merge_tracks(np.zeros(4, dtype=np.int64), [], [], [], 3, core.MERGE_KEEP_ROWS)
    ref = restate(np.zeros(4, dtype=np.int64), [], [], [], KEEP_ROWS)
    for n in OUTPUTS:
        assert out[n].dtype == ref[n].dtype and np.array_equal(out[n], ref[n]), n
