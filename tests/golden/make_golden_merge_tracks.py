"""Generate tests/golden/merge_tracks.npz: track merging on tests/golden/P3Data.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_merge_tracks.py

The matching files are read with the project's own parser (read_matching) and
merged by the plain-Python restatement of tests/test_merge_tracks.py, under
both policies.  Stored: keypoint, component and conflict (the same under both)
and, with the suffix _drop / _keep, label, track_label, track_start, track_obs
and obs_slot.  The same again with the suffix _untruncated for the files parsed
with every coordinate as a float (test_merge_tracks.p3data_untruncated).

Asserted here, the figures of DESIGN.md's "Track merging" table.  From the
untruncated parse, what the files hold: 3,833 rows and 9,226 observations;
5,562 distinct (image, x, y) keypoints, 2,192 of them in more than one row;
1,739 components, the largest of 29 rows, 230 of them conflicting; 931 / 310 /
178 / 90 consistent components of 2 / 3 / 4 / 5 views where the rows themselves
are 2,596 / 955 / 241 / 41.  Through read_matching, which keeps get_data's
int() truncation of the match coordinates (a line's own keypoint stays a
float, so it rarely equals the same keypoint listed as a match): 6,792
keypoints, 1,532 shared, 2,039 components, the largest of 27 rows, 633
conflicting, 1,257 / 133 / 15 / 1 consistent ones of 2 / 3 / 4 / 5 views.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_merge_tracks as mt  # noqa: E402


def main():
    out = {}
    for st, scene, figures in ((mt.p3data(), "", mt.FIGURES),
                               (mt.p3data_untruncated(), "_untruncated", mt.FIGURES_UNTRUNCATED)):
        for policy, tag in ((mt.DROP, "drop"), (mt.KEEP_ROWS, "keep")):
            ref = mt.restate(st._row_start, st.image, st.x, st.y, policy)
            for name in mt.OUTPUTS:
                key = mt.fixture_key(name, tag, scene)
                assert key not in out or np.array_equal(out[key], ref[name]), key
                out[key] = ref[name]
            if policy == mt.DROP:
                fig = mt.scene_figures(st, ref)
                print(scene or "read_matching", fig)
                assert fig == figures, (fig, figures)
                # every consistent component is one track
                assert len(ref["track_label"]) == fig["components"] - fig["conflicting"]
                assert len(ref["track_label"]) == sum(fig["consistent_by_views"])
    f = mt.FIGURES_UNTRUNCATED
    assert (f["rows"], f["keypoints"], f["components"], f["conflicting"]) == (3833, 5562, 1739, 230)
    assert f["consistent_by_views"] == [931, 310, 178, 90]
    path = os.path.join(HERE, "merge_tracks.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
