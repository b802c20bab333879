"""The staging helpers of the CSR entry points (csrc/staging.hpp) on a real
MI355X: packed buffers that regrow between calls, and the call timer.

A fresh host thread starts with empty device buffers, so a small call, a
larger one and the small one again walks the packed layout through an
allocation, a free-and-reallocate and a reuse; every output of every call
must equal, bit for bit, the same call made on the main thread.
"""
import threading

import numpy as np
import pytest

import test_multiview as tm
import test_register_views as trv
import test_robust_tracks as trt

pytestmark = pytest.mark.gpu
H = 64


@pytest.fixture(scope="module")
def core():
    import _sfmcore
    _sfmcore.require_device()
    return _sfmcore


def in_fresh_thread(fn):
    box = {}

    def body():
        try:
            box["out"] = fn()
        except BaseException as e:  # noqa: BLE001 -- handed to the caller's thread
            box["err"] = e

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if "err" in box:
        raise box["err"]
    return box["out"]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def head(c, T):
    """the first T tracks of a case"""
    n = int(c["track_start"][T])
    return c["P"], c["track_start"][:T + 1], c["obs_cam"][:n], c["obs_xy"][:n]


def tracks_calls(core):
    c = tm.load_problem("v5")
    return [lambda T=T: core.triangulate_tracks(*head(c, T)) for T in (1, c["T"], 1)]


def robust_calls(core):
    c = trt.load_case("r5o1")
    return [lambda T=T: core.triangulate_tracks_robust(*head(c, T), threshold=trt.THRESHOLD, min_inliers=3,
                                                       centres=c["C"]) for T in (1, c["T"], 1)]


def views_subset(views):
    """(X, view_start, pt_idx, xy, samples) of the scene's views in the given order"""
    sc = trv.load_scene()
    table = trv.sample_table(H)
    rows = [np.arange(sc["view_start"][v], sc["view_start"][v + 1]) for v in views]
    vs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    sel = np.concatenate(rows)
    return sc["X"], vs, sc["pt_idx"][sel], np.ascontiguousarray(sc["xy"][sel]), np.ascontiguousarray(table[list(views)])


def register_calls(core):
    # sizes 63 | 6, 7, 5, 63, 64 | 63: the five hold a view of fewer than six
    # between two runs of live ones, so the outputs come back in two pieces
    def call(views):
        X, vs, pt, xy, samples = views_subset(views)
        return core.register_views(trv.K, X, vs, pt, xy, samples, want_counts=True, want_models=True)

    return [lambda v=v: call(v) for v in ((3,), (1, 2, 0, 3, 4), (3,))]


CALLS = {"tracks": tracks_calls, "robust": robust_calls, "register": register_calls}


@pytest.mark.parametrize("entry", sorted(CALLS))
def test_buffers_regrow_between_calls(core, entry):
    calls = CALLS[entry](core)
    alone = [f() for f in calls]
    threaded = in_fresh_thread(lambda: [f() for f in calls])
    for i, (a, b) in enumerate(zip(alone, threaded)):
        assert same(a, b), (entry, i)
    assert same(alone[0], alone[2])
    assert len(alone[1][0]) > len(alone[0][0])


def test_call_timer_slots(core):
    core.set_call_timing(True)
    try:
        for entry in sorted(CALLS):
            CALLS[entry](core)[1]()
            t = core.last_timings()
            print(entry, t)
            assert len(t) == 4 and np.all(np.isfinite(t)) and np.all(t >= 0), (entry, t)
            if entry == "register":
                assert t[3] <= t[1], t  # the fit-and-score kernel is one of the two
            else:
                assert t[3] == t[1], (entry, t)
    finally:
        core.set_call_timing(False)
