"""Generates tests/golden/pair_stages_parent.npz on the MI355X: every output of
sfm_verify_pairs and sfm_essential_pairs on the batch of
tests/test_verify_pairs_gpu.py (stages_batch, STAGE_CALLS), as the library of
the checkout it runs in returns them.  It was run at the commit before the two
stages shared a refit loop and a host driver (pair_verify.hpp); the tests of
both stages compare every later build against it, bit for bit.  An array equal
to the main call's (the models do not depend on the threshold) is stored once.

The first seed is taken at which the batch holds no NaN and walks the paths
below, read off the info codes and by comparing calls.

    python tests/golden/make_golden_pair_stages.py [OUT.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_verify_pairs_gpu as vpg  # noqa: E402


def paths_missed(core, seed):
    """the batch at ``seed`` and what it lacks (nothing: [])"""
    out, miss = {}, []
    n_p = np.array(vpg.STAGE_SIZES)
    for stage, min_n in (("F", 8), ("E", 5)):
        o = vpg.stages_run(core, stage, seed)
        out.update(o)
        live = n_p >= min_n
        g = lambda call, name: o[f"{stage}_{call}_{name}"]  # noqa: E731
        if not all(np.isfinite(a).all() for a in o.values()):
            miss.append(f"{stage}: a value that is not finite")
        if not ((g("main", "info")[~live] == -1).all() and (g("main", "best_hyp")[~live] == -1).all()):
            miss.append(f"{stage}: dead pairs")
        # a threshold nothing meets: a winner all the same (the earliest finite, or count 0), kept as it is.
        # At 1e-9 a minimal sample can still hold its own points (five do, to 1e-13 px, some of them with a
        # residual of exactly 0: that call is recorded as it comes); the square of 1e-170 is 0, which nothing is below
        none = dict(info=g("none", "info")[live].tolist(), best_count=g("none", "best_count").tolist(),
                    counts=int(g("none", "counts").sum()), best_hyp=g("none", "best_hyp")[live].tolist())
        if none != dict(info=[-3] * int(live.sum()), best_count=[0] * len(n_p), counts=0, best_hyp=none["best_hyp"]) \
                or min(none["best_hyp"]) < 0:
            miss.append(f"{stage}: threshold 1e-170: {none}")
        if not ((g("high", "info")[live] == -3).all() and (g("high", "best_count")[live] > 0).all()):
            miss.append(f"{stage}: min_inliers above every count")
        # no refit asked for: info 0 wherever the winner had its inliers
        if not np.array_equal(g("rounds0", "info")[live], np.where(g("main", "info")[live] == -3, -3, 0)):
            miss.append(f"{stage}: refit_rounds 0: {g('rounds0', 'info').tolist()}")
        model = "F" if stage == "F" else "E"
        adopted = [p for p in np.where(live)[0] if not np.array_equal(g("main", model)[p], g("rounds0", model)[p])]
        if not adopted:
            miss.append(f"{stage}: no adopted round")
        info = g("main", "info")
        if stage == "E":
            if not (info > 0).any():
                miss.append("E: no positive LM code")
            continue
        if not (info == 1).any():
            miss.append("F: no stop on an unchanged mask")
        # info 2 after 3 rounds and after 50, with the same outputs and eight inliers to fit: a trial was
        # refused (50 strict improvements of a pair's (count, cost) in a row do not happen)
        far = vpg.stages_run(core, "F", seed, {"far": {"refit_rounds": 50}})
        refused = [p for p in np.where(info == 2)[0]
                   if g("main", "n_inliers")[p] >= 8 and far["F_far_info"][p] == 2 and np.array_equal(far["F_far_F"][p], g("main", "F")[p])]
        if not refused:
            miss.append("F: no trial refused as worse")
        print(f"seed {seed}: F info {info.tolist()}, adopted {adopted}, refused {refused}")
    return out, miss


def main():
    import _sfmcore as core
    core.require_device()
    for seed in range(200):
        out, miss = paths_missed(core, seed)
        print(f"seed {seed}: E info {out['E_main_info'].tolist()}; missing: {miss}", flush=True)
        if not miss:
            break
    assert not miss, "no seed in 0..199 walks every path"
    keep = {k: a for k, a in out.items()
            if "_main_" in k or not np.array_equal(a, out[k.split("_")[0] + "_main_" + k.split("_", 2)[2]])}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pair_stages_parent.npz")
    np.savez_compressed(path, seed=np.array(seed), **keep)
    print(f"seed {seed}: wrote {path}, {os.path.getsize(path)} bytes, {len(keep)} of {len(out)} arrays")


if __name__ == "__main__":
    main()
