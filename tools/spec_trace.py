"""Per-iteration table from a rocprofv3 kernel trace (csv) of tools/ba_once.py:
the reduced solve's duration alone and beside the speculative chain, the
speculative sweep's duration, and the chain's tail past the end of the trial
(what k_lm_step waits for).  usage: spec_trace.py run_kernel_trace.csv"""
import csv
import re
import sys

rows = []
for r in csv.DictReader(open(sys.argv[1])):
    m = re.search(r"(k_\w+)", r["Kernel_Name"])
    if m:
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(1), r["Stream_Id"]))
rows.sort()
steps = [i for i, r in enumerate(rows) if r[2] == "k_lm_step"]
main = rows[steps[0]][3]
print("it  period  solve  trial  own_sweep  spec_prep  spec_sweep  spec_tail_past_trial   (us)")
alone, beside, sweeps, tails = [], [], [], []
for n, (a, b) in enumerate(zip(steps[:-1], steps[1:])):
    it = rows[a + 1:b + 1]
    get = lambda name, own: [(e - s) / 1e3 for s, e, k, st in it if k.startswith(name) and (st == main) == own]
    solve, trial = get("k_gj", True)[0], get("k_backsub_trial", True)[0]
    own_sw = get("k_schur_sweep", True)[0]
    sp_prep, sp_sw = get("k_point_prep", False), get("k_schur_sweep", False)
    trial_end = [e for s, e, k, st in it if k.startswith("k_backsub_trial")][0]
    sp_end = [e for s, e, k, st in it if st != main]
    tail = (max(sp_end) - trial_end) / 1e3 if sp_end else None
    period = (rows[b][0] - rows[a][0]) / 1e3
    (beside if sp_sw else alone).append(solve)
    if sp_sw:
        sweeps.append(sp_sw[0])
        tails.append(tail)
    print(f"{n + 1:2d} {period:7.1f} {solve:6.1f} {trial:6.1f} {own_sw:10.1f} "
          + (f"{sp_prep[0]:10.1f} {sp_sw[0]:11.1f} {tail:21.1f}" if sp_sw else f"{'-':>10} {'-':>11} {'-':>21}"))
med = lambda v: sorted(v)[len(v) // 2] if v else float("nan")
print(f"solve alone: median {med(alone):.1f} us over {len(alone)}; beside the chain: median {med(beside):.1f} us over "
      f"{len(beside)}; speculative sweep: median {med(sweeps):.1f} us; tail past the trial: median {med(tails):.1f} us")
