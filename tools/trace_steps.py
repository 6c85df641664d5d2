"""    python tools/trace_steps.py <dir with a rocprofv3 --kernel-trace CSV>
All steps of a rocprofv3 kernel trace of the bench: per step the period, the tail (end of k_apply_side -> next step's
k_chunk_l1), the front (k_chunk_l1 start -> k_chunk_l2 start) and the middle (k_chunk_l2 end -> k_squeeze start)."""
import csv, glob, os, statistics, sys
path = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True))[-1]
rows = list(csv.DictReader(open(path)))
start = next(c for c in rows[0] if "start" in c.lower()); end = next(c for c in rows[0] if "end" in c.lower())
name = next(c for c in rows[0] if c.lower() in ("kernel_name", "name"))
ev = sorted(((int(r[start]), int(r[end]), r[name]) for r in rows), key=lambda e: e[0])
heads = [i for i, e in enumerate(ev) if "k_chunk_l1" in e[2]]
out = {"period": [], "tail": [], "front": [], "middle": [], "dispatches": []}
for a, b in zip(heads[:-1], heads[1:]):
    step = ev[a:b]
    f = lambda key: next(e for e in step if key in e[2])
    try:
        out["period"].append(ev[b][0] - step[0][0]); out["tail"].append(ev[b][0] - f("k_apply_side")[1])
        out["front"].append(f("k_chunk_l2")[0] - step[0][0]); out["middle"].append(f("k_squeeze")[0] - f("k_chunk_l2")[1])
        out["dispatches"].append(len(step))
    except StopIteration:
        pass
for k, v in out.items():
    v = v[-20:]
    print(f"{k:10s} n={len(v)} median {statistics.median(v) / (1 if k == 'dispatches' else 1e3):9.1f} min {min(v) / (1 if k == 'dispatches' else 1e3):9.1f} max {max(v) / (1 if k == 'dispatches' else 1e3):9.1f}")
