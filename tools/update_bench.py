"""Cost of dawn_index_update (index_update.hip) on a large f32 index, against the remove + add_batch it replaces.

  python tools/update_bench.py [rows=100000000] [reps=20]
  python tools/update_bench.py --summarize KERNEL_TRACE_CSV [reps=20]

The run: an index of `rows` synthetic rows with labels 1..rows, then in this order: `reps` updates of 1, 256 and 10 000
scattered labels each (host calls, every one ends synchronised; median and min), then three rounds of remove + add_batch of as
many labels (the re-crawl route before dawn_index_update).  A round's rows move to the end of the index, so every round takes
labels of its own, drawn from rows that have not moved: its removal compacts from a scattered first position, as a re-crawl
does.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/update_bench.py`, then --summarize the
kernel trace: the dispatches of each update kernel split into the three request sizes in order."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1, 256, 10_000)
KERNELS = ("update_hits_kernel", "update_scatter_kernel", "update_dirty_list_kernel", "rows_to_i8s_list_kernel",
           "rows_to_i6s_list_kernel", "rows_to_f6s_list_kernel", "rows_f32_to_f16s_list_kernel", "i6_slack_hist_kernel")


def run(n, reps):
    import dawnsearch_amd as dawn
    from dawnsearch_amd import synth

    out = {"rows": n, "dtype": "f32", "reps": reps}
    idx = dawn.VectorIndex(0)
    t0 = time.perf_counter()
    idx.fill_synthetic(1, 0, n, 1)
    out["fill_s"] = time.perf_counter() - t0
    out["memory"] = idx.memory()
    rng = np.random.default_rng(7)
    perm = rng.permutation(n // 2).astype(np.uint64) + 1  # (labels of the first half: disjoint draws for the removal rounds)
    reqs = {m: rng.choice(np.arange(1, n + 1, dtype=np.uint64), size=m, replace=False) for m in SIZES}
    vecs = {m: [synth.unit_rows(100 + m, 0, m), synth.unit_rows(200 + m, 0, m)] for m in SIZES}
    for m in SIZES:
        assert (idx.update(reqs[m], vecs[m][1]) == 1).all()  # (warm-up: the staging grows once)
        t = []
        for r in range(reps):
            t0 = time.perf_counter()
            idx.update(reqs[m], vecs[m][r & 1])
            t.append((time.perf_counter() - t0) * 1e3)
        out[f"update_{m}"] = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}
    at = 0
    for m in SIZES:
        tr, ta = [], []
        for r in range(3):
            labels = perm[at:at + m]
            at += m
            t0 = time.perf_counter()
            assert idx.remove(labels) == m
            tr.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            idx.add_batch(labels, vecs[m][r & 1])
            ta.append((time.perf_counter() - t0) * 1e3)
        out[f"remove_add_{m}"] = {"remove_ms": tr, "add_batch_ms": ta,
                                  "total_median_ms": float(np.median(np.asarray(tr) + np.asarray(ta)))}
    return out


def summarize(csv_path, reps):
    import csv
    by = {k: [] for k in KERNELS}
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for k in KERNELS:
                if k in name:
                    by[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    per = reps + 1  # (+ the warm-up call of each size)
    for k, v in by.items():
        v.sort()
        if not v:
            continue
        ms = [(e - s) * 1e-6 for s, e in v]
        calls = len(ms) // (per * len(SIZES))  # launches per update call
        if calls and len(ms) == calls * per * len(SIZES):  # launches per call: equal for every call
            for i, m in enumerate(SIZES):
                part = ms[i * per * calls:(i + 1) * per * calls]
                out.setdefault(k, {})[f"size_{m}"] = {"launches_per_call": calls, "median_ms_per_launch": float(np.median(part)),
                                                     "ms_per_call": float(np.sum(part)) / per}
        else:
            out[k] = {"dispatches": len(ms), "median_ms": float(np.median(ms)), "total_ms": float(np.sum(ms))}
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        a = sys.argv[2:]
        print(json.dumps(summarize(a[0], int(a[1]) if len(a) > 1 else 20)))
    else:
        n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
        print(json.dumps(run(n, reps)))
