"""Cost of the rows-by-label calls (index_lookup.hip) on a large f32 index.

  python tools/lookup_bench.py [rows=100000000] [reps=20]
  python tools/lookup_bench.py --summarize KERNEL_TRACE_CSV [reps=20] [rows=100000000] [read_GBps]

The run: the bare-read rate of tools/probes/hbm_read (quick mode, 19.2 GB, a child process before the index is built), then
an index of `rows` synthetic rows with labels 1..rows, then in this order: `reps` counts-only dawn_index_get calls of 1 label
(the lookup launch alone), `reps` of 256 labels, and the end-to-end times of dawn_index_search_like against
dawn_index_search_batch on the vectors dawn_index_get returned, B = 1 and 256 (median of `reps` calls each, interleaved).
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/lookup_bench.py`, then --summarize the
kernel trace: the first `reps` label_lookup_kernel dispatches are the 1-label calls, the next `reps` the 256-label ones; the
label array is 8 B per row, so its read rate is 8 * rows / kernel time."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_rate():
    exe = os.path.join(ROOT, "tools", "probes", "hbm_read")
    out = subprocess.run([exe, "19.2", "4", "quick"], capture_output=True, text=True, timeout=180).stdout
    return json.loads([ln for ln in out.splitlines() if ln.strip()][-1])["hbm_read_ceiling_GBps"]


def run(n, reps):
    import dawnsearch_amd as dawn
    from dawnsearch_amd import _lib

    out = {"rows": n, "dtype": "f32", "reps": reps, "hbm_read_GBps": read_rate()}
    idx = dawn.VectorIndex(0)
    idx.fill_synthetic(1, 0, n, 1)
    rng = np.random.default_rng(7)
    p1 = np.asarray([n // 2 + 1], dtype=np.uint64)
    p256 = rng.integers(1, n + 1, size=256).astype(np.uint64)
    cnt = np.zeros(256, dtype=np.uintp)

    def counts_only(p):
        t0 = time.perf_counter()
        rc = _lib.lib.dawn_index_get(idx._h, len(p), p.ctypes.data, None, cnt.ctypes.data)
        assert rc == 0
        return (time.perf_counter() - t0) * 1e3

    for name, p in (("get_counts_1", p1), ("get_counts_256", p256)):
        t = [counts_only(p) for _ in range(reps)]
        out[name] = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t))}
    for B in (1, 256):
        p = p1 if B == 1 else p256
        rows, counts = idx.get(p)
        assert (counts == 1).all()
        idx.search_batch(rows, 10)  # (warm-up: the paths and their feedback)
        idx.search_like(p, 10)
        tl, tb = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            a = idx.search_like(p, 10)
            tl.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            e = idx.search_batch(rows, 10)
            tb.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(a[0], e[0]) and np.array_equal(a[1].view(np.uint32), e[1].view(np.uint32))
        out[f"B{B}"] = {"search_like_median_ms": float(np.median(tl)), "search_batch_median_ms": float(np.median(tb)),
                        "search_like_min_ms": float(np.min(tl)), "search_batch_min_ms": float(np.min(tb))}
    return out


def summarize(csv_path, reps, n, read_gbps=None):
    import csv
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            if "label_lookup_kernel" in r.get("Kernel_Name", ""):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    ms = [(e - s) * 1e-6 for s, e in rows]
    out = {"lookup_dispatches": len(ms)}
    for name, part in (("probes_1", ms[:reps]), ("probes_256", ms[reps:2 * reps])):
        if not part:
            continue
        med = float(np.median(part))
        out[name] = {"median_ms": med, "min_ms": float(np.min(part)), "GBps": 8.0 * n / (med * 1e-3) / 1e9}
        if read_gbps:
            out[name]["of_bare_read"] = out[name]["GBps"] / read_gbps
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        a = sys.argv[2:]
        print(json.dumps(summarize(a[0], int(a[1]) if len(a) > 1 else 20, int(a[2]) if len(a) > 2 else 100_000_000,
                                   float(a[3]) if len(a) > 3 else None)))
    else:
        n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
        print(json.dumps(run(n, reps)))
