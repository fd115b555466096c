"""Cost of dawn_index_remove (index_compact.hip) on a large f32 index, against a device-to-device copy of the same bytes.

  python tools/remove_bench.py [rows=100000000]

Cases: (a) one label at the last row, (b) one label at row 0 (every row moves), (c) 1000 scattered labels.  Each is timed as
the whole call (mark + scan, one synchronisation, the move, re-quantising the shadows from the first removed sub-tile, the
final synchronisation).  The yardstick is hipMemcpyAsync device-to-device (torch copy_) of a 4 GiB buffer, timed with events
in the same process before the index is built.  Per-kernel times (the move pass alone): run under
`rocprofv3 --kernel-trace --stats -- python tools/remove_bench.py` and read compact_move_kernel from the stats."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dawnsearch_amd as dawn  # noqa: E402
from dawnsearch_amd import synth  # noqa: E402


def copy_rate(device=0, gib=4, reps=5):
    import torch
    dev = torch.device("cuda", device)
    n = (gib << 30) // 4
    a = torch.empty(n, dtype=torch.float32, device=dev)
    b = torch.empty(n, dtype=torch.float32, device=dev)
    a.fill_(1.0)
    b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(reps):
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return 2.0 * (gib << 30) / (best * 1e-3) / 1e9  # GB/s read + written


def run(n=100_000_000, device=0):
    out = {"rows": n, "dtype": "f32", "copy_d2d_GBps": copy_rate(device)}
    idx = dawn.VectorIndex(device)
    idx.fill_synthetic(1, 0, n, 1)
    q = synth.unit_rows(2, 0, 1)[0]
    idx.search(q, 10)
    out["memory_before"] = idx.memory()

    def timed(name, ids):
        t0 = time.perf_counter()
        r = idx.remove(np.asarray(ids, dtype=np.uint64))
        dt = time.perf_counter() - t0
        out[name] = {"removed": r, "ms": dt * 1e3, "size_after": idx.size()}

    timed("a_last_row", [n])
    timed("b_row0", [1])
    moved = idx.size()
    out["b_row0"]["bytes_moved_rw"] = moved * (1536 + 8) * 2
    out["b_row0"]["call_GBps"] = out["b_row0"]["bytes_moved_rw"] / (out["b_row0"]["ms"] * 1e-3) / 1e9
    rng = np.random.default_rng(3)
    timed("c_1000_scattered", rng.choice(np.arange(2, n, dtype=np.uint64), 1000, replace=False))
    lab, dist = idx.search(q, 10)
    out["search_after"] = {"labels": [int(v) for v in lab[:3]]}
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    print(json.dumps(run(n)))
