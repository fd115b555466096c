#!/usr/bin/env python3
"""bench.py — DawnSearch embed-and-rank hot path on MI355X: exact cosine scan + top-k throughput.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1 launched one rank per GPU
with torch.distributed.run (RCCL).  Prints ONE JSON line on rank 0.

Workload (BASELINE.json metric: queries/s + p50 latency, 100M x 384 index, batch 1 & 256, 1/2/4/8 GPUs):
  * the 100M x 384 f32 index (153.6 GB) is generated on the GPU(s) from the seeded synthetic spec
     and stays resident in HBM; with N ranks each holds a contiguous 100M/N-row shard
    (strong scaling: total index fixed, as the metric is quoted);
  * a step = one search of a batch of B query vectors (default B=1, k=10), queries already in HBM,
    through dawn_index_search_device (filter scan -> merge/exact rescore/certificate -> predicated
    exact fallback); for N>1 the per-shard top-k lists are all-gathered over RCCL and merged by
    dawn_topk_merge_device on every rank;
  * `value` = queries per second over the timed K steps (max over ranks).
  * `ms_per_step` = milliseconds of one timed step; `--dump-outputs DIR` writes what the last timed step of the
    headline leg returned (labels, distances, found) as DIR/*.npy — the inputs are seeded, so two builds can be
    compared output for output.
Extra legs, reported in the same line: batch-256 throughput, host-API p50 latency, the 1M-row
configuration, roofline of the dominant kernel (HIP events recorded by the library around the scan
kernel on its launch stream), and a CPU baseline (oracle, bounded sample) on rank 0 at N=1.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
ROW_BYTES = 384 * 4
I6_MIN_ROWS = 3 << 18  # indexes of at least this many rows answer single queries from the packed 5-bit shadow (option i6_min_rows)

MAX_LINE_BYTES = 8192  # the driver keeps the last 8 KB of stdout: the result line must fit (round-4 verdict: a 20 KB line was lost)
EXTRA_FILE = os.path.join(ROOT, "bench_extra.json")  # every leg in full; the result line carries the headline scalars only
DUMP_MAX_BYTES = 64 << 20  # --dump-outputs: all .npy files of one dump together


def _get(d, *path):
    for p in path:
        if not isinstance(d, dict) or p not in d:
            return None
        d = d[p]
    return d


def _r(v, nd=4):
    return round(float(v), nd) if isinstance(v, (int, float)) and not isinstance(v, bool) else v


def short_line(full: dict) -> dict:
    """The ONE result line of the driver's contract, built from the full result dict: the contract's keys, `roofline` and
    `cpu_baseline` without prose, `checks`, and a dozen scalar headlines of the extra legs.  Everything else is in
    bench_extra.json and on earlier stdout lines (prefixed "extra: ").  Hard-checked to stay under MAX_LINE_BYTES."""
    cfg = full.get("config", {})
    rf = full.get("roofline", {})
    ex = full.get("extra", {}) or {}
    line = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                     "scaling", "vs_baseline", "dtype", "data")}
    line["config"] = {k: cfg.get(k) for k in ("workload", "rows_total", "rows_per_gpu", "batch", "k", "ranks", "shards", "sharding",
                                              "collective_backend", "rccl_ranks", "pipelined", "oversubscribed") if k in cfg}
    line["config"]["workload"] = str(cfg.get("workload", ""))[:200]
    line["roofline"] = {k: rf.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic",
                                               "algorithmic_bytes_per_launch", "avg_launch_ms", "launches_timed",
                                               "frac_of_measured_read_ceiling")}
    line["roofline"]["kernel"] = str(rf.get("kernel", "")).split(" ")[0]
    mc = rf.get("measured_read_ceiling") or {}
    ceil = [mc.get(k) for k in ("GBps", "GBps_12B_per_lane", "GBps_packed_stream_pattern") if mc.get(k)]
    line["roofline"]["measured_read_ceiling_GBps"] = max(ceil) if ceil else None
    cb = full.get("cpu_baseline")
    if cb is not None:
        line["cpu_baseline"] = {"value": cb.get("value"), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                                "sample": str(cb.get("sample", ""))[:160], "all_cores": cb.get("all_cores"),
                                "embedder_ms_per_text_1_thread": _get(cb, "embedder", "threads_1", "ms_per_text")}
    line["checks"] = {k: v for k, v in (full.get("checks") or {}).items() if not isinstance(v, (dict, list))}
    if full.get("latency_ms"):
        line["latency_ms"] = {k: v for k, v in full["latency_ms"].items() if k != "what"}
    heads = {
        "batch1_p50_ms_host_api": _get(ex, "host_api_batch1", "p50_ms"),
        "batch256_ms": _get(ex, "batch256", "ms_per_step"),
        "batch256_qps": _get(ex, "batch256", "queries_per_s"),
        "batch256_p50_ms_host_api": _get(ex, "host_api_batch256", "p50_ms"),
        "batch256_first_filter": _get(ex, "batch256", "first_filter") or "int8",
        "batch256_int8_first_filter_ms": _get(ex, "batch256_int8_first_filter", "ms_per_step"),
        "f32_row_stream_hbm_frac": _get(ex, "batch1_streaming_f32_rows", "hbm_frac"),
        "i8_stream_hbm_frac": _get(ex, "batch1_streaming_i8_shadow", "hbm_frac"),
        "topical_batch1_ms": _get(ex, "rows_clustered_topical", "k10_batch1", "ms_per_step"),
        "topical_batch256_ms": _get(ex, "rows_clustered_topical", "k10_batch256", "ms_per_step"),
        "topical_batch256_bounded_rate": _get(ex, "rows_clustered_topical", "k10_batch256", "bounded_rate"),
        "rows_50M_batch1_ms": _get(ex, "rows_50M_batch1", "ms_per_step"),
        "rows_50M_batch256_ms": _get(ex, "rows_50M_batch256", "ms_per_step"),
        "rows_25M_batch1_ms": _get(ex, "rows_25M_batch1", "ms_per_step"),
        "rows_25M_batch256_ms": _get(ex, "rows_25M_batch256", "ms_per_step"),
        "rows_12p5M_batch1_ms": _get(ex, "rows_12p5M_batch1", "ms_per_step"),
        "rows_12p5M_batch256_ms": _get(ex, "rows_12p5M_batch256", "ms_per_step"),
        "rows_1M_batch1_ms": _get(ex, "rows_1M_batch1", "ms_per_step"),
        "rows_1M_batch256_ms": _get(ex, "rows_1M_batch256", "ms_per_step"),
        "embed_one_text_ms": _get(ex, "embed_batch1", "embed_ms"),
        "embed_256_texts_ms": _get(ex, "e2e_1M_batch256", "embed_ms"),
        "bf16_index_batch1_ms": _get(ex, "bf16_index_batch1", "ms_per_step"),
        "fallbacks_all_legs": _get(full, "checks", "all_legs_on_this_index", "fallbacks"),
        "topical_12p5M_batch1_ms": _get(ex, "rows_12p5M_clustered_topical", "k10_batch1", "ms_per_step"),
        "topical_12p5M_batch256_ms": _get(ex, "rows_12p5M_clustered_topical", "k10_batch256", "ms_per_step"),
        "predicted_speedup_8gpu_batch1": _get(ex, "predicted_scaling", "predicted_speedup", 8, "batch1"),
        "predicted_speedup_8gpu_batch256": _get(ex, "predicted_scaling", "predicted_speedup", 8, "batch256"),
    }
    line["extra"] = {k: _r(v) for k, v in heads.items() if v is not None}
    if full.get("mfma_busy_frac"):
        line["extra"]["int8_pass_mfma_busy_frac_pmc"] = _get(full, "mfma_busy_frac", "value")
        if _get(full, "mfma_busy_frac", "fp6_pass") is not None:
            line["extra"]["fp6_pass_mfma_busy_frac_pmc"] = _get(full, "mfma_busy_frac", "fp6_pass")
    line["extra_file"] = os.path.basename(EXTRA_FILE)
    for k in ("value", "ms_per_step"):
        line[k] = _r(line[k], 6)
    for k in ("achieved", "frac", "avg_launch_ms", "frac_of_measured_read_ceiling", "measured_read_ceiling_GBps"):
        line["roofline"][k] = _r(line["roofline"].get(k), 6)
    text = json.dumps(line)
    assert len(text) < MAX_LINE_BYTES, f"bench.py: the result line is {len(text)} bytes (limit {MAX_LINE_BYTES})"
    return line


def emit(full: dict) -> None:
    """bench_extra.json + one "extra: " stdout line per leg (never starting with '{'), then the result line, last."""
    try:
        with open(EXTRA_FILE, "w") as f:
            json.dump(full, f, indent=1)
    except OSError as e:
        print(f"extra: (could not write {EXTRA_FILE}: {e!r})")
    for name, leg in (full.get("extra") or {}).items():
        print("extra: " + json.dumps({name: leg}))
    for name in ("certificate_criterion", "hbm_bytes_per_gpu", "fill_seconds", "mfma_busy_frac", "cpu_baseline"):
        if name in full:
            print("extra: " + json.dumps({name: full[name]}))
    print("extra: " + json.dumps({"roofline_full": full.get("roofline")}))
    sys.stdout.flush()
    print(json.dumps(short_line(full)), flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=100_000_000, help="total index rows (all GPUs)")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--no-extras", action="store_true", help="skip batch-256 / 1M / latency / cpu legs")
    ap.add_argument("--cpu-sample-rows", type=int, default=1_000_000)
    ap.add_argument("--no-pipeline", action="store_true",
                    help="N > 1: all-gather + merge of a step finish before the next search starts (no overlap)")
    ap.add_argument("--no-capi-sharded", action="store_true",
                    help="N > 1: skip the single-process leg (tools/sharded_capi_bench.py: one process, N GPUs, C ABI only)")
    ap.add_argument("--force-collective", action="store_true",
                    help="run the all-gather + packed merge even at world size 1 (exercises the N>1 code path)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps of the headline leg, write what its last step returned (labels, distances, "
                         "found) as DIR/<name>.npy, for comparing two builds output for output")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def dump_outputs(dirpath: str, arrays: dict) -> dict:
    """--dump-outputs: `arrays` (each [B, ...], one row per query) as dirpath/<name>.npy, integers as float64 (exact below
    2**53: labels are row ids), floats as float32.  Past DUMP_MAX_BYTES in all, the same seeded sample of rows is kept from
    every array and its row numbers are written as rows.npy.  Returns {file name: shape}."""
    os.makedirs(dirpath, exist_ok=True)
    conv = {n: np.ascontiguousarray(a, dtype=np.float64 if a.dtype.kind in "iub" or a.dtype == np.float64 else np.float32)
            for n, a in arrays.items()}
    n_rows = len(next(iter(conv.values())))
    assert all(len(a) == n_rows for a in conv.values()), {n: a.shape for n, a in conv.items()}
    total = sum(a.nbytes for a in conv.values())
    if total + 4096 > DUMP_MAX_BYTES:  # (4 KiB: the .npy headers)
        per_row = total // max(n_rows, 1) + 8  # (+ its entry in rows.npy)
        keep = max(1, min(n_rows, (DUMP_MAX_BYTES - 4096) // per_row))
        rows = np.sort(np.random.default_rng(0).choice(n_rows, keep, replace=False))
        conv = {n: a[rows] for n, a in conv.items()}
        conv["rows"] = rows.astype(np.float64)
    for n, a in conv.items():
        np.save(os.path.join(dirpath, n + ".npy"), a)
    return {n + ".npy": list(a.shape) for n, a in conv.items()}


def cpu_baseline(sample_rows: int, k: int, total_rows: int):
    """Oracle (C restatement of vector.rs:128-134 + exact top-k), 1 thread, on a bounded sample."""
    from oracle import oracle_lib as O
    from dawnsearch_amd import synth
    x = O.unit_rows(1, 0, sample_rows)
    ids = np.arange(1, sample_rows + 1, dtype=np.uint64)
    Q = synth.unit_rows(2, 0, 64)
    t0 = time.time()
    nq = 0
    while nq < 64 and (time.time() - t0 < 12.0 or nq < 2):
        O.scan_topk(x, ids, Q[nq], k, threads=1)
        nq += 1
    t1 = time.time() - t0
    rows_per_s = nq * sample_rows / t1
    # all-cores variant (OpenMP) for reference
    cores = min(len(os.sched_getaffinity(0)), 64)
    t0 = time.time()
    nq2 = 0
    while nq2 < 64 and (time.time() - t0 < 5.0 or nq2 < 2):
        O.scan_topk(x, ids, Q[nq2], k, threads=cores)
        nq2 += 1
    t2 = time.time() - t0
    return {
        "value": rows_per_s / total_rows, "unit": "queries/s", "cores": 1, "kind": "port",
        "sample": f"{nq} queries x {sample_rows} rows of the same synthetic index, sequential-f32 oracle, "
                  f"scaled to {total_rows} rows ({rows_per_s / 1e6:.2f} M rows/s)",
        "all_cores": {"value": nq2 * sample_rows / t2 / total_rows, "cores": cores},
    }


def cpu_embedder_baseline():
    """CPU embedder baseline: the oracle's MiniLM forward (C restatement of src/embedding/model.rs), one text
    per call as the reference does (embedding_service.rs:161-163), 1 thread and all cores."""
    from oracle import oracle_lib as O
    from dawnsearch_amd import synth
    import ctypes
    m = O.SynthBert(3)
    seqs = synth.token_sequences(5, 8, 4, 32)
    res = {}
    gomp = ctypes.CDLL("libgomp.so.1")  # the oracle's GEMM loops are `#pragma omp parallel for`
    for name, threads in (("threads_1", 1), ("all_cores", min(len(os.sched_getaffinity(0)), 64))):
        gomp.omp_set_num_threads(threads)
        m.embed(seqs[0])
        t0 = time.time()
        n = 0
        while n < len(seqs) and (time.time() - t0 < 4.0 or n < 2):
            m.embed(seqs[n])
            n += 1
        res[name] = {"texts_per_s": n / (time.time() - t0), "ms_per_text": (time.time() - t0) / n * 1e3, "threads": threads}
    res["what"] = "oracle MiniLM-L6 forward + mean-pool + normalise, 4-32 tokens per text, synthetic weights"
    return res


def rust_probe(sample_rows: int):
    """if a Rust toolchain is on the box, compile the std-only restatement of the reference's scan loop
    (tools/cpu_scan.rs) and time it; otherwise say so."""
    import shutil
    import subprocess
    import tempfile
    rustc = shutil.which("rustc")
    if not rustc:
        return {"rustc": None, "note": "no rustc on this box: the reference's Rust CPU path cannot be built here; "
                                       "cpu_baseline is the C restatement (kind = port)"}
    try:
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "cpu_scan")
            subprocess.run([rustc, "-O", "-o", exe, os.path.join(ROOT, "tools", "cpu_scan.rs")], check=True,
                           capture_output=True, timeout=120)
            out = subprocess.run([exe, str(sample_rows)], check=True, capture_output=True, text=True, timeout=120).stdout
        r = json.loads(out.strip().splitlines()[-1])
        r["rustc"] = rustc
        return r
    except Exception as e:
        return {"rustc": rustc, "error": repr(e)}


def read_ceiling_probe(timeout_s: float = 120.0):
    """The bare-read ceiling of THIS chip, measured in this run: tools/probes/hbm_read (the headline kernel's stream with
    nothing but the loads: same grid, 16 B/lane nt loads, 24-48 KiB in flight per CU) over a 19.2 GB buffer, as a child
    process beside the resident index.  None if the binary is not built (python -c 'import __graft_entry__ as g; g.build()')."""
    import subprocess
    exe = os.path.join(ROOT, "tools", "probes", "hbm_read")
    if not os.path.exists(exe):
        return None
    try:
        # (19.2 GB: far beyond the 256 MiB Infinity Cache, and it fits beside a 100 M-row index that keeps all four shadows)
        out = subprocess.run([exe, "19.2", "4", "quick"], capture_output=True, text=True, timeout=timeout_s).stdout
        lines = [ln for ln in out.splitlines() if ln.strip()]
        js = json.loads(lines[-1])
        best = js["hbm_read_ceiling_GBps"]
        return {"GBps": best, "frac_of_spec": best / HBM_PEAK_GBS, "GBps_12B_per_lane": js.get("hbm_read_ceiling_12B_GBps"),
                "GBps_packed_stream_pattern": js.get("hbm_read_ceiling_i5_pattern_GBps"),
                "lines": [ln for ln in lines if "GB/s" in ln],
                "what": "tools/probes/hbm_read.hip quick mode: best of the bare 16 B/lane nt read streams (2 / 4 / 8 waves per CU, "
                        "rings of 6 and 12 fragments, chip-wide window and per-XCD ranges) over 19.2 GB, 4 launches each; "
                        "GBps_12B_per_lane: the same for 12 B/lane loads (global_load_dwordx3, 768-B "
                        "fragments, 3 / 4 / 8 waves per CU); GBps_packed_stream_pattern: the headline kernel's own mix of loads (per "
                        "7680-B sub-tile two dwordx3 and six dwordx4 loads, rings of 4 and 8) with nothing but the loads"}
    except Exception as e:
        return {"error": repr(e)}


def capi_sharded_leg(n_gpus: int, rows: int, k: int, steps: int, warmup: int, batch: int, logical: bool = False,
                     timeout_s: float = 420.0):
    """The product's own multi-GPU form — ONE process, dawn_index_create_sharded over the N devices, RCCL inside the library —
    measured by tools/sharded_capi_bench.py in a child process (it must own all N devices; this process is one of N ranks).
    logical: a box with fewer GPUs than ranks — G logical shards on device 0 (functional check, not a measurement)."""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sharded_capi_bench.py"), "--rows", str(rows), "--k", str(k),
           "--steps", str(steps), "--warmup", str(warmup), "--batch", str(batch)]
    cmd += ["--logical", str(n_gpus)] if logical else ["--gpus", str(n_gpus)]
    env = {kk: v for kk, v in os.environ.items()
           if kk not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE", "GROUP_RANK",
                         "ROLE_RANK", "TORCHELASTIC_RUN_ID")}
    res = {"command": " ".join(cmd[1:]), "modes": []}
    try:
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=env)
        try:
            stdout, _ = proc.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            proc.kill()
            stdout, _ = proc.communicate()
            res["error"] = f"timed out after {timeout_s:.0f} s"
        res["returncode"] = proc.returncode
        for ln in (stdout or "").splitlines():
            if ln.startswith("{"):
                try:
                    res["modes"].append(json.loads(ln))
                except Exception:
                    pass
    except Exception as e:
        res["error"] = repr(e)
    return res


def launch_ranks(args) -> int:
    """A bare `python bench.py --gpus N` with N > 1 (no WORLD_SIZE in the environment): start N fresh ranks — one process
    per GPU, torch.distributed.run, RCCL — BEFORE this process touches the GPU (it never does), relay rank 0's JSON line
    as the last line of stdout and exit with the job's code.  (Never re-exec a process that has initialised HIP.)"""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is None:
        print(json.dumps({"error": f"the {args.gpus}-rank job printed no result line", "returncode": proc.returncode}))
        return proc.returncode or 1
    print(line, flush=True)
    return proc.returncode


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args))
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...), "
                         "or run `python bench.py --gpus N` without WORLD_SIZE and let it start the ranks")
    n_dev = torch.cuda.device_count()  # (does not initialise the GPU)
    if n_dev < 1 or not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback exists for the product path)")
    # fewer GPUs than ranks (a 1-GPU box asked for --gpus 2): ranks share devices and exchange their result blobs
    # through gloo — RCCL cannot put two ranks on one device.  The line is then marked "oversubscribed": a functional
    # check of the N-rank flow, not a measurement.
    oversub = world > n_dev
    dev_index = local_rank % n_dev
    backend = "gloo" if oversub else "nccl"
    if world > 1 or args.force_collective:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if oversub:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index), rank=rank, world_size=world)
    local_rank = dev_index
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import dawnsearch_amd as dawn
    from dawnsearch_amd import synth

    B, k = args.batch, args.k
    # ---- N > 1: the HEADLINE is the product's own multi-GPU form, one process behind the C ABI (dawn_index_create_sharded over
    # the N devices, RCCL all-gather inside the library), measured by a child of rank 0 that owns all devices while the ranks
    # wait on the CPU (gloo; an NCCL barrier would spin a kernel on every GPU under the measurement) with nothing resident yet.
    # The rank-per-GPU torch.distributed form below is then reported in extra.torch_distributed_ranks.
    capi = None
    if world > 1 and not args.no_capi_sharded:
        ctl = None if oversub else dist.new_group(backend="gloo")
        if rank == 0:
            capi = capi_sharded_leg(world, args.rows, k, args.steps, args.warmup, B, logical=oversub)
        dist.barrier(group=ctl)
    rows_local = args.rows // world
    first_row = rank * rows_local
    idx = dawn.VectorIndex(local_rank)
    t0 = time.time()
    idx.fill_synthetic(1, first_row, rows_local, first_id=1 + first_row)
    fill_s = time.time() - t0

    stream = torch.cuda.current_stream().cuda_stream

    def make_step(index, Bq, seed=2):
        q_host = synth.unit_rows(seed, 0, Bq)
        if Bq >= 1:  # planted: query 0 is a noisy copy of global row 4242 (checked after the run)
            q_host[0] = synth.planted_queries(1, [4242 % args.rows], 5)[0]
        d_q = torch.from_numpy(q_host).to(dev)
        # per-rank result blob: labels | distances | found (dawn_hip.h) — one all-gather per search.  Two sets of buffers:
        # with RCCL the all-gather + merge of step i run (NCCL stream) under the scan of step i + 1 (double buffering; a
        # search server pipelines its batches the same way) — `value` is a throughput; latency is reported by the host_api legs
        nbytes = dawn.result_blob_bytes(Bq, k)
        off_d, off_f = Bq * k * 8, Bq * k * 12
        collective = world > 1 or args.force_collective
        pipelined = collective and not oversub and not args.no_pipeline
        nbuf = 2 if pipelined else 1
        blobs = [torch.zeros((nbytes,), dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        g_blobs = [torch.zeros((world * nbytes,), dtype=torch.uint8, device=dev) if collective else None for _ in range(nbuf)]
        o_lab = torch.zeros((Bq, k), dtype=torch.int64, device=dev)
        o_dist = torch.zeros((Bq, k), dtype=torch.float32, device=dev)
        o_found = torch.zeros((Bq,), dtype=torch.int32, device=dev)
        state = {"i": 0, "pending": None}

        def merge(j):
            dawn.topk_merge_packed_device(local_rank, world, Bq, k, g_blobs[j].data_ptr(), o_lab.data_ptr(),
                                          o_dist.data_ptr(), o_found.data_ptr(), stream)

        def drain():
            if state["pending"] is not None:
                j, work = state["pending"]
                work.wait()  # the current stream waits for the collective (long finished: it ran under the next scan)
                merge(j)
                state["pending"] = None

        def step():
            j = state["i"] % nbuf
            state["i"] += 1
            p = blobs[j].data_ptr()
            index.search_device(d_q.data_ptr(), Bq, k, p, p + off_d, p + off_f, stream)
            if collective and oversub:  # shared device: the blobs travel through host memory (gloo)
                hb = blobs[j].cpu()
                hg = torch.empty((world * nbytes,), dtype=torch.uint8)
                dist.all_gather_into_tensor(hg, hb)
                g_blobs[j].copy_(hg)
                merge(j)
            elif pipelined:
                work = dist.all_gather_into_tensor(g_blobs[j], blobs[j], async_op=True)
                drain()  # the previous step's gather + merge, behind this step's scan on the stream
                state["pending"] = (j, work)
            elif collective:
                dist.all_gather_into_tensor(g_blobs[j], blobs[j])
                merge(j)

        def result():
            """labels [Bq, k] int64, distances [Bq, k] f32, found [Bq] u32 of the last step"""
            drain()
            torch.cuda.synchronize()
            if collective:
                return o_lab.cpu().numpy(), o_dist.cpu().numpy(), o_found.cpu().numpy()
            raw = blobs[0].cpu().numpy()
            return (raw[:off_d].view(np.int64).reshape(Bq, k), raw[off_d:off_f].view(np.float32).reshape(Bq, k),
                    raw[off_f:off_f + Bq * 4].view(np.uint32).copy())

        step.drain = drain
        return step, result

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def settle(seconds=2.0):
        """After anything that RELEASES tens of GB of HBM (an option that drops a shadow, an index closed): every stream on the device
        runs ~3 % slower behind such a hipFree until the device has idled for a second or two (profiles/r05/stream_after_free_probe.log;
        rounds 3 and 4 timed their f32-row and int8 stream legs right behind the release of the packed shadow and read it as a
        regression of the kernels).  The library itself only releases shadows on option changes."""
        torch.cuda.synchronize()
        time.sleep(seconds)

    def scan_passes(Bq):
        """Passes over the index rows made by the dominant kernel for a batch of Bq queries."""
        if Bq >= 2:
            return -(-Bq // 256)          # matrix-core path: 256 queries per pass (scan_batched.hip)
        return -(-Bq // 8)                # streaming path over 16-bit fragments: 8 queries per pass

    def run_leg(index, Bq, steps, warmup, seed=2, check_planted=False, rows_read="default", dump_dir=None):
        """`steps` timed searches of a Bq-query batch.  Returns qps (max over ranks), ms/step and the mean
        duration of the dominant scan kernel measured with HIP events on its launch stream.  dump_dir: rank 0 writes the
        last timed step's results there (dump_outputs)."""
        step, result = make_step(index, Bq, seed)
        f6_before = index.stats_batch_feedback()["f6_batches"] if Bq >= 2 else 0
        index.profile_enable(True)
        for _ in range(warmup):
            step()
        step.drain()
        barrier()
        index.profile_read()  # drop warm-up launches
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        step.drain()  # (pipelined ranks: the last step's gather + merge)
        barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device="cpu" if oversub else dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        n_launch, scan_ms = index.profile_read()
        index.profile_enable(False)
        leg = {"queries_per_s": steps * Bq / el, "ms_per_step": el / steps * 1e3, "steps": steps,
               "scan_kernel_ms": scan_ms / max(n_launch, 1), "launches_timed": n_launch}
        rows_here = index.size()
        # bytes the dominant kernel has to read per row (the exact rescore touches 64 f32 rows per query on top):
        #   "i8"  384.25: the int8 shadow of the index rows (+ 8 B of scale/bound per 32 rows), every batch size
        #   "f16" 768: the f16 shadow of an f32 index, or the rows of a bf16 index themselves (i8_shadow = 0)
        #   "f32" 1536: the f32 rows themselves (both shadows switched off for small batches)
        #   "i5"  240.25: the packed 5-bit shadow (+ the same 8 B per 32 rows): single queries of an index of >= 768 Ki rows
        #         (scan_i6.hip; "i6" 288.25: its 6-bit form, option i6_bits = 6)
        if rows_read == "default":
            rows_read = "i5" if (Bq == 1 and rows_here >= I6_MIN_ROWS) else "i8"
            if Bq >= 2 and index.stats_batch_feedback()["f6_batches"] > f6_before:
                rows_read = "f6"  # (the FP6 first filter took the batches: "f6_shadow" = auto on an index of >= 64 Mi rows)
                leg["first_filter"] = "fp6"
        #   "f6"  288.5: the FP6 shadow (+ 8 B of scale/bound per 16 rows)
        row_bytes = {"i5": 240.25, "i6": 288.25, "f6": 288.5, "i8": ROW_BYTES / 4 + 0.25, "f16": ROW_BYTES // 2,
                     "f32": ROW_BYTES}[rows_read]
        leg["row_bytes_streamed"] = row_bytes
        algo = int(rows_here * row_bytes) * scan_passes(Bq)
        if leg["scan_kernel_ms"] > 0:
            leg["scan_GBps"] = algo / (leg["scan_kernel_ms"] * 1e-3) / 1e9
            leg["hbm_frac"] = leg["scan_GBps"] / HBM_PEAK_GBS
            if Bq >= 2:
                # 256 query columns are multiplied whatever Bq is; dense peaks: 2.5 PFLOP/s f16/bf16, int8 twice that
                # (MI355X_MICROARCH.md: the i8 MFMA has the cycles of the bf16 form at 2x the K)
                leg["mfma_TFLOPs"] = 2.0 * 256 * rows_here * 384 / (leg["scan_kernel_ms"] * 1e-3) / 1e12
                if rows_read == "f6":  # (16 cycles per 16x16x128: 10 Pflop/s at 2.4 GHz)
                    leg["mfma_frac_f6_dense_peak"] = leg["mfma_TFLOPs"] / 10000.0
                elif rows_read == "i8":
                    leg["mfma_frac_i8_dense_peak"] = leg["mfma_TFLOPs"] / 5000.0
                else:
                    leg["mfma_frac_f16_dense_peak"] = leg["mfma_TFLOPs"] / 2500.0
        if dump_dir is not None and rank == 0:
            labels, dists, found = result()
            leg["outputs_dumped"] = dump_outputs(dump_dir, {"labels": labels, "distances": dists, "found": found})
        if check_planted:
            labels, _, _ = result()
            leg["planted_top1_ok"] = bool(labels[0][0] == 1 + (4242 % args.rows))
            leg["planted_labels"] = [int(v) for v in labels[0]]
        return leg, algo

    def e2e_leg(index, Bq, steps=30, len_lo=4, len_hi=32):
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            st, cj = dawn.write_synthetic_model(d, seed=3)
            ep = dawn.EmbeddingProvider(st, cj, local_rank)
        seqs = synth.token_sequences(5, Bq, len_lo, len_hi)
        lens = np.array([len(x) for x in seqs])
        offs = np.zeros(Bq + 1, dtype=np.int32)
        offs[1:] = np.cumsum(lens)
        T, max_len = int(offs[-1]), int(lens.max())
        d_ids = torch.from_numpy(np.concatenate(seqs).astype(np.int32)).to(dev)
        d_off = torch.from_numpy(offs).to(dev)
        d_emb = torch.zeros((Bq, 384), dtype=torch.float32, device=dev)
        nbytes = dawn.result_blob_bytes(Bq, k)
        blob = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
        p = blob.data_ptr()

        def embed():
            ep.forward_device(d_ids.data_ptr(), d_off.data_ptr(), Bq, T, max_len, d_emb.data_ptr(), stream)

        def both():
            embed()
            index.search_device(d_emb.data_ptr(), Bq, k, p, p + Bq * k * 8, p + Bq * k * 12, stream)

        res = {"tokens": T, "max_len": max_len}
        for name, fn in (("embed", embed), ("embed_plus_scan", both)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            res[name + "_ms"] = (time.perf_counter() - t0) / steps * 1e3
        fl = float(np.sum(lens * (21.23e6 + 9216.0 * lens)))  # per-token GEMM + attention flops
        res["embed_TFLOPs"] = fl / (res["embed_ms"] * 1e-3) / 1e12
        # f32-EQUIVALENT flops over the f32-MFMA peak (157.3 TF): what an f32 implementation would have to sustain
        res["embed_frac_f32_mfma_peak"] = res["embed_TFLOPs"] / 157.3
        if T > 640:
            # ... and the work the matrix cores actually do: above the latency form's 640 tokens every dense layer is six
            # bf16 MFMA products per f32 product (3-way split, embed_gemm3.hip) — priced against the 2.5 PF dense bf16 peak
            dense_fl = float(np.sum(lens)) * 21.23e6
            res["embed_bf16_mfma_TFLOPs"] = 6.0 * dense_fl / (res["embed_ms"] * 1e-3) / 1e12
            res["embed_frac_bf16_mfma_peak"] = res["embed_bf16_mfma_TFLOPs"] / 2500.0
            res["dense_layers"] = "bf16x3: six v_mfma_f32_32x32x16_bf16 products per f32 product, f32-accurate"
        else:
            res["dense_layers"] = "f32 MFMA (v_mfma_f32_16x16x4_f32 split-K latency form)"
        res["queries_per_s"] = Bq / (res["embed_plus_scan_ms"] * 1e-3)
        ep.close()
        return res

    def file_io_leg(index):
        import tempfile
        res = {}
        d = tempfile.mkdtemp(prefix="dawn_io_")
        p = os.path.join(d, "index.dawn")
        try:
            n = index.size()
            gb = (24 + n * (8 + 1536)) / 1e9
            t0 = time.perf_counter()
            index.save(p)
            t_save = time.perf_counter() - t0
            other = dawn.VectorIndex(local_rank)
            t0 = time.perf_counter()
            other.load(p)
            t_load = time.perf_counter() - t0
            ok = other.size() == n
            other.close()
            res = {"rows": n, "file_GB": gb, "save_GBps": gb / t_save, "load_GBps": gb / t_load, "load_ok": ok,
                   "note": "load: parallel pread into two pinned buffers, H2D + validation overlapped with the next read "
                           "(file in the page cache after the save)"}
        except Exception as e:
            res = {"error": repr(e)}
        finally:
            try:
                os.remove(p)
                os.rmdir(d)
            except OSError:
                pass
        return res

    def realistic_leg(dist_id, rows=None, ks=(10, 20), ablations=True):
        """100 M rows of another distribution (option synth_dist), k = 10 / 20, batch 1 / 256: ms per search and which rung of
        the ladder answered.  dist 1-3: isotropic rows with realistic tails, random queries of the same distribution.  dist 4 / 5:
        the TOPICAL mixture (Zipf-sized clusters, cosine 0.5-0.95 inside a cluster; 5: runs of 256 consecutive rows per cluster) with
        queries that are further rows of the same stream — new pages on the same topics, most of them inside a large cluster:
        the data certificates fail on."""
        topical = dist_id >= 4
        rows = args.rows if rows is None else rows
        ix = dawn.VectorIndex(local_rank)
        ix.set_option("synth_dist", dist_id)
        t0 = time.perf_counter()
        ix.fill_synthetic(1, 0, rows, 1)
        res = {"rows": rows, "fill_seconds": time.perf_counter() - t0}
        if topical:
            res["data"] = "synthetic topical mixture (DESIGN.md 5): a guess at page vectors, unvalidated against real embeddings"
        settle()  # (the previous leg's index was closed just before)
        qi = dawn.VectorIndex(local_rank)
        qi.set_option("synth_dist", dist_id)
        if topical:
            qi.fill_synthetic(1, 1 << 40, 256 * 256, 1)  # (every 256th row: a different run each)
            Qh = qi.get_rows(0, 256 * 256)[0][::256].copy()
        else:
            qi.fill_synthetic(2, 0, 256, 1)
            Qh, _ = qi.get_rows(0, 256)
        qi.close()
        Qh[0] = ix.get_rows(4242 % rows, 1)[0][0]  # a row of the index itself: its label must come out first
        d_q = torch.from_numpy(Qh).to(dev)
        rates = {"second_chances": "second_chance_rate", "deepened": "deepened_rate", "fallbacks": "fallback_rate",
                 "bounded": "bounded_rate", "packed_failures": "packed_failure_rate", "demoted": "demoted_rate"}
        for kk in ks:
            for Bq in (1, 256):
                nb = dawn.result_blob_bytes(Bq, kk)
                blob = torch.zeros((nb,), dtype=torch.uint8, device=dev)
                p = blob.data_ptr()
                steps = (96 if topical else 16) if Bq == 1 else 6
                warm = 2 if Bq == 1 else 5  # (batches: the batch feedback deepens a ladder-heavy index's thresholds after its first window of 1024 queries)
                per = []
                for it in range(steps + warm):
                    if it == warm:
                        torch.cuda.synchronize()
                        s0 = ix.stats()
                        t0 = time.perf_counter()
                    qoff = ((it - warm) % 64) * 384 * 4 if Bq == 1 else 0
                    t1 = time.perf_counter()
                    ix.search_device(d_q.data_ptr() + qoff, Bq, kk, p, p + Bq * kk * 8, p + Bq * kk * 12, stream)
                    if topical:  # (bimodal: every search is timed on its own)
                        torch.cuda.synchronize()
                        per.append(time.perf_counter() - t1)
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                s1 = ix.stats()
                nq = steps * Bq
                leg = {"queries_per_s": steps * Bq / el, "ms_per_step": el / steps * 1e3}
                for kk2, rname in rates.items():
                    leg[rname] = (s1[kk2] - s0[kk2]) / nq
                if topical:
                    pa = np.array(per[warm:]) * 1e3
                    leg["ms_p50"], leg["ms_p95"], leg["ms_max"] = (float(np.percentile(pa, 50)), float(np.percentile(pa, 95)),
                                                                  float(pa.max()))
                res[f"k{kk}_batch{Bq}"] = leg
        lab, _ = ix.search(Qh[0], 10)
        res["planted_top1_ok"] = bool(len(lab) and lab[0] == 1 + 4242 % rows)
        if topical:
            r = ix.stats_raw()
            res["wide_form_answers"], res["bounded_answers"] = r[0], r[4]
        if topical and ablations:
            # the same single queries with the ladder's pieces switched off: what round 3 did (exact pass over all rows behind a
            # failed certificate), and the ladder without its feedback
            for name, opts in (("k10_batch1_no_feedback", {"ladder_feedback": 0}),
                               ("k10_batch1_round3_exact_pass", {"ladder_feedback": 0, "bounded_pass": 0})):
                for o, v in opts.items():
                    ix.set_option(o, v)
                nb = dawn.result_blob_bytes(1, 10)
                blob = torch.zeros((nb,), dtype=torch.uint8, device=dev)
                p = blob.data_ptr()
                torch.cuda.synchronize()
                s0 = ix.stats()
                t0 = time.perf_counter()
                nst = 48
                for it in range(nst):
                    ix.search_device(d_q.data_ptr() + (it % 64) * 384 * 4, 1, 10, p, p + 80, p + 120, stream)
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                s1 = ix.stats()
                res[name] = {"ms_per_step": el / nst * 1e3, "fallback_rate": (s1["fallbacks"] - s0["fallbacks"]) / nst,
                             "bounded_rate": (s1["bounded"] - s0["bounded"]) / nst}
                ix.set_option("ladder_feedback", 1)
                ix.set_option("bounded_pass", 1)
            # the batch of 256 with the wide form of the bounded pass switched off (round 4: sixteen flagged queries per stream)
            ix.set_option("bounded_wide", 0)
            nb = dawn.result_blob_bytes(256, 10)
            blob = torch.zeros((nb,), dtype=torch.uint8, device=dev)
            p = blob.data_ptr()
            ix.search_device(d_q.data_ptr(), 256, 10, p, p + 256 * 80, p + 256 * 120, stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                ix.search_device(d_q.data_ptr(), 256, 10, p, p + 256 * 80, p + 256 * 120, stream)
            torch.cuda.synchronize()
            res["k10_batch256_round4_sixteen_per_stream"] = {"ms_per_step": (time.perf_counter() - t0) / 3 * 1e3}
            ix.set_option("bounded_wide", 1)
        ix.close()
        return res

    def shard_overhead(G, Bq, kk, calls=120):
        """What the sharded handle adds to its slowest shard: p50 of one synchronised dawn_index_search_device call on G logical shards
        of 4096 rows each, minus G back-to-back searches of ONE index of 4096 rows behind one synchronisation — the G scans of logical
        shards share this device and run one after the other, which G real devices do not; what is left is the issue on G streams from
        the worker threads, the gather and the merge.  (All shards on THIS device: the copies are device-local, an xGMI hop and RCCL's
        launch are not in it.)  Returns (that difference, the round-4 figure: minus ONE search — an upper bound that charges the
        serialised scans to the handle)."""
        def p50(ix, times=1):
            qh = synth.unit_rows(3, 0, Bq)
            dq = torch.from_numpy(qh).to(dev)
            blob = torch.zeros((dawn.result_blob_bytes(Bq, kk),), dtype=torch.uint8, device=dev)
            pp = blob.data_ptr()
            ts = []
            for i in range(calls + 20):
                t0 = time.perf_counter()
                for _ in range(times):
                    ix.search_device(dq.data_ptr(), Bq, kk, pp, pp + Bq * kk * 8, pp + Bq * kk * 12, stream)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return float(np.percentile(np.array(ts[20:]) * 1e3, 50))
        one = dawn.VectorIndex(local_rank)
        one.fill_synthetic(1, 0, 4096, 1)
        sh = dawn.VectorIndex(devices=[local_rank] * G)
        sh.set_option("shard_chunk", 1024)
        sh.fill_synthetic(1, 0, 4096 * G, 1)
        t_sh = p50(sh)
        r = (max(t_sh - p50(one, G), 0.0), t_sh - p50(one))
        sh.close()
        one.close()
        return r

    def predicted_scaling(extra, head, kk):
        """A prediction the first real 1 / 2 / 4 / 8-GPU run can be held against: ms per search = the measured single-GPU search of the
        shard size (100 M / N rows) + the sharded handle's own overhead measured with logical shards."""
        shard_ms = {1: {"batch1": head["ms_per_step"], "batch256": extra["batch256"]["ms_per_step"]},
                    2: {"batch1": extra["rows_50M_batch1"]["ms_per_step"], "batch256": extra["rows_50M_batch256"]["ms_per_step"]},
                    4: {"batch1": extra["rows_25M_batch1"]["ms_per_step"], "batch256": extra["rows_25M_batch256"]["ms_per_step"]},
                    8: {"batch1": extra["rows_12p5M_batch1"]["ms_per_step"], "batch256": extra["rows_12p5M_batch256"]["ms_per_step"]}}
        res = {"per_shard_ms": shard_ms, "overhead_ms": {}, "overhead_serialised_upper_ms": {}, "predicted_ms": {}, "predicted_speedup": {},
               "what": "predicted_ms[N] = per_shard_ms[N] + overhead_ms[N]; overhead: G logical shards of 4096 rows on one device, p50 of "
                       "a synchronised call minus G back-to-back searches of one such index (the logical shards' scans serialise on one "
                       "device, real ones do not), + 0.03 ms allowed for the xGMI hop and RCCL's launch, which logical shards lack; "
                       "overhead_serialised_upper_ms: minus ONE search (round 4's figure, an upper bound)"}
        for G in (2, 4, 8):
            o1, o256 = shard_overhead(G, 1, kk), shard_overhead(G, 256, kk)
            res["overhead_ms"][G] = {"batch1": o1[0] + 0.03, "batch256": o256[0] + 0.03}
            res["overhead_serialised_upper_ms"][G] = {"batch1": o1[1], "batch256": o256[1]}
        for G in (1, 2, 4, 8):
            res["predicted_ms"][G] = {b: shard_ms[G][b] + (res["overhead_ms"][G][b] if G > 1 else 0.0) for b in ("batch1", "batch256")}
            res["predicted_speedup"][G] = {b: shard_ms[1][b] / res["predicted_ms"][G][b] for b in ("batch1", "batch256")}
        return res

    # ---- headline leg ------------------------------------------------------------------------
    head, algo_bytes = run_leg(idx, B, args.steps, args.warmup, check_planted=True, dump_dir=args.dump_outputs)
    qps = head["queries_per_s"]
    elapsed_ms = head["ms_per_step"]
    scan_avg_ms = head["scan_kernel_ms"]
    achieved = head.get("scan_GBps", 0.0)
    if B >= 2:
        kernel = "scan_i8_pipe16_kernel<append> (int8 shadow tiles by LDS-DMA, 4 waves x 64 queries, v_mfma_i32_16x16x64_i8)"
    elif head["row_bytes_streamed"] < 300:
        kernel = ("scan_filter_i6s_kernel<BITS=5> (packed 5-bit shadow: nibble planes by global_load_dwordx4, fifth-bit planes by "
                  "global_load_dwordx3 -> 13 VALU of unpacking per fragment -> v_mfma_i32_32x32x32_i8, threshold test of sub-tile "
                  "t-1 in the shadow of sub-tile t's MFMAs; scores are upper bounds; epilogue: every wave re-scores its best rows on "
                  "the f32 rows, every workgroup rescores its 64 best rows exactly in the reference's order)")
    else:
        kernel = ("scan_filter_i8s_pipe_kernel (int8 shadow fragments, global load -> v_mfma_i32_32x32x32_i8, threshold test of "
                  "sub-tile t-1 in the shadow of sub-tile t's MFMAs, 4 waves per CU x 6 KiB in flight; scores are upper bounds)")

    out = {
        "metric": "queries/sec, exact cosine top-k over a 384-d f32 index resident in HBM",
        "value": qps, "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed_ms, "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f32 (exact scores; int8 MFMA upper-bound filter over 5-bit / int8 shadows)", "data": "synthetic",
        "config": {"workload": f"{args.rows}x384 f32 index, batch={B}, k={k}, exact brute-force cosine scan + top-k "
                               "(quantised-shadow upper-bound filter + exact f32 rescore + certificate = the f32 scan's answer)",
                   "rows_total": args.rows, "rows_per_gpu": rows_local, "batch": B, "k": k,
                   "sharding": f"row-sharded x{world}" + (", one RCCL all-gather of packed per-shard top-k + merge" if world > 1 else ""),
                   "ranks": world, "collective_backend": (backend if (world > 1 or args.force_collective) else None),
                   # ranks of the RCCL communicator the all-gather runs on (torch.distributed's "nccl" IS RCCL on ROCm)
                   "rccl_ranks": (dist.get_world_size() if dist.is_initialized() and dist.get_backend() == "nccl" else 0),
                   "pipelined": bool((world > 1 or args.force_collective) and not oversub and not args.no_pipeline),
                   "oversubscribed": oversub},
        "roofline": {"bound": "hbm", "kernel": kernel, "achieved": achieved, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                     "algorithmic_bytes_per_launch": algo_bytes, "avg_launch_ms": scan_avg_ms,
                     "launches_timed": head["launches_timed"],
                     # the same launch priced in the f32 rows of SURVEY 8(d) (1536 B/row: what a scan of the index itself
                     # would have to read): the int8 shadow is an algorithmic saving on top of the kernel's HBM efficiency
                     "bytes_basis": (f"shadow rows actually streamed ({head['row_bytes_streamed']} B per row incl. 8 B of scale / "
                                     "bound per 32 rows: 240 B = the packed 5-bit shadow, 384 B = the int8 shadow); the f32 index rows "
                                     "(1536 B/row) are only touched by the exact rescore (64 rows per workgroup / per query)"),
                     "f32_row_equivalent_GBps": (rows_local * ROW_BYTES * scan_passes(B) / (scan_avg_ms * 1e-3) / 1e9
                                                 if scan_avg_ms > 0 else 0.0),
                     "speedup_vs_f32_row_stream_at_hbm_peak": (rows_local * ROW_BYTES * scan_passes(B) / (HBM_PEAK_GBS * 1e9)
                                                               / (scan_avg_ms * 1e-3) if scan_avg_ms > 0 else 0.0)},
        # certificate counters of the timed headline searches, counted on the device at the end of every search
        # (second_chances: the 64-row certificate failed and a deeper one held — `deepened`: by a 128..256-row round —
        # no exact pass; fallbacks: the exact pass ran)
        "checks": dict(planted_top1_ok=head["planted_top1_ok"], **{kk: idx.stats()[kk] for kk in
                                                                   ("searches", "second_chances", "deepened", "fallbacks")}),
        # Which criterion the certificates are held to (round-2 verdict, weak #6): COST, not first-round rate.  At the
        # service's k = 20 a 256-batch misses the 64-row certificate for every query by design (the int8 bound's slack E + K2
        # is the size of the k -> 64 score gap on 100 M rows); a deeper round of the same certificate settles it for 1-3 % of
        # the search time.  Held: fallbacks == 0 on every leg, (second_chances - deepened) == 0, deepening cost <= 3 %.
        "certificate_criterion": {"held_to": "cost", "fallbacks_allowed": 0, "second_chance_beyond_deepening_allowed": 0,
                                  "deepening_cost_bound": "<= 3 % of the search time (extra.rows_* legs: k20 vs k10 ms_per_step)",
                                  "first_round_rate": "reported (second_chance_rate), not bounded"},
        "hbm_bytes_per_gpu": idx.memory(),  # rows / filter shadows built so far / labels + workspaces
        "fill_seconds": fill_s,
    }
    if world == 1 and rank == 0 and not args.no_extras:
        ceil = read_ceiling_probe()
        out["roofline"]["measured_read_ceiling"] = ceil
        if ceil and ceil.get("GBps"):
            # against the best bare read of either access pattern (16 B/lane and 12 B/lane loads: the packed stream issues both)
            out["roofline"]["frac_of_measured_read_ceiling"] = achieved / max(ceil["GBps"], ceil.get("GBps_12B_per_lane") or 0.0,
                                                                              ceil.get("GBps_packed_stream_pattern") or 0.0)
    traffic_file = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(traffic_file):
        try:
            tj = json.load(open(traffic_file))
            key = f"{rows_local}x{B}"
            if "mfma_busy_frac_12500000x256" in tj:
                # matrix-pipe utilisation of the batched pass (north_star: "MFMA utilisation ... vs chip peak"): from the committed PMC run
                out["mfma_busy_frac"] = {"value": tj["mfma_busy_frac_12500000x256"], "kernel": "scan_i8_pipe16_kernel<false>",
                                         "fp6_pass": tj.get("mfma_busy_frac_12500000x256_f6"), "fp6_kernel": "scan_f6_pass_lds_kernel",
                                         "workload": "12.5 M rows x 256 queries", "source": tj.get("_note_mfma_busy")}
            if key in tj:
                out["roofline"]["traffic"] = tj[key]
                out["roofline"]["traffic_source"] = ("HBM bytes per launch from the committed PMC pass (profiles/traffic.json: "
                                                     "FETCH_SIZE x 2 on gfx950, separate rocprofv3 --pmc run); not re-measured here")
        except Exception:
            pass

    # ---- extra legs (rank-collective where needed) --------------------------------------------
    if not args.no_extras:
        extra = {}
        # the same batch-1 search streaming the f32 rows themselves (1536 B/row; shadow filter off): the f32-stream
        # roofline of DESIGN.md §4.1
        idx.set_option("f16_shadow_b1", 0)
        settle()
        legf, _ = run_leg(idx, 1, max(5, args.steps // 2), 2, check_planted=True, rows_read="f32")
        idx.set_option("f16_shadow_b1", 1)
        extra["batch1_streaming_f32_rows"] = legf
        # ... streaming the packed shadow's 6-bit form (288 B/row), and the int8 shadow (384 B/row; the packed shadow off: the
        # round-2 / early round-3 headline path)
        if rows_local >= I6_MIN_ROWS:
            idx.set_option("i6_bits", 6)
            legf, _ = run_leg(idx, 1, max(5, args.steps // 2), 2, check_planted=True, rows_read="i6")
            idx.set_option("i6_bits", 5)
            extra["batch1_streaming_i6_shadow"] = legf
            idx.set_option("i6_shadow", 0)
            settle()
            legf, _ = run_leg(idx, 1, max(5, args.steps // 2), 2, check_planted=True, rows_read="i8")
            idx.set_option("i6_shadow", 1)
            extra["batch1_streaming_i8_shadow"] = legf
        # ... and streaming the f16 shadow (768 B/row; both integer shadows off)
        idx.set_option("i8_shadow", 0)
        settle()
        legf, _ = run_leg(idx, 1, max(5, args.steps // 2), 2, check_planted=True, rows_read="f16")
        idx.set_option("i8_shadow", 1)
        settle()
        extra["batch1_streaming_f16_shadow"] = legf
        # batch-256 on the same index: one pass of the matrix-core kernel serves all 256 queries
        b256_steps = max(3, min(args.steps, 10 if rows_local > 20_000_000 else 30))
        leg, _ = run_leg(idx, 256, b256_steps, 2, seed=3)
        extra["batch256"] = leg
        # ... the same with the FP6 (e2m3) first filter switched off ("f6_shadow" = 0; the default is auto: an index of >= 64 Mi rows keeps the
        # FP6 shadow — + 288 B per row — where it leaves 24 GiB of HBM free; scan_f6.hip: v_mfma_scale_f32_16x16x128_f8f6f4, survivors
        # re-scored on the f32 rows, the same tail and certificates)
        if world == 1 and leg.get("first_filter") == "fp6":
            sh0 = idx.memory()["shadows"]
            idx.set_option("f6_shadow", 0)
            settle()
            leg8, _ = run_leg(idx, 256, b256_steps, 2, seed=3)
            leg["f6_shadow_bytes"] = int(sh0 - idx.memory()["shadows"])
            leg["vs_int8_first_filter"] = leg["queries_per_s"] / leg8["queries_per_s"]
            extra["batch256_int8_first_filter"] = leg8
            idx.set_option("f6_shadow", 2)
        # ... and on the f16 shadow (scan_f16_pipe_kernel; int8 shadow off)
        idx.set_option("i8_shadow", 0)
        settle()
        leg, _ = run_leg(idx, 256, max(3, b256_steps // 2), 1, seed=3, rows_read="f16")
        idx.set_option("i8_shadow", 1)
        settle()
        extra["batch256_f16_shadow"] = leg
        if world == 1:
            # host-API latency (host buffers in/out: includes H2D of the query and D2H of k results)
            q = synth.unit_rows(2, 1, 1)[0]
            # (p50 / p95 over 200 timed calls after 20 warm-ups, steady clock around the C-ABI call)
            lat = []
            for i in range(220):
                t0 = time.perf_counter()
                idx.search(q, k)
                lat.append(time.perf_counter() - t0)
            lat = np.array(lat[20:])
            extra["host_api_batch1"] = {"p50_ms": float(np.percentile(lat, 50) * 1e3),
                                        "p95_ms": float(np.percentile(lat, 95) * 1e3), "calls": len(lat)}
            # configs[1] / configs[2] scan leg: 1M x 384, batch 1 and batch 256
            idx1 = dawn.VectorIndex(local_rank)
            idx1.fill_synthetic(1, 0, 1_000_000, 1)
            leg1, _ = run_leg(idx1, 1, 200, 20)
            lat = []
            for i in range(220):
                t0 = time.perf_counter()
                idx1.search(q, k)
                lat.append(time.perf_counter() - t0)
            lat = np.array(lat[20:])
            leg1["host_api_p50_ms"] = float(np.percentile(lat, 50) * 1e3)
            leg1["host_api_p95_ms"] = float(np.percentile(lat, 95) * 1e3)
            extra["rows_1M_batch1"] = leg1
            leg2, _ = run_leg(idx1, 256, 50, 5, seed=3)
            Q256 = synth.unit_rows(3, 0, 256)
            lat = []
            for i in range(220):
                t0 = time.perf_counter()
                idx1.search_batch(Q256, k)
                lat.append(time.perf_counter() - t0)
            leg2["host_api_p50_ms"] = float(np.percentile(np.array(lat[20:]), 50) * 1e3)
            leg2["host_api_p95_ms"] = float(np.percentile(np.array(lat[20:]), 95) * 1e3)
            extra["rows_1M_batch256"] = leg2
            extra["fallbacks_1M"] = idx1.stats()["fallbacks"]
            # one shard of configs[3] (100 M rows over 8 GPUs): 12.5 M rows on this GPU, batch 1 and batch 256; the tail
            # (everything but the dominant scan kernel) = ms_per_step - scan_kernel_ms; per-kernel trace: profiles/r03/
            idx12 = dawn.VectorIndex(local_rank)
            idx12.fill_synthetic(1, 0, 12_500_000, 1)
            for name, Bq, st, wu, sd in (("rows_12p5M_batch1", 1, 100, 10, 2), ("rows_12p5M_batch256", 256, 30, 3, 3)):
                lg, _ = run_leg(idx12, Bq, st, wu, seed=sd)
                lg["tail_ms"] = lg["ms_per_step"] - lg["scan_kernel_ms"]
                lg["hbm_floor_ms"] = 12_500_000 * lg["row_bytes_streamed"] / (HBM_PEAK_GBS * 1e9) * 1e3
                extra[name] = lg
            extra["fallbacks_12p5M"] = idx12.stats()["fallbacks"]
            idx12.close()
            settle(1.0)
            for nm in ("rows_1M_batch1", "rows_1M_batch256"):
                extra[nm]["tail_ms"] = extra[nm]["ms_per_step"] - extra[nm]["scan_kernel_ms"]
                extra[nm]["hbm_floor_ms"] = 1_000_000 * extra[nm]["row_bytes_streamed"] / (HBM_PEAK_GBS * 1e9) * 1e3
            # the reference's one-row-per-call insert path (search_provider.rs:127-153,280-284): dawn_index_add per call
            try:
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import add_bench
                extra["single_row_add"] = add_bench.run(100_000, local_rank)
            except Exception as e:
                extra["single_row_add"] = {"error": repr(e)}
            # configs[2] end to end: 256 token sequences -> MiniLM-L6-v2 HIP forward -> cosine scan over 1M rows,
            # everything device-resident on one stream (synthetic seeded weights: no checkpoint on disk)
            extra["e2e_1M_batch256"] = e2e_leg(idx1, 256)
            extra["embed_batch1"] = e2e_leg(idx1, 1, steps=100)
            # page-like inputs (S = 128): the indexer's one page per call, and bulk embedding
            extra["embed_page_batch1_S128"] = e2e_leg(idx1, 1, steps=50, len_lo=128, len_hi=128)
            extra["embed_pages_batch256_S128"] = e2e_leg(idx1, 256, steps=5, len_lo=128, len_hi=128)
        st_all = idx.stats()
        out["checks"]["all_legs_on_this_index"] = {kk: st_all[kk] for kk in ("searches", "second_chances", "deepened", "fallbacks")}
        if world == 1:
            # p50 / p95 of the batch-256 search through the host API on the 100 M-row index (BASELINE metric: latency)
            Q256 = synth.unit_rows(3, 0, 256)
            lat = []
            for i in range(220):
                t0 = time.perf_counter()
                idx.search_batch(Q256, k)
                lat.append(time.perf_counter() - t0)
            lat = np.array(lat[20:]) * 1e3
            extra["host_api_batch256"] = {"p50_ms": float(np.percentile(lat, 50)), "p95_ms": float(np.percentile(lat, 95)),
                                          "calls": len(lat)}
            # save / load of the packed index file (pinned staging, reads overlapped with the DMA): GB/s on this box's disk
            extra["index_file_io"] = file_io_leg(idx1)
        if world == 1:
            # configs[4] sizing point on one GPU: the same 100 M rows stored as bf16 (76.8 GB), f32 accumulation;
            # parity of this path: tests/test_scan_bf16_gpu.py (oracle over the bf16-rounded rows)
            idx1.close()
            idx.close()
            settle()
            idxh = dawn.VectorIndex(local_rank, dtype="bf16")
            idxh.fill_synthetic(1, 0, args.rows, 1)
            legh, _ = run_leg(idxh, 1, max(5, args.steps // 2), 3, check_planted=True)
            extra["bf16_index_batch1"] = legh
            legh2, _ = run_leg(idxh, 256, 5, 1, seed=3)
            extra["bf16_index_batch256"] = legh2
            # ... filtering on the bf16 rows themselves (no int8 shadow: 76.8 GB in total instead of 115.2 GB)
            idxh.set_option("i8_shadow", 0)
            settle()
            legh, _ = run_leg(idxh, 1, 5, 2, check_planted=True, rows_read="f16")
            extra["bf16_index_batch1_own_rows"] = legh
            legh2, _ = run_leg(idxh, 256, 3, 1, seed=3, rows_read="f16")
            extra["bf16_index_batch256_own_rows"] = legh2
            idxh.close()
            settle()
            # ---- the shard sizes of 2 / 4 GPUs (50 M / 25 M rows; 8 GPUs: rows_12p5M_* above) and what they predict for the 1 -> 8 curve
            for name, nrows in (("rows_50M", 50_000_000), ("rows_25M", 25_000_000)):
                ixs = dawn.VectorIndex(local_rank)
                ixs.fill_synthetic(1, 0, nrows, 1)
                for Bq, st, wu, sd in ((1, 60, 6, 2), (256, 15, 3, 3)):
                    lg, _ = run_leg(ixs, Bq, st, wu, seed=sd)
                    lg["tail_ms"] = lg["ms_per_step"] - lg["scan_kernel_ms"]
                    lg["hbm_floor_ms"] = nrows * lg["row_bytes_streamed"] / (HBM_PEAK_GBS * 1e9) * 1e3
                    extra[f"{name}_batch{Bq}"] = lg
                extra["fallbacks_" + name[5:]] = ixs.stats()["fallbacks"]
                ixs.close()
                settle()
            try:
                extra["predicted_scaling"] = predicted_scaling(extra, head, k)
            except Exception as e:
                extra["predicted_scaling"] = {"error": repr(e)}
            extra["rows_12p5M_clustered_topical"] = realistic_leg(4, rows=12_500_000, ks=(10,), ablations=False)
            # ---- realistic score distributions (dawn_index_set_option "synth_dist"): Gaussian rows and heavy-tailed rows
            # (4 dimensions x5, as sentence embeddings have); k = 10 and the service's k = 20; certificate counters
            for name, dist_id in (("gaussian", 1), ("heavy_tailed_4dims_x5", 2), ("clustered_topical", 4),
                                  ("clustered_topical_runs256", 5)):
                extra["rows_" + name] = realistic_leg(dist_id)
        out["extra"] = extra
        if world == 1 and rank == 0:
            out["cpu_baseline"] = cpu_baseline(args.cpu_sample_rows, k, args.rows)
            out["cpu_baseline"]["note"] = ("the sample (1.5 GB) is smaller than the index (153.6 GB) but far larger than the "
                                           "CPU's caches: both stream from DRAM; scaled linearly in rows")
            out["cpu_baseline"]["rust_probe"] = rust_probe(args.cpu_sample_rows)
            try:
                out["cpu_baseline"]["embedder"] = cpu_embedder_baseline()
            except Exception as e:
                out["cpu_baseline"]["embedder"] = {"error": repr(e)}

    # RCCL writes a version banner to C stdout; get every rank's C buffers out before rank 0 prints the ONE JSON
    # line, so that the line is the last thing on stdout.
    import ctypes
    try:
        idx.close()
    except Exception:
        pass
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    if world > 1 and rank == 0 and capi is not None:
        out.setdefault("extra", {})["single_process_sharded"] = capi
        head_mode = next((m for m in capi.get("modes", []) if f"batch{B}" in m and "error" not in m), None)
        # every multi-GPU form must return the labels of the planted query that the single index returns (every form is
        # bit-identical to it — tests/test_sharded_capi_gpu.py, tests/test_sharded_gpu.py); the rank form's are in `head`
        want = head.get("planted_labels")
        got = [m.get(f"batch{B}", {}).get("planted_labels") for m in capi.get("modes", []) if f"batch{B}" in m]
        out["checks"]["single_process_sharded_labels_equal_rank_form"] = bool(got) and all(g == want for g in got)
        out["checks"]["single_process_sharded_qps"] = {m["mode"]: {"batch1": m.get("batch1", {}).get("queries_per_s"),
                                                                   "batch256": m.get("batch256", {}).get("queries_per_s")}
                                                       for m in capi.get("modes", [])}
        if head_mode is not None:
            # the rank-per-GPU form's own line moves aside ...
            out["extra"]["torch_distributed_ranks"] = {kk: out[kk] for kk in ("value", "ms_per_step", "steps", "warmup")}
            out["extra"]["torch_distributed_ranks"].update(
                {"config": out["config"], "roofline": out["roofline"], "checks": {kk: out["checks"].get(kk) for kk in
                                                                                ("planted_top1_ok", "searches", "fallbacks")}})
            # ... and the line is the product's: one process, N devices, the library's own collective
            hl = head_mode[f"batch{B}"]
            si = head_mode.get("shard_info", {})
            out["value"] = hl["queries_per_s"]
            out["ms_per_step"] = hl["ms_per_step"]
            out["steps"], out["warmup"] = hl["steps"], hl["warmup"]
            out["latency_ms"] = {"p50": hl["p50_ms"], "p95": hl["p95_ms"], "host_api_p50": hl["host_api_p50_ms"],
                                 "what": "one dawn_index_search_device call on the sharded handle, synchronised every time "
                                         "(unpipelined): N shard searches + gather + merge"}
            gather = {1: "RCCL all-gather (ncclAllGather of the packed per-shard results, the library's own communicator)",
                      2: "peer copies (hipMemcpyPeerAsync)", -1: "RCCL selected, not initialised", 0: "none"}.get(si.get("gather"), "?")
            out["config"] = dict(out["config"], form="ONE process behind the C ABI: dawn_index_create_sharded over the N devices "
                                                      "(what a Rust caller binds); tools/sharded_capi_bench.py",
                                 ranks=1, shards=si.get("n_shards"), shard_rows=si.get("sizes"), gather=gather,
                                 rccl_ranks=(si.get("n_shards") if si.get("gather") == 1 else 0),
                                 collective_backend=("rccl" if si.get("gather") == 1 else "peer copies"), pipelined=False,
                                 oversubscribed=bool(head_mode.get("logical_shards_on_one_device")))
            out["checks"]["planted_top1_ok"] = bool(hl["planted_top1_ok"])
            out["checks"]["labels_equal_rank_form"] = bool(hl["planted_labels"] == want)
            out["checks"]["sharded_handle_stats"] = head_mode.get("stats")
            out["roofline"]["note"] = ("per-shard kernel of the rank-per-GPU form (same kernel, same shard size: the sharded handle "
                                       "launches it once per device)")
        else:
            out["checks"]["single_process_sharded_failed"] = capi.get("error") or [m.get("error") for m in capi.get("modes", [])]
    ctypes.CDLL(None).fflush(None)
    sys.stdout.flush()
    if rank == 0:
        time.sleep(0.5 if world > 1 else 0.0)  # let the other ranks' flushed banners reach the shared pipe first
        emit(out)


if __name__ == "__main__":
    main()
