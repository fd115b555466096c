"""Rows by label: dawn_index_get, dawn_index_search_like and dawn_index_search_like_device (index_lookup.hip).

The semantics under test (include/dawn_hip.h): for a label L, count(L) is the number of rows holding L, and the row of L is the
earliest-added row holding it.  Every expectation comes from numpy on the labels as added: the rows must be byte for byte what
get_rows returns at the expected position, search_like must give the bits of the CPU oracle on those rows and of search_batch
on the vectors get returned, and a missing label gives a zero row, count 0 and found 0.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dawnsearch_amd import synth  # noqa: E402

U64MAX = 2**64 - 1


@functools.lru_cache(maxsize=4)
def _rows(n):
    from oracle import oracle_lib
    return oracle_lib.unit_rows(1, 0, n)


def _same(lab, dist, olab, odist):
    assert np.array_equal(lab, olab), (lab, olab)
    assert np.array_equal(np.asarray(dist).view(np.uint32), np.asarray(odist).view(np.uint32)), (dist, odist)


def _index(dawn, x, ids, dtype="f32", opts=None):
    idx = dawn.VectorIndex(0, dtype=dtype)
    for k, v in (opts or {}).items():
        idx.set_option(k, v)
    if len(ids):
        idx.add_batch(np.asarray(ids, dtype=np.uint64), x)
    return idx


def _expect(ids, probes):
    """numpy on the labels: (first position or -1, count) per probe."""
    ids = np.asarray(ids, dtype=np.uint64)
    uniq, first, counts = np.unique(ids, return_index=True, return_counts=True)
    probes = np.asarray(probes, dtype=np.uint64)
    at = np.searchsorted(uniq, probes)
    hit = (at < len(uniq)) & (uniq[np.minimum(at, len(uniq) - 1)] == probes) if len(uniq) else np.zeros(len(probes), bool)
    pos = np.where(hit, first[np.minimum(at, max(len(uniq) - 1, 0))] if len(uniq) else 0, -1)
    cnt = np.where(hit, counts[np.minimum(at, max(len(uniq) - 1, 0))] if len(uniq) else 0, 0)
    return pos.astype(np.int64), cnt.astype(np.int64)


def _check_get(idx, ids, probes):
    rows, counts = idx.get(probes)
    pos, cnt = _expect(ids, probes)
    assert np.array_equal(counts, cnt), (counts, cnt)
    by_pos = {}
    for b, p in enumerate(pos):
        if p < 0:
            assert not rows[b].any(), b  # a missing label: zeros
            continue
        if p not in by_pos:
            by_pos[p] = idx.get_rows(int(p), 1)[0][0]
        assert np.array_equal(rows[b].view(np.uint32), by_pos[p].view(np.uint32)), (b, p)
    return rows, counts


def _labels(n):
    """1..n with a label held by two rows, one held by many, 2**64-1 and 0 present (from 31 rows)."""
    ids = np.arange(1, n + 1, dtype=np.uint64)
    if n >= 3:
        ids[n // 2] = ids[n // 3]
    if n >= 31:
        ids[1] = U64MAX
        ids[-1] = 0
        many = np.arange(n // 4, n, max(1, n // 20))[:16]  # 16 rows spread over the index: label 7
        ids[many] = 7
    return ids


def _probes(n, ids, m):
    rng = np.random.default_rng(n + m)
    present = ids[rng.integers(0, n, size=max(1, m - 12))]
    extra = [0, U64MAX, n + 5, 10**15, 2**63, ids[0], ids[0], ids[n // 3], 7, ids[-1], n + 5, ids[n // 2]]
    p = np.concatenate([present, np.asarray(extra, dtype=np.uint64)])
    rng.shuffle(p)
    return p


# 1. get across sizes, f32 and bf16
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 8191, 8193, 300_001])
def test_get_sizes(dawn, n, dtype):
    x = _rows(n)
    ids = _labels(n)
    idx = _index(dawn, x, ids, dtype)
    m = 40 if n < 8191 else 300  # (300: more than one lookup launch)
    _check_get(idx, ids, _probes(n, ids, m))
    # the rows are the stored ones: the input rows (f32) or their bf16 rounding
    pos, _ = _expect(ids, ids[:1])
    rows, _ = idx.get(ids[:1])
    want = x[pos[0]] if dtype == "f32" else synth.round_bf16(x[pos[0]:pos[0] + 1])[0]
    assert np.array_equal(rows[0].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_get_at_scale(dawn, oracle, dtype):
    n = 12_500_000
    idx = dawn.VectorIndex(0, dtype=dtype)
    idx.fill_synthetic(1, 0, n, 1)
    rng = np.random.default_rng(3)
    probes = np.concatenate([rng.integers(1, n + 1, size=290).astype(np.uint64),
                             np.asarray([1, n, n // 2, 0, n + 1, U64MAX, 1, n, 2**40, 5], dtype=np.uint64)])
    rows, counts = idx.get(probes)
    ok = (probes >= 1) & (probes <= n)
    assert np.array_equal(counts, ok.astype(np.int64))
    assert not rows[~ok].any()
    for b in np.flatnonzero(ok)[::7]:
        want = oracle.unit_rows(1, int(probes[b]) - 1, 1)
        if dtype == "bf16":
            want = synth.round_bf16(want)
        assert np.array_equal(rows[b].view(np.uint32), want[0].view(np.uint32)), b
    # counts only: the lookup alone, no gather
    from dawnsearch_amd import _lib
    c2 = np.zeros(len(probes), dtype=np.uintp)
    assert _lib.lib.dawn_index_get(idx._h, len(probes), probes.ctypes.data, None, c2.ctypes.data) == 0
    assert np.array_equal(c2.astype(np.int64), counts)


# 2. label orders and one label everywhere
@pytest.mark.parametrize("order", ["reversed", "shuffled"])
def test_get_unsorted_labels(dawn, order):
    n = 100_003
    x = _rows(n)
    ids = np.arange(1, n + 1, dtype=np.uint64)[::-1].copy()
    if order == "shuffled":
        np.random.default_rng(1).shuffle(ids)
    ids[5000:5010] = ids[60_000]  # ... and a label held by 11 rows, the earliest at position 5000
    idx = _index(dawn, x, ids)
    _check_get(idx, ids, _probes(n, ids, 280))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_get_one_label_everywhere(dawn, oracle, dtype):
    n = 300_001
    x = _rows(n)
    ids = np.full(n, 42, dtype=np.uint64)
    idx = _index(dawn, x, ids, dtype)
    rows, counts = _check_get(idx, ids, [42, 41, 42, 0, U64MAX])
    assert counts.tolist() == [n, 0, n, 0, 0]
    lab, dist, found = idx.search_like([42, 43], 10)
    q = rows[0]
    xe = synth.round_bf16(x) if dtype == "bf16" else x
    assert found.tolist() == [10, 0]
    _same(lab[0], dist[0], *oracle.scan_topk(xe, ids, q, 10, threads=8))


# 3. after mutations
def test_get_after_remove(dawn):
    n = 5000
    x = _rows(n)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    ids[[100, 900, 4000]] = 77  # label 77: rows 76, 100, 900, 4000 — the earliest is 76
    idx = _index(dawn, x, ids)
    _check_get(idx, ids, [77, 1, n])
    idx.remove([77])
    keep = ids != 77
    _check_get(idx, ids[keep], [77, 1, n, 78])
    # remove the earliest of several rows holding a label: the next one becomes the row of the label
    ids2 = np.arange(1, n + 1, dtype=np.uint64)
    ids2[[10, 20, 30]] = 5011  # a label of three rows
    idx2 = _index(dawn, x, ids2)
    rows, counts = idx2.get([5011])
    assert counts[0] == 3 and np.array_equal(rows[0].view(np.uint32), x[10].view(np.uint32))
    # the earliest holder leaves (remove takes every row of a label: re-add the two later ones): the next one is the row
    idx2.remove([5011])
    idx2.add_batch(np.asarray([5011, 5011], dtype=np.uint64), x[[20, 30]])
    rows, counts = idx2.get([5011, 21])
    assert counts.tolist() == [2, 0]
    assert np.array_equal(rows[0].view(np.uint32), x[20].view(np.uint32))
    # rows move under a label held by two rows: label 41 at rows 40 and 41, row 39 (label 9999) removed
    ids3 = np.arange(1, n + 1, dtype=np.uint64)
    ids3[41] = 41
    ids3[39] = 9999
    idx3 = _index(dawn, x, ids3)
    idx3.remove([9999])
    keep = ids3 != 9999
    _check_get(idx3, ids3[keep], [41, 9999, 1, 40])


def test_get_staged_adds(dawn, oracle):
    n = 3000
    x = _rows(n)
    idx = dawn.VectorIndex(0)
    idx.add_batch(np.arange(1, 2001, dtype=np.uint64), x[:2000])
    for i in range(2000, 2500):  # staged on the host, not yet on the device
        idx.add(i + 1, x[i])
    idx.add(3, x[2600])  # a second row for label 3, staged
    rows, counts = idx.get([2100, 2500, 3, 2501])
    assert counts.tolist() == [1, 1, 2, 0]
    for b, r in ((0, 2099), (1, 2499), (2, 2)):
        assert np.array_equal(rows[b].view(np.uint32), x[r].view(np.uint32))
    for i in range(2500, 2510):
        idx.add(i + 1, x[i])
    lab, dist, found = idx.search_like([2505, 1], 10)  # (the staged row is searched with)
    ids = np.concatenate([np.arange(1, 2501), [3], np.arange(2501, 2511)]).astype(np.uint64)
    xs = np.concatenate([x[:2500], x[2600:2601], x[2500:2510]])
    assert found.tolist() == [10, 10]
    _same(lab[0], dist[0], *oracle.scan_topk(xs, ids, x[2504], 10))
    _same(lab[1], dist[1], *oracle.scan_topk(xs, ids, x[0], 10))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_get_after_save_load(dawn, tmp_path, dtype):
    n = 8193
    x = _rows(n)
    ids = _labels(n)
    idx = _index(dawn, x, ids, dtype)
    p = str(tmp_path / "a.idx")
    idx.save(p)
    back = dawn.VectorIndex(0, dtype=dtype)
    back.load(p)
    probes = _probes(n, ids, 100)
    r1, c1 = _check_get(back, ids, probes)
    r0, c0 = idx.get(probes)
    assert np.array_equal(c0, c1) and np.array_equal(r0.view(np.uint32), r1.view(np.uint32))


def test_get_after_load_page_entries(dawn, tmp_path):
    n = 777
    rows = synth.unit_rows(6, 0, n)
    rec = np.zeros((n, 1568), dtype=np.uint8)
    rec[:, 16:16 + 1536] = rows.view(np.uint8).reshape(n, 1536)
    p = str(tmp_path / "x.warc.emb")
    rec.tofile(p)
    idx = dawn.VectorIndex(0)
    idx.load_page_entries(p, first_id=1000)
    got, counts = idx.get([1000, 1776, 999, 1777, 1400])
    assert counts.tolist() == [1, 1, 0, 0, 1]
    for b, r in ((0, 0), (1, n - 1), (4, 400)):
        assert np.array_equal(got[b].view(np.uint32), rows[r].view(np.uint32))
    lab, dist, found = idx.search_like([1400], 5)
    assert found[0] == 5 and lab[0][0] == 1400


# 4. search_like: bit-identical to the oracle and to search_batch on the rows get returned
def _check_like(idx, ids_all, xe, probes, k, oracle, ref_cache=None):
    lab, dist, found = idx.search_like(probes, k)
    rows, counts = idx.get(probes)
    present = counts > 0
    assert np.array_equal(found[~present], np.zeros(int((~present).sum()), dtype=np.int64))
    if present.any():
        sl, sd, sf = idx.search_batch(rows[present], k)
        assert np.array_equal(sf, found[present])
        for i, b in enumerate(np.flatnonzero(present)):
            f = found[b]
            _same(lab[b][:f], dist[b][:f], sl[i][:f], sd[i][:f])
            key = rows[b].tobytes()
            if ref_cache is not None and key in ref_cache:
                ol, od = ref_cache[key]
            else:
                ol, od = oracle.scan_topk(xe, ids_all, rows[b], 64, threads=8)
                if ref_cache is not None:
                    ref_cache[key] = (ol, od)
            assert f == min(k, len(ol))
            _same(lab[b][:f], dist[b][:f], ol[:k], od[:k])
    return lab, dist, found


_LIKE_CACHE = {}


@pytest.mark.parametrize("k", [1, 10, 20, 64])
@pytest.mark.parametrize("B", [1, 7, 256, 300])
def test_search_like_batches(dawn, oracle, B, k):
    n = 20_000
    x = _rows(n)
    ids = _labels(n)
    idx = _index(dawn, x, ids)
    rng = np.random.default_rng(B)
    probes = ids[rng.integers(0, n, size=B)]
    if B >= 7:
        probes[3] = n + 99  # a missing label
        probes[5] = probes[4]  # a repeat
    _check_like(idx, ids, x, probes, k, oracle, _LIKE_CACHE)


_PATHS = {
    "packed5": {"i6_min_rows": 0},
    "packed6": {"i6_min_rows": 0, "i6_bits": 6},
    "int8": {"i6_shadow": 0},
    "f16": {"i8_shadow": 0},
    "fp6": {"f6_shadow": 1, "f6_min_rows": 0},
    "ladder": {"force_fallback": 2},
}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("path", list(_PATHS))
def test_search_like_paths(dawn, oracle, dtype, path):
    n = 10_000  # (more rows than the candidate slots of a batched pass: the FP6 filter runs)
    x = _rows(n)
    ids = _labels(n)
    idx = _index(dawn, x, ids, dtype, _PATHS[path])
    xe = synth.round_bf16(x) if dtype == "bf16" else x
    probes = np.concatenate([ids[[0, 5, 100, 2048, 9999]], np.asarray([7, n + 3], dtype=np.uint64)])
    for B, k in ((1, 10), (7, 10), (7, 64)):  # (1: the single-query stream; 7: the batched passes)
        _check_like(idx, ids, xe, probes[:B] if B > 1 else probes[2:3], k, oracle)
    probes16 = np.concatenate([probes, ids[np.arange(9) * 400 + 3]])
    _check_like(idx, ids, xe, probes16, 20, oracle)


def test_search_like_ladder_topical(dawn, oracle):
    """Topical rows (clusters of near-ties), every certificate failing: the bounded pass answers the looked-up queries."""
    n = 50_000
    x = oracle.unit_rows_topical(1, 0, n)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    probes = ids[np.linspace(0, n - 1, 16).astype(int)]
    for opts in ({"force_fallback": 2}, {"force_fallback": 2, "i6_min_rows": 0}):
        idx = _index(dawn, x, ids, "f32", opts)
        for B in (1, 16):
            _check_like(idx, ids, x, probes[:B], 10, oracle)


def test_search_like_exploring_marker(dawn):
    """web.rs:339: on an index with unique labels, the page itself comes first, at a distance below 0.001."""
    for dtype in ("f32", "bf16"):
        n = 30_000
        idx = _index(dawn, _rows(n), np.arange(1, n + 1, dtype=np.uint64), dtype)
        probes = np.asarray([1, 2, 777, 15_000, n], dtype=np.uint64)
        lab, dist, found = idx.search_like(probes, 20)
        assert (found == 20).all()
        assert np.array_equal(lab[:, 0], probes)
        # (a bf16 row's own distance is 1 - |bf16(x)|^2: its rounding moves the norm a little)
        assert (dist[:, 0] < (0.001 if dtype == "f32" else 0.01)).all(), dist[:, 0]


def test_search_like_bf16_norm_edge(dawn, oracle):
    """A bf16 row whose widened norm falls outside (0.99, 1.01) is still searched, and answered exactly."""
    n = 2000
    x = _rows(n).copy()
    e = np.zeros(384, dtype=np.float32)
    e[17] = np.float32(0.9901)  # passes the f32 gate; bf16 rounds it to 0.98828125
    x[500] = e
    ids = np.arange(1, n + 1, dtype=np.uint64)
    idx = _index(dawn, x, ids, "bf16")
    rows, counts = idx.get([501])
    norm = float(np.sqrt(np.sum(rows[0].astype(np.float64) ** 2)))
    assert counts[0] == 1 and not (0.99 < norm < 1.01), norm
    with pytest.raises(Exception):
        idx.search_batch(rows, 10)  # (the gate search_batch applies to caller queries)
    xe = synth.round_bf16(x)
    for B, k in ((1, 10), (3, 64)):
        lab, dist, found = idx.search_like(np.asarray([501, 2, 3][:B], dtype=np.uint64), k)
        assert found[0] == k
        _same(lab[0], dist[0], *oracle.scan_topk(xe, ids, rows[0], k))


# 5. the device form, captured into a hipGraph
def test_search_like_device_graph_replay(dawn):
    torch = pytest.importorskip("torch")
    n = 20_000
    x = _rows(n)
    ids = _labels(n)
    idx = _index(dawn, x, ids)
    B, k = 8, 10
    batches = [np.asarray([1, 2, n + 7, 7, ids[n // 2], 9000, 2, U64MAX], dtype=np.uint64),
               np.asarray([0, 19_000, 3, 4, 5, 10**12, 6, 7], dtype=np.uint64),
               np.asarray([500] * 8, dtype=np.uint64)]
    dev = torch.device("cuda", 0)
    d_ids = torch.zeros((B,), dtype=torch.int64, device=dev)
    lab = torch.zeros((B, k), dtype=torch.int64, device=dev)
    dist = torch.zeros((B, k), dtype=torch.float32, device=dev)
    fnd = torch.zeros((B,), dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    d_ids.copy_(torch.from_numpy(batches[0].view(np.int64)))
    with torch.cuda.stream(side):  # warm-up on the capture stream
        idx.search_like_device(d_ids.data_ptr(), B, k, lab.data_ptr(), dist.data_ptr(), fnd.data_ptr(), side.cuda_stream)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        idx.search_like_device(d_ids.data_ptr(), B, k, lab.data_ptr(), dist.data_ptr(), fnd.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    for probes in batches + batches[:1]:
        d_ids.copy_(torch.from_numpy(probes.view(np.int64)))
        g.replay()
        torch.cuda.synchronize()
        L, D, F = lab.cpu().numpy().view(np.uint64), dist.cpu().numpy(), fnd.cpu().numpy()
        hl, hd, hf = idx.search_like(probes, k)
        assert np.array_equal(F.astype(np.int64), hf)
        _same(L, D, hl, hd)
        _, counts = idx.get(probes)
        assert np.array_equal(F > 0, counts > 0)


# 6. sharded handles
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sharded_equals_single(dawn, dtype):
    from dawnsearch_amd import _lib
    n = 10_000
    x = _rows(n)
    ids = _labels(n)
    single = _index(dawn, x, ids, dtype)
    sh = dawn.VectorIndex(devices=[0, 0, 0], dtype=dtype)
    sh.set_option("shard_chunk", 1024)
    sh.add_batch(ids, x)
    assert sh.shard_info()["n_shards"] == 3
    probes = _probes(n, ids, 300)
    r1, c1 = sh.get(probes)
    r0, c0 = _check_get(single, ids, probes)
    assert np.array_equal(c1, c0) and np.array_equal(r1.view(np.uint32), r0.view(np.uint32))
    for k in (1, 10, 64):
        a = sh.search_like(probes[:40], k)
        e = single.search_like(probes[:40], k)
        assert np.array_equal(a[2], e[2])
        for b in range(40):
            _same(a[0][b][:e[2][b]], a[1][b][:e[2][b]], e[0][b][:e[2][b]], e[1][b][:e[2][b]])
    with pytest.raises(_lib.DawnError) as err:
        sh.search_like_device(1 << 20, 1, 10, 1 << 20, 1 << 20, 1 << 20)  # (refused before any pointer is used)
    assert err.value.code == _lib.ERR_UNSUPPORTED


# 7. errors and empty cases
def test_lookup_errors(dawn, oracle):
    from dawnsearch_amd import _lib
    L = _lib.lib
    n = 5000
    x = _rows(n)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    idx = _index(dawn, x, ids)
    q = x[10]
    l0, d0 = idx.search(q, 10)
    probe = np.asarray([5], dtype=np.uint64)
    out = np.zeros((1, 384), dtype=np.float32)
    cnt_a = np.zeros(1, dtype=np.uintp)
    cnt = cnt_a.ctypes.data
    labels = np.zeros(64, dtype=np.uint64)
    dist = np.zeros(64, dtype=np.float32)
    found_a = np.zeros(1, dtype=np.uintp)
    found = found_a.ctypes.data
    p = probe.ctypes.data
    assert L.dawn_index_get(None, 1, p, out.ctypes.data, cnt) == _lib.ERR_INVALID_ARG
    assert L.dawn_index_get(idx._h, 1, None, out.ctypes.data, cnt) == _lib.ERR_INVALID_ARG
    assert L.dawn_index_get(idx._h, 1, p, None, None) == 0  # (nothing wanted: not an error)
    assert L.dawn_index_get(idx._h, 0, p, None, None) == 0
    assert L.dawn_index_search_like(idx._h, 1, None, 10, labels.ctypes.data, dist.ctypes.data, found) == _lib.ERR_INVALID_ARG
    assert L.dawn_index_search_like(idx._h, 1, p, 10, None, dist.ctypes.data, found) == _lib.ERR_INVALID_ARG
    assert L.dawn_index_search_like(idx._h, 1, p, 10, labels.ctypes.data, None, found) == _lib.ERR_INVALID_ARG
    assert L.dawn_index_search_like(idx._h, 1, p, 10, labels.ctypes.data, dist.ctypes.data, None) == _lib.ERR_INVALID_ARG
    assert L.dawn_index_search_like(idx._h, 0, p, 10, None, None, None) == 0
    for k in (0, 65):
        assert L.dawn_index_search_like(idx._h, 1, p, k, labels.ctypes.data, dist.ctypes.data, found) == _lib.ERR_UNSUPPORTED
        assert L.dawn_index_search_like_device(idx._h, 1 << 20, 1, k, 1 << 20, 1 << 20, 1 << 20, None) == _lib.ERR_UNSUPPORTED
    assert L.dawn_index_search_like_device(idx._h, None, 1, 10, 1 << 20, 1 << 20, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert L.dawn_index_search_like_device(idx._h, 1 << 20, 1, 10, None, 1 << 20, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert L.dawn_index_search_like_device(idx._h, 1 << 20, 0, 10, 1 << 20, 1 << 20, 1 << 20, None) == 0
    # the index is unchanged
    assert idx.size() == n
    l1, d1 = idx.search(q, 10)
    _same(l1, d1, l0, d0)
    _same(l1, d1, *oracle.scan_topk(x, ids, q, 10))
    _check_get(idx, ids, [1, 5, n, n + 1])
    # an empty index: every label is missing
    empty = dawn.VectorIndex(0)
    rows, counts = empty.get([1, 0, U64MAX])
    assert counts.tolist() == [0, 0, 0] and not rows.any()
    lab, dist, found = empty.search_like([1, 2], 10)
    assert found.tolist() == [0, 0]
    sh = dawn.VectorIndex(devices=[0, 0])
    rows, counts = sh.get([1])
    assert counts.tolist() == [0] and not rows.any()
    assert sh.search_like([1], 5)[2].tolist() == [0]
