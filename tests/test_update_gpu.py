"""dawn_index_update: rows replaced in place by label on the GPU (index_update.hip).

The property under test (include/dawn_hip.h): after an update the index IS the index built by adding the same rows, in the same
order, with the new vectors in place of the old — rows, labels, the filter shadows, search results and save files.  Every check
is bit-exact: search results against the CPU oracle (oracle.scan_topk over the updated rows), everything else against a fresh
index built from the updated rows.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dawnsearch_amd import synth  # noqa: E402

U64MAX = np.uint64(2**64 - 1)


@functools.lru_cache(maxsize=4)
def _rows(n):
    from oracle import oracle_lib
    return oracle_lib.unit_rows(1, 0, n)


def _new_rows(m, seed=77):
    from oracle import oracle_lib
    return np.ascontiguousarray(oracle_lib.unit_rows(seed, 0, m), dtype=np.float32)


def _patterns(n):
    """name -> row positions whose label is updated (ids are 1..n unless the pattern relabels)."""
    rng = np.random.default_rng(n)
    p = {
        "row0": [0],
        "last": [n - 1],
        "mid_subtile": [min(n - 1, 32 + 17)],
        "every_other": list(range(0, n, 2)),
        "random10": sorted(rng.choice(n, size=max(1, n // 10), replace=False).tolist()),
        "all": list(range(n)),
        "absent": [],
    }
    if n >= 64:
        p["block32"] = list(range(32, 64))  # one aligned sub-tile: all 32 of its rows
    if n >= 3:
        p["dup"] = [n // 3]  # its label is also held by row n // 2
    return p


def _make_ids(n, pattern):
    ids = np.arange(1, n + 1, dtype=np.uint64)
    if pattern == "dup":
        ids[n // 2] = ids[n // 3]
    return ids


def _index(dawn, dtype, opts, x, ids):
    idx = dawn.VectorIndex(0, dtype=dtype)
    for k, v in opts.items():
        idx.set_option(k, v)
    if len(ids):
        idx.add_batch(ids, x)
    return idx


def _same(lab, dist, olab, odist):
    assert np.array_equal(lab, olab), (lab, olab)
    assert np.array_equal(np.asarray(dist).view(np.uint32), np.asarray(odist).view(np.uint32)), (dist, odist)


def _queries(x, extra=()):
    """Queries planted near rows spread over the index, the new vectors themselves (their rows must come first) and a few
    uniform ones."""
    n = x.shape[0]
    picks = np.linspace(0, n - 1, num=min(8, n)).astype(np.int64)
    Q = [synth.planted_queries(1, [int(p)], 100 + i)[0] for i, p in enumerate(picks)]
    Q += [np.asarray(e, dtype=np.float32) for e in list(extra)[:6]]
    Q += list(synth.unit_rows(9, 0, 16 - len(Q)))
    return np.ascontiguousarray(np.stack(Q), dtype=np.float32)


def _check(dawn, oracle, idx, fresh, xu, ids, Q, dtype, batch256=True, f6=False):
    n = len(ids)
    assert idx.size() == n
    rows, got_ids = idx.get_rows(0, n)
    xe = synth.round_bf16(xu) if dtype == "bf16" else xu
    assert np.array_equal(got_ids, ids)
    assert np.array_equal(rows.view(np.uint32), xe.view(np.uint32))
    ref = [oracle.scan_topk(xe, ids, q, 64, threads=8) for q in Q]
    for b in range(0, len(Q), 3):  # single queries
        for k in (1, 10, 64):
            lab, dist = idx.search(Q[b], k)
            _same(lab, dist, ref[b][0][:k], ref[b][1][:k])
    for B, k in ((2, 10), (16, 64), (16, 1)):
        lab, dist, found = idx.search_batch(Q[:B], k)
        for b in range(B):
            f = len(ref[b][0][:k])
            assert found[b] == f
            _same(lab[b][:f], dist[b][:f], ref[b][0][:k], ref[b][1][:k])
    if batch256:  # a full batch of 256: the same bits as the fresh index
        Q256 = np.concatenate([Q, synth.unit_rows(11, 0, 256 - len(Q))])
        for k in (10, 64):
            a = idx.search_batch(Q256, k)
            e = fresh.search_batch(Q256, k)
            assert np.array_equal(a[2], e[2])
            for b in range(256):
                _same(a[0][b][:e[2][b]], a[1][b][:e[2][b]], e[0][b][:e[2][b]], e[1][b][:e[2][b]])
    # the filter shadows are those of the fresh index
    assert np.array_equal(idx.debug_filter_scores(Q[:8]).view(np.uint32), fresh.debug_filter_scores(Q[:8]).view(np.uint32))
    if f6:
        assert np.array_equal(idx.debug_f6_scores(Q[:8]).view(np.uint32), fresh.debug_f6_scores(Q[:8]).view(np.uint32))


def _run(dawn, oracle, n, pattern, dtype="f32", opts=None, batch256=True, f6=False):
    opts = opts or {}
    x = _rows(n)
    ids = _make_ids(n, pattern)
    pos = _patterns(n)[pattern]
    req = np.unique(ids[pos]) if pos else np.asarray([n + 5, n + 1000, 2**63], dtype=np.uint64)
    rng = np.random.default_rng(3)
    req = req[rng.permutation(len(req))]  # (any order)
    V = _new_rows(len(req))
    xu = x.copy()
    for b, lab in enumerate(req):
        xu[ids == lab] = V[b]
    idx = _index(dawn, dtype, opts, x, ids)
    counts = idx.update(req, V)
    assert counts.tolist() == [int((ids == lab).sum()) for lab in req]
    fresh = _index(dawn, dtype, opts, xu, ids)
    _check(dawn, oracle, idx, fresh, xu, ids, _queries(x, V), dtype, batch256, f6)
    return idx, fresh


# 1. equivalence across sizes and patterns (f32, default options)
_SIZES = [1, 31, 32, 33, 4097, 100_003, 300_001]


@pytest.mark.parametrize("n,pattern", [(n, p) for n in _SIZES for p in _patterns(n)])
def test_update_equivalence(dawn, oracle, n, pattern):
    _run(dawn, oracle, n, pattern, batch256=n <= 100_003 or pattern in ("row0", "random10"))


def test_update_dup_rewrites_both(dawn):
    n = 4097
    x, ids = _rows(n), _make_ids(n, "dup")
    idx = _index(dawn, "f32", {}, x, ids)
    V = _new_rows(1)
    assert idx.update([ids[n // 3]], V).tolist() == [2]
    rows, _ = idx.get_rows(0, n)
    assert np.array_equal(rows[n // 3], V[0]) and np.array_equal(rows[n // 2], V[0])


# 2. every filter path, f32 and bf16
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
@pytest.mark.parametrize("n,pattern", [(33, "last"), (4097, "block32"), (100_003, "random10"), (4097, "dup")])
def test_update_paths(dawn, oracle, dtype, path, n, pattern):
    _run(dawn, oracle, n, pattern, dtype, _PATHS[path], batch256=n <= 4097, f6=path == "fp6")


# 3. topical rows through the ladder
def test_update_ladder_topical(dawn, oracle):
    """Rows inside dense clusters (near-ties) get new vectors from the same clusters, and one row moves to another cluster."""
    n = 50_000
    x = oracle.unit_rows_topical(1, 0, n)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    rng = np.random.default_rng(5)
    pos = rng.choice(n, 500, replace=False)
    donors = rng.choice(n, 500, replace=False)
    V = np.ascontiguousarray(x[donors])  # (vectors of the same clusters: near-ties with their old neighbours)
    V[0] = x[(pos[0] + n // 2) % n]  # one row moves to a far cluster
    xu = x.copy()
    xu[pos] = V
    Q = np.ascontiguousarray(np.concatenate([x[np.linspace(0, n - 1, 10).astype(int)], V[:6]]))
    for opts in ({"force_fallback": 2}, {"force_fallback": 2, "i6_min_rows": 0}):
        idx = _index(dawn, "f32", opts, x, ids)
        assert idx.update(ids[pos], V).tolist() == [1] * len(pos)
        fresh = _index(dawn, "f32", opts, xu, ids)
        _check(dawn, oracle, idx, fresh, xu, ids, Q, "f32", batch256=False)


# 4. persistence
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_update_save_byte_identical(dawn, tmp_path, dtype):
    n = 4097
    x, ids = _rows(n), np.arange(1, n + 1, dtype=np.uint64)
    req = np.asarray([4097, 1, 2, 100, 4000], dtype=np.uint64)
    V = _new_rows(len(req))
    xu = x.copy()
    xu[(req - 1).astype(np.int64)] = V
    idx = _index(dawn, dtype, {}, x, ids)
    idx.update(req, V)
    fresh = _index(dawn, dtype, {}, xu, ids)
    a, b = str(tmp_path / "a.idx"), str(tmp_path / "b.idx")
    idx.save(a)
    fresh.save(b)
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()
    back = dawn.VectorIndex(0, dtype=dtype)
    back.load(a)
    Q = _queries(x, V)
    l1, d1, _ = back.search_batch(Q, 10)
    l2, d2, _ = fresh.search_batch(Q, 10)
    assert np.array_equal(l1, l2) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))


# 5. interleaving with other calls
def test_update_staged_row(dawn, oracle):
    n = 3000
    x = _rows(n)
    idx = dawn.VectorIndex(0)
    idx.add_batch(np.arange(1, 2001, dtype=np.uint64), x[:2000])
    for i in range(2000, 2500):  # staged on the host, not yet on the device
        idx.add(i + 1, x[i])
    V = _new_rows(3)
    assert idx.update([2400, 5, 2500], V).tolist() == [1, 1, 1]
    for i in range(2500, 3000):
        idx.add(i + 1, x[i])
    xu = x.copy()
    xu[[2399, 4, 2499]] = V
    ids = np.arange(1, n + 1, dtype=np.uint64)
    rows, got = idx.get_rows(0, n)
    assert np.array_equal(got, ids) and np.array_equal(rows.view(np.uint32), xu.view(np.uint32))
    for q in list(V) + list(_queries(x)[:4]):
        lab, dist = idx.search(q, 10)
        _same(lab, dist, *oracle.scan_topk(xu, ids, q, 10))
    assert idx.search(V[0], 1)[0][0] == 2400


def test_update_after_remove_then_get(dawn, oracle):
    n = 20_000
    x = _rows(n)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    idx = _index(dawn, "f32", {}, x, ids)
    rm = np.arange(1, n + 1, 7, dtype=np.uint64)
    idx.remove(rm)
    keep = ~np.isin(ids, rm)
    xs, ids_s = np.ascontiguousarray(x[keep]), ids[keep]
    req = np.asarray([2, 8, 19_999, 15, 1], dtype=np.uint64)  # (1, 8, 15 were removed)
    V = _new_rows(len(req))
    assert idx.update(req, V).tolist() == [1, 0, 1, 0, 0]
    xs[ids_s == 2] = V[0]
    xs[ids_s == 19_999] = V[2]
    fresh = _index(dawn, "f32", {}, xs, ids_s)
    _check(dawn, oracle, idx, fresh, xs, ids_s, _queries(xs, V[[0, 2]]), "f32")
    rows, counts = idx.get([2, 19_999, 8])
    assert counts.tolist() == [1, 1, 0]
    assert np.array_equal(rows[:2].view(np.uint32), V[[0, 2]].view(np.uint32))
    lab, dist, found = idx.search_like([2, 19_999], 10)
    for b, q in enumerate(V[[0, 2]]):
        _same(lab[b], dist[b], *oracle.scan_topk(xs, ids_s, q, 10))
    assert lab[0][0] == 2 and lab[1][0] == 19_999


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_update_same_vector_changes_nothing(dawn, tmp_path, dtype):
    n = 4097
    x, ids = _rows(n), np.arange(1, n + 1, dtype=np.uint64)
    idx = _index(dawn, dtype, {"i6_min_rows": 0, "f6_shadow": 1, "f6_min_rows": 0}, x, ids)
    Q = _queries(x)
    a0 = str(tmp_path / "a0.idx")
    idx.save(a0)
    f0, s0 = idx.debug_filter_scores(Q[:8]), idx.debug_f6_scores(Q[:8])
    req = np.asarray([1, 33, 64, 4097], dtype=np.uint64)
    assert idx.update(req, x[(req - 1).astype(np.int64)]).tolist() == [1] * 4
    a1 = str(tmp_path / "a1.idx")
    idx.save(a1)
    with open(a0, "rb") as fa, open(a1, "rb") as fb:
        assert fa.read() == fb.read()
    assert np.array_equal(f0.view(np.uint32), idx.debug_filter_scores(Q[:8]).view(np.uint32))
    assert np.array_equal(s0.view(np.uint32), idx.debug_f6_scores(Q[:8]).view(np.uint32))


# 6. large and repeated-label requests
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_update_large_request(dawn, oracle, dtype):
    """12 000 ids (past one LDS-sized piece of the request: the fence + L2 search), half of them absent, in random order."""
    n = 100_003
    x, ids = _rows(n), np.arange(1, n + 1, dtype=np.uint64)
    rng = np.random.default_rng(8)
    present = rng.choice(ids, 6000, replace=False)
    absent = rng.choice(np.arange(n + 1, 10 * n, dtype=np.uint64), 6000, replace=False)
    req = np.concatenate([present, absent])[rng.permutation(12_000)]
    V = _new_rows(len(req))
    xu = x.copy()
    hit = req <= n
    xu[(req[hit] - 1).astype(np.int64)] = V[hit]
    idx = _index(dawn, dtype, {}, x, ids)
    assert np.array_equal(idx.update(req, V), hit.astype(np.int64))
    fresh = _index(dawn, dtype, {}, xu, ids)
    _check(dawn, oracle, idx, fresh, xu, ids, _queries(x, V[hit]), dtype, batch256=True)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_update_one_label_everywhere(dawn, oracle, dtype):
    """Every row holds the requested label: all of them are rewritten, counted by wave-aggregated atomics."""
    n = 300_001
    x = _rows(n)
    ids = np.full(n, 42, dtype=np.uint64)
    idx = _index(dawn, dtype, {}, x, ids)
    V = _new_rows(2)
    assert idx.update([41, 42], V).tolist() == [0, n]
    rows, _ = idx.get_rows(0, n)
    e = synth.round_bf16(V[1:2]) if dtype == "bf16" else V[1:2]
    assert np.array_equal(rows.view(np.uint32), np.broadcast_to(e, rows.shape).view(np.uint32))
    q = synth.unit_rows(9, 0, 1)[0]
    lab, dist = idx.search(q, 10)
    _same(lab, dist, *oracle.scan_topk(np.ascontiguousarray(np.broadcast_to(e, (n, 384))), ids, q, 10, threads=8))
    fresh = _index(dawn, dtype, {}, np.ascontiguousarray(np.broadcast_to(V[1], (n, 384))), ids)
    Q = _queries(x)
    assert np.array_equal(idx.debug_filter_scores(Q[:8]).view(np.uint32), fresh.debug_filter_scores(Q[:8]).view(np.uint32))


# 7. captured graphs
def test_update_search_device_graph_replay(dawn, oracle):
    torch = pytest.importorskip("torch")
    n = 20_000
    x, ids = _rows(n), np.arange(1, n + 1, dtype=np.uint64)
    idx = _index(dawn, "f32", {"i6_min_rows": 0}, x, ids)
    V = _new_rows(40)
    req = np.arange(101, 20_001, 500, dtype=np.uint64)[:40]
    Q = np.ascontiguousarray(np.concatenate([V[:4], _queries(x)[:4]]))
    B, k = len(Q), 10
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    lab = torch.zeros((B, k), dtype=torch.int64, device=dev)
    dist = torch.zeros((B, k), dtype=torch.float32, device=dev)
    fnd = torch.zeros((B,), dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):  # warm-up on the capture stream
        idx.search_device(dq.data_ptr(), B, k, lab.data_ptr(), dist.data_ptr(), fnd.data_ptr(), side.cuda_stream)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        idx.search_device(dq.data_ptr(), B, k, lab.data_ptr(), dist.data_ptr(), fnd.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    xu = x.copy()
    for step in range(2):  # the graph of the original rows, replayed after each of two updates
        sel = slice(20 * step, 20 * step + 20)
        assert idx.update(req[sel], V[sel]).tolist() == [1] * 20
        xu[(req[sel] - 1).astype(np.int64)] = V[sel]
        g.replay()
        torch.cuda.synchronize()
        L, D, F = lab.cpu().numpy().view(np.uint64), dist.cpu().numpy(), fnd.cpu().numpy()
        for b, q in enumerate(Q):
            assert F[b] == k
            _same(L[b], D[b], *oracle.scan_topk(xu, ids, q, k))
    assert L[0][0] == req[0]


# 8. errors: nothing changes
def _snapshot(idx, Q):
    rows, got = idx.get_rows(0, idx.size())
    return rows, got, idx.search_batch(Q, 10), idx.search(Q[0], 10)


def _unchanged(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    for i in range(3):
        assert np.array_equal(np.asarray(a[2][i]).view(np.uint8), np.asarray(b[2][i]).view(np.uint8))
    _same(b[3][0], b[3][1], a[3][0], a[3][1])


def test_update_errors(dawn):
    from dawnsearch_amd import _lib
    n = 5000
    x, ids = _rows(n), np.arange(1, n + 1, dtype=np.uint64)
    idx = _index(dawn, "f32", {"i6_min_rows": 0}, x, ids)
    for i in range(3):  # (staged adds: an error must not lose them either)
        idx.add(n + 1 + i, x[i])
    Q = _queries(x)
    s0 = _snapshot(idx, Q)
    V = _new_rows(3)
    bad = V.copy()
    bad[1] *= 1.5  # not normalised
    with pytest.raises(_lib.DawnError) as e:
        idx.update([1, 2, 3], bad)
    assert e.value.code == _lib.ERR_NOT_NORMALIZED
    _unchanged(s0, _snapshot(idx, Q))
    with pytest.raises(_lib.DawnError) as e:
        idx.update([7, 9, 7], V)
    assert e.value.code == _lib.ERR_INVALID_ARG
    _unchanged(s0, _snapshot(idx, Q))
    upd = np.full(3, 9, dtype=np.uintp)
    h = idx._h
    assert _lib.lib.dawn_index_update(h, 3, None, V.ctypes.data, upd.ctypes.data) == _lib.ERR_INVALID_ARG
    ids3 = np.asarray([1, 2, 3], dtype=np.uint64)
    assert _lib.lib.dawn_index_update(h, 3, ids3.ctypes.data, None, upd.ctypes.data) == _lib.ERR_INVALID_ARG
    assert _lib.lib.dawn_index_update(None, 3, ids3.ctypes.data, V.ctypes.data, upd.ctypes.data) == _lib.ERR_INVALID_ARG
    assert _lib.lib.dawn_index_update(h, 0, None, None, None) == 0
    assert idx.update(np.zeros(0, dtype=np.uint64), np.zeros((0, 384), np.float32)).tolist() == []
    _unchanged(s0, _snapshot(idx, Q))
    # absent labels: updated = 0, nothing changes
    assert idx.update([n + 100, 0, int(U64MAX)], V).tolist() == [0, 0, 0]
    _unchanged(s0, _snapshot(idx, Q))


# 9. sharded handles
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_update_sharded_equals_single(dawn, tmp_path, dtype):
    n = 10_000
    x = _rows(n)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    ids[7000] = ids[1500]  # a label held by rows of two shards
    single = _index(dawn, dtype, {}, x, ids)
    sh = dawn.VectorIndex(devices=[0, 0, 0], dtype=dtype)
    sh.set_option("shard_chunk", 1024)
    sh.add_batch(ids, x)
    rng = np.random.default_rng(4)
    for step in range(2):
        req = np.concatenate([rng.choice(ids, 300, replace=False), [ids[1500], n + 50]]) if step else np.asarray([1, ids[1500], 9999])
        req = np.unique(req.astype(np.uint64))
        V = _new_rows(len(req), seed=80 + step)
        c1 = single.update(req, V)
        c2 = sh.update(req, V)
        assert np.array_equal(c1, c2) and c1[req == ids[1500]].tolist() == [2]
    Q = _queries(x, V)
    for k in (1, 10):
        a, b = single.search_batch(Q, k), sh.search_batch(Q, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert np.array_equal(a[2], b[2])
    probe = np.concatenate([req[:20], [n + 50]]).astype(np.uint64)
    ra, ca = single.get(probe)
    rb, cb = sh.get(probe)
    assert np.array_equal(ca, cb) and np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
    fa, fb = str(tmp_path / "s.idx"), str(tmp_path / "h.idx")
    single.save(fa)
    sh.save(fb)
    with open(fa, "rb") as f1, open(fb, "rb") as f2:
        assert f1.read() == f2.read()


# 10. at scale
def test_update_at_scale(dawn, oracle):
    n, k = 12_500_000, 10
    idx = dawn.VectorIndex(0)
    idx.fill_synthetic(1, 0, n, 1)
    rng = np.random.default_rng(12)
    req = np.sort(rng.choice(np.arange(1, n + 1, dtype=np.uint64), 1000, replace=False))
    V = _new_rows(1000, seed=90)
    assert idx.update(req, V).tolist() == [1] * 1000
    Q = np.concatenate([synth.unit_rows(21, 0, 3), V[[0, 500, 999]], synth.planted_queries(1, [123, n - 7], 5)])
    # the oracle over the synthetic rows, then the updated rows merged in: drop the replaced labels, add their new scores
    olab, odist = oracle.scan_topk_synth(1, 0, n, 1, Q, k + 1000)
    gone = set(req.tolist())
    lab, dist, found = idx.search_batch(Q, k)
    for b, q in enumerate(Q):
        keep = [i for i, l in enumerate(olab[b]) if int(l) not in gone]
        nl, nd = oracle.scan_topk(V, req, q, k)
        cl = np.concatenate([olab[b][keep], nl])
        cd = np.concatenate([odist[b][keep], nd])
        order = np.lexsort((cl, cd))[:k]  # (ties: the lower label = the earlier row, labels are positions + 1 here)
        el, ed = cl[order], cd[order]
        l1, d1 = idx.search(q, k)
        _same(l1, d1, el, ed)
        _same(lab[b], dist[b], el, ed)
    assert lab[3][0] == req[0] and lab[5][0] == req[999]


# 11. the provider
def test_search_provider_refresh_pages(dawn):
    from dawnsearch_amd._lib import NotNormalizedError
    from dawnsearch_amd.search_provider import ExtractedPage, SearchProvider
    sp = SearchProvider(0)
    x = _rows(200)
    sp.insert_batch([ExtractedPage(url=f"https://example.org/{j}", title=f"t{j}") for j in range(200)], x)
    hit = sp.search_embedding(x[10]).pages[0]
    assert hit.url == "https://example.org/10"
    old_id = hit.page_id
    V = _new_rows(2, seed=44)
    bad = V.copy()
    bad[1] *= 2.0
    pages = [ExtractedPage(url="https://example.org/10", title="re-crawled", text="new text"),
             ExtractedPage(url="https://example.org/new", title="fresh")]
    with pytest.raises(NotNormalizedError):
        sp.refresh_pages(pages, bad)
    assert sp.page_count() == 200 and sp.search_embedding(x[10]).pages[0].page_id == old_id
    assert sp.refresh_pages(pages, V) == (1, 1)
    assert sp.page_count() == 201 and sp.index.size() == 201
    top = sp.search_embedding(V[0]).pages[0]
    assert top.page_id == old_id and top.url == "https://example.org/10"
    assert top.title == "re-crawled" and top.text == "new text" and top.distance < 1e-5
    rows, counts = sp.index.get([old_id])
    assert counts.tolist() == [1] and np.array_equal(rows[0].view(np.uint32), V[0].view(np.uint32))
    new = sp.search_embedding(V[1]).pages[0]
    assert new.url == "https://example.org/new" and new.page_id == 201
