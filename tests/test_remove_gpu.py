"""dawn_index_remove: rows leave the index by label, compacted in place on the GPU (index_compact.hip).

The property under test (include/dawn_hip.h): after a removal the index IS the index of the surviving rows added in their
original order — rows, labels, their order, the filter shadows, search results and save files.  Every check is bit-exact:
search results against the CPU oracle (oracle.scan_topk over the survivors), everything else against a fresh index built
from the survivors.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dawnsearch_amd import synth  # noqa: E402


@functools.lru_cache(maxsize=4)
def _rows(n):
    from oracle import oracle_lib
    return oracle_lib.unit_rows(1, 0, n)


def _queries(x, nq=16):
    """Queries planted near rows spread over the index (their top-k sits where rows moved) + a few uniform ones."""
    n = x.shape[0]
    picks = np.linspace(0, n - 1, num=min(nq - 4, n)).astype(np.int64)
    Q = [synth.planted_queries(1, [int(p)], 100 + i)[0] if n > 0 else None for i, p in enumerate(picks)]
    Q = [q for q in Q if q is not None]
    Q += list(synth.unit_rows(9, 0, nq - len(Q)))
    return np.ascontiguousarray(np.stack(Q), dtype=np.float32)


def _patterns(n):
    """name -> labels to remove (ids are 1..n; 'dup' relabels one row with another's label first)."""
    rng = np.random.default_rng(n)
    p = {
        "row0": [1],
        "last": [n],
        "mid_subtile": [min(n, 32 + 17)],
        "every_other": list(range(1, n + 1, 2)),
        "random10": sorted(rng.choice(np.arange(1, n + 1), size=max(1, n // 10), replace=False).tolist()),
        "all": list(range(1, n + 1)),
        "absent": [n + 5, n + 1000, 2**63],
        "repeated": [min(n, 3)] * 3 + [min(n, 3)],
    }
    if n >= 64:
        p["block32"] = list(range(33, 65))  # rows 32..63: one aligned sub-tile
    if n >= 3:
        p["dup"] = [n // 3 + 1]
    return p


def _make_ids(n, pattern):
    ids = np.arange(1, n + 1, dtype=np.uint64)
    if pattern == "dup":
        ids[n // 2] = ids[n // 3]  # a label held by two rows
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


def _check(dawn, oracle, idx, fresh, xs, ids_s, Q, dtype, batch256=True):
    n = len(ids_s)
    assert idx.size() == n
    if n:
        rows, got_ids = idx.get_rows(0, n)
        xe = synth.round_bf16(xs) if dtype == "bf16" else xs
        assert np.array_equal(got_ids, ids_s)
        assert np.array_equal(rows.view(np.uint32), xe.view(np.uint32))
    else:
        xe = xs
    ref = [oracle.scan_topk(xe, ids_s, q, 64, threads=8) for q in Q]
    for b in range(2):  # single queries
        for k in (1, 10, 64):
            lab, dist = idx.search(Q[b], k)
            _same(lab, dist, ref[b][0][:k], ref[b][1][:k])
    for B, k in ((2, 10), (16, 64), (16, 1)):
        lab, dist, found = idx.search_batch(Q[:B], k)
        for b in range(B):
            f = len(ref[b][0][:k])
            assert found[b] == f
            _same(lab[b][:f], dist[b][:f], ref[b][0][:k], ref[b][1][:k])
    if n and batch256:  # a full batch of 256: the same bits as the fresh index of the survivors
        Q256 = np.concatenate([Q, synth.unit_rows(11, 0, 256 - len(Q))])
        for k in (10, 64):
            a = idx.search_batch(Q256, k)
            e = fresh.search_batch(Q256, k)
            assert np.array_equal(a[2], e[2])
            for b in range(256):  # (slots past found[b] are not part of the result)
                _same(a[0][b][:e[2][b]], a[1][b][:e[2][b]], e[0][b][:e[2][b]], e[1][b][:e[2][b]])
    if n:  # the filter shadows are those of the fresh index
        assert np.array_equal(idx.debug_filter_scores(Q[:8]).view(np.uint32), fresh.debug_filter_scores(Q[:8]).view(np.uint32))


def _run(dawn, oracle, n, pattern, dtype="f32", opts=None, batch256=True):
    opts = opts or {}
    x = _rows(n)
    ids = _make_ids(n, pattern)
    rm = _patterns(n)[pattern]
    keep = ~np.isin(ids, np.asarray(rm, dtype=np.uint64))
    idx = _index(dawn, dtype, opts, x, ids)
    removed = idx.remove(np.asarray(rm, dtype=np.uint64))
    assert removed == int((~keep).sum())
    xs, ids_s = np.ascontiguousarray(x[keep]), ids[keep]
    fresh = _index(dawn, dtype, opts, xs, ids_s)
    _check(dawn, oracle, idx, fresh, xs, ids_s, _queries(x), dtype, batch256)
    return idx, fresh


# 1. equivalence across sizes and removal patterns (f32, default options)
_SIZES = [1, 31, 32, 33, 4097, 100_003, 300_001]


@pytest.mark.parametrize("n,pattern", [(n, p) for n in _SIZES for p in _patterns(n)])  # (block32 from 64 rows, dup from 3)
def test_remove_equivalence(dawn, oracle, n, pattern):
    _run(dawn, oracle, n, pattern, batch256=n <= 100_003 or pattern in ("row0", "random10"))


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
@pytest.mark.parametrize("n,pattern", [(33, "row0"), (4097, "every_other"), (100_003, "random10"), (100_003, "row0"), (4097, "dup")])
def test_remove_paths(dawn, oracle, dtype, path, n, pattern):
    idx, fresh = _run(dawn, oracle, n, pattern, dtype, _PATHS[path], batch256=n <= 4097)
    if path == "fp6" and idx.size():
        Q = _queries(_rows(n))[:8]
        assert np.array_equal(idx.debug_f6_scores(Q).view(np.uint32), fresh.debug_f6_scores(Q).view(np.uint32))


def test_remove_ladder_topical(dawn, oracle):
    """Topical rows (clusters of near-ties) with every certificate failing: the bounded pass answers on the compacted shadows."""
    n = 50_000
    x = oracle.unit_rows_topical(1, 0, n)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    rng = np.random.default_rng(5)
    rm = np.concatenate([[1, 2, 3], rng.choice(ids, 4000, replace=False)])
    keep = ~np.isin(ids, rm)
    xs, ids_s = np.ascontiguousarray(x[keep]), ids[keep]
    for opts in ({"force_fallback": 2}, {"force_fallback": 2, "i6_min_rows": 0}):
        idx = _index(dawn, "f32", opts, x, ids)
        assert idx.remove(rm) == int((~keep).sum())
        fresh = _index(dawn, "f32", opts, xs, ids_s)
        Q = np.ascontiguousarray(x[np.linspace(0, n - 1, 16).astype(int)])  # (queries inside the clusters: near-ties)
        _check(dawn, oracle, idx, fresh, xs, ids_s, Q, "f32", batch256=False)


# 3. persistence
def test_remove_save_byte_identical(dawn, oracle, tmp_path):
    for dtype in ("f32", "bf16"):
        n = 4097
        x, ids = _rows(n), np.arange(1, n + 1, dtype=np.uint64)
        rm = np.asarray([1, 2, 100, 4000, 4097], dtype=np.uint64)
        keep = ~np.isin(ids, rm)
        idx = _index(dawn, dtype, {}, x, ids)
        idx.remove(rm)
        fresh = _index(dawn, dtype, {}, np.ascontiguousarray(x[keep]), ids[keep])
        a, b = str(tmp_path / f"a_{dtype}.idx"), str(tmp_path / f"b_{dtype}.idx")
        idx.save(a)
        fresh.save(b)
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read()
        back = dawn.VectorIndex(0, dtype=dtype)
        back.load(a)
        Q = _queries(x)
        l1, d1, _ = back.search_batch(Q, 10)
        l2, d2, _ = fresh.search_batch(Q, 10)
        assert np.array_equal(l1, l2) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))


# 4. staged single-row adds, and the re-crawl case
def test_remove_with_staged_adds(dawn, oracle):
    n = 3000
    x = _rows(n)
    idx = dawn.VectorIndex(0)
    idx.add_batch(np.arange(1, 2001, dtype=np.uint64), x[:2000])
    for i in range(2000, 2500):  # staged on the host, not yet on the device
        idx.add(i + 1, x[i])
    assert idx.size() == 2500
    assert idx.remove([5, 1999, 2100, 2500]) == 4
    for i in range(2500, 3000):
        idx.add(i + 1, x[i])
    ids = np.arange(1, n + 1, dtype=np.uint64)
    keep = ~np.isin(ids, [5, 1999, 2100, 2500])
    xs, ids_s = np.ascontiguousarray(x[keep]), ids[keep]
    assert idx.size() == len(ids_s)
    for q in _queries(x)[:6]:
        lab, dist = idx.search(q, 10)
        _same(lab, dist, *oracle.scan_topk(xs, ids_s, q, 10))
    # re-crawl: label 7 leaves and comes back with another vector, now the last row
    v = synth.unit_rows(42, 0, 1)[0]
    assert idx.remove(7) == 1
    idx.add(7, v)
    keep7 = ids_s != 7
    xs2 = np.concatenate([xs[keep7], v[None]])
    ids2 = np.concatenate([ids_s[keep7], np.asarray([7], dtype=np.uint64)])
    lab, dist = idx.search(v, 5)
    _same(lab, dist, *oracle.scan_topk(xs2, ids2, v, 5))
    assert lab[0] == 7
    rows, got = idx.get_rows(0, idx.size())
    assert np.array_equal(got, ids2) and np.array_equal(rows.view(np.uint32), xs2.view(np.uint32))


# 5. thresholds, emptying, device-resident search
def test_remove_shrinks_below_packed_threshold(dawn, oracle):
    n, cut = 800_000, 20_000  # 800 k rows keep the packed shadow (from 768 Ki); 780 k rows do not
    idx = dawn.VectorIndex(0)
    idx.fill_synthetic(1, 0, n, 1)
    before = idx.memory()["shadows"]
    assert idx.remove(np.arange(1, cut + 1, dtype=np.uint64)) == cut
    after = idx.memory()["shadows"]
    assert idx.size() == n - cut
    assert before - after >= (n - cut) * 240  # the packed shadow went back
    Q = synth.unit_rows(3, 0, 4)
    olab, odist = oracle.scan_topk_synth(1, cut, n - cut, cut + 1, Q, 10)
    for b, q in enumerate(Q):
        lab, dist = idx.search(q, 10)
        _same(lab, dist, olab[b], odist[b])
    lab, dist, _ = idx.search_batch(Q, 10)
    for b in range(len(Q)):
        _same(lab[b], dist[b], olab[b], odist[b])


def test_remove_to_empty_then_add(dawn, oracle):
    n = 1000
    x = _rows(n)
    idx = _index(dawn, "f32", {}, x, np.arange(1, n + 1, dtype=np.uint64))
    assert idx.remove(np.arange(1, n + 1, dtype=np.uint64)) == n
    assert idx.size() == 0
    lab, dist = idx.search(x[0], 10)
    assert len(lab) == 0
    idx.add_batch(np.arange(501, 601, dtype=np.uint64), x[500:600])
    q = x[550]
    lab, dist = idx.search(q, 10)
    _same(lab, dist, *oracle.scan_topk(x[500:600], np.arange(501, 601, dtype=np.uint64), q, 10))


def test_remove_then_search_device(dawn, oracle):
    torch = pytest.importorskip("torch")
    n = 20_000
    x = _rows(n)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    idx = _index(dawn, "f32", {}, x, ids)
    rm = np.arange(1, n + 1, 3, dtype=np.uint64)
    idx.remove(rm)
    keep = ~np.isin(ids, rm)
    xs, ids_s = np.ascontiguousarray(x[keep]), ids[keep]
    Q = _queries(x)
    B, k = len(Q), 10
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    lab = torch.zeros((B, k), dtype=torch.int64, device=dev)
    dist = torch.zeros((B, k), dtype=torch.float32, device=dev)
    fnd = torch.zeros((B,), dtype=torch.int32, device=dev)
    idx.search_device(dq.data_ptr(), B, k, lab.data_ptr(), dist.data_ptr(), fnd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    L, D = lab.cpu().numpy().view(np.uint64), dist.cpu().numpy()
    for b, q in enumerate(Q):
        _same(L[b], D[b], *oracle.scan_topk(xs, ids_s, q, k))


# 6. errors
def test_remove_errors(dawn, oracle):
    from dawnsearch_amd import _lib
    sh = dawn.VectorIndex(devices=[0, 0])
    sh.set_option("shard_chunk", 1024)
    sh.fill_synthetic(1, 0, 5000, 1)
    q = synth.unit_rows(2, 0, 1)[0]
    l0, d0 = sh.search(q, 10)
    with pytest.raises(_lib.DawnError) as e:
        sh.remove([1, 2, 3])
    assert e.value.code == _lib.ERR_UNSUPPORTED
    assert sh.size() == 5000
    l1, d1 = sh.search(q, 10)
    _same(l1, d1, l0, d0)
    idx = dawn.VectorIndex(0)
    idx.fill_synthetic(1, 0, 5000, 1)
    removed = C.c_size_t(7)
    assert _lib.lib.dawn_index_remove(idx._h, 3, None, C.byref(removed)) == _lib.ERR_INVALID_ARG
    assert idx.size() == 5000
    assert _lib.lib.dawn_index_remove(idx._h, 0, None, C.byref(removed)) == 0 and removed.value == 0
    assert idx.remove(np.zeros(0, dtype=np.uint64)) == 0
    assert idx.size() == 5000
    x = _rows(5000)
    lab, dist = idx.search(q, 10)
    _same(lab, dist, *oracle.scan_topk(x, np.arange(1, 5001, dtype=np.uint64), q, 10))


# 7. at scale
def test_remove_at_scale(dawn, oracle):
    n, k = 12_500_000, 10
    idx = dawn.VectorIndex(0)
    idx.fill_synthetic(1, 0, n, 1)
    Q = np.concatenate([synth.unit_rows(21, 0, 4), synth.planted_queries(1, [123, 5_000_000, n - 7, 77_777], 5)])
    m_front = 1000 - 5 * len(Q)
    olab, odist = oracle.scan_topk_synth(1, 0, n, 1, Q, k + 1000)
    rng = np.random.default_rng(12)
    rm = set(olab[:, :5].ravel().tolist())
    front = rng.choice(np.arange(1, 200_001, dtype=np.uint64), size=m_front, replace=False).tolist()
    rm |= set(front)
    rm = np.asarray(sorted(rm), dtype=np.uint64)
    assert idx.remove(rm) == len(rm)
    assert idx.size() == n - len(rm)
    gone = set(rm.tolist())
    lab, dist, found = idx.search_batch(Q, k)
    for b, q in enumerate(Q):
        sel = np.asarray([i for i, l in enumerate(olab[b]) if int(l) not in gone][:k])
        el, ed = olab[b][sel], odist[b][sel]
        l1, d1 = idx.search(q, k)
        _same(l1, d1, el, ed)
        _same(lab[b], dist[b], el, ed)


# 8. the provider
def test_search_provider_remove_pages(dawn):
    from dawnsearch_amd.search_provider import ExtractedPage, SearchProvider
    sp = SearchProvider(0)
    x = _rows(200)
    sp.insert_batch([ExtractedPage(url=f"https://example.org/{j}") for j in range(200)], x)
    assert sp.page_count() == 200
    hit = sp.search_embedding(x[10]).pages[0]
    assert hit.url == "https://example.org/10"
    gone_id = hit.page_id
    assert sp.remove_pages([gone_id, 12345]) == 1
    assert sp.page_count() == 199 and sp.index.size() == 199
    assert all(p.page_id != gone_id for p in sp.search_embedding(x[10]).pages)
    v = synth.unit_rows(43, 0, 1)[0]
    sp.insert(ExtractedPage(url="https://example.org/10", title="re-crawled"), v)
    assert sp.page_count() == 200
    top = sp.search_embedding(v).pages[0]
    assert top.url == "https://example.org/10" and top.page_id != gone_id and top.title == "re-crawled"
