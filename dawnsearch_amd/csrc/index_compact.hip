// index_compact.hip — removal of rows by label (dawn_index_remove): the index is compacted IN PLACE, stably, so that afterwards
// it is exactly the index of its surviving rows added in their original order.  Three launches:
//   mark   every row looks its label up in the sorted, deduplicated list of removed labels: a keep mask per 32-row chunk, the
//          chunk's kept rows as a prefix inside its 8192-row block, the block's total, the first removed position (atomicMin);
//   scan   one workgroup: exclusive scan of the block totals (and their sum: the new size);
//   move   from the chunk of the first removed row on, every kept row (its 16-B pieces and its label) moves to
//          dst = src - (removed rows before src).  Race-free by construction: a chunk's workgroup READS all of its kept rows
//          into registers, then publishes "read" for the chunk (its prefix word becomes CMP_READ), then waits until the at
//          most two chunks whose source rows its destination range covers have published theirs, then WRITES.  Destinations
//          never lie past their sources, so a chunk's writes only ever land on source rows of itself (read before, same
//          workgroup) or of earlier chunks (waited for).  Chunks are claimed in increasing order from a counter, and a
//          workgroup publishes before it waits: the chunk it waits for belongs to a running workgroup that never waits
//          before publishing, so the waits cannot deadlock, and nothing is staged anywhere — each kept byte is read once and
//          written once.
// The shadows are not touched here: dawn_index.cpp re-quantises their sub-tiles from the first affected one.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace dawn {
namespace {

using u32x4 = __attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t;

constexpr uint32_t CMP_READ = 0xFFFFFFFFu;  // a chunk's prefix word once its rows are read (never a valid prefix: < 8192)

__device__ __forceinline__ bool label_listed(const uint64_t* __restrict__ rm, uint32_t n_rm, uint64_t id) {
    uint32_t lo = 0, hi = n_rm;  // first entry >= id
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rm[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_rm && rm[lo] == id;
}

// 256 threads = 4 waves; block b covers rows [8192 b, 8192 (b + 1)) = chunks [256 b, 256 (b + 1)), a wave 64 rows (2 chunks)
// per step.  mask[c] bit r: row 32 c + r is kept; pre[c]: kept rows of the block's chunks before c; blk[b]: the block's kept rows.
__global__ __launch_bounds__(256) void compact_mark_kernel(const uint64_t* __restrict__ ids, uint32_t n_rows,
                                                           const uint64_t* __restrict__ rm, uint32_t n_rm,
                                                           uint32_t* __restrict__ mask, uint32_t* __restrict__ pre,
                                                           uint32_t* __restrict__ blk, uint32_t* __restrict__ first_removed) {
    __shared__ uint32_t sh_cnt[CMP_BLOCK_CHUNKS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t chunk0 = blockIdx.x * CMP_BLOCK_CHUNKS;
    const uint32_t n_chunks = (n_rows + CMP_CHUNK - 1) / CMP_CHUNK;
    uint32_t first = 0xFFFFFFFFu;
    for (int s = 0; s < CMP_BLOCK_CHUNKS / 8; ++s) {
        const uint32_t lc = (uint32_t)(s * 8 + wave * 2);  // the wave's first chunk of this step (block-local)
        const uint32_t row = (chunk0 + lc) * CMP_CHUNK + (uint32_t)lane;
        bool keep = false;
        if (row < n_rows) keep = !label_listed(rm, n_rm, __builtin_nontemporal_load(ids + row));
        const unsigned long long kb = __ballot(keep);
        const unsigned long long valid = __ballot(row < n_rows);
        const unsigned long long gone = valid & ~kb;
        if (gone && lane == 0) first = min(first, (chunk0 + lc) * CMP_CHUNK + (uint32_t)__builtin_ctzll(gone));
        if (lane < 2) {
            const uint32_t m = (uint32_t)(kb >> (32 * lane));
            if (chunk0 + lc + lane < n_chunks) mask[chunk0 + lc + lane] = m;
            sh_cnt[lc + lane] = (uint32_t)__builtin_popcount(m);
        }
    }
    if (lane == 0 && first != 0xFFFFFFFFu) atomicMin(first_removed, first);
    __syncthreads();
    if (threadIdx.x == 0) {  // 256 counts: a sequential prefix costs less than the barriers of a parallel one
        uint32_t acc = 0;
        for (int c = 0; c < CMP_BLOCK_CHUNKS; ++c) {
            const uint32_t v = sh_cnt[c];
            sh_cnt[c] = acc;
            acc += v;
        }
        blk[blockIdx.x] = acc;
    }
    __syncthreads();
    const uint32_t c = chunk0 + threadIdx.x;
    if (c < n_chunks) pre[c] = sh_cnt[threadIdx.x];
}

// One workgroup of 1024: blk[0..nb) -> exclusive prefix, blk[nb] = the sum (rows kept); *claim = 0 for the move.
__global__ __launch_bounds__(1024) void compact_scan_kernel(uint32_t* __restrict__ blk, uint32_t nb, uint32_t* __restrict__ claim) {
    __shared__ uint32_t sh[1024];
    const uint32_t per = (nb + 1023) / 1024;
    const uint32_t b0 = min(nb, threadIdx.x * per), b1 = min(nb, b0 + per);
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; ++b) sum += blk[b];
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan of the 1024 partial sums
        const uint32_t v = threadIdx.x >= (uint32_t)o ? sh[threadIdx.x - o] : 0u;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t acc = sh[threadIdx.x] - sum;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t v = blk[b];
        blk[b] = acc;
        acc += v;
    }
    if (threadIdx.x == 1023) {
        blk[nb] = sh[1023];
        *claim = 0;
    }
}

// 16-B piece e (0 .. U) of a 32-row chunk: its row inside the chunk and its place in the storage of row `row`.
//   f32: rows are 96 pieces, contiguous;  bf16: the chunk is half a 64-row tile, piece e = fragment e / 64, lane e % 64
//   (frag_chunk in wave_topk.hpp: lane = h * 32 + r holds piece 2 s + h of row r of the half)
template <int RT>
struct ChunkLayout {
    static constexpr int U = RT == ROW_BF16 ? CMP_CHUNK * 48 : CMP_CHUNK * 96;  // 16-B pieces per chunk
    __device__ static int row_of(int e) { return RT == ROW_BF16 ? (e & 31) : e / 96; }
    __device__ static int piece_of(int e) { return RT == ROW_BF16 ? (((e >> 6) << 1) | ((e >> 5) & 1)) : e % 96; }
    __device__ static size_t slot(size_t row, int c) {
        if (RT == ROW_BF16) return (row >> 6) * 3072 + (((row >> 5) & 1) * 24 + (c >> 1)) * 64 + (c & 1) * 32 + (row & 31);
        return row * 96 + c;
    }
};

template <int RT>
__global__ __launch_bounds__(256) void compact_move_kernel(u32x4* __restrict__ x, uint64_t* __restrict__ ids,
                                                           const uint32_t* __restrict__ mask, uint32_t* pre,
                                                           const uint32_t* __restrict__ blk, uint32_t* claim, uint32_t first_chunk,
                                                           uint32_t n_chunks) {
    using L = ChunkLayout<RT>;
    constexpr int PER = L::U / 256;  // pieces per thread: 12 (f32) / 6 (bf16)
    static_assert(L::U % 256 == 0, "whole pieces per thread");
    __shared__ uint32_t sh_c;
    for (;;) {
        if (threadIdx.x == 0) sh_c = first_chunk + atomicAdd(claim, 1u);
        __syncthreads();
        const uint32_t c = sh_c;
        if (c >= n_chunks) return;
        const uint32_t m = mask[c];
        const uint32_t dst0 = blk[c / CMP_BLOCK_CHUNKS] + pre[c];  // destination of the chunk's first kept row
        u32x4 v[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = (int)threadIdx.x + 256 * i;
            if ((m >> L::row_of(e)) & 1u)
                v[i] = __builtin_nontemporal_load(x + L::slot((size_t)c * CMP_CHUNK + L::row_of(e), L::piece_of(e)));
        }
        uint64_t id = 0;
        if (threadIdx.x < CMP_CHUNK && ((m >> threadIdx.x) & 1u)) id = ids[(size_t)c * CMP_CHUNK + threadIdx.x];
        // every load of the chunk has returned before the chunk is published as read.  Only that order matters (a returned load
        // cannot see a later store), so the wait is explicit and the flags are relaxed device-scope atomics: a release fence /
        // acquire load at device scope would write back / invalidate L2 for every chunk (measured: 736 ms instead of ~65 for
        // 100 M rows)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __hip_atomic_store(pre + c, CMP_READ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // the destination rows [dst0, dst0 + kept) lie in source chunks dst0 / 32 .. (dst0 + kept - 1) / 32 (<= c): wait for
            // those before c to have been read
            if (m) {
                const uint32_t lo = dst0 / CMP_CHUNK, hi = (dst0 + (uint32_t)__builtin_popcount(m) - 1) / CMP_CHUNK;
                for (uint32_t w = lo; w <= hi && w < c; ++w)
                    while (__hip_atomic_load(pre + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != CMP_READ) __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = (int)threadIdx.x + 256 * i;
            const int r = L::row_of(e);
            if ((m >> r) & 1u) {
                const uint32_t d = dst0 + (uint32_t)__builtin_popcount(m & ((1u << r) - 1u));
                __builtin_nontemporal_store(v[i], x + L::slot(d, L::piece_of(e)));
            }
        }
        if (threadIdx.x < CMP_CHUNK && ((m >> threadIdx.x) & 1u))
            ids[dst0 + (uint32_t)__builtin_popcount(m & ((1u << threadIdx.x) - 1u))] = id;
        __syncthreads();  // (sh_c is re-written by the next claim)
    }
}

}  // namespace

void launch_compact_mark(const uint64_t* d_ids, uint32_t n_rows, const uint64_t* d_rm, uint32_t n_rm, uint32_t* d_mask, uint32_t* d_pre,
                         uint32_t* d_blk, uint32_t* d_first_removed, uint32_t* d_claim, hipStream_t stream) {
    const uint32_t nb = compact_blocks(n_rows);
    if (nb == 0) return;
    hipLaunchKernelGGL(compact_mark_kernel, dim3(nb), dim3(256), 0, stream, d_ids, n_rows, d_rm, n_rm, d_mask, d_pre, d_blk,
                       d_first_removed);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, stream, d_blk, nb, d_claim);
}

void launch_compact_move(void* d_x, int rt, uint64_t* d_ids, const uint32_t* d_mask, uint32_t* d_pre, const uint32_t* d_blk,
                         uint32_t* d_claim, uint32_t n_rows, uint32_t first_row, int grid, hipStream_t stream) {
    const uint32_t n_chunks = (n_rows + CMP_CHUNK - 1) / CMP_CHUNK, c0 = first_row / CMP_CHUNK;
    if (c0 >= n_chunks) return;
    const uint32_t g = std::min<uint32_t>(n_chunks - c0, (uint32_t)std::max(grid, 1));
    if (rt == ROW_BF16)
        hipLaunchKernelGGL(compact_move_kernel<ROW_BF16>, dim3(g), dim3(256), 0, stream, reinterpret_cast<u32x4*>(d_x), d_ids, d_mask,
                           d_pre, d_blk, d_claim, c0, n_chunks);
    else
        hipLaunchKernelGGL(compact_move_kernel<ROW_F32>, dim3(g), dim3(256), 0, stream, reinterpret_cast<u32x4*>(d_x), d_ids, d_mask,
                           d_pre, d_blk, d_claim, c0, n_chunks);
}

}  // namespace dawn
