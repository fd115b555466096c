// index_update.hip — rows replaced in place by label (dawn_index_update).  The request arrives sorted by label and
// free of duplicates (the host rejects an id given twice), so two requests never name the same row and every write below has
// exactly one writer.  Three launches, then the shadows:
//   hits        one read of the label array [0, n) with 16-B non-temporal loads, four in flight per lane.  Every row binary-searches
//               its label in the request: in LDS when the request fits (UP_LDS_KEYS), otherwise in an LDS fence of every k-th
//               label first and then in the k labels between two fences, read from L2.  A hit appends (position, request) to the
//               hit list — one atomicAdd per wave and round of 64 rows — and counts into its request's 64-bit counter, aggregated
//               over the wave and carried from round to round in registers as index_lookup.hip does: an index where every row
//               holds the requested label costs one counter atomic per wave, not one per row;
//   scatter     one wave per listed hit: the request's vector overwrites the row (f32 as given; a bf16 index rounds to nearest
//               even with f32_to_bf16_rne, the rounding of launch_rows_f32_to_bf16) and the row's 32-row sub-tile is marked in a
//               bitmap (atomicOr: several hits may share a sub-tile);
//   dirty list  the bitmap -> a list of sub-tiles and one of 64-row tiles (the f16 shadow's unit), one atomic per wave.
// dawn_index.cpp then re-quantises exactly the listed sub-tiles of every shadow with the converters' own device code
// (launch_rows_to_*_list in scan_i8 / scan_i6 / scan_f6 / scan_batched.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"
#include "wave_topk.hpp"

namespace dawn {
namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

constexpr int UP_THREADS = 256;
constexpr int UP_UNROLL = 4;  // 16-B label loads in flight per lane (8 rows)

// The request slot a wave has counted hits for and not published yet (wave-uniform).
struct ReqRun {
    int j = -1;
    unsigned long long cnt = 0;
};

__device__ __forceinline__ void req_flush(ReqRun& run, unsigned long long* __restrict__ cnt, int lane) {
    if (run.j >= 0 && lane == 0) atomicAdd(cnt + run.j, run.cnt);
    run.j = -1;
}

// The request index j with keys[j] == lab, or -1.  fence[0 .. n_f) = keys[0], keys[stride], ... (stride 1: fence IS the request).
__device__ __forceinline__ int find_key(uint64_t lab, const uint64_t* fence, uint32_t n_f, uint32_t stride,
                                        const uint64_t* __restrict__ keys, uint32_t n_keys) {
    uint32_t lo = 0, hi = n_f;  // first fence > lab (the caller has checked lab >= fence[0])
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (fence[mid] <= lab) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t f = lo - 1;
    if (stride == 1) return fence[f] == lab ? (int)f : -1;
    lo = f * stride + 1;  // (keys[f * stride] = fence[f])
    if (fence[f] == lab) return (int)(f * stride);
    hi = min(n_keys, lo - 1 + stride);
    while (lo < hi) {  // first key >= lab among the keys between two fences
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < lab) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_keys && keys[lo] == lab ? (int)lo : -1;
}

// One row per lane (rows row0 + lane * row_stride; `valid` = the lane holds a row).
__device__ __forceinline__ void hit_round(uint64_t lab, bool valid, size_t row0, size_t row_stride, const uint64_t* fence, uint32_t n_f,
                                          uint32_t stride, const uint64_t* __restrict__ keys, uint32_t n_keys, uint64_t key_lo,
                                          uint64_t key_hi, const uint32_t* __restrict__ perm, ReqRun& run,
                                          unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ total,
                                          uint64_t* __restrict__ hit_pos, uint32_t* __restrict__ hit_req, size_t cap, int lane) {
    int j = -1;
    if (valid && lab >= key_lo && lab <= key_hi) j = find_key(lab, fence, n_f, stride, keys, n_keys);
    const unsigned long long hits = __ballot(j >= 0);
    if (!hits) return;
    // the hit list: one atomic per wave and round
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(total, (unsigned long long)__builtin_popcountll(hits));
    base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 0);
    if (j >= 0) {
        const unsigned long long e = base + (unsigned long long)__builtin_popcountll(hits & ((1ull << lane) - 1ull));
        if (e < cap) {
            hit_pos[e] = row0 + (size_t)lane * row_stride;
            hit_req[e] = perm[j];
        }
    }
    // the requests' counters: one atomic per run of equal requests
    unsigned long long h = hits;
    while (h) {
        const int leader = __builtin_ctzll(h);
        const int s = __shfl(j, leader);
        const unsigned long long same = __ballot(j == s);
        if (s == run.j) {
            run.cnt += (unsigned long long)__builtin_popcountll(same);
        } else {
            req_flush(run, cnt, lane);
            run.j = s;
            run.cnt = (unsigned long long)__builtin_popcountll(same);
        }
        h &= ~same;
    }
}

__global__ __launch_bounds__(UP_THREADS) void update_hits_kernel(const uint64_t* __restrict__ labels, size_t n,
                                                                 const uint64_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                                 uint32_t n_keys, uint32_t stride, unsigned long long* __restrict__ cnt,
                                                                 unsigned long long* __restrict__ total, uint64_t* __restrict__ hit_pos,
                                                                 uint32_t* __restrict__ hit_req, size_t cap) {
    __shared__ uint64_t fence[UP_LDS_KEYS];
    const uint32_t n_f = (n_keys + stride - 1) / stride;  // <= UP_LDS_KEYS
    for (uint32_t i = threadIdx.x; i < n_f; i += UP_THREADS) fence[i] = keys[(size_t)i * stride];
    __syncthreads();
    const uint64_t key_lo = fence[0], key_hi = keys[n_keys - 1];
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * (UP_THREADS / 64) + (threadIdx.x >> 6);
    const size_t n_waves = (size_t)gridDim.x * (UP_THREADS / 64);
    const size_t n_pairs = n / 2;
    const u64x2* __restrict__ lab2 = reinterpret_cast<const u64x2*>(labels);
    ReqRun run;
    // a wave step: UP_UNROLL x 64 consecutive label pairs, lane l holding pairs base + 64 u + l
    for (size_t base = wave * (64 * UP_UNROLL); base < n_pairs; base += n_waves * (64 * UP_UNROLL)) {
        u64x2 v[UP_UNROLL];
#pragma unroll
        for (int u = 0; u < UP_UNROLL; ++u) {
            const size_t p = base + (size_t)(64 * u + lane);
            v[u] = p < n_pairs ? __builtin_nontemporal_load(lab2 + p) : u64x2{0, 0};
        }
#pragma unroll
        for (int u = 0; u < UP_UNROLL; ++u) {
            const size_t p0 = base + (size_t)(64 * u);
            const bool valid = p0 + (size_t)lane < n_pairs;
            hit_round(v[u].x, valid, 2 * p0, 2, fence, n_f, stride, keys, n_keys, key_lo, key_hi, perm, run, cnt, total, hit_pos, hit_req,
                      cap, lane);
            hit_round(v[u].y, valid, 2 * p0 + 1, 2, fence, n_f, stride, keys, n_keys, key_lo, key_hi, perm, run, cnt, total, hit_pos,
                      hit_req, cap, lane);
        }
    }
    if ((n & 1) && wave == 0)  // the odd last row
        hit_round(lane == 0 ? labels[n - 1] : 0, lane == 0, n - 1, 1, fence, n_f, stride, keys, n_keys, key_lo, key_hi, perm, run, cnt,
                  total, hit_pos, hit_req, cap, lane);
    req_flush(run, cnt, lane);
}

// One wave per hit (4 per workgroup).
template <int RT>
__global__ __launch_bounds__(256) void update_scatter_kernel(void* __restrict__ x, size_t n_rows, const uint64_t* __restrict__ pos,
                                                             const uint32_t* __restrict__ req, size_t n_hits, const f32x4* __restrict__ v,
                                                             uint32_t req_lo, uint32_t req_hi, uint32_t* __restrict__ dirty) {
    const size_t e = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= n_hits) return;
    const uint32_t r = req ? req[e] : (uint32_t)e;
    const size_t p = pos[e];
    if (r < req_lo || r >= req_hi || p >= n_rows) return;  // (another chunk's request; p < n_rows always: the hit pass lists rows)
    const f32x4* __restrict__ src = v + (size_t)(r - req_lo) * ROW_F4;
    if (RT == ROW_BF16) {
        u32x4* __restrict__ xb = reinterpret_cast<u32x4*>(x);
        if (lane < ROW_C8) {
            const f32x4 a = src[2 * lane], b = src[2 * lane + 1];
            u32x4 w;
            w.x = f32_to_bf16_rne(a.x) | (f32_to_bf16_rne(a.y) << 16);
            w.y = f32_to_bf16_rne(a.z) | (f32_to_bf16_rne(a.w) << 16);
            w.z = f32_to_bf16_rne(b.x) | (f32_to_bf16_rne(b.y) << 16);
            w.w = f32_to_bf16_rne(b.z) | (f32_to_bf16_rne(b.w) << 16);
            xb[frag_chunk(p, lane)] = w;
        }
    } else {
        f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(x) + p * ROW_F4;
        for (int c = lane; c < ROW_F4; c += 64) dst[c] = src[c];
    }
    if (lane == 0) atomicOr(dirty + (p >> 10), 1u << ((p >> 5) & 31u));
}

// The set bits of `mask` (one per lane) -> list entries first + bit, appended at one atomic per wave.
__device__ __forceinline__ void emit_bits(uint32_t mask, uint32_t first, uint32_t* __restrict__ list, uint32_t* __restrict__ count,
                                          int lane) {
    const uint32_t c = (uint32_t)__builtin_popcount(mask);
    uint32_t incl = c;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += t;
    }
    const uint32_t sum = (uint32_t)__shfl((int)incl, 63);
    uint32_t base = 0;
    if (lane == 0 && sum) base = atomicAdd(count, sum);
    base = (uint32_t)__shfl((int)base, 0);
    uint32_t at = base + incl - c;
    while (mask) {
        const int b = __builtin_ctz(mask);
        list[at++] = first + (uint32_t)b;
        mask &= mask - 1u;
    }
}

__global__ __launch_bounds__(256) void update_dirty_list_kernel(const uint32_t* __restrict__ dirty, uint32_t n_words,
                                                                uint32_t* __restrict__ sub, uint32_t* __restrict__ tile,
                                                                uint32_t* __restrict__ counts) {
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t m = w < n_words ? dirty[w] : 0u;
    uint32_t tm = 0;  // tile i of the word's 16: its sub-tiles 2 i, 2 i + 1
#pragma unroll
    for (int i = 0; i < 16; ++i) tm |= ((m >> (2 * i)) & 3u) ? (1u << i) : 0u;
    emit_bits(m, 32u * w, sub, counts, lane);
    emit_bits(tm, 16u * w, tile, counts + 1, lane);
}

}  // namespace

void launch_update_hits(const uint64_t* d_labels, size_t n, const uint64_t* d_keys, const uint32_t* d_perm, uint32_t n_keys,
                        uint64_t* d_cnt, uint64_t* d_total, uint64_t* d_hit_pos, uint32_t* d_hit_req, size_t cap, int grid,
                        hipStream_t stream) {
    if (n == 0 || n_keys == 0) return;
    const uint32_t stride = (n_keys + UP_LDS_KEYS - 1) / UP_LDS_KEYS;  // 1: the whole request sits in LDS
    const size_t steps = (n / 2 + 64 * UP_UNROLL - 1) / (64 * UP_UNROLL);  // wave steps
    const size_t blocks = std::max<size_t>(1, std::min<size_t>((steps + 3) / 4, (size_t)std::max(grid, 1)));
    hipLaunchKernelGGL(update_hits_kernel, dim3((unsigned)blocks), dim3(UP_THREADS), 0, stream, d_labels, n, d_keys, d_perm, n_keys, stride,
                       reinterpret_cast<unsigned long long*>(d_cnt), reinterpret_cast<unsigned long long*>(d_total), d_hit_pos,
                       d_hit_req, cap);
}

void launch_update_scatter(void* d_x, int rt, size_t n_rows, const uint64_t* d_pos, const uint32_t* d_req, size_t n_hits,
                           const float* d_v, uint32_t req_lo, uint32_t req_hi, uint32_t* d_dirty, hipStream_t stream) {
    if (n_hits == 0) return;
    const dim3 grid((unsigned)((n_hits + 3) / 4));
    const f32x4* v = reinterpret_cast<const f32x4*>(d_v);
    if (rt == ROW_BF16)
        hipLaunchKernelGGL(update_scatter_kernel<ROW_BF16>, grid, dim3(256), 0, stream, d_x, n_rows, d_pos, d_req, n_hits, v, req_lo, req_hi,
                           d_dirty);
    else
        hipLaunchKernelGGL(update_scatter_kernel<ROW_F32>, grid, dim3(256), 0, stream, d_x, n_rows, d_pos, d_req, n_hits, v, req_lo, req_hi,
                           d_dirty);
}

void launch_update_dirty_list(const uint32_t* d_dirty, uint32_t n_words, uint32_t* d_sub, uint32_t* d_tile, uint32_t* d_counts,
                              hipStream_t stream) {
    if (n_words == 0) return;
    hipLaunchKernelGGL(update_dirty_list_kernel, dim3((n_words + 255) / 256), dim3(256), 0, stream, d_dirty, n_words, d_sub, d_tile,
                       d_counts);
}

}  // namespace dawn
