// index_lookup.hip — rows by label (dawn_index_get, dawn_index_search_like).  Labels are not unique: for a probe
// label L, count(L) is the number of rows holding it and first(L) the lowest position holding it (the earliest-added row, the
// row ties in search go to).  Three launches:
//   lookup  (after a one-workgroup launch that empties the slots) one read of the label array [0, n) for up to LK_PROBES probe labels.  Every workgroup loads the probes and sorts them
//           in LDS (a rank sort over (label, probe index): repeats and any order are fine), then every row binary-searches its
//           label there, as compact_mark_kernel does with the removal list.  A hit counts into the slot of the probe's FIRST
//           occurrence in the request.  The lanes of a wave that hit one slot issue one 64-bit atomicAdd (count) and one 64-bit
//           atomicMin (first), and a wave carries its last slot's sums in registers from step to step: an index where every row
//           holds one label costs one pair of atomics per wave, not one per row;
//   gather  query b: the first row of its slot as f32 (a bf16 row widened exactly: bits << 16), or — the label is missing — the
//           fill row and a flag;
//   fixup   found[b] = 0 for the flagged queries, behind the search (index_search_on_device, unchanged).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"
#include "wave_topk.hpp"

namespace dawn {
namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LK_THREADS = 256;
constexpr int LK_UNROLL = 4;  // 16-B label loads in flight per lane (8 rows)

// What a wave has summed for one slot and not published yet (wave-uniform).
struct SlotRun {
    int slot = -1;
    unsigned long long cnt = 0, first = ~0ull;
};

__device__ __forceinline__ void run_flush(SlotRun& run, unsigned long long* __restrict__ first,
                                          unsigned long long* __restrict__ count, int lane) {
    if (run.slot >= 0 && lane == 0) {
        atomicAdd(count + run.slot, run.cnt);
        atomicMin(first + run.slot, run.first);
    }
    run.slot = -1;
}

// One row per lane (rows increase with the lane; `valid` = the lane holds a row): look the label up, aggregate the hits per slot.
__device__ __forceinline__ void lookup_round(uint64_t lab, bool valid, size_t row0, size_t row_stride, const uint64_t* sh_key,
                                             const uint32_t* sh_slot, uint32_t n_probes, uint64_t key_lo, uint64_t key_hi,
                                             SlotRun& run, unsigned long long* __restrict__ first,
                                             unsigned long long* __restrict__ count, int lane) {
    int slot = -1;
    if (valid && lab >= key_lo && lab <= key_hi) {
        uint32_t lo = 0, hi = n_probes;  // first sorted probe >= lab
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (sh_key[mid] < lab) lo = mid + 1;
            else hi = mid;
        }
        if (lo < n_probes && sh_key[lo] == lab) slot = (int)sh_slot[lo];
    }
    unsigned long long hits = __ballot(slot >= 0);
    while (hits) {
        const int leader = __builtin_ctzll(hits);
        const int s = __shfl(slot, leader);
        const unsigned long long same = __ballot(slot == s);
        const unsigned long long r = (unsigned long long)(row0 + (size_t)leader * row_stride);  // (the lowest row of the group)
        if (s == run.slot) {
            run.cnt += (unsigned long long)__builtin_popcountll(same);
            run.first = min(run.first, r);
        } else {
            run_flush(run, first, count, lane);
            run.slot = s;
            run.cnt = (unsigned long long)__builtin_popcountll(same);
            run.first = r;
        }
        hits &= ~same;
    }
}

// The slots start empty: a kernel rather than memsets, so a captured sequence is kernel nodes only, in stream order.
__global__ __launch_bounds__(LK_PROBES) void label_slots_init_kernel(unsigned long long* __restrict__ first,
                                                                     unsigned long long* __restrict__ count, uint32_t n_probes) {
    if (threadIdx.x < n_probes) {
        first[threadIdx.x] = ~0ull;
        count[threadIdx.x] = 0;
    }
}

__global__ __launch_bounds__(LK_THREADS) void label_lookup_kernel(const uint64_t* __restrict__ labels, size_t n,
                                                                  const uint64_t* __restrict__ probes, uint32_t n_probes,
                                                                  unsigned long long* __restrict__ first,
                                                                  unsigned long long* __restrict__ count) {
    __shared__ uint64_t sh_raw[LK_PROBES];
    __shared__ uint64_t sh_key[LK_PROBES];
    __shared__ uint32_t sh_slot[LK_PROBES];
    for (uint32_t i = threadIdx.x; i < n_probes; i += LK_THREADS) sh_raw[i] = probes[i];
    __syncthreads();
    // rank of (label, index) among the probes: equal labels keep request order, so the first of a run of equal sorted labels
    // carries the index of the label's first occurrence — the slot every occurrence shares
    for (uint32_t i = threadIdx.x; i < n_probes; i += LK_THREADS) {
        const uint64_t v = sh_raw[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n_probes; ++j) {
            const uint64_t w = sh_raw[j];
            rank += (w < v || (w == v && j < i)) ? 1u : 0u;
        }
        sh_key[rank] = v;
        sh_slot[rank] = i;
    }
    __syncthreads();
    const uint64_t key_lo = sh_key[0], key_hi = sh_key[n_probes - 1];
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * (LK_THREADS / 64) + (threadIdx.x >> 6);
    const size_t n_waves = (size_t)gridDim.x * (LK_THREADS / 64);
    const size_t n_pairs = n / 2;
    const u64x2* __restrict__ lab2 = reinterpret_cast<const u64x2*>(labels);
    SlotRun run;
    // a wave step: LK_UNROLL x 64 consecutive label pairs, lane l holding pairs base + 64 u + l
    for (size_t base = wave * (64 * LK_UNROLL); base < n_pairs; base += n_waves * (64 * LK_UNROLL)) {
        u64x2 v[LK_UNROLL];
#pragma unroll
        for (int u = 0; u < LK_UNROLL; ++u) {
            const size_t p = base + (size_t)(64 * u + lane);
            v[u] = p < n_pairs ? __builtin_nontemporal_load(lab2 + p) : u64x2{0, 0};
        }
#pragma unroll
        for (int u = 0; u < LK_UNROLL; ++u) {
            const size_t p0 = base + (size_t)(64 * u);
            const bool valid = p0 + (size_t)lane < n_pairs;
            lookup_round(v[u].x, valid, 2 * p0, 2, sh_key, sh_slot, n_probes, key_lo, key_hi, run, first, count, lane);
            lookup_round(v[u].y, valid, 2 * p0 + 1, 2, sh_key, sh_slot, n_probes, key_lo, key_hi, run, first, count, lane);
        }
    }
    if ((n & 1) && wave == 0)  // the odd last row
        lookup_round(lane == 0 ? labels[n - 1] : 0, lane == 0, n - 1, 1, sh_key, sh_slot, n_probes, key_lo, key_hi, run, first,
                     count, lane);
    run_flush(run, first, count, lane);
}

// One workgroup per query: rows[b] = the first row of ids[b]'s slot as f32, or the fill row (unit: e_0; else zeros), missing[b].
template <int RT>
__global__ __launch_bounds__(128) void label_gather_kernel(const void* __restrict__ x, const uint64_t* __restrict__ ids,
                                                           const unsigned long long* __restrict__ first,
                                                           const unsigned long long* __restrict__ count, float* __restrict__ rows,
                                                           uint32_t* __restrict__ missing, int unit_fill, size_t n_rows) {
    const uint32_t b = blockIdx.x;
    const uint64_t id = ids[b];
    uint32_t s = b;  // the slot: the first occurrence of the label in the request
    for (uint32_t j = 0; j < b; ++j)
        if (ids[j] == id) {
            s = j;
            break;
        }
    const bool miss = count[s] == 0 || first[s] >= n_rows;  // (the second never holds after a lookup over these rows)
    f32x4* __restrict__ out = reinterpret_cast<f32x4*>(rows) + (size_t)b * ROW_F4;
    if (threadIdx.x == 0 && missing) missing[b] = miss ? 1u : 0u;
    if (miss) {
        for (int c = threadIdx.x; c < ROW_F4; c += 128) out[c] = f32x4{c == 0 && unit_fill ? 1.0f : 0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
    const size_t row = (size_t)first[s];
    if (RT == ROW_BF16) {
        const u32x4* __restrict__ xb = reinterpret_cast<const u32x4*>(x);
        for (int c = threadIdx.x; c < ROW_C8; c += 128) {
            const u32x4 w = xb[frag_chunk(row, c)];
            out[2 * c] = f32x4{bf16_lo(w.x), bf16_hi(w.x), bf16_lo(w.y), bf16_hi(w.y)};
            out[2 * c + 1] = f32x4{bf16_lo(w.z), bf16_hi(w.z), bf16_lo(w.w), bf16_hi(w.w)};
        }
    } else {
        const f32x4* __restrict__ xf = reinterpret_cast<const f32x4*>(x) + row * ROW_F4;
        for (int c = threadIdx.x; c < ROW_F4; c += 128) out[c] = xf[c];
    }
}

__global__ __launch_bounds__(256) void label_fixup_kernel(const uint32_t* __restrict__ missing, uint32_t B,
                                                          uint32_t* __restrict__ found) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < B && missing[b]) found[b] = 0;
}

}  // namespace

hipError_t launch_label_lookup(const uint64_t* d_labels, size_t n, const uint64_t* d_probes, uint32_t n_probes, uint64_t* d_first,
                               uint64_t* d_count, int grid, hipStream_t stream) {
    if (n_probes == 0 || n_probes > LK_PROBES) return n_probes == 0 ? hipSuccess : hipErrorInvalidValue;
    auto* f = reinterpret_cast<unsigned long long*>(d_first);
    auto* c = reinterpret_cast<unsigned long long*>(d_count);
    hipLaunchKernelGGL(label_slots_init_kernel, dim3(1), dim3(LK_PROBES), 0, stream, f, c, n_probes);
    if (n == 0) return hipGetLastError();
    const size_t steps = (n / 2 + 64 * LK_UNROLL - 1) / (64 * LK_UNROLL);  // wave steps
    const size_t blocks = std::max<size_t>(1, std::min<size_t>((steps + 3) / 4, (size_t)std::max(grid, 1)));
    hipLaunchKernelGGL(label_lookup_kernel, dim3((unsigned)blocks), dim3(LK_THREADS), 0, stream, d_labels, n, d_probes, n_probes, f, c);
    return hipGetLastError();
}

void launch_label_gather(const void* d_x, size_t n_rows, int rt, const uint64_t* d_probes, uint32_t n_probes, const uint64_t* d_first,
                         const uint64_t* d_count, float* d_rows, uint32_t* d_missing, bool unit_fill, hipStream_t stream) {
    if (n_probes == 0 || n_probes > LK_PROBES) return;
    const auto* f = reinterpret_cast<const unsigned long long*>(d_first);
    const auto* c = reinterpret_cast<const unsigned long long*>(d_count);
    if (rt == ROW_BF16)
        hipLaunchKernelGGL(label_gather_kernel<ROW_BF16>, dim3(n_probes), dim3(128), 0, stream, d_x, d_probes, f, c, d_rows,
                           d_missing, unit_fill ? 1 : 0, n_rows);
    else
        hipLaunchKernelGGL(label_gather_kernel<ROW_F32>, dim3(n_probes), dim3(128), 0, stream, d_x, d_probes, f, c, d_rows,
                           d_missing, unit_fill ? 1 : 0, n_rows);
}

void launch_label_fixup(const uint32_t* d_missing, uint32_t B, uint32_t* d_found, hipStream_t stream) {
    if (B == 0) return;
    hipLaunchKernelGGL(label_fixup_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, d_missing, B, d_found);
}

}  // namespace dawn
