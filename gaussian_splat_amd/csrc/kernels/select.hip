// select.hip — re-index the scene planes on the device (gs_select, gs_prune;
// DESIGN.md §7 "the scene after load").
//
// Two steps, neither on a frame's path:
//   mask -> ascending index list (gs_prune): one byte per splat in, the list
//     of the splats with a nonzero byte and its length out.  Blocks of
//     kSelectBlock bytes; a wave takes 256 consecutive bytes in four rounds
//     of 64, ranks its lanes with ballot + mbcnt, and the blocks' offsets
//     come from a scan of their totals (count -> scan -> emit: three
//     launches, no look-back, so no pass that can give up).  Integer
//     arithmetic only and every list position has one writer: the list is
//     the same on every run.
//   plane gather (both calls): new splat j loads index[j] once and moves
//     every plane entry of old splat index[j]: p0, p1, p2 (16 B each), p3
//     (8 B), the float4 SH planes (k-major) and the sh1 tail, all loads of a
//     lane issued before its stores.  An entry >= the old count never forms
//     an address: the lane raises *flag and moves nothing.
// LDS: the four wave totals of a compaction block (16 B), the scan's four
// wave sums; none in the gather.
#include "gs_kernels.h"
#include "gs_wave.h"

namespace gs {

namespace {

constexpr uint32_t kWaveItems = kSelectBlock / 4;  // bytes per wave (four waves per block)
constexpr int kRounds = kWaveItems / 64;
static_assert(kSelectBlock == 1024 && kRounds == 4, "four waves of four 64-byte rounds");

// The keep ballots of this wave's bytes: round r, lane l tests byte
// wave_base + 64 r + l.  Returns the wave's total.
__device__ __forceinline__ uint32_t keep_ballots(const uint8_t* __restrict__ keep, uint64_t n, uint64_t wave_base,
                                                 uint64_t (&mask)[kRounds]) {
    const uint32_t lane = lane_id();
    uint32_t total = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint64_t i = wave_base + (uint64_t)(64 * r) + lane;
        const bool f = i < n && keep[i] != 0;
        mask[r] = __ballot(f);
        total += (uint32_t)__popcll(mask[r]);
    }
    return total;
}

// counts[b] = kept bytes of block b.
__global__ __launch_bounds__(256) void select_count_kernel(const uint8_t* __restrict__ keep, uint32_t n,
                                                           uint32_t* __restrict__ counts) {
    __shared__ uint32_t wtot[4];
    const uint32_t wave = threadIdx.x >> 6;
    uint64_t mask[kRounds];
    const uint32_t t = keep_ballots(keep, n, (uint64_t)blockIdx.x * kSelectBlock + (uint64_t)wave * kWaveItems, mask);
    if ((threadIdx.x & 63u) == 0) wtot[wave] = t;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
}

// In place: v[0 .. nb) becomes its exclusive scan and v[nb] the total.  One
// workgroup, 1024 words per step (a 6M-splat mask has 5860 blocks: 6 steps).
__global__ __launch_bounds__(256) void select_scan_kernel(uint32_t* __restrict__ v, uint32_t nb) {
    __shared__ uint32_t tmp[4];
    uint32_t carry = 0;
    for (uint64_t base = 0; base < nb; base += 1024) {
        const uint64_t i = base + 4ull * threadIdx.x;
        uint32_t a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = i + k < nb ? v[i + k] : 0u;
        uint32_t total;
        uint32_t ex = carry + block256_exclusive_scan((a[0] + a[1]) + (a[2] + a[3]), tmp, &total);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < nb) v[i + k] = ex;
            ex += a[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) v[nb] = carry;
}

// index[offsets[b] + rank] = i for every kept byte i of block b, rank = the
// kept bytes of the block below i.
__global__ __launch_bounds__(256) void select_emit_kernel(const uint8_t* __restrict__ keep, uint32_t n,
                                                          const uint32_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ index) {
    __shared__ uint32_t wtot[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t wave_base = (uint64_t)blockIdx.x * kSelectBlock + (uint64_t)wave * kWaveItems;
    uint64_t mask[kRounds];
    const uint32_t t = keep_ballots(keep, n, wave_base, mask);
    if (lane == 0) wtot[wave] = t;
    __syncthreads();
    uint32_t at = offsets[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) at += wtot[w];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        // (a set bit implies i < n, and the ranks below n kept bytes stay below n: in bounds)
        if ((mask[r] >> lane) & 1ull) index[at + mbcnt(mask[r])] = (uint32_t)(wave_base + (uint64_t)(64 * r) + lane);
        at += (uint32_t)__popcll(mask[r]);
    }
}

// (a native vector: an array of them stays in registers once the plane loops unroll)
typedef float v4f __attribute__((ext_vector_type(4)));

// New splat j = old splat index[j].  NP4 float4 SH planes (+ the sh1 tail).
template <int NP4, bool TAIL>
__global__ __launch_bounds__(256) void select_gather_kernel(SceneDev src, const uint32_t* __restrict__ index,
                                                            ScenePlanes dst, uint32_t* __restrict__ flag) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= dst.n) return;
    const uint32_t i = index[j];
    const bool bad = i >= src.n;
    const uint64_t badmask = __ballot(bad);
    if (bad) {  // (no address is formed from i; one lane of the wave reports)
        if (mbcnt(badmask) == 0) atomicOr(flag, 1u);
        return;
    }
    const float4 a = src.p0[i], b = src.p1[i], c = src.p2[i];
    const float2 d = src.p3[i];
    const v4f* __restrict__ sp = reinterpret_cast<const v4f*>(src.sh4);
    v4f s[NP4 > 0 ? NP4 : 1];
#pragma unroll
    for (int k = 0; k < NP4; ++k) s[k] = sp[(size_t)k * src.n + i];
    float t = 0.0f;
    if (TAIL) t = src.sh1[i];
    dst.p0[j] = a;
    dst.p1[j] = b;
    dst.p2[j] = c;
    dst.p3[j] = d;
    v4f* __restrict__ dp = reinterpret_cast<v4f*>(dst.sh4);
#pragma unroll
    for (int k = 0; k < NP4; ++k) dp[(size_t)k * dst.n + j] = s[k];
    if (TAIL) dst.sh1[j] = t;
}

template <int NP4, bool TAIL>
hipError_t gather(const SceneDev& src, const uint32_t* index, const ScenePlanes& dst, uint32_t* flag, hipStream_t st) {
    const uint32_t blocks = (uint32_t)(((uint64_t)dst.n + 255) / 256);
    select_gather_kernel<NP4, TAIL><<<blocks, 256, 0, st>>>(src, index, dst, flag);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_select_compact(const uint8_t* keep, uint32_t n, uint32_t* offsets, uint32_t* index, hipStream_t st) {
    if (!offsets || (n > 0 && (!keep || !index))) return hipErrorInvalidValue;
    const uint32_t nb = select_blocks(n);
    if (nb) {
        select_count_kernel<<<nb, 256, 0, st>>>(keep, n, offsets);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    select_scan_kernel<<<1, 256, 0, st>>>(offsets, nb);  // (n = 0: the total alone)
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (nb) select_emit_kernel<<<nb, 256, 0, st>>>(keep, n, offsets, index);
    return hipGetLastError();
}

hipError_t launch_select_gather(const SceneDev& src, int sh_degree, const uint32_t* index, const ScenePlanes& dst,
                                uint32_t* flag, hipStream_t st) {
    if (dst.n == 0) return hipSuccess;
    if (!index || !flag || !src.p0 || !src.p1 || !src.p2 || !src.p3 || !dst.p0 || !dst.p1 || !dst.p2 || !dst.p3)
        return hipErrorInvalidValue;
    if (sh_degree > 0 && (!src.sh4 || !dst.sh4)) return hipErrorInvalidValue;
    if ((sh_degree == 1 || sh_degree == 3) && (!src.sh1 || !dst.sh1)) return hipErrorInvalidValue;
    switch (sh_degree) {
        case 0: return gather<0, false>(src, index, dst, flag, st);
        case 1: return gather<2, true>(src, index, dst, flag, st);
        case 2: return gather<6, false>(src, index, dst, flag, st);
        case 3: return gather<11, true>(src, index, dst, flag, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace gs
