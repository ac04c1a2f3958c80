// composite.hip — per-tile front-to-back alpha composite.
//
// One 256-lane workgroup per 16x16 tile, one pixel per lane, each wave an
// 8x8 quadrant.  Lists are binned per 32x32 bin (2x2 tiles: 2.35 instead of
// 4.38 pairs per splat, so sorting is cheaper); the four tiles of a bin are
// consecutive workgroups on one XCD and share the bin list through its L2.
// The list is streamed through LDS in batches of 256 records (one 48-B record
// gathered per lane), software-pipelined: the next batch is in flight into
// registers while the current one is composited.  Per batch every wave
// compacts the records whose pixel rect overlaps its quadrant (64 per
// ballot) and walks only those, two at a time with both records' LDS reads
// issued first: coverage (K6 closed form), gaussian + 0.01 cutoff (F1,
// tile.metal:191-197) and the composite (A1, tile.metal:251-266; or the live
// 50-layer rule, 50layer.metal:208-222).  A finer per-quadrant ellipse test
// was measured and removed: it cost more VALU than the bodies it skipped.
// The per-pixel body is branch-free (a non-covering splat contributes an
// exact zero), a wave leaves the batch once all 64 of its pixels are
// saturated, and the workgroup stops fetching once all 256 are.
// Bins are dealt to workgroups XCD-aware: the four tiles of a bin run on
// one XCD and share the bin's list through its L2.
//
// The kernels' bodies live in composite_kernels.h: the depth and feature
// kernels (composite_depth.hip, composite_features.hip) are the same code with
// another values policy.  This file holds the colour kernels and their launcher.
#include "composite_kernels.h"

namespace gs {

bool composite_strip(uint32_t bins) { return bins > kStripMinBins; }

// The colour kernels: the bodies of composite_kernels.h with the ColourValues
// policy (MODE, CAP, SLAB and PASS are described there).
template <int MODE, bool CAP, int SLAB = 0, int PASS = 0>
GS_COMPOSITE_KERNEL(MODE == 3 ? 4 : ColourValues::kWaves) composite_kernel(CompositeArgs a, uint32_t nwg) {
    composite_tile_body<MODE, CAP, SLAB, PASS>(a, nwg, ColourValues{});
}

template <int MODE, int PASS>
GS_COMPOSITE_KERNEL(GS_STRIP_WAVES) composite_strip_kernel(CompositeArgs a, uint32_t nwg) {
    composite_strip_body<MODE, PASS>(a, nwg, ColourValues{});
}

template <int MODE, bool CAP, int SLAB = 0, int PASS = 0>
static hipError_t launch_mode(const CompositeArgs& a, hipStream_t st, hipEvent_t t0 = nullptr,
                              hipEvent_t t1 = nullptr) {
    // (the strip kernel: tile and live50 rules without cap or slabs)
    if constexpr ((MODE == 0 || MODE == 1) && !CAP && SLAB == 0)
        return launch_composite_kernels(composite_kernel<MODE, CAP, SLAB, PASS>, composite_strip_kernel<MODE, PASS>, a, st, t0,
                                        t1);
    else
        return launch_composite_kernels(composite_kernel<MODE, CAP, SLAB, PASS>, nullptr, a, st, t0, t1);
}

hipError_t launch_composite(const CompositeArgs& a, int mode, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    const bool cap = a.cap > 0;
    // depth frames: the depth kernels (composite_depth.hip); no cap, slabs or MLAB there
    if (a.depth_out) return launch_composite_depth(a, mode, st, t0, t1);
    if (cap && !a.thr) return hipErrorInvalidValue;
    if (a.order && (a.rows || a.compact || a.nrows != a.tiles_y)) return hipErrorInvalidValue;  // (whole frames only)
    if (a.pass) {  // depth-cut frames: tile / live50 rules, no cap, no depth slabs (owned rows allowed)
        if (cap || a.slab || (!a.out && !a.out_bgra8) || !a.qrec || !a.state ||
            (mode != 0 && mode != 1) || a.pass > 2 || (a.pass == 1 && !a.open_q_count))
            return hipErrorInvalidValue;
        if (a.pass == 1)
            return mode == 0 ? launch_mode<0, false, 0, 1>(a, st, t0, t1) : launch_mode<1, false, 0, 1>(a, st, t0, t1);
        return mode == 0 ? launch_mode<0, false, 0, 2>(a, st, t0, t1) : launch_mode<1, false, 0, 2>(a, st, t0, t1);
    }
    if (a.slab) {  // full frame, no cap
        if (cap || a.rows || a.compact || a.out_bgra8 || (a.slab == 1 ? !a.t_out : (!a.out || (a.slab_rank && !a.t_all))))
            return hipErrorInvalidValue;
        if (a.slab == 1) return mode == 0 ? launch_mode<0, false, 1>(a, st, t0, t1) : launch_mode<1, false, 1>(a, st, t0, t1);
        if (a.slab == 2) return mode == 0 ? launch_mode<0, false, 2>(a, st, t0, t1) : launch_mode<1, false, 2>(a, st, t0, t1);
        return hipErrorInvalidValue;
    }
    if (mode == 2) return cap || !a.dkey ? hipErrorInvalidValue : launch_mode<3, false>(a, st, t0, t1);  // MLAB
    if (mode == 0) return cap ? launch_mode<0, true>(a, st, t0, t1) : launch_mode<0, false>(a, st, t0, t1);
    return cap ? launch_mode<1, true>(a, st, t0, t1) : launch_mode<1, false>(a, st, t0, t1);
}

__global__ __launch_bounds__(256) void cut_finalize_kernel(const uint32_t* __restrict__ qrec,
                                                           const uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ dkey, uint32_t* __restrict__ cut,
                                                           uint32_t nbins, uint32_t tiles_x, const RowOwnership own,
                                                           uint32_t margin, const CutFallback fb) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    const bool any_open = fb.cut_in && *fb.open != 0ull;
    if (fb.cut_in && b == 0) {
        *fb.n = any_open ? *fb.npairs : 0u;
        *fb.kept = 0u;
        if (fb.host_open) *fb.host_open = *fb.open;
    }
    if (b >= nbins) return;
    if (!owns_bin_row(b / tiles_x, own)) {  // (another rank's bin: no record, no pairs)
        cut[b] = 0u;
        if (fb.cut_in) {
            fb.table[b] = 0xFFFFFFFFu;
            if (any_open) fb.ranges[b] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        }
        return;
    }
    const uint4* q = reinterpret_cast<const uint4*>(qrec + (size_t)b * kQrecWords);  // (the bin's 16 positions, 16 flags)
    uint32_t p = 0u, open = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 v = q[i];
        p = max(p, max(max(v.x, v.y), max(v.z, v.w)));
        const uint4 f = q[4 + i];
        open |= f.x | f.y | f.z | f.w;
    }
    uint32_t c = 0u;
    if (p == 0xFFFFFFFFu) c = 0xFFFFu;
    else if (p > 0u) c = min(dkey[vals[p - 1u]] + margin, 0xFFFFu);
    cut[b] = c;
    if (fb.cut_in) {
        fb.table[b] = open ? fb.cut_in[b] : 0xFFFFFFFFu;
        if (any_open) fb.ranges[b] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    }
}

hipError_t launch_cut_finalize(const uint32_t* qrec, const uint32_t* vals, const uint32_t* dkey, uint32_t* cut_out,
                               uint32_t nbins, uint32_t tiles_x, const RowOwnership& own, uint32_t margin,
                               hipStream_t st, const CutFallback& fb) {
    if (nbins == 0) return hipSuccess;
    if (tiles_x == 0) return hipErrorInvalidValue;
    if (fb.cut_in && (!fb.open || !fb.npairs || !fb.table || !fb.n || !fb.kept || !fb.ranges))
        return hipErrorInvalidValue;
    cut_finalize_kernel<<<(nbins + 255) / 256, 256, 0, st>>>(qrec, vals, dkey, cut_out, nbins, tiles_x, own, margin,
                                                             fb);
    return hipGetLastError();
}

// Longest-first bin order (launch_order_bins): one 1024-lane workgroup, a
// counting sort of the bins into 128 cost buckets (log2 with two mantissa
// bits), costliest first.
__global__ __launch_bounds__(1024) void order_bins_kernel(const uint32_t* __restrict__ wcost, uint32_t nbins,
                                                          uint32_t* __restrict__ order) {
    constexpr int kB = 128;
    __shared__ uint32_t cnt[kB];
    __shared__ uint8_t bk[kOrderMaxBins];  // each bin's bucket, between the two phases
    static_assert(kOrderMaxBins + kB * 4 <= kLdsBytes, "order_bins_kernel's LDS exceeds a gfx950 workgroup's");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < kB) cnt[tid] = 0u;
    __syncthreads();
    for (uint32_t b = tid; b < nbins; b += 1024u) {
        const uint2 c2 = reinterpret_cast<const uint2*>(wcost)[b];  // (the bin's two halves)
        const uint32_t cost = c2.x + c2.y;
        uint32_t k = 0u;
        if (cost) {
            const uint32_t e = 31u - (uint32_t)__builtin_clz(cost);  // <= 31
            const uint32_t m = e >= 2u ? (cost >> (e - 2u)) & 3u : (cost << (2u - e)) & 3u;
            k = min(1u + e * 4u + m, (uint32_t)kB - 1u);
        }
        bk[b] = (uint8_t)k;
        atomicAdd(&cnt[k], 1u);
    }
    __syncthreads();
    if (tid < 64u) {  // exclusive offsets, costliest bucket first: one wave, two buckets a lane
        const uint32_t hi = cnt[kB - 1 - 2 * lane], lo = cnt[kB - 2 - 2 * lane];
        const uint32_t inc = wave_scan_dpp<false>(hi + lo);
        cnt[kB - 1 - 2 * lane] = inc - hi - lo;
        cnt[kB - 2 - 2 * lane] = inc - lo;
    }
    __syncthreads();
    for (uint32_t b = tid; b < nbins; b += 1024u) order[atomicAdd(&cnt[bk[b]], 1u)] = b;
}

__global__ __launch_bounds__(256) void cut_dilate_kernel(const uint32_t* __restrict__ cut, uint32_t* __restrict__ out,
                                                         uint32_t tiles_x, uint32_t tiles_y, int r) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= tiles_x * tiles_y) return;
    const int by = (int)(b / tiles_x), bx = (int)(b - (uint32_t)by * tiles_x);
    const int y0 = max(by - r, 0), y1 = min(by + r, (int)tiles_y - 1);
    const int x0 = max(bx - r, 0), x1 = min(bx + r, (int)tiles_x - 1);
    uint32_t m = 0u;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) m = max(m, cut[(uint32_t)y * tiles_x + (uint32_t)x]);
    out[b] = m;
}

hipError_t launch_cut_dilate(const uint32_t* cut, uint32_t* out, uint32_t tiles_x, uint32_t tiles_y, int r,
                             hipStream_t st) {
    const uint32_t n = tiles_x * tiles_y;
    if (n == 0) return hipSuccess;
    if (!cut || !out || r < 0) return hipErrorInvalidValue;
    cut_dilate_kernel<<<(n + 255) / 256, 256, 0, st>>>(cut, out, tiles_x, tiles_y, r);
    return hipGetLastError();
}

hipError_t launch_order_bins(const uint32_t* wcost, uint32_t nbins, uint32_t* order, hipStream_t st) {
    if (nbins == 0) return hipSuccess;
    if (!wcost || !order || nbins > kOrderMaxBins) return hipErrorInvalidValue;
    order_bins_kernel<<<1, 1024, 0, st>>>(wcost, nbins, order);
    return hipGetLastError();
}

#ifdef GS_COMPOSITE_TRACE
extern "C" int gs_debug_composite_trace(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_comp_trace), (size_t)n * 8) == hipSuccess ? 0 : -1;
}
#endif

hipError_t launch_cap_threshold(const CompositeArgs& a, hipStream_t st) {
    if (a.cap <= 0 || !a.thr_out) return hipErrorInvalidValue;
    return launch_mode<2, false>(a, st);
}

}  // namespace gs
