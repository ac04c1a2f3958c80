// composite_features.hip — per-splat feature channels composited per pixel
// (gs_render_features).
//
// The caller's features are an N x K float matrix, row i for splat i.  Every
// channel F_k is composited exactly as a colour channel whose per-splat value
// is features[i][k]: the same fragments, order, weights and break rule as
// C0..C2,
//   tile rule:   F_k = fma(f, sa, F_k), sa = alpha * T
//   live50 rule: F_k = fma(f, T, F_k)
// from F_k = 0, not clamped, not normalised; termination depends on T alone.
//
// One launch composites four channels, first .. first + 3, into the
// H x W x K image (channels innermost): T and four accumulators per pixel, no
// colour.  A frame queues ceil(K / 4) launches behind its colour composite,
// over the same whole lists (pass 0: feature frames carry no depth cuts).
//
// composite_feat_kernel and composite_strip_feat_kernel are
// composite_depth_kernel<MODE, 0> and composite_strip_depth_kernel<MODE, 0>
// (composite_depth.hip) with the three colours and the depth replaced by the
// four feature values:
//  - the record's own r, g, b are ignored; the owner lane of each record
//    gathers the splat's four values together with the batch's rc[] chunks
//    (in flight while the batch before it is composited, never loaded after
//    the barrier) and stages them in the slot's value words (tile kernel:
//    b.w, c.x, c.y, c.z; strip kernel: its three value words and a 1-KB side
//    array);
//  - VIN: one 16-B load per record (K % 4 == 0 and a 16-B aligned matrix),
//    else dword loads of the launch's valid channels only: a tail channel
//    past K is never loaded (for the last splat it lies past the matrix);
//  - VOUT: one 16-B store per pixel (K % 4 == 0 and a 16-B aligned image),
//    else dword stores of the valid channels only;
//  - id * K + k and pixel * K + k are 64-bit (50M splats x 64 channels);
//  - no fetch counter, no cut records, no state planes.
// Both forms are picked on the host per launch (template parameters).
// Kernels of their own in a file of their own: the colour and depth kernels'
// code and register budgets stay what they were, and colour and depth frames
// never launch anything from here.
#include <hip/hip_ext.h>

#include <type_traits>

#include "gs_kernels.h"
#include "gs_wave.h"

namespace gs {

namespace {

// One 48-B LDS slot per staged record (first the raw gathered record):
//   a = (U0, V0, Ax', -Ay')   b = (Bx', -By', opacity, f0)   c = (f1, f2, f3, -)
struct StagedRecF {
    float4 a, b, c;
};
static_assert(sizeof(StagedRecF) == 48, "staged record slot");
__device__ __forceinline__ const StagedRecF& staged_at(const StagedRecF* base, uint32_t off) {
    return *reinterpret_cast<const StagedRecF*>(reinterpret_cast<const char*>(base) + off);
}

constexpr int kFeatSgprs = 62;  // the 80-SGPR allocation class (composite.hip, GS_COMPOSITE_SGPRS)
// waves per SIMD the feature composites are built for: the depth composites'
// class (composite_depth.hip kDepthWaves)
constexpr int kFeatWaves = 6;

// The four values of splat `id` in this launch's channels.  VIN: rows are
// 16-B aligned and whole (K % 4 == 0).  Otherwise only the channels below K
// are read (nch of them, wave-uniform), the rest are 0.
template <bool VIN>
__device__ __forceinline__ float4 load_features(const FeatureArgs& f, uint32_t id, uint32_t nch) {
    const float* row = f.feat + ((size_t)id * (size_t)(uint32_t)f.channels + (size_t)(uint32_t)f.first);
    if constexpr (VIN) {
        return *reinterpret_cast<const float4*>(row);
    } else {
        float4 v = make_float4(row[0], 0.0f, 0.0f, 0.0f);
        if (nch > 1u) v.y = row[1];
        if (nch > 2u) v.z = row[2];
        if (nch > 3u) v.w = row[3];
        return v;
    }
}

// The four accumulators of pixel `pix` into the image's channels first .. first + 3.
template <bool VOUT>
__device__ __forceinline__ void store_features(const FeatureArgs& f, size_t pix, uint32_t nch, float F0, float F1,
                                               float F2, float F3) {
    float* o = f.out + (pix * (size_t)(uint32_t)f.channels + (size_t)(uint32_t)f.first);
    if constexpr (VOUT) {
        *reinterpret_cast<float4*>(o) = make_float4(F0, F1, F2, F3);
    } else {
        o[0] = F0;
        if (nch > 1u) o[1] = F1;
        if (nch > 2u) o[2] = F2;
        if (nch > 3u) o[3] = F3;
    }
}

}  // namespace

// composite_depth_kernel<MODE, 0> with four feature accumulators in place of
// (C0, C1, C2, D); whole frames (every bin row, no band).
template <int MODE, bool VIN, bool VOUT>
__global__ __launch_bounds__(256, kFeatWaves) __attribute__((amdgpu_num_sgpr(kFeatSgprs))) void composite_feat_kernel(
    CompositeArgs a, FeatureArgs f, uint32_t nwg) {
    static_assert(MODE == 0 || MODE == 1, "feature composite: tile / live50 rules");
    __shared__ StagedRecF srec[kTileThreads];
    __shared__ uint16_t wlist[4][kTileThreads];  // per wave: slot byte offsets
    __shared__ uint8_t sqm[kTileThreads];        // per staged record: the quadrants it may reach
    __shared__ uint32_t sopen[4];                // per wave: pixels still open after its last walk

    // XCD-aware bijective remap, bins and tiles as composite_kernel
    const uint32_t orig = blockIdx.x;
    const uint32_t full = nwg & ~31u;
    const uint32_t kk = orig >> 3;
    const uint32_t wg = orig < full ? 32u * (kk >> 2) + 4u * (orig & 7u) + (kk & 3u) : orig;
    const uint32_t per_row = 4u * (uint32_t)a.tiles_x;
    const int by = (int)(wg / per_row);
    const uint32_t k4 = wg - (uint32_t)by * per_row;
    const int bx = (int)(k4 >> 2);
    const int tx = 2 * bx + (int)(k4 & 1u), ty = 2 * by + (int)((k4 >> 1) & 1u);
    const int width = a.width, height = a.height;
    const uint32_t bin = (uint32_t)(by * a.tiles_x + bx);
    const int tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lane = tid & 63;
    const uint32_t tx0 = (uint32_t)(tx * kTile), ty0 = (uint32_t)(ty * kTile);
    const uint32_t lxi = (wave & 1u) * 8u + (lane & 7u), lyi = (wave >> 1) * 8u + (lane >> 3);
    const int px = (int)(tx0 + lxi);
    const int py = (int)(ty0 + lyi);
    const bool inside = px < width && py < height;
    const float lx = (float)lxi + 0.5f;  // tile-local pixel centre (exact)
    const float ly = (float)lyi + 0.5f;
    const float ftx0 = (float)tx0, fty0 = (float)ty0;
    // channels of this launch that exist (1..4; 4 with VIN / VOUT)
    const uint32_t nch = (uint32_t)(f.channels - f.first) < 4u ? (uint32_t)(f.channels - f.first) : 4u;

    uint2 rg = decode_range(a.ranges[bin]);
    if (tx0 >= (uint32_t)width || ty0 >= (uint32_t)height) rg.y = rg.x;
    // pixels outside the frame start finished (T = 0), see composite_kernel
    float T = inside ? 1.0f : 0.0f;
    float F0 = 0.0f, F1 = 0.0f, F2 = 0.0f, F3 = 0.0f;
    auto finished = [&]() -> bool {
        if constexpr (MODE == 0) return T <= kTSat;
        else return T < kTMin;
    };
    // one record at this lane's pixel (composite_kernel's body_v), its four values in bb.w, cc.xyz
    auto body_v = [&](const float4 aa, const float4 bb, const float4 cc) {
        const float u = __builtin_fmaf(aa.z, lx, __builtin_fmaf(aa.w, ly, aa.x));
        const float v = __builtin_fmaf(bb.x, lx, __builtin_fmaf(bb.y, ly, aa.y));
        const float qq = __builtin_fmaf(v, v, u * u);
        const bool covered = fmaxf(fabsf(u), fabsf(v)) <= kBoxS && qq <= kQMaxS;
        if (!finished() && covered) {
            const float alpha = bb.z * gs_gauss2(qq);
            if constexpr (MODE == 0) {
                const float sa = alpha * T;
                F0 = __builtin_fmaf(bb.w, sa, F0);
                F1 = __builtin_fmaf(cc.x, sa, F1);
                F2 = __builtin_fmaf(cc.y, sa, F2);
                F3 = __builtin_fmaf(cc.z, sa, F3);
                T = T - sa;
            } else {
                F0 = __builtin_fmaf(bb.w, T, F0);
                F1 = __builtin_fmaf(cc.x, T, F1);
                F2 = __builtin_fmaf(cc.y, T, F2);
                F3 = __builtin_fmaf(cc.z, T, F3);
                T = T * (1.0f - alpha);
            }
        }
    };
    auto body = [&](uint32_t off) {
        const StagedRecF& r = staged_at(srec, off);
        body_v(r.a, r.b, r.c);
    };

    // Software pipeline and coalesced gathers as composite_kernel; the owner
    // lane of each record also loads its four feature values (fc) with the chunks.
    const uint32_t last = rg.y > rg.x ? rg.y - 1u : rg.x;
    uint32_t ck[3], cp[3];  // this lane's chunks: record (in the wave's 64) and part
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint32_t c = lane + 64u * (uint32_t)i;
        ck[i] = c / 3u;
        cp[i] = c - 3u * ck[i];
    }
    float4 rc[3] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f),
                    make_float4(0.f, 0.f, 0.f, 0.f)};
    float4 fc = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t id_cur = 0, id_next = 0;
    auto gather = [&](uint32_t own_id) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t idk = (uint32_t)__shfl((int)own_id, (int)ck[i], 64);
            rc[i] = a.rec[(size_t)a.rec_stride * idk + cp[i]];
        }
        fc = load_features<VIN>(f, own_id, nch);
    };
    if (rg.y > rg.x) {
        const uint32_t j = rg.x + tid;
        id_cur = a.vals[j < last ? j : last];
        gather(id_cur);
        id_next = a.vals[j + kTileThreads < last ? j + kTileThreads : last];
    }
    for (uint32_t b = rg.x; b < rg.y; b += kTileThreads) {
        if (b != rg.x) {
            const bool open = __ballot(!finished()) != 0;
            if (lane == 0) sopen[wave] = open ? 1u : 0u;
            block_lds_sync();
            const uint4 o = *reinterpret_cast<const uint4*>(sopen);
            if ((o.x | o.y | o.z | o.w) == 0u) break;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) reinterpret_cast<float4*>(srec)[192u * wave + lane + 64u * (uint32_t)i] = rc[i];
        wave_lds_sync();  // the wave's 64 slots are only touched by this wave until the barrier
        if (b + tid < rg.y) {
            StagedRecF& st = srec[tid];
            const float4 r0 = st.a, r1 = st.b, r2 = st.c;
            const float ax = r0.z * kConicScale, ay = r0.w * kConicScale;
            const float bxs = r1.x * kConicScale, bys = r1.y * kConicScale;
            const float ex = ftx0 - r0.x, ey = r0.y - fty0;
            st.a = make_float4(__builtin_fmaf(ax, ex, ay * ey), __builtin_fmaf(bxs, ex, bys * ey), ax, -ay);
            st.b = make_float4(bxs, -bys, r1.z, fc.x);
            st.c = make_float4(fc.y, fc.z, fc.w, 0.0f);
            const uint32_t wlo = __float_as_uint(r2.z), whi = __float_as_uint(r2.w);
            const uint32_t lo = rect_coords(wlo, a.cell_mask), hi = rect_coords(whi, a.cell_mask);
            const uint32_t x0 = lo & 0xFFFFu, y0 = lo >> 16, x1 = hi & 0xFFFFu, y1 = hi >> 16;
            const bool c0 = !(x1 < tx0 || x0 > tx0 + 7u), c1 = !(x1 < tx0 + 8u || x0 > tx0 + 15u);
            const bool w0 = !(y1 < ty0 || y0 > ty0 + 7u), w1 = !(y1 < ty0 + 8u || y0 > ty0 + 15u);
            uint32_t qm = (uint32_t)(c0 && w0) | (uint32_t)(c1 && w0) << 1 | (uint32_t)(c0 && w1) << 2 |
                          (uint32_t)(c1 && w1) << 3;
            if (a.cell_mask && qm) {
                const uint32_t cm = rect_cell_mask(wlo, whi);
#pragma unroll
                for (uint32_t w = 0; w < 4; ++w) {
                    const uint32_t dcx = (tx0 >> 3) + (w & 1u) - (x0 >> 3), dcy = (ty0 >> 3) + (w >> 1) - (y0 >> 3);
                    if (dcx < 4u && dcy < 4u && ((cm >> (dcy * 4u + dcx)) & 1u)) qm &= ~(1u << w);
                }
            }
            sqm[tid] = (uint8_t)qm;
        }
        __syncthreads();
        {
            const uint32_t j = b + 2u * kTileThreads + tid;
            id_cur = id_next;
            gather(id_cur);
            id_next = a.vals[j < last ? j : last];
        }
        const uint32_t cnt_b = rg.y - b < (uint32_t)kTileThreads ? rg.y - b : (uint32_t)kTileThreads;
        uint32_t nl = 0;
        if (__ballot(!finished()) != 0) {
            for (uint32_t k0 = 0; k0 < cnt_b; k0 += 64) {
                const uint32_t k = k0 + lane;
                const bool hit = k < cnt_b && ((sqm[k] >> wave) & 1u);
                const uint64_t m = __ballot(hit);
                if (hit) wlist[wave][nl + mbcnt(m)] = (uint16_t)(k * sizeof(StagedRecF));
                nl += (uint32_t)__popcll(m);
            }
        }
        wave_lds_sync();  // wlist[wave] is only touched by this wave
        uint32_t i = 0;
        // two records per step, both records' LDS reads issued before either body
        const uint32_t* wl2 = reinterpret_cast<const uint32_t*>(wlist[wave]);
        uint32_t w2 = nl >= 2 ? wl2[0] : 0u;
        for (; i + 1 < nl; i += 2) {
            if (__ballot(!finished()) == 0) break;
            const StagedRecF& p0 = staged_at(srec, w2 & 0xFFFFu);
            const StagedRecF& p1 = staged_at(srec, w2 >> 16);
            const float4 a0 = p0.a, b0 = p0.b, c0 = p0.c;
            const float4 a1 = p1.a, b1 = p1.b, c1 = p1.c;
            if (i + 3 < nl) w2 = wl2[(i >> 1) + 1];
            body_v(a0, b0, c0);
            body_v(a1, b1, c1);
        }
        if (i < nl && __ballot(!finished()) != 0) body(wlist[wave][i++]);
    }
    if (inside) store_features<VOUT>(f, (size_t)py * (size_t)width + (size_t)px, nch, F0, F1, F2, F3);
}

// composite_strip_depth_kernel<MODE, 0> with four feature accumulators per
// pixel (two pixels per lane).  The fourth staged value lives in sf3[slot]
// beside the 48-B slots.
template <int MODE, bool VIN, bool VOUT>
__global__ __launch_bounds__(256, kFeatWaves) __attribute__((amdgpu_num_sgpr(kFeatSgprs))) void composite_strip_feat_kernel(
    CompositeArgs a, FeatureArgs f, uint32_t nwg) {
    static_assert(MODE == 0 || MODE == 1, "strip composite: tile / live50 rules");
    __shared__ float4 srec[3 * kTileThreads];        // 256 slots of 48 B (raw record, then staged)
    __shared__ float sf3[kTileThreads];              // per slot: the record's fourth value
    __shared__ uint16_t wlist[4][kTileThreads + 4];  // per wave: slot byte offset | selector << 14
    __shared__ uint8_t sqm[kTileThreads];            // per staged record: the 8 quadrants it may reach
    __shared__ uint32_t sopen[4];
    static_assert(sizeof(float4) * 3 * kTileThreads + 4 * kTileThreads + 2 * 4 * (kTileThreads + 4) + kTileThreads + 16 <=
                      16 * 1024,
                  "strip feature composite: LDS per workgroup");

    const uint32_t orig = blockIdx.x;
    const uint32_t full = nwg & ~15u;
    const uint32_t kk = orig >> 3;
    const uint32_t wg = orig < full ? 16u * (kk >> 1) + 2u * (orig & 7u) + (kk & 1u) : orig;
    const uint32_t per_row = 2u * (uint32_t)a.tiles_x;
    int bx, by;
    const uint32_t half = wg & 1u;  // the bin's top (0) or bottom (1) row of tiles
    if (a.order) {
        const uint32_t ob = a.order[wg >> 1];
        by = (int)(ob / (uint32_t)a.tiles_x);
        bx = (int)(ob - (uint32_t)by * (uint32_t)a.tiles_x);
    } else {
        by = (int)(wg / per_row);
        bx = (int)((wg - (uint32_t)by * per_row) >> 1);
    }
    const int width = a.width, height = a.height;
    const uint32_t bin = (uint32_t)(by * a.tiles_x + bx);
    const uint32_t tx0 = (uint32_t)(bx * kBin), ty0 = (uint32_t)(by * kBin) + 16u * half;  // left tile's origin
    const int tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lane = tid & 63;
    const uint32_t wt = wave >> 1, ws = wave & 1u;  // the wave's tile (left / right) and strip (top / bottom)
    const uint32_t lxi = lane & 7u, lyi = 8u * ws + (lane >> 3);
    const float lxA = (float)lxi + 0.5f, lxB = (float)lxi + 8.5f, ly = (float)lyi + 0.5f;  // tile-local (exact)
    const int pxA = (int)(tx0 + 16u * wt + lxi), pxB = pxA + 8, py = (int)(ty0 + lyi);
    const bool inA = pxA < width && py < height, inB = pxB < width && py < height;
    const float ftx0 = (float)tx0, ftx1 = (float)(tx0 + 16u), fty0 = (float)ty0;
    // channels of this launch that exist (1..4; 4 with VIN / VOUT)
    const uint32_t nch = (uint32_t)(f.channels - f.first) < 4u ? (uint32_t)(f.channels - f.first) : 4u;

    uint2 rg = decode_range(a.ranges[bin]);
    if (tx0 >= (uint32_t)width || ty0 >= (uint32_t)height) rg.y = rg.x;  // both tiles outside the frame
    float TA = inA ? 1.0f : 0.0f, TB = inB ? 1.0f : 0.0f;
    float A0 = 0.0f, A1 = 0.0f, A2 = 0.0f, A3 = 0.0f, B0 = 0.0f, B1 = 0.0f, B2 = 0.0f, B3 = 0.0f;
    auto fin = [](float T) -> bool {
        if constexpr (MODE == 0) return T <= kTSat;
        else return T < kTMin;
    };
    // bb = (opacity, f0, f1, f2), f3 the slot's fourth value
    auto pixel = [&](float lx, float tu, float tv, const float4& aa, const float4& bb, float f3, float& T, float& F0,
                     float& F1, float& F2, float& F3) {
        const float u = __builtin_fmaf(aa.x, lx, tu);
        const float v = __builtin_fmaf(aa.z, lx, tv);
        const float qq = __builtin_fmaf(v, v, u * u);
        const bool covered = fmaxf(fabsf(u), fabsf(v)) <= kBoxS && qq <= kQMaxS;
        if (!fin(T) && covered) {
            const float alpha = bb.x * gs_gauss2(qq);
            if constexpr (MODE == 0) {
                const float sa = alpha * T;
                F0 = __builtin_fmaf(bb.y, sa, F0);
                F1 = __builtin_fmaf(bb.z, sa, F1);
                F2 = __builtin_fmaf(bb.w, sa, F2);
                F3 = __builtin_fmaf(f3, sa, F3);
                T = T - sa;
            } else {
                F0 = __builtin_fmaf(bb.y, T, F0);
                F1 = __builtin_fmaf(bb.z, T, F1);
                F2 = __builtin_fmaf(bb.w, T, F2);
                F3 = __builtin_fmaf(f3, T, F3);
                T = T * (1.0f - alpha);
            }
        }
    };
    auto body = [&](const float4& aa, const float4& bb, const float2& cc, float f3, uint32_t sel) {
        const float tu = __builtin_fmaf(aa.y, ly, cc.x);  // fma(-A'y, ly, U0)
        const float tv = __builtin_fmaf(aa.w, ly, cc.y);  // fma(-B'y, ly, V0)
        if (sel & 1u) pixel(lxA, tu, tv, aa, bb, f3, TA, A0, A1, A2, A3);
        if (sel & 2u) pixel(lxB, tu, tv, aa, bb, f3, TB, B0, B1, B2, B3);
    };

    const uint32_t last = rg.y > rg.x ? rg.y - 1u : rg.x;
    float4 rc[3] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f),
                    make_float4(0.f, 0.f, 0.f, 0.f)};
    float4 fc = make_float4(0.f, 0.f, 0.f, 0.f);  // the four values of this lane's own record of the batch in flight
    uint32_t id_next = 0;
    auto gather = [&](uint32_t own_id) {
        uint32_t ln;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0" : "=v"(ln));
        ln = __builtin_amdgcn_mbcnt_hi(~0u, ln);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t c = ln + 64u * (uint32_t)i;
            const uint32_t ck = (c * 43691u) >> 17;  // c / 3 for c < 2^15
            const uint32_t idk = (uint32_t)__shfl((int)own_id, (int)ck, 64);
            rc[i] = a.rec[idk * (uint32_t)a.rec_stride + (c - 3u * ck)];
        }
        fc = load_features<VIN>(f, own_id, nch);
    };
    if (rg.y > rg.x) {
        const uint32_t j = rg.x + tid;
        gather(a.vals[j < last ? j : last]);
        id_next = a.vals[j + kTileThreads < last ? j + kTileThreads : last];
    }
    const uint32_t* const wl2 = reinterpret_cast<const uint32_t*>(wlist[wave]);
    for (uint32_t b = rg.x; b < rg.y; b += kTileThreads) {
        {  // progress-ordered issue priority, as composite_strip_kernel
            const uint32_t nb = (b - rg.x) / kTileThreads;
            if (nb == 0) __builtin_amdgcn_s_setprio(3);
            else if (nb == 2) __builtin_amdgcn_s_setprio(2);
            else if (nb == 4) __builtin_amdgcn_s_setprio(1);
            else if (nb == 6) __builtin_amdgcn_s_setprio(0);
        }
        if (b != rg.x) {  // early out (one LDS barrier)
            const bool open = __ballot(!fin(TA) || !fin(TB)) != 0;
            if (lane == 0) sopen[wave] = open ? 1u : 0u;
            block_lds_sync();
            const uint4 o = *reinterpret_cast<const uint4*>(sopen);
            if ((o.x | o.y | o.z | o.w) == 0u) break;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) srec[192u * wave + lane + 64u * (uint32_t)i] = rc[i];
        sf3[tid] = fc.w;  // (the slot's fourth value; the barrier above freed the last batch's)
        wave_lds_sync();  // the wave's 64 slots are only touched by this wave until the barrier
        if (b + tid < rg.y) {
            float4* st = &srec[3u * tid];
            const float4 r0 = st[0], r1 = st[1], r2 = st[2];
            const float ax = r0.z * kConicScale, ay = r0.w * kConicScale;
            const float bxs = r1.x * kConicScale, bys = r1.y * kConicScale;
            const float exl = ftx0 - r0.x, exr = ftx1 - r0.x, ey = r0.y - fty0;
            const float aye = ay * ey, bye = bys * ey;
            st[0] = make_float4(ax, -ay, bxs, -bys);
            st[1] = make_float4(r1.z, fc.x, fc.y, fc.z);
            st[2] = make_float4(__builtin_fmaf(ax, exl, aye), __builtin_fmaf(bxs, exl, bye), __builtin_fmaf(ax, exr, aye),
                                __builtin_fmaf(bxs, exr, bye));
            const uint32_t wlo = __float_as_uint(r2.z), whi = __float_as_uint(r2.w);
            const uint32_t lo = rect_coords(wlo, a.cell_mask), hi = rect_coords(whi, a.cell_mask);
            const int rx0 = (int)(lo & 0xFFFFu) - (int)tx0, rx1 = (int)(hi & 0xFFFFu) - (int)tx0;
            const int ry0 = (int)(lo >> 16) - (int)ty0, ry1 = (int)(hi >> 16) - (int)ty0;
            const int cl = max(rx0, 0) >> 3, ch = min(rx1, 31) >> 3;
            const int rl = max(ry0, 0) >> 3, rh = min(ry1, 15) >> 3;
            uint32_t cols = rx1 >= 0 && cl <= ch ? (2u << ch) - (1u << cl) : 0u;
            const uint32_t rows = ry1 >= 0 && rl <= rh ? (2u << rh) - (1u << rl) : 0u;
            uint32_t ex0 = 0u, ex1 = 0u;  // excluded columns in rows 0 / 1
            if (a.cell_mask) {
                const uint32_t cm = rect_cell_mask(wlo, whi);
                const int dx = (int)(tx0 >> 3) - (int)((lo & 0xFFFFu) >> 3);
                const int dy = (int)(ty0 >> 3) - (int)(lo >> 19);
                auto row_excl = [&](int dcy) -> uint32_t {
                    if (dcy < 0 || dcy > 3) return 0u;
                    const uint32_t rb = (cm >> (4 * dcy)) & 0xFu;  // rect cells 0..3 of that row
                    if (dx >= 4 || dx <= -4) return 0u;
                    return (dx >= 0 ? rb >> dx : rb << (-dx)) & 0xFu;
                };
                ex0 = row_excl(dy);
                ex1 = row_excl(dy + 1);
            }
            auto spread = [](uint32_t c4) { return (c4 & 3u) | ((c4 & 0xCu) << 2); };  // columns -> bits 0,1,4,5
            const uint32_t qm = ((rows & 1u) ? spread(cols & ~ex0) : 0u) | ((rows & 2u) ? spread(cols & ~ex1) << 2 : 0u);
            sqm[tid] = (uint8_t)qm;
        }
        __syncthreads();
        {
            const uint32_t j = b + 2u * kTileThreads + tid;
            gather(id_next);
            id_next = a.vals[j < last ? j : last];
        }
        const uint32_t cnt_b = rg.y - b < (uint32_t)kTileThreads ? rg.y - b : (uint32_t)kTileThreads;
        const uint32_t open2 = (__ballot(!fin(TA)) != 0 ? 1u : 0u) | (__ballot(!fin(TB)) != 0 ? 2u : 0u);
        uint32_t nl = 0;
        if (open2) {
            for (uint32_t k0 = 0; k0 < cnt_b; k0 += 64) {
                const uint32_t k = k0 + lane;
                const uint32_t sel = k < cnt_b ? (sqm[k] >> (2u * wave)) & open2 : 0u;
                const uint64_t m = __ballot(sel != 0u);
                if (sel) wlist[wave][nl + mbcnt(m)] = (uint16_t)(k * 48u | sel << 14);
                nl += (uint32_t)__popcll(m);
            }
            // three empty entries (selector 0, slot 0) after the list: the half
            // pair of an odd list and the walk's unconditional read-ahead
            if (lane < 3u) wlist[wave][nl + lane] = 0;
        }
        wave_lds_sync();  // wlist[wave] is only touched by this wave
        auto walk = [&](auto tile) {
            constexpr uint32_t kC = 32u + 8u * decltype(tile)::value;
            const char* base = reinterpret_cast<const char*>(srec);
            const char* fbase = reinterpret_cast<const char*>(sf3);
            if (nl == 0u) return;
            auto ld4 = [&](uint32_t o) { return *reinterpret_cast<const float4*>(base + o); };
            auto ld2 = [&](uint32_t o) { return *reinterpret_cast<const float2*>(base + o); };
            // slot byte offset 48 k -> the fourth value's byte offset 4 k
            auto ldf = [&](uint32_t o) { return *reinterpret_cast<const float*>(fbase + o / 12u); };
            uint32_t w2 = wl2[0];
            uint32_t o = w2 & 0x3FFFu;
            float4 aA = ld4(o), bA = ld4(o + 16u);
            float2 cA = ld2(o + kC);
            float zA = ldf(o);
            for (uint32_t i = 0; i < nl; i += 2) {
                if (__ballot(!fin(TA) || !fin(TB)) == 0) break;
                const uint32_t e = __builtin_amdgcn_readfirstlane(w2);
                o = (w2 >> 16) & 0x3FFFu;
                const float4 aB = ld4(o), bB = ld4(o + 16u);
                const float2 cB = ld2(o + kC);
                const float zB = ldf(o);
                w2 = wl2[(i >> 1) + 1];  // (past the list: empty entries)
                body(aA, bA, cA, zA, (e >> 14) & 3u);
                o = w2 & 0x3FFFu;
                aA = ld4(o);
                bA = ld4(o + 16u);
                cA = ld2(o + kC);
                zA = ldf(o);
                body(aB, bB, cB, zB, e >> 30);
            }
        };
        if (wt) walk(std::integral_constant<uint32_t, 1>{});
        else walk(std::integral_constant<uint32_t, 0>{});
    }
    uint32_t ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0" : "=v"(ln));
    ln = __builtin_amdgcn_mbcnt_hi(~0u, ln);
    const int qx = (int)(tx0 + 16u * wt + (ln & 7u)), qy = (int)(ty0 + 8u * ws + (ln >> 3));
    if (qy < height) {
        const size_t pix = (size_t)qy * (size_t)width + (size_t)qx;
        if (qx < width) store_features<VOUT>(f, pix, nch, A0, A1, A2, A3);
        if (qx + 8 < width) store_features<VOUT>(f, pix + 8, nch, B0, B1, B2, B3);
    }
}

namespace {

template <int MODE, bool VIN, bool VOUT>
hipError_t launch_feat_pass(const CompositeArgs& a, const FeatureArgs& f, bool strip, uint32_t nwg, hipStream_t st) {
    if (strip)
        hipLaunchKernelGGL((composite_strip_feat_kernel<MODE, VIN, VOUT>), dim3(nwg), dim3(kTileThreads), 0, st, a, f, nwg);
    else
        hipLaunchKernelGGL((composite_feat_kernel<MODE, VIN, VOUT>), dim3(nwg), dim3(kTileThreads), 0, st, a, f, nwg);
    return hipGetLastError();
}

template <int MODE>
hipError_t launch_feat_mode(const CompositeArgs& a, const FeatureArgs& f, bool vin, bool vout, bool strip, uint32_t nwg,
                            hipStream_t st) {
    if (vin) return vout ? launch_feat_pass<MODE, true, true>(a, f, strip, nwg, st)
                         : launch_feat_pass<MODE, true, false>(a, f, strip, nwg, st);
    return vout ? launch_feat_pass<MODE, false, true>(a, f, strip, nwg, st)
                : launch_feat_pass<MODE, false, false>(a, f, strip, nwg, st);
}

}  // namespace

hipError_t launch_composite_features(const CompositeArgs& a, const float* feat, float* out, int channels, int mode,
                                     hipStream_t st) {
    // tile / live50 rules over whole lists of whole frames: no cap, no slabs, no MLAB, no cut passes, no bands
    if (!out || channels < 1 || channels > kMaxFeatureChannels || a.cap > 0 || a.slab || a.pass ||
        (mode != 0 && mode != 1))
        return hipErrorInvalidValue;
    if (a.rows || a.compact || a.nrows != a.tiles_y || a.tiles_x <= 0 || a.tiles_y <= 0) return hipErrorInvalidValue;
    if (!a.vals || !a.ranges || !a.rec) return hipErrorInvalidValue;
    // (the strip kernel for launches of many bins, as the colour composite)
    const bool strip = composite_strip((uint32_t)(a.tiles_x * a.tiles_y));
    const uint32_t nwg = (uint32_t)((strip ? 2 : 4) * a.tiles_x * a.tiles_y);
    // 16-B rows and pixels: whole groups of four channels, on 16-B aligned bases
    const bool vin = channels % 4 == 0 && reinterpret_cast<uintptr_t>(feat) % 16 == 0;
    const bool vout = channels % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    FeatureArgs f;
    f.feat = feat;
    f.out = out;
    f.channels = channels;
    for (int first = 0; first < channels; first += 4) {
        f.first = first;
        const hipError_t e = mode == 0 ? launch_feat_mode<0>(a, f, vin, vout, strip, nwg, st)
                                       : launch_feat_mode<1>(a, f, vin, vout, strip, nwg, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace gs
