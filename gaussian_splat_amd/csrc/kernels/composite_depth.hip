// composite_depth.hip — the composite with one more accumulator per pixel: the
// accumulated view depth D (gs_render_depth).
//
// D is composited exactly as a colour channel whose per-splat value is the
// fp32 zF of the projection (zf_plane_kernel: -xform_row(V, 2, x, y, z), the
// preprocess's own value): the same fragments, order, weights and break rule
// as C0..C2,
//   tile rule:   D = fma(zF, sa, D), sa = alpha * T
//   live50 rule: D = fma(zF, T, D)
// from D = 0, one pass over the lists, no atomics.  The colour frame is
// gs_render's bit for bit.
//
// composite_depth_kernel and composite_strip_depth_kernel are
// composite_kernel and composite_strip_kernel (composite.hip; tile and live50
// rules, no cap, no slabs, no BGRA8; depth-cut passes 0/1/2) op for op, plus:
//  - the staged record's zF, gathered from the zf plane by splat id by the
//    record's owner lane together with the batch's rc[] chunks (so it is in
//    flight while the batch before it is composited, never loaded after the
//    barrier), and staged in the slot's free word (tile kernel: c.w) or in a
//    1-KB side array (strip kernel: its 48-B slot is full);
//  - depth-cut passes: a quadrant left open saves D beside (C, T) in a second
//    state plane (CompositeArgs::state_d) and pass 2 resumes it; cut positions,
//    open flags and wcost are written exactly as in the colour kernels
//    (termination depends on T alone);
//  - D written to depth_out wherever the colour pixel is written.
// They are kernels of their own, not template parameters of the colour
// kernels, whose code and register budgets (tests/test_kernel_resources.py)
// stay what they were; colour-only frames never launch anything from here.
// Built for 6 waves per SIMD (the 80-VGPR class): the extra accumulators and
// the staged depths do not fit the colour kernels' 64 without spilling.
#include <hip/hip_ext.h>

#include <type_traits>

#include "gs_kernels.h"
#include "gs_wave.h"

namespace gs {

__global__ __launch_bounds__(256) void zf_plane_kernel(const float4* __restrict__ p0, uint32_t n, const FrameUniforms U,
                                                       float* __restrict__ zf) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 a0 = p0[i];
    zf[i] = -xform_row(U.V, 2, a0.x, a0.y, a0.z);  // K3 (tile.metal:94-105), as preprocess_kernel
}

hipError_t launch_zf_plane(const SceneDev& s, const FrameUniforms& U, float* zf, hipStream_t st) {
    if (s.n == 0) return hipSuccess;
    if (!zf || !s.p0) return hipErrorInvalidValue;
    zf_plane_kernel<<<(s.n + 255) / 256, 256, 0, st>>>(s.p0, s.n, U, zf);
    return hipGetLastError();
}

namespace {

// One 48-B LDS slot per staged record (first the raw gathered record):
//   a = (U0, V0, Ax', -Ay')   b = (Bx', -By', opacity, r)   c = (g, b, -, zF)
struct StagedRecD {
    float4 a, b, c;
};
static_assert(sizeof(StagedRecD) == 48, "staged record slot");
__device__ __forceinline__ const StagedRecD& staged_at(const StagedRecD* base, uint32_t off) {
    return *reinterpret_cast<const StagedRecD*>(reinterpret_cast<const char*>(base) + off);
}

constexpr int kDepthSgprs = 62;  // the 80-SGPR allocation class (composite.hip, GS_COMPOSITE_SGPRS)
// waves per SIMD the depth composites are built for (7, the strip kernel in 72 VGPRs, measured
// the same frame time: profiles/depth/ab_depth_waves.txt; 8 spills)
constexpr int kDepthWaves = 6;

}  // namespace

// composite_kernel<MODE, false, 0, PASS> with the depth accumulator.
template <int MODE, int PASS>
__global__ __launch_bounds__(256, kDepthWaves) __attribute__((amdgpu_num_sgpr(kDepthSgprs))) void composite_depth_kernel(
    CompositeArgs a, uint32_t nwg) {
    static_assert(MODE == 0 || MODE == 1, "depth composite: tile / live50 rules");
    __shared__ StagedRecD srec[kTileThreads];
    __shared__ uint16_t wlist[4][kTileThreads];  // per wave: slot byte offsets
    __shared__ uint8_t sqm[kTileThreads];        // per staged record: the quadrants it may reach
    __shared__ uint32_t sopen[4];                // per wave: pixels still open after its last walk

    // XCD-aware bijective remap, bins and tiles as composite_kernel
    const uint32_t orig = blockIdx.x;
    const uint32_t full = nwg & ~31u;
    const uint32_t kk = orig >> 3;
    const uint32_t wg = orig < full ? 32u * (kk >> 2) + 4u * (orig & 7u) + (kk & 3u) : orig;
    const uint32_t per_row = 4u * (uint32_t)a.tiles_x;
    const int owned_row = (int)(wg / per_row);
    const uint32_t k4 = wg - (uint32_t)owned_row * per_row;
    const int bx = (int)(k4 >> 2);
    const int by = a.rows ? (int)a.rows[owned_row] : owned_row;
    const int tx = 2 * bx + (int)(k4 & 1u), ty = 2 * by + (int)((k4 >> 1) & 1u);
    const int width = a.width, height = a.height;
    const uint32_t bin = (uint32_t)(by * a.tiles_x + bx);
    uint32_t* const qr = a.qrec ? a.qrec + (size_t)bin * kQrecWords : nullptr;
    const uint32_t tq = (k4 & 3u) * 4u;
    uint4 oq = make_uint4(0u, 0u, 0u, 0u);  // (PASS 2) the tile's open quadrants
    if constexpr (PASS == 2) {
        oq = *reinterpret_cast<const uint4*>(qr + 16u + tq);
        if ((oq.x | oq.y | oq.z | oq.w) == 0u) return;  // (whole workgroup) the front list finished the tile
    }
    const int tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lane = tid & 63;
    const bool trunc = PASS == 1 && a.cut_in && a.cut_in[bin] < kDepthInf;
    const uint32_t tx0 = (uint32_t)(tx * kTile), ty0 = (uint32_t)(ty * kTile);
    const uint32_t lxi = (wave & 1u) * 8u + (lane & 7u), lyi = (wave >> 1) * 8u + (lane >> 3);
    const int px = (int)(tx0 + lxi);
    const int py = (int)(ty0 + lyi);
    const bool inside = px < width && py < height;
    const float lx = (float)lxi + 0.5f;  // tile-local pixel centre (exact)
    const float ly = (float)lyi + 0.5f;
    const float ftx0 = (float)tx0, fty0 = (float)ty0;

    uint2 rg = decode_range(a.ranges[bin]);
    if (tx0 >= (uint32_t)width || ty0 >= (uint32_t)height) rg.y = rg.x;
    // pixels outside the frame start finished (T = 0), see composite_kernel
    float T = inside ? 1.0f : 0.0f;
    float C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, D = 0.0f;
    const int orow = a.compact ? owned_row * kBin + (py - by * kBin) : py;
    const size_t pix = (size_t)py * width + px;
    const bool resumed = PASS == 2 && (wave == 0 ? oq.x : wave == 1 ? oq.y : wave == 2 ? oq.z : oq.w) != 0u;
    if constexpr (PASS == 2) {
        T = 0.0f;
        if (inside && resumed) {  // the state the front list left: the same registers, resumed
            const float4 st = a.state[pix];
            C0 = st.x;
            C1 = st.y;
            C2 = st.z;
            T = st.w;
            D = a.state_d[pix];
        }
    }
    auto finished = [&]() -> bool {
        if constexpr (MODE == 0) return T <= kTSat;
        else return T < kTMin;
    };
    // one record at this lane's pixel (composite_kernel's body_v), zz its zF
    auto body_v = [&](const float4 aa, const float4 bb, const float2 cc, const float zz) {
        const float u = __builtin_fmaf(aa.z, lx, __builtin_fmaf(aa.w, ly, aa.x));
        const float v = __builtin_fmaf(bb.x, lx, __builtin_fmaf(bb.y, ly, aa.y));
        const float qq = __builtin_fmaf(v, v, u * u);
        const bool covered = fmaxf(fabsf(u), fabsf(v)) <= kBoxS && qq <= kQMaxS;
        if (!finished() && covered) {
            const float alpha = bb.z * gs_gauss2(qq);
            if constexpr (MODE == 0) {
                const float sa = alpha * T;
                C0 = __builtin_fmaf(bb.w, sa, C0);
                C1 = __builtin_fmaf(cc.x, sa, C1);
                C2 = __builtin_fmaf(cc.y, sa, C2);
                D = __builtin_fmaf(zz, sa, D);
                T = T - sa;
            } else {
                C0 = __builtin_fmaf(bb.w, T, C0);
                C1 = __builtin_fmaf(cc.x, T, C1);
                C2 = __builtin_fmaf(cc.y, T, C2);
                D = __builtin_fmaf(zz, T, D);
                T = T * (1.0f - alpha);
            }
        }
    };
    auto body = [&](uint32_t off) {
        const StagedRecD& r = staged_at(srec, off);
        const float4 c = r.c;
        body_v(r.a, r.b, make_float2(c.x, c.y), c.w);
    };

    // Software pipeline and coalesced gathers as composite_kernel; the owner
    // lane of each record also loads its zF (zc) with the chunks.
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
    float zc = 0.0f;
    uint32_t id_cur = 0, id_next = 0;
    auto gather = [&](uint32_t own_id) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t idk = (uint32_t)__shfl((int)own_id, (int)ck[i], 64);
            rc[i] = a.rec[(size_t)a.rec_stride * idk + cp[i]];
        }
        zc = a.zf[own_id];
    };
    if (rg.y > rg.x) {
        const uint32_t j = rg.x + tid;
        id_cur = a.vals[j < last ? j : last];
        gather(id_cur);
        id_next = a.vals[j + kTileThreads < last ? j + kTileThreads : last];
    }
    const uint32_t len = rg.y > rg.x ? rg.y - rg.x : 0u;  // (empty bins: {~0, 0})
    uint32_t fetched = len < (uint32_t)kTileThreads ? len : (uint32_t)kTileThreads;
    uint32_t wend = 0u;  // (PASS 1) end of the last batch this wave walked with an open pixel
    for (uint32_t b = rg.x; b < rg.y; b += kTileThreads) {
        if (b != rg.x) {
            const bool open = __ballot(!finished()) != 0;
            if (lane == 0) sopen[wave] = open ? 1u : 0u;
            block_lds_sync();
            const uint4 o = *reinterpret_cast<const uint4*>(sopen);
            if ((o.x | o.y | o.z | o.w) == 0u) break;
        }
        if (rg.y - b > (uint32_t)kTileThreads) {
            const uint32_t left = rg.y - b - (uint32_t)kTileThreads;
            fetched += left < (uint32_t)kTileThreads ? left : (uint32_t)kTileThreads;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) reinterpret_cast<float4*>(srec)[192u * wave + lane + 64u * (uint32_t)i] = rc[i];
        wave_lds_sync();  // the wave's 64 slots are only touched by this wave until the barrier
        if (b + tid < rg.y) {
            StagedRecD& st = srec[tid];
            const float4 r0 = st.a, r1 = st.b, r2 = st.c;
            const float ax = r0.z * kConicScale, ay = r0.w * kConicScale;
            const float bxs = r1.x * kConicScale, bys = r1.y * kConicScale;
            const float ex = ftx0 - r0.x, ey = r0.y - fty0;
            st.a = make_float4(__builtin_fmaf(ax, ex, ay * ey), __builtin_fmaf(bxs, ex, bys * ey), ax, -ay);
            st.b = make_float4(bxs, -bys, r1.z, r1.w);
            st.c = make_float4(r2.x, r2.y, 0.0f, zc);
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
            wend = b + cnt_b;
            for (uint32_t k0 = 0; k0 < cnt_b; k0 += 64) {
                const uint32_t k = k0 + lane;
                const bool hit = k < cnt_b && ((sqm[k] >> wave) & 1u);
                const uint64_t m = __ballot(hit);
                if (hit) wlist[wave][nl + mbcnt(m)] = (uint16_t)(k * sizeof(StagedRecD));
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
            const StagedRecD& p0 = staged_at(srec, w2 & 0xFFFFu);
            const StagedRecD& p1 = staged_at(srec, w2 >> 16);
            const float4 a0 = p0.a, b0 = p0.b, c0 = p0.c;
            const float4 a1 = p1.a, b1 = p1.b, c1 = p1.c;
            if (i + 3 < nl) w2 = wl2[(i >> 1) + 1];
            body_v(a0, b0, make_float2(c0.x, c0.y), c0.w);
            body_v(a1, b1, make_float2(c1.x, c1.y), c1.w);
        }
        if (i < nl && __ballot(!finished()) != 0) body(wlist[wave][i++]);
    }
    if (tid == 0 && a.fetched) (void)atomicAdd(a.fetched, (unsigned long long)fetched);
    bool open_w = false, keep = false;
    if constexpr (PASS == 1) {
        open_w = __ballot(!finished()) != 0;
        keep = open_w && trunc;
    }
    const bool write = inside && (PASS != 2 || resumed);  // (PASS 2: the rest was written by pass 1)
    if (write) {
        if (keep) {
            a.state[pix] = make_float4(C0, C1, C2, T);  // (C, T) and D
            a.state_d[pix] = D;
        } else {
            a.out[(size_t)orow * width + px] = make_float4(C0, C1, C2, 1.0f - T);
            a.depth_out[(size_t)orow * width + px] = D;
        }
    }
    if constexpr (PASS == 1) {
        if (lane == 0) {
            qr[tq + wave] = open_w ? 0xFFFFFFFFu : wend;
            qr[16u + tq + wave] = keep ? 1u : 0u;
            if (keep) (void)atomicAdd(a.open_q_count, 1ull);
        }
    }
}

// composite_strip_kernel<MODE, PASS> with the depth accumulators (two pixels
// per lane).  The staged depths live in szf[slot] beside the 48-B slots.
template <int MODE, int PASS>
__global__ __launch_bounds__(256, kDepthWaves) __attribute__((amdgpu_num_sgpr(kDepthSgprs))) void composite_strip_depth_kernel(
    CompositeArgs a, uint32_t nwg) {
    static_assert(MODE == 0 || MODE == 1, "strip composite: tile / live50 rules");
    __shared__ float4 srec[3 * kTileThreads];        // 256 slots of 48 B (raw record, then staged)
    __shared__ float szf[kTileThreads];              // per slot: the record's zF
    __shared__ uint16_t wlist[4][kTileThreads + 4];  // per wave: slot byte offset | selector << 14
    __shared__ uint8_t sqm[kTileThreads];            // per staged record: the 8 quadrants it may reach
    __shared__ uint32_t sopen[4];
    static_assert(sizeof(float4) * 3 * kTileThreads + 4 * kTileThreads + 2 * 4 * (kTileThreads + 4) + kTileThreads + 16 <=
                      16 * 1024,
                  "strip depth composite: LDS per workgroup");

    const uint32_t orig = blockIdx.x;
    const uint32_t full = nwg & ~15u;
    const uint32_t kk = orig >> 3;
    const uint32_t wg = orig < full ? 16u * (kk >> 1) + 2u * (orig & 7u) + (kk & 1u) : orig;
    const uint32_t per_row = 2u * (uint32_t)a.tiles_x;
    int owned_row, bx, by;
    const uint32_t half = wg & 1u;  // the bin's top (0) or bottom (1) row of tiles
    if (a.order && !a.rows) {  // (single-GPU frames: every row owned)
        const uint32_t ob = a.order[wg >> 1];
        owned_row = by = (int)(ob / (uint32_t)a.tiles_x);
        bx = (int)(ob - (uint32_t)by * (uint32_t)a.tiles_x);
    } else {
        owned_row = (int)(wg / per_row);
        bx = (int)((wg - (uint32_t)owned_row * per_row) >> 1);
        by = a.rows ? (int)a.rows[owned_row] : owned_row;
    }
    const int width = a.width, height = a.height;
    const uint32_t bin = (uint32_t)(by * a.tiles_x + bx);
    const uint32_t tx0 = (uint32_t)(bx * kBin), ty0 = (uint32_t)(by * kBin) + 16u * half;  // left tile's origin
    const int tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lane = tid & 63;
    const uint32_t wt = wave >> 1, ws = wave & 1u;  // the wave's tile (left / right) and strip (top / bottom)
    uint32_t* const qr = a.qrec ? a.qrec + (size_t)bin * kQrecWords : nullptr;
    const uint32_t qA = 4u * (2u * half + wt) + 2u * ws;
    bool resA = false, resB = false;  // (PASS 2) the quadrants left open by the front list
    if constexpr (PASS == 2) {
        const uint4 f0 = *reinterpret_cast<const uint4*>(qr + 16u + 8u * half);
        const uint4 f1 = *reinterpret_cast<const uint4*>(qr + 20u + 8u * half);
        if ((f0.x | f0.y | f0.z | f0.w | f1.x | f1.y | f1.z | f1.w) == 0u) return;  // (whole workgroup)
        resA = qr[16u + qA] != 0u;
        resB = qr[17u + qA] != 0u;
    }
    const bool trunc = PASS == 1 && a.cut_in && a.cut_in[bin] < kDepthInf;
    const uint32_t lxi = lane & 7u, lyi = 8u * ws + (lane >> 3);
    const float lxA = (float)lxi + 0.5f, lxB = (float)lxi + 8.5f, ly = (float)lyi + 0.5f;  // tile-local (exact)
    const int pxA = (int)(tx0 + 16u * wt + lxi), pxB = pxA + 8, py = (int)(ty0 + lyi);
    const bool inA = pxA < width && py < height, inB = pxB < width && py < height;
    const float ftx0 = (float)tx0, ftx1 = (float)(tx0 + 16u), fty0 = (float)ty0;

    uint2 rg = decode_range(a.ranges[bin]);
    if (tx0 >= (uint32_t)width || ty0 >= (uint32_t)height) rg.y = rg.x;  // both tiles outside the frame
    float TA = inA ? 1.0f : 0.0f, TB = inB ? 1.0f : 0.0f;
    float A0 = 0.0f, A1 = 0.0f, A2 = 0.0f, B0 = 0.0f, B1 = 0.0f, B2 = 0.0f, DA = 0.0f, DB = 0.0f;
    const size_t pixA = (size_t)py * width + pxA, pixB = pixA + 8;
    if constexpr (PASS == 2) {
        TA = 0.0f;
        TB = 0.0f;
        if (inA && resA) {
            const float4 st = a.state[pixA];
            A0 = st.x, A1 = st.y, A2 = st.z, TA = st.w;
            DA = a.state_d[pixA];
        }
        if (inB && resB) {
            const float4 st = a.state[pixB];
            B0 = st.x, B1 = st.y, B2 = st.z, TB = st.w;
            DB = a.state_d[pixB];
        }
    }
    auto fin = [](float T) -> bool {
        if constexpr (MODE == 0) return T <= kTSat;
        else return T < kTMin;
    };
    auto pixel = [&](float lx, float tu, float tv, const float4& aa, const float4& bb, float zz, float& T, float& C0,
                     float& C1, float& C2, float& D) {
        const float u = __builtin_fmaf(aa.x, lx, tu);
        const float v = __builtin_fmaf(aa.z, lx, tv);
        const float qq = __builtin_fmaf(v, v, u * u);
        const bool covered = fmaxf(fabsf(u), fabsf(v)) <= kBoxS && qq <= kQMaxS;
        if (!fin(T) && covered) {
            const float alpha = bb.x * gs_gauss2(qq);
            if constexpr (MODE == 0) {
                const float sa = alpha * T;
                C0 = __builtin_fmaf(bb.y, sa, C0);
                C1 = __builtin_fmaf(bb.z, sa, C1);
                C2 = __builtin_fmaf(bb.w, sa, C2);
                D = __builtin_fmaf(zz, sa, D);
                T = T - sa;
            } else {
                C0 = __builtin_fmaf(bb.y, T, C0);
                C1 = __builtin_fmaf(bb.z, T, C1);
                C2 = __builtin_fmaf(bb.w, T, C2);
                D = __builtin_fmaf(zz, T, D);
                T = T * (1.0f - alpha);
            }
        }
    };
    auto body = [&](const float4& aa, const float4& bb, const float2& cc, float zz, uint32_t sel) {
        const float tu = __builtin_fmaf(aa.y, ly, cc.x);  // fma(-A'y, ly, U0)
        const float tv = __builtin_fmaf(aa.w, ly, cc.y);  // fma(-B'y, ly, V0)
        if (sel & 1u) pixel(lxA, tu, tv, aa, bb, zz, TA, A0, A1, A2, DA);
        if (sel & 2u) pixel(lxB, tu, tv, aa, bb, zz, TB, B0, B1, B2, DB);
    };

    const uint32_t last = rg.y > rg.x ? rg.y - 1u : rg.x;
    float4 rc[3] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f),
                    make_float4(0.f, 0.f, 0.f, 0.f)};
    float zc = 0.0f;  // the zF of this lane's own record of the batch in flight
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
        zc = a.zf[own_id];
    };
    if (rg.y > rg.x) {
        const uint32_t j = rg.x + tid;
        gather(a.vals[j < last ? j : last]);
        id_next = a.vals[j + kTileThreads < last ? j + kTileThreads : last];
    }
    const uint32_t len = rg.y > rg.x ? rg.y - rg.x : 0u;
    uint32_t fetched = len < (uint32_t)kTileThreads ? len : (uint32_t)kTileThreads;
    uint32_t wendA = 0u, wendB = 0u;  // (PASS 1) end of the last batch each quadrant walked with an open pixel
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
        if (rg.y - b > (uint32_t)kTileThreads) {
            const uint32_t left = rg.y - b - (uint32_t)kTileThreads;
            fetched += left < (uint32_t)kTileThreads ? left : (uint32_t)kTileThreads;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) srec[192u * wave + lane + 64u * (uint32_t)i] = rc[i];
        szf[tid] = zc;  // (the slot's depth; the barrier above freed the last batch's)
        wave_lds_sync();  // the wave's 64 slots are only touched by this wave until the barrier
        if (b + tid < rg.y) {
            float4* st = &srec[3u * tid];
            const float4 r0 = st[0], r1 = st[1], r2 = st[2];
            const float ax = r0.z * kConicScale, ay = r0.w * kConicScale;
            const float bxs = r1.x * kConicScale, bys = r1.y * kConicScale;
            const float exl = ftx0 - r0.x, exr = ftx1 - r0.x, ey = r0.y - fty0;
            const float aye = ay * ey, bye = bys * ey;
            st[0] = make_float4(ax, -ay, bxs, -bys);
            st[1] = make_float4(r1.z, r1.w, r2.x, r2.y);
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
        if constexpr (PASS == 1) {
            if (open2 & 1u) wendA = b + cnt_b;
            if (open2 & 2u) wendB = b + cnt_b;
        }
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
            const char* zbase = reinterpret_cast<const char*>(szf);
            if (nl == 0u) return;
            auto ld4 = [&](uint32_t o) { return *reinterpret_cast<const float4*>(base + o); };
            auto ld2 = [&](uint32_t o) { return *reinterpret_cast<const float2*>(base + o); };
            // slot byte offset 48 k -> the depth's byte offset 4 k
            auto ldz = [&](uint32_t o) { return *reinterpret_cast<const float*>(zbase + o / 12u); };
            uint32_t w2 = wl2[0];
            uint32_t o = w2 & 0x3FFFu;
            float4 aA = ld4(o), bA = ld4(o + 16u);
            float2 cA = ld2(o + kC);
            float zA = ldz(o);
            for (uint32_t i = 0; i < nl; i += 2) {
                if (__ballot(!fin(TA) || !fin(TB)) == 0) break;
                const uint32_t e = __builtin_amdgcn_readfirstlane(w2);
                o = (w2 >> 16) & 0x3FFFu;
                const float4 aB = ld4(o), bB = ld4(o + 16u);
                const float2 cB = ld2(o + kC);
                const float zB = ldz(o);
                w2 = wl2[(i >> 1) + 1];  // (past the list: empty entries)
                body(aA, bA, cA, zA, (e >> 14) & 3u);
                o = w2 & 0x3FFFu;
                aA = ld4(o);
                bA = ld4(o + 16u);
                cA = ld2(o + kC);
                zA = ldz(o);
                body(aB, bB, cB, zB, e >> 30);
            }
        };
        if (wt) walk(std::integral_constant<uint32_t, 1>{});
        else walk(std::integral_constant<uint32_t, 0>{});
    }
    if (tid == 0 && a.fetched) (void)atomicAdd(a.fetched, (unsigned long long)fetched);
    if (PASS == 1 && tid == 0 && a.wcost) a.wcost[2u * bin + half] = fetched;  // (the next bin order's cost)
    bool openA = false, openB = false, keepA = false, keepB = false;
    if constexpr (PASS == 1) {
        openA = __ballot(!fin(TA)) != 0;
        openB = __ballot(!fin(TB)) != 0;
        keepA = openA && trunc;
        keepB = openB && trunc;
    }
    uint32_t ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0" : "=v"(ln));
    ln = __builtin_amdgcn_mbcnt_hi(~0u, ln);
    const int qx = (int)(tx0 + 16u * wt + (ln & 7u)), qy = (int)(ty0 + 8u * ws + (ln >> 3));
    const int orow = a.compact ? owned_row * kBin + (qy - by * kBin) : qy;
    auto store = [&](bool res, bool keep, int px, float C0, float C1, float C2, float T, float D) {
        if (px >= width || qy >= height || (PASS == 2 && !res)) return;  // (PASS 2: the rest was written by pass 1)
        const size_t pix = (size_t)qy * width + px;
        if (keep) {
            a.state[pix] = make_float4(C0, C1, C2, T);
            a.state_d[pix] = D;
        } else {
            a.out[(size_t)orow * width + px] = make_float4(C0, C1, C2, 1.0f - T);
            a.depth_out[(size_t)orow * width + px] = D;
        }
    };
    store(resA, keepA, qx, A0, A1, A2, TA, DA);
    store(resB, keepB, qx + 8, B0, B1, B2, TB, DB);
    if constexpr (PASS == 1) {
        if (lane == 0) {
            qr[qA] = openA ? 0xFFFFFFFFu : wendA;
            qr[qA + 1u] = openB ? 0xFFFFFFFFu : wendB;
            qr[16u + qA] = keepA ? 1u : 0u;
            qr[17u + qA] = keepB ? 1u : 0u;
            const uint32_t nk = (keepA ? 1u : 0u) + (keepB ? 1u : 0u);
            if (nk) (void)atomicAdd(a.open_q_count, (unsigned long long)nk);
        }
    }
}

template <int MODE, int PASS>
static hipError_t launch_depth_mode(const CompositeArgs& a, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    if (a.nrows < 0 || a.nrows > a.tiles_y || (!a.rows && a.nrows != a.tiles_y)) return hipErrorInvalidValue;
    // (the strip kernel for launches of many bins, as the colour composite)
    const bool strip = composite_strip((uint32_t)(a.tiles_x * a.nrows));
    const uint32_t nwg = (uint32_t)((strip ? 2 : 4) * a.tiles_x * a.nrows);
    if (nwg == 0) {  // no owned tiles: the timing events still mark the (empty) stage
        if (t0 && hipEventRecord(t0, st) != hipSuccess) return hipGetLastError();
        if (t1 && hipEventRecord(t1, st) != hipSuccess) return hipGetLastError();
        return hipSuccess;
    }
    if (strip)
        hipExtLaunchKernelGGL(composite_strip_depth_kernel<MODE, PASS>, dim3(nwg), dim3(kTileThreads), 0, st, t0, t1, 0, a,
                              nwg);
    else
        hipExtLaunchKernelGGL(composite_depth_kernel<MODE, PASS>, dim3(nwg), dim3(kTileThreads), 0, st, t0, t1, 0, a, nwg);
    return hipGetLastError();
}

hipError_t launch_composite_depth(const CompositeArgs& a, int mode, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    // tile / live50 rules on fp32 frames: no cap, no slabs, no MLAB, no BGRA8
    if (!a.depth_out || !a.zf || !a.out || a.out_bgra8 || a.cap > 0 || a.slab || (mode != 0 && mode != 1))
        return hipErrorInvalidValue;
    if (a.order && (a.rows || a.compact || a.nrows != a.tiles_y)) return hipErrorInvalidValue;  // (whole frames only)
    if (a.pass) {
        if (!a.qrec || !a.state || !a.state_d || a.pass > 2 || (a.pass == 1 && !a.open_q_count))
            return hipErrorInvalidValue;
        if (a.pass == 1)
            return mode == 0 ? launch_depth_mode<0, 1>(a, st, t0, t1) : launch_depth_mode<1, 1>(a, st, t0, t1);
        return mode == 0 ? launch_depth_mode<0, 2>(a, st, t0, t1) : launch_depth_mode<1, 2>(a, st, t0, t1);
    }
    return mode == 0 ? launch_depth_mode<0, 0>(a, st, t0, t1) : launch_depth_mode<1, 0>(a, st, t0, t1);
}

}  // namespace gs
