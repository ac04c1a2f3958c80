// composite_kernels.h — the composite kernels' bodies, written once, and the
// "values" policies that tell colour, depth, feature and contrib frames apart.
//
// composite_tile_body (one 16x16 tile per workgroup) and composite_strip_body (two tiles
// per workgroup, two pixels per lane) are the bodies of every composite kernel:
// the XCD remap, the gather, the software pipeline, the staging maths, the
// quadrant masks, the list compaction, the walk and the quadrant records exist
// here and nowhere else.  The kernels themselves are thin __global__ entry
// points that fix the launch bounds and the policy: composite_kernel and
// composite_strip_kernel (composite.hip, colour), composite_depth_kernel and
// composite_strip_depth_kernel (composite_depth.hip, gs_render_depth, DESIGN.md
// §2.11), composite_feat_kernel and composite_strip_feat_kernel
// (composite_features.hip, gs_render_features, §2.12), composite_contrib_kernel
// and composite_strip_contrib_kernel (composite_contrib.hip, gs_render_contrib,
// §2.13), composite_ids_kernel and composite_strip_ids_kernel (composite_ids.hip,
// gs_render_ids, §2.14).
//
// Everything that differs between them is stated in a policy V, what a
// frame kind composites per pixel beside T:
//   Own, gather   what the record's owner lane loads beside its rc[] chunks,
//                 with them (in flight while the batch before is composited)
//   values        the up to four values staged per record: each is composited
//                 as a colour channel (tile rule X = fma(x, alpha T, X), live50
//                 rule X = fma(x, T, X)); termination depends on T alone
//   kFourth       a fourth accumulator, its staged word (tile slot: c.w, which
//                 MLAB's half depth uses otherwise; strip kernel: a 1-KB side
//                 array) and, in depth-cut passes, its state plane exist
//   kWaves        waves per SIMD the kernels are built for
//   kWholeFrame   every launch is a whole-frame pass-0 launch: the instances
//                 carry no owned-row, band-buffer, fetch-counter, wcost or
//                 quadrant-record code
//   store         (kFourth) a finished pixel (px, row) of the output: o = (the
//                 three first accumulators, alpha), d the fourth accumulator;
//                 without a fourth value the bodies' own colour epilogues run
//   kContrib      the transposed pass (ContribValues, gs_render_contrib, §2.13;
//                 composite_contrib_kernel and composite_strip_contrib_kernel,
//                 composite_contrib.hip): no pixel is stored; scale, weight and
//                 scatter turn each fragment's blend weight into its splat's
//                 totals
//   kTopK, Top    (IdValues<K>, gs_render_ids, §2.14; composite_ids_kernel and
//                 composite_strip_ids_kernel, composite_ids.hip) a contrib-shaped
//                 pass that keeps, per pixel, the K fragments of largest quantised
//                 weight in registers (Top; insert in scatter's place) and stores
//                 them at the end of the pixel; 0 and an empty Top elsewhere
#pragma once

#include <hip/hip_ext.h>

#include <type_traits>

#include "gs_kernels.h"
#include "gs_wave.h"

namespace gs {

// Colour frames: the record's own r, g, b; fp32 or BGRA8 pixels.  (Cap, slab
// and MLAB frames are colour frames: their epilogues are the kernel's modes.)
struct ColourValues {
    struct Own {};
    static constexpr bool kFourth = false, kWholeFrame = false, kContrib = false;
    static constexpr int kWaves = 8;
    static constexpr int kTopK = 0;
    struct Top {};
    __device__ __forceinline__ Own gather(const CompositeArgs&, uint32_t) const { return {}; }
    __device__ __forceinline__ float4 values(const Own&, float r, float g, float b) const {
        return make_float4(r, g, b, 0.0f);
    }
};

// Depth frames: colour plus D, the fp32 zF of the projection (a.zf, written by
// launch_zf_plane) accumulated as a fourth channel from D = 0; the colour frame
// is gs_render's bit for bit.  Tile / live50 rules on fp32 frames; a quadrant
// left open by a depth-cut pass keeps D in a.state_d.  Built for 6 waves per
// SIMD (the 80-VGPR class; 7, the strip kernel in 72 VGPRs, measured the same
// frame time: profiles/depth/ab_depth_waves.txt; 8 spills).
struct DepthValues {
    using Own = float;
    static constexpr bool kFourth = true, kWholeFrame = false, kContrib = false;
    static constexpr int kWaves = 6;
    static constexpr int kTopK = 0;
    struct Top {};
    __device__ __forceinline__ Own gather(const CompositeArgs& a, uint32_t id) const { return a.zf[id]; }
    __device__ __forceinline__ float4 values(const Own& zf, float r, float g, float b) const {
        return make_float4(r, g, b, zf);
    }
    __device__ __forceinline__ void store(const CompositeArgs& a, int row, int px, const float4& o, float d) const {
        const size_t at = (size_t)row * a.width + px;
        a.out[at] = o;
        a.depth_out[at] = d;
    }
};

// Feature frames: one launch composites the channels f.first .. f.first + 3 of
// the caller's N x K matrix (row i for splat i) into the H x W x K image
// (channels innermost), from 0, not clamped, not normalised; the record's own
// r, g, b are ignored and no colour is written.  The depth kernels' class.
//  - VIN: one 16-B load per record (K % 4 == 0 and a 16-B aligned matrix),
//    else dword loads of the launch's valid channels only: a tail channel
//    past K is never loaded (for the last splat it lies past the matrix);
//  - VOUT: one 16-B store per pixel (K % 4 == 0 and a 16-B aligned image),
//    else dword stores of the valid channels only;
//  - id * K + k and pixel * K + k are 64-bit (50M splats x 64 channels).
template <bool VIN, bool VOUT>
struct FeatureValues {
    using Own = float4;
    static constexpr bool kFourth = true, kWholeFrame = true, kContrib = false;
    static constexpr int kWaves = 6;
    static constexpr int kTopK = 0;
    struct Top {};
    FeatureArgs f;
    // channels of this launch that exist (1..4; 4 with VIN / VOUT)
    __device__ __forceinline__ uint32_t nch() const {
        return (uint32_t)(f.channels - f.first) < 4u ? (uint32_t)(f.channels - f.first) : 4u;
    }
    __device__ __forceinline__ Own gather(const CompositeArgs&, uint32_t id) const {
        const float* row = f.feat + ((size_t)id * (size_t)(uint32_t)f.channels + (size_t)(uint32_t)f.first);
        if constexpr (VIN) {
            return *reinterpret_cast<const float4*>(row);
        } else {
            const uint32_t n = nch();  // (wave-uniform)
            float4 v = make_float4(row[0], 0.0f, 0.0f, 0.0f);
            if (n > 1u) v.y = row[1];
            if (n > 2u) v.z = row[2];
            if (n > 3u) v.w = row[3];
            return v;
        }
    }
    __device__ __forceinline__ float4 values(const Own& v, float, float, float) const { return v; }
    __device__ __forceinline__ void store(const CompositeArgs& a, int row, int px, const float4& o, float d) const {
        const size_t at = (size_t)row * (size_t)a.width + (size_t)px;
        float* p = f.out + (at * (size_t)(uint32_t)f.channels + (size_t)(uint32_t)f.first);
        if constexpr (VOUT) {
            *reinterpret_cast<float4*>(p) = make_float4(o.x, o.y, o.z, d);
        } else {
            const uint32_t n = nch();
            p[0] = o.x;
            if (n > 1u) p[1] = o.y;
            if (n > 2u) p[2] = o.z;
            if (n > 3u) p[3] = d;
        }
    }
};

// Contrib frames (gs_render_contrib): the transposed pass.
// T per pixel and nothing else: no colour is accumulated and no pixel is
// written (kContrib drops the stores, so the bodies' accumulators are dead).
// Per record and pixel the blend weight w the colour frame multiplies the
// splat's colour with (tile rule: alpha T; live50 rule: T) is quantised,
//   q(w) = (uint32_t)(min(max(w, 0), 1) * 2^24)   (truncation; NaN -> 0),
// so every total is an integer whatever the order of summation.  The scale is
// the pixel's own (scale()): 2^24, or 0 for a pixel the caller's mask leaves
// out, which then composites as always and contributes nothing.
//  - the record's splat id travels where a colour frame stages r: the owner
//    lane holds it (gather), values() puts its bits into the first value;
//  - weight() is the hook inside the exec-masked update; scatter() runs after
//    it with every lane of the wave active, q = 0 in the lanes that skipped
//    the update: count = popcount(ballot(q > 0)), sum and max by a 6-step DPP
//    reduction (a wave's sum is at most 128 * 2^24 = 2^31), then one lane issues
//    the three atomics of the (record, wave); nothing when no lane has q > 0.
struct ContribValues {
    using Own = uint32_t;
    static constexpr bool kFourth = false, kWholeFrame = true, kContrib = true;
    static constexpr int kWaves = 8;
    static constexpr int kTopK = 0;
    struct Top {};
    ContribArgs k;
    __device__ __forceinline__ Own gather(const CompositeArgs&, uint32_t id) const { return id; }
    __device__ __forceinline__ float4 values(const Own& id, float, float, float) const {
        return make_float4(__uint_as_float(id), 0.0f, 0.0f, 0.0f);
    }
    __device__ __forceinline__ float scale(bool inside, size_t pix) const {
        return inside && (!k.mask || k.mask[pix] != 0) ? 16777216.0f : 0.0f;
    }
    __device__ __forceinline__ uint32_t weight(float w, float scale) const {
        return (uint32_t)(fminf(fmaxf(w, 0.0f), 1.0f) * scale);
    }
    // qs: the lane's quantised weights summed (one pixel, or the strip kernel's
    // two), qm: their max, cnt: the wave's pixels with q > 0 (scalar)
    __device__ __forceinline__ void scatter(float id_bits, uint32_t qs, uint32_t qm, uint32_t cnt) const {
        if (cnt == 0u) return;  // (wave-uniform)
        // (the scans' last lane holds the totals and issues the atomics.  The id passes
        // through an identity DPP move, quad_perm [0, 1, 2, 3], which the compiler takes
        // for a per-lane value: with an address it knows to be wave-uniform its atomic
        // optimiser wraps each of the three atomics in a lane election, a reduction over
        // the active lanes and a branch of its own, all for the one lane that is active)
        const uint32_t s = wave_scan_dpp<false>(qs), m = wave_scan_dpp<true>(qm);
        const uint32_t id = (uint32_t)__builtin_amdgcn_mov_dpp((int)__float_as_uint(id_bits), 0xE4, 0xf, 0xf, true);
        if (lane_id() == 63u) {
            (void)atomicAdd(k.sum + id, (unsigned long long)s);
            (void)atomicAdd(k.count + id, cnt);
            (void)atomicMax(k.max + id, m);
        }
    }
};

// Ids frames (gs_render_ids): each pixel's K fragments of
// largest quantised weight.  ContribValues' sibling: T per pixel, no colour,
// the record's id staged where a colour frame stages r, the same q(w) at the
// same hooks, no mask.  Instead of scattering, a lane keeps per pixel
//   key[k] = q << 32 | ~id,  k < K, descending (0: an empty slot),
// and the number of fragments with q > 0.  One unsigned 64-bit order is the
// call's: q descending, then id ascending; a splat is in a bin's list once, so
// no two candidates of a pixel compare equal.  A candidate that does not beat
// key[K - 1] is dropped after that one comparison; one that does replaces it
// and is moved up by K - 1 compare-exchanges, in the lanes that have one (exec
// mask); the chain is skipped when no lane of the wave has one (a ballot).
// store() writes the pixel's slots with vector stores: ~key (GS_ID_NONE for an
// empty slot), key >> 32 and the count; 16-B stores of ids / q where the call
// has 4 slots and the array is 16-B aligned (IdArgs::vec), else a dword each.
template <int K>
struct IdValues {
    static_assert(K == 1 || K == 2 || K == 4, "ids composites: 1, 2 or 4 slots in registers");
    using Own = uint32_t;
    static constexpr bool kFourth = false, kWholeFrame = true, kContrib = true;
    static constexpr int kTopK = K;
    struct Top {
        unsigned long long key[K];
        uint32_t n;
    };
    IdArgs i;
    __device__ __forceinline__ Own gather(const CompositeArgs&, uint32_t id) const { return id; }
    __device__ __forceinline__ float4 values(const Own& id, float, float, float) const {
        return make_float4(__uint_as_float(id), 0.0f, 0.0f, 0.0f);
    }
    __device__ __forceinline__ float scale(bool inside, size_t) const { return inside ? 16777216.0f : 0.0f; }
    __device__ __forceinline__ uint32_t weight(float w, float scale) const {
        return (uint32_t)(fminf(fmaxf(w, 0.0f), 1.0f) * scale);
    }
    static __device__ __forceinline__ unsigned long long cand(float id_bits, uint32_t q) {
        return (unsigned long long)q << 32 | (unsigned long long)(~__float_as_uint(id_bits));
    }
    static __device__ __forceinline__ void push(Top& t, unsigned long long c, bool beats) {
        if (beats) {
            t.key[K - 1] = c;
#pragma unroll
            for (int k = K - 1; k > 0; --k) {
                const unsigned long long lo = t.key[k], hi = t.key[k - 1];
                t.key[k - 1] = lo > hi ? lo : hi;
                t.key[k] = lo > hi ? hi : lo;
            }
        }
    }
    // one record at one pixel (every lane; q = 0 where the update was skipped)
    __device__ __forceinline__ void insert(Top& t, float id_bits, uint32_t q) const {
        const unsigned long long c = cand(id_bits, q);
        const bool beats = q != 0u && c > t.key[K - 1];
        t.n += q != 0u ? 1u : 0u;
        if (__ballot(beats) != 0) push(t, c, beats);  // (wave-uniform)
    }
    // one record at the strip body's two pixels: one ballot for both chains
    __device__ __forceinline__ void insert2(Top& ta, Top& tb, float id_bits, uint32_t qa, uint32_t qb) const {
        const unsigned long long ca = cand(id_bits, qa), cb = cand(id_bits, qb);
        const bool ba = qa != 0u && ca > ta.key[K - 1], bb = qb != 0u && cb > tb.key[K - 1];
        ta.n += qa != 0u ? 1u : 0u;
        tb.n += qb != 0u ? 1u : 0u;
        if (__ballot(ba || bb) != 0) {  // (wave-uniform)
            push(ta, ca, ba);
            push(tb, cb, bb);
        }
    }
    // a finished pixel inside the frame (an empty Top: GS_ID_NONE, 0, 0)
    __device__ __forceinline__ void store(const Top& t, size_t pix) const {
        const uint32_t s = (uint32_t)i.slots;  // (<= K; 3 on the K = 4 instance)
        uint32_t* const pi = i.ids + pix * (size_t)s;
        if (K == 4 && (i.vec & 1)) {
            *reinterpret_cast<uint4*>(pi) = make_uint4(~(uint32_t)t.key[0], ~(uint32_t)t.key[1 % K],
                                                       ~(uint32_t)t.key[2 % K], ~(uint32_t)t.key[3 % K]);
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if ((uint32_t)k < s) pi[k] = ~(uint32_t)t.key[k];
        }
        if (i.q) {  // (wave-uniform)
            uint32_t* const pq = i.q + pix * (size_t)s;
            if (K == 4 && (i.vec & 2)) {
                *reinterpret_cast<uint4*>(pq) =
                    make_uint4((uint32_t)(t.key[0] >> 32), (uint32_t)(t.key[1 % K] >> 32),
                               (uint32_t)(t.key[2 % K] >> 32), (uint32_t)(t.key[3 % K] >> 32));
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if ((uint32_t)k < s) pq[k] = (uint32_t)(t.key[k] >> 32);
            }
        }
        if (i.count) i.count[pix] = t.n;
    }
};

#ifdef GS_COMPOSITE_TRACE
// Debug build only (tools/composite_trace.py): per strip workgroup, its start
// and end (s_memrealtime, 100 MHz), its bin pair slot and the fetched record
// count, written with vector stores by lane 0; read by
// gs_debug_composite_trace (composite.hip), which no product path calls.
static __device__ unsigned long long g_comp_trace[4 * 65536];
#endif

// MLAB k-buffer (gaussian_splat.metal:201-361): six premultiplied half
// layers + half depths per pixel in registers, updated per covering fragment
// in arrival order with the reference's insertion and under-merge, resolved
// front to back.  Every op is a correctly rounded half op (oracle: mlab_*).
namespace mlab {
using h16 = _Float16;
__device__ __forceinline__ h16 mul(h16 a, h16 b) { return (h16)((float)a * (float)b); }  // exact in f32, one rounding
__device__ __forceinline__ h16 add(h16 a, h16 b) { return (h16)((float)a + (float)b); }  // no double-rounding tie
__device__ __forceinline__ h16 sub(h16 a, h16 b) { return (h16)((float)a - (float)b); }
constexpr int kLayers = 6;  // NUM_OIT_LAYERS (gaussian_splat.metal:11)
struct KBuf {
    h16 L[kLayers][4];
    h16 D[kLayers];
    __device__ __forceinline__ void clear() {  // all attachments (0,0,0,1) (instanced_splat_renderer.mm:540)
#pragma unroll
        for (int i = 0; i < kLayers; ++i) {
            L[i][0] = L[i][1] = L[i][2] = (h16)0.0f;
            L[i][3] = (h16)1.0f;
            D[i] = (h16)0.0f;
        }
        D[3] = (h16)1.0f;  // depths01.a
    }
    __device__ __forceinline__ void insert(float r, float g, float b, float alpha, h16 nd) {  // :206-294
        // alpha is rounded to f32 first (float alpha = g * opacity, :200), then
        // to half: keep the compiler from fusing the product and the
        // conversion into one v_fma_mix rounding
        asm volatile("" : "+v"(alpha));
        const h16 ha = (h16)alpha;
        h16 nl[4] = {mul((h16)r, ha), mul((h16)g, ha), mul((h16)b, ha), sub((h16)1.0f, ha)};
#pragma unroll
        for (int i = 0; i < kLayers; ++i) {
            const bool ins = nd >= D[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const h16 t = L[i][c];
                L[i][c] = ins ? nl[c] : t;
                nl[c] = ins ? t : nl[c];
            }
            const h16 t = D[i];
            D[i] = ins ? nd : t;
            nd = ins ? t : nd;
        }
        const int l = kLayers - 1;
        const bool closer = nd >= D[l];
        h16 m[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const h16 fr = closer ? nl[c] : L[l][c], bk = closer ? L[l][c] : nl[c];
            const h16 ba = closer ? L[l][3] : nl[3];
            m[c] = add(bk, mul(fr, ba));
        }
        m[3] = mul(nl[3], L[l][3]);  // front.a * back.a (commutative)
#pragma unroll
        for (int c = 0; c < 4; ++c) L[l][c] = m[c];
        D[l] = closer ? nd : D[l];
    }
    __device__ __forceinline__ float4 resolve() const {  // :330-361
        h16 C0 = (h16)0.0f, C1 = C0, C2 = C0, at = (h16)1.0f;
#pragma unroll
        for (int i = 0; i < kLayers; ++i) {
            C0 = add(C0, mul(L[i][0], at));
            C1 = add(C1, mul(L[i][1], at));
            C2 = add(C2, mul(L[i][2], at));
            at = mul(at, L[i][3]);
        }
        return make_float4((float)C0, (float)C1, (float)C2, (float)sub((h16)1.0f, at));
    }
};
}  // namespace mlab

// MODE 0: tile rule, 1: live50 rule, 2: cap threshold pass (index-ordered
// lists; per pixel the id of the a.cap-th covering fragment), 3: MLAB
// k-buffer (index-ordered lists, no early out).  CAP: composite
// only fragments with id <= thr[pixel] (the first a.cap in arrival order).
// SLAB (depth-slab multi-GPU): 1 = transmittance pass, 2 =
// colour pass from the earlier slabs' transmittance product.
//
// Staged record (per tile): the conic scaled by kConicScale
// and its offset at the tile origin, so a lane's coverage is four fmas on
// its tile-local pixel centre (lx, ly) = (px - tx0 + 1/2, py - ty0 + 1/2):
//   u' = fma(Ax', lx, fma(-Ay', ly, U0)),  U0 = fma(Ax', tx0 - cx, Ay' (cy - ty0))
// and likewise v' from (Bx', By', V0).
// One 48-B LDS slot per staged record (first the raw gathered record):
//   a = (U0, V0, Ax', -Ay')   b = (Bx', -By', opacity, r)   c = (g, b, id, half(zF))
// (id: the splat id, cap modes; half(zF) bits: MLAB, or the values policy's
// fourth value, with its first three in r, g, b), and the wave lists hold
// slot byte offsets (u16), so a record's reads take one address VGPR.
struct StagedRec {
    float4 a, b, c;
};
static_assert(sizeof(StagedRec) == 48, "staged record slot");
__device__ __forceinline__ const StagedRec& staged_at(const StagedRec* base, uint32_t off) {
    return *reinterpret_cast<const StagedRec*>(reinterpret_cast<const char*>(base) + off);
}

// PASS (depth-cut frames, gs_options.depth_split; modes 0/1,
// no cap, no slabs): 1 = the front lists (CompositeArgs: a tile left open
// with a cut list keeps its per-pixel state, every tile raises its bin's next
// cut); 2 = the fallback lists, resuming the open tiles only.
//
// SGPR budget: at most 62 (TotalSGPRs <= 64, tests/test_kernel_resources.py).
// gfx950 allocates a wave's SGPRs in blocks of 16 (plus 16), from 800 per
// SIMD, and the composite shares its SIMDs with the preprocess kernel
// (96-SGPR class) in the pipelined frame.  Left alone the pass-1 kernel takes
// 68-76 SGPRs (the 96 class, against 80 for pass 0): standalone no slower,
// but in the co-run with the preprocess its span grew 0.445 -> 0.527 ms and
// the frame 0.687 -> 0.738 ms (profiles/r04/ab_composite_sgpr.txt).  The cap
// costs pass 1 one spilled dword (stored at entry, reloaded at the end).
#define GS_COMPOSITE_SGPRS 62
#define GS_COMPOSITE_KERNEL(waves) \
    __global__ __launch_bounds__(256, waves) __attribute__((amdgpu_num_sgpr(GS_COMPOSITE_SGPRS))) void
// V: the values policy: colour, colour and depth, or four feature channels.
// What it adds to the colour kernel sits behind V::kFourth, what it drops
// behind V::kWholeFrame; the colour kernels' instruction streams are those of
// the kernel before it had V.
template <int MODE, bool CAP, int SLAB, int PASS, class V>
__device__ __forceinline__ void composite_tile_body(const CompositeArgs a, uint32_t nwg, const V v) {
    constexpr bool kIds = CAP || MODE == 2;  // the body needs the splat id
    static_assert(PASS == 0 || ((MODE == 0 || MODE == 1) && !CAP && SLAB == 0), "depth-cut passes: tile/live50 rules");
    static_assert(!V::kFourth || ((MODE == 0 || MODE == 1) && !CAP && SLAB == 0), "fourth value: tile/live50 rules");
    static_assert(!V::kWholeFrame || PASS == 0, "whole-frame policies: no depth-cut passes");
    const uint16_t* const rows = V::kWholeFrame ? nullptr : a.rows;
    __shared__ StagedRec srec[kTileThreads];
    __shared__ uint16_t wlist[4][kTileThreads];  // per wave: slot byte offsets
    __shared__ uint8_t sqm[kTileThreads];  // per staged record: the quadrants it may reach
    __shared__ uint32_t sopen[4];          // per wave: pixels still open after its last walk

    // XCD-aware bijective remap (blocks b and b+8 share an XCD,
    // cdna_hip_programming.md §5, T1): bins dealt round-robin over the XCDs,
    // a bin's 4 tiles on one XCD (they share its list through that L2).
    // Measured against giving each XCD a contiguous band of bin rows: -2 %
    // composite, since the bands' costs differ and the launch ends with the
    // slowest XCD.
    const uint32_t orig = blockIdx.x;
    const uint32_t full = nwg & ~31u;
    const uint32_t kk = orig >> 3;
    const uint32_t wg = orig < full ? 32u * (kk >> 2) + 4u * (orig & 7u) + (kk & 3u) : orig;

    // Grid covers only the owned bin rows.  The four 16x16
    // tiles of a bin are consecutive workgroups (same XCD / L2).
    const uint32_t per_row = 4u * (uint32_t)a.tiles_x;
    const int owned_row = (int)(wg / per_row);
    const uint32_t k4 = wg - (uint32_t)owned_row * per_row;
    const int bx = (int)(k4 >> 2);
    const int by = rows ? (int)rows[owned_row] : owned_row;
    const int tx = 2 * bx + (int)(k4 & 1u), ty = 2 * by + (int)((k4 >> 1) & 1u);
    const int width = a.width, height = a.height;
    const uint32_t bin = (uint32_t)(by * a.tiles_x + bx);
    // (depth cuts: the bin's 128-B quadrant record, CompositeArgs::qrec; this
    // tile's quadrants are [4 (k4 & 3), +4))
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
    // PASS 1: the bin's list was cut (a quadrant left open keeps its state)
    const bool trunc = PASS == 1 && a.cut_in && a.cut_in[bin] < kDepthInf;
    // this wave's quadrant: pixels [tx0 + ox, +7] x [ty0 + oy, +7]
    const uint32_t tx0 = (uint32_t)(tx * kTile), ty0 = (uint32_t)(ty * kTile);
    const uint32_t lxi = (wave & 1u) * 8u + (lane & 7u), lyi = (wave >> 1) * 8u + (lane >> 3);
    const int px = (int)(tx0 + lxi);
    const int py = (int)(ty0 + lyi);
    const bool inside = px < width && py < height;
    const float lx = (float)lxi + 0.5f;  // tile-local pixel centre (exact)
    const float ly = (float)lyi + 0.5f;
    const float ftx0 = (float)tx0, fty0 = (float)ty0;

    // (a tile wholly outside the frame, the last bin row's lower half, has
    // nothing to composite)
    uint2 rg = decode_range(a.ranges[bin]);
    if (tx0 >= (uint32_t)width || ty0 >= (uint32_t)height) rg.y = rg.x;
    // Pixels outside the frame start finished (T = 0): for the tile and live50
    // rules "finished" is then just the break test on T itself, so no
    // separate per-lane flag is carried through the loop.
    float T = inside ? 1.0f : 0.0f;  // transmittance (tile rule: T = 1 - A)
    float C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, D = 0.0f;  // (D: V::kFourth)
    // compact = owned bin rows stacked (multi-GPU band buffer)
    const int orow = !V::kWholeFrame && a.compact ? owned_row * kBin + (py - by * kBin) : py;
    const size_t pix = (size_t)py * width + px;
    float qscale = 0.0f;  // (V::kContrib) the pixel's weight scale, 0 where the mask leaves it out
    if constexpr (V::kContrib) qscale = v.scale(inside, pix);
    typename V::Top top{};  // (V::kTopK) the pixel's K heaviest fragments and its fragment count
    // PASS 2: this quadrant was left open by the front list (else its pixels
    // start finished, and were written already)
    const bool resumed = PASS == 2 && (wave == 0 ? oq.x : wave == 1 ? oq.y : wave == 2 ? oq.z : oq.w) != 0u;
    if constexpr (PASS == 2) {
        T = 0.0f;
        if (inside && resumed) {  // the state the front list left: the same registers, resumed
            const float4 st = a.state[pix];
            C0 = st.x;
            C1 = st.y;
            C2 = st.z;
            T = st.w;
            if constexpr (V::kFourth) D = a.state_d[pix];
        }
    }
    bool done = !inside;  // MODE 2 / 3
    uint32_t thr = 0xFFFFFFFFu;  // CAP: last admitted id; MODE 2: result
    int cnt = 0;                 // MODE 2: covering fragments seen
    if constexpr (CAP) {
        if (inside) thr = a.thr[pix];
    }
    // slab colour pass: the state the earlier (farther) slabs leave, exactly
    // the ordered product of their transmittance, rank order = depth order
    float T0 = 1.0f;
    mlab::KBuf kb;
    if constexpr (MODE == 3) kb.clear();
    if constexpr (SLAB == 2) {
        float ts = 1.0f;
        if (inside)
            for (int j = 0; j < a.slab_rank; ++j) ts *= a.t_all[((size_t)j * height + py) * width + px];
        // saturated before this slab (T <= 0.01 / T < 0.01): the loop broke earlier
        if (inside) T = ts;
        T0 = T;
    }
    auto finished = [&]() -> bool {
        if constexpr (MODE == 0) return T <= kTSat;
        else if constexpr (MODE == 1) return T < kTMin;
        else return done;
    };

    // One record at this lane's pixel: coverage (K6 closed form: the quad box
    // |uv| <= 3 and the 0.01 cutoff, tile.metal:142-156,191-195), then the
    // gaussian alpha (:197) and the composite update (A1).  Skipping a lane is
    // bit-identical to adding its exact zero, so the update sits in the
    // gaussian's exec-masked block.
    auto body_v = [&](const float4 aa, const float4 bb, const float2 cc, uint32_t id, _Float16 hd, float dd) {
        const float u = __builtin_fmaf(aa.z, lx, __builtin_fmaf(aa.w, ly, aa.x));
        const float vv = __builtin_fmaf(bb.x, lx, __builtin_fmaf(bb.y, ly, aa.y));
        const float qq = __builtin_fmaf(vv, vv, u * u);
        const bool covered = fmaxf(fabsf(u), fabsf(vv)) <= kBoxS && qq <= kQMaxS;
        if constexpr (MODE == 2) {
            // arrival order: the a.cap-th covering fragment fixes the threshold
            const bool in = !done && covered;
            cnt += in ? 1 : 0;
            if (in && cnt == a.cap) {
                thr = id;
                done = true;
            }
        } else if constexpr (MODE == 3) {
            if (!done && covered) kb.insert(bb.w, cc.x, cc.y, bb.z * gs_gauss2(qq), hd);
        } else {
            bool in = !finished() && covered;
            if constexpr (CAP) in = in && id <= thr;
            uint32_t q = 0u;  // (V::kContrib) the fragment's quantised weight
            if (in) {
                const float alpha = bb.z * gs_gauss2(qq);
                if constexpr (MODE == 0) {
                    const float sa = alpha * T;
                    if constexpr (V::kContrib) q = v.weight(sa, qscale);
                    C0 = __builtin_fmaf(bb.w, sa, C0);
                    C1 = __builtin_fmaf(cc.x, sa, C1);
                    C2 = __builtin_fmaf(cc.y, sa, C2);
                    if constexpr (V::kFourth) D = __builtin_fmaf(dd, sa, D);
                    T = T - sa;
                } else {
                    if constexpr (V::kContrib) q = v.weight(T, qscale);
                    C0 = __builtin_fmaf(bb.w, T, C0);
                    C1 = __builtin_fmaf(cc.x, T, C1);
                    C2 = __builtin_fmaf(cc.y, T, C2);
                    if constexpr (V::kFourth) D = __builtin_fmaf(dd, T, D);
                    T = T * (1.0f - alpha);
                }
            }
            // (every lane again: the record's id is the first staged value)
            if constexpr (V::kTopK > 0) v.insert(top, bb.w, q);
            else if constexpr (V::kContrib) v.scatter(bb.w, q, q, (uint32_t)__popcll(__ballot(q != 0u)));
        }
    };
    // a record's c words: (g, b), the id where the body needs it, and the
    // fourth value (then one 16-B read)
    struct CWords {
        float2 c;
        uint32_t id;
        float d;
    };
    auto cwords = [](const StagedRec& r) -> CWords {
        if constexpr (V::kFourth) {
            const float4 c = r.c;
            return {make_float2(c.x, c.y), 0u, c.w};
        } else {
            return {make_float2(r.c.x, r.c.y), kIds ? __float_as_uint(r.c.z) : 0u, 0.0f};
        }
    };
    auto body = [&](uint32_t off) {
        const StagedRec& r = staged_at(srec, off);
        const CWords c = cwords(r);
        body_v(r.a, r.b, c.c, c.id, MODE == 3 ? __builtin_bit_cast(_Float16, (uint16_t)__float_as_uint(r.c.w)) : (_Float16)0.0f,
               c.d);
    };

    // Software pipeline: while batch b is composited, batch b+1's records are
    // in flight into registers and batch b+2's ids are being loaded.
    // Coalesced gathers: wave w stages records 64w..64w+63 of a batch, and
    // their 192 16-B chunks are loaded by its 64 lanes three apiece (chunk
    // c = lane + 64i is part c % 3 of record c / 3), so adjacent lanes read
    // adjacent bytes of one record; the owner lane of each record collects
    // its chunks through LDS.  Every lane loads, its list position clamped to
    // the last entry: a conditional load joins the old and the loaded
    // registers, and the copy the compiler then emits waits for the load it
    // was meant to overlap.
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
    typename V::Own own{};  // what the policy gathers for this lane's own record, with the chunks
    uint32_t id_cur = 0, id_next = 0;
    auto gather = [&](uint32_t own_id) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t idk = (uint32_t)__shfl((int)own_id, (int)ck[i], 64);
            rc[i] = a.rec[(size_t)a.rec_stride * idk + cp[i]];
        }
        own = v.gather(a, own_id);
    };
    if (rg.y > rg.x) {
        const uint32_t j = rg.x + tid;
        id_cur = a.vals[j < last ? j : last];
        gather(id_cur);
        id_next = a.vals[j + kTileThreads < last ? j + kTileThreads : last];
    }
    // records this workgroup fetched: the first batch, then one prefetched
    // batch per batch it composites (the early-out stops both)
    const uint32_t len = rg.y > rg.x ? rg.y - rg.x : 0u;  // (empty bins: {~0, 0})
    uint32_t fetched = len < (uint32_t)kTileThreads ? len : (uint32_t)kTileThreads;
    uint32_t wend = 0u;  // (PASS 1) end of the last batch this wave walked with an open pixel
    for (uint32_t b = rg.x; b < rg.y; b += kTileThreads) {
        // every wave publishes whether it still has open pixels; one LDS
        // barrier both orders that and frees the slots of the last batch
        // (__syncthreads_count takes three)
        if (b != rg.x) {
            const bool open = __ballot(!finished()) != 0;
            if (lane == 0) sopen[wave] = open ? 1u : 0u;
            block_lds_sync();
            const uint4 o = *reinterpret_cast<const uint4*>(sopen);
            if ((o.x | o.y | o.z | o.w) == 0u) break;
        }
        if (!V::kWholeFrame && rg.y - b > (uint32_t)kTileThreads) {
            const uint32_t left = rg.y - b - (uint32_t)kTileThreads;
            fetched += left < (uint32_t)kTileThreads ? left : (uint32_t)kTileThreads;
        }
        // the wave's gathered chunks into their records' slots (raw layout):
        // chunk c of the wave is float4 192 w + c of the slot array
#pragma unroll
        for (int i = 0; i < 3; ++i) reinterpret_cast<float4*>(srec)[192u * wave + lane + 64u * (uint32_t)i] = rc[i];
        wave_lds_sync();  // the wave's 64 slots are only touched by this wave until the barrier
        if (b + tid < rg.y) {
            // record (cx, cy, ax, ay) (bx, by, op, r) (g, b, rect_lo, rect_hi)
            // staged for this tile (scaled conic, offsets at the tile origin)
            StagedRec& st = srec[tid];
            const float4 r0 = st.a, r1 = st.b, r2 = st.c;
            const float ax = r0.z * kConicScale, ay = r0.w * kConicScale;
            const float bxs = r1.x * kConicScale, bys = r1.y * kConicScale;
            const float ex = ftx0 - r0.x, ey = r0.y - fty0;
            st.a = make_float4(__builtin_fmaf(ax, ex, ay * ey), __builtin_fmaf(bxs, ex, bys * ey), ax, -ay);
            const float4 val = v.values(own, r1.w, r2.x, r2.y);
            st.b = make_float4(bxs, -bys, r1.z, val.x);
            uint32_t sid = 0, shd = 0;
            if constexpr (kIds) sid = id_cur;
            if constexpr (MODE == 3) shd = kDepthInf - a.dkey[id_cur];  // half(zF) (dkey = 0x7C00 - half bits)
            st.c = make_float4(val.y, val.z, __uint_as_float(sid), V::kFourth ? val.w : __uint_as_float(shd));
            // which of the tile's 8x8 quadrants (wave w: column w & 1, row
            // w >> 1) the record's rect reaches and its cell mask does not
            // rule out: computed once here instead of by every wave
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
        // wave-level compaction of the splats reaching this quadrant (index order kept)
        uint32_t nl = 0;
        if (__ballot(!finished()) != 0) {
            wend = b + cnt_b;
            for (uint32_t k0 = 0; k0 < cnt_b; k0 += 64) {
                const uint32_t k = k0 + lane;
                const bool hit = k < cnt_b && ((sqm[k] >> wave) & 1u);
                const uint64_t m = __ballot(hit);
                if (hit) wlist[wave][nl + mbcnt(m)] = (uint16_t)(k * sizeof(StagedRec));
                nl += (uint32_t)__popcll(m);
            }
        }
        wave_lds_sync();  // wlist[wave] is only touched by this wave
        uint32_t i = 0;
        if constexpr (MODE == 2 || MODE == 3) {
            for (; i < nl; ++i) {
                if (__ballot(!done) == 0) break;
                body(wlist[wave][i]);
            }
        } else {
            // two records per step, both records' LDS reads issued before
            // either body; the next pair's slot offsets are read one step ahead
            const uint32_t* wl2 = reinterpret_cast<const uint32_t*>(wlist[wave]);
            uint32_t w2 = nl >= 2 ? wl2[0] : 0u;
            for (; i + 1 < nl; i += 2) {
                if (__ballot(!finished()) == 0) break;
                const StagedRec& p0 = staged_at(srec, w2 & 0xFFFFu);
                const StagedRec& p1 = staged_at(srec, w2 >> 16);
                const float4 a0 = p0.a, b0 = p0.b;
                const CWords c0 = cwords(p0);
                const float4 a1 = p1.a, b1 = p1.b;
                const CWords c1 = cwords(p1);
                if (i + 3 < nl) w2 = wl2[(i >> 1) + 1];
                body_v(a0, b0, c0.c, c0.id, (_Float16)0.0f, c0.d);
                body_v(a1, b1, c1.c, c1.id, (_Float16)0.0f, c1.d);
            }
            if (i < nl && __ballot(!finished()) != 0) body(wlist[wave][i++]);
        }
    }
    if (!V::kWholeFrame && tid == 0 && a.fetched) (void)atomicAdd(a.fetched, (unsigned long long)fetched);
    // PASS 1, per quadrant (no workgroup barrier, no contended atomic): a
    // pixel still open at the end of a list that was cut keeps its state for
    // the fallback lists instead of its final value
    bool open_w = false, keep = false;
    if constexpr (PASS == 1) {
        open_w = __ballot(!finished()) != 0;
        keep = open_w && trunc;
    }
    // (V::kContrib: the pass writes no pixel)
    const bool write = !V::kContrib && inside && (PASS != 2 || resumed);  // (PASS 2: the rest was written by pass 1)
    if (write) {
        if (keep) {
            a.state[pix] = make_float4(C0, C1, C2, T);  // (C, T) and D
            if constexpr (V::kFourth) a.state_d[pix] = D;
        } else if constexpr (SLAB == 1) {
            a.t_out[pix] = T;
        } else if constexpr (SLAB == 2) {
            // contributions: colour and the alpha this slab adds (sum over slabs)
            a.out[pix] = make_float4(C0, C1, C2, T0 - T);
        } else if constexpr (MODE == 2) {
            a.thr_out[pix] = thr;
        } else {
            const float4 o = MODE == 3 ? kb.resolve() : make_float4(C0, C1, C2, 1.0f - T);
            // (the colour store stays here, not in ColourValues: as a policy
            // member its index arithmetic is placed differently, and the colour
            // instances' instruction streams are pinned)
            if constexpr (V::kFourth)
                v.store(a, orow, px, o, D);
            else if (a.out_bgra8)
                a.out_bgra8[(size_t)orow * width + px] = pack_bgra8(o.x, o.y, o.z, o.w);
            else
                a.out[(size_t)orow * width + px] = o;
        }
    }
    if constexpr (V::kTopK > 0) {  // (an ids pass: every pixel of the frame, those of empty bins too)
        if (inside) v.store(top, pix);
    }
    // the quadrant's record words, after its pixels (a store queued before
    // them would hold the pixel stores' wait, vmcnt counting stores too): its
    // cut position (the end of the last batch it walked with an open pixel,
    // ~0 while one stays open) and its open flag
    if constexpr (PASS == 1) {
        if (lane == 0) {
            qr[tq + wave] = open_w ? 0xFFFFFFFFu : wend;
            qr[16u + tq + wave] = keep ? 1u : 0u;
            if (keep) (void)atomicAdd(a.open_q_count, 1ull);
        }
    }
}

// Strip composite: the tile and live50 rules (MODE 0/1; no cap, no depth
// slabs; depth-cut PASS 0/1/2), the bench frame's kernel.  The same contract
// as composite_kernel, op for op, with more pixels per record read:
//  - one 256-lane workgroup per half bin (two 16x16 tiles side by side, the
//    bin's top or bottom row of tiles), so each bin record is gathered and
//    staged twice per bin instead of four times;
//  - each wave a 16x8 strip of one tile, two pixels per lane (tile-local
//    (lx, ly) and (lx + 8, ly): the two 8x8 quadrants of the strip), so one
//    broadcast read of a staged record (40 B) serves both quadrants and the
//    inner fma(-A'y, ly, U0) of the coverage test is shared by them;
//  - per record and wave a 2-bit quadrant selector (from the record's rect
//    and 8x8 cell mask, as composite_kernel's per-quadrant filter), tested in
//    scalar registers: a pixel whose quadrant the record cannot reach skips
//    its coverage test.
// Staged slot (48 B): a = (Ax', -Ay', Bx', -By'), b = (opacity, r, g, b),
// c = (U0, V0) at the left tile's origin, then at the right tile's.  The slot
// is full: a policy's fourth value (V::kFourth; b then holds its first three)
// lives in a 1-KB side array, sv3[slot].
#ifndef GS_STRIP_PRIO_TOP  // the first batches' issue priority (then one lower every two batches)
#define GS_STRIP_PRIO_TOP 3
#endif
#ifndef GS_STRIP_WAVES  // tunable: waves per SIMD the colour strip composite is built for
#define GS_STRIP_WAVES 8
#endif
template <int MODE, int PASS, class V>
__device__ __forceinline__ void composite_strip_body(const CompositeArgs a, uint32_t nwg, const V v) {
    static_assert(MODE == 0 || MODE == 1, "strip composite: tile / live50 rules");
    static_assert(!V::kWholeFrame || PASS == 0, "whole-frame policies: no depth-cut passes");
    __shared__ float4 srec[3 * kTileThreads];    // 256 slots of 48 B (raw record, then staged)
    __shared__ float sv3[V::kFourth ? kTileThreads : 1];  // per slot: the record's fourth value
    __shared__ uint16_t wlist[4][kTileThreads + 4];  // per wave: slot byte offset | selector << 14
    __shared__ uint8_t sqm[kTileThreads];        // per staged record: the 8 quadrants it may reach
    __shared__ uint32_t sopen[4];
    static_assert(sizeof(srec) + sizeof(sv3) + sizeof(wlist) + sizeof(sqm) + sizeof(sopen) <= 16 * 1024,
                  "strip composite: LDS per workgroup");
    const uint16_t* const rows = V::kWholeFrame ? nullptr : a.rows;

    // XCD-aware remap (as composite_kernel): blocks b and b + 8 share an XCD,
    // so a bin's two halves (consecutive wg) run on one XCD and share its list
    // through that L2; bins dealt round-robin over the XCDs.
    const uint32_t orig = blockIdx.x;
    const uint32_t full = nwg & ~15u;
    const uint32_t kk = orig >> 3;
    const uint32_t wg = orig < full ? 16u * (kk >> 1) + 2u * (orig & 7u) + (kk & 1u) : orig;
    const uint32_t per_row = 2u * (uint32_t)a.tiles_x;
    int owned_row, bx, by;
    const uint32_t half = wg & 1u;  // the bin's top (0) or bottom (1) row of tiles
    if (a.order && !rows) {  // (single-GPU frames: every row owned)
        const uint32_t ob = a.order[wg >> 1];
        owned_row = by = (int)(ob / (uint32_t)a.tiles_x);
        bx = (int)(ob - (uint32_t)by * (uint32_t)a.tiles_x);
    } else {
        owned_row = (int)(wg / per_row);
        bx = (int)((wg - (uint32_t)owned_row * per_row) >> 1);
        by = rows ? (int)rows[owned_row] : owned_row;
    }
    const int width = a.width, height = a.height;
    const uint32_t bin = (uint32_t)(by * a.tiles_x + bx);
    const uint32_t tx0 = (uint32_t)(bx * kBin), ty0 = (uint32_t)(by * kBin) + 16u * half;  // left tile's origin
    const int tid = threadIdx.x;
#ifdef GS_COMPOSITE_TRACE
    const unsigned long long trace_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lane = tid & 63;
    const uint32_t wt = wave >> 1, ws = wave & 1u;  // the wave's tile (left / right) and strip (top / bottom)
    // quadrant records of depth-cut frames: tile k4 = 2 half + wt of the bin,
    // quadrants (x half, y half) = (0, ws) and (1, ws): words 4 k4 + 2 ws + {0, 1}
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
    // this lane's pixels: A = (ttx0 + lxi, py), B = A + (8, 0), ttx0 = tx0 + 16 wt
    const uint32_t lxi = lane & 7u, lyi = 8u * ws + (lane >> 3);
    const float lxA = (float)lxi + 0.5f, lxB = (float)lxi + 8.5f, ly = (float)lyi + 0.5f;  // tile-local (exact)
    const int pxA = (int)(tx0 + 16u * wt + lxi), pxB = pxA + 8, py = (int)(ty0 + lyi);
    const bool inA = pxA < width && py < height, inB = pxB < width && py < height;
    const float ftx0 = (float)tx0, ftx1 = (float)(tx0 + 16u), fty0 = (float)ty0;

    uint2 rg = decode_range(a.ranges[bin]);
    if (tx0 >= (uint32_t)width || ty0 >= (uint32_t)height) rg.y = rg.x;  // both tiles outside the frame
    // pixels outside the frame start finished (T = 0), see composite_kernel
    float TA = inA ? 1.0f : 0.0f, TB = inB ? 1.0f : 0.0f;
    // accumulators per pixel (an array: a fourth accumulator named beside three
    // others is captured by the lambdas below in colour instances too, and
    // reordered their registers)
    constexpr int kAcc = V::kFourth ? 4 : 3;
    float A[kAcc] = {}, B[kAcc] = {};
    const size_t pixA = (size_t)py * width + pxA, pixB = pixA + 8;
    float qsA = 0.0f, qsB = 0.0f;  // (V::kContrib) the pixels' weight scales, 0 where the mask leaves one out
    if constexpr (V::kContrib) {
        qsA = v.scale(inA, pixA);
        qsB = v.scale(inB, pixB);
    }
    typename V::Top topA{}, topB{};  // (V::kTopK) per pixel: its K heaviest fragments and its fragment count
    if constexpr (PASS == 2) {
        TA = 0.0f;
        TB = 0.0f;
        if (inA && resA) {
            const float4 st = a.state[pixA];
            A[0] = st.x, A[1] = st.y, A[2] = st.z, TA = st.w;
            if constexpr (V::kFourth) A[3] = a.state_d[pixA];
        }
        if (inB && resB) {
            const float4 st = a.state[pixB];
            B[0] = st.x, B[1] = st.y, B[2] = st.z, TB = st.w;
            if constexpr (V::kFourth) B[3] = a.state_d[pixB];
        }
    }
    auto fin = [](float T) -> bool {
        if constexpr (MODE == 0) return T <= kTSat;
        else return T < kTMin;
    };
    // One pixel and one record (composite_kernel's body_v): coverage, the
    // gaussian alpha and the update, the update exec-masked (an uncovered or
    // finished pixel adds an exact zero).
    auto pixel = [&](float lx, float tu, float tv, const float4& aa, const float4& bb, float dd, float& T,
                     float (&C)[kAcc]) {
        const float u = __builtin_fmaf(aa.x, lx, tu);
        const float vv = __builtin_fmaf(aa.z, lx, tv);
        const float qq = __builtin_fmaf(vv, vv, u * u);
        const bool covered = fmaxf(fabsf(u), fabsf(vv)) <= kBoxS && qq <= kQMaxS;
        if (!fin(T) && covered) {
            const float alpha = bb.x * gs_gauss2(qq);
            const float val[4] = {bb.y, bb.z, bb.w, dd};
            if constexpr (MODE == 0) {
                const float sa = alpha * T;
#pragma unroll
                for (int k = 0; k < kAcc; ++k) C[k] = __builtin_fmaf(val[k], sa, C[k]);
                T = T - sa;
            } else {
#pragma unroll
                for (int k = 0; k < kAcc; ++k) C[k] = __builtin_fmaf(val[k], T, C[k]);
                T = T * (1.0f - alpha);
            }
        }
    };
    // (V::kContrib) the same pixel and record without accumulators: coverage,
    // alpha and T op for op, and the fragment's quantised weight (qs: the
    // pixel's weight scale) where pixel() has its fmas, 0 where it skips.  A
    // route of its own: as a hook inside pixel(), behind `if constexpr`, the
    // extra parameters moved the colour strip kernels' instruction streams
    // (profiles/contrib/instr_compare.txt).
    auto pixel_w = [&](float lx, float tu, float tv, const float4& aa, const float4& bb, float& T,
                       float qs) -> uint32_t {
        const float u = __builtin_fmaf(aa.x, lx, tu);
        const float vv = __builtin_fmaf(aa.z, lx, tv);
        const float qq = __builtin_fmaf(vv, vv, u * u);
        const bool covered = fmaxf(fabsf(u), fabsf(vv)) <= kBoxS && qq <= kQMaxS;
        uint32_t q = 0u;
        if constexpr (V::kContrib) {
            if (!fin(T) && covered) {
                const float alpha = bb.x * gs_gauss2(qq);
                if constexpr (MODE == 0) {
                    const float sa = alpha * T;
                    q = v.weight(sa, qs);
                    T = T - sa;
                } else {
                    q = v.weight(T, qs);
                    T = T * (1.0f - alpha);
                }
            }
        }
        return q;
    };
    // a record for both of the wave's quadrants; sel (scalar): bit 0 quadrant
    // A may be reached, bit 1 quadrant B; dd its fourth value
    auto body = [&](const float4& aa, const float4& bb, const float2& cc, float dd, uint32_t sel) {
        const float tu = __builtin_fmaf(aa.y, ly, cc.x);  // fma(-A'y, ly, U0)
        const float tv = __builtin_fmaf(aa.w, ly, cc.y);  // fma(-B'y, ly, V0)
        if constexpr (V::kContrib) {
            uint32_t qA = 0u, qB = 0u;
            if (sel & 1u) qA = pixel_w(lxA, tu, tv, aa, bb, TA, qsA);
            if (sel & 2u) qB = pixel_w(lxB, tu, tv, aa, bb, TB, qsB);
            // (every lane again: the record's id is the first staged value)
            if constexpr (V::kTopK > 0)
                v.insert2(topA, topB, bb.y, qA, qB);
            else
                v.scatter(bb.y, qA + qB, qA > qB ? qA : qB,
                          (uint32_t)__popcll(__ballot(qA != 0u)) + (uint32_t)__popcll(__ballot(qB != 0u)));
        } else {
            if (sel & 1u) pixel(lxA, tu, tv, aa, bb, dd, TA, A);
            if (sel & 2u) pixel(lxB, tu, tv, aa, bb, dd, TB, B);
        }
    };

    // Gathers as composite_kernel: wave w loads records 64w..64w+63 of a
    // batch as 192 adjacent 16-B chunks (lane + 64 i), the next batch in
    // flight while the current one is composited.
    const uint32_t last = rg.y > rg.x ? rg.y - 1u : rg.x;
    float4 rc[3] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f),
                    make_float4(0.f, 0.f, 0.f, 0.f)};
    typename V::Own own{};  // what the policy gathers for this lane's own record of the batch in flight
    uint32_t id_next = 0;
    // (the chunk's record and part are recomputed per gather from a lane id
    // the compiler cannot hoist: kept live across the walk they spilled)
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
        own = v.gather(a, own_id);
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
        // progress-ordered issue priority: a workgroup's waves drop
        // priority as they walk batches, so late-started workgroups are not
        // starved behind older ones (age arbitration) into a long drain
        {
            const uint32_t nb = (b - rg.x) / kTileThreads;
            if (nb == 0) __builtin_amdgcn_s_setprio(GS_STRIP_PRIO_TOP);
            else if (nb == 2) __builtin_amdgcn_s_setprio(GS_STRIP_PRIO_TOP > 1 ? GS_STRIP_PRIO_TOP - 1 : 0);
            else if (nb == 4) __builtin_amdgcn_s_setprio(GS_STRIP_PRIO_TOP > 2 ? GS_STRIP_PRIO_TOP - 2 : 0);
            else if (nb == 6) __builtin_amdgcn_s_setprio(0);
        }
        if (b != rg.x) {  // early out (one LDS barrier, as composite_kernel)
            const bool open = __ballot(!fin(TA) || !fin(TB)) != 0;
            if (lane == 0) sopen[wave] = open ? 1u : 0u;
            block_lds_sync();
            const uint4 o = *reinterpret_cast<const uint4*>(sopen);
            if ((o.x | o.y | o.z | o.w) == 0u) break;
        }
        if (!V::kWholeFrame && rg.y - b > (uint32_t)kTileThreads) {
            const uint32_t left = rg.y - b - (uint32_t)kTileThreads;
            fetched += left < (uint32_t)kTileThreads ? left : (uint32_t)kTileThreads;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) srec[192u * wave + lane + 64u * (uint32_t)i] = rc[i];
        // (the slot's fourth value; the barrier above freed the last batch's)
        if constexpr (V::kFourth) sv3[tid] = v.values(own, 0.0f, 0.0f, 0.0f).w;
        wave_lds_sync();  // the wave's 64 slots are only touched by this wave until the barrier
        if (b + tid < rg.y) {
            // raw (cx, cy, ax, ay) (bx, by, op, r) (g, b, rect_lo, rect_hi),
            // staged for both tiles (scaled conic, offsets at each tile's origin)
            float4* st = &srec[3u * tid];
            const float4 r0 = st[0], r1 = st[1], r2 = st[2];
            const float ax = r0.z * kConicScale, ay = r0.w * kConicScale;
            const float bxs = r1.x * kConicScale, bys = r1.y * kConicScale;
            const float exl = ftx0 - r0.x, exr = ftx1 - r0.x, ey = r0.y - fty0;
            const float aye = ay * ey, bye = bys * ey;
            const float4 val = v.values(own, r1.w, r2.x, r2.y);
            st[0] = make_float4(ax, -ay, bxs, -bys);
            st[1] = make_float4(r1.z, val.x, val.y, val.z);
            st[2] = make_float4(__builtin_fmaf(ax, exl, aye), __builtin_fmaf(bxs, exl, bye), __builtin_fmaf(ax, exr, aye),
                                __builtin_fmaf(bxs, exr, bye));
            // the 8 quadrants (columns c = 0..3 of 8 px from tx0, rows r = 0..1
            // from ty0) the rect reaches and the cell mask does not rule out;
            // bit 4 (c >> 1) + 2 r + (c & 1): wave w's selector is bits 2w, 2w+1
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
                // the rect's cell grid starts at (x0 >> 3, y0 >> 3); column c is
                // rect cell dx + c, row r rect cell dy + r
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
        // wave-level compaction of the records reaching an open quadrant of
        // this strip (index order kept), with their selectors
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
            // three empty entries (selector 0) after the list: the half pair of an
            // odd list and the walk's unconditional read-ahead of the next pair
            if (lane < 3u) wlist[wave][nl + lane] = 0;
        }
        wave_lds_sync();  // wlist[wave] is only touched by this wave
        // two records per step, both records' LDS reads issued before either
        // body; the next pair of entries is read one step ahead.  The c half
        // read depends on the wave's tile, so the walk is instantiated per tile.
        auto walk = [&](auto tile) {
            constexpr uint32_t kC = 32u + 8u * decltype(tile)::value;
            const char* base = reinterpret_cast<const char*>(srec);
            if (nl == 0u) return;
            auto ld4 = [&](uint32_t o) { return *reinterpret_cast<const float4*>(base + o); };
            auto ld2 = [&](uint32_t o) { return *reinterpret_cast<const float2*>(base + o); };
            // the fourth value: slot byte offset 48 k -> its byte offset 4 k
            const char* base3 = reinterpret_cast<const char*>(sv3);
            auto ld1 = [&](uint32_t o) -> float {
                if constexpr (V::kFourth) return *reinterpret_cast<const float*>(base3 + o / 12u);
                else return 0.0f;
            };
            // Rolling read-ahead, one record deep: while record i is
            // composited, record i + 1's reads are in flight (two register
            // sets, A and B, alternate), so every LDS read has a record's
            // bodies to hide behind.
            uint32_t w2 = wl2[0];
            uint32_t o = w2 & 0x3FFFu;
            float4 aA = ld4(o), bA = ld4(o + 16u);
            float2 cA = ld2(o + kC);
            float dA = ld1(o);
            for (uint32_t i = 0; i < nl; i += 2) {
                if (__ballot(!fin(TA) || !fin(TB)) == 0) break;
                const uint32_t e = __builtin_amdgcn_readfirstlane(w2);
                o = (w2 >> 16) & 0x3FFFu;
                const float4 aB = ld4(o), bB = ld4(o + 16u);
                const float2 cB = ld2(o + kC);
                const float dB = ld1(o);
                w2 = wl2[(i >> 1) + 1];  // (past the list: empty entries)
                body(aA, bA, cA, dA, (e >> 14) & 3u);
                o = w2 & 0x3FFFu;
                aA = ld4(o);
                bA = ld4(o + 16u);
                cA = ld2(o + kC);
                dA = ld1(o);
                body(aB, bB, cB, dB, e >> 30);
            }
        };
        if (wt) walk(std::integral_constant<uint32_t, 1>{});
        else walk(std::integral_constant<uint32_t, 0>{});
    }
    if (!V::kWholeFrame && tid == 0 && a.fetched) (void)atomicAdd(a.fetched, (unsigned long long)fetched);
    if (PASS == 1 && tid == 0 && a.wcost) a.wcost[2u * bin + half] = fetched;  // (the next bin order's cost)
#ifdef GS_COMPOSITE_TRACE
    __syncthreads();
    if (tid == 0 && blockIdx.x < 65536u) {
        g_comp_trace[4u * blockIdx.x + 0] = trace_t0;
        g_comp_trace[4u * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
        g_comp_trace[4u * blockIdx.x + 2] = wg;
        g_comp_trace[4u * blockIdx.x + 3] = fetched;
    }
#endif
    // PASS 1, per quadrant: a pixel still open at the end of a cut list keeps
    // its state for the fallback lists instead of its final value
    bool openA = false, openB = false, keepA = false, keepB = false;
    if constexpr (PASS == 1) {
        openA = __ballot(!fin(TA)) != 0;
        openB = __ballot(!fin(TB)) != 0;
        keepA = openA && trunc;
        keepB = openB && trunc;
    }
    // (pixel positions recomputed from a fresh lane id: kept live across the
    // loop they cost registers the walk needs)
    uint32_t ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0" : "=v"(ln));
    ln = __builtin_amdgcn_mbcnt_hi(~0u, ln);
    const int qx = (int)(tx0 + 16u * wt + (ln & 7u)), qy = (int)(ty0 + 8u * ws + (ln >> 3));
    const int orow = !V::kWholeFrame && a.compact ? owned_row * kBin + (qy - by * kBin) : qy;
    auto store = [&](bool res, bool keep, int px, float C0, float C1, float C2, float T, float C3) {
        if (px >= width || qy >= height || (PASS == 2 && !res)) return;  // (PASS 2: the rest was written by pass 1)
        const size_t pix = (size_t)qy * width + px;
        if (keep) {
            a.state[pix] = make_float4(C0, C1, C2, T);
            if constexpr (V::kFourth) a.state_d[pix] = C3;
        } else if constexpr (V::kFourth) {
            v.store(a, orow, px, make_float4(C0, C1, C2, 1.0f - T), C3);
        } else if (a.out_bgra8) {
            a.out_bgra8[(size_t)orow * width + px] = pack_bgra8(C0, C1, C2, 1.0f - T);
        } else {
            a.out[(size_t)orow * width + px] = make_float4(C0, C1, C2, 1.0f - T);
        }
    };
    if constexpr (!V::kContrib) {  // (a contrib pass writes no pixel)
        store(resA, keepA, qx, A[0], A[1], A[2], TA, A[kAcc - 1]);  // (C3: the fourth accumulator where one exists)
        store(resB, keepB, qx + 8, B[0], B[1], B[2], TB, B[kAcc - 1]);
    }
    if constexpr (V::kTopK > 0) {  // (an ids pass: every pixel of the frame, those of empty bins too)
        const size_t pix = (size_t)qy * width + qx;
        if (qx < width && qy < height) v.store(topA, pix);
        if (qx + 8 < width && qy < height) v.store(topB, pix + 8);
    }
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
// One composite launch of `tile` (one workgroup per 16x16 tile) or, for
// launches of many bins (composite_strip()), of `strip` (nullptr: the rule
// has no strip kernel); x: the kernels' arguments between a and nwg.  A small
// launch -- a rank's band at 8 ranks, a small frame -- runs the tile kernel:
// there the slowest workgroup bounds the launch, and a tile's walks one pixel
// per lane.  t0/t1 (optional) are recorded by the dispatch packet itself.
template <class KT, class KS, class... X>
inline hipError_t launch_composite_kernels(KT tile, KS strip, const CompositeArgs& a, hipStream_t st, hipEvent_t t0,
                                           hipEvent_t t1, const X&... x) {
    if (a.nrows < 0 || a.nrows > a.tiles_y || (!a.rows && a.nrows != a.tiles_y)) return hipErrorInvalidValue;
    constexpr bool kStripOk = !std::is_same_v<KS, std::nullptr_t>;
    const bool use_strip = kStripOk && composite_strip((uint32_t)(a.tiles_x * a.nrows));
    const uint32_t nwg = (uint32_t)((use_strip ? 2 : 4) * a.tiles_x * a.nrows);
    if (nwg == 0) {  // no owned tiles: the timing events still mark the (empty) stage
        if (t0 && hipEventRecord(t0, st) != hipSuccess) return hipGetLastError();
        if (t1 && hipEventRecord(t1, st) != hipSuccess) return hipGetLastError();
        return hipSuccess;
    }
    if constexpr (kStripOk) {
        if (use_strip) {
            hipExtLaunchKernelGGL(strip, dim3(nwg), dim3(kTileThreads), 0, st, t0, t1, 0, a, x..., nwg);
            return hipGetLastError();
        }
    }
    hipExtLaunchKernelGGL(tile, dim3(nwg), dim3(kTileThreads), 0, st, t0, t1, 0, a, x..., nwg);
    return hipGetLastError();
}

}  // namespace gs
