// composite_depth.hip — the composite with one more accumulator per pixel: the
// accumulated view depth D (gs_render_depth).
//
// D is composited exactly as a colour channel whose per-splat value is the
// fp32 zF of the projection (zf_plane_kernel: -xform_row(V, 2, x, y, z), the
// preprocess's own value): the same fragments, order, weights and break rule
// as C0..C2, from D = 0, one pass over the lists, no atomics.  The colour
// frame is gs_render's bit for bit.
//
// The kernels here are entry points only: the composite bodies of
// composite_kernels.h with the DepthValues policy (tile and live50 rules, no
// cap, no slabs, no BGRA8; depth-cut passes 0/1/2), built for 6 waves per
// SIMD.  Colour-only frames never launch anything from here.
#include "composite_kernels.h"

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

template <int MODE, int PASS>
GS_COMPOSITE_KERNEL(DepthValues::kWaves) composite_depth_kernel(CompositeArgs a, uint32_t nwg) {
    composite_tile_body<MODE, false, 0, PASS>(a, nwg, DepthValues{});
}

template <int MODE, int PASS>
GS_COMPOSITE_KERNEL(DepthValues::kWaves) composite_strip_depth_kernel(CompositeArgs a, uint32_t nwg) {
    composite_strip_body<MODE, PASS>(a, nwg, DepthValues{});
}

template <int MODE, int PASS>
static hipError_t launch_depth_mode(const CompositeArgs& a, hipStream_t st, hipEvent_t t0, hipEvent_t t1) {
    return launch_composite_kernels(composite_depth_kernel<MODE, PASS>, composite_strip_depth_kernel<MODE, PASS>, a, st, t0,
                                    t1);
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
