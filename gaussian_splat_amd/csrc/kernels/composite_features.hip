// composite_features.hip — per-splat feature channels composited per pixel
// (gs_render_features).
//
// The caller's features are an N x K float matrix, row i for splat i.  Every
// channel F_k is composited exactly as a colour channel whose per-splat value
// is features[i][k], from F_k = 0, not clamped, not normalised; termination
// depends on T alone.  One launch composites four channels, first .. first + 3,
// into the H x W x K image (channels innermost): T and four accumulators per
// pixel, no colour.  A frame queues ceil(K / 4) launches behind its colour
// composite, over the same whole lists (pass 0: feature frames carry no depth
// cuts).
//
// The kernels here are entry points only: the composite bodies of
// composite_kernels.h with the FeatureValues<VIN, VOUT> policy (16-B or dword
// gather and store, picked on the host per launch), the depth kernels' class.
// Colour and depth frames never launch anything from here.
#include "composite_kernels.h"

namespace gs {

template <int MODE, bool VIN, bool VOUT>
GS_COMPOSITE_KERNEL((FeatureValues<VIN, VOUT>::kWaves)) composite_feat_kernel(CompositeArgs a, FeatureArgs f, uint32_t nwg) {
    composite_tile_body<MODE, false, 0, 0>(a, nwg, FeatureValues<VIN, VOUT>{f});
}

template <int MODE, bool VIN, bool VOUT>
GS_COMPOSITE_KERNEL((FeatureValues<VIN, VOUT>::kWaves)) composite_strip_feat_kernel(CompositeArgs a, FeatureArgs f, uint32_t nwg) {
    composite_strip_body<MODE, 0>(a, nwg, FeatureValues<VIN, VOUT>{f});
}

template <int MODE, bool VIN, bool VOUT>
static hipError_t launch_feat_pass(const CompositeArgs& a, const FeatureArgs& f, hipStream_t st) {
    return launch_composite_kernels(composite_feat_kernel<MODE, VIN, VOUT>, composite_strip_feat_kernel<MODE, VIN, VOUT>, a, st,
                                    nullptr, nullptr, f);
}

template <int MODE>
static hipError_t launch_feat_mode(const CompositeArgs& a, const FeatureArgs& f, bool vin, bool vout, hipStream_t st) {
    if (vin) return vout ? launch_feat_pass<MODE, true, true>(a, f, st) : launch_feat_pass<MODE, true, false>(a, f, st);
    return vout ? launch_feat_pass<MODE, false, true>(a, f, st) : launch_feat_pass<MODE, false, false>(a, f, st);
}

hipError_t launch_composite_features(const CompositeArgs& a, const float* feat, float* out, int channels, int mode,
                                     hipStream_t st) {
    // tile / live50 rules over whole lists of whole frames: no cap, no slabs, no MLAB, no cut passes, no bands
    if (!out || channels < 1 || channels > kMaxFeatureChannels || a.cap > 0 || a.slab || a.pass ||
        (mode != 0 && mode != 1))
        return hipErrorInvalidValue;
    if (a.rows || a.compact || a.nrows != a.tiles_y || a.tiles_x <= 0 || a.tiles_y <= 0) return hipErrorInvalidValue;
    if (!a.vals || !a.ranges || !a.rec) return hipErrorInvalidValue;
    // 16-B rows and pixels: whole groups of four channels, on 16-B aligned bases
    const bool vin = channels % 4 == 0 && reinterpret_cast<uintptr_t>(feat) % 16 == 0;
    const bool vout = channels % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    FeatureArgs f;
    f.feat = feat;
    f.out = out;
    f.channels = channels;
    for (int first = 0; first < channels; first += 4) {
        f.first = first;
        const hipError_t e = mode == 0 ? launch_feat_mode<0>(a, f, vin, vout, st) : launch_feat_mode<1>(a, f, vin, vout, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace gs
