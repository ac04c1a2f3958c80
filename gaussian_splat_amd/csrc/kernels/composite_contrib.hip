// composite_contrib.hip — per-splat blend weight totals of a frame
// (gs_render_contrib).
//
// The other composites gather from splats to pixels; this pass scatters from
// pixels to splats.  For every fragment the colour frame composites, the
// factor w that multiplies the splat's colour there (tile rule: alpha T, the
// fp32 product as the kernel forms it; live50 rule: T before the fragment) is
// quantised, q(w) = (uint32_t)(min(max(w, 0), 1) * 2^24), and per splat the
// pass adds up sum q, the number of pixels with q > 0 and max q, over the
// pixels the caller's mask counts.  Integers, so the totals do not depend on
// the order the atomics land in.
//
// A frame queues one launch behind its colour composite, over the same whole
// lists (pass 0: contrib frames carry no depth cuts).  The kernels here are
// entry points only: the composite bodies of composite_kernels.h with the
// ContribValues policy, which carries T per pixel and no colour, writes no
// pixel, reduces each record's weights over the wave (ballot, DPP) and lets
// one lane issue the three atomics of a (record, wave) with a weight.  Colour,
// depth and feature frames never launch anything from here.
#include "composite_kernels.h"

namespace gs {

template <int MODE>
GS_COMPOSITE_KERNEL((ContribValues::kWaves)) composite_contrib_kernel(CompositeArgs a, ContribArgs k, uint32_t nwg) {
    composite_tile_body<MODE, false, 0, 0>(a, nwg, ContribValues{k});
}

template <int MODE>
GS_COMPOSITE_KERNEL((ContribValues::kWaves)) composite_strip_contrib_kernel(CompositeArgs a, ContribArgs k, uint32_t nwg) {
    composite_strip_body<MODE, 0>(a, nwg, ContribValues{k});
}

template <int MODE>
static hipError_t launch_contrib_pass(const CompositeArgs& a, const ContribArgs& k, hipStream_t st) {
    return launch_composite_kernels(composite_contrib_kernel<MODE>, composite_strip_contrib_kernel<MODE>, a, st, nullptr,
                                    nullptr, k);
}

hipError_t launch_composite_contrib(const CompositeArgs& a, const ContribArgs& k, int mode, hipStream_t st) {
    // tile / live50 rules over whole lists of whole frames: no cap, no slabs, no MLAB, no cut passes, no bands
    if (!k.sum || !k.count || !k.max || a.cap > 0 || a.slab || a.pass || (mode != 0 && mode != 1))
        return hipErrorInvalidValue;
    if (a.rows || a.compact || a.nrows != a.tiles_y || a.tiles_x <= 0 || a.tiles_y <= 0) return hipErrorInvalidValue;
    if (!a.vals || !a.ranges || !a.rec) return hipErrorInvalidValue;
    return mode == 0 ? launch_contrib_pass<0>(a, k, st) : launch_contrib_pass<1>(a, k, st);
}

}  // namespace gs
