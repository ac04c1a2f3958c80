// composite_ids.hip — each pixel's top-K splats by blend weight
// (gs_render_ids).
//
// The question between the colour composites (what a pixel looks like) and
// the contrib pass (what a splat puts into the frame): which splats make up a
// pixel.  For every fragment the colour frame composites, the contrib pass's
// quantised weight q(w) is formed at the same place from the same operands;
// per pixel the pass keeps the K candidates of largest (q, ~id) in registers,
// counts the candidates, and stores ids, weights and the count at the end of
// the pixel.  No LDS beyond the bodies' own and no atomics.
//
// A frame queues one launch behind its colour composite, over the same whole
// lists (pass 0: ids frames carry no depth cuts).  Every bin of the frame has
// its workgroups in the launch and a workgroup with an empty list falls through
// to the store, so the pixels of empty bins are written as every other pixel
// (GS_ID_NONE, 0, 0) and the outputs need no clear.  The kernels here are entry
// points only: the composite bodies of composite_kernels.h with the IdValues<K>
// policy, K = 1, 2 or 4 (3 slots run K = 4 and store three).  Colour, depth,
// feature and contrib frames never launch anything from here.
#include "composite_kernels.h"

namespace gs {

// Waves per SIMD the instances are built for, from what the compiler reports
// (tests/test_ids_kernel_resources.py): the K (q, id) pairs and the counter per
// pixel are 2 K + 1 VGPRs in the tile body and 4 K + 2 in the strip body, on
// top of the contrib kernels' 56-57.
constexpr int ids_waves(int k, bool strip) { return !strip ? 8 : k == 4 ? 5 : 7; }

template <int MODE, int K>
GS_COMPOSITE_KERNEL((ids_waves(K, false))) composite_ids_kernel(CompositeArgs a, IdArgs i, uint32_t nwg) {
    composite_tile_body<MODE, false, 0, 0>(a, nwg, IdValues<K>{i});
}

template <int MODE, int K>
GS_COMPOSITE_KERNEL((ids_waves(K, true))) composite_strip_ids_kernel(CompositeArgs a, IdArgs i, uint32_t nwg) {
    composite_strip_body<MODE, 0>(a, nwg, IdValues<K>{i});
}

template <int MODE, int K>
static hipError_t launch_ids_pass(const CompositeArgs& a, const IdArgs& i, hipStream_t st) {
    return launch_composite_kernels(composite_ids_kernel<MODE, K>, composite_strip_ids_kernel<MODE, K>, a, st, nullptr,
                                    nullptr, i);
}

template <int MODE>
static hipError_t launch_ids_rule(const CompositeArgs& a, const IdArgs& i, hipStream_t st) {
    return i.slots == 1 ? launch_ids_pass<MODE, 1>(a, i, st)
           : i.slots == 2 ? launch_ids_pass<MODE, 2>(a, i, st)
                          : launch_ids_pass<MODE, 4>(a, i, st);
}

hipError_t launch_composite_ids(const CompositeArgs& a, const IdArgs& i, int mode, hipStream_t st) {
    // tile / live50 rules over whole lists of whole frames: no cap, no slabs, no MLAB, no cut passes, no bands
    if (!i.ids || i.slots < 1 || i.slots > kMaxIdSlots || a.cap > 0 || a.slab || a.pass || (mode != 0 && mode != 1))
        return hipErrorInvalidValue;
    if (a.rows || a.compact || a.nrows != a.tiles_y || a.tiles_x <= 0 || a.tiles_y <= 0) return hipErrorInvalidValue;
    if (a.order || !a.vals || !a.ranges || !a.rec) return hipErrorInvalidValue;
    if (((uintptr_t)i.ids | (uintptr_t)i.q | (uintptr_t)i.count) & 3u) return hipErrorInvalidValue;
    IdArgs v = i;
    v.vec = 0;
    if (i.slots == 4) v.vec = (((uintptr_t)i.ids & 15u) == 0 ? 1 : 0) | (i.q && ((uintptr_t)i.q & 15u) == 0 ? 2 : 0);
    return mode == 0 ? launch_ids_rule<0>(a, v, st) : launch_ids_rule<1>(a, v, st);
}

}  // namespace gs
