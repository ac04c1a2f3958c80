"""CPU reference of gs_render_depth's depth image.

D is composited exactly as a colour channel whose per-splat value is the fp32
zF.  The oracle composites whatever float a record carries in its `r` channel
with C0 = fmaf(r, w, C0) and no clamp (ora_composite_records), so the depth
image is the red channel of the frame's own records with r replaced by the
oracle's zF (ora_debug.zf): the same fragments, order, weights and break rule
as the colour frame, whose G, B and A channels must therefore come out
unchanged, bit for bit.  depth_ref asserts that on every call."""
import numpy as np


def _bits(a, b):
    return int(np.count_nonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)))


def project_zf(scene, V, P, W, H, sh_degree=0):
    """(records, depth keys, tiles per splat, zF per splat) of the oracle's projection."""
    from oracle import oracle_py as O
    rec_d, dbg = O.project_debug(scene, V, P, W, H, sh_degree)
    rec, dkey, ntiles = O.project(scene, V, P, W, H, sh_degree)
    vis = ntiles > 0
    assert _bits(rec_d[vis].view(np.uint32), rec[vis].view(np.uint32)) == 0  # (one projection, two entry points)
    return rec, dkey, ntiles, dbg["zf"].astype(np.float32)


def depth_from_projection(scene, V, P, W, H, mode, sh_degree, proj):
    """depth_ref from a projection computed once (project_zf) and shared between the rules."""
    from oracle import oracle_py as O
    rec, dkey, ntiles, zf = proj
    colour, _ = O.render(scene, V, P, W, H, sh_degree=sh_degree, mode=mode)
    again = O.composite_records(rec, dkey, W, H, mode=mode)
    assert _bits(again, colour) == 0  # the record composite is the oracle's frame
    drec = rec.copy()
    drec["r"] = np.where(ntiles > 0, zf, np.float32(0.0)).astype(np.float32)
    d = O.composite_records(drec, dkey, W, H, mode=mode)
    assert _bits(d[..., 1:], colour[..., 1:]) == 0  # G, B and A untouched: same fragments, weights and breaks
    depth = np.ascontiguousarray(d[..., 0])
    depth.setflags(write=False)
    colour.setflags(write=False)
    return depth, colour


def depth_ref(scene, V, P, W, H, mode, sh_degree=0, with_colour=False):
    """The accumulated depth image (H, W) float32 of the frame; with_colour: also the oracle's colour frame."""
    depth, colour = depth_from_projection(scene, V, P, W, H, mode, sh_degree, project_zf(scene, V, P, W, H, sh_degree))
    return (depth, colour) if with_colour else depth
