"""Scenes of degenerate and non-finite splat values (plain helper, shared by
test_degenerate_oracle.py and test_gpu_degenerate.py).

zoo(): the suite's synthetic scene with classes of K splats overwritten on
the activated Scene (the values reach the kernels unchanged), at indices of
one seeded permutation, so a wave's lanes mix degenerate and ordinary splats;
plus two block-aligned runs of zero quaternions (a whole wave and a whole
workgroup of culled splats).  thresholds(): splats on the view axis at the
depths around the fragment-discard cull and the half overflow of the depth
key.  same_frame(): the comparison that allows a NaN's sign and payload.

Every NaN written here is numpy's canonical quiet NaN (0x7FC00000), so no
arithmetic on either side can produce the guard sentinel's payload."""
import functools

import numpy as np

K = 48             # splats per class
N_BASE = 6000
N_DENSE = 60000    # dense=True: more base splats ...
GROW_DENSE = 3.0   # ... with scales grown (chosen on the CPU oracle: see test_degenerate_oracle.py)
RUNS = ((1024, 256), (2112, 64))  # (first index, length): a whole workgroup, a whole wave (not at a block's start)
FULL_FRAME = ("scale_inf", "scale_1e19", "scale_needle")  # given opacity 0.02-0.05: they tint, not saturate
SH_CLASSES = ("sh_nan", "sh_inf", "sh_1e30", "sh_dc_zero_nan_rest")
CLASS_NAMES = ("rot_zero", "rot_1e-20", "rot_1e19", "rot_nan",
               "scale_zero", "scale_axis_zero", "scale_inf", "scale_1e19", "scale_1e10", "scale_1e-30",
               "scale_negated", "scale_nan", "scale_needle",
               "opacity_zero", "opacity_one", "opacity_1.5", "opacity_-0.5", "opacity_nan",
               "color_nan", "color_range",
               "pos_x_nan", "pos_y_inf", "pos_z_-1e30")


def _apply(sc, name, idx, rng):
    """Overwrites class `name` on splats idx of the activated scene."""
    k = len(idx)
    lane = np.arange(k)
    if name in FULL_FRAME:
        sc.opacity[idx] = rng.uniform(0.02, 0.05, k).astype(np.float32)
    if name == "rot_zero":
        sc.rot[idx] = 0.0
    elif name == "rot_1e-20":
        sc.rot[idx] *= np.float32(1e-20)   # qs = |q|^2 ~ 1e-40: subnormal
    elif name == "rot_1e19":
        sc.rot[idx] *= np.float32(1e19)    # qs overflows to inf
    elif name == "rot_nan":
        sc.rot[idx, lane % 4] = np.nan
    elif name == "scale_zero":
        sc.scale[idx] = 0.0
    elif name == "scale_axis_zero":
        sc.scale[idx, lane % 3] = 0.0
    elif name == "scale_inf":
        sc.scale[idx] = np.inf
    elif name == "scale_1e19":
        sc.scale[idx] = 1e19
    elif name == "scale_1e10":
        sc.scale[idx] = 1e10
    elif name == "scale_1e-30":
        sc.scale[idx] = 1e-30
    elif name == "scale_negated":
        sc.scale[idx] *= np.float32(-1.0)
    elif name == "scale_nan":
        sc.scale[idx, lane % 3] = np.nan
        sc.scale[idx[3::4]] = np.nan       # (every fourth: all three, a NaN bound in the band cull)
    elif name == "scale_needle":
        sc.scale[idx] = np.float32([100.0, 1e-4, 1e-4])
    elif name == "opacity_zero":
        sc.opacity[idx] = 0.0
    elif name == "opacity_one":
        sc.opacity[idx] = 1.0
    elif name == "opacity_1.5":
        sc.opacity[idx] = 1.5
    elif name == "opacity_-0.5":
        sc.opacity[idx] = -0.5
    elif name == "opacity_nan":
        sc.opacity[idx] = np.nan
    elif name == "color_nan":
        sc.color[idx, lane % 3] = np.nan
    elif name == "color_range":
        sc.color[idx] = np.float32([2.0, -1.0, 0.5])
    elif name == "pos_x_nan":
        sc.pos[idx, 0] = np.nan
    elif name == "pos_y_inf":
        sc.pos[idx, 1] = np.inf
    elif name == "pos_z_-1e30":
        sc.pos[idx, 2] = -1e30
    elif name == "sh_nan":
        sc.sh_rest[idx, (lane * 7) % 45] = np.nan
    elif name == "sh_inf":
        sc.sh_rest[idx, (lane * 7) % 45] = np.inf
    elif name == "sh_1e30":
        sc.sh_rest[idx] = 1e30
    elif name == "sh_dc_zero_nan_rest":   # the all-zero f_dc quirk must win over the NaN rest
        sc.color[idx] = 0.0
        sc.sh_rest[idx] = np.nan
    else:
        raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _zoo(W, H, sh, dense):
    from gaussian_splat_amd import scene as S
    from gaussian_splat_amd.api import default_camera
    n = N_DENSE if dense else N_BASE
    sc = S.activate(S.synthetic_raw(n, seed=41, aspect=W / H, rest=sh > 0), sh)
    for f in ("pos", "rot", "scale", "opacity", "color", "sh_rest"):  # (own, writable arrays)
        if getattr(sc, f) is not None:
            setattr(sc, f, np.array(getattr(sc, f), np.float32, order="C"))
    if dense:
        sc.scale *= np.float32(GROW_DENSE)
    rng = np.random.default_rng([41, int(dense)])
    in_run = np.zeros(n, bool)
    for a, m in RUNS:
        in_run[a:a + m] = True
    perm = rng.permutation(np.nonzero(~in_run)[0])
    names = CLASS_NAMES + (SH_CLASSES if sh > 0 else ())
    classes = {}
    for c, name in enumerate(names):
        idx = np.sort(perm[c * K:(c + 1) * K])
        _apply(sc, name, idx, rng)
        classes[name] = idx
    run = np.nonzero(in_run)[0]
    sc.rot[run] = 0.0
    classes["rot_zero_runs"] = run
    touched = np.zeros(n, bool)
    for idx in classes.values():
        assert not touched[idx].any()
        touched[idx] = True
    classes["untouched"] = np.nonzero(~touched)[0]
    for f in ("pos", "rot", "scale", "opacity", "color", "sh_rest"):
        v = getattr(sc, f)
        if v is not None:
            bits = v.view(np.uint32)
            assert np.all(bits[np.isnan(v)] == 0x7FC00000)  # canonical NaNs only
            v.setflags(write=False)
    for idx in classes.values():
        idx.setflags(write=False)
    cam = default_camera(W, H)
    return sc, cam.getViewMatrix(), cam.getProjectionMatrix(), classes


def zoo(W, H, sh=0, dense=False):
    """(scene, V, P, classes) for the default camera of a W x H frame.
    classes: name -> sorted index array, including "rot_zero_runs" (the two
    contiguous runs) and "untouched" (the base splats left as generated).
    Cached; the arrays are read-only."""
    return _zoo(int(W), int(H), int(sh), bool(dense))


THRESHOLD_DEPTHS = (0.0009, 0.001, 0.0011, 65503.0, 65504.0, 65519.0, 65520.0, 1e5)


@functools.lru_cache(maxsize=None)
def thresholds(W, H):
    """(scene, V, P, depths): one splat per view depth of THRESHOLD_DEPTHS, its
    centre on the view axis and its scale 0.01 of its depth (the same few
    pixels at every depth).  The view matrix is the identity (eye at the
    origin, looking down -z), so zFront is the float32 depth exactly; the
    projection's planes (5e-4, 1e6) leave every depth inside the z-clip."""
    from gaussian_splat_amd.api import Scene, perspective
    d = np.asarray(THRESHOLD_DEPTHS, np.float32)
    n = len(d)
    rng = np.random.default_rng(43)
    pos = np.zeros((n, 3), np.float32)
    pos[:, 2] = -d
    sc = Scene(pos=pos, rot=rng.standard_normal((n, 4)), scale=np.float32(0.01) * d[:, None] * rng.uniform(0.7, 1.4, (n, 3)),
               opacity=rng.uniform(0.3, 0.6, n), color=rng.uniform(0.0, 1.0, (n, 3)),
               sh_rest=rng.standard_normal((n, 45)) * 0.1)
    V = np.eye(4, dtype=np.float32)
    P = perspective(45.0, np.float32(W) / np.float32(H), 5e-4, 1e6)
    return sc, V, P, d


def same_frame(img, ref):
    """(pixels whose NaN-ness differs in some channel, channel values that are
    not NaN in either frame and differ bitwise); both must be 0.  A NaN's
    sign and payload are not compared (an invalid operation's default NaN is
    not the same on every machine, and the contract does not fix them).
    BGRA8 frames: (0, differing bytes)."""
    img, ref = np.asarray(img), np.asarray(ref)
    assert img.shape == ref.shape and img.dtype == ref.dtype, (img.shape, ref.shape, img.dtype, ref.dtype)
    if img.dtype == np.uint8:
        return 0, int(np.count_nonzero(img != ref))
    na, nb = np.isnan(img), np.isnan(ref)
    both = ~na & ~nb
    nbit = int(np.count_nonzero(both & (img.view(np.uint32) != ref.view(np.uint32))))
    return int(np.count_nonzero((na != nb).any(axis=-1))), nbit


def same_records(rec, ref):
    """same_frame for record arrays (RECORD_DTYPE rows as 12 words): the float
    fields under the NaN allowance, the rect words as they are."""
    a = np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 12)
    b = np.ascontiguousarray(ref).view(np.uint32).reshape(-1, 12)
    fa, fb = a[:, :10].view(np.float32), b[:, :10].view(np.float32)
    na, nb = np.isnan(fa), np.isnan(fb)
    nbit = int(np.count_nonzero(~na & ~nb & (a[:, :10] != b[:, :10]))) + int(np.count_nonzero(a[:, 10:] != b[:, 10:]))
    return int(np.count_nonzero((na != nb).any(axis=-1))), nbit
