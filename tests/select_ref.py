"""Shared helpers of the gs_select / gs_prune tests: the numpy reference is
Scene.subset(index); scenes are compared on bits, so NaN payloads count."""
import numpy as np

FIELDS = ("pos", "rot", "scale", "opacity", "color", "sh_rest")
GS_OK, GS_ERR_INVALID_ARG, GS_ERR_UNSUPPORTED, GS_ERR_STATE = 0, 1, 7, 8
NAN_PAYLOAD = 0x7FC5A5A5  # a quiet NaN with a payload no arithmetic produces
SELECT_BLOCK = 1024  # mask bytes per compaction block (kSelectBlock, gs_kernels.h): four waves of 256


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


def scene_diff(a, b):
    """Differing 32-bit words between two Scenes, per array: {} when they are the same bits."""
    out = {}
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if x.shape != y.shape:
            out[f] = (x.shape, y.shape)
        elif bits(x, y):
            out[f] = bits(x, y)
    return out


def payload_scene(n, sh, seed=1):
    """A seeded scene of n splats (SH coefficients for sh > 0) in which a few splats carry a NaN
    with a payload in their colour and SH coefficients: a copy through float arithmetic would
    not keep it.  Positions, scales and opacities stay finite (the scene still renders)."""
    from gaussian_splat_amd import scene as S
    sc = S.synthetic_scene(n, seed=seed, sh_degree=sh)
    if n >= 8:
        at = np.arange(3, n, max(n // 5, 1))
        sc.color.view(np.uint32)[at, 1] = NAN_PAYLOAD
        if sc.sh_rest is not None:
            sc.sh_rest.view(np.uint32)[at, 0] = NAN_PAYLOAD + 1
            sc.sh_rest.view(np.uint32)[at, 44] = NAN_PAYLOAD + 2
    return sc


def select_lists(n, seed=11):
    """name -> uint32 list over a scene of n splats: identity, reversal, a seeded permutation,
    repeats with m = n + 37, m = 1, m = 0."""
    rng = np.random.default_rng(seed)
    out = {"identity": np.arange(n), "reversal": np.arange(n)[::-1].copy(), "permutation": rng.permutation(n),
           "repeats": rng.integers(0, max(n, 1), n + 37) if n else np.zeros(0, np.int64),
           "one": np.array([n // 2]) if n else np.zeros(0, np.int64), "none": np.zeros(0, np.int64)}
    return {k: np.ascontiguousarray(v, dtype=np.uint32) for k, v in out.items()}


def prune_masks(n, seed=13, block=SELECT_BLOCK):
    """name -> uint8 mask of n entries: all, none, first only, last only, alternating, a seeded
    half, the values 0 / 1 / 255, and one run of ones straddling a compaction block boundary
    (or the middle of a scene shorter than a block)."""
    rng = np.random.default_rng(seed)
    z = np.zeros(n, np.uint8)
    first, last, alt, run = z.copy(), z.copy(), z.copy(), z.copy()
    first[:1] = 1
    last[-1:] = 1
    alt[::2] = 1
    edge = block if n > block else n // 2
    run[max(edge - 37, 0):edge + 41] = 1
    return {"all": np.ones(n, np.uint8), "none": z, "first": first, "last": last, "alternating": alt,
            "half": (rng.random(n) < 0.5).astype(np.uint8), "values": rng.choice(np.array([0, 1, 255], np.uint8), n),
            "run": run}
