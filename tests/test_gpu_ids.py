"""gs_render_ids on the GPU: the colour frame and each pixel's top-K splats by quantised blend
weight (ids, q, count), against the CPU oracle for equality (tests/ids_ref.py
over tests/contrib_ref.py's fragments).

Shapes: 333 x 211 runs composite_ids_kernel (77 bins), 1037 x 531 composite_strip_ids_kernel
(561 bins); 1024 x 512 / 1025 x 512 are the last tile-kernel and first strip-kernel bin counts;
17 x 9 and 1 x 1 the smallest frames.  The scenes, views, sentinels and cached references are
test_gpu_contrib.py's: a (scene, shape, rule)'s fragments are computed once per session, shared
with the contrib tests, and left unchanged."""
import functools

import numpy as np
import pytest

from conftest import orbit_views
from contrib_ref import contrib_fragments
from depth_ref import depth_from_projection, project_zf
from features_ref import features_from_projection
from ids_ref import ID_NONE, ids_ref, tie_counts
from test_gpu_contrib import GUARD, MODES, SENT32, SHAPES, SMALL, STACK_BACK, _key, _np, _ref
from test_gpu_depth_output import STRIP_MIN_BINS, _bins, _bits, _hip, _projection, _scene
from test_gpu_frame_shapes import _cat, _splats_at

pytestmark = pytest.mark.gpu

NAMES = ("ids", "q", "count")


@functools.lru_cache(maxsize=None)
def _want(key, mode, K):
    """ids_ref of a cached reference's fragments, computed once per (scene, shape, rule, K)."""
    W, H = key[1], key[2]
    out = ids_ref(_ref(key, mode)[3], W, H, K)
    for a in out:
        a.setflags(write=False)
    return out


def _u32(*tensors):
    """Device int32 tensors (or None) as the uint32 arrays they hold."""
    return tuple(None if t is None else t.cpu().numpy().view(np.uint32) for t in tensors)


def _same(got, want, what=None):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, name, bad.shape[0], bad[0].tolist(), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


# ------------------------------------------------------------------ 1. parity

PARITY = ([(W, H, m, c, fif, s, 0) for (W, H) in SHAPES for m in MODES for c in (False, True) for fif in (1, 2)
           for s in (1, 4)] +
          [(333, 211, "tile", True, 2, 2, 0), (333, 211, "tile", True, 2, 3, 0), (1037, 531, "live50", True, 2, 2, 0),
           (1037, 531, "live50", True, 2, 3, 0), (1037, 531, "tile", True, 2, 4, 3)])


@pytest.mark.parametrize("W,H,mode,cut,fif,slots,sh", PARITY)
def test_ids_parity(built, W, H, mode, cut, fif, slots, sh):
    """Four frames under a still camera: ids, q and count equal ids_ref on the first and the last
    frame; colour equals the oracle's and gs_render's on a second (whole-list) handle on every
    frame; every frame is a whole-list frame whatever depth_split says.  On the reference alone:
    at 333 x 211 nearly every pixel has more than 4 candidates (eviction; measured 99.99 %), at
    1037 x 531 some have none (3.2 %), most have 1..4 (partly filled slots) and over a fifth have
    more than 4 (29 %)."""
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1037, 531))
    sc, V, P, fr, cref, info, N = _ref(_key(W, H, sh), mode)
    want = _want(_key(W, H, sh), mode, slots)
    cnt = want[2]
    if (W, H) == (333, 211):
        assert (cnt > 4).mean() > 0.99, (cnt > 4).mean()
    else:
        assert (cnt == 0).any() and ((cnt >= 1) & (cnt <= 4)).mean() > 0.5 and (cnt > 4).mean() > 0.2, \
            ((cnt == 0).mean(), ((cnt >= 1) & (cnt <= 4)).mean(), (cnt > 4).mean())
    r = _hip(sc, mode=mode, depth_split=cut, sh_degree=sh, frames_in_flight=fif)
    plain = _hip(sc, mode=mode, depth_split=False, sh_degree=sh)
    for k in range(4):
        rgba, ids, q, count = r.render_ids(V, P, W, H, slots=slots)
        assert tuple(ids.shape) == (H, W, slots) and tuple(q.shape) == (H, W, slots) and tuple(count.shape) == (H, W)
        rgba = rgba.cpu().numpy()
        st = r.last_stats()
        assert _bits(rgba, plain.render_host(V, P, W, H)) == 0, k
        assert _bits(rgba, cref) == 0, k
        if k in (0, 3):
            _same(_u32(ids, q, count), want, k)
        assert st["cut_frame"] == 0, (k, st)
    print(f"{W}x{H} {mode} cuts {cut} fif {fif} slots {slots} sh {sh}: pairs {st['pairs']} fetched "
          f"{st['records_fetched']} count 0 {(cnt == 0).mean():.4f} 1..4 {((cnt >= 1) & (cnt <= 4)).mean():.4f} "
          f">4 {(cnt > 4).mean():.4f} longest tile list {info['longest_tile_list']}")
    # an ids frame's algorithmic composite bytes: its pass reads the range words and the fetched
    # records again (B0) and writes the slots' ids and weights and the counts
    ps = plain.last_stats()
    assert ps["cut_frame"] == 0 and st["records_fetched"] == ps["records_fetched"] > 0
    B0 = ps["bytes_composite"] - 16 * W * H
    assert st["bytes_composite"] - ps["bytes_composite"] == B0 + 4 * W * H * (2 * slots + 1)


# -------------------------------------------------------------------- 2. ties

TIE_WINDOW = (640, 300)  # the strip case's 96 x 64 window of the 1037 x 531 frame (its top left corner)


@functools.lru_cache(maxsize=None)
def _tie_ref(strip, mode):
    """(scene, V, P, W, H, fragments, colour): 400 splats about 6 px wide with opacities of
    2e-7 .. 4e-6, whose weights quantise to a few small integers, so that equal q is the rule
    among a pixel's heaviest fragments; alone in a 96 x 64 frame (tile kernel), or over a 96 x 64
    window of the 1037 x 531 parity scene (strip kernel)."""
    rng = np.random.default_rng(5)
    if strip:
        W, H = 1037, 531
        V, P = orbit_views(W, H, 1)[0]
        x0, y0 = TIE_WINDOW
        low = _splats_at(V, P, W, H, x0 + rng.uniform(0, 96, 400), y0 + rng.uniform(0, 64, 400), rng, sigma_px=6.0)
    else:
        W, H = 96, 64
        V, P = orbit_views(W, H, 1)[0]
        low = _splats_at(V, P, W, H, rng.uniform(0, W, 400), rng.uniform(0, H, 400), rng, sigma_px=6.0)
    low.opacity = rng.uniform(2e-7, 4e-6, 400).astype(np.float32)
    sc = _cat(_scene(4000, 7, 0, W / H, 3.0), low) if strip else low
    fr = contrib_fragments(sc, V, P, W, H, mode, 0, project_zf(sc, V, P, W, H, 0))
    return sc, V, P, W, H, fr, fr[3]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strip", [False, True])
def test_ids_ties(built, strip, mode):
    """Equal weights near the top: the order is q descending, then index ascending, whatever
    order the composite met the fragments in.  Conditions on the reference (measured on the
    oracle): 96 x 64, tile rule 2,345 equal-q neighbours within ranks <= 4 and 827 pixels tied
    across the slot-4 boundary, live50 rule 3,149 and 643; the window at (640, 300) of
    1037 x 531 (strip kernel), tile rule: 1,223 and 803.  Then equality for slots 1..4."""
    sc, V, P, W, H, fr, cref = _tie_ref(strip, mode)
    assert (_bins(W, H) > STRIP_MIN_BINS) == strip
    near, across = tie_counts(fr, W, H, 4)
    print(f"{W}x{H} {mode}: {near} equal-q neighbours within ranks <= 4, {across} pixels tied across the slot-4 boundary")
    if strip:
        assert across >= 100, (near, across)
    else:
        assert near >= 1000 and across >= 300, (near, across)
    r = _hip(sc, mode=mode)
    for slots in (1, 2, 3, 4):
        rgba, ids, q, count = r.render_ids(V, P, W, H, slots=slots)
        assert _bits(rgba.cpu().numpy(), cref) == 0, slots
        _same(_u32(ids, q, count), ids_ref(fr, W, H, slots), slots)


# ---------------------------------------- 3. edges of the kernel choice and of the frame

@pytest.mark.parametrize("W,H", [(1, 1), (17, 9), (1024, 512), (1025, 512)])
def test_ids_edges(built, W, H):
    """The last tile-kernel and first strip-kernel bin counts and the smallest frames, slots 4
    and 1, on test_contrib_bounds' scenes (the half-empty one and a covering one)."""
    assert (_bins(W, H) > STRIP_MIN_BINS) == ((W, H) == (1025, 512))
    scenes = ("half", (20000, 5, 0, max(W / H, 1.0), 2.0))
    if _bins(W, H) == 1:
        scenes = ("small_half", (SMALL[0], SMALL[1], 0, max(W / H, 1.0), SMALL[4]))
    for skey in scenes:
        key = (skey, W, H, 0)
        sc, V, P, fr, cref, info, N = _ref(key, "tile")
        r = _hip(sc)
        for slots in (4, 1, 4):
            rgba, ids, q, count = r.render_ids(V, P, W, H, slots=slots)
            _same(_u32(ids, q, count), _want(key, "tile", slots), (skey, slots))
            assert _bits(rgba.cpu().numpy(), cref) == 0, (skey, slots)


# ------------------------------------------------------------ 4. long lists

@pytest.mark.parametrize("W,H,mode", [(333, 211, "live50"), (1037, 531, "tile")])
def test_ids_long_lists(built, W, H, mode):
    """Lists of more than three 256-record batches and pixels that saturate: the 550 splats
    behind the saturated middle of the stack's bin are in no slot of the pixels that had stopped
    before them, and ids, q and count equal the reference."""
    key = ("stacked", W, H, 0)
    sc, V, P, fr, cref, info, N = _ref(key, mode)
    assert info["longest_tile_list"] >= 513, info
    cx, cy = (528, 272) if W == 1037 else (176, 112)
    sat = cref[..., 3] >= np.float32(1.0) - np.float32(0.01)
    assert sat[cy - 4:cy + 4, cx - 4:cx + 4].all()
    r = _hip(sc, mode=mode)
    for k, slots in enumerate((4, 1)):
        want = _want(key, mode, slots)
        rgba, ids, q, count = r.render_ids(V, P, W, H, slots=slots)
        got = _u32(ids, q, count)
        assert _bits(rgba.cpu().numpy(), cref) == 0, k
        _same(got, want, slots)
        mid = got[0][cy - 4:cy + 4, cx - 4:cx + 4]
        assert (mid != ID_NONE).all() and (mid < N - STACK_BACK).all()
        assert (got[2][cy - 4:cy + 4, cx - 4:cx + 4] > 4).all()


# ------------------------------------- 5. every element is written, and nothing else

class GuardedIds:
    """ids and q of W * H * slots entries and count of W * H, each between two guards of GUARD
    entries, all filled with a sentinel; shift: ids and q start that many entries later (1: not
    16-B aligned)."""

    def __init__(self, W, H, slots, shift=0):
        import torch
        self.n = (W * H * slots, W * H * slots, W * H)
        self.off = (GUARD + shift, GUARD + shift, GUARD)
        self.shapes = ((H, W, slots), (H, W, slots), (H, W))
        self.buf = [torch.full((n + 2 * GUARD + shift,), SENT32, dtype=torch.int32, device="cuda:0") for n in self.n]
        self.ids, self.q, self.count = (b[o:o + n].view(s) for b, o, n, s in zip(self.buf, self.off, self.n, self.shapes))
        assert self.buf[0].data_ptr() % 16 == 0 and self.buf[1].data_ptr() % 16 == 0
        assert self.ids.data_ptr() % 16 == 4 * (shift % 4) and self.q.data_ptr() % 16 == 4 * (shift % 4)

    def arrays(self, written=(True, True, True)):
        import torch
        torch.cuda.synchronize()
        out = []
        for b, o, n, s, wr, name in zip(self.buf, self.off, self.n, self.shapes, written, NAMES):
            raw = b.cpu().numpy().view(np.uint32)
            assert (raw[:o] == SENT32).all() and (raw[o + n:] == SENT32).all(), f"{name}: guard entries written"
            mid = raw[o:o + n]
            if wr:
                assert not (mid == SENT32).any(), f"{name}: entries never written"
            else:
                assert (mid == SENT32).all(), f"{name}: written though not wanted"
            out.append(mid.reshape(s).copy())
        return tuple(out)


@pytest.mark.parametrize("W,H", SHAPES)
def test_ids_every_element_is_written(built, W, H):
    """The small scene's left half: most bins have empty lists.  Into sentinel-filled arrays
    between guards: the guards stay, no sentinel is left inside, pixels without a candidate hold
    GS_ID_NONE, 0 and 0, and everything equals the reference; 16-B aligned arrays and arrays one
    element off (the dword stores) at slots 4, and slots 3, 2 and 1."""
    key = ("small_half", W, H, 0)
    sc, V, P, fr, cref, info, N = _ref(key, "tile")
    cnt = _want(key, "tile", 4)[2]
    assert (cnt == 0).mean() > 0.5 and (cnt > 0).any()
    r = _hip(sc)
    for slots, shift in ((4, 0), (4, 1), (3, 0), (2, 1), (1, 0)):
        g = GuardedIds(W, H, slots, shift)
        rgba = r.render_ids(V, P, W, H, slots=slots, ids=g.ids, q=g.q, count=g.count)[0]
        got = g.arrays()
        _same(got, _want(key, "tile", slots), (slots, shift))
        empty = got[2] == 0
        assert (got[0][empty] == ID_NONE).all() and (got[1][empty] == 0).all()
        assert _bits(rgba.cpu().numpy(), cref) == 0, (slots, shift)


# ------------------------------------------------------- 6. outputs not wanted

@pytest.mark.parametrize("W,H", SHAPES)
def test_ids_null_outputs(built, W, H):
    """NULL out_q, NULL out_count and both: the other outputs are what they are with all three,
    and the arrays not handed over are not written."""
    key = _key(W, H)
    sc, V, P, fr, cref, info, N = _ref(key, "tile")
    r = _hip(sc)
    for slots in (4, 1):
        want = _want(key, "tile", slots)
        for wq, wc in ((False, True), (True, False), (False, False)):
            g = GuardedIds(W, H, slots)
            rgba, ids, q, count = r.render_ids(V, P, W, H, slots=slots, ids=g.ids, q=g.q if wq else None,
                                               count=g.count if wc else None, want_q=wq, want_count=wc)
            assert (q is None) == (not wq) and (count is None) == (not wc)
            got = g.arrays(written=(True, wq, wc))
            _same((got[0], got[1] if wq else None, got[2] if wc else None), want, (slots, wq, wc))
            assert _bits(rgba.cpu().numpy(), cref) == 0


# ------------------------------------------- 7. against gs_render_contrib, no reference

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_ids_against_contrib(built, W, H, mode):
    """The same handle and view through both calls: the candidates of all pixels are the
    contrib call's counted fragments, the heaviest candidate of the frame is its largest max,
    and every splat in a first slot has a contrib count."""
    sc = _scene(*_key(W, H)[0])
    V, P = orbit_views(W, H, 1)[0]
    r = _hip(sc, mode=mode)
    _, cs, cc, cm = r.render_contrib(V, P, W, H)
    cs, cc, cm = _np(cs, cc, cm)
    ids4, q4, n4 = _u32(*r.render_ids(V, P, W, H, slots=4)[1:])
    ids1, q1, n1 = _u32(*r.render_ids(V, P, W, H, slots=1)[1:])
    assert int(n4.astype(np.uint64).sum()) == int(cc.astype(np.uint64).sum()) > 0
    assert (n1 == n4).all() and (ids1[..., 0] == ids4[..., 0]).all() and (q1[..., 0] == q4[..., 0]).all()
    assert int(q4[..., 0].max()) == int(cm.max()) > 0
    first = ids1[..., 0][ids1[..., 0] != ID_NONE]
    assert first.size > 0 and (first < cc.shape[0]).all() and (cc[first] > 0).all()
    assert ((ids1[..., 0] == ID_NONE) == (n1 == 0)).all()


# ------------------------------------------------------------- 8. unsupported

@pytest.mark.parametrize("opts", [dict(cap=32), dict(mode="mlab"), dict(shard=True)])
def test_ids_unsupported(built, opts):
    """cap > 0, MLAB and a handle configured as one rank of two: GS_ERR_UNSUPPORTED, and the
    output buffers stay untouched."""
    import torch
    from gaussian_splat_amd._lib import GsError, check, lib
    W, H = 333, 211
    opts = dict(opts)
    shard = opts.pop("shard", False)
    sc = _scene(40000, 7, 0, W / H, 3.0)
    V, P = orbit_views(W, H, 1)[0]
    r = _hip(sc, **opts)
    if shard:
        check(lib().gs_shard_configure(r._h, 0, 2, 0), "gs_shard_configure")
    g = GuardedIds(W, H, 4)
    out = torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda:0")
    with pytest.raises(GsError) as e:
        r.render_ids(V, P, W, H, out=out, ids=g.ids, q=g.q, count=g.count)
    assert e.value.status == 7 and "GS_ERR_UNSUPPORTED" in str(e.value) and "gs_render_ids" in str(e.value)
    g.arrays(written=(False, False, False))
    assert (out.cpu().numpy() == -3.0).all()
    with pytest.raises(GsError) as e:
        r.render_ids_host(V, P, W, H)
    assert e.value.status == 7
    if shard:  # back to one rank: the call works again
        check(lib().gs_shard_configure(r._h, 0, 1, 0), "gs_shard_configure")
        _same(r.render_ids_host(V, P, W, H)[1:], _want(_key(W, H), "tile", 4), "unsharded")


# ------------------------------------------------------------- 9. alternation

def test_ids_sequence_on_one_handle(built):
    """render, ids, render, depth, ids, features, contrib, ids, render, render on one handle
    with depth cuts and two frames in flight, into reused tensors: every colour frame equals the
    oracle's, every other output its reference; ids, feature and contrib frames are whole-list
    frames, the colour and depth frames around them are depth-cut frames again."""
    import torch
    from contrib_ref import contrib_totals
    W, H, K = 1037, 531, 4
    key = _key(W, H)
    sc, V, P, fr, cref, info, N = _ref(key, "tile")
    proj = _projection(key)[3]
    dref, _ = depth_from_projection(sc, V, P, W, H, "tile", 0, proj)
    f = np.random.default_rng(5).standard_normal((N, K)).astype(np.float32)
    fref, _ = features_from_projection(sc, V, P, W, H, "tile", 0, proj, f)
    r = _hip(sc, depth_split=True, frames_in_flight=2)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    depth = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    fd = torch.tensor(f, device="cuda:0")
    got = []
    slots = iter((4, 1, 3))
    for step in ("render", "ids", "render", "depth", "ids", "features", "contrib", "ids", "render", "render"):
        extra = None
        if step == "render":
            r.render(V, P, W, H, out=out)
        elif step == "depth":
            r.render_depth(V, P, W, H, out=out, depth=depth)
            extra = depth.clone()
        elif step == "features":
            extra = r.render_features(V, P, W, H, fd, out=out)[1]
        elif step == "contrib":
            extra = r.render_contrib(V, P, W, H, out=out)[1:]
        else:
            extra = r.render_ids(V, P, W, H, slots=next(slots), out=out)[1:]
        got.append((step, out.clone(), extra, r.last_stats()["cut_frame"]))
    torch.cuda.synchronize()
    for j, (step, c, extra, cutf) in enumerate(got):
        assert _bits(c.cpu().numpy(), cref) == 0, (j, step)
        assert cutf == (1 if step in ("render", "depth") else 0), (j, step, cutf)
        if step == "depth":
            assert _bits(extra.cpu().numpy(), dref) == 0, j
        elif step == "features":
            assert _bits(extra.cpu().numpy(), fref) == 0, j
        elif step == "contrib":
            for name, g, w in zip(("sum", "count", "max"), _np(*extra), contrib_totals(fr, N)):
                assert (g == w).all(), (j, name)
        elif step == "ids":
            _same(_u32(*extra), _want(key, "tile", int(extra[0].shape[2])), (j, step))


# ------------------------------------------------------------- 10. host path

@pytest.mark.parametrize("W,H", SHAPES)
def test_ids_host_path(built, W, H):
    """render_ids_host equals the device path and the reference, with and without q and count."""
    key = _key(W, H)
    sc, V, P, fr, cref, info, N = _ref(key, "tile")
    r = _hip(sc)
    for slots in (4, 3):
        want = _want(key, "tile", slots)
        ch, hi, hq, hc = r.render_ids_host(V, P, W, H, slots=slots)
        cd, di, dq, dc = r.render_ids(V, P, W, H, slots=slots)
        assert hi.dtype == np.uint32 and hq.dtype == np.uint32 and hc.dtype == np.uint32
        assert _bits(ch, cd.cpu().numpy()) == 0 and _bits(ch, cref) == 0, slots
        _same((hi, hq, hc), want, slots)
        _same(_u32(di, dq, dc), want, slots)
    ch, hi, hq, hc = r.render_ids_host(V, P, W, H, slots=2, want_q=False, want_count=False)
    assert hq is None and hc is None and _bits(ch, cref) == 0
    _same((hi, None, None), _want(key, "tile", 2), "ids only")
