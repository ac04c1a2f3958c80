"""CPU reference of gs_render_contrib's per-splat totals.

w(i, p) is the factor that multiplies splat i's colour at pixel p in the frame's
composite.  The oracle composites whatever float a record carries in `r`, `g`
and `b` with C = fmaf(c, w, C) (ora_composite_records), so an indicator channel
that is 1.0 for a set of splats no two of which can share a pixel, and 0.0
elsewhere, yields w bit for bit: fmaf(1, w, 0) = w and fmaf(0, w', C) = C for
finite w'.  Two splats may share a set only if the 16-px tile ranges of their
record rects, widened by 2 px and clamped to the frame (the region in which the
oracle can composite them, gs_oracle.c ORA_RECT), are disjoint.  Sets are picked
greedily in index order and composited three at a time; each tile's pixels
belong to the set's one owner there.  q and the mask are applied in numpy.

Asserted on every call: each composite's alpha is the colour frame's bit for
bit (same fragments, weights and breaks), and an indicator image is 0 outside
its set's tiles.  Finite scenes only: a NaN weight would leak into the other
sets' images through fmaf(0, NaN, C).

contrib_fragments returns the frame's fragments with q > 0 once (splat, pixel,
q), from which contrib_totals builds sum / count / max for any mask."""
import numpy as np

TILE = 16
Q_ONE = np.float32(16777216.0)


def _bits(a, b):
    return int(np.count_nonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)))


def quantise(w):
    """q(w) = (uint32)(fminf(fmaxf(w, 0), 1) * 2^24), truncation, float32 throughout."""
    w = np.asarray(w, np.float32)
    c = np.fmin(np.fmax(w, np.float32(0.0)), np.float32(1.0)).astype(np.float32)
    return (c * Q_ONE).astype(np.float32).astype(np.uint32)


def tile_ranges(rec, dkey, W, H):
    """(listed, tx0, ty0, tx1, ty1): which records the oracle puts into lists, and the 16-px
    tile ranges (inclusive) in which it can composite them."""
    lo, hi = rec["rect_lo"].astype(np.int64), rec["rect_hi"].astype(np.int64)
    listed = ~((np.asarray(dkey) == 0) & (rec["rect_hi"] == 0) & (rec["opacity"] == 0))
    x0 = np.maximum((lo & 0xFFFF) - 2, 0) // TILE
    y0 = np.maximum((lo >> 16) - 2, 0) // TILE
    x1 = np.minimum((hi & 0xFFFF) + 2, W - 1) // TILE
    y1 = np.minimum((hi >> 16) + 2, H - 1) // TILE
    return listed, x0, y0, x1, y1


def colour_sets(listed, x0, y0, x1, y1, TW, TH):
    """Greedy colouring in index order: set[i] (-1 for unlisted records), the number of sets,
    and per tile the number of records that can reach it (its list length in the oracle)."""
    n = listed.shape[0]
    cap = 64
    occ = np.zeros((TH, TW, cap), bool)
    sets = np.full(n, -1, np.int32)
    nsets = 0
    for i in np.nonzero(listed)[0]:
        a, b, c, d = y0[i], y1[i] + 1, x0[i], x1[i] + 1
        if a >= b or c >= d:  # (a rect wholly outside the frame reaches no tile)
            continue
        used = occ[a:b, c:d, :nsets].any(axis=(0, 1)) if nsets else np.zeros(0, bool)
        free = np.nonzero(~used)[0]
        s = int(free[0]) if free.size else nsets
        if s == nsets:
            nsets += 1
            if nsets > cap:
                occ = np.concatenate([occ, np.zeros_like(occ)], axis=2)
                cap *= 2
        occ[a:b, c:d, s] = True
        sets[i] = s
    return sets, nsets, occ[:, :, :max(nsets, 1)].sum(axis=2)


def contrib_fragments(scene, V, P, W, H, mode, sh_degree, proj):
    """(ids int64, pix int64, q uint32, colour (H, W, 4), info) of the frame: one entry per
    composited fragment with q > 0; info: sets, composites, longest tile list."""
    from oracle import oracle_py as O
    rec, dkey, _, _ = proj
    n = rec.shape[0]
    colour, _ = O.render(scene, V, P, W, H, sh_degree=sh_degree, mode=mode)
    again = O.composite_records(rec, dkey, W, H, mode=mode)
    assert _bits(again, colour) == 0  # the record composite is the oracle's frame
    TW, TH = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    listed, x0, y0, x1, y1 = tile_ranges(rec, dkey, W, H)
    sets, nsets, per_tile = colour_sets(listed, x0, y0, x1, y1, TW, TH)
    # per set, the owner of each tile
    owner = np.full((max(nsets, 1), TH, TW), -1, np.int64)
    for i in np.nonzero(sets >= 0)[0]:
        o = owner[sets[i], y0[i]:y1[i] + 1, x0[i]:x1[i] + 1]
        assert (o == -1).all()
        o[...] = i
    ids, pix, qs = [], [], []
    zero = np.zeros(n, np.float32)
    ncomp = 0
    for g in range(0, nsets, 3):
        frec = rec.copy()
        for j, ch in enumerate("rgb"):
            frec[ch] = np.where(sets == g + j, np.float32(1.0), np.float32(0.0)).astype(np.float32) if g + j < nsets else zero
        img = O.composite_records(frec, dkey, W, H, mode=mode)
        ncomp += 1
        assert _bits(img[..., 3], colour[..., 3]) == 0  # alpha untouched: same fragments, weights and breaks
        for j in range(min(3, nsets - g)):
            own = np.repeat(np.repeat(owner[g + j], TILE, axis=0), TILE, axis=1)[:H, :W]
            w = img[..., j]
            assert (w[own < 0].view(np.uint32) == 0).all()  # 0 outside the set's tiles
            assert np.isfinite(w).all()
            q = quantise(w)
            hit = np.nonzero((q > 0) & (own >= 0))
            ids.append(own[hit])
            pix.append(hit[0].astype(np.int64) * W + hit[1])
            qs.append(q[hit])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    out = (cat(ids, np.int64), cat(pix, np.int64), cat(qs, np.uint32))
    for a in out:
        a.setflags(write=False)
    colour.setflags(write=False)
    info = dict(sets=nsets, composites=ncomp, longest_tile_list=int(per_tile.max()) if per_tile.size else 0)
    return out[0], out[1], out[2], colour, info


def contrib_totals(frags, n, mask=None):
    """(sum uint64, count uint32, max uint32), n entries each, over the pixels with mask != 0."""
    ids, pix, q = frags[0], frags[1], frags[2]
    if mask is not None:
        keep = np.asarray(mask).reshape(-1)[pix] != 0
        ids, q = ids[keep], q[keep]
    tot = np.bincount(ids, weights=q.astype(np.float64), minlength=n)
    assert tot.max(initial=0.0) < 2.0 ** 53  # (exact in float64)
    s = tot.astype(np.uint64)
    c = np.bincount(ids, minlength=n).astype(np.uint32)
    m = np.zeros(n, np.uint32)
    if ids.size:
        order = np.argsort(ids, kind="stable")
        si, sq = ids[order], q[order]
        starts = np.nonzero(np.r_[True, si[1:] != si[:-1]])[0]
        m[si[starts]] = np.maximum.reduceat(sq, starts)
    return s, c, m


def contrib_ref(scene, V, P, W, H, mode, sh_degree=0, mask=None, with_colour=False):
    """The frame's (sum, count, max); with_colour: also the oracle's colour frame."""
    from depth_ref import project_zf
    proj = project_zf(scene, V, P, W, H, sh_degree)
    fr = contrib_fragments(scene, V, P, W, H, mode, sh_degree, proj)
    tot = contrib_totals(fr, proj[0].shape[0], mask)
    return (*tot, fr[3]) if with_colour else tot


def single_splat_totals(rec, dkey, W, H, mode, splats, mask=None):
    """The slow way, for checking contrib_ref: one indicator composite per splat (three at a
    time); {splat: (sum, count, max)}."""
    from oracle import oracle_py as O
    out = {}
    splats = list(splats)
    for g in range(0, len(splats), 3):
        frec = rec.copy()
        grp = splats[g:g + 3]
        for j, ch in enumerate("rgb"):
            ind = np.zeros(rec.shape[0], np.float32)
            if j < len(grp):
                ind[grp[j]] = 1.0
            frec[ch] = ind
        img = O.composite_records(frec, dkey, W, H, mode=mode)
        for j, i in enumerate(grp):
            q = quantise(img[..., j])
            if mask is not None:
                q = np.where(np.asarray(mask) != 0, q, np.uint32(0))
            out[int(i)] = (int(q.astype(np.uint64).sum()), int((q > 0).sum()), int(q.max(initial=0)))
    return out
