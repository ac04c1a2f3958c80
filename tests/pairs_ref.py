"""Reference for the bin lists (plain helper, shared by the GPU test modules)."""
import numpy as np


def rect_bin_pairs(rec, dk, nt, W):
    """(bin, dkey, splat) for every 32x32 bin of every visible splat's rect
    (the superset the bin lists are drawn from), and the set of (bin, splat)
    pairs whose splat surely covers a pixel centre of the bin (float64,
    threshold shrunk by 1e-4: must be present)."""
    bx = (W + 31) // 32
    qmax = 9.21034037197618 * (1.0 - 1e-4)
    pairs, must = [], set()
    for i in np.nonzero(nt)[0]:
        lo, hi = int(rec["rect_lo"][i]), int(rec["rect_hi"][i])
        x0, y0, x1, y1 = lo & 0xFFFF, lo >> 16, hi & 0xFFFF, hi >> 16
        r = rec[i]
        for by in range(y0 >> 5, (y1 >> 5) + 1):
            for b in range(x0 >> 5, (x1 >> 5) + 1):
                key = by * bx + b
                pairs.append((key, int(dk[i]), int(i)))
                px = np.arange(max(b * 32, x0), min(b * 32 + 31, x1) + 1) + 0.5
                py = np.arange(max(by * 32, y0), min(by * 32 + 31, y1) + 1) + 0.5
                dx = px[None, :] - float(r["cx"])
                dy = float(r["cy"]) - py[:, None]
                u = dy * float(r["ay"]) + dx * float(r["ax"])
                v = dy * float(r["by"]) + dx * float(r["bx"])
                if np.any((u * u + v * v <= qmax) & (np.maximum(np.abs(u), np.abs(v)) <= 3.0 * (1 - 1e-5))):
                    must.add((key, int(i)))
    return pairs, must


def check_sorted_pairs(keys, vals, rec, dk, nt, W):
    """The bin lists (keys = bin ids, vals = splats, as gs_sorted_pairs_host
    returns them) against the rects: no duplicates, only bins of the rect,
    every surely covered bin, and the order of a stable sort by (bin, depth
    key) of the depth-ordered pairs.  Returns the number of pairs checked."""
    pairs, must = rect_bin_pairs(rec, dk, nt, W)
    got = set(zip(keys.tolist(), vals.tolist()))
    assert len(got) == len(keys)                                  # no duplicates
    assert got <= {(k, i) for k, _, i in pairs}                   # only bins of the rect
    assert must <= got                                            # every surely covered bin
    ek = np.array([(k << 15) | d for k, d, i in pairs if (k, i) in got], np.uint64)
    ev = np.array([i for k, d, i in pairs if (k, i) in got], np.uint32)
    order = np.argsort(ek, kind="stable")  # (bin, dkey), ties by splat index
    np.testing.assert_array_equal(keys.astype(np.uint64), ek[order] >> np.uint64(15))  # bin id
    np.testing.assert_array_equal(vals, ev[order])
    return len(keys), len(must)
