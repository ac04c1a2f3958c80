"""CPU reference of gs_render_ids, from the fragment set alone.

contrib_ref.contrib_fragments gives the frame's (splat, pixel, q) fragments with
q > 0 from the oracle; a pixel's candidates are its fragments, ordered by q
descending, then splat index ascending.  Nothing about the order in which the
composite met them enters."""
import numpy as np

ID_NONE = np.uint32(0xFFFFFFFF)


def ids_ref(frags, W, H, K):
    """(ids (H, W, K) uint32, q (H, W, K) uint32, count (H, W) uint32): per pixel its first K
    fragments by (-q, id), ID_NONE / 0 in the empty slots, and its number of fragments."""
    sid, pix, q = (np.asarray(a) for a in frags[:3])
    n = W * H
    ids = np.full((n, K), ID_NONE, np.uint32)
    qs = np.zeros((n, K), np.uint32)
    count = np.bincount(pix, minlength=n).astype(np.uint32)
    if sid.size:
        order = np.lexsort((sid, -q.astype(np.int64), pix))  # (pixel, -q, id)
        sp, ss, sq = pix[order], sid[order], q[order]
        start = np.cumsum(count.astype(np.int64)) - count  # first entry of each pixel's run
        rank = np.arange(sp.size, dtype=np.int64) - start[sp]
        keep = rank < K
        ids[sp[keep], rank[keep]] = ss[keep].astype(np.uint32)
        qs[sp[keep], rank[keep]] = sq[keep]
    return ids.reshape(H, W, K), qs.reshape(H, W, K), count.reshape(H, W)


def ids_loop(frags, W, H, K):
    """The same by a plain loop over the pixels, for checking ids_ref."""
    sid, pix, q = (np.asarray(a) for a in frags[:3])
    per = [[] for _ in range(W * H)]
    for s, p, w in zip(sid.tolist(), pix.tolist(), q.tolist()):
        per[p].append((-w, s))
    ids = np.full((W * H, K), ID_NONE, np.uint32)
    qs = np.zeros((W * H, K), np.uint32)
    count = np.zeros(W * H, np.uint32)
    for p, lst in enumerate(per):
        lst.sort()
        count[p] = len(lst)
        for k, (nw, s) in enumerate(lst[:K]):
            ids[p, k] = s
            qs[p, k] = -nw
    return ids.reshape(H, W, K), qs.reshape(H, W, K), count.reshape(H, W)


def tie_counts(frags, W, H, K=4):
    """(equal-q neighbours among a pixel's first K + 1 candidates, summed over the pixels; pixels
    whose K-th and (K + 1)-th candidates have equal q): how much a frame's fragments test the tie
    rule, and the tie across the last slot's boundary."""
    i, q, c = ids_ref(frags, W, H, K + 1)
    q = q.reshape(-1, K + 1)
    eq = (q[:, :-1] == q[:, 1:]) & (q[:, 1:] > 0)
    return int(eq.sum()), int(eq[:, K - 1].sum())
