"""Reference for the repair over window replay (bcp_pq_repair_stripes_win_async),
written from the contract in include/bcp.h on top of pq_window.replay and
gf256; nothing here comes from the library under test.

Thresholds: the distinct T_k = (lw_k + 1) * W over the positions k with bit k in
`allow`, len_k > 0 and T_k < out_len, E_1 < ... < E_m.  Phase i is the stream
offsets [E_i, E_{i+1}) (E_0 = 0, E_{m+1} = out_len).  The phases run in order,
each on the bytes the earlier ones left: the syndromes of a phase's offsets are
recomputed from the current members, and per bad offset j

    Ps != 0, Qs == 0:  P[j] ^= Ps   when allow has BAD_P, else left
    Ps == 0, Qs != 0:  Q[j] ^= Qs   when allow has BAD_Q, else left
    both != 0:         D_k[j] ^= Ps for k = (LOG[Qs] - LOG[Ps]) mod 255 when k < nsrc, allow has bit k,
                       source k is not replayed at j (j < T_k) and j < len_k; else left

Inside a phase the offsets are independent of one another: a byte of D_k
written at its home offset is read again only at its echoes j + W, j + 2W, ...,
which lie at or past T_k and so in a later phase."""
import numpy as np

import gf256 as G
from pq_window import rows

BAD_P, BAD_Q, NOWHERE = 1 << 56, 1 << 57, 1 << 58
ALL = 2 ** 64 - 1
NONE_BAD = 2 ** 64 - 1


def _len(c):
    return 0 if c is None else len(c)


def lim_of(n, w):
    """T_k: where the stream of a source of length n starts to replay (None: never)."""
    return ((n - 1) // w + 1) * w if w and n else None


def thresholds(lens, w, out_len, allow):
    """E_1 < ... < E_m by the definition."""
    out = set()
    for k, n in enumerate(lens):
        t = lim_of(n, w)
        if t is not None and (allow >> k) & 1 and t < out_len:
            out.add(t)
    return sorted(out)


def phase_of(bounds, off):
    return sum(1 for e in bounds if e <= off)


def syndromes(chunks, p, q, w, out_len):
    r = rows(chunks, w, out_len)
    return p[:out_len] ^ G.p_of(r, out_len), q[:out_len] ^ G.q_sum(r, out_len)


def check_record(chunks, p, q, w, out_len):
    """bcp_pq_check_result over the replayed streams, by its definition."""
    ps, qs = syndromes(chunks, p, q, w, out_len)
    bad = np.flatnonzero((ps != 0) | (qs != 0))
    members = (BAD_P if np.any((ps != 0) & (qs == 0)) else 0) | (BAD_Q if np.any((ps == 0) & (qs != 0)) else 0)
    both = (ps != 0) & (qs != 0)
    for k in np.unique((G.LOG[qs[both]] - G.LOG[ps[both]]) % 255):
        members |= (1 << int(k)) if k < len(chunks) else NOWHERE
    return (int(bad[0]) if bad.size else NONE_BAD, int(np.count_nonzero(ps)), int(np.count_nonzero(qs)), members)


def repair(chunks, p, q, w, out_len, allow):
    """((first_bad, p_bad, q_bad, members, fixed, left), chunks, p, q, phases) after the repair.
    chunks: arrays, None for the source (0, 0)."""
    chunks = [None if c is None else np.array(c, dtype=np.uint8, copy=True) for c in chunks]
    p, q = np.array(p, dtype=np.uint8, copy=True), np.array(q, dtype=np.uint8, copy=True)
    lens = [_len(c) for c in chunks]
    edges = [0] + thresholds(lens, w, out_len, allow) + [out_len]
    first, p_bad, q_bad, members, fixed, left = NONE_BAD, 0, 0, 0, 0, 0
    for lo, hi in zip(edges[:-1], edges[1:]):
        ps, qs = syndromes(chunks, p, q, w, out_len)    # from the bytes as the earlier phases left them
        at = np.arange(lo, hi)
        ps, qs = ps[lo:hi], qs[lo:hi]
        bad = at[(ps != 0) | (qs != 0)]
        if bad.size:
            first = min(first, int(bad[0]))
        p_bad += int(np.count_nonzero(ps))
        q_bad += int(np.count_nonzero(qs))
        for body, own, other, bit in ((p, ps, qs, BAD_P), (q, qs, ps, BAD_Q)):
            sel = (own != 0) & (other == 0)
            if sel.any():
                members |= bit
                if allow & bit:
                    body[at[sel]] ^= own[sel]
                    fixed += int(sel.sum())
                else:
                    left += int(sel.sum())
        for i in np.flatnonzero((ps != 0) & (qs != 0)):
            j, k = int(at[i]), int((G.LOG[qs[i]] - G.LOG[ps[i]]) % 255)
            members |= (1 << k) if k < len(chunks) else NOWHERE
            t = lim_of(lens[k], w) if k < len(chunks) else None
            if k < len(chunks) and (allow >> k) & 1 and (t is None or j < t) and j < lens[k]:
                chunks[k][j] ^= ps[i]
                fixed += 1
            else:
                left += 1
    return (first, p_bad, q_bad, members, fixed, left), chunks, p, q, len(edges) - 1
