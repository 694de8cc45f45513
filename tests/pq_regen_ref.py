"""Reference for the parity restore, from the definition in include/bcp.h: a
complete stripe of which one parity body is kept and the other is written.  With

    P' = XOR_k D_k        Q' = XOR_k g^k * D_k

over the sources (their replayed streams R_k under a window), each zero-padded
to out_len,

    keep P:  Q' is written, byte j is bad when Ps[j] = P[j] ^ P'[j] != 0
    keep Q:  P' is written, byte j is bad when Qs[j] = Q[j] ^ Q'[j] != 0

Field arithmetic is tests/gf256.py's, the replay tests/pq_window.py's; nothing
here comes from the library under test."""
import numpy as np

import gf256 as G
import pq_window as PW

KEEP_P, KEEP_Q = 1, 2
CLEAN = (2 ** 64 - 1, 0)  # (first_bad, bad_bytes) of a stripe whose kept parity agrees with the sources


def residuals(chunks, p, q, out_len, window=0):
    """(Ps, Qs) over [0, out_len); p or q may be None (that residual is then None)."""
    rows = PW.rows(chunks, window, out_len)
    ps = None if p is None else np.asarray(p, np.uint8)[:out_len] ^ G.p_of(rows, out_len)
    qs = None if q is None else np.asarray(q, np.uint8)[:out_len] ^ G.q_sum(rows, out_len)
    return ps, qs


def regen(chunks, kept, keep, out_len, window=0):
    """(the body written, (first_bad, bad_bytes)).  kept: the kept body, at least out_len bytes."""
    assert keep in (KEEP_P, KEEP_Q)
    rows = PW.rows(chunks, window, out_len)
    p, q = G.p_of(rows, out_len), G.q_sum(rows, out_len)
    mine, other = (p, q) if keep == KEEP_P else (q, p)
    bad = np.flatnonzero(np.asarray(kept, np.uint8)[:out_len] ^ mine)
    return other, ((int(bad[0]), int(bad.size)) if bad.size else CLEAN)
