"""Reference for the verified rebuild (bcp_pq_rebuild_check_stripes_async and
its _win namesake), from the definition in include/bcp.h: exactly one data
member x is lost, P and Q survive, and with

    Ps = P ^ XOR_{k != x} D_k        Qs = Q ^ XOR_{k != x} g^k * D_k

over the survivors (their replayed streams R_k under a window),

    D_x[j] = Ps[j]                         0 <= j < len_x
    r[j]   = Qs[j] ^ g^x * Ps[j]           byte j < len_x is bad when r[j] != 0.

Field arithmetic is tests/gf256.py's, the replay tests/pq_window.py's; nothing
here comes from the library under test."""
import numpy as np

import gf256 as G
import pq_window as PW

CLEAN = (2 ** 64 - 1, 0)  # (first_bad, bad_bytes) of a stripe whose Q agrees with the rebuilt member


def syndromes(survivors, p, q, out_len, window=0):
    """(Ps, Qs) over [0, out_len).  survivors: the stripe's chunks in position order with None (or an
    empty array) at the lost position; p, q: the bodies, at least out_len bytes."""
    rows = PW.rows(survivors, window, out_len)
    ps = np.asarray(p, np.uint8)[:out_len] ^ G.p_of(rows, out_len)
    qs = np.asarray(q, np.uint8)[:out_len] ^ G.q_sum(rows, out_len)
    return ps, qs


def residual(survivors, p, q, x, out_len, window=0):
    """r over [0, out_len): zero wherever the survivors, P and Q are consistent."""
    ps, qs = syndromes(survivors, p, q, out_len, window)
    return qs ^ G.mul(ps, np.uint8(G.gpow(x)))


def rebuild(survivors, p, q, x, out_len, len_x, window=0):
    """(D_x cut to len_x, (first_bad, bad_bytes)): what the call writes and what its record holds."""
    assert len_x <= out_len
    ps, qs = syndromes(survivors, p, q, out_len, window)
    r = (qs ^ G.mul(ps, np.uint8(G.gpow(x))))[:len_x]
    bad = np.flatnonzero(r)
    return ps[:len_x].copy(), ((int(bad[0]), int(bad.size)) if bad.size else CLEAN)
