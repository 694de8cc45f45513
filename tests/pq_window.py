"""Reference for P + Q over window replay (the bcp_pq_*_win_async entry
points): the replayed stream R_k of a source, written from its definition,

    R_k[j] = D_k'[j]                      for j <  (lw_k + 1) * W
    R_k[j] = D_k'[lw_k * W + j mod W]     for j >= (lw_k + 1) * W
             lw_k = (len_k - 1) // W, D_k' = D_k zero-padded, len_k = 0: zeros

and P, Q as tests/gf256.py's over the R_k.  test_pq_window_cpu.py pins replay()
to the oracle's parity body; nothing here comes from the library under test."""
import numpy as np

import gf256 as G

KiB, MiB = 1024, 1024 * 1024
W = 32 * KiB
# a full window replayed (32768, 98304, 163840), a length below W (100, 1, 17, 9), sources ending inside a tile of
# their last window (65541, 32771, 32769, 114695, 40000, 70000, 32784, 65537), length 0, 9 sources, odd out_len
LISTS = ([65541, 32771, 100, 0, 32768, 98304],
         [32769, 1],
         [163840, 163840, 17],
         [114695, 32767, 65536, 40000, 0, 70000, 9, 32784, 65537])


def replay(c, w, out_len):
    """R_k[0 .. out_len) of chunk c under window w (w = 0: plain zero padding)."""
    out = np.zeros(out_len, dtype=np.uint8)
    n = 0 if c is None else len(c)
    if n == 0:
        return out
    c = np.asarray(c, dtype=np.uint8)
    if w == 0:
        out[:min(n, out_len)] = c[:out_len]
        return out
    lw = (n - 1) // w
    padded = np.zeros((lw + 1) * w, dtype=np.uint8)
    padded[:n] = c
    j = np.arange(out_len, dtype=np.int64)
    src = np.where(j < (lw + 1) * w, j, lw * w + j % w)
    return padded[src]


def replayed_places(n, w, out_len, j):
    """Every offset below out_len that byte j of a source of length n appears at."""
    assert 0 <= j < n
    places = [j] if j < out_len else []
    if w:
        lw = (n - 1) // w
        if j >= lw * w:
            places += list(range(j + w, out_len, w))
    return places


def chunks_of(lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 256, size=L, dtype=np.uint8) for L in lens]


def rows(chunks, w, out_len):
    return [replay(c, w, out_len) for c in chunks]


def p_win(chunks, w, out_len):
    return G.p_of(rows(chunks, w, out_len), out_len)


def q_win(chunks, w, out_len):
    return G.q_sum(rows(chunks, w, out_len), out_len)
