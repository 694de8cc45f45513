"""Q parity over window replay without a device: the replayed stream R_k that
the GPU tests use as their reference (tests/pq_window.py) against the oracle's
parity body, the algebra over R_k, the new symbols, argument validation and
the CLI's usage path."""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import gf256 as G
from pq_window import LISTS, W, chunks_of, p_win, q_win, replay, replayed_places

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN_SYMBOLS = ("bcp_pq_stripes_win_async", "bcp_pq_recover_stripes_win_async", "bcp_pq_check_stripes_win_async")


def test_replay_by_hand():
    c = np.arange(1, 8, dtype=np.uint8)                       # len 7, W 4: lw = 1, window 1 is [5 6 7 0]
    assert replay(c, 4, 14).tolist() == [1, 2, 3, 4, 5, 6, 7, 0, 5, 6, 7, 0, 5, 6]
    assert replay(c[:4], 4, 10).tolist() == [1, 2, 3, 4, 1, 2, 3, 4, 1, 2]   # an exact multiple: a full window replayed
    assert replay(c[:2], 4, 9).tolist() == [1, 2, 0, 0, 1, 2, 0, 0, 1]       # below W: window 0 with its padding
    assert replay(c[:0], 4, 6).tolist() == [0] * 6 and replay(None, 4, 3).tolist() == [0] * 3
    assert replay(c, 4, 5).tolist() == [1, 2, 3, 4, 5]                       # cut below the source's length
    assert replay(c, 0, 9).tolist() == [1, 2, 3, 4, 5, 6, 7, 0, 0]           # no window: zero padding
    assert replayed_places(7, 4, 14, 5) == [5, 9, 13] and replayed_places(7, 4, 14, 2) == [2]
    assert replayed_places(2, 4, 9, 1) == [1, 5] and replayed_places(7, 0, 14, 5) == [5]


@pytest.mark.parametrize("lens", LISTS, ids=[f"n{len(x)}" for x in LISTS])
def test_xor_of_the_replayed_streams_is_the_oracles_body(oracle, lens):
    chunks = chunks_of(lens, seed=len(lens))
    out_len = max(lens)
    body = np.frombuffer(oracle.gen_parity_file(chunks, W), np.uint8)[8 * len(lens):]
    assert len(body) == out_len
    assert np.array_equal(p_win(chunks, W, out_len), body)
    # every place a byte is replayed to holds that byte
    for k, c in enumerate(chunks):
        if len(c):
            r = replay(c, W, out_len)
            j = len(c) - 1
            places = replayed_places(len(c), W, out_len, j)
            assert places[0] == j and all(r[p] == c[j] for p in places)


@pytest.mark.parametrize("lens", LISTS, ids=[f"n{len(x)}" for x in LISTS])
def test_two_loss_algebra_over_the_replayed_streams(lens):
    chunks = chunks_of(lens, seed=10 + len(lens))
    n, out_len = len(lens), max(lens)
    rows = [replay(c, W, out_len) for c in chunks]
    p, q = p_win(chunks, W, out_len), q_win(chunks, W, out_len)
    pairs = [(x, y) for x in range(n) for y in range(x + 1, n)]
    for x, y in pairs[:: max(1, len(pairs) // 8)]:
        surv = [None if k in (x, y) else r for k, r in enumerate(rows)]
        dx, dy = G.recover_two(surv, p, q, x, y, out_len)
        assert np.array_equal(dx[:lens[x]], chunks[x]) and np.array_equal(dy[:lens[y]], chunks[y]), (x, y)


def test_symbols_are_declared_and_exported(bcp):
    h = open(os.path.join(ROOT, "include", "bcp.h")).read()
    ht = open(os.path.join(ROOT, "include", "bcp_task.h")).read()
    L = bcp.lib()
    for name in WIN_SYMBOLS:
        assert re.search(r"\bint %s\(bcp_queue \*q," % name, h), name
        assert getattr(L, name).argtypes is not None
    assert re.search(r"\bint bcp_pipeline_set_q_windowed\(bcp_pipeline \*pl, int on\);", ht)
    assert L.bcp_pipeline_set_q_windowed.argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", bcp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(WIN_SYMBOLS) | {"bcp_pipeline_set_q_windowed"} <= exported


def test_null_arguments(bcp):
    L = bcp.lib()
    E = -errno.EINVAL
    st = (bcp.Stripe * 1)(bcp.Stripe(0, 0, 0, 0, 32768))
    so = (bcp.Source * 1)()
    qd = (ctypes.c_uint64 * 1)(0)
    lost = (bcp.PqLost * 1)()
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 12), ctypes.c_void_p)
    assert L.bcp_pq_stripes_win_async(None, st, 1, so, 0, qd) == E
    assert L.bcp_pq_stripes_win_async(fake, None, 1, so, 0, qd) == E
    assert L.bcp_pq_stripes_win_async(fake, st, 1, so, 0, None) == E
    assert L.bcp_pq_stripes_win_async(fake, st, 1, None, 1, qd) == E
    assert L.bcp_pq_recover_stripes_win_async(None, st, 1, so, 0, lost) == E
    assert L.bcp_pq_recover_stripes_win_async(fake, None, 1, so, 0, lost) == E
    assert L.bcp_pq_recover_stripes_win_async(fake, st, 1, so, 0, None) == E
    assert L.bcp_pq_recover_stripes_win_async(fake, st, 1, None, 1, lost) == E
    assert L.bcp_pq_check_stripes_win_async(None, st, 1, so, 0, qd, fake) == E
    assert L.bcp_pq_check_stripes_win_async(fake, None, 1, so, 0, qd, fake) == E
    assert L.bcp_pq_check_stripes_win_async(fake, st, 1, so, 0, None, fake) == E
    assert L.bcp_pq_check_stripes_win_async(fake, st, 1, so, 0, qd, None) == E
    assert L.bcp_pq_check_stripes_win_async(fake, st, 1, None, 1, qd, fake) == E
    assert L.bcp_pipeline_set_q_windowed(None, 1) == E


def test_set_q_windowed_takes_0_or_1(bcp):
    # the value is checked before the handle is used, so a stand-in will do where there is no device
    L = bcp.lib()
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    assert L.bcp_pipeline_set_q_windowed(fake, 2) == -errno.EINVAL
    assert L.bcp_pipeline_set_q_windowed(fake, -1) == -errno.EINVAL


def test_cli_usage_paths(bcp):
    for args in (["parity-gen", "--complete", "--q-windowed", "--protocol", "store", "4"],
                 ["parity-gen", "--complete", "--procs", "--q-windowed", "store", "4"],
                 ["parity-rebuild", "--q-windowed", "store", "4", "1"],                       # without --also
                 ["parity-rebuild", "--protocol", "--also", "2", "--q-windowed", "store", "4", "1"],
                 ["parity-verify", "--q-windowed", "store", "4"]):                            # without --q
        r = subprocess.run([bcp.BIN_PATH, *args], capture_output=True)
        assert r.returncode == 1 and r.stderr.startswith(b"usage:"), args
        assert b"--q-windowed" in r.stderr and r.stdout == b""
