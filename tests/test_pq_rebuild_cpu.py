"""The verified rebuild's host-side contract, without a device: the numpy
reference of the residual (tests/pq_rebuild_ref.py) against the algebra it
rests on, the exported symbols and argument validation."""
import ctypes
import errno

import numpy as np

import gf256 as G
import pq_rebuild_ref as R

WIDTH = 56  # BCP_MAX_SOURCES


def test_single_member_fault_always_shows_in_the_residual():
    """For every lost x, every other member z < 56 and every non-zero error byte e the residual's
    coefficient is non-zero: a survivor gives (g^z ^ g^x) * e, P gives g^x * e, Q gives e."""
    e = np.arange(1, 256, dtype=np.uint8)
    for x in range(WIDTH):
        gx = G.gpow(x)
        assert np.all(G.mul(e, np.uint8(gx)) != 0)          # P alone
        for z in range(WIDTH):
            if z != x:
                assert G.gpow(z) ^ gx != 0
                assert np.all(G.mul(e, np.uint8(G.gpow(z) ^ gx)) != 0), (x, z)


def test_reference_residual_on_stripes():
    """The helper itself: clean stripes give r = 0 and D_x, and a one-byte fault in any single member -- every
    survivor position, P, Q -- gives r != 0 exactly there, at width 56 for every x and every error byte."""
    rng = np.random.default_rng(3)
    n = 255                                  # one offset per error byte
    chunks = [rng.integers(0, 256, size=n, dtype=np.uint8) for _ in range(WIDTH)]
    p, q = G.p_of(chunks, n), G.q_sum(chunks, n)
    err = np.arange(1, 256, dtype=np.uint8)  # byte j gets error j + 1
    for x in range(WIDTH):
        surv = [None if k == x else c for k, c in enumerate(chunks)]
        dx, rec = R.rebuild(surv, p, q, x, n, n)
        assert rec == R.CLEAN and np.array_equal(dx, chunks[x])
        assert not R.residual(surv, p, q, x, n).any()
        for z in list(range(WIDTH)) + ["p", "q"]:
            if z == x:
                continue
            s2, p2, q2 = list(surv), p, q
            if z == "p":
                p2 = p ^ err
            elif z == "q":
                q2 = q ^ err
            else:
                s2[z] = chunks[z] ^ err
            r = R.residual(s2, p2, q2, x, n)
            assert np.all(r != 0), (x, z)
            want = err if z == "q" else G.mul(err, np.uint8(G.gpow(x) if z == "p" else G.gpow(z) ^ G.gpow(x)))
            assert np.array_equal(r, want), (x, z)
    # a fault counts only below len_x, and the bytes written are Ps whatever the record says
    x, len_x = 3, 100
    surv = [None if k == x else c for k, c in enumerate(chunks)]
    surv[7] = chunks[7].copy()
    surv[7][[5, 99, 100, 200]] ^= 0x5A
    dx, rec = R.rebuild(surv, p, q, x, n, len_x)
    assert rec == (5, 2)
    want = chunks[x][:len_x].copy()
    want[[5, 99]] ^= 0x5A
    assert np.array_equal(dx, want)


def test_reference_residual_over_window_replay():
    """Under a window the algebra holds over the replayed streams: clean is clean, R_x cut to len_x is D_x,
    and a wrong byte of a survivor's last window counts at every place below len_x it is replayed to."""
    import pq_window as PW
    w, lens, x = 32768, [65541, 32771, 100, 0, 32768, 98304], 5
    chunks = PW.chunks_of(lens, 9)
    out_len = max(lens)
    p, q = PW.p_win(chunks, w, out_len), PW.q_win(chunks, w, out_len)
    surv = [None if k == x else c for k, c in enumerate(chunks)]
    dx, rec = R.rebuild(surv, p, q, x, out_len, lens[x], w)
    assert rec == R.CLEAN and np.array_equal(dx, chunks[x])
    surv[1] = chunks[1].copy()
    surv[1][32769] ^= 1                       # in source 1's last window: replayed to 65537, not to 98305 (= len_x)
    _, rec = R.rebuild(surv, p, q, x, out_len, lens[x], w)
    assert rec == (32769, 2) and PW.replayed_places(lens[1], w, lens[x], 32769) == [32769, 65537]


def test_new_symbols_are_exported(bcp):
    L = bcp.lib()
    for name in ("bcp_pq_rebuild_check_stripes_async", "bcp_pq_rebuild_check_stripes_win_async"):
        assert getattr(L, name) is not None
    assert callable(bcp.Queue.pq_rebuild_check)
    assert bcp.lib().bcp_abi_version() == 4
    assert ctypes.sizeof(bcp.CheckResult) == 16 and ctypes.sizeof(bcp.PqLost) == 56   # the records and arguments reused


def test_null_arguments(bcp):
    L = bcp.lib()
    st = (bcp.Stripe * 1)(bcp.Stripe(0, 0, 0, 0, 0))
    so = (bcp.Source * 1)()
    lo = (bcp.PqLost * 1)()
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for fn in (L.bcp_pq_rebuild_check_stripes_async, L.bcp_pq_rebuild_check_stripes_win_async):
        assert fn(None, st, 1, so, 0, lo, fake) == -errno.EINVAL   # a null queue
        assert fn(fake, None, 1, so, 0, lo, fake) == -errno.EINVAL
        assert fn(fake, st, 1, so, 0, None, fake) == -errno.EINVAL  # no lost records
        assert fn(fake, st, 1, so, 0, lo, None) == -errno.EINVAL   # no result records
        assert fn(fake, st, 1, None, 1, lo, fake) == -errno.EINVAL
