"""The parity restore's host side, without a device: the numpy statement of the
two residuals (tests/pq_regen_ref.py) and the limit bcp.h documents, the
exported symbol and the constants the bindings assume, and the rule
bcp_restore_plan against a Python restatement."""
import errno
import os
import subprocess

import numpy as np

import gf256 as G
import pq_regen_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH = 56  # BCP_MAX_SOURCES


def test_single_member_fault_always_shows_in_the_kept_residual():
    """Every position k < 56 and every non-zero error byte e: a data member gives Ps = e and Qs = g^k * e,
    the kept parity gives e; none of them is zero."""
    e = np.arange(1, 256, dtype=np.uint8)
    for k in range(WIDTH):
        assert np.all(G.mul(e, np.uint8(G.gpow(k))) != 0), k
    rng = np.random.default_rng(5)
    n = 255                                   # one offset per error byte
    chunks = [rng.integers(0, 256, size=n, dtype=np.uint8) for _ in range(WIDTH)]
    p, q = G.p_of(chunks, n), G.q_sum(chunks, n)
    out, rec = R.regen(chunks, p, R.KEEP_P, n)
    assert rec == R.CLEAN and np.array_equal(out, q)
    out, rec = R.regen(chunks, q, R.KEEP_Q, n)
    assert rec == R.CLEAN and np.array_equal(out, p)
    for k in range(WIDTH):
        c2 = list(chunks)
        c2[k] = chunks[k] ^ e
        ps, qs = R.residuals(c2, p, q, n)
        assert np.array_equal(ps, e) and np.array_equal(qs, G.mul(e, np.uint8(G.gpow(k)))), k
        assert np.all(ps != 0) and np.all(qs != 0)
        for keep, kept in ((R.KEEP_P, p), (R.KEEP_Q, q)):
            assert R.regen(c2, kept, keep, n)[1] == (0, n)
    ps, qs = R.residuals(chunks, p ^ e, q ^ e, n)     # the kept parity itself
    assert np.array_equal(ps, e) and np.array_equal(qs, e)


def test_the_cancelling_pair_is_the_documented_limit():
    """Two members wrong at one offset can cancel: e in D_a and in D_b leaves Ps clean (Qs shows it), and
    e_a, e_b with g^a * e_a = g^b * e_b leave Qs clean (Ps shows it)."""
    rng = np.random.default_rng(6)
    n = 255
    chunks = [rng.integers(0, 256, size=n, dtype=np.uint8) for _ in range(9)]
    p, q = G.p_of(chunks, n), G.q_sum(chunks, n)
    e = np.arange(1, 256, dtype=np.uint8)
    for a, b in ((0, 1), (2, 7), (8, 3)):
        c2 = list(chunks)
        c2[a], c2[b] = chunks[a] ^ e, chunks[b] ^ e
        ps, qs = R.residuals(c2, p, q, n)
        assert not ps.any() and np.all(qs != 0)
        assert R.regen(c2, p, R.KEEP_P, n)[1] == R.CLEAN
        eb = G.mul(e, np.uint8(G.gpow(a - b)))        # g^b * eb = g^a * e
        c3 = list(chunks)
        c3[a], c3[b] = chunks[a] ^ e, chunks[b] ^ eb
        ps, qs = R.residuals(c3, p, q, n)
        assert not qs.any() and np.all(ps != 0)
        assert R.regen(c3, q, R.KEEP_Q, n)[1] == R.CLEAN


def test_reference_over_window_replay():
    """Under a window the residuals are over the replayed streams: a wrong byte of a source's last window
    counts at every place below out_len it is replayed to."""
    import pq_window as PW
    w, lens = 32768, [98304, 32771, 100, 0]
    chunks = PW.chunks_of(lens, 9)
    out_len = max(lens)
    p, q = PW.p_win(chunks, w, out_len), PW.q_win(chunks, w, out_len)
    for keep, kept, other in ((R.KEEP_P, p, q), (R.KEEP_Q, q, p)):
        out, rec = R.regen(chunks, kept, keep, out_len, w)
        assert rec == R.CLEAN and np.array_equal(out, other)
        c2 = list(chunks)
        c2[2] = chunks[2].copy()
        c2[2][99] ^= 1
        assert R.regen(c2, kept, keep, out_len, w)[1] == (99, 3)
    assert PW.replayed_places(100, w, out_len, 99) == [99, w + 99, 2 * w + 99]


def test_new_symbol_is_exported_and_declared(bcp):
    L = bcp.lib()
    assert L.bcp_restore_plan is not None and callable(bcp.restore_plan)
    assert L.bcp_abi_version() == 4
    t = open(os.path.join(ROOT, "include", "bcp_task.h")).read()
    assert "int bcp_restore_plan(" in t


def test_constants_have_the_c_values(bcp, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "bcp.h"\n#include "bcp_task.h"\n'
                   'int main(void) { printf("%u %u\\n", BCP_PQ_KEEP_P, BCP_PQ_KEEP_Q); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [bcp.PQ_KEEP_P, bcp.PQ_KEEP_Q]
    assert (bcp.PQ_KEEP_P, bcp.PQ_KEEP_Q) == (R.KEEP_P, R.KEEP_Q) == (1, 2)


# ---- the rule ---------------------------------------------------------------
def plan(loc, n, a, b, q_on, windowed_no_q):
    """bcp_restore_plan, restated from bcp_task.h's comment."""
    lost = {a, b} - {-1}
    p = loc >> 56
    has_p = p != 0xFF and p < n
    qt = G.q_target(loc, n)
    has_q = q_on and not windowed_no_q and qt >= 0
    p_lost = has_p and p in lost
    q_lost = has_q and qt in lost
    if p_lost and q_lost:
        keep = 0
    elif p_lost:
        keep = R.KEEP_Q if has_q else 0
    elif q_lost:
        keep = R.KEEP_P
    else:
        keep = 0
    return p_lost, q_lost, keep


def random_locations(rng, n):
    kind = int(rng.integers(0, 10))
    if kind == 0:                                      # NO_P
        return int(rng.integers(0, 1 << n)) | (0xFF << 56)
    p = int(rng.integers(0, n))
    if kind == 1:                                      # every other target is a holder: no Q target
        return (((1 << n) - 1) & ~(1 << p)) | (p << 56)
    mask = int(rng.integers(0, 1 << n)) & ~(1 << p)
    if kind == 2:
        mask = 0                                       # no holders
    return mask | (p << 56)


def test_restore_plan_against_the_restatement(bcp):
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(4000):
        n = int(rng.integers(2, 20))
        loc = random_locations(rng, n)
        a = int(rng.integers(0, n))
        b = -1 if rng.integers(0, 2) else int((a + 1 + rng.integers(0, n - 1)) % n)
        for q_on in (False, True):
            for wnq in (False, True):
                got = bcp.restore_plan(loc, n, a, b, q_on, wnq)
                assert got == plan(loc, n, a, b, q_on, wnq), (hex(loc), n, a, b, q_on, wnq)
                seen.add(got)
    # every outcome the rule has was met
    assert seen == {(False, False, 0), (True, False, 0), (True, False, R.KEEP_Q), (False, True, R.KEEP_P),
                    (True, True, 0)}


def test_restore_plan_by_hand(bcp):
    loc = 0b00110 | (0 << 56)                          # holders 1, 2; P on 0; Q on 3 (of 5)
    assert G.q_target(loc, 5) == 3
    assert bcp.restore_plan(loc, 5, 0) == (True, False, R.KEEP_Q)
    assert bcp.restore_plan(loc, 5, 3) == (False, True, R.KEEP_P)
    assert bcp.restore_plan(loc, 5, 0, 3) == (True, True, 0)
    assert bcp.restore_plan(loc, 5, 3, 0) == (True, True, 0)
    assert bcp.restore_plan(loc, 5, 1) == (False, False, 0)
    assert bcp.restore_plan(loc, 5, 4, 2) == (False, False, 0)
    assert bcp.restore_plan(loc, 5, 0, q_on=False) == (True, False, 0)
    assert bcp.restore_plan(loc, 5, 3, q_on=False) == (False, False, 0)
    assert bcp.restore_plan(loc, 5, 0, windowed_no_q=True) == (True, False, 0)
    assert bcp.restore_plan(loc, 5, 3, windowed_no_q=True) == (False, False, 0)
    full = 0b0110 | (0 << 56)                          # 3 targets: no Q target
    assert G.q_target(full, 3) == -1 and bcp.restore_plan(full, 3, 0) == (True, False, 0)
    assert bcp.restore_plan(0b011 | (0xFF << 56), 4, 2) == (False, False, 0)   # NO_P
    L = bcp.lib()
    for args in ((loc, 0, 0, -1), (loc, 57, 0, -1), (loc, 5, -1, -1), (loc, 5, 5, -1), (loc, 5, 0, 5), (loc, 5, 0, -2),
                 (loc, 5, 2, 2)):
        assert L.bcp_restore_plan(*args, 1, 0, None, None, None) == -errno.EINVAL, args
    assert L.bcp_restore_plan(loc, 5, 0, -1, 1, 0, None, None, None) == 0      # each pointer may be null
