"""Q parity without a device: the field arithmetic the kernels and the tests
rely on (tests/gf256.py), bcp_q_target, argument validation of the new entry
points, the ctypes structures against the C headers, and the CLI's usage
paths."""
import ctypes
import errno
import os
import subprocess

import numpy as np

import bcp_store as S
import gf256 as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slow_mul(a: int, b: int) -> int:
    """Carry-less multiply modulo 0x11d, bit by bit (no tables)."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11D
        b >>= 1
    return r


def test_field_tables_and_check_values():
    assert G.gpow(8) == 0x1D and G.gpow(55) == 0xA0
    assert G.gpow(0) == 1 and G.gpow(255) == 1 and G.gpow(-1) == G.div(1, 2)
    a = np.arange(256, dtype=np.uint8)
    for b in (0, 1, 2, 3, 0x1D, 0x80, 0xA0, 0xFF):
        assert np.array_equal(G.mul(a, np.uint8(b)), np.array([_slow_mul(int(x), b) for x in a], np.uint8)), b
    for x in range(1, 256):
        assert int(G.mul(np.uint8(x), np.uint8(G.div(1, x)))) == 1


def test_packed_mul2_equals_the_tables():
    # every byte value in every lane, beside every neighbour pattern that could carry into it
    vals = np.arange(256, dtype=np.uint32)
    for shift in (0, 8, 16, 24):
        for other in (0x00000000, 0xFFFFFFFF, 0x80808080, 0x7F7F7F7F):
            x = (vals << np.uint32(shift)) | (np.uint32(other) & ~np.uint32(0xFF << shift))
            got = G.mul2_packed(x).view(np.uint8)
            want = G.mul(x.astype(np.uint32).view(np.uint8), np.uint8(2))
            assert np.array_equal(got, want), (shift, hex(other))
    rng = np.random.default_rng(1)
    x = rng.integers(0, 2 ** 32, size=100000, dtype=np.uint32)
    assert np.array_equal(G.mul2_packed(x).view(np.uint8), G.mul(x.view(np.uint8), np.uint8(2)))


def test_horner_form_equals_the_sum_form():
    rng = np.random.default_rng(2)
    for width in (1, 2, 3, 8, 9, 56):
        out_len = 97
        chunks = [rng.integers(0, 256, size=int(rng.integers(0, out_len + 1)), dtype=np.uint8) for _ in range(width)]
        chunks[0] = rng.integers(0, 256, size=out_len, dtype=np.uint8)
        if width > 2:
            chunks[1] = None
        assert np.array_equal(G.q_horner(chunks, out_len), G.q_sum(chunks, out_len)), width
    assert np.array_equal(G.q_sum([np.array([1], np.uint8)] * 9, 1), [np.bitwise_xor.reduce(G.EXP[:9])])


def test_recovery_formulas_for_every_pair_of_a_9_wide_stripe():
    rng = np.random.default_rng(3)
    width = 9
    lens = [0, 1, 15, 16, 17, 33, 40, 7, 40]
    out_len = max(lens)
    chunks = [rng.integers(1, 256, size=L, dtype=np.uint8) for L in lens]
    p, q = G.p_of(chunks, out_len), G.q_sum(chunks, out_len)
    full = G.padded(chunks, out_len)
    npairs = 0
    for x in range(width):
        surv = [None if k == x else c for k, c in enumerate(chunks)]
        assert np.array_equal(G.recover_one_from_q(surv, q, x, out_len), full[x]), x
        for y in range(x + 1, width):
            surv = [None if k in (x, y) else c for k, c in enumerate(chunks)]
            dx, dy = G.recover_two(surv, p, q, x, y, out_len)
            assert np.array_equal(dx, full[x]) and np.array_equal(dy, full[y]), (x, y)
            npairs += 1
    assert npairs == 36


def test_q_target_cases(bcp):
    qt = bcp.q_target
    assert qt(S.with_p(0b00011, 2), 5) == 3                 # the first free target after P
    assert qt(S.with_p(0b01011, 2), 5) == 4                 # the next one holds a chunk
    assert qt(S.with_p(0b00111, 4), 5) == 3                 # wraps past the last target, over three holders
    assert qt(S.with_p(0b00110, 4), 5) == 0                 # wraps to target 0
    assert qt(S.with_p(0b01111, 4), 5) == -1                # none free
    assert qt(S.with_p(0b1, 1), 2) == -1
    assert qt(S.with_p(0b0, 1), 2) == 0                     # an item without holders still has a Q target
    assert qt(S.with_p(0b00011, S.NO_P), 5) == -1           # NO_P
    assert qt(S.with_p(0b00111, 2), 5) == -1                # P holds a chunk
    assert qt(S.with_p(0b00011, 5), 5) == -1                # P outside the targets
    assert qt(S.with_p(0b00011, 2), 0) == -1 and qt(S.with_p(0b00011, 2), 57) == -1
    assert qt(S.with_p((1 << 54) - 1, 54), 56) == 55 and qt(S.with_p((1 << 54) - 1, 55), 56) == 54


def test_q_target_agrees_with_the_restatement(bcp):
    rng = np.random.default_rng(4)
    for _ in range(1000):
        nt = int(rng.integers(1, 57))
        holders = int(rng.integers(0, 2 ** 56, dtype=np.uint64))
        if rng.random() < 0.7:
            holders &= (1 << nt) - 1
            if rng.random() < 0.5:  # few holders
                holders &= int(rng.integers(0, 2 ** 56, dtype=np.uint64)) & int(rng.integers(0, 2 ** 56, dtype=np.uint64))
        p = int(rng.choice([int(rng.integers(0, nt)), int(rng.integers(0, 256)), 0xFF], p=[.8, .15, .05]))
        loc = S.with_p(holders, p)
        assert bcp.q_target(loc, nt) == G.q_target(loc, nt), (hex(loc), nt)


def test_engine_calls_null_arguments(bcp):
    L = bcp.lib()
    st = (bcp.Stripe * 1)(bcp.Stripe(0, 0, 0, 0, 0))
    so = (bcp.Source * 1)()
    qd = (ctypes.c_uint64 * 1)(0)
    lost = (bcp.PqLost * 1)()
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 12), ctypes.c_void_p)
    assert L.bcp_pq_stripes_async(None, st, 1, so, 0, qd) == -errno.EINVAL
    assert L.bcp_pq_stripes_async(fake, None, 1, so, 0, qd) == -errno.EINVAL
    assert L.bcp_pq_stripes_async(fake, st, 1, so, 0, None) == -errno.EINVAL
    assert L.bcp_pq_stripes_async(fake, st, 1, None, 1, qd) == -errno.EINVAL
    assert L.bcp_pq_recover_stripes_async(None, st, 1, so, 0, lost) == -errno.EINVAL
    assert L.bcp_pq_recover_stripes_async(fake, None, 1, so, 0, lost) == -errno.EINVAL
    assert L.bcp_pq_recover_stripes_async(fake, st, 1, so, 0, None) == -errno.EINVAL
    assert L.bcp_pq_recover_stripes_async(fake, st, 1, None, 1, lost) == -errno.EINVAL


def _rebuild2(bcp, pl, ntargets, a, b, items):
    arr, keep = bcp._items(items)
    st, st2 = bcp.RunStats(), bcp.Rebuild2Stats()
    return bcp.lib().bcp_pipeline_rebuild2(pl, b"/nonexistent-store", ntargets, a, b, arr, len(items), None, None, None,
                                           ctypes.byref(st), ctypes.byref(st2))


def test_rebuild2_validates_before_it_touches_anything(bcp):
    ok = [("a", 0, S.with_p(0b011, 2))]
    assert _rebuild2(bcp, None, 4, 0, 1, ok) == -errno.EINVAL
    # arguments and every item are checked before the pipeline is used at all,
    # so a stand-in for the handle (no device here to make one) is never read
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    assert _rebuild2(bcp, fake, 1, 0, 1, ok) == -errno.EINVAL
    assert _rebuild2(bcp, fake, 57, 0, 1, ok) == -errno.EINVAL
    assert _rebuild2(bcp, fake, 4, 1, 1, ok) == -errno.EINVAL     # target_a == target_b
    assert _rebuild2(bcp, fake, 4, -1, 1, ok) == -errno.EINVAL
    assert _rebuild2(bcp, fake, 4, 0, 4, ok) == -errno.EINVAL
    for loc in (S.with_p(0b011, 4),        # P outside the targets
                S.with_p(0b111, 2),        # P holds a chunk too
                S.with_p(0b10011, 2)):     # a holder outside the targets
        assert _rebuild2(bcp, fake, 4, 0, 1, ok + [("b", 0, loc)]) == -errno.EINVAL, hex(loc)
    L = bcp.lib()
    assert L.bcp_pipeline_set_q_parity(None, 1) == -errno.EINVAL
    assert L.bcp_pipeline_q_stats(None, None, None, None) == -errno.EINVAL


def test_structures_have_the_c_sizes(bcp, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "bcp.h"\n#include "bcp_task.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %d\\n", sizeof(bcp_pq_lost), '
                   'offsetof(bcp_pq_lost, q), offsetof(bcp_pq_lost, x), offsetof(bcp_pq_lost, y), '
                   'offsetof(bcp_pq_lost, dst_x), offsetof(bcp_pq_lost, len_x), offsetof(bcp_pq_lost, dst_y), '
                   'offsetof(bcp_pq_lost, len_y), sizeof(bcp_rebuild2_stats), '
                   'offsetof(bcp_rebuild2_stats, unrecoverable), BCP_PQ_NONE, BCP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, R = bcp.PqLost, bcp.Rebuild2Stats
    assert got == [ctypes.sizeof(P), P.q.offset, P.x.offset, P.y.offset, P.dst_x.offset, P.len_x.offset, P.dst_y.offset,
                   P.len_y.offset, ctypes.sizeof(R), R.unrecoverable.offset, bcp.PQ_NONE, 4]
    assert ctypes.sizeof(P) == 56 and ctypes.sizeof(R) == 32


def test_cli_usage_paths(bcp):
    for args in (["parity-gen", "--complete", "--q", "--protocol", "store", "4"],
                 ["parity-gen", "--complete", "--procs", "--q", "store", "4"],
                 ["parity-rebuild", "store", "4", "1", "--also"],
                 ["parity-rebuild", "--also"],
                 ["parity-rebuild", "--also", "x", "store", "4", "1"],
                 ["parity-rebuild", "--also", "1", "store", "4", "1"],      # --also equal to the target
                 ["parity-rebuild", "--also", "4", "store", "4", "1"],      # outside the targets
                 ["parity-rebuild", "--protocol", "--also", "2", "store", "4", "1"],
                 ["parity-rebuild", "--procs", "--also", "2", "store", "4", "1"],
                 ["parity-rebuild", "--lost", "f", "store", "4", "1"]):     # --lost without --also
        r = subprocess.run([bcp.BIN_PATH, *args], capture_output=True)
        assert r.returncode == 1 and r.stderr.startswith(b"usage:"), args
        assert b"--q" in r.stderr and b"--also TARGET" in r.stderr and r.stdout == b""
