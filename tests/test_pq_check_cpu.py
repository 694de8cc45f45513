"""The Q-aware scrub's host-side contract, without a device: bcp_pq_culprit,
the ctypes structures against the C headers, argument validation, and the
CLI's --q / --culprits parsing."""
import ctypes
import errno
import os
import subprocess

import bcp_store as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_P, BAD_Q, NOWHERE = 1 << 56, 1 << 57, 1 << 58


def test_culprit_of_a_record(bcp):
    assert bcp.pq_culprit((2 ** 64 - 1, 0, 0, 0)) == (bcp.CULPRIT_NONE, -1)
    assert bcp.pq_culprit((7, 1, 1, 1 << 0)) == (bcp.CULPRIT_DATA, 0)
    assert bcp.pq_culprit((7, 1, 1, 1 << 55)) == (bcp.CULPRIT_DATA, 55)
    assert bcp.pq_culprit((7, 300, 300, 1 << 31)) == (bcp.CULPRIT_DATA, 31)
    assert bcp.pq_culprit((7, 1, 0, BAD_P)) == (bcp.CULPRIT_P, -1)
    assert bcp.pq_culprit((7, 0, 1, BAD_Q)) == (bcp.CULPRIT_Q, -1)
    assert bcp.pq_culprit((7, 1, 1, NOWHERE)) == (bcp.CULPRIT_MANY, -1)
    bits = [1 << 0, 1 << 1, 1 << 55, BAD_P, BAD_Q, NOWHERE]
    for i, a in enumerate(bits):
        for b in bits[i + 1:]:
            assert bcp.pq_culprit((7, 2, 2, a | b)) == (bcp.CULPRIT_MANY, -1), hex(a | b)
    assert (bcp.PQ_BAD_P, bcp.PQ_BAD_Q, bcp.PQ_BAD_NOWHERE) == (BAD_P, BAD_Q, NOWHERE)
    L = bcp.lib()
    pos = ctypes.c_int(5)
    assert L.bcp_pq_culprit(None, ctypes.byref(pos)) == -errno.EINVAL
    r = bcp.PqCheckResult(3, 1, 1, 1 << 9)
    assert L.bcp_pq_culprit(ctypes.byref(r), None) == bcp.CULPRIT_DATA  # the position is optional


def test_structures_have_the_c_sizes(bcp, tmp_path):
    assert ctypes.sizeof(bcp.PqCheckResult) == 32 and ctypes.sizeof(bcp.VerifyQItem) == 40
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "bcp.h"\n#include "bcp_task.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(bcp_pq_check_result), '
                   'sizeof(bcp_verify_q_item), sizeof(bcp_verify_q_stats), offsetof(bcp_pq_check_result, members), '
                   'offsetof(bcp_verify_q_item, target), offsetof(bcp_verify_q_item, q_bad), '
                   'offsetof(bcp_verify_q_stats, culprit_many));\n'
                   'printf("%d %d %d %d %d %d %d %d\\n", BCP_CULPRIT_NONE, BCP_CULPRIT_DATA, BCP_CULPRIT_P, BCP_CULPRIT_Q, '
                   'BCP_CULPRIT_MANY, BCP_QSTATE_CHECKED, BCP_QSTATE_NONE, BCP_QSTATE_BAD); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 40, ctypes.sizeof(bcp.VerifyQStats), bcp.PqCheckResult.members.offset,
                   bcp.VerifyQItem.target.offset, bcp.VerifyQItem.q_bad.offset, bcp.VerifyQStats.culprit_many.offset,
                   bcp.CULPRIT_NONE, bcp.CULPRIT_DATA, bcp.CULPRIT_P, bcp.CULPRIT_Q, bcp.CULPRIT_MANY,
                   bcp.QSTATE_CHECKED, bcp.QSTATE_NONE, bcp.QSTATE_BAD]


def test_pq_check_null_arguments(bcp):
    L = bcp.lib()
    st = (bcp.Stripe * 1)(bcp.Stripe(0, 0, 0, 0, 0))
    so = (bcp.Source * 1)()
    qb = (ctypes.c_uint64 * 1)(0)
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    assert L.bcp_pq_check_stripes_async(None, st, 1, so, 0, qb, fake) == -errno.EINVAL
    assert L.bcp_pq_check_stripes_async(fake, st, 1, so, 0, qb, None) == -errno.EINVAL   # no result records
    assert L.bcp_pq_check_stripes_async(fake, st, 1, so, 0, None, fake) == -errno.EINVAL  # no Q bodies
    assert L.bcp_pq_check_stripes_async(fake, None, 1, so, 0, qb, fake) == -errno.EINVAL


def _verify_q(bcp, pl, ntargets, items):
    arr, keep = bcp._items(items)
    st = bcp.VerifyQStats()
    return bcp.lib().bcp_pipeline_verify_q(pl, b"/nonexistent-store", ntargets, arr, len(items), None, None, None, None,
                                           ctypes.byref(st))


def test_pipeline_verify_q_validates_before_it_touches_anything(bcp):
    ok = [("a", 0, S.with_p(0b011, 2))]
    assert _verify_q(bcp, None, 4, ok) == -errno.EINVAL
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    assert _verify_q(bcp, fake, 0, ok) == -errno.EINVAL
    assert _verify_q(bcp, fake, 57, ok) == -errno.EINVAL
    for loc in (S.with_p(0b011, 4), S.with_p(0b111, 2), S.with_p(0b10011, 2)):
        assert _verify_q(bcp, fake, 4, ok + [("b", 0, loc)]) == -errno.EINVAL, hex(loc)


def test_cli_culprits_needs_q(bcp, tmp_path):
    f = str(tmp_path / "culprits")
    for args in (["--culprits", f, "store", "4"], ["--culprits", "store", "4"], ["--q", "--culprits"],
                 ["--q", "store"], ["--q", "store", "57"]):
        r = subprocess.run([bcp.BIN_PATH, "parity-verify", *args], capture_output=True)
        assert r.returncode == 1 and r.stderr.startswith(b"usage:") and b"--culprits" in r.stderr, args
        assert r.stdout == b""
    assert not os.path.exists(f)


def test_cli_q_parses_and_reaches_the_engine(bcp, tmp_path):
    """Without a device the run ends with the engine's error, not with usage; with one it verifies the
    (empty) store."""
    root = str(tmp_path / "store")
    S.make_store(root, 4)
    r = subprocess.run([bcp.BIN_PATH, "parity-gen", "--complete", "--protocol", root, "4"], capture_output=True)
    f = str(tmp_path / "culprits")
    r = subprocess.run([bcp.BIN_PATH, "parity-verify", "--q", "--culprits", f, root, "4"], capture_output=True)
    assert not r.stderr.startswith(b"usage:"), r.stderr
    if bcp.device_count() == 0:
        assert r.returncode == 1 and r.stdout == b"" and b"parity-verify" in r.stderr and b"device" in r.stderr.lower()
