"""The scrub repair's host-side contract, without a device: the policy
(bcp_pq_repair_verdict) against a few lines of Python, the in-place patch
(bcp_patch_file) on temporary files, the ctypes structures against the C
headers, argument validation, and the CLI's --repair parsing."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_P, BAD_Q, NOWHERE = 1 << 56, 1 << 57, 1 << 58
BLOCK = 4096


def ref_verdict(bcp, members, nsrc, mode, max_members):
    """The policy by its definition (include/bcp.h)."""
    if not members:
        return bcp.VERDICT_CLEAN, 0
    data = members & ((1 << 56) - 1)
    if members & ~(data | BAD_P | BAD_Q) or data >> nsrc:
        return bcp.VERDICT_UNLOCATED, 0
    if bin(members).count("1") > max_members or (data and mode == bcp.REPAIR_PARITY):
        return bcp.VERDICT_POLICY, 0
    return bcp.VERDICT_REPAIR, members


def test_verdict_of_hand_made_records(bcp):
    V = bcp.pq_repair_verdict
    P, A = bcp.REPAIR_PARITY, bcp.REPAIR_ALL
    # a single data bit in both modes
    assert V((7, 1, 1, 1 << 3), 9, A) == (bcp.VERDICT_REPAIR, 1 << 3)
    assert V((7, 1, 1, 1 << 3), 9, P) == (bcp.VERDICT_POLICY, 0)
    assert V((7, 300, 300, 1 << 55), 56, A) == (bcp.VERDICT_REPAIR, 1 << 55)
    # P alone, and Q alone
    for mode in (P, A):
        assert V((0, 1, 0, BAD_P), 9, mode) == (bcp.VERDICT_REPAIR, BAD_P)
        assert V((0, 0, 1, BAD_Q), 9, mode) == (bcp.VERDICT_REPAIR, BAD_Q)
    # two members with max_members 1 and 2
    for m in ((1 << 0) | (1 << 8), (1 << 2) | BAD_P, BAD_P | BAD_Q):
        assert V((7, 2, 2, m), 9, A, 1) == (bcp.VERDICT_POLICY, 0), hex(m)
        assert V((7, 2, 2, m), 9, A, 2) == (bcp.VERDICT_REPAIR, m), hex(m)
    assert V((7, 2, 2, BAD_P | BAD_Q), 9, P, 2) == (bcp.VERDICT_REPAIR, BAD_P | BAD_Q)
    assert V((7, 2, 2, (1 << 2) | BAD_P), 9, P, 2) == (bcp.VERDICT_POLICY, 0)  # a data bit under PARITY
    # BAD_NOWHERE, whatever else is set; a clean record
    for m in (NOWHERE, NOWHERE | 1, NOWHERE | BAD_P):
        assert V((7, 1, 1, m), 9, A, 3) == (bcp.VERDICT_UNLOCATED, 0), hex(m)
    assert V(bcp.PQ_CHECK_CLEAN, 9, A) == (bcp.VERDICT_CLEAN, 0)
    # everything against the definition
    bits = [0, 1 << 0, 1 << 1, 1 << 8, 1 << 9, 1 << 55, BAD_P, BAD_Q, NOWHERE, 1 << 59]
    for a in bits:
        for b in bits:
            for nsrc in (1, 9, 56):
                for mode in (P, A):
                    for mm in (1, 2, 3):
                        assert V((7, 2, 2, a | b), nsrc, mode, mm) == ref_verdict(bcp, a | b, nsrc, mode, mm), \
                            (hex(a | b), nsrc, mode, mm)


def test_verdict_refuses_bad_arguments(bcp):
    with pytest.raises(bcp.BcpError) as e:
        bcp.pq_repair_verdict(None, 9, bcp.REPAIR_ALL)  # a null record
    assert e.value.rc == -errno.EINVAL
    for mode in (0, 3, -1):
        with pytest.raises(bcp.BcpError) as e:
            bcp.pq_repair_verdict((7, 1, 1, 1), 9, mode)
        assert e.value.rc == -errno.EINVAL
    r = bcp.PqCheckResult(7, 1, 1, 1)
    assert bcp.lib().bcp_pq_repair_verdict(ctypes.byref(r), 9, bcp.REPAIR_ALL, 1, None) == -errno.EINVAL


def _file(tmp_path, name, data, when_ns=(1_600_000_000_123_456_789, 1_500_000_000_987_654_321)):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data.tobytes())
    os.utime(p, ns=when_ns)  # (atime, mtime)
    return p


def _times(p):
    st = os.stat(p)
    return st.st_size, st.st_atime_ns, st.st_mtime_ns


def test_patch_writes_only_the_blocks_that_differ(bcp, tmp_path):
    rng = np.random.default_rng(1)
    head = 72                                   # a parity file's header: the body starts here
    n = 5 * BLOCK + 123                         # the last block is clipped at the file's end
    now = rng.integers(0, 256, size=n, dtype=np.uint8)
    hdr = rng.integers(0, 256, size=head, dtype=np.uint8)
    for flips, want in (((0,), BLOCK), ((BLOCK - 1, BLOCK), 2 * BLOCK), ((n - 1,), 123),
                        ((2 * BLOCK + 7, 5 * BLOCK), BLOCK + 123), (tuple(range(3 * BLOCK, 4 * BLOCK)), BLOCK),
                        ((), 0)):
        was = now.copy()
        was[list(flips)] ^= 0x5A
        p = _file(tmp_path, "f", np.concatenate([hdr, was]))
        before = _times(p)
        got = bcp.patch_file(p, head, was, now, before[0], before[2])
        assert got == want, (flips, got, want)
        assert _times(p) == before, flips       # size, atime and mtime, in nanoseconds (before this test reads it)
        assert np.array_equal(np.fromfile(p, dtype=np.uint8), np.concatenate([hdr, now])), flips


def test_patch_touches_nothing_outside_the_differing_blocks(bcp, tmp_path):
    """The file differs from `was` in a block where now == was: that block is not written."""
    n = 3 * BLOCK
    was = np.zeros(n, np.uint8)
    now = was.copy()
    now[BLOCK + 5] = 9
    on_disk = was.copy()
    on_disk[7] = 0xEE                           # block 0, not part of the patch
    p = _file(tmp_path, "g", on_disk)
    before = _times(p)
    assert bcp.patch_file(p, 0, was, now, n, before[2]) == BLOCK
    want = on_disk.copy()
    want[BLOCK:2 * BLOCK] = now[BLOCK:2 * BLOCK]
    assert np.array_equal(np.fromfile(p, dtype=np.uint8), want)


def test_patch_leaves_a_changed_file_alone(bcp, tmp_path):
    n = 2 * BLOCK + 1
    was = np.arange(n, dtype=np.uint32).astype(np.uint8)
    now = was.copy()
    now[3] ^= 1
    p = _file(tmp_path, "h", was)
    size, atime, mtime = _times(p)
    for exp_size, exp_mtime in ((size + 1, mtime), (size, mtime + 1), (size, mtime - 10 ** 9)):
        with pytest.raises(bcp.BcpError) as e:
            bcp.patch_file(p, 0, was, now, exp_size, exp_mtime)
        assert e.value.rc == -errno.ESTALE
        assert _times(p) == (size, atime, mtime) and np.array_equal(np.fromfile(p, dtype=np.uint8), was)
        os.utime(p, ns=(atime, mtime))          # (this test's own read may have moved the atime)
    os.utime(p, ns=(atime, mtime + 5))          # modified by a user after the scrub's stat
    with pytest.raises(bcp.BcpError) as e:
        bcp.patch_file(p, 0, was, now, size, mtime)
    assert e.value.rc == -errno.ESTALE
    assert _times(p) == (size, atime, mtime + 5) and np.array_equal(np.fromfile(p, dtype=np.uint8), was)
    # a body that would reach past the file's end is refused, nothing is resized
    with pytest.raises(bcp.BcpError) as e:
        bcp.patch_file(p, 1, was, now, size, mtime + 5)
    assert e.value.rc == -errno.EINVAL and _times(p)[0] == size


def test_patch_of_a_missing_file(bcp, tmp_path):
    p = str(tmp_path / "missing")
    a = np.zeros(16, np.uint8)
    with pytest.raises(bcp.BcpError) as e:
        bcp.patch_file(p, 0, a, a + 1, 16, 0)
    assert e.value.rc == -errno.ENOENT
    assert not os.path.exists(p)                # and it is not created


def test_structures_have_the_c_sizes(bcp, tmp_path):
    assert ctypes.sizeof(bcp.PqRepairResult) == 48 and ctypes.sizeof(bcp.RepairQItem) == 56
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <time.h>\n#include "bcp.h"\n#include "bcp_task.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(bcp_pq_repair_result), '
                   'sizeof(bcp_repair_q_item), sizeof(bcp_repair_q_stats), offsetof(bcp_pq_repair_result, fixed), '
                   'offsetof(bcp_pq_repair_result, left), offsetof(bcp_repair_q_item, repair), '
                   'offsetof(bcp_repair_q_item, bytes_fixed), offsetof(bcp_repair_q_stats, none), '
                   'offsetof(bcp_repair_q_stats, repair_launches));\n'
                   'printf("%d %d %d %d %d %d\\n", BCP_REPAIR_PARITY, BCP_REPAIR_ALL, BCP_VERDICT_CLEAN, '
                   'BCP_VERDICT_REPAIR, BCP_VERDICT_UNLOCATED, BCP_VERDICT_POLICY);\n'
                   'printf("%d %d %d %d %d %d %d\\n", BCP_REPAIRED_NONE, BCP_REPAIRED_DONE, BCP_REPAIRED_DRY, '
                   'BCP_REPAIRED_POLICY, BCP_REPAIRED_UNLOCATED, BCP_REPAIRED_CHANGED, BCP_REPAIRED_FAILED);\n'
                   'printf("%zu %zu\\n", sizeof(struct timespec), offsetof(struct timespec, tv_nsec)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [48, 56, ctypes.sizeof(bcp.RepairQStats), bcp.PqRepairResult.fixed.offset,
                   bcp.PqRepairResult.left.offset, bcp.RepairQItem.repair.offset, bcp.RepairQItem.bytes_fixed.offset,
                   bcp.RepairQStats.none.offset, bcp.RepairQStats.repair_launches.offset,
                   bcp.REPAIR_PARITY, bcp.REPAIR_ALL, bcp.VERDICT_CLEAN, bcp.VERDICT_REPAIR, bcp.VERDICT_UNLOCATED,
                   bcp.VERDICT_POLICY, bcp.REPAIRED_NONE, bcp.REPAIRED_DONE, bcp.REPAIRED_DRY, bcp.REPAIRED_POLICY,
                   bcp.REPAIRED_UNLOCATED, bcp.REPAIRED_CHANGED, bcp.REPAIRED_FAILED,
                   ctypes.sizeof(bcp.Timespec), bcp.Timespec.tv_nsec.offset]
    # the verify_q fields come first, unchanged
    for name, _ in bcp.VerifyQItem._fields_:
        assert getattr(bcp.RepairQItem, name).offset == getattr(bcp.VerifyQItem, name).offset


def test_pq_repair_null_arguments(bcp):
    L = bcp.lib()
    st = (bcp.Stripe * 1)(bcp.Stripe(0, 0, 0, 0, 0))
    so = (bcp.Source * 1)()
    qb = (ctypes.c_uint64 * 1)(0)
    al = (ctypes.c_uint64 * 1)(2 ** 64 - 1)
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    assert L.bcp_pq_repair_stripes_async(None, st, 1, so, 0, qb, al, fake) == -errno.EINVAL   # a null queue
    assert L.bcp_pq_repair_stripes_async(fake, st, 1, so, 0, qb, None, fake) == -errno.EINVAL  # no masks
    assert L.bcp_pq_repair_stripes_async(fake, st, 1, so, 0, qb, al, None) == -errno.EINVAL   # no result records
    assert L.bcp_pq_repair_stripes_async(fake, st, 1, so, 0, None, al, fake) == -errno.EINVAL  # no Q bodies
    assert L.bcp_pq_repair_stripes_async(fake, None, 1, so, 0, qb, al, fake) == -errno.EINVAL


def test_pipeline_repair_q_validates_before_it_touches_anything(bcp):
    import bcp_store as S
    items = [("a", 0, S.with_p(0b011, 2))]
    arr, keep = bcp._items(items)
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)

    def rc(pl, mode, members):
        return bcp.lib().bcp_pipeline_repair_q(pl, b"/nonexistent-store", 4, arr, 1, mode, members, 0, None, None,
                                               None, None, None, None)

    assert rc(None, bcp.REPAIR_ALL, 1) == -errno.EINVAL
    assert rc(fake, 0, 1) == -errno.EINVAL and rc(fake, 3, 1) == -errno.EINVAL  # a mode that is neither
    assert rc(fake, bcp.REPAIR_ALL, 0) == -errno.EINVAL                          # no member may be written
    del keep


def test_cli_repair_usage_errors(bcp, tmp_path):
    f = str(tmp_path / "repaired")
    for args in (["--repair", "all", "store", "4"],                      # without --q
                 ["--repair", "parity", "--repaired", f, "store", "4"],
                 ["--q", "--repair", "chunks", "store", "4"],             # a bad mode
                 ["--q", "--repair", "", "store", "4"],
                 ["--q", "--repair", "all", "--repair-members", "0", "store", "4"],
                 ["--q", "--repair", "all", "--repair-members", "two", "store", "4"],
                 ["--q", "--dry-run", "store", "4"],                      # the repair's options without --repair
                 ["--q", "--repaired", f, "store", "4"],
                 ["--q", "--repair-members", "2", "store", "4"]):
        r = subprocess.run([bcp.BIN_PATH, "parity-verify", *args], capture_output=True)
        assert r.returncode == 2 and r.stderr.startswith(b"usage:") and b"--repair" in r.stderr, args
        assert r.stdout == b""
    assert not os.path.exists(f)


def test_cli_repair_parses_and_reaches_the_engine(bcp, tmp_path):
    """Without a device the run ends with the engine's error, not with usage."""
    import bcp_store as S
    root = str(tmp_path / "store")
    S.make_store(root, 4)
    subprocess.run([bcp.BIN_PATH, "parity-gen", "--complete", "--protocol", root, "4"], capture_output=True)
    r = subprocess.run([bcp.BIN_PATH, "parity-verify", "--q", "--repair", "parity", "--repair-members", "2", "--dry-run",
                        "--repaired", str(tmp_path / "repaired"), root, "4"], capture_output=True)
    assert not r.stderr.startswith(b"usage:"), r.stderr
    if bcp.device_count() == 0:
        assert r.returncode == 1 and r.stdout == b"" and b"parity-verify" in r.stderr and b"device" in r.stderr.lower()
