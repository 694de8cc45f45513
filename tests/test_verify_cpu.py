"""The parity scrub's host-side contract, without a device: argument
validation of bcp_check_stripes_async and bcp_pipeline_verify, the CLI's usage
path, and the ctypes structures against the C headers."""
import ctypes
import errno
import os
import subprocess

import bcp_store as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_stripes_null_arguments(bcp):
    L = bcp.lib()
    st = (bcp.Stripe * 1)(bcp.Stripe(0, 0, 0, 0, 0))
    so = (bcp.Source * 1)()
    assert L.bcp_check_stripes_async(None, st, 1, so, 0, None) == -errno.EINVAL
    assert L.bcp_check_stripes_async(None, None, 0, None, 0, None) == -errno.EINVAL


def _verify(bcp, pl, ntargets, items):
    arr, keep = bcp._items(items)
    st = bcp.VerifyStats()
    return bcp.lib().bcp_pipeline_verify(pl, b"/nonexistent-store", ntargets, arr, len(items), None, None, None,
                                         ctypes.byref(st))


def test_pipeline_verify_validates_before_it_touches_anything(bcp):
    ok = [("a", 0, S.with_p(0b011, 2))]
    assert _verify(bcp, None, 4, ok) == -errno.EINVAL
    # arguments and every item are checked before the pipeline is used at all,
    # so a stand-in for the handle (no device here to make one) is never read
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    assert _verify(bcp, fake, 0, ok) == -errno.EINVAL
    assert _verify(bcp, fake, 57, ok) == -errno.EINVAL
    for loc in (S.with_p(0b011, 4),        # P outside the targets
                S.with_p(0b111, 2),        # P holds a chunk too
                S.with_p(0b10011, 2)):     # a holder outside the targets
        assert _verify(bcp, fake, 4, ok + [("b", 0, loc)]) == -errno.EINVAL, hex(loc)


def test_cli_parity_verify_usage(bcp):
    for args in ([], ["store"], ["store", "4", "extra"], ["--bad"], ["--read", "sideways", "store", "4"],
                 ["--frobnicate", "store", "4"], ["store", "0"], ["store", "57"]):
        r = subprocess.run([bcp.BIN_PATH, "parity-verify", *args], capture_output=True)
        assert r.returncode == 1 and r.stderr.startswith(b"usage:") and b"parity-verify" in r.stderr, args
        assert r.stdout == b""


def test_structures_have_the_c_sizes(bcp, tmp_path):
    assert ctypes.sizeof(bcp.CheckResult) == 16
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "bcp.h"\n#include "bcp_task.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(bcp_check_result), sizeof(bcp_verify_item), '
                   'sizeof(bcp_verify_stats), offsetof(bcp_verify_item, first_bad), '
                   'offsetof(bcp_verify_stats, errors)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(bcp.CheckResult), ctypes.sizeof(bcp.VerifyItem), ctypes.sizeof(bcp.VerifyStats),
                   bcp.VerifyItem.first_bad.offset, bcp.VerifyStats.errors.offset]
    assert bcp.VERIFY_OK == 0 and bcp.VERIFY_SKIPPED == 5
