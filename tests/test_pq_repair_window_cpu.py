"""The windowed repair's host side, without a device: the phase rule
(bcp_pq_repair_win_phases) against its definition, the tests' own oracle
(tests/pq_repair_window.py) against the properties the contract promises, the
new entry point's export and null-argument validation, the ctypes prototypes
against the C header, and the CLI's --repair-windowed parsing."""
import ctypes
import errno
import itertools
import os
import subprocess

import numpy as np
import pytest

import pq_repair_window as R
from pq_window import LISTS, W, chunks_of, p_win, q_win, replayed_places

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_P, BAD_Q, ALL = R.BAD_P, R.BAD_Q, R.ALL
E = -errno.EINVAL


def _masks(n):
    """Every single-bit mask, every pair, a few triples, everything, nothing, and P / Q bits alone."""
    one = [1 << k for k in range(n)]
    two = [a | b for a, b in itertools.combinations(one, 2)]
    three = [a | b | c for a, b, c in itertools.islice(itertools.combinations(one, 3), 0, 20)]
    return one + two + three + [ALL, 0, BAD_P | BAD_Q, ALL & ~1]


@pytest.mark.parametrize("lens", LISTS, ids=lambda ls: f"{len(ls)}src")
def test_phases_against_the_definition(bcp, lens):
    for out_len in (max(lens), max(lens) - 1, 2 * W, 2 * W + 1, 1, 0):
        for allow in _masks(len(lens)):
            want = R.thresholds(lens, W, out_len, allow)
            assert bcp.pq_repair_win_phases(out_len, W, lens, allow) == (len(want) + 1, want), (lens, out_len, hex(allow))
            # a short buffer gets the first thresholds and the count is still the whole one
            assert bcp.pq_repair_win_phases(out_len, W, lens, allow, cap=1) == (len(want) + 1, want[:1])
            assert bcp.pq_repair_win_phases(out_len, 0, lens, allow) == (1, [])  # no window: one phase


def test_phases_of_hand_made_stripes(bcp):
    V = bcp.pq_repair_win_phases
    lens = LISTS[0]                                    # [65541, 32771, 100, 0, 32768, 98304], out_len 98304
    n = max(lens)
    assert [R.lim_of(x, W) for x in lens] == [3 * W, 2 * W, W, None, W, 3 * W]
    assert V(n, W, lens, 1 << 2) == (2, [W])
    assert V(n, W, lens, (1 << 2) | (1 << 4)) == (2, [W])        # two members, one T_k: one threshold
    assert V(n, W, lens, (1 << 1) | (1 << 2)) == (3, [W, 2 * W])
    assert V(n, W, lens, (1 << 0) | (1 << 5)) == (1, [])          # T_k >= out_len: no phase of its own
    assert V(n, W, lens, 1 << 3) == (1, [])                       # len_k = 0
    assert V(n, W, lens, BAD_P | BAD_Q) == (1, [])                # P and Q have no echo
    assert V(n, W, lens, ALL) == (3, [W, 2 * W])
    assert V(n, 0, lens, ALL) == (1, [])                          # window 0
    assert V(n + 1, W, lens, ALL) == (4, [W, 2 * W, 3 * W])       # now 3 W lies below out_len
    assert V(2 * W, W, lens, ALL) == (2, [W])
    assert V(n, 2 * W, lens, ALL) == (2, [2 * W])                 # a larger window: T = 4W, 2W, 2W, -, 2W, 4W
    assert V(0, W, [], ALL) == (1, [])
    # the phase of a tile, both tile sizes: no tile straddles a threshold
    for T in (16384, 32768):
        b = R.thresholds(lens, W, n, ALL)
        assert [R.phase_of(b, off) for off in range(0, n, T)] == sorted(R.phase_of(b, off) for off in range(0, n, T))
        assert all(R.phase_of(b, off) == R.phase_of(b, off + T - 1) for off in range(0, n, T))


def test_phases_refuse_bad_arguments(bcp):
    L = bcp.lib()
    st = bcp.Stripe(0, 100, 0, 1, W)
    so = (bcp.Source * 57)()
    bounds = (ctypes.c_uint64 * 56)()
    assert L.bcp_pq_repair_win_phases(None, so, 1, bounds, 56) == E
    assert L.bcp_pq_repair_win_phases(ctypes.byref(st), None, 1, bounds, 56) == E
    assert L.bcp_pq_repair_win_phases(ctypes.byref(st), so, 1, None, 56) == E
    assert L.bcp_pq_repair_win_phases(ctypes.byref(st), so, 1, None, 0) == 1      # counting only
    for window in (16384, 1, W + 16, 10 * 1024 * 1024 + 512):
        with pytest.raises(bcp.BcpError) as e:
            bcp.pq_repair_win_phases(100, window, [100], 1)
        assert e.value.rc == E, window
    assert bcp.pq_repair_win_phases(100, 10 * 1024 * 1024, [100], 1) == (1, [])  # BCP_WINDOW_BYTES is a multiple
    with pytest.raises(bcp.BcpError) as e:
        bcp.pq_repair_win_phases(100, W, [1] * 57, 1)
    assert e.value.rc == E
    assert bcp.pq_repair_win_phases(100, W, [1] * 56, ALL) == (1, [])


def _damage(lens, seed):
    """One stripe of `lens` with one wrong byte per stream offset at most: two data members in their last
    windows (so with every echo the list gives them), a P byte and a Q byte.  Returns the pristine and the
    damaged (chunks, p, q) and the damaged data positions."""
    chunks = chunks_of(lens, seed)
    n = max(lens)
    p, q = p_win(chunks, W, n), q_win(chunks, W, n)
    short = sorted((k for k, x in enumerate(lens) if x), key=lambda k: (R.lim_of(lens[k], W), k))
    victims = [short[0], short[-1]] if len(short) > 1 else short[:1]
    bad = [np.array(c, copy=True) for c in chunks]
    taken = set()
    for i, k in enumerate(victims):
        j = lens[k] - 1 - i                     # in the last window: replayed wherever the stream is
        if j < 0 or any(x in taken for x in replayed_places(lens[k], W, n, j)):
            continue
        bad[k][j] ^= 0x5A
        taken |= set(replayed_places(lens[k], W, n, j))
    free = [j for j in range(n - 1, -1, -1) if j not in taken]
    p2, q2 = p.copy(), q.copy()
    p2[free[0]] ^= 0x11
    q2[free[1]] ^= 0x22
    return (chunks, p, q), (bad, p2, q2), victims


@pytest.mark.parametrize("lens", LISTS, ids=lambda ls: f"{len(ls)}src")
def test_oracle_restores_single_member_damage(lens):
    (chunks, p, q), (bad, p2, q2), _ = _damage(lens, seed=len(lens))
    n = max(lens)
    found = R.check_record(bad, p2, q2, W, n)
    rec, c3, p3, q3, phases = R.repair(bad, p2, q2, W, n, ALL)
    assert all(np.array_equal(a, b) for a, b in zip(c3, chunks)) and np.array_equal(p3, p) and np.array_equal(q3, q)
    assert rec[5] == 0 and rec[4] >= 3
    assert rec[0] == found[0] and rec[3] == found[3]
    assert rec[1] <= found[1] and rec[2] <= found[2]
    assert phases == len(R.thresholds(lens, W, n, ALL)) + 1
    assert R.check_record(c3, p3, q3, W, n) == (R.NONE_BAD, 0, 0, 0)


def test_oracle_counts_echoes_as_the_contract_says():
    lens = LISTS[0]
    n = max(lens)
    chunks = chunks_of(lens, 7)
    p, q = p_win(chunks, W, n), q_win(chunks, W, n)
    bad = [np.array(c, copy=True) for c in chunks]
    bad[2][50] ^= 0x5A                                  # len 100: echoes at 50 + W and 50 + 2 W
    assert R.check_record(bad, p, q, W, n) == (50, 3, 3, 1 << 2)
    rec, c3, _, _, phases = R.repair(bad, p, q, W, n, 1 << 2)
    assert rec == (50, 1, 1, 1 << 2, 1, 0) and phases == 2 and np.array_equal(c3[2], chunks[2])
    # the member left out of the mask: nothing written, every echo counted and left, one phase
    rec, c3, p3, q3, phases = R.repair(bad, p, q, W, n, ALL & ~(1 << 2))
    assert rec == (50, 3, 3, 1 << 2, 0, 3) and np.array_equal(c3[2], bad[2])
    assert phases == len(R.thresholds(lens, W, n, ALL & ~(1 << 2))) + 1
    # a window of 0 is the plain repair
    p0, q0 = p_win(chunks, 0, n), q_win(chunks, 0, n)
    rec, c3, _, _, phases = R.repair(bad, p0, q0, 0, n, ALL)
    assert rec == (50, 1, 1, 1 << 2, 1, 0) and phases == 1 and np.array_equal(c3[2], chunks[2])


def test_entry_point_is_exported_and_refuses_null_arguments(bcp):
    L = bcp.lib()
    assert hasattr(L, "bcp_pq_repair_stripes_win_async") and hasattr(L, "bcp_pipeline_set_repair_windowed")
    st = (bcp.Stripe * 1)(bcp.Stripe(0, 0, 0, 0, W))
    so = (bcp.Source * 1)()
    qb = (ctypes.c_uint64 * 1)(0)
    al = (ctypes.c_uint64 * 1)(ALL)
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    f = L.bcp_pq_repair_stripes_win_async
    assert f(None, st, 1, so, 0, qb, al, fake) == E        # a null queue
    assert f(fake, st, 1, so, 0, qb, None, fake) == E      # no masks
    assert f(fake, st, 1, so, 0, qb, al, None) == E        # no result records
    assert f(fake, st, 1, so, 0, None, al, fake) == E      # no Q bodies
    assert f(fake, None, 1, so, 0, qb, al, fake) == E
    assert f(fake, st, 1, None, 1, qb, al, fake) == E      # sources announced but absent
    assert L.bcp_pipeline_set_repair_windowed(None, 1) == E
    assert L.bcp_abi_version() == 4                        # additive: the ABI version stays


def test_prototypes_match_the_header(bcp, tmp_path):
    """A C file that assigns each new function to a pointer of the type the ctypes table assumes compiles
    without a warning, and the structures the calls pass have the C sizes."""
    src = tmp_path / "protos.c"
    src.write_text('#include <stdio.h>\n#include "bcp.h"\n#include "bcp_task.h"\n'
                   'int (*f1)(bcp_queue *, const bcp_stripe *, uint32_t, const bcp_source *, uint32_t, const uint64_t *,'
                   ' const uint64_t *, bcp_pq_repair_result *) = bcp_pq_repair_stripes_win_async;\n'
                   'int (*f2)(const bcp_stripe *, const bcp_source *, uint64_t, uint64_t *, uint32_t) = '
                   'bcp_pq_repair_win_phases;\n'
                   'int (*f3)(bcp_pipeline *, int) = bcp_pipeline_set_repair_windowed;\n'
                   'int main(void) { printf("%zu %zu %zu %d %d\\n", sizeof(bcp_stripe), sizeof(bcp_source), '
                   'sizeof(bcp_pq_repair_result), BCP_ABI_VERSION, BCP_MAX_SOURCES); return !(f1 && f2 && f3); }\n')
    exe = tmp_path / "protos"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", os.path.dirname(bcp.LIB_PATH), "-lbcp", "-Wl,-rpath," + os.path.dirname(bcp.LIB_PATH)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(bcp.Stripe), ctypes.sizeof(bcp.Source), ctypes.sizeof(bcp.PqRepairResult), 4,
                   bcp.MAX_SOURCES]
    for name in ("bcp_pq_repair_stripes_win_async", "bcp_pq_repair_win_phases", "bcp_pipeline_set_repair_windowed"):
        assert name in bcp._SIGS and hasattr(bcp.lib(), name)
    assert len(bcp.lib().bcp_pq_repair_stripes_win_async.argtypes) == 8
    assert len(bcp.lib().bcp_pq_repair_win_phases.argtypes) == 5


def test_cli_repair_windowed_usage_errors(bcp, tmp_path):
    for args in (["--q", "--q-windowed", "--repair-windowed", "store", "4"],              # without --repair
                 ["--q", "--repair", "all", "--repair-windowed", "store", "4"],           # without --q-windowed
                 ["--repair-windowed", "store", "4"],
                 ["--q", "--repair-windowed", "store", "4"]):
        r = subprocess.run([bcp.BIN_PATH, "parity-verify", *args], capture_output=True)
        assert r.returncode == 2 and r.stderr.startswith(b"usage:") and b"--repair-windowed" in r.stderr, args
        assert r.stdout == b""


def test_cli_repair_windowed_parses_and_reaches_the_engine(bcp, tmp_path):
    """With both --repair and --q-windowed the flag is accepted: the run ends with the engine's verdict (or its
    error where there is no device), not with usage."""
    import bcp_store as S
    root = str(tmp_path / "store")
    S.make_store(root, 4)
    subprocess.run([bcp.BIN_PATH, "parity-gen", "--complete", "--protocol", root, "4"], capture_output=True)
    r = subprocess.run([bcp.BIN_PATH, "parity-verify", "--q", "--q-windowed", "--repair", "all", "--repair-windowed",
                        "--dry-run", root, "4"], capture_output=True)
    assert not r.stderr.startswith(b"usage:") and r.returncode != 2, r.stderr
