"""Scrub repair of items past the 10 MiB window, end to end
(bcp_pipeline_set_repair_windowed, bin/bcp parity-verify --q --q-windowed
--repair ... --repair-windowed).  The store is a handful of small items and the
two smallest windowed shapes the suite uses, written once with Q and
q_windowed; tests work on copies with the mtimes kept.

The chunk damage is byte 1000 of the 10 MiB chunk of [10485760, 26214405]: its
last readable window is window 0, so the streams replay it at + 10 MiB and
+ 20 MiB and the scrub counts it three times; the repair corrects it once, at
its home, and its echo tiles -- a later launch -- find it clean.  With the
switch off windowed items are reported and left alone, as they always were."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bcp_store as S
from pq_window import replayed_places
from test_gpu_repair_q import (_same_as_found, _write_db, chunk, hdr, parity, parityq, read_lines,  # noqa: F401
                               repair_counts)
from test_gpu_verify_q import flip, gpu_fold, q_target, read_path, snapshot  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
KiB, MiB = 1024, 1024 * 1024
NT = 16
BLOCK = 4096
WIN = 10 * MiB
KAT4, THREE, SMALL = 5, 6, 2       # indices in the store's file list
P_OFF = WIN + 777                  # of w/three's P body: past the window, where the 64 KiB member is replayed


@pytest.fixture(scope="module")
def pristine(bcp, engine, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pristine_win"))
    rng = np.random.default_rng(11)
    files = []
    for i in range(5):
        holders, p = S.random_layout(rng, NT, i + 1)
        files.append((f"s/c{i}", holders, p, [int(x) | 1 for x in rng.integers(20 * KiB, 120 * KiB, size=i + 1)]))
    files.append(("w/kat4", [0, 1], 2, [10485760, 26214405]))
    files.append(("w/three", [0, 1, 2], 3, [11 * MiB + 3, 64 * KiB + 5, 10 * MiB]))
    items, _ = S.populate(root, NT, files, seed=11)
    bcp.set_xor_hook(None)
    pl = bcp.Pipeline(io_threads=4)
    try:
        pl.set_q_parity(True)
        pl.set_q_windowed(True)
        st = pl.run(root, NT, items)
    finally:
        pl.close()
        bcp.task_shutdown()
    assert st.errors == 0 and st.tasks == len(files)
    assert all(q_target(f) >= 0 for f in files)
    return root, files, items


@pytest.fixture
def store(pristine, tmp_path):
    src, files, items = pristine
    root = str(tmp_path / "store")
    shutil.copytree(src, root, copy_function=shutil.copy2)
    return root, files, items


def damage(root, files, small=True):
    """Byte 1000 of w/kat4's 10 MiB chunk, a P byte of w/three past 10 MiB and (small) a Q byte of a small item,
    mtimes kept.  Returns the repaired-list lines a full repair writes, sorted."""
    assert replayed_places(10485760, WIN, 26214405, 1000) == [1000, 1000 + WIN, 1000 + 2 * WIN]
    flip(chunk(root, files[KAT4], 0), 1000)
    flip(parity(root, files[THREE]), hdr(files[THREE]) + P_OFF)
    lines = [f"w/kat4\tdata\t{files[KAT4][1][0]}\t{BLOCK}", f"w/three\tp\t{files[THREE][2]}\t{BLOCK}"]
    if small:
        f = files[SMALL]
        assert max(f[3]) > 2 * BLOCK
        flip(parityq(root, f), hdr(f) + BLOCK + 5)
        lines.append(f"{f[0]}\tq\t{q_target(f)}\t{BLOCK}")
    return sorted(lines)


def run_both(bcp, root, items, tmp, windowed=True, **kw):
    """verify_q just before, then repair_q with the switch as given."""
    names = [str(tmp / n) for n in ("bad0", "culprits0", "bad1", "culprits1", "repaired")]
    pl = bcp.Pipeline(io_threads=4)
    try:
        pl.set_q_windowed(True)
        if windowed is not None:
            pl.set_repair_windowed(windowed)
        vst, vres = pl.verify_q(root, NT, items, bad_list=names[0], culprit_list=names[1])
        rst, rres = pl.repair_q(root, NT, items, bad_list=names[2], culprit_list=names[3], repaired_list=names[4], **kw)
    finally:
        pl.close()
    return vst, vres, (read_lines(names[0]), read_lines(names[1])), rst, rres, (read_lines(names[2]),
                                                                                read_lines(names[3])), read_lines(names[4])


def test_repair_all_restores_the_store(bcp, store, tmp_path, read_path):
    root, files, items = store
    before = snapshot(root)
    want_lines = damage(root, files)
    assert snapshot(root) != before
    vst, vres, vlists, rst, rres, rlists, repaired = run_both(bcp, root, items, tmp_path, mode=bcp.REPAIR_ALL)
    assert vst.v.mismatch == 3 and rlists == vlists
    _same_as_found(vres, rres)                    # the as-found fields are a verify_q's made just before
    assert (rres[KAT4].first_bad, rres[KAT4].p_bad, rres[KAT4].q_bad) == (1000, 3, 3)  # the byte and its two echoes
    assert (rres[THREE].first_bad, rres[THREE].p_bad, rres[THREE].q_bad) == (P_OFF, 1, 0)
    bad = sorted((SMALL, KAT4, THREE))
    assert [i for i, r in enumerate(rres) if r.repair != bcp.REPAIRED_NONE] == bad
    assert [rres[i].repair for i in bad] == [bcp.REPAIRED_DONE] * 3
    assert [rres[i].bytes_fixed for i in bad] == [1, 1, 1]
    assert repair_counts(rst) == dict(none=len(items) - 3, done=3, dry=0, policy=0, unlocated=0, changed=0, failed=0)
    assert rst.files_written == 3 and rst.bytes_written == 3 * BLOCK and rst.q.v.errors == 0  # one block per file
    assert 1 <= rst.repair_launches <= 3
    assert sorted(repaired) == want_lines
    assert snapshot(root) == before               # SHA-256 and mtime in nanoseconds
    pl = bcp.Pipeline(io_threads=4)
    try:
        pl.set_q_windowed(True)
        st, res = pl.verify_q(root, NT, items)
    finally:
        pl.close()
    assert [r.status for r in res] == [bcp.VERIFY_OK] * len(items) and st.v.errors == 0


def test_repair_parity_leaves_the_chunk_alone(bcp, store, tmp_path):
    root, files, items = store
    before = snapshot(root)
    damage(root, files)
    damaged = snapshot(root)
    vst, vres, vlists, rst, rres, rlists, repaired = run_both(bcp, root, items, tmp_path, mode=bcp.REPAIR_PARITY)
    assert rlists == vlists
    _same_as_found(vres, rres)
    assert (rres[KAT4].repair, rres[THREE].repair, rres[SMALL].repair) == (bcp.REPAIRED_POLICY, bcp.REPAIRED_DONE,
                                                                          bcp.REPAIRED_DONE)
    assert repair_counts(rst) == dict(none=len(items) - 3, done=2, dry=0, policy=1, unlocated=0, changed=0, failed=0)
    assert rst.files_written == 2 and rst.bytes_written == 2 * BLOCK
    after = snapshot(root)
    c = chunk(root, files[KAT4], 0)
    assert after[c] == damaged[c] != before[c]    # byte-identical to the damaged chunk
    assert {k: v for k, v in after.items() if k != c} == {k: v for k, v in before.items() if k != c}


def test_dry_run_writes_nothing(bcp, store, tmp_path):
    root, files, items = store
    damage(root, files)
    damaged = snapshot(root)
    *_, rst, rres, _, repaired = run_both(bcp, root, items, tmp_path, mode=bcp.REPAIR_ALL, dry_run=True)
    assert [rres[i].repair for i in (SMALL, KAT4, THREE)] == [bcp.REPAIRED_DRY] * 3
    assert [rres[i].bytes_fixed for i in (SMALL, KAT4, THREE)] == [1, 1, 1]
    assert repaired == [] and rst.files_written == 0 and rst.bytes_written == 0 and rst.repair_launches >= 1
    assert repair_counts(rst) == dict(none=len(items) - 3, done=0, dry=3, policy=0, unlocated=0, changed=0, failed=0)
    assert snapshot(root) == damaged


@pytest.mark.parametrize("switch", (None, False))
def test_switch_off_reports_and_leaves_alone(bcp, store, tmp_path, switch):
    """Never set, and set to 0: windowed items are UNLOCATED and nothing is launched for them."""
    root, files, items = store
    damage(root, files, small=False)
    damaged = snapshot(root)
    vst, vres, vlists, rst, rres, rlists, repaired = run_both(bcp, root, items, tmp_path, windowed=switch,
                                                               mode=bcp.REPAIR_ALL, max_members=3)
    assert rlists == vlists and repaired == []
    _same_as_found(vres, rres)
    for i in (KAT4, THREE):
        assert (rres[i].status, rres[i].q_state, rres[i].repair) == (bcp.VERIFY_MISMATCH, bcp.QSTATE_CHECKED,
                                                                     bcp.REPAIRED_UNLOCATED)
    assert repair_counts(rst) == dict(none=len(items) - 2, done=0, dry=0, policy=0, unlocated=2, changed=0, failed=0)
    assert rst.repair_launches == 0 and rst.files_written == 0 and rst.q.v.errors == 0
    assert snapshot(root) == damaged


def test_switch_takes_only_0_and_1(bcp):
    pl = bcp.Pipeline(io_threads=1)
    try:
        for bad in (2, -1):
            with pytest.raises(bcp.BcpError):
                pl.set_repair_windowed(bad)
        pl.set_repair_windowed(True)
        pl.set_repair_windowed(False)
    finally:
        pl.close()


def test_cli_repair_windowed(bcp, store, tmp_path):
    root, files, items = store
    before = snapshot(root)
    want_lines = damage(root, files)
    damaged = snapshot(root)
    db = str(tmp_path / "db")
    _write_db(bcp, db, items)
    repaired = str(tmp_path / "repaired")
    args = [bcp.BIN_PATH, "parity-verify", "--db", db, "--q", "--q-windowed", "--repair", "all"]
    # without the flag: the small item is repaired, the windowed ones are reported and not written
    r = subprocess.run(args + [root, str(NT)], capture_output=True)
    assert r.returncode == 1, r.stdout + r.stderr
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 3 and " 3 mismatch, " in lines[0], r.stdout
    assert lines[2].startswith(f"repair (all): 1 done, 0 dry, 0 policy, 2 unlocated, 0 changed, 0 failed; 1 files, "
                               f"{BLOCK} bytes written, "), r.stdout
    after = snapshot(root)
    windowed = [p for p in before if "/w/" in p]
    assert len(windowed) == 2 + 3 + 2 * 2 and all(after[p] == damaged[p] for p in windowed)
    # with it: every mismatch ends DONE
    r = subprocess.run(args + ["--repair-windowed", "--repaired", repaired, root, str(NT)], capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 3 and " 2 mismatch, " in lines[0], r.stdout
    assert lines[1] == f"q files: {len(items)} checked, 0 none, 0 bad; culprits: 1 data, 1 p, 0 q, 0 many"
    assert lines[2].startswith(f"repair (all): 2 done, 0 dry, 0 policy, 0 unlocated, 0 changed, 0 failed; 2 files, "
                               f"{2 * BLOCK} bytes written, "), r.stdout
    assert sorted(read_lines(repaired)) == [ln for ln in want_lines if ln.startswith("w/")]
    assert snapshot(root) == before
    r = subprocess.run(args[:6] + [root, str(NT)], capture_output=True)
    assert r.returncode == 0 and len(r.stdout.decode().splitlines()) == 2, r.stdout + r.stderr
