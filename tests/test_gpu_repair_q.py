"""The scrub repair end to end (bcp_pipeline_repair_q, bin/bcp parity-verify --q
--repair): a small store written with Q parity is damaged with the mtimes kept
and repaired in place.  The verdicts and both lists are bcp_pipeline_verify_q's
for the store as found; a repair restores the snapshot taken before the damage
-- every file's SHA-256 and its mtime in nanoseconds -- by writing only the
4 KiB blocks that changed; what must not be repaired (policy, dry run, windowed
items, items without Q, stale items) stays byte-identical to the damaged store."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bcp_store as S
from test_gpu_verify_q import WINDOWED, flip, gpu_fold, has_q, q_target, read_path, snapshot  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
KiB, MiB = 1024, 1024 * 1024
NT = 16
BLOCK = 4096


@pytest.fixture(scope="module")
def pristine(bcp, engine, tmp_path_factory):
    """The store, generated once with Q on: a dozen items of widths 1..9 with chunks of 20-200 KiB and odd
    lengths (one with a chunk missing at generation), one item with every target taken (no Q), and the smallest
    windowed item, with its Q file.  Tests work on copies (mtimes kept)."""
    root = str(tmp_path_factory.mktemp("pristine"))
    rng = np.random.default_rng(7)
    files = []
    for i in range(12):
        width = i % 9 + 1
        holders, p = S.random_layout(rng, NT, width)
        lens = [int(x) | 1 for x in rng.integers(20 * KiB, 200 * KiB, size=width)]
        files.append((f"v/{i % 3}/c{i:02d}", holders, p, lens))
    files.append(("full/all", [t for t in range(NT) if t != 5], 5, [20 * KiB + 2 * t + 1 for t in range(NT - 1)]))
    files.append(("big/a", [0, 1], 4, list(WINDOWED)))
    items, contents = S.populate(root, NT, files, seed=7)
    missing = files[5]  # width 6: its second holder's chunk never existed
    os.remove(S.chunk_path(root, missing[1][1], missing[0]))
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
    assert not has_q(files[12]) and q_target(files[13]) >= 0
    return root, files, items


@pytest.fixture
def store(pristine, tmp_path):
    src, files, items = pristine
    root = str(tmp_path / "store")
    shutil.copytree(src, root, copy_function=shutil.copy2)
    return root, files, items


def chunk(root, f, k):
    return S.chunk_path(root, f[1][k], f[0])


def parity(root, f):
    return S.parity_path(root, f[2], f[0])


def parityq(root, f):
    return S.parityq_path(root, q_target(f), f[0])


def hdr(f):
    return 8 * len(f[1])


def damage3(root, files):
    """One byte in a chunk of item A, a 4 KiB run in item B's P, one byte in item C's Q (mtimes kept).
    Returns ([(item index, repaired-list line without the byte count)], bytes a repair has to write)."""
    a, b, c = 2, 7, 3
    flip(chunk(root, files[a], 1), 10001)
    run0 = 3 * BLOCK + 100  # of the body: the run straddles two of its blocks
    p = parity(root, files[b])
    st = os.stat(p)
    with open(p, "r+b") as f:
        f.seek(hdr(files[b]) + run0)
        old = f.read(BLOCK)
        f.seek(hdr(files[b]) + run0)
        f.write(bytes(x ^ 0xFF for x in old))
    os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns))
    qlen = max(files[c][3])
    flip(parityq(root, files[c]), hdr(files[c]) + qlen - 1)  # the body's last byte: its block is clipped
    lines = [(a, f"{files[a][0]}\tdata\t{files[a][1][1]}"), (c, f"{files[c][0]}\tq\t{q_target(files[c])}"),
             (b, f"{files[b][0]}\tp\t{files[b][2]}")]
    clipped = qlen % BLOCK or BLOCK
    return sorted(lines), {a: BLOCK, b: 2 * BLOCK, c: clipped}


def repair_counts(st):
    return dict(none=st.none, done=st.done, dry=st.dry, policy=st.policy, unlocated=st.unlocated,
                changed=st.changed, failed=st.failed)


def read_lines(p):
    return S.read_file(p).decode().splitlines()


def test_clean_store(bcp, store, read_path):
    root, files, items = store
    before = snapshot(root)
    pl = bcp.Pipeline(io_threads=4)
    try:
        pl.set_q_windowed(True)
        st, res = pl.repair_q(root, NT, items, bcp.REPAIR_ALL, repaired_list=str(root) + ".repaired")
    finally:
        pl.close()
    assert [r.status for r in res] == [bcp.VERIFY_OK] * len(items)
    assert [r.repair for r in res] == [bcp.REPAIRED_NONE] * len(items)
    assert st.repair_launches == 0 and st.files_written == 0 and st.bytes_written == 0 and st.q.v.errors == 0
    assert repair_counts(st) == dict(none=len(items), done=0, dry=0, policy=0, unlocated=0, changed=0, failed=0)
    assert read_lines(str(root) + ".repaired") == []
    assert snapshot(root) == before


def _run_both(bcp, root, items, tmp, **kw):
    """verify_q just before, then repair_q: (verify stats, verify results, verify lists, repair stats, repair
    results, repair lists, repaired lines)."""
    names = [str(tmp / n) for n in ("bad0", "culprits0", "bad1", "culprits1", "repaired")]
    pl = bcp.Pipeline(io_threads=4)
    try:
        pl.set_q_windowed(True)
        vst, vres = pl.verify_q(root, NT, items, bad_list=names[0], culprit_list=names[1])
        rst, rres = pl.repair_q(root, NT, items, bad_list=names[2], culprit_list=names[3], repaired_list=names[4], **kw)
    finally:
        pl.close()
    return vst, vres, (read_lines(names[0]), read_lines(names[1])), rst, rres, (read_lines(names[2]),
                                                                                read_lines(names[3])), read_lines(names[4])


def _same_as_found(vres, rres):
    for v, r in zip(vres, rres):
        assert (v.status, v.q_state, v.culprit, v.target, v.first_bad, v.p_bad, v.q_bad) == \
               (r.status, r.q_state, r.culprit, r.target, r.first_bad, r.p_bad, r.q_bad)


def test_repair_all(bcp, store, tmp_path, read_path):
    root, files, items = store
    before = snapshot(root)
    want_lines, blocks = damage3(root, files)
    assert snapshot(root) != before
    vst, vres, vlists, rst, rres, rlists, repaired = _run_both(bcp, root, items, tmp_path, mode=bcp.REPAIR_ALL)
    assert vst.v.mismatch == 3 and len(vlists[0]) == 3 and len(vlists[1]) == 3
    assert rlists == vlists                       # the lists are those of a verify_q run made just before
    _same_as_found(vres, rres)
    assert rst.q.v.mismatch == 3 and rst.q.v.errors == 0
    bad = sorted(blocks)
    assert [i for i, r in enumerate(rres) if r.repair != bcp.REPAIRED_NONE] == bad
    assert all(rres[i].repair == bcp.REPAIRED_DONE for i in bad)
    assert [rres[i].bytes_fixed for i in bad] == [1, 1, BLOCK]  # items 2 (chunk byte), 3 (Q byte), 7 (P run)
    assert repair_counts(rst) == dict(none=len(items) - 3, done=3, dry=0, policy=0, unlocated=0, changed=0, failed=0)
    assert rst.files_written == 3 and rst.bytes_written == sum(blocks.values()) and 1 <= rst.repair_launches <= 3
    assert sorted(repaired) == sorted(f"{line}\t{blocks[i]}" for i, line in want_lines)
    assert snapshot(root) == before               # mtimes included
    pl = bcp.Pipeline(io_threads=4)
    try:
        pl.set_q_windowed(True)
        st, res = pl.verify_q(root, NT, items)
    finally:
        pl.close()
    assert [r.status for r in res] == [bcp.VERIFY_OK] * len(items) and st.v.errors == 0


def test_repair_parity_leaves_chunks_alone(bcp, store, tmp_path, read_path):
    root, files, items = store
    before = snapshot(root)
    want_lines, blocks = damage3(root, files)
    damaged = snapshot(root)
    vst, vres, vlists, rst, rres, rlists, repaired = _run_both(bcp, root, items, tmp_path, mode=bcp.REPAIR_PARITY)
    assert rlists == vlists
    _same_as_found(vres, rres)
    assert (rres[2].repair, rres[3].repair, rres[7].repair) == (bcp.REPAIRED_POLICY, bcp.REPAIRED_DONE,
                                                                bcp.REPAIRED_DONE)
    assert repair_counts(rst) == dict(none=len(items) - 3, done=2, dry=0, policy=1, unlocated=0, changed=0, failed=0)
    assert rst.files_written == 2 and rst.bytes_written == blocks[3] + blocks[7]
    after = snapshot(root)
    c = chunk(root, files[2], 1)
    assert after[c] == damaged[c] != before[c]    # the chunk byte-identical to the damaged one
    assert {k: v for k, v in after.items() if k != c} == {k: v for k, v in before.items() if k != c}


def test_dry_run_writes_nothing(bcp, store, tmp_path, read_path):
    root, files, items = store
    want_lines, blocks = damage3(root, files)
    damaged = snapshot(root)
    vst, vres, vlists, rst, rres, rlists, repaired = _run_both(bcp, root, items, tmp_path, mode=bcp.REPAIR_ALL,
                                                               dry_run=True)
    assert rlists == vlists and repaired == []
    assert [rres[i].repair for i in (2, 3, 7)] == [bcp.REPAIRED_DRY] * 3
    assert [rres[i].bytes_fixed for i in (2, 3, 7)] == [1, 1, BLOCK]
    assert repair_counts(rst) == dict(none=len(items) - 3, done=0, dry=3, policy=0, unlocated=0, changed=0, failed=0)
    assert rst.files_written == 0 and rst.bytes_written == 0 and rst.repair_launches >= 1
    assert snapshot(root) == damaged


def test_two_members_of_one_item(bcp, store, tmp_path):
    root, files, items = store
    before = snapshot(root)
    f = files[8]  # width 9
    flip(chunk(root, f, 0), 77)
    flip(chunk(root, f, 8), f[3][8] - 1)
    damaged = snapshot(root)
    *_, rst, rres, _, repaired = _run_both(bcp, root, items, tmp_path, mode=bcp.REPAIR_ALL, max_members=1)
    assert rres[8].repair == bcp.REPAIRED_POLICY and rres[8].culprit == bcp.CULPRIT_MANY and rst.policy == 1
    assert repaired == [] and rst.repair_launches == 0 and snapshot(root) == damaged
    *_, rst, rres, _, repaired = _run_both(bcp, root, items, tmp_path, mode=bcp.REPAIR_ALL, max_members=2)
    assert rres[8].repair == bcp.REPAIRED_DONE and rres[8].bytes_fixed == 2 and rst.done == 1
    assert rst.files_written == 2 and len(repaired) == 2 and rst.bytes_written == BLOCK + (f[3][8] % BLOCK or BLOCK)
    assert snapshot(root) == before


def test_what_must_not_be_repaired(bcp, store, tmp_path):
    root, files, items = store
    big, full, stale = 13, 12, 4
    flip(chunk(root, files[big], 0), 1000)        # windowed, under q_windowed: blamed, never repaired
    flip(chunk(root, files[full], 2), 11)         # every target taken: no Q, nobody named
    c = chunk(root, files[stale], 0)
    flip(c, 5, keep_mtime=False)                  # modified since the last round, by a user
    os.utime(c, (items[stale][1] + 10, items[stale][1] + 10))
    damaged = snapshot(root)
    vst, vres, vlists, rst, rres, rlists, repaired = _run_both(bcp, root, items, tmp_path, mode=bcp.REPAIR_ALL,
                                                               max_members=3)
    assert rlists == vlists and repaired == []
    _same_as_found(vres, rres)
    assert (rres[big].status, rres[big].q_state, rres[big].repair) == (bcp.VERIFY_MISMATCH, bcp.QSTATE_CHECKED,
                                                                       bcp.REPAIRED_UNLOCATED)
    assert (rres[full].status, rres[full].q_state, rres[full].repair) == (bcp.VERIFY_MISMATCH, bcp.QSTATE_NONE,
                                                                          bcp.REPAIRED_UNLOCATED)
    assert (rres[stale].status, rres[stale].repair) == (bcp.VERIFY_STALE, bcp.REPAIRED_NONE)
    assert repair_counts(rst) == dict(none=len(items) - 2, done=0, dry=0, policy=0, unlocated=2, changed=0, failed=0)
    assert rst.repair_launches == 0 and rst.files_written == 0 and rst.q.v.errors == 0
    assert snapshot(root) == damaged


def test_cli_parity_verify_repair(bcp, store, tmp_path):
    root, files, items = store
    before = snapshot(root)
    want_lines, blocks = damage3(root, files)
    db = str(tmp_path / "db")  # the CLI reads the database: the one these items make
    _write_db(bcp, db, items)
    repaired = str(tmp_path / "repaired")
    args = [bcp.BIN_PATH, "parity-verify", "--db", db, "--q", "--q-windowed"]
    r = subprocess.run(args + ["--repair", "all", "--dry-run", root, str(NT)], capture_output=True)
    assert r.returncode == 1, r.stdout + r.stderr          # a dry run's status is parity-verify --q's
    assert b"repair (all, dry run): 0 done, 3 dry" in r.stdout, r.stdout
    # parity mode: P and Q are repaired, the chunk is refused by the policy, so the store is still wrong
    r = subprocess.run(args + ["--repair", "parity", root, str(NT)], capture_output=True)
    assert r.returncode == 1, r.stdout + r.stderr
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 3 and " 3 mismatch, " in lines[0], r.stdout
    assert lines[1] == f"q files: {len(items) - 1} checked, 1 none, 0 bad; culprits: 1 data, 1 p, 1 q, 0 many"
    assert lines[2].startswith("repair (parity): 2 done, 0 dry, 1 policy, 0 unlocated, 0 changed, 0 failed; 2 files, "
                               f"{blocks[3] + blocks[7]} bytes written, ")
    # all: the chunk too; every mismatch ended DONE
    r = subprocess.run(args + ["--repair", "all", "--repaired", repaired, root, str(NT)], capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 3, r.stdout
    assert lines[0].startswith(f"verified {len(items)} items: {len(items) - 1} ok, 0 stale, 0 no parity, 0 wrong size, "
                               "1 mismatch, 0 skipped (0 refused), 0 errors, ")
    assert lines[1] == f"q files: {len(items) - 1} checked, 1 none, 0 bad; culprits: 1 data, 0 p, 0 q, 0 many"
    assert lines[2].startswith("repair (all): 1 done, 0 dry, 0 policy, 0 unlocated, 0 changed, 0 failed; 1 files, "
                               f"{blocks[2]} bytes written, 1 launches")
    assert read_lines(repaired) == [f"{line}\t{blocks[i]}" for i, line in want_lines if i == 2]
    assert snapshot(root) == before
    r = subprocess.run(args + [root, str(NT)], capture_output=True)
    assert r.returncode == 0 and len(r.stdout.decode().splitlines()) == 2, r.stdout + r.stderr


def _write_db(bcp, db, items):
    """A parity database holding exactly these items (the CLI's --db)."""
    os.makedirs(db)
    pdb = bcp.PDB(db)
    try:
        for path, ts, loc in items:
            pdb.set(path, ts, loc)
        pdb.sync()
    finally:
        pdb.close()
