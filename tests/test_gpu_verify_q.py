"""The scrub with Q end to end (bcp_pipeline_verify_q, bin/bcp parity-verify
--q): a store written with Q parity is verified clean and with one defect per
item; verdicts, Q states, culprits, their storage targets, the counts and both
lists are exact, nothing under the store changes, and bcp_pipeline_verify gives
on the same damaged store what it always gave."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import bcp_store as S
import gf256 as G

pytestmark = pytest.mark.gpu
KiB, MiB = 1024, 1024 * 1024
NT = 16
WINDOWED = [10485760, 26214405]  # the smallest two-source case past the 10 MiB window


@pytest.fixture(autouse=True)
def gpu_fold(bcp, engine):
    bcp.set_xor_hook(None)
    yield
    bcp.task_shutdown()


@pytest.fixture(params=["copy", "direct"])
def read_path(request, monkeypatch):
    """Both read paths of the pipeline (AUTO resolves through BCP_PIPELINE_READ)."""
    monkeypatch.setenv("BCP_PIPELINE_READ", request.param)
    return request.param


def make_store(bcp, pl, root, seed=3, nitems=26):
    """The scrub tests' store -- widths 1..15, chunks of 64 KiB .. 3 MiB with unaligned lengths, one item
    with a chunk missing at generation time, two items past the window -- generated with Q on."""
    rng = np.random.default_rng(seed)
    files = []
    for i in range(nitems):
        width = i % 15 + 1
        holders, p = S.random_layout(rng, NT, width)
        hi = 3 * MiB if width <= 4 else 400 * KiB
        lens = [int(x) | 1 for x in np.exp(rng.uniform(np.log(64 * KiB), np.log(hi), size=width))]
        files.append((f"v/{i % 5}/c{i:02d}", holders, p, lens))
    files.append(("big/a", [0, 1], 4, list(WINDOWED)))
    files.append(("big/b", [1, 2, 3], 0, [11 * MiB + 3, 70 * KiB + 1, 12 * MiB + 5]))
    items, contents = S.populate(root, NT, files, seed=seed)
    missing = files[5]
    os.remove(S.chunk_path(root, missing[1][1], missing[0]))  # width 6: its second holder's chunk never existed
    contents[missing[0]][1] = np.zeros(0, np.uint8)
    pl.set_q_parity(True)
    st = pl.run(root, NT, items)
    pl.set_q_parity(False)
    assert st.errors == 0 and st.tasks == len(files)
    return files, items, contents


def q_target(f):
    return G.q_target(S.with_p(sum(1 << h for h in f[1]), f[2]), NT)


def has_q(f):
    return q_target(f) >= 0 and max(f[3]) <= 10 * MiB


def flip(path, offset, keep_mtime=True):
    st = os.stat(path)
    with open(path, "r+b") as f:
        f.seek(offset)
        b = f.read(1)
        f.seek(offset)
        f.write(bytes([b[0] ^ 0x5A]))
    if keep_mtime:
        os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))


def snapshot(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            out[p] = (hashlib.sha256(S.read_file(p)).hexdigest(), os.stat(p).st_mtime_ns)
    return out


def counts(st):
    return dict(ok=st.v.ok, stale=st.v.stale, no_parity=st.v.no_parity, size=st.v.size, mismatch=st.v.mismatch,
                skipped=st.v.skipped, q_checked=st.q_checked, q_none=st.q_none, q_bad=st.q_bad,
                data=st.culprit_data, p=st.culprit_p, q=st.culprit_q, many=st.culprit_many)


def test_clean_store_verifies_and_is_untouched(bcp, oracle, tmp_path, read_path):
    root = str(tmp_path)
    pl = bcp.Pipeline(io_threads=4)
    try:
        files, items, contents = make_store(bcp, pl, root)
        before = snapshot(root)
        st, res = pl.verify_q(root, NT, items)
        tm = pl.last_timing()
    finally:
        pl.close()
    assert [r.status for r in res] == [bcp.VERIFY_OK] * len(items)
    want_q = [bcp.QSTATE_CHECKED if has_q(f) else bcp.QSTATE_NONE for f in files]
    assert [r.q_state for r in res] == want_q
    assert want_q.count(bcp.QSTATE_NONE) == 3 and not has_q(files[14])  # two windowed, one with every target taken
    assert all(r.first_bad == 2 ** 64 - 1 and r.p_bad == 0 and r.q_bad == 0 and r.target == -1 and
               r.culprit == bcp.CULPRIT_NONE for r in res)
    assert st.v.errors == 0 and st.v.refused == 0 and st.v.items == len(items)
    assert counts(st) == dict(ok=len(items), stale=0, no_parity=0, size=0, mismatch=0, skipped=0,
                              q_checked=len(items) - 3, q_none=3, q_bad=0, data=0, p=0, q=0, many=0)
    # every chunk as the header has it, every P body, and the Q bodies of the checked items
    want = sum(sum(len(c) for c in contents[f[0]]) + max(len(c) for c in contents[f[0]]) * (2 if has_q(f) else 1)
               for f in files)
    assert st.v.bytes_read == want
    assert tm["batches"] >= 1 and tm["read_mode"] == {"copy": bcp.READ_COPY, "direct": bcp.READ_DIRECT}[read_path]
    assert snapshot(root) == before


def test_one_defect_per_item(bcp, oracle, tmp_path, read_path):
    root = str(tmp_path)
    pl = bcp.Pipeline(io_threads=4)
    try:
        files, items, contents = make_store(bcp, pl, root)
        # path -> (status, q_state, culprit, target, first_bad, p_bad, q_bad); p_only: bcp_pipeline_verify's status
        expect, p_only = {}, {}

        def chunk(i, k):
            return S.chunk_path(root, files[i][1][k], files[i][0])

        def parity(i):
            return S.parity_path(root, files[i][2], files[i][0])

        def parityq(i):
            assert has_q(files[i]), files[i]
            return S.parityq_path(root, q_target(files[i]), files[i][0])

        def hdr(i):
            return 8 * len(files[i][1])

        # a flipped chunk byte (mtime kept: silent corruption): the syndromes name the holder
        flip(chunk(2, 1), 60001)
        expect[files[2][0]] = (bcp.VERIFY_MISMATCH, bcp.QSTATE_CHECKED, bcp.CULPRIT_DATA, files[2][1][1], 60001, 1, 1)
        # the last byte of a P body
        m = max(files[7][3])
        flip(parity(7), hdr(7) + m - 1)
        expect[files[7][0]] = (bcp.VERIFY_MISMATCH, bcp.QSTATE_CHECKED, bcp.CULPRIT_P, files[7][2], m - 1, 1, 0)
        # a byte of a Q body: the P-only scrub cannot see it
        flip(parityq(3), hdr(3) + 100)
        expect[files[3][0]] = (bcp.VERIFY_MISMATCH, bcp.QSTATE_CHECKED, bcp.CULPRIT_Q, q_target(files[3]), 100, 0, 1)
        p_only[files[3][0]] = bcp.VERIFY_OK
        # a chunk byte and a P byte of one item: not a single-member fault
        flip(chunk(4, 0), 7000)
        flip(parity(4), hdr(4) + 300)
        expect[files[4][0]] = (bcp.VERIFY_MISMATCH, bcp.QSTATE_CHECKED, bcp.CULPRIT_MANY, -1, 300, 2, 1)
        # the last holder of the widest item with a Q file (position 13), last byte of its chunk
        assert len(files[13][1]) == 14
        flip(chunk(13, 13), files[13][3][13] - 1)
        expect[files[13][0]] = (bcp.VERIFY_MISMATCH, bcp.QSTATE_CHECKED, bcp.CULPRIT_DATA, files[13][1][13],
                                files[13][3][13] - 1, 1, 1)
        # a windowed item: the P check with its window, nobody named
        big = len(files) - 2
        assert files[big][0] == "big/a"
        flip(chunk(big, 0), 1000)
        changed = [c.copy() for c in contents["big/a"]]
        changed[0][1000] ^= 0x5A
        stored = np.frombuffer(oracle.gen_parity_file(contents["big/a"]), np.uint8)[16:]
        now = np.frombuffer(oracle.gen_parity_file(changed), np.uint8)[16:]
        w = np.flatnonzero(stored != now)
        assert w.size == 3
        expect["big/a"] = (bcp.VERIFY_MISMATCH, bcp.QSTATE_NONE, bcp.CULPRIT_MANY, -1, int(w[0]), 3, 0)
        # every target taken, so no Q by rule: as the P-only scrub
        flip(chunk(14, 2), 11)
        expect[files[14][0]] = (bcp.VERIFY_MISMATCH, bcp.QSTATE_NONE, bcp.CULPRIT_MANY, -1, 11, 1, 0)
        # Q file removed / truncated / with another header: the status is the P check's, the item is listed
        os.remove(parityq(6))
        expect[files[6][0]] = (bcp.VERIFY_OK, bcp.QSTATE_BAD, None, None, None, None, None)
        os.truncate(parityq(8), os.path.getsize(parityq(8)) - 1)
        flip(chunk(8, 0), 5)
        expect[files[8][0]] = (bcp.VERIFY_MISMATCH, bcp.QSTATE_BAD, bcp.CULPRIT_MANY, -1, 5, 1, 0)
        k = int(np.argmin(files[9][3]))
        qst = os.stat(parityq(9))
        with open(parityq(9), "r+b") as f:
            f.seek(8 * k)
            f.write(np.uint64(files[9][3][k] - 1).tobytes())
        os.utime(parityq(9), ns=(qst.st_atime_ns, qst.st_mtime_ns))
        expect[files[9][0]] = (bcp.VERIFY_OK, bcp.QSTATE_BAD, None, None, None, None, None)
        # the verdicts that come before any Q
        flip(chunk(10, 0), 5, keep_mtime=False)
        os.utime(chunk(10, 0), (items[10][1] + 10, items[10][1] + 10))
        expect[files[10][0]] = (bcp.VERIFY_STALE,) + (None,) * 6
        os.remove(parity(12))
        expect[files[12][0]] = (bcp.VERIFY_NO_PARITY,) + (None,) * 6
        with open(chunk(11, 0), "ab") as f:
            f.write(b"x")
        os.utime(chunk(11, 0), (items[11][1] - 10, items[11][1] - 10))
        expect[files[11][0]] = (bcp.VERIFY_SIZE,) + (None,) * 6
        ts = items[0][1]
        extra = [("nop/x", ts, S.with_p(0b110, S.NO_P)), ("none/y", ts, S.with_p(0, 3)), ("../x", ts, S.with_p(0b11, 2))]
        for path, _, _ in extra:
            expect[path] = (bcp.VERIFY_SKIPPED,) + (None,) * 6
        all_items = items[:6] + extra[:1] + items[6:20] + extra[1:] + items[20:]
        bad_list, culprit_list = str(tmp_path / "bad.txt"), str(tmp_path / "culprits.txt")
        before = snapshot(root)
        st, res = pl.verify_q(root, NT, all_items, bad_list=bad_list, culprit_list=culprit_list)
        assert pl.last_timing()["batches"] >= 1
        lists = S.read_file(bad_list).decode().splitlines(), S.read_file(culprit_list).decode().splitlines()
        os.remove(bad_list)
        os.remove(culprit_list)
        assert snapshot(root) == before
        # bcp_pipeline_verify on the same store: what it always said, with Q off and on
        st_p, res_p = pl.verify(root, NT, all_items)
        pl.set_q_parity(True)
        st_p2, res_p2 = pl.verify(root, NT, all_items)
        assert snapshot(root) == before
    finally:
        pl.close()
    by_path = {f[0]: f for f in files}
    kind = {bcp.CULPRIT_DATA: "data", bcp.CULPRIT_P: "p", bcp.CULPRIT_Q: "q", bcp.CULPRIT_MANY: "many"}
    want_bad, want_culprits = [], []
    for (path, _, _), r, rp, rp2 in zip(all_items, res, res_p, res_p2):
        if path not in expect:  # untouched
            expect[path] = (bcp.VERIFY_OK, bcp.QSTATE_CHECKED if has_q(by_path[path]) else bcp.QSTATE_NONE) + (None,) * 5
        status, q_state, culprit, target, first, p_bad, q_bad = expect[path]
        assert r.status == status, (path, r.status, status)
        if status in (bcp.VERIFY_OK, bcp.VERIFY_MISMATCH):
            assert r.q_state == q_state, (path, r.q_state, q_state)
        if status == bcp.VERIFY_MISMATCH:
            print(f"{path}: culprit {r.culprit} target {r.target} first_bad {r.first_bad} p_bad {r.p_bad} q_bad {r.q_bad}")
            assert (r.culprit, r.target, r.first_bad, r.p_bad, r.q_bad) == (culprit, target, first, p_bad, q_bad), path
            want_culprits.append(f"{path}\t{kind[culprit]}\t{target}")
        if status in (bcp.VERIFY_NO_PARITY, bcp.VERIFY_SIZE, bcp.VERIFY_MISMATCH) or q_state == bcp.QSTATE_BAD:
            want_bad.append(path)
        want_p = p_only.get(path, status)
        assert rp.status == rp2.status == want_p, (path, rp.status, rp2.status, want_p)
        if want_p == bcp.VERIFY_MISMATCH:
            assert (rp.first_bad, rp.bad_bytes) == (rp2.first_bad, rp2.bad_bytes) == (first, p_bad), path
    assert st.v.errors == 0 and st.v.refused == 1 and st.v.items == len(all_items)
    n_ok = sum(e[0] == bcp.VERIFY_OK for e in expect.values())
    assert counts(st) == dict(ok=n_ok, stale=1, no_parity=1, size=1, mismatch=8, skipped=3,
                              q_checked=n_ok + 8 - 3 - 3, q_none=3, q_bad=3, data=2, p=1, q=1, many=4)
    assert lists == (want_bad, want_culprits)
    assert len(want_bad) == 12 and len(want_culprits) == 8
    assert st_p.mismatch == st_p2.mismatch == 7 and st_p.ok == st_p2.ok == n_ok + 1 and st_p.errors == st_p2.errors == 0


def test_verdicts_land_on_their_items_across_batches_and_lanes(bcp, oracle, tmp_path):
    """Small slabs: many batches, most of them with both launches."""
    root = str(tmp_path)
    pl = bcp.Pipeline(slab_bytes=1 << 20, io_threads=4, nslots=2, ndevices=2)
    try:
        files, items, contents = make_store(bcp, pl, root)
        picks = [0, 14, 20, len(files) - 1]
        for i in picks:
            flip(S.chunk_path(root, files[i][1][0], files[i][0]), 4097 + i)
        st, res = pl.verify_q(root, NT, items)
        tm = pl.last_timing()
    finally:
        pl.close()
    assert tm["batches"] >= 4, tm
    assert [i for i, r in enumerate(res) if r.status != bcp.VERIFY_OK] == picks
    for i in picks:
        r = res[i]
        assert (r.status, r.first_bad) == (bcp.VERIFY_MISMATCH, 4097 + i)
        if has_q(files[i]):
            assert (r.q_state, r.culprit, r.target, r.p_bad, r.q_bad) == (bcp.QSTATE_CHECKED, bcp.CULPRIT_DATA,
                                                                          files[i][1][0], 1, 1)
        else:
            assert (r.q_state, r.culprit, r.target, r.q_bad) == (bcp.QSTATE_NONE, bcp.CULPRIT_MANY, -1, 0)
    assert st.v.mismatch == 4 and st.v.ok == len(items) - 4 and st.v.errors == 0
    assert (st.culprit_data, st.culprit_many) == (2, 2)


def test_cli_parity_verify_q(bcp, oracle, tmp_path):
    rng = np.random.default_rng(31)
    root, nt = str(tmp_path / "store"), 6
    S.make_store(root, nt)
    files = {}
    for i in range(12):
        path = f"u{i % 2}/{i:02X}/c{i}"
        holders = sorted(int(x) for x in rng.choice(nt, size=int(rng.integers(1, nt - 1)), replace=False))
        for h in holders:
            S.write_chunk(root, h, path, S.synthetic_chunk(i * 13 + h, int(rng.integers(1, 300_000))))
        files[path] = holders
    r = subprocess.run([bcp.BIN_PATH, "parity-gen", "--complete", "--q", root, str(nt)], capture_output=True)
    assert r.returncode == 0, r.stderr
    culprits = str(tmp_path / "culprits")
    r = subprocess.run([bcp.BIN_PATH, "parity-verify", "--q", "--culprits", culprits, root, str(nt)], capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 2 and lines[0].startswith("verified 12 items: 12 ok, 0 stale"), r.stdout
    assert lines[1] == "q files: 12 checked, 0 none, 0 bad; culprits: 0 data, 0 p, 0 q, 0 many"
    assert S.read_file(culprits) == b""
    # without --q: the one line the command always printed
    r = subprocess.run([bcp.BIN_PATH, "parity-verify", root, str(nt)], capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = r.stdout.decode().splitlines()
    assert len(plain) == 1 and plain[0].startswith("verified 12 items: 12 ok, 0 stale, 0 no parity, 0 wrong size, "
                                                   "0 mismatch, 0 skipped (0 refused), 0 errors, ")
    assert plain[0].endswith(" MiB read") and b"q files" not in r.stdout
    path = "u1/03/c3"
    flip(S.chunk_path(root, files[path][-1], path), 0)
    bad = str(tmp_path / "bad")
    r = subprocess.run([bcp.BIN_PATH, "parity-verify", "--read", "copy", "--bad", bad, "--q", "--culprits", culprits,
                        root, str(nt)], capture_output=True)
    assert r.returncode == 1, r.stdout + r.stderr
    assert b"11 ok" in r.stdout and b"1 mismatch" in r.stdout, r.stdout
    assert b"q files: 12 checked, 0 none, 0 bad; culprits: 1 data, 0 p, 0 q, 0 many" in r.stdout, r.stdout
    assert S.read_file(bad).decode().splitlines() == [path]
    assert S.read_file(culprits).decode().splitlines() == [f"{path}\tdata\t{files[path][-1]}"]
