"""The parity scrub end to end (bcp_pipeline_verify, bin/bcp parity-verify):
stores written by the batched pipeline are verified on the device, clean and
with one defect per item; verdicts, counts and the bad list are exact, and the
verify changes nothing under the store."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import bcp_store as S

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


def make_store(bcp, root, seed=3, nitems=26):
    """Widths 1..15, chunks of 64 KiB .. 3 MiB with unaligned lengths, one item
    with a chunk missing at generation time, two items past the window."""
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
    st = bcp.pipeline_gen(root, NT, items, slab_bytes=64 << 20, io_threads=4)
    assert st.errors == 0 and st.tasks == len(files)
    return files, items, contents


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
    return dict(ok=st.ok, stale=st.stale, no_parity=st.no_parity, size=st.size, mismatch=st.mismatch,
                skipped=st.skipped)


def test_clean_store_verifies_and_is_untouched(bcp, oracle, tmp_path, read_path):
    root = str(tmp_path)
    files, items, contents = make_store(bcp, root)
    before = snapshot(root)
    pl = bcp.Pipeline(io_threads=4)
    try:
        st, res = pl.verify(root, NT, items)
        tm = pl.last_timing()
    finally:
        pl.close()
    assert [r.status for r in res] == [bcp.VERIFY_OK] * len(items)
    assert all(r.first_bad == 2 ** 64 - 1 and r.bad_bytes == 0 for r in res)
    assert st.errors == 0 and st.refused == 0 and st.items == len(items)
    assert counts(st) == dict(ok=len(items), stale=0, no_parity=0, size=0, mismatch=0, skipped=0)
    # every chunk as the header has it, and every parity body
    want = sum(sum(len(c) for c in contents[f[0]]) + max(len(c) for c in contents[f[0]]) for f in files)
    assert st.bytes_read == want
    assert tm["batches"] >= 1 and tm["read_mode"] == {"copy": bcp.READ_COPY, "direct": bcp.READ_DIRECT}[read_path]
    assert snapshot(root) == before


def test_one_defect_per_item(bcp, oracle, tmp_path, read_path):
    root = str(tmp_path)
    files, items, contents = make_store(bcp, root)
    by_path = {f[0]: f for f in files}
    expect = {}  # path -> (status, first_bad or None, bad_bytes or None)

    def chunk(i, k):
        return S.chunk_path(root, files[i][1][k], files[i][0])

    def parity(i):
        return S.parity_path(root, files[i][2], files[i][0])

    # a flipped byte in a chunk (mtime kept: silent corruption, not a modification)
    flip(chunk(2, 1), 60001)
    expect[files[2][0]] = (bcp.VERIFY_MISMATCH, 60001, 1)
    # the last byte of a parity body
    n, m = len(files[7][1]), max(files[7][3])
    flip(parity(7), 8 * n + m - 1)
    expect[files[7][0]] = (bcp.VERIFY_MISMATCH, m - 1, 1)
    # a chunk byte whose window is replayed: big/a's first source is exactly one window long
    big = len(files) - 2
    assert files[big][0] == "big/a"
    flip(chunk(big, 0), 1000)
    changed = [c.copy() for c in contents["big/a"]]
    changed[0][1000] ^= 0x5A
    stored = np.frombuffer(oracle.gen_parity_file(contents["big/a"]), np.uint8)[16:]
    now = np.frombuffer(oracle.gen_parity_file(changed), np.uint8)[16:]
    w = np.flatnonzero(stored != now)
    assert w.size == 3 and int(w[1]) == 1000 + WINDOWED[0]  # the flipped byte and its two replays
    expect["big/a"] = (bcp.VERIFY_MISMATCH, int(w[0]), int(w.size))
    # a size in a parity header changed: not the largest -> SIZE; the largest -> the file size no longer fits
    for i, largest in ((8, False), (9, True)):
        lens = files[i][3]
        k = int(np.argmax(lens)) if largest else int(np.argmin(lens))
        with open(parity(i), "r+b") as f:
            f.seek(8 * k)
            f.write(np.uint64(lens[k] + 1).tobytes())
        expect[files[i][0]] = (bcp.VERIFY_NO_PARITY if largest else bcp.VERIFY_SIZE, None, None)
    os.truncate(chunk(10, 3), files[10][3][3] - 100)
    expect[files[10][0]] = (bcp.VERIFY_SIZE, None, None)
    os.remove(chunk(11, 0))
    expect[files[11][0]] = (bcp.VERIFY_SIZE, None, None)
    os.remove(parity(12))
    expect[files[12][0]] = (bcp.VERIFY_NO_PARITY, None, None)
    os.truncate(parity(13), os.path.getsize(parity(13)) - 1)
    expect[files[13][0]] = (bcp.VERIFY_NO_PARITY, None, None)
    # modified after the item's timestamp: expected in a delayed scheme
    flip(chunk(14, 0), 5, keep_mtime=False)
    os.utime(chunk(14, 0), (items[14][1] + 10, items[14][1] + 10))
    expect[files[14][0]] = (bcp.VERIFY_STALE, None, None)
    ts = items[0][1]
    extra = [("nop/x", ts, S.with_p(0b110, S.NO_P)), ("none/y", ts, S.with_p(0, 3)),
             ("../x", ts, S.with_p(0b11, 2))]
    for path, _, _ in extra:
        expect[path] = (bcp.VERIFY_SKIPPED, None, None)
    all_items = items[:6] + extra[:1] + items[6:20] + extra[1:] + items[20:]
    bad_list = str(tmp_path / "bad.txt")
    pl = bcp.Pipeline(io_threads=4)
    try:
        st, res = pl.verify(root, NT, all_items, bad_list=bad_list)
    finally:
        pl.close()
    names = {bcp.VERIFY_OK: "OK", bcp.VERIFY_STALE: "STALE", bcp.VERIFY_NO_PARITY: "NO_PARITY",
             bcp.VERIFY_SIZE: "SIZE", bcp.VERIFY_MISMATCH: "MISMATCH", bcp.VERIFY_SKIPPED: "SKIPPED"}
    want_bad = []
    for (path, _, _), r in zip(all_items, res):
        status, first, nbad = expect.get(path, (bcp.VERIFY_OK, None, None))
        assert r.status == status, (path, names[r.status], names[status], by_path.get(path))
        if status == bcp.VERIFY_MISMATCH:
            assert (r.first_bad, r.bad_bytes) == (first, nbad), path
            print(f"{path}: first_bad {r.first_bad} bad_bytes {r.bad_bytes}")
        if status in (bcp.VERIFY_NO_PARITY, bcp.VERIFY_SIZE, bcp.VERIFY_MISMATCH):
            want_bad.append(path)
    assert st.errors == 0 and st.refused == 1 and st.items == len(all_items)
    assert counts(st) == dict(ok=len(all_items) - len(expect), stale=1, no_parity=3, size=3, mismatch=3, skipped=3)
    assert S.read_file(bad_list).decode().splitlines() == want_bad
    assert len(want_bad) == 9
    assert not os.path.exists(os.path.join(root, "st2", "x")) and not os.path.exists(parity(12))


def test_verdicts_land_on_their_items_across_batches_and_lanes(bcp, oracle, tmp_path, read_path):
    root = str(tmp_path)
    files, items, contents = make_store(bcp, root)
    picks = [0, len(files) // 2, len(files) - 1]
    for i in picks:
        flip(S.chunk_path(root, files[i][1][0], files[i][0]), 4097 + i)
    pl = bcp.Pipeline(slab_bytes=1 << 20, io_threads=4, nslots=2, ndevices=2)
    try:
        st, res = pl.verify(root, NT, items)
        tm = pl.last_timing()
    finally:
        pl.close()
    assert tm["batches"] >= 4, tm
    assert [i for i, r in enumerate(res) if r.status != bcp.VERIFY_OK] == picks
    for i in picks:
        assert (res[i].status, res[i].first_bad) == (bcp.VERIFY_MISMATCH, 4097 + i)
    assert res[picks[0]].bad_bytes == res[picks[1]].bad_bytes == 1
    assert st.mismatch == 3 and st.ok == len(items) - 3 and st.errors == 0


def test_clean_verdict_means_the_rebuild_works(bcp, oracle, tmp_path, read_path):
    root = str(tmp_path)
    files, items, contents = make_store(bcp, root)
    pl = bcp.Pipeline(io_threads=4)
    try:
        st, res = pl.verify(root, NT, items)
        assert st.ok == len(items) and st.errors == 0
        victim, lost = 1, {}
        for (path, holders, p, lens) in files:
            if victim in holders and os.path.exists(S.chunk_path(root, victim, path)):
                lost[path] = S.read_file(S.chunk_path(root, victim, path))
                os.remove(S.chunk_path(root, victim, path))
        assert len(lost) >= 3
        rst = pl.rebuild(root, NT, victim, sorted(items, key=lambda x: x[0].encode()))
        assert rst.errors == 0
        for path, data in lost.items():
            assert S.read_file(S.chunk_path(root, victim, path)) == data, path
    finally:
        pl.close()


def test_cli_parity_verify(bcp, oracle, tmp_path):
    rng = np.random.default_rng(31)
    root, nt = str(tmp_path / "store"), 6
    S.make_store(root, nt)
    files = {}
    for i in range(12):
        path = f"u{i % 2}/{i:02X}/c{i}"
        holders = sorted(int(x) for x in rng.choice(nt, size=int(rng.integers(1, nt)), replace=False))
        for h in holders:
            S.write_chunk(root, h, path, S.synthetic_chunk(i * 13 + h, int(rng.integers(1, 300_000))))
        files[path] = holders
    r = subprocess.run([bcp.BIN_PATH, "parity-gen", "--complete", root, str(nt)], capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([bcp.BIN_PATH, "parity-verify", root, str(nt)], capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert b"verified 12 items: 12 ok, 0 stale" in r.stdout, r.stdout
    path = "u1/03/c3"
    flip(S.chunk_path(root, files[path][0], path), 0)
    bad = str(tmp_path / "bad")
    r = subprocess.run([bcp.BIN_PATH, "parity-verify", "--read", "copy", "--bad", bad, root, str(nt)],
                       capture_output=True)
    assert r.returncode == 1, r.stdout + r.stderr
    assert b"11 ok" in r.stdout and b"1 mismatch" in r.stdout, r.stdout
    assert S.read_file(bad).decode().splitlines() == [path]
    r = subprocess.run([bcp.BIN_PATH, "parity-verify", "--frobnicate", root, str(nt)], capture_output=True)
    assert r.returncode == 1 and b"usage:" in r.stderr and b"parity-verify" in r.stderr
