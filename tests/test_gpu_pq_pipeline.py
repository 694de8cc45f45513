"""Q parity through the batched pipeline: Q files written beside byte-identical
P files (Pipeline.set_q_parity), and the rebuild of two lost targets
(Pipeline.rebuild2, bin/bcp parity-rebuild --also).  Expected Q bodies are
numpy's (tests/gf256.py); expected roles, counters and lists are computed here
from the items' locations."""
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bcp_store as S
import gf256 as G

pytestmark = pytest.mark.gpu
KiB, MiB = 1024, 1024 * 1024
SIZES = [0, 1, 4095, 64 * KiB + 5, 1 * MiB + 17]


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


def header(lens):
    return struct.pack(f"<{len(lens)}Q", *lens)


def tree(root, sub):
    """{path relative to root: (sha256, mtime_ns)} of every file under <root>/st*/<sub>."""
    out = {}
    for st in sorted(os.listdir(root)):
        top = os.path.join(root, st, sub)
        for d, _, names in os.walk(top):
            for n in names:
                p = os.path.join(d, n)
                out[os.path.relpath(p, root)] = (hashlib.sha256(S.read_file(p)).hexdigest(), os.stat(p).st_mtime_ns)
    return out


# ---------------------------------------------------------------------------
# gen
# ---------------------------------------------------------------------------
NT_GEN = 7


def gen_files(rng):
    files = []
    for i in range(36):
        width = i % 5 + 1
        holders, p = S.random_layout(rng, NT_GEN, width)
        lens = [SIZES[int(x)] for x in rng.integers(0, len(SIZES), size=width)]
        files.append((f"g/{i % 4}/c{i:02d}", holders, p, lens))
    for i in range(3):  # 6 holders + P: every target taken, no Q target
        holders, p = S.random_layout(rng, NT_GEN, 6)
        files.append((f"six/c{i}", holders, p, [SIZES[int(x)] for x in rng.integers(1, len(SIZES), size=6)]))
    files.append(("nop/a", [1, 2], S.NO_P, [4095, 1]))
    files.append(("empty/a", [], 3, []))                                    # no holders: both files are unlinked
    files.append(("big/a", [0, 2], 5, [11 * MiB + 3, 64 * KiB + 5]))        # windowed: P only
    return files


def test_gen_writes_q_files_and_the_same_p_files(bcp, oracle, tmp_path, read_path):
    root, plain = str(tmp_path / "q"), str(tmp_path / "plain")
    files = gen_files(np.random.default_rng(5))
    items, contents = S.populate(root, NT_GEN, files, seed=5)
    by_path = {f[0]: f for f in files}
    qt = {f[0]: G.q_target(S.with_p(sum(1 << h for h in f[1]), f[2]), NT_GEN) for f in files}
    assert qt["big/a"] >= 0 and qt["empty/a"] >= 0 and all(qt[f"six/c{i}"] == -1 for i in range(3))
    # stale files that a Q run has to remove
    for p in (S.parityq_path(root, qt["big/a"], "big/a"), S.parityq_path(root, qt["empty/a"], "empty/a"),
              S.parity_path(root, 3, "empty/a")):
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "wb").write(b"stale")
    shutil.copytree(root, plain)
    pl = bcp.Pipeline(slab_bytes=1 * MiB, io_threads=4)
    try:
        st0 = pl.run(plain, NT_GEN, items)
        assert pl.q_stats() == dict(written=0, no_target=0, windowed=0)
        pl.set_q_parity(True)
        st = pl.run(root, NT_GEN, items)
        assert pl.last_timing()["batches"] >= 3
        stats = pl.q_stats()
        assert st.errors == 0 and st0.errors == 0 and st.tasks == st0.tasks
        # P files: byte-identical to the run without Q
        p_q, p_plain = tree(root, "parity"), tree(plain, "parity")
        assert {k: v[0] for k, v in p_q.items()} == {k: v[0] for k, v in p_plain.items()} and len(p_q) == len(files) - 2
        assert not os.path.exists(S.parity_path(root, 3, "empty/a"))
        # Q files: exactly the eligible items', header + numpy's Q
        eligible = [f for f in files if f[1] and f[2] != S.NO_P and qt[f[0]] >= 0 and max(f[3]) <= bcp.WINDOW_BYTES]
        want = {os.path.relpath(S.parityq_path(root, qt[f[0]], f[0]), root): f for f in eligible}
        got = tree(root, "parityq")
        assert sorted(got) == sorted(want)
        for rel, f in want.items():
            chunks = contents[f[0]]
            body = G.q_sum(chunks, max(f[3]))
            assert S.read_file(os.path.join(root, rel)) == header(f[3]) + body.tobytes(), f[0]
        assert stats == dict(written=len(eligible), no_target=3, windowed=1)
        assert st.bytes_written == st0.bytes_written + sum(8 * len(f[3]) + max(f[3]) for f in eligible)
        # a run with Q off again leaves the Q files alone
        pl.set_q_parity(False)
        st2 = pl.run(root, NT_GEN, items)
        assert st2.errors == 0 and tree(root, "parityq") == got and pl.q_stats() == dict(written=0, no_target=0, windowed=0)
    finally:
        pl.close()
    assert by_path["nop/a"][2] == S.NO_P and not os.path.exists(S.parity_path(root, 0, "nop/a"))


# ---------------------------------------------------------------------------
# rebuild2
# ---------------------------------------------------------------------------
NT = 5
R_SIZES = [0, 1, 4095, 20000, 64 * KiB + 5]


def rebuild_files(rng):
    files = []
    for i in range(18):
        width = i % 3 + 1
        holders, p = S.random_layout(rng, NT, width)
        lens = [R_SIZES[int(x)] for x in rng.integers(0, len(R_SIZES), size=width)]
        files.append((f"r/{i % 3}/c{i:02d}", holders, p, lens))
    files.append(("r/wide", [0, 1, 2, 3], 4, [20000, 1, 4095, 300]))   # 4 holders + P: no Q target
    files.append(("r/nop", [0, 1], S.NO_P, [100, 200]))
    return files


def make_q_store(bcp, root, files, nt, seed):
    items, contents = S.populate(root, nt, files, seed=seed)
    pl = bcp.Pipeline(slab_bytes=1 * MiB, io_threads=4)
    try:
        pl.set_q_parity(True)
        st = pl.run(root, nt, items)
        assert st.errors == 0
    finally:
        pl.close()
    return sorted(items, key=lambda x: x[0].encode()), contents


def lose(root, targets):
    for t in targets:
        for sub in ("chunks", "parity", "parityq"):
            shutil.rmtree(os.path.join(root, f"st{t}", sub), ignore_errors=True)


def role(f, a, b, nt):
    """'skip', 'xor', 'q', 'pq' or 'lost' for item f when targets a and b are gone, and its lost holders."""
    path, holders, p, lens = f
    gone = [h for h in holders if h in (a, b)]
    if p == S.NO_P or not gone:
        return "skip", gone
    if len(gone) == 1 and p not in (a, b):
        return "xor", gone
    if G.q_target(S.with_p(sum(1 << h for h in holders), p), nt) < 0:
        return "lost", gone
    return ("pq" if len(gone) == 2 else "q"), gone


def counters(st2):
    return dict(xor=st2.xor_items, q=st2.q_items, pq=st2.pq_items, lost=st2.unrecoverable)


def test_rebuild2_every_pair_of_targets(bcp, oracle, tmp_path, read_path):
    base = str(tmp_path / "base")
    files = rebuild_files(np.random.default_rng(11))
    items, contents = make_q_store(bcp, base, files, NT, seed=11)
    by_path = {f[0]: f for f in files}
    order = [it[0] for it in items]
    pl = bcp.Pipeline(slab_bytes=1 * MiB, io_threads=4)
    seen = set()
    try:
        for a in range(NT):
            for b in range(a + 1, NT):
                root, ref = str(tmp_path / f"p{a}{b}"), str(tmp_path / f"x{a}{b}")
                shutil.copytree(base, root)
                lose(root, (a, b))
                shutil.copytree(root, ref)
                lost_list, corrupt = str(tmp_path / f"lost{a}{b}"), str(tmp_path / f"corrupt{a}{b}")
                st, st2 = pl.rebuild2(root, NT, b, a, items, corrupt_list=corrupt, lost_list=lost_list)
                roles = {f[0]: role(f, a, b, NT) for f in files}
                seen |= {r for r, _ in roles.values()}
                want = dict(xor=0, q=0, pq=0, lost=0)
                for r, _ in roles.values():
                    if r != "skip":
                        want[r] += 1
                assert st.errors == 0 and counters(st2) == want, (a, b)
                assert S.read_file(lost_list).decode().splitlines() == [p for p in order if roles[p][0] == "lost"]
                assert S.read_file(corrupt) == b""
                for path, (r, gone) in roles.items():
                    f = by_path[path]
                    for h in gone:
                        fn = S.chunk_path(root, h, path)
                        if r in ("skip", "lost"):
                            assert not os.path.exists(fn), (a, b, path, "written although " + r)
                        else:
                            assert S.read_file(fn) == contents[path][f[1].index(h)].tobytes(), (a, b, path, r, h)
                # nothing but those chunks appeared
                made = {os.path.relpath(S.chunk_path(root, h, path), root) for path, (r, gone) in roles.items()
                        if r in ("xor", "q", "pq") for h in gone}
                assert set(tree(root, "chunks")) - set(tree(ref, "chunks")) == made
                assert tree(root, "parity") == tree(ref, "parity") and tree(root, "parityq") == tree(ref, "parityq")
                # one lost holder with P present: the files Pipeline.rebuild writes
                for t in (a, b):
                    if any(r == "xor" and gone == [t] for r, gone in roles.values()):
                        one = str(tmp_path / f"one{a}{b}{t}")
                        shutil.copytree(ref, one)
                        pl.rebuild(one, NT, t, items)
                        for path, (r, gone) in roles.items():
                            if r == "xor" and gone == [t]:
                                assert S.read_file(S.chunk_path(root, t, path)) == S.read_file(S.chunk_path(one, t, path))
                        shutil.rmtree(one)
                for d in (root, ref):
                    shutil.rmtree(d)
    finally:
        pl.close()
    assert seen == {"skip", "xor", "q", "pq", "lost"}


def test_rebuild2_unusable_parity_files_and_the_corrupt_list(bcp, oracle, tmp_path, read_path):
    base = str(tmp_path / "base")
    files = [("d/pq", [0, 1, 2], 3, [70000, 5000, 300]),       # Q on target 4
             ("d/q", [0, 2], 1, [4095, 33000]),                # Q on target 3
             ("d/ok", [0, 1], 2, [5000, 64 * KiB + 5]),        # Q on target 3
             ("d/win", [0, 1], 2, [10 * MiB + 7, 100])]        # windowed: no Q file
    items, contents = make_q_store(bcp, base, files, NT, seed=12)
    ts = items[0][1]
    assert not os.path.exists(S.parityq_path(base, 3, "d/win"))
    pl = bcp.Pipeline(slab_bytes=1 * MiB, io_threads=4)

    def run(name, a, b, damage):
        root = str(tmp_path / name)
        shutil.copytree(base, root)
        lose(root, (a, b))
        damage(root)
        lost_list, corrupt = str(tmp_path / (name + ".lost")), str(tmp_path / (name + ".corrupt"))
        st, st2 = pl.rebuild2(root, NT, a, b, items, corrupt_list=corrupt, lost_list=lost_list)
        assert st.errors == 0
        return root, counters(st2), S.read_file(lost_list).decode().split(), S.read_file(corrupt).decode().split()

    def restored(root, path, holders):
        f = next(x for x in files if x[0] == path)
        return all(os.path.exists(S.chunk_path(root, h, path)) and
                   S.read_file(S.chunk_path(root, h, path)) == contents[path][f[1].index(h)].tobytes() for h in holders)

    try:
        # undamaged: targets 0 and 1 take two holders of d/pq, d/ok and d/win, and d/q's holder 0 and P
        root, c, lost, corrupt = run("clean", 0, 1, lambda r: None)
        assert c == dict(xor=0, q=1, pq=2, lost=1) and lost == ["d/win"] and corrupt == []
        assert restored(root, "d/pq", [0, 1]) and restored(root, "d/q", [0]) and restored(root, "d/ok", [0, 1])
        assert not os.path.exists(S.chunk_path(root, 0, "d/win"))

        # a truncated Q file
        def truncate(r):
            p = S.parityq_path(r, 4, "d/pq")
            os.truncate(p, os.path.getsize(p) - 1)
        root, c, lost, corrupt = run("short", 0, 1, truncate)
        assert c == dict(xor=0, q=1, pq=1, lost=2) and lost == ["d/pq", "d/win"]
        assert not os.path.exists(S.chunk_path(root, 0, "d/pq")) and not os.path.exists(S.chunk_path(root, 1, "d/pq"))
        assert restored(root, "d/ok", [0, 1])

        # P and Q headers that differ (both files still have a consistent size)
        def reheader(r):
            p = S.parityq_path(r, 4, "d/pq")
            data = bytearray(S.read_file(p))
            data[16:24] = struct.pack("<Q", 301)
            open(p, "wb").write(data)
        root, c, lost, corrupt = run("header", 0, 1, reheader)
        assert c == dict(xor=0, q=1, pq=1, lost=2) and lost == ["d/pq", "d/win"]
        assert not os.path.exists(S.chunk_path(root, 0, "d/pq"))

        # a missing Q file where only Q can help
        root, c, lost, corrupt = run("noq", 0, 1, lambda r: os.remove(S.parityq_path(r, 3, "d/q")))
        assert c == dict(xor=0, q=0, pq=2, lost=2) and lost == ["d/q", "d/win"]

        # a survivor modified after the item's timestamp: rebuilt, and on the corrupt list
        def touch(r):
            os.utime(S.chunk_path(r, 2, "d/pq"), (ts + 10, ts + 10))
        root, c, lost, corrupt = run("newer", 0, 1, touch)
        assert c == dict(xor=0, q=1, pq=2, lost=1) and corrupt == ["d/pq"] and restored(root, "d/pq", [0, 1])

        # the windowed item with one victim and P present is the plain rebuild
        root, c, lost, corrupt = run("win", 0, 4, lambda r: None)
        assert c == dict(xor=4, q=0, pq=0, lost=0) and lost == [] and restored(root, "d/win", [0])
    finally:
        pl.close()


def test_cli_gen_q_and_rebuild_also(bcp, oracle, tmp_path):
    rng = np.random.default_rng(41)
    root, nt = str(tmp_path / "store"), 6
    S.make_store(root, nt)
    data = {}
    for i in range(14):
        path = f"u{i % 2}/{i:02X}/c{i}"
        holders = sorted(int(x) for x in rng.choice(nt, size=int(rng.integers(1, 4)), replace=False))
        for h in holders:
            data[(h, path)] = S.synthetic_chunk(i * 13 + h, int(rng.integers(1, 200_000)))
            S.write_chunk(root, h, path, data[(h, path)])
    r = subprocess.run([bcp.BIN_PATH, "parity-gen", "--complete", "--q", root, str(nt)], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert len(tree(root, "parityq")) == 14 and len(tree(root, "parity")) == 14
    a, b = 1, 4
    lose(root, (a, b))
    lost = str(tmp_path / "lost")
    r = subprocess.run([bcp.BIN_PATH, "parity-rebuild", "--also", str(b), "--lost", lost, root, str(nt), str(a)],
                       capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert b"0 unrecoverable" in r.stdout and S.read_file(lost) == b""
    gone = [(h, path) for (h, path) in data if h in (a, b)]
    assert len(gone) >= 4
    for h, path in gone:
        assert S.read_file(S.chunk_path(root, h, path)) == data[(h, path)].tobytes(), (h, path)
