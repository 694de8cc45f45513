"""Q parity for items past the 10 MiB window through the batched pipeline
(Pipeline.set_q_windowed): Q files over the replayed streams beside
byte-identical P files, the rebuild of two lost targets, the scrub with Q --
and, with the switch off, the same store and calls with the results they have
always had.  Expected Q bodies are numpy's over tests/pq_window.py's replayed
streams."""
import os
import shutil
import struct

import numpy as np
import pytest

import bcp_store as S
import gf256 as G
from pq_window import q_win, replayed_places

pytestmark = pytest.mark.gpu
KiB, MiB = 1024, 1024 * 1024
WIN = 10 * MiB
NT = 6
FILES = [("w/kat4", [0, 1], 2, [10485760, 26214405]),
         ("w/three", [0, 1, 2], 3, [11 * MiB + 3, 64 * KiB + 5, 10 * MiB]),
         ("s/a", [1, 3], 4, [4095, 64 * KiB + 5]),
         ("s/b", [0, 2, 4], 5, [1 * MiB + 17, 0, 20000])]
WINDOWED = ["w/kat4", "w/three"]


@pytest.fixture(autouse=True)
def gpu_fold(bcp, engine):
    bcp.set_xor_hook(None)
    yield
    bcp.task_shutdown()


def header(lens):
    return struct.pack(f"<{len(lens)}Q", *lens)


def q_target(f):
    return G.q_target(S.with_p(sum(1 << h for h in f[1]), f[2]), NT)


def files_under(root, sub):
    out = {}
    for st in sorted(os.listdir(root)):
        for d, _, names in os.walk(os.path.join(root, st, sub)):
            for n in names:
                p = os.path.join(d, n)
                out[os.path.relpath(p, root)] = S.read_file(p)
    return out


def lose(root, targets):
    for t in targets:
        for sub in ("chunks", "parity", "parityq"):
            shutil.rmtree(os.path.join(root, f"st{t}", sub), ignore_errors=True)


def flip(path, offset):
    st = os.stat(path)
    with open(path, "r+b") as f:
        f.seek(offset)
        b = f.read(1)
        f.seek(offset)
        f.write(bytes([b[0] ^ 0x5A]))
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))


@pytest.fixture(scope="module")
def store(bcp, engine, tmp_path_factory):
    """The store after a run with Q and the switch (base), the same chunks after a run without Q (plain), and
    the reference Q files; made once, every test works on a copy."""
    top = tmp_path_factory.mktemp("qwin")
    base, plain = str(top / "base"), str(top / "plain")
    items, contents = S.populate(base, NT, FILES, seed=21)
    items = sorted(items, key=lambda x: x[0].encode())
    assert all(q_target(f) >= 0 for f in FILES)
    shutil.copytree(base, plain)
    pl = bcp.Pipeline(io_threads=4)
    try:
        st0 = pl.run(plain, NT, items)
        pl.set_q_parity(True)
        pl.set_q_windowed(True)
        st = pl.run(base, NT, items)
        stats = pl.q_stats()
    finally:
        pl.close()
    assert st0.errors == 0 and st.errors == 0
    want_q = {os.path.relpath(S.parityq_path(base, q_target(f), f[0]), base):
              header(f[3]) + q_win(contents[f[0]], WIN if max(f[3]) > WIN else 0, max(f[3])).tobytes() for f in FILES}
    return dict(base=base, plain=plain, items=items, contents=contents, stats=stats, want_q=want_q, top=top)


def test_run_writes_q_for_windowed_items_and_the_same_p(bcp, store):
    assert files_under(store["base"], "parity") == files_under(store["plain"], "parity")
    assert len(files_under(store["base"], "parity")) == len(FILES)
    got = files_under(store["base"], "parityq")
    assert sorted(got) == sorted(store["want_q"])
    for rel, want in store["want_q"].items():
        assert len(got[rel]) == len(want), rel
        if got[rel] != want:
            a, b = np.frombuffer(got[rel], np.uint8), np.frombuffer(want, np.uint8)
            w = np.flatnonzero(a != b)
            raise AssertionError(f"{rel}: {w.size} bytes differ, first at file offset {int(w[0])}")
    assert store["stats"] == dict(written=len(FILES), no_target=0, windowed=0)
    assert files_under(store["plain"], "parityq") == {}


def restored(root, contents, path, holders):
    f = next(x for x in FILES if x[0] == path)
    return all(os.path.exists(S.chunk_path(root, h, path)) and
               S.read_file(S.chunk_path(root, h, path)) == contents[path][f[1].index(h)].tobytes() for h in holders)


def rebuild2(bcp, store, name, a, b, windowed):
    root = str(store["top"] / name)
    shutil.copytree(store["base"], root)
    lose(root, (a, b))
    lost_list = str(store["top"] / (name + ".lost"))
    pl = bcp.Pipeline(io_threads=4)
    try:
        pl.set_q_windowed(windowed)
        st, st2 = pl.rebuild2(root, NT, a, b, store["items"], lost_list=lost_list)
    finally:
        pl.close()
    assert st.errors == 0
    return root, dict(xor=st2.xor_items, q=st2.q_items, pq=st2.pq_items, lost=st2.unrecoverable), \
        S.read_file(lost_list).decode().split()


def test_rebuild2_two_holders_of_windowed_items(bcp, store):
    # targets 0 and 1: both holders of w/kat4, two of w/three's three; one holder each of s/a and s/b, P present
    root, c, lost = rebuild2(bcp, store, "r01", 0, 1, True)
    assert c == dict(xor=2, q=0, pq=2, lost=0) and lost == []
    for path in ("w/kat4", "w/three"):
        assert restored(root, store["contents"], path, [0, 1]), path
    assert restored(root, store["contents"], "s/a", [1]) and restored(root, store["contents"], "s/b", [0])
    shutil.rmtree(root)


def test_rebuild2_one_holder_and_p_of_a_windowed_item(bcp, store):
    # targets 2 and 3: w/three loses holder 2 (10 MiB) and its P; w/kat4 only its P (skipped); s/a and s/b a holder
    root, c, lost = rebuild2(bcp, store, "r23", 2, 3, True)
    assert c == dict(xor=2, q=1, pq=0, lost=0) and lost == []
    assert restored(root, store["contents"], "w/three", [2])
    assert restored(root, store["contents"], "s/a", [3]) and restored(root, store["contents"], "s/b", [2])
    shutil.rmtree(root)
    # targets 1 and 3: the 64 KiB + 5 member (replayed into the second window) and P
    root, c, lost = rebuild2(bcp, store, "r13", 1, 3, True)
    assert c["q"] == 1 and c["lost"] == 0 and lost == []
    assert restored(root, store["contents"], "w/three", [1]) and restored(root, store["contents"], "w/kat4", [1])
    shutil.rmtree(root)


def verify_q(bcp, root, items, windowed):
    pl = bcp.Pipeline(io_threads=4)
    try:
        pl.set_q_windowed(windowed)
        st, res = pl.verify_q(root, NT, items)
    finally:
        pl.close()
    assert st.v.errors == 0
    return st, {it[0]: r for it, r in zip(items, res)}


def test_verify_q_checks_windowed_items_and_names_the_culprit(bcp, store):
    root = str(store["top"] / "v")
    shutil.copytree(store["base"], root)
    st, res = verify_q(bcp, root, store["items"], True)
    assert all(r.status == bcp.VERIFY_OK and r.q_state == bcp.QSTATE_CHECKED for r in res.values())
    assert st.q_checked == len(FILES) and st.q_none == 0 and st.q_bad == 0
    # one byte of w/three's 64 KiB + 5 chunk (holder 1): it is replayed into the second window too
    flip(S.chunk_path(root, 1, "w/three"), 60001)
    places = replayed_places(64 * KiB + 5, WIN, 11 * MiB + 3, 60001)
    assert places == [60001, 60001 + WIN]
    st, res = verify_q(bcp, root, store["items"], True)
    r = res["w/three"]
    assert (r.status, r.q_state, r.culprit, r.target) == (bcp.VERIFY_MISMATCH, bcp.QSTATE_CHECKED, bcp.CULPRIT_DATA, 1)
    assert (r.first_bad, r.p_bad, r.q_bad) == (60001, 2, 2)
    assert all(v.status == bcp.VERIFY_OK for k, v in res.items() if k != "w/three")
    # the switch off: the windowed items have no Q by rule, the P check alone names nobody
    st, res = verify_q(bcp, root, store["items"], False)
    r = res["w/three"]
    assert (r.status, r.q_state, r.culprit, r.target) == (bcp.VERIFY_MISMATCH, bcp.QSTATE_NONE, bcp.CULPRIT_MANY, -1)
    assert (r.first_bad, r.p_bad, r.q_bad) == (60001, 2, 0)
    assert (res["w/kat4"].status, res["w/kat4"].q_state) == (bcp.VERIFY_OK, bcp.QSTATE_NONE)
    assert all(res[p].q_state == bcp.QSTATE_CHECKED for p in ("s/a", "s/b"))
    shutil.rmtree(root)


def test_switch_off_behaves_as_before(bcp, store):
    # rebuild2 over the store that has the Q files: windowed items that need Q are unrecoverable
    root, c, lost = rebuild2(bcp, store, "off01", 0, 1, False)
    assert c == dict(xor=2, q=0, pq=0, lost=2) and lost == WINDOWED
    assert not os.path.exists(S.chunk_path(root, 0, "w/kat4")) and not os.path.exists(S.chunk_path(root, 1, "w/three"))
    shutil.rmtree(root)
    # one holder lost with P present stays the plain rebuild, switch on or off
    for windowed in (False, True):
        root, c, lost = rebuild2(bcp, store, f"off05{int(windowed)}", 0, 5, windowed)
        assert c == dict(xor=2, q=1, pq=0, lost=0) and lost == []     # s/b: holder 0 and P = 5
        assert restored(root, store["contents"], "w/kat4", [0]) and restored(root, store["contents"], "w/three", [0])
        shutil.rmtree(root)
    # a run with Q and without the switch removes the windowed items' Q files and leaves the rest as it was
    root = str(store["top"] / "offrun")
    shutil.copytree(store["base"], root)
    pl = bcp.Pipeline(io_threads=4)
    try:
        pl.set_q_parity(True)
        st = pl.run(root, NT, store["items"])
        assert st.errors == 0 and pl.q_stats() == dict(written=2, no_target=0, windowed=2)
        pl.set_q_parity(False)      # the switch alone does nothing
        pl.set_q_windowed(True)
        st = pl.run(root, NT, store["items"])
        assert st.errors == 0 and pl.q_stats() == dict(written=0, no_target=0, windowed=0)
    finally:
        pl.close()
    want = {k: v for k, v in store["want_q"].items() if not any(k.endswith(w) for w in WINDOWED)}
    assert files_under(root, "parityq") == want
    assert files_under(root, "parity") == files_under(store["plain"], "parity")
    shutil.rmtree(root)
