"""The repair form of the P + Q kernel over window replay
(bcp_pq_repair_stripes_win_async) against the phase-by-phase oracle of
tests/pq_repair_window.py: the full six-field record and every byte of every
member, for both tile sizes (desc_vecs_per_thread 4 and 8).

W = 32 KiB and the lengths are pq_window.LISTS', so a stripe is a few hundred
KiB at most.  Every source and body is an upload of its own between random
non-zero poison (tests/devbuf.py); MARGIN bytes of that poison on either side
are read back before and after the launches and must not have changed -- a
store one byte before a member or one byte past len_k or out_len shows -- and
Dev.free reads every guard back.  Around each repair the windowed check form
runs over the same buffers: before it, for the state as found; after it, for
what the oracle says is left."""
import errno

import numpy as np
import pytest

import gf256 as G
import pq_repair_window as R
from devbuf import FILL, Dev
from pq_window import LISTS, W, chunks_of, p_win, q_win, replayed_places

pytestmark = pytest.mark.gpu
VECS = (4, 8)
CLEAN6 = (2 ** 64 - 1, 0, 0, 0, 0, 0)
CLEAN4 = (2 ** 64 - 1, 0, 0, 0)
BAD_P, BAD_Q, NOWHERE, ALL = R.BAD_P, R.BAD_Q, R.NOWHERE, R.ALL
FLIP = 0x5A
MARGIN = 64  # bytes of an upload's poison read back on either side (devbuf.POISON is 256)


@pytest.fixture
def dev(engine, queue):
    d = Dev(engine, queue)
    yield d
    d.free()


@pytest.fixture
def tuned(engine):
    """Set engine options for one test; the defaults come back afterwards."""
    saved = {}

    def set_option(key, value):
        saved.setdefault(key, engine.option(key))
        engine.option(key, value)

    yield set_option
    for k, v in saved.items():
        engine.option(k, v)


def flipped(a, at, x=FLIP):
    b = np.array(a, dtype=np.uint8, copy=True)
    b[at] ^= x
    return b


def blame(p, q, k, j, x=FLIP):
    """P and Q altered together at stream offset j so that the syndromes name data position k there."""
    return flipped(p, j, x), flipped(q, j, int(G.mul(np.uint8(x), np.uint8(G.gpow(k)))))


def stripe(lens, seed, window=W, none=()):
    """Pristine (chunks, p, q, out_len): chunks[k] is None (the source (0, 0)) for k in `none`."""
    chunks = [None if k in none else c for k, c in enumerate(chunks_of(lens, seed))]
    n = max(lens)
    return chunks, p_win(chunks, window, n), q_win(chunks, window, n), n


class Batch:
    """Stripes of one launch, every source and body an upload of its own."""

    def __init__(self):
        self.stripes = []

    def add(self, chunks, p, q, out_len, window=W, allow=ALL):
        i = len(self.stripes)
        self.stripes.append(dict(chunks=[None if c is None else np.array(c, dtype=np.uint8, copy=True) for c in chunks],
                                 p=np.array(p, dtype=np.uint8, copy=True), q=np.array(q, dtype=np.uint8, copy=True),
                                 out_len=out_len, window=window, allow=allow,
                                 pads=[(2 * (i + 3 * k) + 1) % 16 for k in range(len(chunks))],
                                 p_pad=(2 * i + 3) % 16, q_pad=(6 * i + 5) % 16))
        return i

    def run(self, engine, dev, queue):
        """Upload; check, repair, check; read everything back and compare it with the oracle.
        Returns (records, the check's records before, the oracle's records, form, launches)."""
        ups, where = [], []
        for s in self.stripes:
            idx = []
            for c, pad in zip(s["chunks"], s["pads"]):
                idx.append(None if c is None else len(ups))
                if c is not None:
                    ups.append((c, pad))
            where.append((idx, len(ups), len(ups) + 1))
            ups += [(s["p"], s["p_pad"]), (s["q"], s["q_pad"])]
        addrs = dev.put_many(ups)
        descs, sources, qb, allow = [], [], [], []
        for s, (idx, ip, iq) in zip(self.stripes, where):
            first = len(sources)
            sources += [(0, 0) if i is None else (addrs[i], len(ups[i][0])) for i in idx]
            descs.append((addrs[ip], s["out_len"], first, len(idx), s["window"]))
            qb.append(addrs[iq])
            allow.append(s["allow"])
        n = len(self.stripes)

        def snapshot():
            got = [np.empty(len(a) + 2 * MARGIN, np.uint8) for a, _ in ups]
            for g, ptr in zip(got, addrs):
                queue.d2h(g, ptr - MARGIN, g.size)
            queue.sync()
            return got

        before_img = snapshot()
        res0, res, res2 = dev.alloc(32 * n, fill=FILL), dev.alloc(48 * n, fill=FILL), dev.alloc(32 * n, fill=FILL)
        queue.pq_check(descs, sources, qb, res0, windowed=True)
        queue.pq_repair(descs, sources, qb, allow, res, windowed=True)
        queue.sync()
        form, launches = engine.option("last_desc_form"), engine.option("last_pq_repair_phases")
        queue.pq_check(descs, sources, qb, res2, windowed=True)
        raw0 = dev.get(res0, 32 * n).view(np.uint64).reshape(n, 4)
        raw = dev.get(res, 48 * n).view(np.uint64).reshape(n, 6)
        raw2 = dev.get(res2, 32 * n).view(np.uint64).reshape(n, 4)
        after_img = snapshot()
        found = [tuple(int(x) for x in r) for r in raw0]
        records = [tuple(int(x) for x in r) for r in raw]
        after = [tuple(int(x) for x in r) for r in raw2]
        for u, (b, a) in enumerate(zip(before_img, after_img)):
            assert np.array_equal(b[:MARGIN], a[:MARGIN]) and np.array_equal(b[-MARGIN:], a[-MARGIN:]), \
                f"upload {u} ({len(ups[u][0])} bytes): a byte outside it changed"
        refs, phases = [], 1
        for i, (s, (idx, ip, iq)) in enumerate(zip(self.stripes, where)):
            w, m = s["window"], s["out_len"]
            assert found[i] == R.check_record(s["chunks"], s["p"], s["q"], w, m), f"stripe {i}: the check before"
            want, chunks, p, q, np_ = R.repair(s["chunks"], s["p"], s["q"], w, m, s["allow"])
            refs.append(want)
            phases = max(phases, np_)
            assert records[i] == want, (
                f"stripe {i}: got first_bad={records[i][0]} p_bad={records[i][1]} q_bad={records[i][2]} "
                f"members={records[i][3]:#x} fixed={records[i][4]} left={records[i][5]}, expected {want[:3]} "
                f"members={want[3]:#x} fixed={want[4]} left={want[5]}")
            for name, u, exp in [(f"source {k}", u, chunks[k]) for k, u in enumerate(idx) if u is not None] + \
                                [("the P body", ip, p), ("the Q body", iq, q)]:
                got = after_img[u][MARGIN:MARGIN + len(exp)]
                if not np.array_equal(got, exp):
                    d = np.flatnonzero(got != exp)
                    raise AssertionError(f"stripe {i}, {name}: {d.size} bytes differ from the oracle after the repair, "
                                         f"first at offset {int(d[0])} (got 0x{int(got[d[0]]):02x}, expected "
                                         f"0x{int(exp[d[0]]):02x})")
            assert after[i] == R.check_record(chunks, p, q, w, m), f"stripe {i}: the check after the repair"
            if want[5] == 0:
                assert after[i] == CLEAN4, f"stripe {i}: left == 0 but not clean afterwards"
        windowed = any(s["window"] and s["out_len"] for s in self.stripes)
        assert form == (11 if windowed else 10)
        assert launches == (phases if windowed else 1)
        return records, found, refs, form, launches


# LISTS[0] = [65541, 32771, 100, 0, 32768, 98304]: T_k = 3W, 2W, W, -, W, 3W and out_len = 3W
L0 = LISTS[0]


@pytest.mark.parametrize("vecs", VECS)
def test_one_byte_with_two_echoes(engine, queue, dev, tuned, vecs):
    """Case 1: a byte of the 100-byte source, replayed into windows 1 and 2; only its bit allowed."""
    tuned("desc_vecs_per_thread", vecs)
    chunks, p, q, n = stripe(L0, seed=700)
    assert replayed_places(100, W, n, 50) == [50, 50 + W, 50 + 2 * W]
    b = Batch()
    b.add([flipped(c, 50) if k == 2 else c for k, c in enumerate(chunks)], p, q, n, allow=1 << 2)
    got, found, _, form, launches = b.run(engine, dev, queue)
    assert found == [(50, 3, 3, 1 << 2)]                # the check counts the byte and its two echoes
    assert got == [(50, 1, 1, 1 << 2, 1, 0)]            # the repair meets it once, at its home
    assert (form, launches) == (11, 2) and engine.option("last_desc_vecs") == vecs


@pytest.mark.parametrize("vecs", VECS)
def test_member_outside_the_mask(engine, queue, dev, tuned, vecs):
    """Case 2: the same damage with the bit left out: nothing written, every echo left, one launch.  (Position
    0's T_k is out_len, so its bit adds no phase.)"""
    tuned("desc_vecs_per_thread", vecs)
    chunks, p, q, n = stripe(L0, seed=701)
    b = Batch()
    for allow in (BAD_P | BAD_Q | 1, 0):
        b.add([flipped(c, 50) if k == 2 else c for k, c in enumerate(chunks)], p, q, n, allow=allow)
    got, found, _, form, launches = b.run(engine, dev, queue)   # (run: no byte changed)
    assert got == [(50, 3, 3, 1 << 2, 0, 3)] * 2 and found == [(50, 3, 3, 1 << 2)] * 2
    assert (form, launches) == (11, 1)


@pytest.mark.parametrize("vecs", VECS)
def test_two_data_members_p_and_q(engine, queue, dev, tuned, vecs):
    """Case 3: two data members with different T_k, a P byte inside a replay region and a Q byte, all at
    distinct stream offsets, all four allowed: three launches, everything restored."""
    tuned("desc_vecs_per_thread", vecs)
    chunks, p, q, n = stripe(L0, seed=702)
    places = replayed_places(100, W, n, 50) + replayed_places(32771, W, n, 32769)
    jp, jq = 2 * W + 1000, 70000                        # past 2W positions 1, 2 and 4 are replayed
    assert places == [50, 50 + W, 50 + 2 * W, 32769, 32769 + W] and not {jp, jq} & set(places)
    bad = [flipped(c, 50) if k == 2 else flipped(c, 32769, 0x81) if k == 1 else c for k, c in enumerate(chunks)]
    allow = (1 << 2) | (1 << 1) | BAD_P | BAD_Q
    b = Batch()
    b.add(bad, flipped(p, jp), flipped(q, jq, 0x3C), n, allow=allow)
    got, found, _, form, launches = b.run(engine, dev, queue)
    assert found == [(50, 6, 6, allow)]
    assert got == [(50, 3, 3, allow, 4, 0)] and (form, launches) == (11, 3)


@pytest.mark.parametrize("vecs", VECS)
def test_bytes_that_must_not_be_written(engine, queue, dev, tuned, vecs):
    """Case 4.  Syndromes that name a position at or past its len_k inside its home window, a (0, 0) source and
    a len 0 source: left, nothing written.  A byte below the last window of a long source, the last byte of
    sources that end inside a tile, the last byte of an odd out_len: repaired, and nothing beside them."""
    tuned("desc_vecs_per_thread", vecs)
    b = Batch()
    want = []
    chunks, p, q, n = stripe(L0, seed=703, none=(3,))
    for k, j in ((2, 100), (2, 200), (2, W - 1), (1, 32771), (1, 2 * W - 1), (3, 0), (3, W + 5), (4, W)):
        p2, q2 = blame(p, q, k, j)
        b.add(chunks, p2, q2, n)
        want.append((j, 1, 1, 1 << k, 0, 1))
    b.add([flipped(c, 7) if k == 0 else c for k, c in enumerate(chunks)], p, q, n)   # below lw * W: no echo
    want.append((7, 1, 1, 1, 1, 0))
    b.add([flipped(c, 65540) if k == 0 else c for k, c in enumerate(chunks)], p, q, n)  # ends 5 bytes into a tile
    want.append((65540, 1, 1, 1, 1, 0))
    # LISTS[3] = [114695, 32767, 65536, 40000, 0, 70000, 9, 32784, 65537]: odd out_len, a len 0 source
    lens = LISTS[3]
    chunks, p, q, n = stripe(lens, seed=704)
    assert n % 2 == 1 and lens[4] == 0
    p2, q2 = blame(p, q, 4, 12345)                      # the empty source blamed
    b.add(chunks, p2, q2, n)
    want.append((12345, 1, 1, 1 << 4, 0, 1))
    p2, q2 = blame(p, q, 7, 32790)                      # past len_7 = 32784, below T_7 = 2W
    b.add(chunks, p2, q2, n)
    want.append((32790, 1, 1, 1 << 7, 0, 1))
    b.add([flipped(c, n - 1) if k == 0 else c for k, c in enumerate(chunks)], p, q, n)   # the stream's last byte
    want.append((n - 1, 1, 1, 1, 1, 0))
    echoes = replayed_places(32784, W, n, 32783)        # source 7 ends 16 bytes into a tile; two echoes
    assert echoes == [32783, 32783 + W, 32783 + 2 * W]
    b.add([flipped(c, 32783) if k == 7 else c for k, c in enumerate(chunks)], p, q, n)
    want.append((32783, 1, 1, 1 << 7, 1, 0))
    b.add(chunks, flipped(p, n - 1), flipped(q, n - 2), n)  # P and Q at the odd end
    want.append((n - 2, 1, 1, BAD_P | BAD_Q, 2, 0))
    got, _, _, form, _ = b.run(engine, dev, queue)
    assert got == want and form == 11


@pytest.mark.parametrize("vecs", VECS)
def test_mixed_batch_and_batch_without_a_window(engine, queue, dev, tuned, vecs):
    """Case 5: a window 0 stripe beside a windowed one, both damaged; then no window at all through the _win
    entry point: the plain repair kernel (form 10), one launch."""
    tuned("desc_vecs_per_thread", vecs)
    chunks, p, q, n = stripe(L0, seed=705)
    chunks0, p0, q0, _ = stripe(L0, seed=706, window=0)
    bad = [flipped(c, 50) if k == 2 else c for k, c in enumerate(chunks)]
    bad0 = [flipped(c, 99) if k == 2 else c for k, c in enumerate(chunks0)]
    b = Batch()
    b.add(bad0, flipped(p0, W + 3), q0, n, window=0)
    b.add(bad, p, flipped(q, 2 * W + 9), n)
    b.add(chunks0, p0, q0, n, window=0)
    got, _, _, form, launches = b.run(engine, dev, queue)
    assert got == [(99, 2, 1, (1 << 2) | BAD_P, 2, 0), (50, 1, 2, (1 << 2) | BAD_Q, 2, 0), CLEAN6]
    assert (form, launches) == (11, 3)                  # ALL: thresholds W and 2W of the windowed stripe
    b = Batch()
    b.add(bad0, flipped(p0, W + 3), q0, n, window=0)
    b.add(chunks0, p0, q0, n, window=0)
    got, _, _, form, launches = b.run(engine, dev, queue)
    assert got == [(99, 2, 1, (1 << 2) | BAD_P, 2, 0), CLEAN6] and (form, launches) == (10, 1)


@pytest.mark.parametrize("vecs", VECS)
def test_clean_windowed_batch(engine, queue, dev, tuned, vecs):
    """Case 6: every list clean, under W and 2W: the clean record, no byte changed (Batch.run), form 11."""
    tuned("desc_vecs_per_thread", vecs)
    b = Batch()
    for i, lens in enumerate(LISTS):
        for window in (W, 2 * W):
            b.add(*stripe(lens, seed=710 + i, window=window), window=window)
    got, found, _, form, launches = b.run(engine, dev, queue)
    assert got == [CLEAN6] * len(got) and found == [CLEAN4] * len(got) and form == 11
    assert launches == max(len(R.thresholds(lens, w, max(lens), ALL)) + 1 for lens in LISTS for w in (W, 2 * W))


def test_batch_without_a_tile(engine, queue, dev):
    """out_len 0 everywhere: every record written, nothing launched."""
    empty = np.zeros(0, np.uint8)
    ups = dev.put_many([(empty, 0)] * 2)
    res = dev.alloc(96, fill=FILL)
    queue.pq_repair([(ups[0], 0, 0, 0, W), (ups[0], 0, 0, 0, 0)], [], [ups[1], ups[1]], [ALL, ALL], res, windowed=True)
    queue.sync()
    assert [tuple(int(x) for x in r) for r in dev.get(res, 96).view(np.uint64).reshape(2, 6)] == [CLEAN6] * 2
    assert engine.option("last_pq_repair_phases") == 0


def test_refuses_bad_arguments(bcp, engine, queue, dev):
    """Case 7.  Every pointer is valid and nothing is launched: the records and the buffers keep their bytes."""
    data = np.arange(64, dtype=np.uint8)
    src, p, q = dev.put(data), dev.put(data), dev.put(data)
    res = dev.alloc(96, fill=FILL)
    E = -errno.EINVAL

    def rc(stripes, sources, q_body, allow=(ALL,), results=res):
        with pytest.raises(bcp.BcpError) as e:
            queue.pq_repair(stripes, sources, q_body, allow, results, windowed=True)
        return e.value.rc

    ok_src = [(src, 64)]
    assert rc([(p, 64, 0, 1, 16 * 1024)], ok_src, [q]) == E        # a window of 16 KiB
    assert rc([(p, 64, 0, 1, W + 16)], ok_src, [q]) == E
    assert rc([(p, 64, 0, 1, W)], ok_src, [q], allow=None) == E    # no masks
    assert rc([(p, 64, 0, 1, W)], ok_src, [q], results=0) == E     # no result records
    assert rc([(0, 64, 0, 1, W)], ok_src, [q]) == E                # no P body with out_len > 0
    assert rc([(p, 64, 0, 1, W)], ok_src, [0]) == E                # no Q body
    assert rc([(p, 64, 0, 57, W)], ok_src * 57, [q]) == E          # wider than BCP_MAX_SOURCES
    assert rc([(p, 64, 0, 2, W)], ok_src, [q]) == E                # sources outside the table
    assert rc([(p, 64, 0, 1, W)], [(0, 64)], [q]) == E             # a source without an address
    queue.sync()
    assert np.all(dev.get(res, 96) == FILL)
    for ptr in (src, p, q):
        assert np.array_equal(dev.get(ptr, 64), data)
    # the plain entry point still refuses every window
    with pytest.raises(bcp.BcpError) as e:
        queue.pq_repair([(p, 64, 0, 1, W)], ok_src, [q], [ALL], res)
    assert e.value.rc == E
