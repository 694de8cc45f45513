"""The repair form of the P + Q kernel (bcp_pq_repair_stripes_async) against
numpy's GF(2^8) (tests/gf256.py), byte by byte by the three rules of bcp.h:

    Ps != 0, Qs == 0:  P[j] ^= Ps   when allow has BAD_P, else the byte is left
    Ps == 0, Qs != 0:  Q[j] ^= Qs   when allow has BAD_Q, else the byte is left
    both != 0:         D_k[j] ^= Ps for k = (LOG[Qs] - LOG[Ps]) mod 255, when k < nsrc, allow has bit k
                       and j < len_k; else the byte is left

The reference yields the expected record and the expected contents of every
buffer.  Every source, body and record array lies between guards or random
non-zero poison (tests/devbuf.py), and after each launch every upload is read
back and must equal the reference exactly: corrected bytes corrected, everything
else unchanged, guards intact (Dev.free).  Then the existing check form runs
over the same buffers and must report what the reference says is left -- the
all-clear for every stripe with left == 0.  Stripes share no uploads: that is
the entry point's contract.  Both tile sizes (desc_vecs_per_thread 4 and 8: 16
and 32 KiB) run everything."""
import ctypes
import errno

import numpy as np
import pytest

import gf256 as G
from devbuf import FILL, Dev
from test_gpu_pq_check import boundary_stripes, ref_record

pytestmark = pytest.mark.gpu
KiB = 1024
VECS = (4, 8)
CLEAN = (2 ** 64 - 1, 0, 0, 0, 0, 0)
BAD_P, BAD_Q, NOWHERE = 1 << 56, 1 << 57, 1 << 58
ALL = 2 ** 64 - 1
FLIP = 0x5A


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


def ref_repair(chunks, p, q, out_len, allow):
    """(record, chunks, p, q) after the repair, by the rules.  chunks: arrays, None for the source (0, 0)."""
    chunks = [None if c is None else np.array(c, dtype=np.uint8, copy=True) for c in chunks]
    p, q = np.array(p, dtype=np.uint8, copy=True), np.array(q, dtype=np.uint8, copy=True)
    ps = p[:out_len] ^ G.p_of(chunks, out_len)
    qs = q[:out_len] ^ G.q_sum(chunks, out_len)
    # the state as found: the check form's record, by its definition
    bad = np.flatnonzero((ps != 0) | (qs != 0))
    members = (BAD_P if np.any((ps != 0) & (qs == 0)) else 0) | (BAD_Q if np.any((ps == 0) & (qs != 0)) else 0)
    both = np.flatnonzero((ps != 0) & (qs != 0))
    ks = (G.LOG[qs[both]] - G.LOG[ps[both]]) % 255
    for k in np.unique(ks):
        members |= (1 << int(k)) if k < len(chunks) else NOWHERE
    found = (int(bad[0]) if bad.size else 2 ** 64 - 1, int(np.count_nonzero(ps)), int(np.count_nonzero(qs)), members)
    fixed = left = 0
    for body, own, other, bit in ((p, ps, qs, BAD_P), (q, qs, ps, BAD_Q)):
        j = np.flatnonzero((own != 0) & (other == 0))
        if allow & bit:
            body[j] ^= own[j]
            fixed += j.size
        else:
            left += j.size
    for j, k in zip(both, ks):
        j, k = int(j), int(k)
        if k < len(chunks) and (allow >> k) & 1 and chunks[k] is not None and j < len(chunks[k]):
            chunks[k][j] ^= ps[j]
            fixed += 1
        else:
            left += 1
    return found + (fixed, left), chunks, p, q


class Batch:
    """Stripes of one launch, every source and body an upload of its own."""

    def __init__(self):
        self.stripes = []

    def add(self, chunks, p, q, out_len, pads=None, p_pad=0, q_pad=0, allow=ALL):
        self.stripes.append(dict(chunks=[None if c is None else np.array(c, dtype=np.uint8, copy=True) for c in chunks],
                                 p=np.array(p, dtype=np.uint8, copy=True), q=np.array(q, dtype=np.uint8, copy=True),
                                 out_len=out_len, pads=pads or [0] * len(chunks), p_pad=p_pad, q_pad=q_pad,
                                 allow=allow))
        return len(self.stripes) - 1

    def run(self, bcp, dev, queue):
        """Upload, repair, read everything back and compare it with the reference; then the check form over
        the same buffers.  Returns (records, reference records)."""
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
            descs.append((addrs[ip], s["out_len"], first, len(idx), 0))
            qb.append(addrs[iq])
            allow.append(s["allow"])
        n = len(self.stripes)
        res = dev.alloc(48 * n, fill=FILL)
        res2 = dev.alloc(32 * n, fill=FILL)
        queue.pq_repair(descs, sources, qb, allow, res)
        queue.pq_check(descs, sources, qb, res2)
        raw = dev.get(res, 48 * n).view(np.uint64).reshape(n, 6)
        raw2 = dev.get(res2, 32 * n).view(np.uint64).reshape(n, 4)
        got = [np.empty(max(len(a), 1), np.uint8) for a, _ in ups]
        for g, ptr, (a, _) in zip(got, addrs, ups):
            if len(a):
                queue.d2h(g, ptr, len(a))
        queue.sync()
        records = [tuple(int(x) for x in r) for r in raw]
        after = [tuple(int(x) for x in r) for r in raw2]
        refs = []
        for i, (s, (idx, ip, iq)) in enumerate(zip(self.stripes, where)):
            want, chunks, p, q = ref_repair(s["chunks"], s["p"], s["q"], s["out_len"], s["allow"])
            refs.append(want)
            assert records[i] == want, (
                f"stripe {i}: got first_bad={records[i][0]} p_bad={records[i][1]} q_bad={records[i][2]} "
                f"members={records[i][3]:#x} fixed={records[i][4]} left={records[i][5]}, expected {want[:3]} "
                f"members={want[3]:#x} fixed={want[4]} left={want[5]}")
            for name, u, exp in [(f"source {k}", u, chunks[k]) for k, u in enumerate(idx) if u is not None] + \
                                [("the P body", ip, p), ("the Q body", iq, q)]:
                if not np.array_equal(got[u][:len(exp)], exp):
                    w = np.flatnonzero(got[u][:len(exp)] != exp)
                    raise AssertionError(f"stripe {i}, {name}: {w.size} bytes differ from the reference after the "
                                         f"repair, first at offset {int(w[0])} (got 0x{int(got[u][w[0]]):02x}, "
                                         f"expected 0x{int(exp[w[0]]):02x})")
            # what the check form finds afterwards is what the reference left: nothing when left == 0
            assert after[i] == ref_record(chunks, p, q, s["out_len"]), f"stripe {i}: pq_check after the repair"
            if want[5] == 0:
                assert after[i] == bcp.PQ_CHECK_CLEAN, f"stripe {i}: left == 0 but not clean afterwards"
        return records, refs


def _flip_offsets(T, out_len, len_k=None):
    """0, out_len - 1, T - 1, T and a member's own last byte, where they exist."""
    offs = {0, out_len - 1, T - 1, T}
    if len_k is not None:
        offs.add(len_k - 1)
        return sorted(o for o in offs if 0 <= o < min(len_k, out_len))
    return sorted(o for o in offs if 0 <= o < out_len)


@pytest.mark.parametrize("victim", ("clean", "data", "p", "q"))
@pytest.mark.parametrize("vecs", VECS)
def test_boundary_shapes(bcp, engine, queue, dev, tuned, vecs, victim):
    """Every shape clean (the clean record, nothing changed) or with one flipped byte in one data member, in P
    or in Q, at every boundary offset; everything allowed."""
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(400 + vecs)
    b = Batch()
    nbad = 0
    for chunks, out_len, pads, p_pad, q_pad in boundary_stripes(T, rng):
        p, q = G.p_of(chunks, out_len), G.q_sum(chunks, out_len)
        if victim == "clean":
            b.add(chunks, p, q, out_len, pads, p_pad, q_pad)
            continue
        if out_len == 0:
            continue
        if victim == "data":
            live = [k for k, c in enumerate(chunks) if c is not None and len(c)]
            # the longest member (it reaches every offset) and, where there is one, a member that ends inside the
            # output: its own last byte
            short = [k for k in live if len(chunks[k]) < out_len]
            for k in [max(live, key=lambda k: len(chunks[k]))] + short[:1]:
                for off in _flip_offsets(T, out_len, len(chunks[k])):
                    c2 = [None if c is None else c.copy() for c in chunks]
                    c2[k][off] ^= FLIP
                    b.add(c2, p, q, out_len, pads, p_pad, q_pad)
                    nbad += 1
        else:
            for off in _flip_offsets(T, out_len):
                body = (p if victim == "p" else q).copy()
                body[off] ^= FLIP
                b.add(chunks, body if victim == "p" else p, body if victim == "q" else q, out_len, pads, p_pad, q_pad)
                nbad += 1
    got, refs = b.run(bcp, dev, queue)
    assert engine.option("last_desc_form") == 6 and engine.option("last_desc_vecs") == vecs  # (run ends on the check)
    if victim == "clean":
        assert got == [CLEAN] * len(got)
    else:
        assert nbad > 100 and all(g[4:] == (1, 0) for g in got)  # every flipped byte found and put right
        bit = {"p": BAD_P, "q": BAD_Q}.get(victim)
        assert all(g[3] == bit for g in got) if bit else all(0 < g[3] < (1 << 56) for g in got)


def test_last_desc_form_is_the_repair_forms(bcp, engine, queue, dev):
    data = np.arange(64, dtype=np.uint8)
    src, p, q = dev.put(data), dev.put(data), dev.put(G.q_sum([data], 64))
    res = dev.alloc(48, fill=FILL)
    queue.pq_repair([(p, 64, 0, 1, 0)], [(src, 64)], [q], [ALL], res)
    queue.sync()
    assert engine.option("last_desc_form") == 10
    assert tuple(int(x) for x in dev.get(res, 48).view(np.uint64)) == CLEAN
    assert ctypes.sizeof(bcp.PqRepairResult) == 48 and bcp.PQ_REPAIR_CLEAN == CLEAN


@pytest.mark.parametrize("vecs", VECS)
def test_whole_members(bcp, engine, queue, dev, tuned, vecs):
    """A whole member replaced by random bytes: a data member (one that ends inside a tile too), P, Q."""
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(410 + vecs)
    out_len = 2 * T + 17
    b = Batch()
    for width, short_pos in ((9, 5), (56, 13), (1, 0)):
        chunks = [rng.integers(0, 256, size=out_len, dtype=np.uint8) for _ in range(width)]
        if width > 1:
            chunks[short_pos] = rng.integers(0, 256, size=T + 1000 + 5, dtype=np.uint8)
        pads = [(width + 3 * k) % 16 for k in range(width)]
        p, q = G.p_of(chunks, out_len), G.q_sum(chunks, out_len)
        for k in sorted({0, short_pos, width - 1}):
            c2 = list(chunks)
            c2[k] = rng.integers(0, 256, size=len(chunks[k]), dtype=np.uint8)
            b.add(c2, p, q, out_len, pads, 5, 11)
        b.add(chunks, rng.integers(0, 256, size=out_len, dtype=np.uint8), q, out_len, pads, 5, 11)
        b.add(chunks, p, rng.integers(0, 256, size=out_len, dtype=np.uint8), out_len, pads, 5, 11)
    got, _ = b.run(bcp, dev, queue)
    assert all(g[5] == 0 and g[4] > T for g in got)


@pytest.mark.parametrize("vecs", VECS)
def test_two_members_in_one_stripe(bcp, engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(420 + vecs)
    out_len = T + 4096 + 3
    b = Batch()
    firsts = []
    for width in (3, 56):
        chunks = [rng.integers(0, 256, size=out_len, dtype=np.uint8) for _ in range(width)]
        pads = [(2 * width + 5 * k) % 16 for k in range(width)]
        p, q = G.p_of(chunks, out_len), G.q_sum(chunks, out_len)
        lo, hi = 0, width - 1

        def damaged(flips, pf=(), qf=()):
            c2 = [c.copy() for c in chunks]
            for k, off, e in flips:
                c2[k][off] ^= e
            p2, q2 = p.copy(), q.copy()
            for off in pf:
                p2[off] ^= FLIP
            for off in qf:
                q2[off] ^= FLIP
            return c2, p2, q2

        # different offsets, both allowed: both fixed (and clean afterwards: Batch.run)
        firsts.append((b.add(*damaged([(lo, 100, FLIP), (hi, T + 7, FLIP)]), out_len, pads, 3, 9), hi))
        b.add(*damaged([(hi, T + 7, FLIP)], pf=[T - 1]), out_len, pads, 3, 9)
        b.add(*damaged([(1, 5, 0x01)], pf=[6], qf=[7, out_len - 1]), out_len, pads, 3, 9)
        # the same offset, by the same value (reads as Q) and by different values (may name a third member):
        # whatever the rules make of it
        b.add(*damaged([(lo, 33, FLIP), (hi, 33, FLIP)]), out_len, pads, 3, 9)
        for e in (0x01, 0x80, 0xC3):
            b.add(*damaged([(lo, T + 1, FLIP), (hi, T + 1, e)]), out_len, pads, 3, 9)
            b.add(*damaged([(1, 77, e)], pf=[77]), out_len, pads, 3, 9)
    got, refs = b.run(bcp, dev, queue)
    for first, hi in firsts:
        assert got[first] == (100, 2, 2, 1 | (1 << hi), 2, 0)
        assert got[first + 1][3:] == ((1 << hi) | BAD_P, 2, 0) and got[first + 2][3:] == (2 | BAD_P | BAD_Q, 4, 0)


@pytest.mark.parametrize("vecs", VECS)
def test_mask_honoured(bcp, engine, queue, dev, tuned, vecs):
    """A blamed member outside the mask is bit-identical afterwards, its bytes are counted as left, and
    members is as found; members inside the mask are still corrected."""
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(430 + vecs)
    out_len = T + 300
    width = 9
    chunks = [rng.integers(0, 256, size=out_len, dtype=np.uint8) for _ in range(width)]
    pads = [(3 * k + 1) % 16 for k in range(width)]
    p, q = G.p_of(chunks, out_len), G.q_sum(chunks, out_len)
    b = Batch()
    want = []
    for offs in ((0,), (T - 1, T, out_len - 1), tuple(range(T - 20, T + 20))):
        c2 = [c.copy() for c in chunks]
        c2[4][list(offs)] ^= FLIP
        p2, q2 = p.copy(), q.copy()
        p2[list(offs)] ^= FLIP
        q2[list(offs)] ^= FLIP
        n = len(offs)
        for allow in (0, ALL & ~(1 << 4), 1 << 3, BAD_P | BAD_Q):
            b.add(c2, p, q, out_len, pads, 2, 7, allow=allow)
            want.append((offs[0], n, n, 1 << 4, 0, n))
        for allow in (0, ALL & ~BAD_P, BAD_Q | 0xFF):
            b.add(chunks, p2, q, out_len, pads, 2, 7, allow=allow)
            want.append((offs[0], n, 0, BAD_P, 0, n))
        for allow in (0, ALL & ~BAD_Q, BAD_P | 0xFF):
            b.add(chunks, p, q2, out_len, pads, 2, 7, allow=allow)
            want.append((offs[0], 0, n, BAD_Q, 0, n))
    # a data member and P damaged at different offsets, only one of them allowed
    c2 = [c.copy() for c in chunks]
    c2[8][10] ^= FLIP
    p2 = p.copy()
    p2[T + 5] ^= FLIP
    b.add(c2, p2, q, out_len, pads, 2, 7, allow=1 << 8)
    want.append((10, 2, 1, (1 << 8) | BAD_P, 1, 1))
    b.add(c2, p2, q, out_len, pads, 2, 7, allow=BAD_P)
    want.append((10, 2, 1, (1 << 8) | BAD_P, 1, 1))
    got, refs = b.run(bcp, dev, queue)
    assert got == want


@pytest.mark.parametrize("vecs", VECS)
def test_padding_blamed(bcp, engine, queue, dev, tuned, vecs):
    """P and Q altered consistently so that the syndromes name position k at an offset at or past len_k (and
    a (0, 0) source, and a position past nsrc): zero padding cannot be wrong, so the byte is left."""
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(440 + vecs)
    out_len = T + 100
    lens = [out_len, T - 5, 40, 0, out_len]
    chunks = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in lens]
    chunks.append(None)  # position 5: the source (0, 0)
    pads = [1, 2, 3, 4, 5, 0]
    p, q = G.p_of(chunks, out_len), G.q_sum(chunks, out_len)
    b = Batch()
    want = []
    for k, j in ((1, T - 5), (1, T), (1, out_len - 1), (2, 40), (3, 0), (5, 7), (5, T + 1), (9, 3)):
        p2, q2 = p.copy(), q.copy()
        p2[j] ^= FLIP
        q2[j] ^= int(G.mul(np.uint8(FLIP), np.uint8(G.gpow(k))))
        b.add(chunks, p2, q2, out_len, pads, 6, 13)
        want.append((j, 1, 1, (1 << k) if k < len(chunks) else NOWHERE, 0, 1))
    got, refs = b.run(bcp, dev, queue)  # (run: no buffer changed)
    assert got == want


def test_many_small_stripes_some_bad(bcp, engine, queue, dev):
    """More stripes than a few workgroups take at once, a third of them with a defect somewhere, random masks."""
    rng = np.random.default_rng(450)
    b = Batch()
    for i in range(240):
        width = int(rng.integers(1, 10))
        out_len = int(rng.integers(1, 700))
        chunks = [rng.integers(0, 256, size=int(rng.integers(0, out_len + 1)), dtype=np.uint8) for _ in range(width)]
        chunks[0] = rng.integers(0, 256, size=out_len, dtype=np.uint8)
        p, q = G.p_of(chunks, out_len), G.q_sum(chunks, out_len)
        if i % 3 == 0:
            victim = (chunks[0], p, q)[i // 3 % 3]
            victim[int(rng.integers(0, out_len))] ^= int(rng.integers(1, 256))
        allow = ALL if i % 2 else int(rng.integers(0, 2 ** 62)) << 1 | int(rng.integers(0, 2))
        b.add(chunks, p, q, out_len, [int(x) for x in rng.integers(0, 16, size=width)], int(rng.integers(0, 16)),
              int(rng.integers(0, 16)), allow=allow)
    got, refs = b.run(bcp, dev, queue)
    assert sum(g != CLEAN for g in got) == 80 and sum(g[4] for g in got) >= 40


def test_batch_without_a_tile_writes_every_record(bcp, engine, queue, dev):
    b = Batch()
    empty = np.zeros(0, np.uint8)
    for width in (0, 1, 3):
        b.add([empty] * width, empty, empty, 0)
    got, _ = b.run(bcp, dev, queue)
    assert got == [CLEAN] * 3


def test_refuses_bad_arguments(bcp, engine, queue, dev):
    data = np.arange(64, dtype=np.uint8)
    src, p, q = dev.put(data), dev.put(data), dev.put(data)
    res = dev.alloc(96, fill=FILL)
    E = -errno.EINVAL

    def rc(stripes, sources, q_body, allow=(ALL,), results=res):
        with pytest.raises(bcp.BcpError) as e:
            queue.pq_repair(stripes, sources, q_body, allow, results)
        return e.value.rc

    ok_src = [(src, 64)]
    assert rc([(p, 64, 0, 1, 16 * KiB)], ok_src, [q]) == E        # a window
    assert rc([(p, 64, 0, 1, 32 * KiB)], ok_src, [q]) == E        # also one the windowed entry points take
    assert rc([(p, 64, 0, 1, 0)], ok_src, [q], allow=None) == E   # no masks
    assert rc([(p, 64, 0, 1, 0)], ok_src, [q], results=0) == E    # no result records
    assert rc([(0, 64, 0, 1, 0)], ok_src, [q]) == E               # no P body
    assert rc([(p, 64, 0, 1, 0)], ok_src, [0]) == E               # no Q body
    assert rc([(p, 64, 0, 57, 0)], ok_src * 57, [q]) == E         # wider than BCP_MAX_SOURCES
    assert rc([(p, 64, 0, 2, 0)], ok_src, [q]) == E               # sources outside the table
    assert rc([(p, 64, 0, 1, 0)], [(0, 64)], [q]) == E            # a source without an address
    queue.sync()
    assert np.all(dev.get(res, 96) == FILL)
    for ptr in (src, p, q):
        assert np.array_equal(dev.get(ptr, 64), data)
