"""The syndrome form of the P + Q kernel (bcp_pq_check_stripes_async) against
numpy's GF(2^8) (tests/gf256.py): per byte Ps = P ^ XOR D_k, Qs = Q ^ XOR g^k D_k
and, where both are non-zero, k = (LOG[Qs] - LOG[Ps]) mod 255.  All four fields
of every record must be equal to the reference.

Every source, P body, Q body and result array lies between guards or random
non-zero poison (tests/devbuf.py): a load outside a buffer turns a clean stripe
into a mismatch, a store outside the records fails Dev.free.  After every run
the sources and bodies are read back and must be unchanged.  Both tile sizes
(desc_vecs_per_thread 4 and 8: 16 and 32 KiB) run everything."""
import ctypes
import errno

import numpy as np
import pytest

import gf256 as G
from devbuf import FILL, Dev

pytestmark = pytest.mark.gpu
KiB = 1024
VECS = (4, 8)
CLEAN = (2 ** 64 - 1, 0, 0, 0)
BAD_P, BAD_Q, NOWHERE = 1 << 56, 1 << 57, 1 << 58
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


def ref_record(chunks, p, q, out_len):
    """The record by the definition.  chunks: arrays, None for the source (0, 0)."""
    ps = p[:out_len] ^ G.p_of(chunks, out_len)
    qs = q[:out_len] ^ G.q_sum(chunks, out_len)
    bad = np.flatnonzero((ps != 0) | (qs != 0))
    members = 0
    if np.any((ps != 0) & (qs == 0)):
        members |= BAD_P
    if np.any((ps == 0) & (qs != 0)):
        members |= BAD_Q
    both = (ps != 0) & (qs != 0)
    for k in np.unique((G.LOG[qs[both]] - G.LOG[ps[both]]) % 255):
        members |= (1 << int(k)) if k < len(chunks) else NOWHERE
    return (int(bad[0]) if bad.size else 2 ** 64 - 1, int(np.count_nonzero(ps)), int(np.count_nonzero(qs)), members)


class Batch:
    """Stripes of one launch over shared uploads: a stripe names its sources and bodies by upload index,
    so a defect costs one more upload, not a copy of the stripe."""

    def __init__(self):
        self.ups, self.stripes = [], []

    def up(self, arr, pad=0):
        self.ups.append((np.ascontiguousarray(arr, np.uint8), pad))
        return len(self.ups) - 1

    def stripe(self, src, p, q, out_len):
        """src: upload indices in position order, None for the source (0, 0)."""
        self.stripes.append((list(src), p, q, out_len))
        return len(self.stripes) - 1

    def host(self, i):
        src, p, q, out_len = self.stripes[i]
        return [None if s is None else self.ups[s][0] for s in src], self.ups[p][0], self.ups[q][0], out_len

    def refs(self):
        return [ref_record(*self.host(i)) for i in range(len(self.stripes))]

    def run(self, bcp, dev, queue):
        """Upload, launch, read the records back; sources and bodies must be unchanged afterwards."""
        addrs = dev.put_many(self.ups)
        descs, sources, qb = [], [], []
        for src, p, q, out_len in self.stripes:
            first = len(sources)
            sources += [(0, 0) if s is None else (addrs[s], len(self.ups[s][0])) for s in src]
            descs.append((addrs[p], out_len, first, len(src), 0))
            qb.append(addrs[q])
        n = len(self.stripes)
        res = dev.alloc(32 * n, fill=FILL)
        queue.pq_check(descs, sources, qb, res)
        raw = dev.get(res, 32 * n).view(np.uint64).reshape(n, 4)
        got = [np.empty(max(len(a), 1), np.uint8) for a, _ in self.ups]
        for g, ptr, (a, _) in zip(got, addrs, self.ups):
            if len(a):
                queue.d2h(g, ptr, len(a))
        queue.sync()
        for i, (g, (a, _)) in enumerate(zip(got, self.ups)):
            assert np.array_equal(g[:len(a)], a), f"upload {i} (a source or a body) changed on the device"
        return [tuple(int(x) for x in r) for r in raw]


def assert_records(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f"{what} stripe {i}: got first_bad={g[0]} p_bad={g[1]} q_bad={g[2]} members={g[3]:#x}, "
                        f"expected first_bad={w[0]} p_bad={w[1]} q_bad={w[2]} members={w[3]:#x}")


def boundary_stripes(T, rng):
    """(chunks, out_len, pads, p_pad, q_pad): the shapes of the gen and recovery tests of the same kernel."""
    out = []
    i = 0
    for out_len in (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 17):
        for width in (1, 2, 3, 8, 9, 56):
            lens = [int(x) for x in rng.integers(0, out_len + 1, size=width)]
            lens[int(rng.integers(0, width))] = out_len
            chunks = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in lens]
            if width >= 8 and out_len > 64:
                inside = (out_len - 40) // 16 * 16
                chunks[1] = rng.integers(0, 256, size=inside, dtype=np.uint8)      # ends inside the last tile at a
                chunks[2] = rng.integers(0, 256, size=inside + 5, dtype=np.uint8)  # multiple of 16, and 5 further
                chunks[3] = None                                                    # the source (0, 0)
                chunks[4] = np.zeros(0, np.uint8)                                   # empty, at a valid address
            out.append((chunks, out_len, [(i * 7 + 3 * k) % 16 for k in range(width)], (i * 5 + 1) % 16,
                        (i * 11 + 2) % 16))
            i += 1
    # zero tails, sources ending inside the first and second tile, and sources longer than the output (cut)
    out.append(([rng.integers(0, 256, size=L, dtype=np.uint8) for L in (T + 160, T + 163, 48, 2 * T)], 2 * T + 17,
                [1, 2, 3, 4], 9, 6))
    out.append(([rng.integers(0, 256, size=L, dtype=np.uint8) for L in (3 * T, T + 5, 7)], T + 21, [15, 0, 8], 0, 0))
    return out


def add_clean(b, chunks, out_len, pads, p_pad, q_pad):
    """The stripe with the reference's own bodies; returns (stripe index, source, P and Q upload indices)."""
    src = [None if c is None else b.up(c, pad) for c, pad in zip(chunks, pads)]
    p, q = b.up(G.p_of(chunks, out_len), p_pad), b.up(G.q_sum(chunks, out_len), q_pad)
    return b.stripe(src, p, q, out_len), src, p, q


@pytest.mark.parametrize("host_max", (4096, 0))  # the tables: by size, always copied
@pytest.mark.parametrize("vecs", VECS)
def test_clean_boundary_shapes(bcp, engine, queue, dev, tuned, vecs, host_max):
    """One batch of every shape, stripes with and without tiles mixed: every record is the all-clear."""
    tuned("desc_vecs_per_thread", vecs)
    tuned("table_host_max", host_max)
    T = 256 * 16 * vecs
    b = Batch()
    for shape in boundary_stripes(T, np.random.default_rng(300 + vecs)):
        add_clean(b, *shape)
    got = b.run(bcp, dev, queue)
    assert engine.option("last_desc_form") == 6 and engine.option("last_desc_vecs") == vecs
    assert_records(got, [CLEAN] * len(got), "clean")


def test_batch_without_a_tile_writes_every_record(bcp, engine, queue, dev):
    b = Batch()
    empty = b.up(np.zeros(0, np.uint8))
    for width in (0, 1, 3):
        b.stripe([empty] * width, empty, empty, 0)
    assert_records(b.run(bcp, dev, queue), [CLEAN] * 3, "empty")


@pytest.mark.parametrize("vecs", VECS)
def test_bytes_past_out_len_do_not_count(bcp, engine, queue, dev, tuned, vecs):
    """Clean bodies that end in the middle of a vector, short sources and sources longer than the output:
    what follows them on the device is non-zero poison (or the source's own bytes), and none of it may
    reach the verdict."""
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(310 + vecs)
    b = Batch()
    i = 0
    for out_len in (5, 16 + 3, T - 7, T + 21, 2 * T + 9):
        for lens in ((out_len, out_len // 2 + 1, 1), (out_len + 100, out_len, 3), (out_len + T + 3, out_len - 1),
                     (out_len + 1,)):
            chunks = [rng.integers(1, 256, size=L, dtype=np.uint8) for L in lens]
            add_clean(b, chunks, out_len, [(i + 5 * k) % 16 for k in range(len(lens))], (3 * i + 1) % 16, (7 * i + 2) % 16)
            i += 1
    got = b.run(bcp, dev, queue)
    assert engine.option("last_desc_form") == 6
    assert_records(got, [CLEAN] * len(got), "tail")


def _flipped(arr, offs):
    a = np.array(arr, dtype=np.uint8, copy=True)
    a[list(offs)] ^= FLIP
    return a


def _base_stripe(rng, width, out_len, short_pos, short_len):
    """Full-length members but one, which ends inside a tile."""
    chunks = [rng.integers(0, 256, size=out_len, dtype=np.uint8) for _ in range(width)]
    chunks[short_pos] = rng.integers(0, 256, size=short_len, dtype=np.uint8)
    return chunks


@pytest.mark.parametrize("vecs", VECS)
def test_one_flipped_byte_names_its_member(bcp, engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(320 + vecs)
    out_len = 2 * T + 17
    b = Batch()
    want = []
    for width, short_pos in ((56, 13), (9, 5), (4, 1)):
        short_len = T + 1000 + 5  # ends inside the second tile, in the middle of a vector
        chunks = _base_stripe(rng, width, out_len, short_pos, short_len)
        pads = [(width + 3 * k) % 16 for k in range(width)]
        _, src, p, q = add_clean(b, chunks, out_len, pads, 5, 11)
        want.append(CLEAN)
        offsets = (0, 15, 16, T - 1, T, out_len - 1, short_len - 1)
        for pos in (0, width // 2, width - 1):
            for off in offsets:
                s2 = list(src)
                s2[pos] = b.up(_flipped(chunks[pos], [off]), pads[pos])
                b.stripe(s2, p, q, out_len)
                want.append((off, 1, 1, 1 << pos))
        s2 = list(src)  # the short member's own last byte
        s2[short_pos] = b.up(_flipped(chunks[short_pos], [short_len - 1]), pads[short_pos])
        b.stripe(s2, p, q, out_len)
        want.append((short_len - 1, 1, 1, 1 << short_pos))
        for off in offsets:
            b.stripe(src, b.up(_flipped(b.ups[p][0], [off]), 5), q, out_len)
            want.append((off, 1, 0, BAD_P))
            b.stripe(src, p, b.up(_flipped(b.ups[q][0], [off]), 11), out_len)
            want.append((off, 0, 1, BAD_Q))
        # 300 consecutive bytes of one member across a tile boundary
        pos = width // 2
        s2 = list(src)
        s2[pos] = b.up(_flipped(chunks[pos], range(T - 150, T + 150)), pads[pos])
        b.stripe(s2, p, q, out_len)
        want.append((T - 150, 300, 300, 1 << pos))
    got = b.run(bcp, dev, queue)
    assert engine.option("last_desc_form") == 6 and engine.option("last_desc_vecs") == vecs
    assert_records(got, want, "one defect (expected)")
    assert_records(got, b.refs(), "one defect (reference)")
    for g in got[1:1 + 21]:
        assert bcp.pq_culprit(g)[0] == bcp.CULPRIT_DATA


@pytest.mark.parametrize("vecs", VECS)
def test_more_than_one_defect(bcp, engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(330 + vecs)
    out_len = T + 4096 + 3
    b = Batch()
    want = []
    for width, far in ((3, 5), (56, 200)):
        chunks = [rng.integers(0, 256, size=out_len, dtype=np.uint8) for _ in range(width)]
        pads = [(2 * width + 5 * k) % 16 for k in range(width)]
        _, src, p, q = add_clean(b, chunks, out_len, pads, 3, 9)
        want.append(CLEAN)
        lo, hi = 0, width - 1
        # two data members at different offsets: two bits
        s2 = list(src)
        s2[lo] = b.up(_flipped(chunks[lo], [100]), pads[lo])
        s2[hi] = b.up(_flipped(chunks[hi], [T + 7]), pads[hi])
        b.stripe(s2, p, q, out_len)
        want.append((100, 2, 2, (1 << lo) | (1 << hi)))
        # a data member and P at different offsets: bit k and BAD_P
        s3 = list(src)
        s3[hi] = s2[hi]
        b.stripe(s3, b.up(_flipped(b.ups[p][0], [T - 1]), 3), q, out_len)
        want.append((T - 1, 2, 1, (1 << hi) | BAD_P))
        # Qs = g^far * Ps with far >= nsrc: no member explains it
        e = 0x5A
        p_bad, q_bad = b.ups[p][0].copy(), b.ups[q][0].copy()
        p_bad[T + 1] ^= e
        q_bad[T + 1] ^= int(G.mul(np.uint8(e), np.uint8(G.gpow(far))))
        b.stripe(src, b.up(p_bad, 3), b.up(q_bad, 9), out_len)
        want.append((T + 1, 1, 1, NOWHERE))
        # two members changed by the same value at the same offset: Ps = 0, Qs != 0, which by the record's
        # definition reads as Q (a double fault the syndromes cannot tell from a bad Q byte)
        s4 = list(src)
        s4[lo] = b.up(_flipped(chunks[lo], [33]), pads[lo])
        s4[hi] = b.up(_flipped(chunks[hi], [33]), pads[hi])
        b.stripe(s4, p, q, out_len)
        want.append((33, 0, 1, BAD_Q))
    got = b.run(bcp, dev, queue)
    assert engine.option("last_desc_form") == 6
    assert_records(got, want, "several defects (expected)")
    assert_records(got, b.refs(), "several defects (reference)")
    assert [bcp.pq_culprit(g)[0] for g in got[1:5]] == [bcp.CULPRIT_MANY, bcp.CULPRIT_MANY, bcp.CULPRIT_MANY,
                                                        bcp.CULPRIT_Q]


def test_many_small_stripes_some_bad(bcp, engine, queue, dev):
    """More stripes than a few workgroups take at once, a third of them with a defect somewhere."""
    rng = np.random.default_rng(340)
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
        src = [b.up(c, int(rng.integers(0, 16))) for c in chunks]
        b.stripe(src, b.up(p, int(rng.integers(0, 16))), b.up(q, int(rng.integers(0, 16))), out_len)
    got = b.run(bcp, dev, queue)
    assert_records(got, b.refs(), "small")
    assert sum(g != CLEAN for g in got) == 80


def test_refuses_bad_arguments(bcp, engine, queue, dev):
    data = np.arange(64, dtype=np.uint8)
    src, p, q = dev.put(data), dev.put(data), dev.put(data)
    res = dev.alloc(64, fill=FILL)
    E = -errno.EINVAL

    def rc(stripes, sources, q_body, results=res):
        with pytest.raises(bcp.BcpError) as e:
            queue.pq_check(stripes, sources, q_body, results)
        return e.value.rc

    ok_src = [(src, 64)]
    assert rc([(p, 64, 0, 1, 16 * KiB)], ok_src, [q]) == E        # a window
    assert rc([(p, 64, 0, 1, 0)], ok_src, [q], results=0) == E    # no result records
    assert rc([(0, 64, 0, 1, 0)], ok_src, [q]) == E               # no P body
    assert rc([(p, 64, 0, 1, 0)], ok_src, [0]) == E               # no Q body
    assert rc([(p, 64, 0, 57, 0)], ok_src * 57, [q]) == E         # wider than BCP_MAX_SOURCES
    assert rc([(p, 64, 0, 2, 0)], ok_src, [q]) == E               # sources outside the table
    assert rc([(p, 64, 0, 1, 0)], [(0, 64)], [q]) == E            # a source without an address
    queue.sync()
    assert np.all(dev.get(res, 64) == FILL)
    assert ctypes.sizeof(bcp.PqCheckResult) == 32
