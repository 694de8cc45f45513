"""The verified-rebuild form of the P + Q kernel (bcp_pq_rebuild_check_stripes_async
and its _win namesake) against numpy (tests/pq_rebuild_ref.py): the bytes of the
lost member and both fields of every record must be equal to the reference.

Every source, body, output area and result array lies between guards or random
non-zero poison (tests/devbuf.py): a load outside a buffer turns a clean stripe
into a suspect, a store outside [dst_x, dst_x + len_x) or the records fails the
area check or Dev.free.  After every run the sources and bodies are read back
and must be unchanged.  Both tile sizes (desc_vecs_per_thread 4 and 8: 16 and
32 KiB) run everything."""
import errno

import numpy as np
import pytest

import gf256 as G
import pq_rebuild_ref as R
import pq_window as PW
from devbuf import FILL, SLACK, Dev

pytestmark = pytest.mark.gpu
KiB = 1024
VECS = (4, 8)
NONE = 0xFFFFFFFF
FLIP = 0x5A
WIDTH_X = [(1, 0), (2, 0), (2, 1), (5, 0), (5, 2), (5, 4), (9, 0), (9, 4), (9, 8), (56, 0), (56, 31), (56, 55)]


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


class Batch:
    """Stripes of one launch over shared uploads: a stripe names its survivors and bodies by upload index, so a
    fault costs one more upload, not a copy of the stripe."""

    def __init__(self):
        self.ups, self.stripes = [], []

    def up(self, arr, pad=0):
        self.ups.append((np.ascontiguousarray(arr, np.uint8), pad))
        return len(self.ups) - 1

    def stripe(self, src, p, q, x, out_len, len_x, window=0, dst_pad=0):
        """src: upload indices in position order, None for the source (0, 0); position x is None or an empty upload."""
        assert src[x] is None or len(self.ups[src[x]][0]) == 0
        self.stripes.append((list(src), p, q, x, out_len, len_x, window, dst_pad))
        return len(self.stripes) - 1

    def refs(self):
        out = []
        for src, p, q, x, out_len, len_x, window, _ in self.stripes:
            chunks = [None if s is None else self.ups[s][0] for s in src]
            out.append(R.rebuild(chunks, self.ups[p][0], self.ups[q][0], x, out_len, len_x, window))
        return out

    def run(self, dev, queue, windowed=False):
        """Upload, launch, read everything back -> [(output bytes, (first_bad, bad_bytes))].  The output areas
        outside [dst_x, dst_x + len_x) must still hold the fill, the uploads must be unchanged."""
        addrs = dev.put_many(self.ups)
        descs, sources, lost, areas = [], [], [], []
        for src, p, q, x, out_len, len_x, window, dst_pad in self.stripes:
            first = len(sources)
            sources += [(0, 0) if s is None else (addrs[s], len(self.ups[s][0])) for s in src]
            base = dev.alloc(dst_pad + len_x + SLACK, fill=FILL)
            areas.append((base, dst_pad, len_x))
            descs.append((0, out_len, first, len(src), window))
            lost.append((addrs[p], addrs[q], x, NONE, base + dst_pad, len_x, 0, 0))
        n = len(self.stripes)
        res = dev.alloc(16 * n, fill=FILL)
        queue.pq_rebuild_check(descs, sources, lost, res, windowed=windowed)
        raw = dev.get(res, 16 * n).view(np.uint64).reshape(n, 2)
        outs = [np.empty(dst_pad + len_x + SLACK, np.uint8) for _, dst_pad, len_x in areas]
        for (base, _, _), a in zip(areas, outs):
            queue.d2h(a, base, a.size)
        got = [np.empty(max(len(a), 1), np.uint8) for a, _ in self.ups]
        for g, ptr, (a, _) in zip(got, addrs, self.ups):
            if len(a):
                queue.d2h(g, ptr, len(a))
        queue.sync()
        for i, (g, (a, _)) in enumerate(zip(got, self.ups)):
            assert np.array_equal(g[:len(a)], a), f"upload {i} (a source or a body) changed on the device"
        result = []
        for i, ((_, dst_pad, len_x), a) in enumerate(zip(areas, outs)):
            for part, off0 in ((a[:dst_pad], -dst_pad), (a[dst_pad + len_x:], len_x)):
                w = np.flatnonzero(part != FILL)
                assert not w.size, (f"stripe {i}: byte at offset {off0 + int(w[0]) if w.size else 0} from dst_x "
                                    f"(len_x {len_x}) was overwritten")
            result.append((a[dst_pad:dst_pad + len_x], tuple(int(v) for v in raw[i])))
        return result


def assert_equal(got, want, what=""):
    assert len(got) == len(want)
    for i, ((go, gr), (wo, wr)) in enumerate(zip(got, want)):
        assert gr == wr, f"{what} stripe {i}: record {gr}, expected {wr}"
        if not np.array_equal(go, wo):
            w = np.flatnonzero(go != wo)
            raise AssertionError(f"{what} stripe {i}: {w.size} output bytes differ, first at {int(w[0])} "
                                 f"(got 0x{int(go[w[0]]):02x}, expected 0x{int(wo[w[0]]):02x})")


def make_stripe(b, rng, width, x, out_len, len_x, pad0=0, lens=None):
    """A clean stripe: random members (member x has len_x bytes), P and Q over all of them.  Returns the stripe's
    arguments (src, p, q) and the members."""
    if lens is None:
        lens = [int(v) for v in rng.integers(0, out_len + 1, size=width)]
        if width > 1:
            lens[(x + 1) % width] = out_len
    lens = list(lens)
    lens[x] = len_x
    chunks = [rng.integers(1, 256, size=L, dtype=np.uint8) for L in lens]
    p, q = G.p_of(chunks, out_len), G.q_sum(chunks, out_len)
    src = [None if k == x else b.up(c, (pad0 + 3 * k) % 16) for k, c in enumerate(chunks)]
    return src, b.up(p, (pad0 * 5 + 1) % 16), b.up(q, (pad0 * 11 + 8) % 16), chunks


@pytest.mark.parametrize("vecs", VECS)
def test_boundary_shapes_clean(bcp, engine, queue, dev, tuned, vecs):
    """len_x around the tile and lane sizes with out_len equal to and above it, every width and position of x,
    survivors longer than len_x, ending inside a tile below it, (0, 0) sources, unaligned pointers (bodies at an
    8-byte offset among them): the member comes back and every record is clean."""
    tuned("desc_vecs_per_thread", vecs)
    T = vecs * 4 * KiB
    rng = np.random.default_rng(40 + vecs)
    b = Batch()
    want = []
    i = 0
    for len_x in (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 5):
        for out_len in (len_x, len_x + T // 2 + 3):
            for width, x in (WIDTH_X[i % len(WIDTH_X)], WIDTH_X[(i * 5 + 7) % len(WIDTH_X)]):
                lens = None
                if width >= 5 and len_x > 64:
                    lens = [int(v) for v in rng.integers(0, out_len + 1, size=width)]
                    free = [k for k in range(width) if k != x]
                    lens[free[0]] = out_len + 37                 # longer than the bodies: cut
                    lens[free[1]] = (len_x - 40) // 16 * 16 + 5  # ends inside the last tile below len_x
                    lens[free[2]] = out_len                      # longer than len_x where out_len is
                src, p, q, chunks = make_stripe(b, rng, width, x, out_len, len_x, pad0=i, lens=lens)
                if width >= 5:
                    k0 = next(k for k in range(width) if k != x and (lens is None or k not in free[:3]))
                    src[k0] = None                               # the source (0, 0): rebuild P and Q without it
                    chunks[k0] = np.zeros(0, np.uint8)
                    b.ups[p] = (G.p_of(chunks, out_len), b.ups[p][1])
                    b.ups[q] = (G.q_sum(chunks, out_len), b.ups[q][1])
                if i % 4 == 1:
                    src[x] = b.up(np.zeros(0, np.uint8), 5)      # member x as an empty source at a valid address
                b.stripe(src, p, q, x, out_len, len_x, dst_pad=(i * 7) % 16)
                want.append((chunks[x], R.CLEAN))
                i += 1
    got = b.run(dev, queue)
    assert engine.option("last_desc_form") == 12 and engine.option("last_desc_vecs") == vecs
    assert_equal(got, b.refs(), "reference")
    assert_equal(got, want, "members")


@pytest.mark.parametrize("vecs", VECS)
def test_every_width_and_position(bcp, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    T = vecs * 4 * KiB
    rng = np.random.default_rng(50 + vecs)
    b = Batch()
    want = []
    for i, (width, x) in enumerate(WIDTH_X):
        src, p, q, chunks = make_stripe(b, rng, width, x, T + 301, T + 1, pad0=i)
        b.stripe(src, p, q, x, T + 301, T + 1, dst_pad=i % 16)
        want.append((chunks[x], R.CLEAN))
        # and the same stripe with one wrong byte in Q: (offset, 1) whatever the width
        q2 = b.ups[q][0].copy()
        q2[T] ^= FLIP
        b.stripe(src, p, b.up(q2, 8), x, T + 301, T + 1)
        want.append((chunks[x], (T, 1)))
    got = b.run(dev, queue)
    assert_equal(got, b.refs(), "reference")
    assert_equal(got, want, "members")


@pytest.mark.parametrize("vecs", VECS)
def test_faults_are_reported_and_the_output_is_the_plain_rebuild(bcp, queue, dev, tuned, vecs):
    """One flipped byte at a time, several in one tile and across two tiles, in a survivor, in P and in Q; bytes
    at or past len_x do not count.  dst_x is Ps cut to len_x whatever the record says."""
    tuned("desc_vecs_per_thread", vecs)
    T = vecs * 4 * KiB
    rng = np.random.default_rng(60 + vecs)
    width, x, len_x = 9, 4, 2 * T + 5
    out_len = len_x + 100
    lens = [out_len, len_x + 60, T + 9, 0, len_x, out_len, 700, out_len, len_x + 1]
    b = Batch()
    src, p, q, chunks = make_stripe(b, rng, width, x, out_len, len_x, lens=lens)
    b.stripe(src, p, q, x, out_len, len_x)
    want = [(chunks[x], R.CLEAN)]
    single = [0, len_x - 1, T - 1, T, 2 * T, 15, 16, 1023, 1024]
    several = [[5, 6, 700], [T - 1, T, T + 1], [0, len_x - 1], list(range(2 * T - 3, 2 * T + 5))]
    outside = [[len_x], [len_x + 50], [len_x, len_x + 59]]
    cases = []
    for z in (0, 1, 8, "p", "q"):
        for offs in [[o] for o in single] + several:
            cases.append((z, offs, True))
        for offs in outside if z != 8 else outside[:1]:  # (member 8 has one byte past len_x)
            cases.append((z, offs, False))
    cases.append((2, [T + 8], True))             # the last byte of a survivor that ends inside the second tile
    cases.append((6, [699], True))
    for z, offs, counts in cases:
        s2, p2, q2 = list(src), p, q
        member = b.ups[p if z == "p" else q if z == "q" else src[z]][0].copy()
        member[offs] ^= FLIP
        new = b.up(member, 8 if z in ("p", "q") else 3)
        if z == "p":
            p2 = new
        elif z == "q":
            q2 = new
        else:
            s2[z] = new
        b.stripe(s2, p2, q2, x, out_len, len_x)
        out = chunks[x].copy()
        if z != "q" and counts:
            out[offs] ^= FLIP                     # a wrong survivor or P byte goes into the member, as without Q
        want.append((out, (min(offs), len(offs)) if counts else R.CLEAN))
    got = b.run(dev, queue)
    assert_equal(got, b.refs(), "reference")
    assert_equal(got, want, "by hand")


@pytest.mark.parametrize("vecs", VECS)
def test_mixed_and_empty_batches(bcp, queue, dev, tuned, vecs):
    """Clean and faulty stripes around stripes without a tile: every record is written.  A batch without any
    tile still initialises its records."""
    tuned("desc_vecs_per_thread", vecs)
    T = vecs * 4 * KiB
    rng = np.random.default_rng(70 + vecs)
    b = Batch()
    want = []
    for i, (len_x, out_len, fault) in enumerate([(T + 3, T + 3, None), (0, 500, None), (3 * T, 3 * T + 1, 2 * T + 1),
                                                 (0, 0, None), (77, 200, 76), (T, 2 * T, None), (0, T + 1, None)]):
        src, p, q, chunks = make_stripe(b, rng, 5, i % 5, out_len, len_x, pad0=i)
        if fault is not None:
            k = (i + 1) % 5
            c = b.ups[src[k]][0].copy()
            c[fault] ^= FLIP
            src[k] = b.up(c, 1)
        b.stripe(src, p, q, i % 5, out_len, len_x)
        out = chunks[i % 5].copy()
        if fault is not None:
            out[fault] ^= FLIP
        want.append((out, (fault, 1) if fault is not None else R.CLEAN))
    got = b.run(dev, queue)
    assert_equal(got, b.refs(), "reference")
    assert_equal(got, want, "by hand")
    e = Batch()
    for i in range(3):
        src, p, q, _ = make_stripe(e, rng, 3, i, 300 * i, 0, pad0=i)
        e.stripe(src, p, q, i, 300 * i, 0)
    got = e.run(dev, queue)
    assert [r for _, r in got] == [R.CLEAN] * 3


@pytest.mark.parametrize("vecs", VECS)
@pytest.mark.parametrize("w", (32768, 65536))
def test_windowed_entry(bcp, engine, queue, dev, tuned, vecs, w):
    """Over window replay: a short x, a replayed survivor, and a fault in a survivor's last window, which counts
    at every place below len_x it is replayed to; a stripe without a window in the same batch keeps the plain
    semantics."""
    tuned("desc_vecs_per_thread", vecs)
    x, len_x = 4, 2 * w + 7
    lens = [3 * w, w + 3, 100, 0, len_x, w]
    out_len = 3 * w
    chunks = PW.chunks_of(lens, 80 + vecs)
    p, q = PW.p_win(chunks, w, out_len), PW.q_win(chunks, w, out_len)
    b = Batch()
    src = [None if k == x else b.up(c, (3 * k) % 16) for k, c in enumerate(chunks)]
    ip, iq = b.up(p, 8), b.up(q, 1)
    b.stripe(src, ip, iq, x, out_len, len_x, window=w)
    want = [(chunks[x], R.CLEAN)]
    for z, off, places in ((1, w + 1, [w + 1, 2 * w + 1]),    # home and one echo below len_x (the next is past it)
                           (1, 5, [5]),                       # not in its last window: no echo
                           (5, 6, [6, w + 6, 2 * w + 6]),     # a full window replayed twice
                           (5, 7, [7, w + 7]),                # its second echo is at len_x: does not count
                           (2, 99, [99, w + 99]),             # a source below one window: replayed too
                           (0, 2 * w + 6, [2 * w + 6])):
        assert [j for j in PW.replayed_places(lens[z], w, out_len, off) if j < len_x] == places
        c = chunks[z].copy()
        c[off] ^= FLIP
        s2 = list(src)
        s2[z] = b.up(c, 2)
        b.stripe(s2, ip, iq, x, out_len, len_x, window=w)
        out = chunks[x].copy()
        out[places] ^= FLIP
        want.append((out, (places[0], len(places))))
    # window 0 in the windowed batch: plain zero padding
    rng = np.random.default_rng(90)
    src0, p0, q0, ch0 = make_stripe(b, rng, 5, 2, 40000, 33000)
    b.stripe(src0, p0, q0, 2, 40000, 33000)
    want.append((ch0[2], R.CLEAN))
    bad = b.ups[src0[3]][0].copy()                            # (the member make_stripe gives out_len bytes)
    bad[32999] ^= FLIP
    b.stripe(src0[:3] + [b.up(bad)] + src0[4:], p0, q0, 2, 40000, 33000)
    out = ch0[2].copy()
    out[32999] ^= FLIP
    want.append((out, (32999, 1)))
    got = b.run(dev, queue, windowed=True)
    assert engine.option("last_desc_form") == 13 and engine.option("last_desc_vecs") == vecs
    assert_equal(got, b.refs(), "reference")
    assert_equal(got, want, "by hand")


def test_windowed_entry_without_a_window_is_the_plain_launch(bcp, engine, queue, dev):
    rng = np.random.default_rng(91)
    b = Batch()
    src, p, q, chunks = make_stripe(b, rng, 3, 1, 5000, 4000)
    b.stripe(src, p, q, 1, 5000, 4000)
    got = b.run(dev, queue, windowed=True)
    assert engine.option("last_desc_form") == 12
    assert_equal(got, [(chunks[1], R.CLEAN)])


def test_validation(bcp, queue, dev):
    body = dev.put(np.zeros(4096, np.uint8))
    data = dev.put(np.ones(4096, np.uint8))
    out = dev.alloc(4096, fill=FILL)
    res = dev.alloc(16, fill=FILL)
    good_src = [(data, 4096), (0, 0), (data, 100)]

    def rc(lost, sources=good_src, stripe=(0, 4096, 0, 3, 0), windowed=False):
        try:
            queue.pq_rebuild_check([stripe], sources, [lost], res, windowed=windowed)
        except bcp.BcpError as e:
            return e.rc
        return 0

    ok = (body, body, 1, NONE, out, 4096, 0, 0)
    for windowed in (False, True):
        assert rc((body, body, 1, 2, out, 4096, out, 10), windowed=windowed) == -errno.EINVAL       # y != NONE
        assert rc((0, body, 1, NONE, out, 4096, 0, 0), windowed=windowed) == -errno.EINVAL           # P is lost
        assert rc((body, 0, 1, NONE, out, 4096, 0, 0), windowed=windowed) == -errno.EINVAL           # no Q body
        assert rc(ok, sources=[(data, 4096), (data, 1), (data, 100)], windowed=windowed) == -errno.EINVAL  # x has bytes
        assert rc((body, body, 3, NONE, out, 4096, 0, 0), windowed=windowed) == -errno.EINVAL        # x >= nsrc
        assert rc((body, body, 1, NONE, out, 4097, 0, 0), windowed=windowed) == -errno.EINVAL        # len_x > out_len
        assert rc((body, body, 1, NONE, 0, 4096, 0, 0), windowed=windowed) == -errno.EINVAL          # no dst_x
    assert rc(ok, stripe=(0, 4096, 0, 3, 32768)) == -errno.EINVAL                                    # a window, plain entry
    assert rc(ok, stripe=(0, 4096, 0, 3, 16384), windowed=True) == -errno.EINVAL                     # not a multiple of 32768
    queue.sync()
    assert np.all(dev.get(out, 4096) == FILL) and np.all(dev.get(res, 16) == FILL)                  # nothing ran
    assert rc(ok) == 0 and rc(ok, stripe=(0, 4096, 0, 3, 32768), windowed=True) == 0
    queue.sync()


def test_recover_still_refuses_p_present_one_lost(bcp, queue, dev):
    """The neighbour is unchanged: the combination the new call takes is still -EINVAL there."""
    body = dev.put(np.zeros(256, np.uint8))
    out = dev.alloc(256, fill=FILL)
    for windowed in (False, True):
        with pytest.raises(bcp.BcpError) as e:
            queue.pq_recover([(0, 256, 0, 2, 0)], [(body, 256), (0, 0)], [(body, body, 1, NONE, out, 256, 0, 0)],
                             windowed=windowed)
        assert e.value.rc == -errno.EINVAL
    queue.sync()
    assert np.all(dev.get(out, 256) == FILL)
