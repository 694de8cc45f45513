"""Self-test of the device-test harness (tests/devbuf.py) on a numpy fake of
the engine and queue: the real Dev and gpu_stripes run against a plain numpy
xor_stripes, which passes when correct and is caught -- with the right stripe
and offset -- for each class of kernel defect injected into it: a byte stored
past out_len, a byte stored before dst, a source read past its end, the
stores of an all-padding region skipped, an output left unwritten.  This
stands in for running mutant kernels on the device."""
import numpy as np
import pytest

from devbuf import CANARY, FILL, GUARD, POISON, SLACK, Dev, GuardError, assert_stripes_equal, gpu_stripes

BASE = 0x7F0000000000


class FakeEngine:
    """Device memory as one numpy array, zero when fresh (as device memory
    usually is); alloc bumps a 256-byte aligned offset."""

    def __init__(self, nbytes=8 << 20):
        self.mem = np.zeros(nbytes, dtype=np.uint8)
        self.off = 4096
        self.live = {}

    def alloc(self, n):
        p = self.off
        self.off = (p + n + 255) // 256 * 256 + 256
        assert self.off <= self.mem.size
        self.live[BASE + p] = n
        return BASE + p

    def free(self, ptr):
        del self.live[ptr]

    def queue(self):
        return FakeQueue(self)


class FakeQueue:
    def __init__(self, eng):
        self.eng, self.mem = eng, eng.mem
        self.defect = None        # (kind, stripe)

    def sync(self):
        pass

    def h2d(self, dptr, host, nbytes=None):
        host = np.asarray(host, dtype=np.uint8).reshape(-1)
        n = host.size if nbytes is None else nbytes
        self.mem[dptr - BASE:dptr - BASE + n] = host[:n]

    def d2h(self, host, dptr, nbytes=None):
        n = host.size if nbytes is None else nbytes
        host.reshape(-1)[:n] = self.mem[dptr - BASE:dptr - BASE + n]

    def d2d(self, dst, src, nbytes):
        self.mem[dst - BASE:dst - BASE + nbytes] = self.mem[src - BASE:src - BASE + nbytes].copy()

    def memset(self, dptr, value, nbytes):
        self.mem[dptr - BASE:dptr - BASE + nbytes] = value

    def xor_stripes(self, stripes, sources):
        """The zero-padded XOR in plain numpy, with one optional defect."""
        for i, (dst, out_len, first, nsrc, window) in enumerate(stripes):
            assert window == 0
            kind = self.defect[0] if self.defect and self.defect[1] == i else None
            d = dst - BASE
            out = np.zeros(out_len, dtype=np.uint8)
            longest = 0
            for ptr, ln in sources[first:first + nsrc]:
                take = min(ln, out_len)
                if kind == "read_past" and ln < out_len:
                    take = ln + 1  # no check against the source's length for its last vector
                if take:
                    out[:take] ^= self.mem[ptr - BASE:ptr - BASE + take]
                longest = max(longest, take)
            if kind == "unwritten":
                continue
            if kind == "skip_padding":
                out_len = longest  # tiles that no source reaches are never stored
            self.mem[d:d + out_len] = out[:out_len]
            if kind == "store_past":
                self.mem[d + out_len] = 0  # a whole vector stored where a partial one was due
            if kind == "store_past_slack":
                self.mem[d + out_len + SLACK] = 0
            if kind == "store_before":
                self.mem[d - 1] = 0


@pytest.fixture
def fake():
    eng = FakeEngine()
    q = eng.queue()
    return eng, q, Dev(eng, q, slab_bytes=1 << 20)


def batch(seed=1, dst_pad=3):
    """Three stripes; stripe 1 has sources shorter than its output (two of the
    same length) and an output longer than all of them."""
    rng = np.random.default_rng(seed)
    shapes = [([100, 37], 100), ([64, 64, 200], 333), ([48, 0, 17], 48)]
    stripes, refs = [], []
    for lens, out_len in shapes:
        chunks = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in lens]
        stripes.append(dict(chunks=chunks, out_len=out_len, pads=[int(x) for x in rng.integers(0, 16, size=len(lens))],
                            dst_pad=dst_pad))
        ref = np.zeros(out_len, dtype=np.uint8)
        for c in chunks:
            ref[:len(c)] ^= c
        refs.append(ref)
    return stripes, refs


def test_correct_fold_passes_and_everything_is_freed(fake):
    eng, q, dev = fake
    stripes, refs = batch()
    stripes.append(dict(chunks=[None, np.zeros(0, np.uint8)], out_len=20))  # (0, 0) and an empty chunk at an address
    refs.append(np.zeros(20, np.uint8))
    big = dev.alloc(600_000, fill=FILL)  # above a quarter slab: an allocation of its own
    assert len(dev.big) == 1 and (eng.mem[big - BASE:big - BASE + 600_000] == FILL).all()
    assert_stripes_equal(gpu_stripes(dev, q, stripes), refs)
    dev.free()
    assert not eng.live


def test_buffers_are_aligned_guarded_and_poisoned(fake):
    eng, q, dev = fake
    p = dev.alloc(100)
    assert p % 256 == 0
    m = eng.mem
    assert (m[p - BASE - GUARD:p - BASE] == CANARY).all() and (m[p - BASE + 100:p - BASE + 100 + GUARD] == CANARY).all()
    a = np.arange(1, 51, dtype=np.uint8)
    pa, pb, pe = dev.put(a, 5), dev.put(a, 5), dev.put(np.zeros(0, np.uint8), 9)
    assert pa % 256 == 5 and pe % 256 == 9 and pe != 0
    for ptr, n in ((pa, 50), (pb, 50), (pe, 0)):
        o = ptr - BASE
        assert np.array_equal(m[o:o + n], a[:n])
        assert m[o - POISON:o].all() and m[o + n:o + n + POISON].all()  # never zero next to the chunk
    after = [m[ptr - BASE + n:ptr - BASE + n + POISON].copy() for ptr, n in ((pa, 50), (pb, 50), (pe, 0))]
    assert not np.array_equal(after[0], after[1]) and not np.array_equal(after[1], after[2])  # and never the same
    assert len(set(int(x[0]) for x in after)) == 3  # the very next byte differs too (this seed)
    dev.free()


def test_large_uploads_keep_guards_and_poison_whatever_follows(fake):
    """Chunks above the one-copy size: the upper poison's copy runs on into
    the next buffer's first bytes.  Whatever is carved next -- another large
    upload, a small one, a plain buffer smaller than that look-ahead, a large
    buffer of its own -- every chunk is intact, poisoned on both sides, and
    every guard is whole."""
    eng, q, dev = fake
    m = eng.mem
    rng = np.random.default_rng(3)
    ups = []
    for n, pad, then in ((70_000, 0, None), (66_001, 7, None), (100_003, 15, "small"), (65_537, 1, "tiny"),
                         (80_000, 3, "big"), (70_001, 9, "filled"), (200_000, 5, None),
                         (300_000, 4, None)):  # the last one: an allocation of its own
        a = rng.integers(0, 256, size=n, dtype=np.uint8)
        ups.append((dev.put(a, pad), a, pad))
        if then == "small":
            b = rng.integers(0, 256, size=10, dtype=np.uint8)
            ups.append((dev.put(b, 2), b, 2))
        elif then == "tiny":
            p = dev.alloc(16)
            assert (m[p - BASE - GUARD:p - BASE + 16 + GUARD] == CANARY).all()
        elif then == "big":
            dev.alloc(600_000)
        elif then == "filled":
            p = dev.alloc(40, fill=FILL)
            assert (m[p - BASE:p - BASE + 40] == FILL).all() and (m[p - BASE + 40:p - BASE + 40 + GUARD] == CANARY).all()
    # and a mixed batch: the small ones in one copy, the large ones after them
    items = [(rng.integers(0, 256, size=n, dtype=np.uint8), pad)
             for n, pad in ((90_000, 3), (100, 5), (0, 11), (70_000, 0), (65_536, 1), (65_537, 2))]
    ups += [(ptr, a, pad) for ptr, (a, pad) in zip(dev.put_many(items), items)]
    for ptr, a, pad in ups:
        o = ptr - BASE
        assert ptr % 256 == pad and np.array_equal(m[o:o + a.size], a)
        assert m[o - POISON:o].all() and m[o + a.size:o + a.size + POISON].all()
        assert (m[o - POISON - pad - GUARD:o - POISON - pad] == CANARY).all()
        assert (m[o + a.size + POISON:o + a.size + POISON + GUARD] == CANARY).all()
    dev.free()
    assert not eng.live


@pytest.mark.parametrize("kind,offset", [("store_past", 333), ("store_before", -1)])
def test_stray_store_next_to_the_output_names_stripe_and_offset(fake, kind, offset):
    eng, q, dev = fake
    stripes, _ = batch()
    q.defect = (kind, 1)
    with pytest.raises(GuardError, match=rf"stripe 1: byte at offset {offset} from dst \(out_len 333\)"):
        gpu_stripes(dev, q, stripes)
    dev.free()  # the stray byte lay inside the destination area: the guards are whole
    assert not eng.live


@pytest.mark.parametrize("kind,dst_pad,where,offset", [("store_before", 0, "below", -1),
                                                       ("store_past_slack", 3, "above", 3 + 333 + SLACK)])
def test_stray_store_outside_the_area_is_caught_by_the_guards_after_freeing(fake, kind, dst_pad, where, offset):
    eng, q, dev = fake
    stripes, refs = batch(dst_pad=dst_pad)
    q.defect = (kind, 1)
    assert_stripes_equal(gpu_stripes(dev, q, stripes), refs)  # the output itself is right
    n = dst_pad + 333 + SLACK
    with pytest.raises(GuardError, match=rf"\({n} bytes\): guard {where} it changed at offset {offset} \(found 0x00, 1 "):
        dev.free()
    assert not eng.live and not dev.slabs  # freed before the failure was raised


def test_stray_store_next_to_a_large_allocation(fake):
    eng, q, dev = fake
    p = dev.alloc(600_000)
    eng.mem[p - BASE + 600_000] = 1
    eng.mem[p - BASE - GUARD] = 2
    with pytest.raises(GuardError) as e:
        dev.free()
    assert "offset 600000 (found 0x01" in str(e.value) and f"offset {-GUARD} (found 0x02" in str(e.value)
    assert not eng.live


def test_source_read_past_its_end_is_caught(fake):
    """Sources 0 and 1 of stripe 1 have the same length and both read one
    byte too many: constant poison would cancel, random poison does not."""
    eng, q, dev = fake
    stripes, refs = batch()
    q.defect = ("read_past", 1)
    outs = gpu_stripes(dev, q, stripes)
    with pytest.raises(AssertionError, match=r"stripe 1: 2 bytes differ, first at offset 64 "):
        assert_stripes_equal(outs, refs)
    dev.free()


def test_source_read_past_its_end_needs_the_poison():
    """The same defect over sources uploaded the old way (zero bytes after the
    chunk) passes: what the poison is for."""
    eng = FakeEngine()
    q = eng.queue()
    dev = Dev(eng, q, slab_bytes=1 << 20)
    stripes, refs = batch()
    q.defect = ("read_past", 1)
    real_put_many = dev.put_many

    def put_many_zero_slack(items):
        addrs = real_put_many(items)
        for p, (arr, _) in zip(addrs, items):
            q.memset(p + len(arr), 0, 16)
        return addrs
    dev.put_many = put_many_zero_slack
    assert_stripes_equal(gpu_stripes(dev, q, stripes), refs)
    dev.free()


@pytest.mark.parametrize("kind,offset,n", [("skip_padding", 200, 133), ("unwritten", 0, 333)])
def test_skipped_stores_are_caught(fake, kind, offset, n):
    """Stripe 1's bytes past its longest source (200) are zero: over fresh,
    zero memory a skipped store would pass; over the 0xA5 pre-fill it fails."""
    eng, q, dev = fake
    stripes, refs = batch()
    q.defect = (kind, 1)
    outs = gpu_stripes(dev, q, stripes)
    with pytest.raises(AssertionError, match=rf"stripe 1: \d+ bytes differ, first at offset {offset} \(got 0xa5"):
        assert_stripes_equal(outs, refs)
    assert (outs[1][offset:] == FILL).sum() == n
    dev.free()
