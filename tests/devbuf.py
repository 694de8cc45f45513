"""Guarded device buffers for the kernel tests.

Everything here talks to the device only through an engine's alloc / free and
a queue's h2d / d2h / d2d / memset / sync / xor_stripes, so the same code runs on a
numpy fake (test_guard_harness_cpu.py) and shows there which kernel defects it
catches:

  * Dev.alloc puts a canary guard below and above every buffer and Dev.free
    reads all of them back: a store before a buffer or past its end fails the
    test that made it.
  * Dev.put surrounds an uploaded chunk with random non-zero poison: a load
    before a source or past its end folds garbage into the output instead of
    the zeros that fresh device memory usually holds.
  * gpu_stripes pre-fills each stripe's destination area with 0xA5 and checks
    every byte of it around [dst, dst + out_len) afterwards: a skipped store
    shows even where the expected byte is zero, a stray one at byte
    granularity.
"""
import numpy as np

MiB = 1024 * 1024
GUARD = 256        # canary bytes below and above every allocation (a multiple of 256: pointers stay 256-byte aligned)
CANARY = 0xC7
POISON = 256       # random bytes before and after an uploaded chunk
FILL = 0xA5        # what an output area holds before the fold
SLACK = 32         # bytes of a stripe's destination area past out_len
SLAB = 64 * MiB    # small buffers are carved from slabs of this size (one malloc / free and one read-back for many)
PRE = POISON + 16  # look-ahead poison: the lower poison of an upload at any pad (0..15)
POOL = 256 * 1024  # poison bytes drawn at a time
CONCAT_MAX = 64 * 1024  # chunks up to this size travel with their poison in one copy (larger: three copies, no host copy)


_CANARIES = np.full(3 * GUARD, CANARY, dtype=np.uint8)


class GuardError(AssertionError):
    pass


class Dev:
    """Scratch device allocations freed at test end, each between two canary
    guards that free() checks."""

    def __init__(self, eng, q, slab_bytes=SLAB, seed=0x5EED):
        self.eng, self.q, self.slab_bytes = eng, q, slab_bytes
        self.rng = np.random.default_rng(seed)
        self.slabs = []   # [base, used, [(index, slot offset, n)]]
        self.big = []     # (index, slot base, n, slot bytes)
        self.count = 0
        self._keep = []   # host buffers of copies in flight
        self._pool, self._pool_at = np.empty(0, dtype=np.uint8), 0
        self._pre, self._lo_done, self._room = 0, False, 0  # put's look-ahead poison (address of the body it lies in)

    def alloc(self, n, fill=None, _put=False):
        """n bytes at a 256-byte aligned address, GUARD canary bytes directly
        below and at least GUARD directly above; fill: pre-set the n bytes (on
        the queue) so that a store that never happens shows."""
        slot = (2 * GUARD + n + 255) // 256 * 256
        idx, self.count = self.count, self.count + 1
        self._room, self._lo_done = 0, False  # bytes of the slab after this slot; lower poison already there
        if slot > self.slab_bytes // 4:
            base = self.eng.alloc(slot)
            self.big.append((idx, base, n, slot))
            self.q.memset(base, CANARY, GUARD)
            self.q.memset(base + GUARD + n, CANARY, slot - GUARD - n)
            self.q.sync()
        else:
            if not self.slabs or self.slabs[-1][1] + slot > self.slab_bytes:
                sbase = self.eng.alloc(self.slab_bytes)
                self.slabs.append([sbase, 0, []])
                self.q.memset(sbase, CANARY, self.slab_bytes)
                self.q.sync()  # other queues and the ring may use the memory next
            slab = self.slabs[-1]
            base = slab[0] + slab[1]
            slab[2].append((idx, slab[1], n))
            slab[1] += slot
            self._room = self.slab_bytes - slab[1]
            pre, self._pre = self._pre, 0
            self._lo_done = _put and pre == base + GUARD
            if pre == base + GUARD and not _put:
                self.q.memset(pre, CANARY, PRE)  # put's look-ahead poison: this is no upload after all
        if fill is not None and n:
            self.q.memset(base + GUARD, fill, n)
        return base + GUARD

    def put(self, arr, pad=0):
        """Upload [poison | arr | poison] with arr at byte offset `pad` from a
        256-byte boundary; returns arr's device address (valid, and poisoned
        around, for an empty arr too).

        The poison is drawn from an rng, new for every upload and never zero.
        Zero would hide an over-read (the kernel's padding is zero), and so
        would any constant: two sources of one stripe that both read the same
        constant past their ends cancel in the XOR.  Any over-read starts at
        the chunk's end, so a few hundred bytes per side catch it."""
        arr = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1)
        lo, n = POISON + pad, arr.size
        base = self.alloc(lo + n + POISON, _put=True)
        p = self._poison(lo + POISON)
        plo, phi = p[:lo], p[lo:]
        if n <= CONCAT_MAX:
            host = np.concatenate([plo, arr, phi])
            self.q.h2d(base, host)
            self._keep.append(host)
            return base + lo
        # a large chunk travels as it is, its poison in small copies of its
        # own.  The upper poison's copy goes on over the guards that follow to
        # the first PRE bytes of the slab's next buffer: if that is an upload
        # too, its lower poison is there already (alloc puts the canary back
        # if it is not) -- one small copy per large chunk instead of two.
        if not self._lo_done:
            self.q.h2d(base, plo)
            self._keep.append(plo)
        self.q.h2d(base + lo, arr)
        end = base + lo + n + POISON               # the body's end; the slot's: the next 256-byte boundary + GUARD
        gap = (-(end - GUARD) % 256) + 2 * GUARD   # this buffer's upper guard and the next one's lower
        if self._room >= gap + PRE:
            tail = np.concatenate([phi, _CANARIES[:gap], self._poison(PRE)])
            self._pre = end + gap
        else:
            tail = phi
        self.q.h2d(base + lo + n, tail)
        self._keep += [arr, tail]
        return base + lo

    def put_many(self, items):
        """put() for a list of (arr, pad): the same layout and poison, but the
        small chunks, which lie one after the other in a slab, travel in one
        copy per slab (their guards between them rewritten with the canary)
        instead of one each -- a fuzz batch has hundreds."""
        addrs = [0] * len(items)
        run, run_slab = [], None  # (body address, host bytes) of consecutive small uploads

        def flush():
            if run:
                start = run[0][0]
                host = np.full(run[-1][0] + run[-1][1].size - start, CANARY, dtype=np.uint8)
                for a, h in run:
                    host[a - start:a - start + h.size] = h
                self.q.h2d(start, host)
                self._keep.append(host)
                del run[:]

        for i, (arr, pad) in enumerate(items):
            arr = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1)
            if arr.size > CONCAT_MAX:
                continue
            lo = POISON + pad
            base = self.alloc(lo + arr.size + POISON, _put=True)
            if self.slabs[-1][0] != run_slab:
                flush()
                run_slab = self.slabs[-1][0]
            p = self._poison(lo + POISON)
            run.append((base, np.concatenate([p[:lo], arr, p[lo:]])))
            addrs[i] = base + lo
        flush()
        for i, (arr, pad) in enumerate(items):
            if not addrs[i]:
                addrs[i] = self.put(arr, pad)
        return addrs

    def _poison(self, n):
        """n random non-zero bytes, never handed out before: consecutive
        slices of a pool that is drawn afresh when it runs out (one draw per
        upload would cost the fuzz more than the upload)."""
        if self._pool_at + n > self._pool.size:
            self._pool = self.rng.integers(1, 256, size=max(POOL, n), dtype=np.uint8)
            self._pool_at = 0
        self._pool_at += n
        return self._pool[self._pool_at - n:self._pool_at]

    def get(self, ptr, n):
        out = np.empty(max(n, 1), dtype=np.uint8)
        if n:
            self.q.d2h(out, ptr, n)
        self.q.sync()
        self._keep = []
        return out[:n]

    def _check(self, idx, n, lo, hi, bad):
        for name, g, off0 in (("below", lo, -GUARD), ("above", hi, n)):
            if g.tobytes().count(CANARY) == g.size:  # the quick look: thousands of guards per fuzz round
                continue
            w = np.flatnonzero(g != CANARY)
            if w.size:
                bad.append(f"allocation #{idx} ({n} bytes): guard {name} it changed at offset {off0 + int(w[0])} "
                           f"(found 0x{int(g[w[0]]):02x}, {w.size} guard bytes changed)")

    def free(self):
        """Sync, read every guard back, free everything, then raise if a guard
        byte changed (after the frees: a failure leaks nothing into later tests)."""
        bad = []
        own = None
        try:
            self.q.sync()
            # a slab's guards lie back to back (one buffer's upper, the next
            # one's lower): each such run is copied into a staging buffer on
            # the device and all come back in one copy, without the buffers'
            # own bytes between them
            runs = []  # (device address, length)
            for sbase, used, allocs in self.slabs:
                edges = [0] + [x for _, off, n in allocs for x in (off + GUARD, off + GUARD + n)] + [used]
                runs += [(sbase + edges[i], edges[i + 1] - edges[i]) for i in range(0, len(edges), 2)]
            total = sum(ln for _, ln in runs)
            if total:
                if self.slab_bytes - self.slabs[-1][1] >= total:
                    stage = self.slabs[-1][0] + self.slabs[-1][1]  # the last slab's unused end
                else:
                    stage = own = self.eng.alloc(total)
                at = 0
                for addr, ln in runs:
                    self.q.d2d(stage + at, addr, ln)
                    at += ln
                buf = np.empty(total, dtype=np.uint8)
                self.q.d2h(buf, stage, total)
                self.q.sync()
                at = 0
                for sbase, used, allocs in self.slabs:
                    for i, (idx, off, n) in enumerate(allocs):
                        end = allocs[i + 1][1] if i + 1 < len(allocs) else used
                        hi_len = end - (off + GUARD + n)
                        self._check(idx, n, buf[at:at + GUARD], buf[at + GUARD:at + GUARD + hi_len], bad)
                        at += GUARD + hi_len
            for idx, base, n, slot in self.big:
                lo, hi = np.empty(GUARD, dtype=np.uint8), np.empty(slot - GUARD - n, dtype=np.uint8)
                self.q.d2h(lo, base, lo.size)
                self.q.d2h(hi, base + GUARD + n, hi.size)
                self.q.sync()
                self._check(idx, n, lo, hi, bad)
        finally:
            slabs, big = self.slabs, self.big
            self.slabs, self.big, self._keep = [], [], []
            if own is not None:
                self.eng.free(own)
            for s in slabs:
                self.eng.free(s[0])
            for b in big:
                self.eng.free(b[1])
        if bad:
            raise GuardError("device guard bytes overwritten:\n  " + "\n  ".join(bad[:8]))


def gpu_stripes(dev, queue, stripes):
    """stripes: list of dict(chunks=[np arrays or None], out_len, window, pads, dst_pad) -> list of outputs.

    A chunk given as None is the source (0, 0); an empty array is a source of
    length 0 at a valid, poisoned address.  Each stripe's destination area
    (dst_pad bytes, out_len, SLACK) holds 0xA5 before the fold; afterwards
    every byte before dst and from dst + out_len on must still be 0xA5."""
    descs, sources, areas = [], [], []
    ups = [(c, pad) for st in stripes
           for c, pad in zip(st["chunks"], st.get("pads") or [0] * len(st["chunks"])) if c is not None]
    addrs = iter(dev.put_many(ups))
    for st in stripes:
        first = len(sources)
        for c in st["chunks"]:
            sources.append((0, 0) if c is None else (next(addrs), len(c)))
        dst_pad, out_len = st.get("dst_pad", 0), st["out_len"]
        base = dev.alloc(dst_pad + out_len + SLACK, fill=FILL)
        areas.append((base, dst_pad, out_len))
        descs.append((base + dst_pad, out_len, first, len(st["chunks"]), st.get("window", 0)))
    queue.xor_stripes(descs, sources)
    queue.sync()
    got = [np.empty(dst_pad + out_len + SLACK, dtype=np.uint8) for _, dst_pad, out_len in areas]
    for (base, _, _), area in zip(areas, got):
        queue.d2h(area, base, area.size)
    queue.sync()
    outs = []
    for i, ((base, dst_pad, out_len), area) in enumerate(zip(areas, got)):
        for part, off0 in ((area[:dst_pad], -dst_pad), (area[dst_pad + out_len:], out_len)):
            w = np.flatnonzero(part != FILL)
            if w.size:
                raise GuardError(f"stripe {i}: byte at offset {off0 + int(w[0])} from dst (out_len {out_len}) was "
                                 f"overwritten with 0x{int(part[w[0]]):02x}; {w.size} bytes outside the output changed")
        outs.append(area[dst_pad:dst_pad + out_len])
    return outs


def assert_stripes_equal(outs, refs, what=""):
    """Every output equal to its reference, or a failure naming the stripe and
    the first differing offset."""
    assert len(outs) == len(refs)
    for i, (o, r) in enumerate(zip(outs, refs)):
        assert len(o) == len(r), (what, i, len(o), len(r))
        if not np.array_equal(o, r):
            w = np.flatnonzero(o != r)
            raise AssertionError(f"{what} stripe {i}: {w.size} bytes differ, first at offset {int(w[0])} "
                                 f"(got 0x{int(o[w[0]]):02x}, expected 0x{int(r[w[0]]):02x})")
