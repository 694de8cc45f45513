"""The computing forms of the CPU stand-in for the device (tests/native/hipdouble/)
against the numpy references of the suite: the byte loops of the stand-in have
to be right before its silence about the pipeline means anything.

Run as a program by tests/test_hipdouble_cpu.py with BCP_LIB naming
libbcp_double.so (tools/hipdouble_pipeline.sh builds it: libbcp's host code
over the stand-in, no sanitizer), so that bcp_ctypes drives the engine's public
entry points and every launch lands in the stand-in:

    xor_stream, plain and gather     oracle.xor_padded_np
    desc_tiles + xor_desc, windows   oracle.gen_parity_file (the reference's replay)
    xor_desc_args                    oracle.xor_padded_np
    check_init + check_desc          a body with known wrong bytes
    pq GEN, SOLVE                    gf256.p_of / q_sum, the lost members themselves
    pq_check_init + pq_check         the syndromes by definition
    pq_win forms 0 .. 2              pq_window.p_win / q_win

Shapes: lengths 0, 1, 15, 16, 17, one tile - 1, one tile, one tile + 1 and two
tiles + 1 for tiles of U = 2, 4 and 8 vectors per lane (4096 * U bytes), widths
1, 2, 8, 9 and 56, and a window of 32 KiB with sources of 1, 2 and 2.5 windows.
Prints "forms: N checks, 0 wrong" and exits 0, or lists what was wrong."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "beegfs-chunk-parity_amd"), os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import bcp_ctypes as B  # noqa: E402
import gf256 as G  # noqa: E402
import oracle as O  # noqa: E402
import pq_window as PW  # noqa: E402

KiB = 1024
W = 32 * KiB
WIDTHS = (1, 2, 8, 9, 56)
US = (2, 4, 8)
BAD_P, BAD_Q, BAD_NOWHERE = 1 << 56, 1 << 57, 1 << 58
CHECK = np.dtype([("first_bad", "<u8"), ("bad_bytes", "<u8")])
PQCHECK = np.dtype([("first_bad", "<u8"), ("p_bad", "<u8"), ("q_bad", "<u8"), ("members", "<u8")])
NONE = 2 ** 64 - 1

checks = 0
wrong = []


def expect(what, got, want):
    global checks
    checks += 1
    if not np.array_equal(np.asarray(got), np.asarray(want)):
        wrong.append(what)


def lengths(u):
    t = 4096 * u
    return [0, 1, 15, 16, 17, t - 1, t, t + 1, 2 * t + 1]


class Arena:
    """Device memory of one batch: rows at 256-byte pitch."""

    def __init__(self, eng, q, nbytes):
        self.eng, self.q, self.cap = eng, q, nbytes + 4096
        self.base = eng.alloc(self.cap)
        self.off = 0

    def room(self, n):
        a = self.base + self.off
        self.off += (n + 255) // 256 * 256 + 256
        assert self.off <= self.cap
        return a

    def put(self, arr):
        a = self.room(len(arr))
        if len(arr):
            self.q.h2d(a, np.ascontiguousarray(arr, dtype=np.uint8))
        return a

    def get(self, addr, n, dtype=np.uint8):
        out = np.zeros(max(n, 1), dtype=dtype)
        self.q.d2h(out, addr, n * np.dtype(dtype).itemsize)
        self.q.sync()
        return out[:n]

    def close(self):
        self.q.sync()
        self.eng.free(self.base)


def stripe_chunks(rng, out_len, width, full=False):
    """width sources for an output of out_len: the first as long as the output, the others
    shorter at random (full: all as long), one of them empty when there are three or more."""
    lens = [out_len] + [out_len if full else int(rng.integers(0, out_len + 1)) for _ in range(width - 1)]
    if width >= 3 and not full:
        lens[2] = 0
    return [rng.integers(0, 256, size=n, dtype=np.uint8) for n in lens]


def size_of(batches):
    return sum((len(c) + 512) for chunks in batches for c in chunks) + sum(
        2 * (max(len(c) for c in chunks) + 512) for chunks in batches)


def describe(ar, batches, window=0, with_dst=True):
    """Upload every stripe's sources; returns (stripes, sources, dst addresses)."""
    st, so, dsts = [], [], []
    for chunks in batches:
        out_len = max(len(c) for c in chunks)
        first = len(so)
        for c in chunks:
            so.append((ar.put(c) if len(c) else 0, len(c)))
        d = ar.room(out_len) if with_dst else 0
        dsts.append(d)
        st.append((d, out_len, first, len(chunks), window))
    return st, so, dsts


def xor_forms(eng, q, rng):
    for u in US:
        for width in WIDTHS:
            tag = f"U={u} width={width}"
            # xor_stream, plain: the strided entry point with aligned strides (any length: a byte tail)
            eng.option("vecs_per_thread", u)
            for n in lengths(u):
                if n == 0:
                    continue  # nothing is launched for it
                pitch = (n + 15) // 16 * 16
                data = rng.integers(0, 256, size=(3, width, pitch), dtype=np.uint8)
                ar = Arena(eng, q, data.size + 3 * pitch + 1024)
                src = ar.put(data.reshape(-1))
                dst = ar.room(3 * pitch)
                q.xor_strided(dst, pitch, src, width * pitch, pitch, 3, width, n)
                got = ar.get(dst, 3 * pitch).reshape(3, pitch)[:, :n]
                expect(f"xor_stream {tag} len={n}", got, np.bitwise_xor.reduce(data[:, :, :n], axis=1))
                ar.close()
            # xor_stream, gather: a uniform descriptor batch
            for n in lengths(u):
                if n == 0:
                    continue
                batches = [stripe_chunks(rng, n, width, full=True) for _ in range(3)]
                ar = Arena(eng, q, size_of(batches))
                st, so, dsts = describe(ar, batches)
                q.xor_stripes(st, so)
                for s, chunks in enumerate(batches):
                    expect(f"xor_stream gather {tag} len={n}", ar.get(dsts[s], n), O.xor_padded_np(chunks))
                ar.close()
            # the descriptor forms: one stripe per length, ragged sources
            eng.option("desc_vecs_per_thread", u)
            batches = [stripe_chunks(rng, n, width) for n in lengths(u)]
            for form, args_max in (("xor_desc_args", 16), ("desc_tiles + xor_desc", 0)):
                if form == "xor_desc_args" and width > 8:
                    continue  # more than 8 sources per stripe never travel in the arguments
                eng.option("desc_args_max", args_max)
                ar = Arena(eng, q, size_of(batches))
                st, so, dsts = describe(ar, batches)
                q.xor_stripes(st, so)
                want_form = 2 if form == "xor_desc_args" else 1
                expect(f"{form} {tag}: the form taken", eng.option("last_desc_form"), want_form)
                for s, chunks in enumerate(batches):
                    expect(f"{form} {tag} len={st[s][1]}", ar.get(dsts[s], st[s][1]), O.xor_padded_np(chunks))
                # check_init + check_desc over the same stripes: clean, then with wrong bytes planted
                res = ar.room(len(st) * CHECK.itemsize)
                q.check_stripes(st, so, res)
                got = ar.get(res, len(st), CHECK)
                expect(f"check_desc {tag} clean", got.tolist(), [(NONE, 0)] * len(st))
                want = []
                for s, chunks in enumerate(batches):
                    n = st[s][1]
                    body = O.xor_padded_np(chunks).copy()
                    at = sorted(set(int(x) for x in rng.integers(0, n, size=min(n, 3)))) if n else []
                    for j in at:
                        body[j] ^= 0x5A
                    if n:
                        q.h2d(dsts[s], body)
                    want.append((at[0] if at else NONE, len(at)))
                q.check_stripes(st, so, res)
                expect(f"check_desc {tag} planted", ar.get(res, len(st), CHECK).tolist(), want)
                ar.close()
    # window replay through desc_tiles + xor_desc: sources of 1, 2 and 2.5 windows and shorter ones
    eng.option("desc_args_max", 16)
    for u in US:
        eng.option("desc_vecs_per_thread", u)
        for lens in ([W], [2 * W, 5], [2 * W + W // 2, W, 17, 0], [2 * W + W // 2, 2 * W, W + 1, W - 1, 2 * W + 1]):
            chunks = [rng.integers(0, 256, size=n, dtype=np.uint8) for n in lens]
            ar = Arena(eng, q, size_of([chunks]))
            st, so, dsts = describe(ar, [chunks], window=W)
            q.xor_stripes(st, so)
            if len(lens) > 1:  # (one source as long as the output is a uniform batch: xor_stream)
                expect(f"xor_desc window U={u} lens={lens}: the form taken", eng.option("last_desc_form"), 1)
            want = np.frombuffer(O.gen_parity_file(chunks, W), dtype=np.uint8)[8 * len(chunks):]
            expect(f"xor_desc window U={u} lens={lens}", ar.get(dsts[0], max(lens)), want)
            ar.close()


def syndromes(rows, p_body, q_body):
    """bcp_pq_check_result by its definition in bcp.h."""
    n = len(p_body)
    ps = p_body ^ (np.bitwise_xor.reduce(rows, axis=0) if len(rows) else np.zeros(n, np.uint8))
    qs = q_body.copy()
    for k, r in enumerate(rows):
        qs ^= G.mul(r, np.uint8(G.gpow(k)))
    bad = np.nonzero((ps != 0) | (qs != 0))[0]
    members = 0
    for j in bad:
        if qs[j] == 0:
            members |= BAD_P
        elif ps[j] == 0:
            members |= BAD_Q
        else:
            ks = [k for k in range(len(rows)) if int(G.mul(ps[j], np.uint8(G.gpow(k)))) == int(qs[j])]
            members |= (1 << ks[0]) if ks else BAD_NOWHERE
    return (int(bad[0]) if len(bad) else NONE, int(np.count_nonzero(ps)), int(np.count_nonzero(qs)), members)


def pq_forms(eng, q, rng, windowed):
    name = "pq_win" if windowed else "pq"
    for u in US:
        eng.option("desc_vecs_per_thread", u)  # the P + Q kernels take 4 or 8, else 4
        for width in WIDTHS:
            tag = f"{name} U={u} width={width}"
            if windowed:
                # one stripe over the window (sources of 2.5, 2 and 1 windows and short ones), the rest without
                lens = ([2 * W + W // 2, 2 * W, W, 17, 0] * 12)[:width]
                batches = [[rng.integers(1, 256, size=n, dtype=np.uint8) for n in lens]]
                batches += [stripe_chunks(rng, n, width) for n in lengths(u)[:5]]
                windows = [W] + [0] * 5
            else:
                batches = [stripe_chunks(rng, n, width) for n in lengths(u)]
                windows = [0] * len(batches)
            ar = Arena(eng, q, size_of(batches) * 6)
            st, so, pd = describe(ar, batches)
            st = [(d, n, f, w, windows[s]) for s, (d, n, f, w, _) in enumerate(st)]
            qd = [ar.room(s[1]) for s in st]
            q.pq_stripes(st, so, qd, windowed=windowed)
            expect(f"{tag} gen: the form taken", eng.option("last_desc_form"), 7 if windowed else 4)
            rows = [PW.rows(chunks, windows[s], st[s][1]) for s, chunks in enumerate(batches)]
            for s, chunks in enumerate(batches):
                n = st[s][1]
                expect(f"{tag} gen P len={n}", ar.get(pd[s], n), PW.p_win(chunks, windows[s], n))
                expect(f"{tag} gen Q len={n}", ar.get(qd[s], n), PW.q_win(chunks, windows[s], n))
            # check: clean, then one wrong byte in a source, in P and in Q of different stripes
            res = ar.room(len(st) * PQCHECK.itemsize)
            q.pq_check(st, so, qd, res, windowed=windowed)
            expect(f"{tag} check clean", ar.get(res, len(st), PQCHECK).tolist(), [(NONE, 0, 0, 0)] * len(st))
            want = []
            for s, chunks in enumerate(batches):
                n = st[s][1]
                p_body, q_body = PW.p_win(chunks, windows[s], n).copy(), PW.q_win(chunks, windows[s], n).copy()
                if n:
                    j = int(rng.integers(0, n))
                    (p_body if s % 2 else q_body)[j] ^= 0x21
                    if n > 40:
                        p_body[n - 1] ^= 0x7
                        q_body[n - 1] ^= 0x9  # both syndromes, some position or nowhere
                    q.h2d(pd[s], p_body)
                    q.h2d(qd[s], q_body)
                want.append(syndromes(rows[s], p_body, q_body))
            q.pq_check(st, so, qd, res, windowed=windowed)
            expect(f"{tag} check: the form taken", eng.option("last_desc_form"), 9 if windowed else 6)
            expect(f"{tag} check planted", ar.get(res, len(st), PQCHECK).tolist(), want)
            # solve: two members from P and Q (width >= 3), one member from Q alone (width >= 2)
            for two in (True, False):
                if width < (3 if two else 2):
                    continue
                st2, so2, lost, outs = [], [], [], []
                for s, chunks in enumerate(batches):
                    n = st[s][1]
                    x, y = (0, width - 1) if two else (width - 1, None)
                    first = len(so2)
                    for k, c in enumerate(chunks):
                        gone = k == x or k == y
                        so2.append((0, 0) if gone or not len(c) else (ar.put(c), len(c)))
                    pb = ar.put(PW.p_win(chunks, windows[s], n)) if two else 0
                    qb = ar.put(PW.q_win(chunks, windows[s], n))
                    lx = len(chunks[x])
                    ly = len(chunks[y]) if two else 0
                    dx, dy = ar.room(lx), ar.room(ly)
                    st2.append((0, n, first, width, windows[s]))
                    lost.append((pb, qb, x, y if two else B.PQ_NONE, dx, lx, dy, ly))
                    outs.append((dx, chunks[x], dy, chunks[y] if two else None))
                q.pq_recover(st2, so2, lost, windowed=windowed)
                expect(f"{tag} solve: the form taken", eng.option("last_desc_form"), 8 if windowed else 5)
                for s, (dx, cx, dy, cy) in enumerate(outs):
                    expect(f"{tag} solve two={two} x, stripe {s}", ar.get(dx, len(cx)), cx)
                    if cy is not None:
                        expect(f"{tag} solve two={two} y, stripe {s}", ar.get(dy, len(cy)), cy)
            ar.close()


def main():
    assert "double" in os.path.basename(B.LIB_PATH), "BCP_LIB must name the stand-in's library"
    O.build()
    rng = np.random.default_rng(20)
    eng = B.Engine(0)
    q = eng.queue()
    # tables both ways: read in place from pinned memory, and uploaded
    for host_max in (None, 0):
        if host_max is not None:
            eng.option("table_host_max", host_max)
            eng.option("desc_table_host_max", host_max)
        xor_forms(eng, q, rng)
        pq_forms(eng, q, rng, windowed=False)
        pq_forms(eng, q, rng, windowed=True)
    q.close()
    eng.close()
    for w in wrong[:40]:
        print("WRONG:", w)
    print(f"forms: {checks} checks, {len(wrong)} wrong")
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
