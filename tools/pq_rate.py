#!/usr/bin/env python3
"""Rate of the P + Q kernel (bcp_pq_stripes_async) beside the fold
(bcp_xor_stripes_async) on the same descriptors, in one process.

Device-resident synthetic sources (bcp_dev_fill_synthetic_async).  The two
descriptor sets of tools/check_rate.py:

  uniform  8 x 512 KiB stripes, as many as bench.py's default run (12,500; the
           fold takes the pointer-table xor_stream for these)
  mixed    the config-5 shapes bench.py --mode mixed draws (8-wide stripes,
           log-uniform 64 KiB - 4 MiB chunks, zero-padded to the stripe max)

Before anything is timed, P and Q of a sample of stripes are copied back and
compared with a host-computed XOR and Q (GF(2^8), polynomial 0x11d, g = 2).
Then PQ and fold launches alternate on one queue, back to back, --steps timed
ones each after --warmup pairs, each between two of the queue's HIP-event
marks.  Bytes: (n + 2) x out_len per stripe for PQ (n sources read, P and Q
written), (n + 1) x out_len for the fold.  Reported: ms, the fraction of the
8 TB/s peak, the ratio of the medians and each kernel's launch-to-launch spread
((max - min) / median) -- a ratio inside that spread is noise.

--sweep repeats the PQ side for every tile size (desc_vecs_per_thread 4, 8)
and 1..3 workgroups per CU (pq_blocks_per_cu); without it the engine's
defaults run.

--windowed times the windowed GEN kernel (bcp_pq_stripes_win_async, window
10 MiB) instead, against the existing one (bcp_pq_stripes_async, window 0) on
the same buffers, launches alternating as above, on two shapes:

  equal16m  8 x 16 MiB stripes (--win-stripes of them, default 200): every
            source is longer than the window and as long as the output, so
            nothing is replayed and both kernels read and write the same
            bytes -- the cost of the windowed form's per-source remap alone;
            their outputs are compared with each other and with the host's
  replay    one 24 MiB source and seven of 64 KiB: the windowed kernel replays
            the short ones' first window (64 KiB and its padding) into every
            later window, for the other they are zero padding, so the two do
            different work -- described, not compared.  Bytes are the streams'
            ((n + 2) x out_len, padding included) for the windowed kernel and
            the bytes actually read and written for the other.

One JSON line per figure, on stdout and appended to --out
(default profiles/pq/pq_rate.jsonl; --windowed: profiles/pq/pq_win_rate.jsonl).

    python tools/pq_rate.py [--steps 20] [--warmup 3] [--stripes 12500] [--sweep]
    python tools/pq_rate.py --windowed [--win-stripes 200]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "beegfs-chunk-parity_amd"), os.path.join(ROOT, "oracle"), ROOT,
          os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import bcp_ctypes as bcp  # noqa: E402

KiB, MiB, GiB = 1024, 1024 ** 2, 1024 ** 3
HBM_PEAK = 8.0e12  # bytes/s, MI355X


def emit(out, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def figures(ms, nbytes):
    med = statistics.median(ms)
    return dict(ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                spread=round((max(ms) - min(ms)) / med, 4), GBps=round(nbytes / med / 1e6, 1),
                pct_of_8TBps=round(100 * nbytes / (med * 1e-3) / HBM_PEAK, 2))


def gf_tables():
    exp, log, x = np.zeros(510, np.uint8), np.zeros(256, np.int32), 1
    for i in range(255):
        exp[i] = exp[i + 255] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    return exp, log


def host_pq(rows):
    """rows: [n][out_len] uint8, zero-padded -> (P, Q) with Q = sum of g^k * row k."""
    exp, log = gf_tables()
    p = np.bitwise_xor.reduce(rows, axis=0)
    q = np.zeros(rows.shape[1], np.uint8)
    for k in range(rows.shape[0]):
        q ^= np.where(rows[k] == 0, np.uint8(0), exp[(log[rows[k]] + k) % 255])
    return p, q


def device_shape(a, eng, q, name, lens_all, configs):
    """lens_all: per stripe the source lengths; sources and outputs at 256-byte pitch."""
    align = lambda x: (x + 255) & ~255  # noqa: E731
    src_bytes = sum(sum(align(int(x)) for x in ls) for ls in lens_all)
    out_bytes = sum(align(int(max(ls))) for ls in lens_all)
    src, out, qout = eng.alloc(src_bytes), eng.alloc(out_bytes), eng.alloc(out_bytes)
    q.fill_synthetic(src, src_bytes, seed=1)
    stripes, sources, qd, so_off, do_off = [], [], [], 0, 0
    for ls in lens_all:
        first = len(sources)
        for x in ls:
            sources.append((src + so_off, int(x)))
            so_off += align(int(x))
        m = int(max(ls))
        stripes.append((out + do_off, m, first, len(ls), 0))
        qd.append(qout + do_off)
        do_off += align(m)
    st = (bcp.Stripe * len(stripes))(*[bcp.Stripe(*x) for x in stripes])
    so = (bcp.Source * len(sources))(*[bcp.Source(*x) for x in sources])
    qdst = (bcp.ctypes.c_uint64 * len(qd))(*qd)
    L = bcp.lib()
    fold_bytes = sum((len(ls) + 1) * int(max(ls)) for ls in lens_all)
    pq_bytes = sum((len(ls) + 2) * int(max(ls)) for ls in lens_all)

    def fold():
        bcp.check("bcp_xor_stripes_async", L.bcp_xor_stripes_async(q.h, st, len(stripes), so, len(sources)))

    def pq():
        bcp.check("bcp_pq_stripes_async", L.bcp_pq_stripes_async(q.h, st, len(stripes), so, len(sources), qdst))

    def verify():
        """P and Q of a sample of stripes against the host's."""
        q.memset(out, 0xA5, out_bytes)
        q.memset(qout, 0xA5, out_bytes)
        pq()
        q.sync()
        n = len(stripes)
        for s in sorted({0, 1, n // 3, n // 2, n - 1}):
            dst, m, first, nsrc, _ = stripes[s]
            rows = np.zeros((nsrc, m), np.uint8)
            for k in range(nsrc):
                ptr, ln = sources[first + k]
                q.d2h(rows[k], ptr, ln)
            gp, gq = np.empty(m, np.uint8), np.empty(m, np.uint8)
            q.d2h(gp, dst, m)
            q.d2h(gq, qd[s], m)
            q.sync()
            hp, hq = host_pq(rows)
            if not (np.array_equal(gp, hp) and np.array_equal(gq, hq)):
                return False
        return True

    ok = True
    for cfg in configs:
        for k, v in cfg.items():
            eng.option(k, v)
        good = verify()
        ok &= good
        for _ in range(a.warmup):
            pq()
            fold()
        q.sync()
        forms = {}
        fold()
        q.sync()
        forms["fold"] = dict(desc_form=eng.option("last_desc_form"), desc_vecs=eng.option("last_desc_vecs"),
                             stream_vecs=eng.option("last_stream_vecs"))
        pq()
        q.sync()
        forms["pq"] = dict(desc_form=eng.option("last_desc_form"), desc_vecs=eng.option("last_desc_vecs"),
                           blocks_per_cu=eng.option("pq_blocks_per_cu"))
        # 2 x steps launches back to back, a mark between each two (slots 0 .. 2 * steps)
        q.mark(0)
        for i in range(a.steps):
            pq()
            q.mark(2 * i + 1)
            fold()
            q.mark(2 * i + 2)
        q.sync()
        pq_ms = [q.elapsed_ms(2 * i, 2 * i + 1) for i in range(a.steps)]
        fold_ms = [q.elapsed_ms(2 * i + 1, 2 * i + 2) for i in range(a.steps)]
        f, c = figures(fold_ms, fold_bytes), figures(pq_ms, pq_bytes)
        emit(a.out, shape=name, stripes=len(stripes), config=cfg, steps=a.steps, warmup=a.warmup,
             fold_bytes_per_launch=fold_bytes, pq_bytes_per_launch=pq_bytes, fold=f, pq=c, forms=forms,
             pq_ms_over_fold_ms=round(c["ms_median"] / f["ms_median"], 4),
             pq_rate_over_fold_rate=round(c["GBps"] / f["GBps"], 4), sample_verified=good,
             fold_ms=[round(x, 4) for x in fold_ms], pq_ms=[round(x, 4) for x in pq_ms])
    for p in (src, out, qout):
        eng.free(p)
    return ok


def replayed_rows(q, sources, first, nsrc, m, w):
    """[nsrc][m] uint8: the replayed stream of every source of one stripe (w = 0: zero padding)."""
    rows = np.zeros((nsrc, m), np.uint8)
    for k in range(nsrc):
        ptr, ln = sources[first + k]
        if not ln:
            continue
        lw = (ln - 1) // w if w else 0
        pad = np.zeros((lw + 1) * w if w else max(ln, m), np.uint8)
        q.d2h(pad[:ln], ptr, ln)
        q.sync()
        j = np.arange(m, dtype=np.int64)
        rows[k] = pad[np.where(j < (lw + 1) * w, j, lw * w + j % w)] if w else pad[:m]
    return rows


def windowed_shape(a, eng, q, name, lens, nstripes, same_output):
    """The windowed GEN kernel (window W) against the existing one (window 0) on the same buffers."""
    W = bcp.WINDOW_BYTES
    align = lambda x: (x + 255) & ~255  # noqa: E731
    m = max(lens)
    src_bytes, out_bytes = nstripes * sum(align(x) for x in lens), nstripes * align(m)
    src, out, qout = eng.alloc(src_bytes), eng.alloc(out_bytes), eng.alloc(out_bytes)
    q.fill_synthetic(src, src_bytes, seed=1)
    stripes = {0: [], W: []}
    sources, qd, so_off = [], [], 0
    for s in range(nstripes):
        first = len(sources)
        for x in lens:
            sources.append((src + so_off, x))
            so_off += align(x)
        for w in stripes:
            stripes[w].append((out + s * align(m), m, first, len(lens), w))
        qd.append(qout + s * align(m))
    so = (bcp.Source * len(sources))(*[bcp.Source(*x) for x in sources])
    st = {w: (bcp.Stripe * nstripes)(*[bcp.Stripe(*x) for x in v]) for w, v in stripes.items()}
    qdst = (bcp.ctypes.c_uint64 * nstripes)(*qd)
    L = bcp.lib()

    def plain():
        bcp.check("bcp_pq_stripes_async", L.bcp_pq_stripes_async(q.h, st[0], nstripes, so, len(sources), qdst))

    def win():
        bcp.check("bcp_pq_stripes_win_async",
                  L.bcp_pq_stripes_win_async(q.h, st[W], nstripes, so, len(sources), qdst))

    def outputs(fn, sample):
        q.memset(out, 0xA5, out_bytes)
        q.memset(qout, 0xA5, out_bytes)
        fn()
        got = []
        for s in sample:
            gp, gq = np.empty(m, np.uint8), np.empty(m, np.uint8)
            q.d2h(gp, stripes[0][s][0], m)
            q.d2h(gq, qd[s], m)
            got.append((gp, gq))
        q.sync()
        return got

    sample = sorted({0, nstripes // 2, nstripes - 1})
    got_w, got_p = outputs(win, sample), outputs(plain, sample)
    good = True
    for i, s in enumerate(sample[:2]):
        for w, got in ((W, got_w), (0, got_p)):
            hp, hq = host_pq(replayed_rows(q, sources, stripes[0][s][2], len(lens), m, w))
            good &= np.array_equal(got[i][0], hp) and np.array_equal(got[i][1], hq)
    if same_output:
        good &= all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(got_w, got_p))
    for _ in range(a.warmup):
        win()
        plain()
    q.sync()
    forms = {}
    for key, fn in (("plain", plain), ("windowed", win)):
        fn()
        q.sync()
        forms[key] = dict(desc_form=eng.option("last_desc_form"), desc_vecs=eng.option("last_desc_vecs"),
                          blocks_per_cu=eng.option("pq_blocks_per_cu"))
    q.mark(0)
    for i in range(a.steps):
        win()
        q.mark(2 * i + 1)
        plain()
        q.mark(2 * i + 2)
    q.sync()
    win_ms = [q.elapsed_ms(2 * i, 2 * i + 1) for i in range(a.steps)]
    plain_ms = [q.elapsed_ms(2 * i + 1, 2 * i + 2) for i in range(a.steps)]
    win_bytes = nstripes * (len(lens) + 2) * m
    plain_bytes = nstripes * (sum(lens) + 2 * m)
    fw, fp = figures(win_ms, win_bytes), figures(plain_ms, plain_bytes)
    emit(a.out, shape=name, lens=lens, window=W, stripes=nstripes, steps=a.steps, warmup=a.warmup,
         windowed_bytes_per_launch=win_bytes, plain_bytes_per_launch=plain_bytes, windowed=fw, plain=fp, forms=forms,
         windowed_ms_over_plain_ms=round(fw["ms_median"] / fp["ms_median"], 4),
         same_work=same_output, sample_verified=bool(good),
         windowed_ms=[round(x, 4) for x in win_ms], plain_ms=[round(x, 4) for x in plain_ms])
    for p in (src, out, qout):
        eng.free(p)
    return bool(good)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stripes", type=int, default=0, help="stripes of the uniform batch (default: bench.py's)")
    ap.add_argument("--shapes", default="uniform,mixed")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--windowed", action="store_true", help="the windowed GEN kernel against the existing one")
    ap.add_argument("--win-stripes", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert 1 <= a.steps <= 31, "two marks per step, 64 timer slots"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "pq", "pq_win_rate.jsonl" if a.windowed else "pq_rate.jsonl")
    if a.windowed:
        eng = bcp.Engine(0)
        q = eng.queue()
        cus, name = eng.info()
        emit(a.out, device=name, cus=cus, tool="pq_rate --windowed")
        ok = windowed_shape(a, eng, q, "equal16m", [16 * MiB] * 8, a.win_stripes, True)
        ok &= windowed_shape(a, eng, q, "replay", [24 * MiB] + [64 * KiB] * 7, a.win_stripes, False)
        q.close()
        eng.close()
        sys.exit(0 if ok else 3)
    import bench
    S = a.stripes or bench.default_stripes(1, 0)
    eng = bcp.Engine(0)
    q = eng.queue()
    cus, name = eng.info()
    emit(a.out, device=name, cus=cus, tool="pq_rate")
    configs = [{}]
    if a.sweep:
        configs = [dict(desc_vecs_per_thread=v, pq_blocks_per_cu=b) for v in (4, 8) for b in (1, 2, 3)]
    ok = True
    for shape in a.shapes.split(","):
        if shape == "mixed":
            lens_all = [[int(x) for x in ls] for ls in bench.mixed_lengths(S, 8, 512 * KiB, 0)]
        else:
            lens_all = [[512 * KiB] * 8] * S
        ok &= device_shape(a, eng, q, shape, lens_all, configs)
    q.close()
    eng.close()
    sys.exit(0 if ok else 3)


if __name__ == "__main__":
    main()
