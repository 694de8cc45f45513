#!/usr/bin/env python3
"""Time of the repair form of the P + Q kernel (bcp_pq_repair_stripes_async) on
clean bodies beside its check form (bcp_pq_check_stripes_async) on the same
descriptors, in one process.

On a clean stripe the repair form executes the check form's loads and its one
ballot per tile and nothing else, so the expectation is a time ratio inside the
check form's own launch-to-launch spread.  The pipeline does not depend on the
figure (it launches the repair form over flagged stripes only); it says whether
a one-pass repair run would cost anything.

Layout, shapes and byte counts are tools/pq_check_rate.py's: device-resident
synthetic sources, bodies stored by the GEN form, `allow` all ones, the uniform
and the mixed descriptor set.  Check and repair launches alternate on one queue,
back to back, --steps timed ones each after --warmup pairs, each between two of
the queue's HIP-event marks.  Each kernel's first timed launch is set aside (as
DESIGN.md section 4 does) before medians and spreads are taken; all launches are
listed.

--windowed times the windowed repair form (bcp_pq_repair_stripes_win_async)
beside the windowed check form (bcp_pq_check_stripes_win_async) the same way,
window 10 MiB, bodies stored by the windowed GEN form, on the two shapes of
tools/pq_rate.py --windowed: 200 stripes of 8 x 16 MiB (no threshold below
out_len: one launch) and 200 of one 24 MiB source and seven of 64 KiB (their
T_k = 10 MiB is a threshold: two launches, recorded as repair_launches).

One JSON line per shape, on stdout and appended to --out (default
profiles/pqrepair/pq_repair_rate.jsonl; --windowed: pq_repair_win_rate.jsonl).

    python tools/pq_repair_rate.py [--steps 20] [--warmup 3] [--stripes 12500]
    python tools/pq_repair_rate.py --windowed [--win-stripes 200]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pq_check_rate import KiB, MiB, ROOT, bcp, emit, figures  # noqa: E402


def device_shape(a, eng, q, name, lens_all):
    align = lambda x: (x + 255) & ~255  # noqa: E731
    src_bytes = sum(sum(align(int(x)) for x in ls) for ls in lens_all)
    out_bytes = sum(align(int(max(ls))) for ls in lens_all)
    n = len(lens_all)
    src, out, qout = eng.alloc(src_bytes), eng.alloc(out_bytes), eng.alloc(out_bytes)
    res, rres = eng.alloc(32 * n), eng.alloc(48 * n)
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
    st = (bcp.Stripe * n)(*[bcp.Stripe(*x) for x in stripes])
    so = (bcp.Source * len(sources))(*[bcp.Source(*x) for x in sources])
    qb = (bcp.ctypes.c_uint64 * n)(*qd)
    al = (bcp.ctypes.c_uint64 * n)(*([2 ** 64 - 1] * n))
    L = bcp.lib()
    nbytes = sum((len(ls) + 2) * int(max(ls)) for ls in lens_all)

    def check():
        bcp.check("bcp_pq_check_stripes_async",
                  L.bcp_pq_check_stripes_async(q.h, st, n, so, len(sources), qb, bcp._V(res)))

    def repair():
        bcp.check("bcp_pq_repair_stripes_async",
                  L.bcp_pq_repair_stripes_async(q.h, st, n, so, len(sources), qb, al, bcp._V(rres)))

    bcp.check("bcp_pq_stripes_async", L.bcp_pq_stripes_async(q.h, st, n, so, len(sources), qb))  # the bodies
    for _ in range(a.warmup):
        check()
        repair()
    q.sync()
    forms = {}
    for key, fn in (("check", check), ("repair", repair)):
        fn()
        q.sync()
        forms[key] = dict(desc_form=eng.option("last_desc_form"), desc_vecs=eng.option("last_desc_vecs"))
    forms["pq_blocks_per_cu"] = eng.option("pq_blocks_per_cu")
    q.mark(0)
    for i in range(a.steps):
        check()
        q.mark(2 * i + 1)
        repair()
        q.mark(2 * i + 2)
    q.sync()
    chk_ms = [q.elapsed_ms(2 * i, 2 * i + 1) for i in range(a.steps)]
    rep_ms = [q.elapsed_ms(2 * i + 1, 2 * i + 2) for i in range(a.steps)]
    recs, rrecs = np.empty(4 * n, dtype=np.uint64), np.empty(6 * n, dtype=np.uint64)
    q.d2h(recs, res, recs.nbytes)
    q.d2h(rrecs, rres, rrecs.nbytes)
    q.sync()
    full = np.uint64(2 ** 64 - 1)
    clean = bool((recs[0::4] == full).all() and (recs.reshape(n, 4)[:, 1:] == 0).all() and
                 (rrecs[0::6] == full).all() and (rrecs.reshape(n, 6)[:, 1:] == 0).all())
    c, r = figures(chk_ms[1:], nbytes), figures(rep_ms[1:], nbytes)  # each kernel's first timed launch set aside
    over = r["ms_median"] / c["ms_median"]
    emit(a.out, shape=name, stripes=n, steps=a.steps, warmup=a.warmup, bytes_per_launch=nbytes, check=c, repair=r,
         forms=forms, repair_ms_over_check_ms=round(over, 4), check_spread=c["spread"],
         within_check_spread=bool(abs(over - 1.0) <= c["spread"]), all_clean=clean,
         first_timed_launch_set_aside=True, check_ms=[round(x, 4) for x in chk_ms],
         repair_ms=[round(x, 4) for x in rep_ms])
    for p in (src, out, qout, res, rres):
        eng.free(p)
    return clean


def windowed_shape(a, eng, q, name, lens, nstripes):
    """Windowed REPAIR (bcp_pq_repair_stripes_win_async, allow all ones, clean bodies: one phase per stripe's
    thresholds, every tile on the clean path) beside windowed CHECK on the same descriptors, window 10 MiB."""
    W = bcp.WINDOW_BYTES
    align = lambda x: (x + 255) & ~255  # noqa: E731
    m = max(lens)
    src_bytes, out_bytes = nstripes * sum(align(x) for x in lens), nstripes * align(m)
    src, out, qout = eng.alloc(src_bytes), eng.alloc(out_bytes), eng.alloc(out_bytes)
    res, rres = eng.alloc(32 * nstripes), eng.alloc(48 * nstripes)
    q.fill_synthetic(src, src_bytes, seed=1)
    stripes, sources, qd, so_off = [], [], [], 0
    for s in range(nstripes):
        first = len(sources)
        for x in lens:
            sources.append((src + so_off, x))
            so_off += align(x)
        stripes.append((out + s * align(m), m, first, len(lens), W))
        qd.append(qout + s * align(m))
    n = nstripes
    st = (bcp.Stripe * n)(*[bcp.Stripe(*x) for x in stripes])
    so = (bcp.Source * len(sources))(*[bcp.Source(*x) for x in sources])
    qb = (bcp.ctypes.c_uint64 * n)(*qd)
    al = (bcp.ctypes.c_uint64 * n)(*([2 ** 64 - 1] * n))
    L = bcp.lib()
    nbytes = n * (len(lens) + 2) * m  # the streams' bytes, replayed padding included (as pq_rate.py --windowed)

    def check():
        bcp.check("bcp_pq_check_stripes_win_async",
                  L.bcp_pq_check_stripes_win_async(q.h, st, n, so, len(sources), qb, bcp._V(res)))

    def repair():
        bcp.check("bcp_pq_repair_stripes_win_async",
                  L.bcp_pq_repair_stripes_win_async(q.h, st, n, so, len(sources), qb, al, bcp._V(rres)))

    bcp.check("bcp_pq_stripes_win_async", L.bcp_pq_stripes_win_async(q.h, st, n, so, len(sources), qb))  # the bodies
    for _ in range(a.warmup):
        check()
        repair()
    q.sync()
    forms = {}
    for key, fn in (("check", check), ("repair", repair)):
        fn()
        q.sync()
        forms[key] = dict(desc_form=eng.option("last_desc_form"), desc_vecs=eng.option("last_desc_vecs"))
    forms["pq_blocks_per_cu"] = eng.option("pq_blocks_per_cu")
    forms["repair_launches"] = eng.option("last_pq_repair_phases")
    q.mark(0)
    for i in range(a.steps):
        check()
        q.mark(2 * i + 1)
        repair()
        q.mark(2 * i + 2)
    q.sync()
    chk_ms = [q.elapsed_ms(2 * i, 2 * i + 1) for i in range(a.steps)]
    rep_ms = [q.elapsed_ms(2 * i + 1, 2 * i + 2) for i in range(a.steps)]
    recs, rrecs = np.empty(4 * n, dtype=np.uint64), np.empty(6 * n, dtype=np.uint64)
    q.d2h(recs, res, recs.nbytes)
    q.d2h(rrecs, rres, rrecs.nbytes)
    q.sync()
    full = np.uint64(2 ** 64 - 1)
    clean = bool((recs[0::4] == full).all() and (recs.reshape(n, 4)[:, 1:] == 0).all() and
                 (rrecs[0::6] == full).all() and (rrecs.reshape(n, 6)[:, 1:] == 0).all())
    c, r = figures(chk_ms[1:], nbytes), figures(rep_ms[1:], nbytes)  # each kernel's first timed launch set aside
    over = r["ms_median"] / c["ms_median"]
    emit(a.out, shape=name, lens=lens, window=W, stripes=n, steps=a.steps, warmup=a.warmup, stream_bytes_per_launch=nbytes,
         check=c, repair=r, forms=forms, repair_ms_over_check_ms=round(over, 4), check_spread=c["spread"],
         within_check_spread=bool(abs(over - 1.0) <= c["spread"]), all_clean=clean,
         first_timed_launch_set_aside=True, check_ms=[round(x, 4) for x in chk_ms],
         repair_ms=[round(x, 4) for x in rep_ms])
    for p in (src, out, qout, res, rres):
        eng.free(p)
    return clean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stripes", type=int, default=0, help="stripes of the uniform batch (default: bench.py's)")
    ap.add_argument("--shapes", default="uniform,mixed")
    ap.add_argument("--windowed", action="store_true", help="windowed REPAIR beside windowed CHECK")
    ap.add_argument("--win-stripes", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert 2 <= a.steps <= 31, "two marks per step, 64 timer slots; the first launch of each is set aside"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "pqrepair",
                             "pq_repair_win_rate.jsonl" if a.windowed else "pq_repair_rate.jsonl")
    if a.windowed:
        eng = bcp.Engine(0)
        q = eng.queue()
        cus, name = eng.info()
        emit(a.out, device=name, cus=cus, tool="pq_repair_rate --windowed")
        ok = windowed_shape(a, eng, q, "equal16m", [16 * MiB] * 8, a.win_stripes)
        ok &= windowed_shape(a, eng, q, "replay", [24 * MiB] + [64 * KiB] * 7, a.win_stripes)
        q.close()
        eng.close()
        sys.exit(0 if ok else 3)
    import bench
    S = a.stripes or bench.default_stripes(1, 0)
    eng = bcp.Engine(0)
    q = eng.queue()
    cus, name = eng.info()
    emit(a.out, device=name, cus=cus, tool="pq_repair_rate")
    ok = True
    for shape in a.shapes.split(","):
        if shape == "mixed":
            lens_all = [[int(x) for x in ls] for ls in bench.mixed_lengths(S, 8, 512 * KiB, 0)]
        else:
            lens_all = [[512 * KiB] * 8] * S
        ok &= device_shape(a, eng, q, shape, lens_all)
    q.close()
    eng.close()
    sys.exit(0 if ok else 3)


if __name__ == "__main__":
    main()
