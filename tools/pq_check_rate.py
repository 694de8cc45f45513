#!/usr/bin/env python3
"""Rate of the syndrome form of the P + Q kernel (bcp_pq_check_stripes_async)
beside its GEN form (bcp_pq_stripes_async) and the P check kernel
(bcp_check_stripes_async) on the same descriptors, in one process.

Device-resident synthetic sources (bcp_dev_fill_synthetic_async); the bodies
are what the GEN form itself stored, so every check is clean (the clean path:
the loads, one ballot per tile, no store, no atomic).  The two descriptor sets
of tools/pq_rate.py and tools/check_rate.py:

  uniform  8 x 512 KiB stripes, as many as bench.py's default run (12,500)
  mixed    the config-5 shapes bench.py --mode mixed draws (8-wide stripes,
           log-uniform 64 KiB - 4 MiB chunks, zero-padded to the stripe max)

Syndrome, GEN and P check launches alternate on one queue, back to back,
--steps timed ones each after --warmup triples, each between two of the
queue's HIP-event marks.  Bytes: (n + 2) x out_len per stripe for the syndrome
form (n sources and both bodies read) and for GEN (n sources read, both bodies
written), (n + 1) x out_len for the P check.  The yardstick for the syndrome
form is GEN of the same run: the ratio of the medians is printed beside GEN's
launch-to-launch spread ((max - min) / median), the only noise figure the run
can justify.  The ratio to the P check is reported for information: the byte
counts differ.

One JSON line per figure, on stdout and appended to --out
(default profiles/pqcheck/pq_check_rate.jsonl).

    python tools/pq_check_rate.py [--steps 20] [--warmup 3] [--stripes 12500]
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


def device_shape(a, eng, q, name, lens_all):
    """lens_all: per stripe the source lengths; sources and bodies at 256-byte pitch."""
    align = lambda x: (x + 255) & ~255  # noqa: E731
    src_bytes = sum(sum(align(int(x)) for x in ls) for ls in lens_all)
    out_bytes = sum(align(int(max(ls))) for ls in lens_all)
    n = len(lens_all)
    src, out, qout = eng.alloc(src_bytes), eng.alloc(out_bytes), eng.alloc(out_bytes)
    res, pres = eng.alloc(32 * n), eng.alloc(16 * n)
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
    L = bcp.lib()
    pq_bytes = sum((len(ls) + 2) * int(max(ls)) for ls in lens_all)
    p_bytes = sum((len(ls) + 1) * int(max(ls)) for ls in lens_all)

    def syndrome():
        bcp.check("bcp_pq_check_stripes_async",
                  L.bcp_pq_check_stripes_async(q.h, st, n, so, len(sources), qb, bcp._V(res)))

    def gen():
        bcp.check("bcp_pq_stripes_async", L.bcp_pq_stripes_async(q.h, st, n, so, len(sources), qb))

    def pcheck():
        bcp.check("bcp_check_stripes_async", L.bcp_check_stripes_async(q.h, st, n, so, len(sources), bcp._V(pres)))

    gen()  # the bodies every check reads
    for _ in range(a.warmup):
        syndrome()
        gen()
        pcheck()
    q.sync()
    forms = {}
    for key, fn in (("syndrome", syndrome), ("gen", gen), ("p_check", pcheck)):
        fn()
        q.sync()
        forms[key] = dict(desc_form=eng.option("last_desc_form"), desc_vecs=eng.option("last_desc_vecs"))
    forms["pq_blocks_per_cu"] = eng.option("pq_blocks_per_cu")
    # 3 x steps launches back to back, a mark between each two (slots 0 .. 3 * steps)
    q.mark(0)
    for i in range(a.steps):
        syndrome()
        q.mark(3 * i + 1)
        gen()
        q.mark(3 * i + 2)
        pcheck()
        q.mark(3 * i + 3)
    q.sync()
    syn_ms = [q.elapsed_ms(3 * i, 3 * i + 1) for i in range(a.steps)]
    gen_ms = [q.elapsed_ms(3 * i + 1, 3 * i + 2) for i in range(a.steps)]
    pc_ms = [q.elapsed_ms(3 * i + 2, 3 * i + 3) for i in range(a.steps)]
    # the checks were clean: every record {UINT64_MAX, 0, 0, 0} and {UINT64_MAX, 0}
    recs, precs = np.empty(4 * n, dtype=np.uint64), np.empty(2 * n, dtype=np.uint64)
    q.d2h(recs, res, recs.nbytes)
    q.d2h(precs, pres, precs.nbytes)
    q.sync()
    full = np.uint64(2 ** 64 - 1)
    clean = bool((recs[0::4] == full).all() and (recs.reshape(n, 4)[:, 1:] == 0).all() and
                 (precs[0::2] == full).all() and (precs[1::2] == 0).all())
    s, g, c = figures(syn_ms, pq_bytes), figures(gen_ms, pq_bytes), figures(pc_ms, p_bytes)
    over = s["ms_median"] / g["ms_median"]
    emit(a.out, shape=name, stripes=n, steps=a.steps, warmup=a.warmup, pq_bytes_per_launch=pq_bytes,
         p_check_bytes_per_launch=p_bytes, syndrome=s, gen=g, p_check=c, forms=forms,
         syndrome_ms_over_gen_ms=round(over, 4), gen_spread=g["spread"],
         within_gen_spread=bool(over - 1.0 <= g["spread"]),
         syndrome_ms_over_p_check_ms=round(s["ms_median"] / c["ms_median"], 4),
         syndrome_rate_over_p_check_rate=round(s["GBps"] / c["GBps"], 4), all_clean=clean,
         syndrome_ms=[round(x, 4) for x in syn_ms], gen_ms=[round(x, 4) for x in gen_ms],
         p_check_ms=[round(x, 4) for x in pc_ms])
    for p in (src, out, qout, res, pres):
        eng.free(p)
    return clean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stripes", type=int, default=0, help="stripes of the uniform batch (default: bench.py's)")
    ap.add_argument("--shapes", default="uniform,mixed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pqcheck", "pq_check_rate.jsonl"))
    a = ap.parse_args()
    assert 1 <= a.steps <= 21, "three marks per step, 64 timer slots"
    import bench
    S = a.stripes or bench.default_stripes(1, 0)
    eng = bcp.Engine(0)
    q = eng.queue()
    cus, name = eng.info()
    emit(a.out, device=name, cus=cus, tool="pq_check_rate")
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
