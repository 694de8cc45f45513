#!/usr/bin/env python3
"""Rate of the verified-rebuild form of the P + Q kernel
(bcp_pq_rebuild_check_stripes_async) beside the existing XOR rebuild
(bcp_xor_stripes_async over the survivors and the P body) and the syndrome form
(bcp_pq_check_stripes_async) on the same descriptors, in one process.

Device-resident synthetic members (bcp_dev_fill_synthetic_async); the bodies are
what the GEN form stored over all n members, so every record is clean (the clean
path: the loads, the member's store, one ballot per tile, no atomic).  Member
x = s mod n of stripe s is the lost one.  The two descriptor sets of
tools/pq_check_rate.py:

  uniform  8 x 512 KiB stripes, as many as bench.py's default run (12,500)
  mixed    the config-5 shapes bench.py --mode mixed draws (8-wide stripes,
           log-uniform 64 KiB - 4 MiB chunks, zero-padded to the stripe max)

The three launches alternate on one queue, back to back, --steps timed ones
each after --warmup triples, each between two of the queue's HIP-event marks.
Each kernel's first timed launch is set aside (as tools/pq_repair_rate.py does),
so the default 21 steps give 20.  Streams per stripe: the new form reads n + 1
(n - 1 survivors, P, Q) and writes one; the XOR rebuild reads n and writes one;
the syndrome form reads n + 2 and writes none.  Bytes are counted as moved:
below len_x only for the two rebuilds (their tiles cover [0, len_x)), the whole
out_len for the syndrome form.  The yardsticks are the ratios of the median
times, printed beside the syndrome form's own launch-to-launch spread
((max - min) / median) of the same run, the only noise figure the run can
justify.

After the timed launches the new form's output is compared with the XOR
rebuild's on the device (bcp_dev_compare_async) and every record must be clean.

One JSON line per figure, on stdout and appended to --out
(default profiles/pqrebuild/pq_rebuild_rate.jsonl).

    python tools/pq_rebuild_rate.py [--steps 21] [--warmup 3] [--stripes 12500]
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
    """lens_all: per stripe the member lengths; members, bodies and outputs at 256-byte pitch."""
    align = lambda x: (x + 255) & ~255  # noqa: E731
    src_bytes = sum(sum(align(int(x)) for x in ls) for ls in lens_all)
    body_bytes = sum(align(int(max(ls))) for ls in lens_all)
    n = len(lens_all)
    src, pbody, qbody = eng.alloc(src_bytes), eng.alloc(body_bytes), eng.alloc(body_bytes)
    out_v, out_x = eng.alloc(body_bytes), eng.alloc(body_bytes)  # member x by the new form and by the XOR rebuild
    res, vres, cmp8 = eng.alloc(32 * n), eng.alloc(16 * n), eng.alloc(8)
    q.fill_synthetic(src, src_bytes, seed=1)
    q.memset(out_v, 0, body_bytes)
    q.memset(out_x, 0, body_bytes)
    full, surv, xsrc, gen_st, reb_st, xor_st, qd, lost = [], [], [], [], [], [], [], []
    so_off, do_off = 0, 0
    v_bytes = x_bytes = c_bytes = 0
    for s, ls in enumerate(lens_all):
        w, x, m = len(ls), s % len(ls), int(max(ls))
        len_x = int(ls[x])
        f0, s0, x0 = len(full), len(surv), len(xsrc)
        for k, L in enumerate(ls):
            ptr = src + so_off
            so_off += align(int(L))
            full.append((ptr, int(L)))
            surv.append((0, 0) if k == x else (ptr, int(L)))
            if k != x:
                xsrc.append((ptr, int(L)))
        xsrc.append((pbody + do_off, m))
        gen_st.append((pbody + do_off, m, f0, w, 0))
        reb_st.append((0, m, s0, w, 0))
        xor_st.append((out_x + do_off, len_x, x0, w, 0))
        qd.append(qbody + do_off)
        lost.append(bcp.PqLost(pbody + do_off, qbody + do_off, x, bcp.PQ_NONE, out_v + do_off, len_x, 0, 0))
        do_off += align(m)
        moved = sum(min(int(L), len_x) for k, L in enumerate(ls) if k != x) + 2 * len_x  # survivors, P, the store
        x_bytes += moved
        v_bytes += moved + len_x                                                        # and Q
        c_bytes += (w + 2) * m
    arr = lambda T, xs: (T * len(xs))(*[v if isinstance(v, T) else T(*v) for v in xs])  # noqa: E731
    gst, rst, xst = arr(bcp.Stripe, gen_st), arr(bcp.Stripe, reb_st), arr(bcp.Stripe, xor_st)
    fso, sso, xso = arr(bcp.Source, full), arr(bcp.Source, surv), arr(bcp.Source, xsrc)
    lo = arr(bcp.PqLost, lost)
    qb = (bcp.ctypes.c_uint64 * n)(*qd)
    L = bcp.lib()

    def verified():
        bcp.check("bcp_pq_rebuild_check_stripes_async",
                  L.bcp_pq_rebuild_check_stripes_async(q.h, rst, n, sso, len(surv), lo, bcp._V(vres)))

    def xor_rebuild():
        bcp.check("bcp_xor_stripes_async", L.bcp_xor_stripes_async(q.h, xst, n, xso, len(xsrc)))

    def syndrome():
        bcp.check("bcp_pq_check_stripes_async",
                  L.bcp_pq_check_stripes_async(q.h, gst, n, fso, len(full), qb, bcp._V(res)))

    bcp.check("bcp_pq_stripes_async", L.bcp_pq_stripes_async(q.h, gst, n, fso, len(full), qb))  # the bodies
    for _ in range(a.warmup):
        verified()
        xor_rebuild()
        syndrome()
    q.sync()
    forms = {}
    for key, fn in (("verified", verified), ("xor_rebuild", xor_rebuild), ("syndrome", syndrome)):
        fn()
        q.sync()
        forms[key] = dict(desc_form=eng.option("last_desc_form"), desc_vecs=eng.option("last_desc_vecs"))
    forms["pq_blocks_per_cu"] = eng.option("pq_blocks_per_cu")
    # 3 x steps launches back to back, a mark between each two (slots 0 .. 3 * steps)
    q.mark(0)
    for i in range(a.steps):
        verified()
        q.mark(3 * i + 1)
        xor_rebuild()
        q.mark(3 * i + 2)
        syndrome()
        q.mark(3 * i + 3)
    q.sync()
    v_ms = [q.elapsed_ms(3 * i, 3 * i + 1) for i in range(a.steps)]
    x_ms = [q.elapsed_ms(3 * i + 1, 3 * i + 2) for i in range(a.steps)]
    c_ms = [q.elapsed_ms(3 * i + 2, 3 * i + 3) for i in range(a.steps)]
    # every record clean, and the member the new form wrote is the XOR rebuild's
    vrecs, recs, diff = np.empty(2 * n, dtype=np.uint64), np.empty(4 * n, dtype=np.uint64), np.empty(1, dtype=np.uint64)
    q.compare(out_v, out_x, body_bytes, cmp8)
    q.d2h(vrecs, vres, vrecs.nbytes)
    q.d2h(recs, res, recs.nbytes)
    q.d2h(diff, cmp8, 8)
    q.sync()
    allf = np.uint64(2 ** 64 - 1)
    clean = bool((vrecs[0::2] == allf).all() and (vrecs[1::2] == 0).all() and (recs[0::4] == allf).all() and
                 (recs.reshape(n, 4)[:, 1:] == 0).all())
    same = int(diff[0]) == 0
    v, x, c = figures(v_ms[1:], v_bytes), figures(x_ms[1:], x_bytes), figures(c_ms[1:], c_bytes)  # first launch aside
    over_c, over_x = v["ms_median"] / c["ms_median"], v["ms_median"] / x["ms_median"]
    emit(a.out, shape=name, stripes=n, steps=a.steps, warmup=a.warmup, first_timed_launch_set_aside=True,
         verified_bytes_per_launch=v_bytes, xor_rebuild_bytes_per_launch=x_bytes, syndrome_bytes_per_launch=c_bytes,
         verified=v, xor_rebuild=x, syndrome=c, forms=forms,
         verified_ms_over_syndrome_ms=round(over_c, 4), syndrome_spread=c["spread"],
         within_syndrome_spread=bool(abs(over_c - 1.0) <= c["spread"]),
         verified_ms_over_xor_rebuild_ms=round(over_x, 4),
         verified_rate_over_xor_rebuild_rate=round(v["GBps"] / x["GBps"], 4),
         all_clean=clean, output_equals_xor_rebuild=same,
         verified_ms=[round(t, 4) for t in v_ms], xor_rebuild_ms=[round(t, 4) for t in x_ms],
         syndrome_ms=[round(t, 4) for t in c_ms])
    for p in (src, pbody, qbody, out_v, out_x, res, vres, cmp8):
        eng.free(p)
    return clean and same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stripes", type=int, default=0, help="stripes of the uniform batch (default: bench.py's)")
    ap.add_argument("--shapes", default="uniform,mixed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pqrebuild", "pq_rebuild_rate.jsonl"))
    a = ap.parse_args()
    assert 2 <= a.steps <= 21, "three marks per step, 64 timer slots; the first launch of each is set aside"
    import bench
    S = a.stripes or bench.default_stripes(1, 0)
    eng = bcp.Engine(0)
    q = eng.queue()
    cus, name = eng.info()
    emit(a.out, device=name, cus=cus, tool="pq_rebuild_rate")
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
