#!/usr/bin/env python3
"""Rate of the check kernel (bcp_check_stripes_async) beside the fold
(bcp_xor_stripes_async) on the same descriptors, in one process.

Device-resident synthetic sources (bcp_dev_fill_synthetic_async); the bodies
are what the fold itself stored, so every check is clean (its clean path: the
loads, one ballot per tile, no store, no atomic).  Two shapes:

  mixed    the config-5 shapes bench.py --mode mixed draws (8-wide stripes,
           log-uniform 64 KiB - 4 MiB chunks, zero-padded to the stripe max)
  uniform  8 x 512 KiB stripes, as many as bench.py's default run (the fold
           takes the pointer-table xor_stream for these, the check its own
           staged form: check batches never take the uniform form)

Fold and check launches alternate on one queue, back to back, --steps timed
ones each after --warmup pairs, each between two of the queue's HIP-event
marks.  Bytes are counted alike for both: (n + 1) x out_len per stripe.  The
yardstick for the check is the fold of the same run: the ratio of the medians
is printed beside each kernel's launch-to-launch spread ((max - min) / median).

--e2e adds one end-to-end figure: on the in-memory config-5 store of
tools/e2e_bench.py, Pipeline.run and Pipeline.verify alternate --e2e-reps
times each; GiB/s of the bytes each run read.

One JSON line per figure, on stdout and appended to --out
(default profiles/scrub/check_rate.jsonl).

    python tools/check_rate.py [--steps 20] [--warmup 3] [--stripes 12500] [--e2e]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

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
    """lens_all: per stripe the source lengths; sources and outputs at 256-byte pitch."""
    align = lambda x: (x + 255) & ~255  # noqa: E731
    src_bytes = sum(sum(align(int(x)) for x in ls) for ls in lens_all)
    out_bytes = sum(align(int(max(ls))) for ls in lens_all)
    src, out = eng.alloc(src_bytes), eng.alloc(out_bytes)
    res = eng.alloc(16 * len(lens_all))
    q.fill_synthetic(src, src_bytes, seed=1)
    stripes, sources, so_off, do_off = [], [], 0, 0
    for ls in lens_all:
        first = len(sources)
        for x in ls:
            sources.append((src + so_off, int(x)))
            so_off += align(int(x))
        m = int(max(ls))
        stripes.append((out + do_off, m, first, len(ls), 0))
        do_off += align(m)
    st = (bcp.Stripe * len(stripes))(*[bcp.Stripe(*x) for x in stripes])
    so = (bcp.Source * len(sources))(*[bcp.Source(*x) for x in sources])
    L = bcp.lib()
    nbytes = sum((len(ls) + 1) * int(max(ls)) for ls in lens_all)

    def fold():
        bcp.check("bcp_xor_stripes_async", L.bcp_xor_stripes_async(q.h, st, len(stripes), so, len(sources)))

    def check():
        bcp.check("bcp_check_stripes_async",
                  L.bcp_check_stripes_async(q.h, st, len(stripes), so, len(sources), bcp._V(res)))

    for _ in range(a.warmup):
        fold()
        check()
    q.sync()
    forms = {}
    fold()
    q.sync()
    forms["fold"] = dict(desc_form=eng.option("last_desc_form"), desc_vecs=eng.option("last_desc_vecs"),
                         stream_vecs=eng.option("last_stream_vecs"))
    check()
    q.sync()
    forms["check"] = dict(desc_form=eng.option("last_desc_form"), desc_vecs=eng.option("last_desc_vecs"))
    # 2 x steps launches back to back, a mark between each two (slots 0 .. 2 * steps)
    q.mark(0)
    for i in range(a.steps):
        fold()
        q.mark(2 * i + 1)
        check()
        q.mark(2 * i + 2)
    q.sync()
    fold_ms = [q.elapsed_ms(2 * i, 2 * i + 1) for i in range(a.steps)]
    check_ms = [q.elapsed_ms(2 * i + 1, 2 * i + 2) for i in range(a.steps)]
    # the checks were clean: every record {UINT64_MAX, 0}
    import numpy as np
    recs = np.empty(2 * len(stripes), dtype=np.uint64)
    q.d2h(recs, res, recs.nbytes)
    q.sync()
    clean = bool((recs[0::2] == np.uint64(2 ** 64 - 1)).all() and (recs[1::2] == 0).all())
    f, c = figures(fold_ms, nbytes), figures(check_ms, nbytes)
    emit(a.out, shape=name, stripes=len(stripes), bytes_per_launch=nbytes, steps=a.steps, warmup=a.warmup,
         fold=f, check=c, forms=forms, check_over_fold=round(c["ms_median"] / f["ms_median"], 4),
         all_clean=clean, fold_ms=[round(x, 4) for x in fold_ms], check_ms=[round(x, 4) for x in check_ms])
    for p in (src, out, res):
        eng.free(p)
    return clean


def e2e(a):
    """Pipeline.run and Pipeline.verify alternating on the config-5 store of tools/e2e_bench.py."""
    import numpy as np
    import bcp_store as S
    import e2e_bench
    root = os.path.join(a.e2e_root, "c5_scrub")
    shutil.rmtree(root, ignore_errors=True)
    rng = np.random.default_rng(5)
    ntargets, files = 9, []
    for i in range(a.e2e_stripes):
        holders, p = S.random_layout(rng, ntargets, 8)
        lens = [int(x) for x in np.exp(rng.uniform(np.log(64 * KiB), np.log(4 * MiB), size=8))]
        files.append((f"u{i % 8}/{(i * 2654435761) % 65536:04X}/chunk{i}", holders, p, lens))
    e2e_bench.write_store(root, files, 2)
    ts = int(time.time()) + 3600  # nothing is stale
    items = [(path, ts, S.with_p(sum(1 << h for h in holders), p)) for path, holders, p, _ in files]
    ndev = max(1, bcp.device_count())
    pl = bcp.Pipeline(ndevices=ndev)
    try:
        pl.run(root, ntargets, items)  # cold: the parity files exist from here on
        gen, ver = [], []
        for _ in range(a.e2e_reps):
            t0 = time.perf_counter()
            st = pl.run(root, ntargets, items)
            gen.append((time.perf_counter() - t0, st.bytes_read, st.errors))
            t0 = time.perf_counter()
            vs, _ = pl.verify(root, ntargets, items)
            ver.append((time.perf_counter() - t0, vs.bytes_read, vs.errors))
            assert vs.ok == len(items) and vs.errors == 0, (vs.ok, vs.stale, vs.mismatch, vs.errors)
    finally:
        pl.close()
        shutil.rmtree(root, ignore_errors=True)
    for name, runs in (("pipeline_run", gen), ("pipeline_verify", ver)):
        rates = [b / s / GiB for s, b, _ in runs]
        emit(a.out, e2e=name, store="config 5, in memory", stripes=len(files), gpus=ndev,
             GiBps_read_median=round(statistics.median(rates), 3), GiBps_read=[round(x, 3) for x in rates],
             seconds=[round(s, 4) for s, _, _ in runs], bytes_read=runs[0][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stripes", type=int, default=0, help="stripes of the uniform batch (default: bench.py's)")
    ap.add_argument("--shapes", default="mixed,uniform")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-stripes", type=int, default=1000)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--e2e-root", default="/dev/shm" if os.path.isdir("/dev/shm") else os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub", "check_rate.jsonl"))
    a = ap.parse_args()
    assert 1 <= a.steps <= 31, "two marks per step, 64 timer slots"
    import bench
    S = a.stripes or bench.default_stripes(1, 0)
    ok = True
    if a.shapes:
        eng = bcp.Engine(0)
        q = eng.queue()
        cus, name = eng.info()
        emit(a.out, device=name, cus=cus, tool="check_rate")
        for shape in a.shapes.split(","):
            if shape == "mixed":
                lens_all = [[int(x) for x in ls] for ls in bench.mixed_lengths(S, 8, 512 * KiB, 0)]
            else:
                lens_all = [[512 * KiB] * 8] * S
            ok &= device_shape(a, eng, q, shape, lens_all)
        q.close()
        eng.close()
    if a.e2e:
        e2e(a)
    sys.exit(0 if ok else 3)


if __name__ == "__main__":
    main()
