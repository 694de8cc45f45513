"""The P + Q kernel (bcp_pq_stripes_async) and its recovery form
(bcp_pq_recover_stripes_async) against numpy's GF(2^8) (tests/gf256.py) and the
oracle's zero-padded XOR.

Every source, P body and Q body is uploaded with Dev.put_many between random
non-zero poison, every output area is pre-filled with 0xA5 and checked byte for
byte around the output, and Dev.free reads every guard back: a load outside a
source corrupts the result, a store outside an output fails the test.  Both
tile sizes the path can select (desc_vecs_per_thread 4 and 8: 16 and 32 KiB)
run every boundary shape."""
import errno

import numpy as np
import pytest

import gf256 as G
from devbuf import FILL, SLACK, Dev, GuardError, assert_stripes_equal

pytestmark = pytest.mark.gpu
KiB, MiB = 1024, 1024 * 1024
VECS = (4, 8)  # vectors per lane of the kernel's two variants; tile = 256 * 16 * vecs bytes


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


def _area(dev, pad, n):
    """An output area [pad | n | SLACK] holding 0xA5; returns (base, pad, n)."""
    return dev.alloc(pad + n + SLACK, fill=FILL), pad, n


def _collect(queue, areas, what):
    """Read the areas back; every byte outside [dst, dst + n) must still be 0xA5."""
    got = [np.empty(pad + n + SLACK, dtype=np.uint8) for _, pad, n in areas]
    for (base, _, _), a in zip(areas, got):
        queue.d2h(a, base, a.size)
    queue.sync()
    outs = []
    for i, ((_, pad, n), a) in enumerate(zip(areas, got)):
        for part, off0 in ((a[:pad], -pad), (a[pad + n:], n)):
            w = np.flatnonzero(part != FILL)
            if w.size:
                raise GuardError(f"{what} {i}: byte at offset {off0 + int(w[0])} from dst (length {n}) was overwritten "
                                 f"with 0x{int(part[w[0]]):02x}; {w.size} bytes outside the output changed")
        outs.append(a[pad:pad + n])
    return outs


def _unchanged(queue, uploads, what):
    """uploads: list of (ptr, array): the device copy must equal the array."""
    got = [np.empty(max(len(a), 1), np.uint8) for _, a in uploads]
    for g, (ptr, a) in zip(got, uploads):
        if len(a):
            queue.d2h(g, ptr, len(a))
    queue.sync()
    for i, (g, (_, a)) in enumerate(zip(got, uploads)):
        assert np.array_equal(g[:len(a)], a), f"{what} {i} changed on the device"


def gpu_pq(dev, queue, stripes, check_sources=True):
    """stripes: dicts(chunks=[array | None], out_len, pads, p_pad (None: no P), q_pad) -> (P outputs with
    None where no P was asked for, Q outputs).  A None chunk is the source (0, 0), an empty array a source
    of length 0 at a valid, poisoned address."""
    ups = [(c, pad) for st in stripes
           for c, pad in zip(st["chunks"], st.get("pads") or [0] * len(st["chunks"])) if c is not None]
    addrs = dev.put_many(ups)
    it = iter(addrs)
    descs, sources, q_dst, p_areas, q_areas = [], [], [], [], []
    for st in stripes:
        first = len(sources)
        for c in st["chunks"]:
            sources.append((0, 0) if c is None else (next(it), len(c)))
        n = st["out_len"]
        p_pad = st.get("p_pad", 0)
        if p_pad is not None:
            p_areas.append(_area(dev, p_pad, n))
        q_areas.append(_area(dev, st.get("q_pad", 0), n))
        descs.append((p_areas[-1][0] + p_pad if p_pad is not None else 0, n, first, len(st["chunks"]), 0))
        q_dst.append(q_areas[-1][0] + q_areas[-1][1])
    queue.pq_stripes(descs, sources, q_dst)
    q_out = _collect(queue, q_areas, "Q of stripe")
    p_got = iter(_collect(queue, p_areas, "P of stripe"))
    p_out = [next(p_got) if st.get("p_pad", 0) is not None else None for st in stripes]
    if check_sources:
        _unchanged(queue, [(a, np.ascontiguousarray(c, np.uint8)) for a, (c, _) in zip(addrs, ups)], "source")
    return p_out, q_out


def pq_refs(oracle, st):
    present = [np.zeros(0, np.uint8) if c is None else c for c in st["chunks"]]
    body = oracle.xor_padded_np(present)
    p = np.zeros(st["out_len"], np.uint8)
    k = min(len(body), st["out_len"])
    p[:k] = body[:k]
    return p, G.q_sum(st["chunks"], st["out_len"])


def boundary_stripes(T, rng):
    stripes = []
    i = 0
    for out_len in (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 17):
        for width in (1, 2, 3, 8, 9, 56):
            lens = [int(x) for x in rng.integers(0, out_len + 1, size=width)]
            lens[int(rng.integers(0, width))] = out_len
            chunks = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in lens]
            if width >= 8 and out_len > 64:
                inside = (out_len - 40) // 16 * 16                                     # ends inside the last tile ...
                chunks[1] = rng.integers(0, 256, size=inside, dtype=np.uint8)          # ... at a multiple of 16
                chunks[2] = rng.integers(0, 256, size=inside + 5, dtype=np.uint8)      # ... and 5 bytes further
                chunks[3] = None                                                        # the source (0, 0)
                chunks[4] = np.zeros(0, np.uint8)                                       # empty, at a valid address
            stripes.append(dict(chunks=chunks, out_len=out_len, pads=[(i * 7 + 3 * k) % 16 for k in range(width)],
                                p_pad=(i * 5 + 1) % 16, q_pad=(i * 11 + 2) % 16))
            i += 1
    # every source ends before the output does (a zero tail), sources end inside the first and second tile,
    # and one source is longer than the output (cut)
    stripes.append(dict(chunks=[rng.integers(0, 256, size=L, dtype=np.uint8) for L in (T + 160, T + 163, 48, 2 * T)],
                        out_len=2 * T + 17, pads=[1, 2, 3, 4], p_pad=9, q_pad=6))
    stripes.append(dict(chunks=[rng.integers(0, 256, size=L, dtype=np.uint8) for L in (3 * T, T + 5, 7)],
                        out_len=T + 21, pads=[15, 0, 8], p_pad=0, q_pad=0))
    return stripes


@pytest.mark.parametrize("host_max", (4096, 0, 1 << 24))  # the tables: by size, always copied, always read in place
@pytest.mark.parametrize("vecs", VECS)
def test_gen_boundary_shapes(oracle, engine, queue, dev, tuned, vecs, host_max):
    tuned("desc_vecs_per_thread", vecs)
    tuned("table_host_max", host_max)
    T = 256 * 16 * vecs
    stripes = boundary_stripes(T, np.random.default_rng(100 + vecs))
    p_out, q_out = gpu_pq(dev, queue, stripes)
    assert engine.option("last_desc_form") == 4 and engine.option("last_desc_vecs") == vecs
    refs = [pq_refs(oracle, st) for st in stripes]
    assert_stripes_equal(p_out, [r[0] for r in refs], "P")
    assert_stripes_equal(q_out, [r[1] for r in refs], "Q")


@pytest.mark.parametrize("vecs", VECS)
def test_gen_without_p_stores_no_p(oracle, engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(7)
    chunks = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in (T + 33, T // 2, 2 * T + 5)]
    stripes = [dict(chunks=chunks, out_len=2 * T + 5, pads=[3, 0, 9], p_pad=None, q_pad=5),
               dict(chunks=chunks, out_len=2 * T + 5, pads=[1, 2, 3], p_pad=7, q_pad=0)]
    # (no P address: a stray P store would land in a guard or an output's slack, or fault at address 0)
    p_out, q_out = gpu_pq(dev, queue, stripes)
    p_ref, q_ref = pq_refs(oracle, stripes[1])
    assert p_out[0] is None
    assert_stripes_equal(q_out, [q_ref, q_ref], "Q")
    assert_stripes_equal(p_out[1:], [p_ref], "P")


@pytest.mark.parametrize("blocks", (2, 1, 3))  # workgroups per CU (the default first); tile size by the engine
def test_gen_many_small_stripes_in_one_batch(oracle, engine, queue, dev, tuned, blocks):
    tuned("pq_blocks_per_cu", blocks)
    rng = np.random.default_rng(8)
    stripes = []
    for i in range(320):
        width = int(rng.integers(1, 10))
        out_len = int(rng.integers(0, 700))
        chunks = [rng.integers(0, 256, size=int(rng.integers(0, out_len + 1)), dtype=np.uint8) for _ in range(width)]
        stripes.append(dict(chunks=chunks, out_len=out_len, pads=[int(x) for x in rng.integers(0, 16, size=width)],
                            p_pad=int(rng.integers(0, 16)), q_pad=int(rng.integers(0, 16))))
    p_out, q_out = gpu_pq(dev, queue, stripes, check_sources=False)
    refs = [pq_refs(oracle, st) for st in stripes]
    assert_stripes_equal(p_out, [r[0] for r in refs], "P")
    assert_stripes_equal(q_out, [r[1] for r in refs], "Q")


@pytest.mark.parametrize("grid", (3, 0))
def test_gen_more_tiles_than_workgroups(oracle, engine, queue, dev, tuned, grid):
    """grid 3: three workgroups take ~60 tiles; grid 0: the default launch (two workgroups per CU) and a
    batch of more 16 KiB tiles than that."""
    tuned("desc_vecs_per_thread", 4)
    tuned("desc_grid", grid)
    T = 16 * KiB
    rng = np.random.default_rng(9)
    ncus = engine.info()[0] if grid == 0 else 0
    ntiles = 60 if grid else 2 * ncus + 77
    per = 20 if grid else (ntiles + 3) // 4
    stripes = []
    for s in range((ntiles + per - 1) // per):
        out_len = per * T - 1000 * s
        chunks = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in (out_len, out_len // 2 + 3, out_len - T - 1)]
        stripes.append(dict(chunks=chunks, out_len=out_len, pads=[0, 5, 11], p_pad=s % 16, q_pad=(3 * s) % 16))
    p_out, q_out = gpu_pq(dev, queue, stripes, check_sources=False)
    refs = [pq_refs(oracle, st) for st in stripes]
    assert_stripes_equal(p_out, [r[0] for r in refs], "P")
    assert_stripes_equal(q_out, [r[1] for r in refs], "Q")


def test_gen_refuses_bad_arguments(bcp, engine, queue, dev):
    src = dev.put(np.arange(64, dtype=np.uint8))
    out = dev.alloc(256, fill=FILL)
    E = -errno.EINVAL

    def rc(stripes, sources, q_dst):
        with pytest.raises(bcp.BcpError) as e:
            queue.pq_stripes(stripes, sources, q_dst)
        return e.value.rc

    ok_src = [(src, 64)]
    assert rc([(out, 64, 0, 1, 16 * KiB)], ok_src, [out + 128]) == E      # a window
    assert rc([(out, 64, 0, 1, 10 * MiB)], ok_src, [out + 128]) == E
    assert rc([(out, 64, 0, 57, 0)], ok_src * 57, [out + 128]) == E        # wider than BCP_MAX_SOURCES
    assert rc([(out, 64, 0, 2, 0)], ok_src, [out + 128]) == E              # sources outside the table
    assert rc([(out, 64, 0, 1, 0)], ok_src, [0]) == E                      # no Q body
    assert rc([(out, 64, 0, 1, 0)], [(0, 64)], [out + 128]) == E           # a source without an address
    queue.sync()
    assert np.all(dev.get(out, 256) == FILL)


def gpu_recover(dev, queue, jobs):
    """jobs: dicts(chunks (every member), x, y (None: only x, and P is lost too), out_len, len_x, len_y,
    pads, dx_pad, dy_pad, p_pad, q_pad) -> list of (D_x, D_y or None).  P and Q are numpy's."""
    ups, where = [], []
    for j in jobs:
        n = j["out_len"]
        lost = {j["x"], j["y"]}
        pads = j.get("pads") or [0] * len(j["chunks"])
        surv = [(c, pad) for k, (c, pad) in enumerate(zip(j["chunks"], pads)) if k not in lost and c is not None]
        bodies = [(G.q_sum(j["chunks"], n), j.get("q_pad", 0))]
        if j["y"] is not None:
            bodies.append((G.p_of(j["chunks"], n), j.get("p_pad", 0)))
        where.append((len(ups), len(surv), len(bodies)))
        ups += surv + bodies
    addrs = dev.put_many(ups)
    descs, sources, lost_recs, x_areas, y_areas = [], [], [], [], []
    for j, (at, nsurv, nbody) in zip(jobs, where):
        it = iter(addrs[at:at + nsurv])
        first = len(sources)
        for k, c in enumerate(j["chunks"]):
            sources.append((0, 0) if k in (j["x"], j["y"]) or c is None else (next(it), len(c)))
        q = addrs[at + nsurv]
        p = addrs[at + nsurv + 1] if nbody == 2 else 0
        x_areas.append(_area(dev, j.get("dx_pad", 0), j["len_x"]))
        dx = x_areas[-1][0] + x_areas[-1][1]
        dy = ly = 0
        if j["y"] is not None:
            y_areas.append(_area(dev, j.get("dy_pad", 0), j["len_y"]))
            dy, ly = y_areas[-1][0] + y_areas[-1][1], j["len_y"]
        descs.append((0, j["out_len"], first, len(j["chunks"]), 0))
        lost_recs.append((p, q, j["x"], 0xFFFFFFFF if j["y"] is None else j["y"], dx, j["len_x"], dy, ly))
    queue.pq_recover(descs, sources, lost_recs)
    xs = _collect(queue, x_areas, "D_x of stripe")
    ys = iter(_collect(queue, y_areas, "D_y of stripe"))
    _unchanged(queue, [(a, np.ascontiguousarray(c, np.uint8)) for a, (c, _) in zip(addrs, ups)], "survivor or parity body")
    return [(x, next(ys) if j["y"] is not None else None) for x, j in zip(xs, jobs)]


def _check_recovered(jobs, got):
    for i, (j, (dx, dy)) in enumerate(zip(jobs, got)):
        full = G.padded(j["chunks"], j["out_len"])
        assert_stripes_equal([dx], [full[j["x"]][:j["len_x"]]], f"job {i} (x={j['x']}, y={j['y']}) D_x")
        if j["y"] is not None:
            assert_stripes_equal([dy], [full[j["y"]][:j["len_y"]]], f"job {i} (x={j['x']}, y={j['y']}) D_y")


def _stripe(rng, width, out_len):
    lens = [int(x) for x in rng.integers(0, out_len + 1, size=width)]
    lens[int(rng.integers(0, width))] = out_len
    return [rng.integers(0, 256, size=L, dtype=np.uint8) for L in lens]


@pytest.mark.parametrize("vecs", VECS)
def test_recover_every_pair_of_a_9_wide_stripe(engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(20 + vecs)
    out_len = T + 4096 + 13
    chunks = _stripe(rng, 9, out_len)
    chunks[4] = rng.integers(0, 256, size=T // 2 + 5, dtype=np.uint8)  # a survivor ending inside the first tile
    cuts = (0, 1, out_len - 1, out_len)
    jobs, i = [], 0
    for x in range(9):
        for y in range(x + 1, 9):
            jobs.append(dict(chunks=chunks, x=x, y=y, out_len=out_len, len_x=cuts[i % 4], len_y=cuts[(i // 4 + 1) % 4],
                             pads=[(i + 3 * k) % 16 for k in range(9)], dx_pad=(5 * i + 1) % 16, dy_pad=(3 * i + 2) % 16,
                             p_pad=i % 16, q_pad=(7 * i) % 16))
            i += 1
    assert len(jobs) == 36
    got = gpu_recover(dev, queue, jobs)
    assert engine.option("last_desc_form") == 5 and engine.option("last_desc_vecs") == vecs
    _check_recovered(jobs, got)


@pytest.mark.parametrize("vecs", VECS)
def test_recover_pairs_of_a_56_wide_stripe(engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(30 + vecs)
    out_len = T + 777
    chunks = _stripe(rng, 56, out_len)
    chunks[5] = None
    jobs = [dict(chunks=chunks, x=x, y=y, out_len=out_len, len_x=lx, len_y=ly, pads=[(x + k) % 16 for k in range(56)],
                 dx_pad=3, dy_pad=14, p_pad=1, q_pad=15)
            for (x, y), (lx, ly) in zip(((0, 1), (0, 55), (27, 28), (54, 55)),
                                        ((out_len, out_len), (out_len - 1, 1), (T + 1, out_len), (16, T)))]
    _check_recovered(jobs, gpu_recover(dev, queue, jobs))


@pytest.mark.parametrize("host_max", (4096, 0))
@pytest.mark.parametrize("vecs", VECS)
def test_recover_from_q_alone(engine, queue, dev, tuned, vecs, host_max):
    """P is lost too: every x of a 9-wide stripe, and x = 55 of a 56-wide one."""
    tuned("desc_vecs_per_thread", vecs)
    tuned("table_host_max", host_max)
    T = 256 * 16 * vecs
    rng = np.random.default_rng(40 + vecs)
    out_len = 2 * T + 17
    nine, wide = _stripe(rng, 9, out_len), _stripe(rng, 56, T // 2 + 3)
    cuts = (out_len, 0, 1, out_len - 1)
    jobs = [dict(chunks=nine, x=x, y=None, out_len=out_len, len_x=cuts[x % 4], len_y=0,
                 pads=[(x + 5 * k) % 16 for k in range(9)], dx_pad=(x * 3 + 1) % 16, q_pad=(x * 9) % 16) for x in range(9)]
    jobs.append(dict(chunks=wide, x=55, y=None, out_len=T // 2 + 3, len_x=T // 2 + 3, len_y=0, dx_pad=7, q_pad=9))
    jobs.append(dict(chunks=wide, x=0, y=None, out_len=T // 2 + 3, len_x=T // 2 + 2, len_y=0, dx_pad=0, q_pad=0))
    _check_recovered(jobs, gpu_recover(dev, queue, jobs))


def test_recover_refuses_bad_arguments(bcp, engine, queue, dev):
    data = np.arange(64, dtype=np.uint8)
    a, p, q = dev.put(data), dev.put(data), dev.put(data)
    out = dev.alloc(256, fill=FILL)
    E = -errno.EINVAL
    NONE = bcp.PQ_NONE
    stripe = [(0, 64, 0, 3, 0)]
    srcs = [(0, 0), (a, 64), (0, 0)]

    def rc(lost, stripes=stripe, sources=srcs):
        with pytest.raises(bcp.BcpError) as e:
            queue.pq_recover(stripes, sources, [lost])
        return e.value.rc

    assert rc((p, q, 0, 2, out, 64, out + 128, 64), stripes=[(0, 64, 0, 3, 16 * KiB)]) == E   # a window
    assert rc((p, q, 3, NONE, out, 64, 0, 0)) == E                     # x outside the stripe
    assert rc((p, q, 2, 0, out, 64, out + 128, 64)) == E               # y below x
    assert rc((p, q, 0, 0, out, 64, out + 128, 64)) == E               # y == x
    assert rc((p, q, 0, 3, out, 64, out + 128, 64)) == E               # y outside the stripe
    assert rc((p, q, 0, NONE, out, 64, 0, 0)) == E                     # P present and one loss: RAID-5
    assert rc((0, q, 0, 2, out, 64, out + 128, 64)) == E               # two losses need P
    assert rc((p, 0, 0, 2, out, 64, out + 128, 64)) == E               # no Q body
    assert rc((p, q, 0, 1, out, 64, out + 128, 64)) == E               # position 1 is lost but has a source
    assert rc((0, q, 1, NONE, out, 64, 0, 0)) == E                     # the same with P lost
    assert rc((p, q, 0, 2, out, 65, out + 128, 64)) == E               # len_x above out_len
    assert rc((p, q, 0, 2, out, 64, out + 128, 65)) == E               # len_y above out_len
    assert rc((p, q, 0, 2, out, 64, out + 128, 64), stripes=[(0, 64, 0, 57, 0)], sources=srcs * 19) == E
    queue.sync()
    assert np.all(dev.get(out, 256) == FILL)
