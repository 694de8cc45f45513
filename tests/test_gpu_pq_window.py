"""The windowed forms of the P + Q kernel (bcp_pq_stripes_win_async,
bcp_pq_recover_stripes_win_async, bcp_pq_check_stripes_win_async) against the
replayed streams R_k of tests/pq_window.py (pinned to the oracle's parity body
by test_pq_window_cpu.py) and numpy's GF(2^8) (tests/gf256.py) over them.
Every comparison is byte-exact.

Sources and bodies are uploaded between random non-zero poison, outputs lie in
areas pre-filled with 0xA5 that are checked around the output, and Dev.free
reads every guard back (tests/devbuf.py).  W = 32 KiB unless stated, so a few
hundred KiB cover every case: full windows replayed, lengths below W, sources
that end inside a tile of their last window, length 0, two groups of four and
a remainder, an out_len that is no multiple of 16."""
import errno

import numpy as np
import pytest

import gf256 as G
from devbuf import FILL, SLACK, Dev, GuardError, assert_stripes_equal, gpu_stripes
from pq_window import LISTS, W, chunks_of, p_win, q_win, replay, replayed_places, rows

pytestmark = pytest.mark.gpu
KiB, MiB = 1024, 1024 * 1024
VECS = (4, 8)
CLEAN = (2 ** 64 - 1, 0, 0, 0)
BAD_P, BAD_Q, NOWHERE = 1 << 56, 1 << 57, 1 << 58
NONE = 0xFFFFFFFF
IDS = [f"n{len(x)}" for x in LISTS]


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


def _unchanged(queue, addrs, ups, what):
    got = [np.empty(max(len(a), 1), np.uint8) for a, _ in ups]
    for g, ptr, (a, _) in zip(got, addrs, ups):
        if len(a):
            queue.d2h(g, ptr, len(a))
    queue.sync()
    for i, (g, (a, _)) in enumerate(zip(got, ups)):
        assert np.array_equal(g[:len(a)], a), f"{what} {i} changed on the device"


def odd_pads(n, i=0):
    """Byte offsets of the sources from a 256-byte boundary: odd ones."""
    return [(2 * (i + 3 * k) + 1) % 16 for k in range(n)]


def stripe_of(lens, seed, window=W, i=0, p=True):
    chunks = chunks_of(lens, seed)
    return dict(chunks=chunks, out_len=max(lens), window=window, pads=odd_pads(len(lens), i),
                p_pad=(2 * i + 3) % 16 if p else None, q_pad=(6 * i + 5) % 16)


def gpu_gen(dev, queue, stripes, windowed=True):
    """stripes: dicts(chunks, out_len, window, pads, p_pad (None: dst = 0), q_pad) -> (P outputs, Q outputs)."""
    ups = [(np.ascontiguousarray(c, np.uint8), pad) for st in stripes for c, pad in zip(st["chunks"], st["pads"])]
    addrs = dev.put_many(ups)
    it = iter(addrs)
    descs, sources, q_dst, p_areas, q_areas = [], [], [], [], []
    for st in stripes:
        first = len(sources)
        sources += [(next(it), len(c)) for c in st["chunks"]]
        n = st["out_len"]
        if st["p_pad"] is not None:
            p_areas.append(_area(dev, st["p_pad"], n))
        q_areas.append(_area(dev, st["q_pad"], n))
        descs.append((p_areas[-1][0] + st["p_pad"] if st["p_pad"] is not None else 0, n, first, len(st["chunks"]),
                      st["window"]))
        q_dst.append(q_areas[-1][0] + q_areas[-1][1])
    queue.pq_stripes(descs, sources, q_dst, windowed=windowed)
    q_out = _collect(queue, q_areas, "Q of stripe")
    p_got = iter(_collect(queue, p_areas, "P of stripe"))
    p_out = [next(p_got) if st["p_pad"] is not None else None for st in stripes]
    _unchanged(queue, addrs, ups, "source")
    return p_out, q_out


def refs_of(st):
    return p_win(st["chunks"], st["window"], st["out_len"]), q_win(st["chunks"], st["window"], st["out_len"])


# ---------------------------------------------------------------------------
# GEN
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lens", LISTS, ids=IDS)
@pytest.mark.parametrize("vecs", VECS)
def test_gen_equals_the_reference_and_the_xor_path(oracle, engine, queue, dev, tuned, vecs, lens):
    tuned("desc_vecs_per_thread", vecs)
    st = stripe_of(lens, seed=len(lens) + vecs, i=vecs)
    p_out, q_out = gpu_gen(dev, queue, [st])
    assert engine.option("last_desc_form") == 7 and engine.option("last_desc_vecs") == vecs
    p_ref, q_ref = refs_of(st)
    body = np.frombuffer(oracle.gen_parity_file(st["chunks"], W), np.uint8)[8 * len(lens):]
    assert np.array_equal(p_ref, body)
    assert_stripes_equal(p_out, [p_ref], "P")
    assert_stripes_equal(q_out, [q_ref], "Q")
    # the same stripe with the same window through bcp_xor_stripes_async
    xor = gpu_stripes(dev, queue, [dict(chunks=st["chunks"], out_len=st["out_len"], window=W, pads=st["pads"],
                                        dst_pad=st["p_pad"])])
    assert_stripes_equal(p_out, xor, "P against the XOR path's")


@pytest.mark.parametrize("vecs", VECS)
def test_gen_q_only(engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    stripes = [stripe_of(lens, seed=20 + i, i=i, p=False) for i, lens in enumerate(LISTS)]
    # (dst = 0: a stray P store would land in a guard or an output's slack, or fault at address 0)
    p_out, q_out = gpu_gen(dev, queue, stripes)
    assert all(p is None for p in p_out)
    assert_stripes_equal(q_out, [refs_of(st)[1] for st in stripes], "Q")


@pytest.mark.parametrize("vecs", VECS)
def test_gen_one_batch_mixes_windows(engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    stripes = []
    for i, lens in enumerate(LISTS):
        stripes.append(stripe_of(lens, seed=30 + i, window=W, i=3 * i))
        stripes.append(stripe_of(lens, seed=40 + i, window=0, i=3 * i + 1))
        stripes.append(stripe_of(lens, seed=50 + i, window=2 * W, i=3 * i + 2))
    p_out, q_out = gpu_gen(dev, queue, stripes)
    assert engine.option("last_desc_form") == 7
    refs = [refs_of(st) for st in stripes]
    assert_stripes_equal(p_out, [r[0] for r in refs], "P")
    assert_stripes_equal(q_out, [r[1] for r in refs], "Q")
    # the stripes without a window are the plain P and Q
    for st, (p, q) in zip(stripes, refs):
        if st["window"] == 0:
            assert np.array_equal(p, G.p_of(st["chunks"], st["out_len"]))
            assert np.array_equal(q, G.q_sum(st["chunks"], st["out_len"]))


@pytest.mark.parametrize("vecs", VECS)
def test_gen_stripes_without_a_window_equal_the_old_entry_point(engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    stripes = [stripe_of(lens, seed=60 + i, window=0, i=i) for i, lens in enumerate(LISTS)]
    old = gpu_gen(dev, queue, stripes, windowed=False)
    assert engine.option("last_desc_form") == 4
    new = gpu_gen(dev, queue, stripes, windowed=True)
    assert_stripes_equal(new[0], old[0], "P")
    assert_stripes_equal(new[1], old[1], "Q")
    # and in a batch that takes the windowed kernel because another stripe has a window
    mixed = gpu_gen(dev, queue, stripes + [stripe_of(LISTS[1], seed=70, window=W, i=9)])
    assert engine.option("last_desc_form") == 7
    assert_stripes_equal(mixed[0][:-1], old[0], "P")
    assert_stripes_equal(mixed[1][:-1], old[1], "Q")


# ---------------------------------------------------------------------------
# SOLVE
# ---------------------------------------------------------------------------
def gpu_recover(dev, queue, jobs, window=W):
    """jobs: dicts(chunks (every member), x, y (None: only x, P lost too), i) -> list of (D_x, D_y or None).
    P and Q are the reference's over the replayed streams; out_len is the longest member's length."""
    ups, where = [], []
    for j in jobs:
        chunks, n = j["chunks"], max(len(c) for c in j["chunks"])
        pads = odd_pads(len(chunks), j["i"])
        surv = [(c, pad) for k, (c, pad) in enumerate(zip(chunks, pads)) if k not in (j["x"], j["y"])]
        bodies = [(q_win(chunks, window, n), (5 * j["i"] + 1) % 16)]
        if j["y"] is not None:
            bodies.append((p_win(chunks, window, n), (3 * j["i"] + 2) % 16))
        where.append((len(ups), len(surv), len(bodies)))
        ups += surv + bodies
    addrs = dev.put_many(ups)
    descs, sources, lost, x_areas, y_areas = [], [], [], [], []
    for j, (at, nsurv, nbody) in zip(jobs, where):
        chunks, n = j["chunks"], max(len(c) for c in j["chunks"])
        it = iter(addrs[at:at + nsurv])
        first = len(sources)
        sources += [(0, 0) if k in (j["x"], j["y"]) else (next(it), len(c)) for k, c in enumerate(chunks)]
        q = addrs[at + nsurv]
        p = addrs[at + nsurv + 1] if nbody == 2 else 0
        x_areas.append(_area(dev, (7 * j["i"] + 1) % 16, len(chunks[j["x"]])))
        dx = x_areas[-1][0] + x_areas[-1][1]
        dy = ly = 0
        if j["y"] is not None:
            y_areas.append(_area(dev, (9 * j["i"] + 3) % 16, len(chunks[j["y"]])))
            dy, ly = y_areas[-1][0] + y_areas[-1][1], len(chunks[j["y"]])
        descs.append((0, n, first, len(chunks), window))
        lost.append((p, q, j["x"], NONE if j["y"] is None else j["y"], dx, len(chunks[j["x"]]), dy, ly))
    queue.pq_recover(descs, sources, lost, windowed=True)
    xs = _collect(queue, x_areas, "D_x of stripe")
    ys = iter(_collect(queue, y_areas, "D_y of stripe"))
    _unchanged(queue, addrs, ups, "survivor or parity body")
    return [(x, next(ys) if j["y"] is not None else None) for x, j in zip(xs, jobs)]


@pytest.mark.parametrize("vecs", VECS)
def test_recover_every_pair_and_every_single_member(engine, queue, dev, tuned, vecs):
    """The 6-source list: the longest member (position 5) lost alone and in a pair, the member of length 0
    (position 3) lost, a member whose length is a multiple of W (4, 5)."""
    tuned("desc_vecs_per_thread", vecs)
    lens = LISTS[0]
    assert lens.index(max(lens)) == 5 and lens[3] == 0
    chunks = chunks_of(lens, seed=80 + vecs)
    n = len(lens)
    jobs = [dict(chunks=chunks, x=x, y=y, i=0) for x in range(n) for y in range(x + 1, n)]
    jobs += [dict(chunks=chunks, x=x, y=None, i=0) for x in range(n)]
    for i, j in enumerate(jobs):
        j["i"] = i
    assert len(jobs) == 15 + 6
    got = gpu_recover(dev, queue, jobs)
    assert engine.option("last_desc_form") == 8 and engine.option("last_desc_vecs") == vecs
    for j, (dx, dy) in zip(jobs, got):
        assert_stripes_equal([dx], [chunks[j["x"]]], f"(x={j['x']}, y={j['y']}) D_x")
        if j["y"] is not None:
            assert_stripes_equal([dy], [chunks[j["y"]]], f"(x={j['x']}, y={j['y']}) D_y")


@pytest.mark.parametrize("lens", LISTS[1:], ids=IDS[1:])
def test_recover_the_other_lists(engine, queue, dev, lens):
    chunks = chunks_of(lens, seed=90 + len(lens))
    n = len(lens)
    pairs = [(x, y) for x in range(n) for y in range(x + 1, n)]
    jobs = [dict(chunks=chunks, x=x, y=y, i=i) for i, (x, y) in enumerate(pairs[::max(1, len(pairs) // 6)])]
    jobs += [dict(chunks=chunks, x=x, y=None, i=x) for x in (0, n - 1)]
    for j, (dx, dy) in zip(jobs, gpu_recover(dev, queue, jobs)):
        assert_stripes_equal([dx], [chunks[j["x"]]], f"(x={j['x']}, y={j['y']}) D_x")
        if j["y"] is not None:
            assert_stripes_equal([dy], [chunks[j["y"]]], f"(x={j['x']}, y={j['y']}) D_y")


# ---------------------------------------------------------------------------
# CHECK
# ---------------------------------------------------------------------------
def ref_record(chunks, p, q, window, out_len):
    """The record by the definition, over the replayed streams."""
    r = rows(chunks, window, out_len)
    ps = p[:out_len] ^ G.p_of(r, out_len)
    qs = q[:out_len] ^ G.q_sum(r, out_len)
    bad = np.flatnonzero((ps != 0) | (qs != 0))
    members = 0
    if np.any((ps != 0) & (qs == 0)):
        members |= BAD_P
    if np.any((ps == 0) & (qs != 0)):
        members |= BAD_Q
    both = (ps != 0) & (qs != 0)
    for k in np.unique((G.LOG[qs[both]] - G.LOG[ps[both]]) % 255):
        members |= (1 << int(k)) if k < len(chunks) else NOWHERE
    return (int(bad[0]) if bad.size else 2 ** 64 - 1, int(np.count_nonzero(ps)), int(np.count_nonzero(qs)), members)


def gpu_check(dev, queue, stripes):
    """stripes: dicts(chunks, p, q, window, out_len, i) -> records."""
    ups = []
    for st in stripes:
        ups += [(np.ascontiguousarray(c, np.uint8), pad) for c, pad in zip(st["chunks"], odd_pads(len(st["chunks"]), st["i"]))]
        ups += [(st["p"], (3 * st["i"] + 1) % 16), (st["q"], (5 * st["i"] + 2) % 16)]
    addrs = dev.put_many(ups)
    it = iter(addrs)
    descs, sources, qb = [], [], []
    for st in stripes:
        first = len(sources)
        sources += [(next(it), len(c)) for c in st["chunks"]]
        descs.append((next(it), st["out_len"], first, len(st["chunks"]), st["window"]))
        qb.append(next(it))
    n = len(stripes)
    res = dev.alloc(32 * n, fill=FILL)
    queue.pq_check(descs, sources, qb, res, windowed=True)
    raw = dev.get(res, 32 * n).view(np.uint64).reshape(n, 4)
    _unchanged(queue, addrs, ups, "source or body")
    return [tuple(int(x) for x in r) for r in raw]


def flipped(a, at, x=0x5A):
    b = np.array(a, dtype=np.uint8, copy=True)
    b[at] ^= x
    return b


@pytest.mark.parametrize("vecs", VECS)
def test_check_clean_stripes(engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    stripes = []
    for i, lens in enumerate(LISTS):
        for window in (W, 0, 2 * W):
            chunks = chunks_of(lens, seed=100 + i)
            n = max(lens)
            stripes.append(dict(chunks=chunks, p=p_win(chunks, window, n), q=q_win(chunks, window, n), window=window,
                                out_len=n, i=len(stripes)))
    assert gpu_check(dev, queue, stripes) == [CLEAN] * len(stripes)
    assert engine.option("last_desc_form") == 9 and engine.option("last_desc_vecs") == vecs


@pytest.mark.parametrize("vecs", VECS)
def test_check_names_the_member_at_every_place_it_is_replayed_to(engine, queue, dev, tuned, vecs):
    tuned("desc_vecs_per_thread", vecs)
    lens = LISTS[0]                                  # [65541, 32771, 100, 0, 32768, 98304]
    chunks = chunks_of(lens, seed=110)
    n = max(lens)
    p, q = p_win(chunks, W, n), q_win(chunks, W, n)

    def st(i, ch=chunks, pb=p, qb=q):
        return dict(chunks=ch, p=pb, q=qb, window=W, out_len=n, i=i)

    def with_flip(k, at):
        return [flipped(c, at) if j == k else c for j, c in enumerate(chunks)]

    # a short source (len 100: window 0 with its padding replayed into windows 1 and 2)
    places2 = replayed_places(100, W, n, 50)
    assert places2 == [50, 50 + W, 50 + 2 * W]
    # a source ending inside a tile of its last window (len 32771: bytes 32768..32770 replayed into window 2)
    places1 = replayed_places(32771, W, n, 32769)
    assert places1 == [32769, 32769 + W]
    # a byte below the last window is not replayed
    assert replayed_places(65541, W, n, 7) == [7]
    two = with_flip(2, 50)
    two[0] = flipped(two[0], 7)
    stripes = [st(0, with_flip(2, 50)), st(1, with_flip(1, 32769)), st(2, with_flip(0, 7)),
               st(3, pb=flipped(p, 40000)), st(4, qb=flipped(q, n - 1)), st(5, two), st(6)]
    got = gpu_check(dev, queue, stripes)
    want = [(50, 3, 3, 1 << 2), (32769, 2, 2, 1 << 1), (7, 1, 1, 1 << 0),
            (40000, 1, 0, BAD_P), (n - 1, 0, 1, BAD_Q), (7, 4, 4, (1 << 2) | (1 << 0)), CLEAN]
    assert want == [ref_record(s["chunks"], s["p"], s["q"], W, n) for s in stripes]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f"stripe {i}: got first_bad={g[0]} p_bad={g[1]} q_bad={g[2]} members={g[3]:#x}, "
                        f"expected first_bad={w[0]} p_bad={w[1]} q_bad={w[2]} members={w[3]:#x}")


# ---------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------
def test_window_validation(bcp, engine, queue, dev):
    data = np.arange(64, dtype=np.uint8)
    src, body = dev.put(data), dev.put(data)
    out = dev.alloc(256, fill=FILL)
    res = dev.alloc(64, fill=FILL)
    E = -errno.EINVAL

    def gen(window):
        queue.pq_stripes([(out, 64, 0, 1, window)], [(src, 64)], [out + 128], windowed=True)

    def solve(window):
        queue.pq_recover([(0, 64, 0, 2, window)], [(0, 0), (src, 64)], [(0, body, 0, NONE, out, 64, 0, 0)], windowed=True)

    def check(window):
        queue.pq_check([(body, 64, 0, 1, window)], [(src, 64)], [body], res, windowed=True)

    for call in (gen, solve, check):
        for window in (16 * KiB, 48 * KiB, 16, 10 * MiB + 16):
            with pytest.raises(bcp.BcpError) as e:
                call(window)
            assert e.value.rc == E, (call.__name__, window)
    queue.sync()
    assert np.all(dev.get(out, 256) == FILL)
    for call in (gen, solve, check):
        for window in (32 * KiB, 10 * MiB, 0):
            call(window)
    queue.sync()
    # gen: Q = the source (one member, position 0); solve, the last to write `out`: D_0 = Q ^ g * D_1
    assert np.array_equal(dev.get(out + 128, 64), data)
    assert np.array_equal(dev.get(out, 64), data ^ G.mul(data, np.uint8(2)))
