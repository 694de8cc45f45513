"""The check sink of the descriptor path (bcp_check_stripes_async): for every
stripe the bytes bcp_xor_stripes_async would store into [dst, dst + out_len)
are compared with the bytes already there, and one record per stripe comes
back: the smallest differing offset and the number of differing bytes, both
exact.  dst is only read.

Every expected body is uploaded with Dev.put at pads 0..15, so it lies between
random non-zero poison (an over-read at either end shows as a false mismatch),
is read back after the check and must be unchanged, and Dev.free finds every
guard intact: together these show the kernel stores nothing.  Expected records
are numpy's, from the oracle's fold."""
import os
import time

import numpy as np
import pytest

from devbuf import GuardError
from test_gpu_fuzz import TUNING, _batch
from test_gpu_xor import Dev

pytestmark = pytest.mark.gpu
KiB, MiB = 1024, 1024 * 1024
CLEAN = (2 ** 64 - 1, 0)
REC_FILL = 0xA5  # what the result records hold before a check


@pytest.fixture
def dev(engine, queue):
    d = Dev(engine, queue)
    yield d
    d.free()


def fold_ref(chunks, out_len, window=0):
    """What bcp_xor_stripes_async stores for these sources (None: a missing one)."""
    from oracle import gen_parity_file, xor_padded_np
    present = [np.zeros(0, np.uint8) if c is None else c for c in chunks]
    if window:
        body = np.frombuffer(gen_parity_file(present, window), dtype=np.uint8)[8 * len(present):]
    else:
        body = xor_padded_np(present)
    ref = np.zeros(out_len, np.uint8)
    k = min(len(body), out_len)
    ref[:k] = body[:k]
    return ref


def verdict(ref, body):
    w = np.flatnonzero(ref != body)
    return (int(w[0]), int(w.size)) if w.size else CLEAN


def upload_sources(dev, groups):
    """groups: list of (chunks, pads or None) -> per group the list of (ptr, len)."""
    ups = [(c, pad) for chunks, pads in groups
           for c, pad in zip(chunks, pads or [0] * len(chunks)) if c is not None]
    addrs = iter(dev.put_many(ups))
    return [[(0, 0) if c is None else (next(addrs), len(c)) for c in chunks] for chunks, _ in groups]


def submit_check(dev, queue, jobs, src_tables):
    """jobs: list of (group index, out_len, window, body, pad).  Uploads the
    bodies, submits one check batch and returns what is needed to collect it
    (no sync here: batches can be queued back to back)."""
    sources, first_of = [], []
    for tab in src_tables:
        first_of.append(len(sources))
        sources += tab
    body_ptrs = dev.put_many([(body, pad) for _, _, _, body, pad in jobs])
    descs = [(ptr, out_len, first_of[g], len(src_tables[g]), window)
             for ptr, (g, out_len, window, _, _) in zip(body_ptrs, jobs)]
    res = dev.alloc(16 * len(jobs), fill=REC_FILL)
    queue.check_stripes(descs, sources, res)
    return res, body_ptrs, jobs


def collect(dev, queue, pending):
    """Records of a submitted batch as (first_bad, bad_bytes) pairs; asserts
    that no body changed."""
    res, body_ptrs, jobs = pending
    raw = dev.get(res, 16 * len(jobs)).copy()
    got = [np.empty(max(len(j[3]), 1), np.uint8) for j in jobs]
    for g, ptr, j in zip(got, body_ptrs, jobs):
        if len(j[3]):
            queue.d2h(g, ptr, len(j[3]))
    queue.sync()
    for i, (g, j) in enumerate(zip(got, jobs)):
        assert np.array_equal(g[:len(j[3])], j[3]), f"stripe {i}: the check changed bytes of dst"
    recs = raw.view(np.uint64).reshape(-1, 2)
    return [(int(a), int(b)) for a, b in recs]


def run_check(dev, queue, jobs, src_tables):
    return collect(dev, queue, submit_check(dev, queue, jobs, src_tables))


def corrupted(ref, places):
    """A copy of ref with byte off ^= mask for every (off, mask)."""
    body = ref.copy()
    for off, mask in places:
        body[off] ^= mask
    return body


def boundary_shapes(T, rng):
    """(lens with None for a missing source, out_len, window) for tile size T."""
    shapes = []
    for out_len in (0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 17):
        for width in (1, 2, 8, 9, 56):
            lens = [out_len] + [int(x) for x in rng.integers(0, out_len + 1, size=width - 1)]
            if width >= 8 and out_len > 64:
                lens[1] = out_len // 2 // 16 * 16      # ends inside a tile at a multiple of 16
                lens[2] = out_len // 2 // 16 * 16 + 5  # ... and not
                lens[3] = None                          # a missing source (0, 0)
            shapes.append((lens, out_len, 0))
    shapes += [
        ([2 * T + 17, T + 160, T + 163, 48], 2 * T + 17, 0),       # sources ending inside a tile
        ([8 * T + 5, T // 2], 8 * T + 5, 0),                       # grouped: 1 source x 8 subtiles
        ([9 * T, 8 * T, 3 * T + 7], 9 * T, 0),                     # 2 covering sources
        ([8 * T, 8 * T, 8 * T, T + 1], 8 * T, 0),                  # 3
        ([8 * T, 8 * T, 8 * T, 8 * T, 100, None], 8 * T, 0),       # 4, and a missing one
        ([2 * T + 17, 2 * T, T], T + 5, 0),                        # rebuild truncation
        ([3 * T + 40, 3 * T, T], 3 * T, 0),                        # truncation at a tile boundary
        ([T + 3, 100], 2 * T + 17, 0),                             # a zero tail (whole tiles of it)
        ([21], T + 1, 0),
        ([40 * KiB + 5, 16 * KiB + 3, 0], 40 * KiB + 5, 16 * KiB),  # window replay
        ([40 * KiB + 5, 16 * KiB + 3, 0], 40 * KiB + 5 + T + 20, 16 * KiB),  # ... and out_len past the longest source
    ]
    return shapes


def corruption_sets(lens, out_len, window, T):
    """Lists of (offset, mask): one place per run, then several at once."""
    if out_len == 0:
        return []
    longest = max([x for x in lens if x is not None] + [0])
    v = out_len // 16 * 16  # start of the vector that straddles out_len (or out_len itself)
    places = {0, out_len - 1, 15, 16, T - 1, T, 2 * T - 1, 2 * T, v - 1, v, v - 16, v + 15 - 16}
    if out_len > longest:  # the zero tail
        places |= {longest, (longest + out_len) // 2}
    if window:             # a byte where a shorter source's last window is replayed
        places |= {2 * window + 1, 2 * window + 100}
    single = [[(p, 0xFF)] for p in sorted(places) if 0 <= p < out_len]
    multi = [[(out_len // 2, 0x10)]]  # a single flipped bit
    if out_len >= 16:
        base = (out_len // 2) // 16 * 16
        multi.append([(base + 1, 0x01), (base + 5, 0x80), (base + 14, 0x7E)])  # three bytes of one vector
        multi.append([(p, 0x40) for p in sorted({out_len - 1, out_len // 3, 17 % out_len, min(T, out_len - 1)})])
    return single + multi


@pytest.mark.parametrize("vecs", [1, 2, 4, 8, 16])
def test_boundary_shapes(oracle, engine, dev, queue, vecs):
    T = 4096 * vecs
    rng = np.random.default_rng(4100 + vecs)
    groups, jobs, want, what = [], [], [], []
    for lens, out_len, window in boundary_shapes(T, rng):
        chunks = [None if L is None else rng.integers(0, 256, size=L, dtype=np.uint8) for L in lens]
        g = len(groups)
        groups.append((chunks, [int(x) for x in rng.integers(0, 16, size=len(chunks))]))
        ref = fold_ref(chunks, out_len, window)
        for places in [[]] + corruption_sets(lens, out_len, window, T):
            body = corrupted(ref, places)
            jobs.append((g, out_len, window, body, len(jobs) % 16))
            want.append(verdict(ref, body))
            assert want[-1] == ((min(p for p, _ in places), len(places)) if places else CLEAN)
            what.append((lens, out_len, window, places))
    engine.option("desc_vecs_per_thread", vecs)
    try:
        got = run_check(dev, queue, jobs, upload_sources(dev, groups))
        assert engine.option("last_desc_form") == 3
        assert engine.option("last_desc_vecs") == vecs
    finally:
        engine.option("desc_vecs_per_thread", 0)
    bad = [(i, g, w, what[i]) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{len(bad)} of {len(jobs)} records wrong; first (index, got, want, shape): {bad[0]}"


def test_no_cross_stripe_leakage(oracle, dev, queue):
    rng = np.random.default_rng(77)
    groups, jobs, want = [], [], []
    for i in range(40):
        n = int(rng.integers(1, 10))
        lens = [int(x) for x in rng.integers(0, 200000, size=n)]
        chunks = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in lens]
        groups.append((chunks, [int(x) for x in rng.integers(0, 16, size=n)]))
        ref = fold_ref(chunks, max(lens))
        places = [(int(p), 0x21) for p in set(rng.integers(0, max(lens), size=3))] if i in (3, 17, 39) else []
        body = corrupted(ref, places)
        jobs.append((i, max(lens), 0, body, i % 16))
        want.append(verdict(ref, body))
    got = run_check(dev, queue, jobs, upload_sources(dev, groups))
    assert [i for i, g in enumerate(got) if g != CLEAN] == [3, 17, 39]
    assert got == want


def test_nothing_to_fold_still_initialises_the_records(dev, queue):
    src = upload_sources(dev, [([np.arange(100, dtype=np.uint8)], None), ([], None)])
    jobs = [(0, 0, 0, np.zeros(0, np.uint8), 3), (1, 0, 0, np.zeros(0, np.uint8), 0), (0, 0, 0, np.zeros(0, np.uint8), 9)]
    assert run_check(dev, queue, jobs, src) == [CLEAN] * 3


def test_whole_stripe_mismatch(oracle, dev, queue):
    """8 x 4 MiB, every byte of the body drawn afresh: every wave of every
    tile takes the mismatch path (the worst case for the atomics)."""
    rng = np.random.default_rng(5)
    n, L = 8, 4 * MiB
    chunks = [rng.integers(0, 256, size=L, dtype=np.uint8) for _ in range(n)]
    ref = fold_ref(chunks, L)
    body = rng.integers(0, 256, size=L, dtype=np.uint8)
    want = verdict(ref, body)
    assert want[1] > L * 0.99
    t0 = time.monotonic()
    got = run_check(dev, queue, [(0, L, 0, body, 7)], upload_sources(dev, [(chunks, None)]))
    print(f"whole-stripe mismatch: {want[1]} differing bytes, check + read-back {time.monotonic() - t0:.3f} s")
    assert got == [want]


def test_back_to_back_batches_keep_their_own_records(oracle, dev, queue):
    """Two check batches on one queue with no sync between them (the second
    takes the next descriptor slot), one clean and one corrupted."""
    rng = np.random.default_rng(11)
    groups, refs = [], []
    for i in range(20):
        lens = [int(x) for x in rng.integers(1, 150000, size=int(rng.integers(1, 9)))]
        chunks = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in lens]
        groups.append((chunks, [int(x) for x in rng.integers(0, 16, size=len(lens))]))
        refs.append(fold_ref(chunks, max(lens)))
    src = upload_sources(dev, groups)
    clean = [(i, len(r), 0, r, i % 16) for i, r in enumerate(refs)]
    dirty_bodies = [corrupted(r, [(len(r) - 1, 0x80), (len(r) // 2, 0x01)] if len(r) > 1 else [(0, 1)]) for r in refs]
    dirty = [(i, len(r), 0, b, (i + 5) % 16) for i, (r, b) in enumerate(zip(refs, dirty_bodies))]
    pending = [submit_check(dev, queue, jobs, src) for jobs in (clean, dirty, clean, dirty, clean)]  # slots wrap at 4
    got = [collect(dev, queue, p) for p in pending]
    assert got[0] == got[2] == got[4] == [CLEAN] * len(refs)
    assert got[1] == got[3] == [verdict(r, b) for r, b in zip(refs, dirty_bodies)]


def test_interleaved_with_the_fold(oracle, engine, dev, queue):
    """xor_stripes and check_stripes alternate on one queue over the same
    sources: the fold's own output, fed as the check's dst, is clean."""
    rng = np.random.default_rng(12)
    results = []
    for rnd in range(3):
        groups = []
        for i in range(24):  # past desc_args_max: the fold takes desc_tiles + xor_desc too
            lens = [int(x) for x in rng.integers(0, 120000, size=int(rng.integers(1, 12)))]
            groups.append(([rng.integers(0, 256, size=L, dtype=np.uint8) for L in lens],
                           [int(x) for x in rng.integers(0, 16, size=len(lens))]))
        tabs = upload_sources(dev, groups)
        sources, descs = [], []
        for i, tab in enumerate(tabs):
            out_len = max(L for _, L in tab)
            dst = dev.alloc(out_len + 32, fill=0xA5) + (i % 16)
            descs.append((dst, out_len, len(sources), len(tab), 0))
            sources += tab
        res = dev.alloc(16 * len(descs), fill=REC_FILL)
        queue.xor_stripes(descs, sources)
        queue.check_stripes(descs, sources, res)
        results.append((res, len(descs)))
    for res, n in results:
        recs = dev.get(res, 16 * n).view(np.uint64).reshape(-1, 2)
        assert [(int(a), int(b)) for a, b in recs] == [CLEAN] * n


def test_random_batches_match_numpy(oracle, engine, queue):
    budget = float(os.environ.get("BCP_FUZZ_SECONDS", "6"))
    seed = int(os.environ.get("BCP_FUZZ_SEED", "2027"))
    rng, xrng = np.random.default_rng(seed), np.random.default_rng([seed, 1])
    crng = np.random.default_rng([seed, 2])  # corruptions
    defaults = {k: engine.option(k) for k in TUNING}
    t_end = time.monotonic() + budget
    rounds = stripes_done = dirty_done = 0
    try:
        while time.monotonic() < t_end or rounds < 3:
            tuning = {k: (v[0] if rng.random() < 0.5 else v[int(rng.integers(0, len(v)))]) for k, v in TUNING.items()}
            for k, v in tuning.items():
                engine.option(k, v)
            stripes, refs = _batch(rng, 24 * MiB, xrng)
            groups = [(st["chunks"], st.get("pads")) for st in stripes]
            jobs, want = [], []
            for i, (st, ref) in enumerate(zip(stripes, refs)):
                places = []
                if len(ref) and crng.random() < 0.5:
                    offs = set(int(x) for x in crng.integers(0, len(ref), size=int(crng.integers(0, 5))))
                    places = [(o, int(crng.integers(1, 256))) for o in offs]
                body = corrupted(ref, places)
                jobs.append((i, st["out_len"], st.get("window", 0), body, st.get("dst_pad", 0)))
                want.append(verdict(ref, body))
            dev = Dev(engine, queue)
            try:
                try:
                    got = run_check(dev, queue, jobs, upload_sources(dev, groups))
                finally:
                    dev.free()
            except GuardError as e:
                pytest.fail(f"seed {seed} round {rounds} tuning {tuning}: {e}")
            assert engine.option("last_desc_form") == 3 or not any(j[1] for j in jobs)
            for i, (g, w) in enumerate(zip(got, want)):
                if g != w:
                    st = stripes[i]
                    lens = [0 if c is None else len(c) for c in st["chunks"]]
                    pytest.fail(f"seed {seed} round {rounds} stripe {i}: record {g}, numpy {w}; lens {lens} "
                                f"out_len {st['out_len']} window {st.get('window', 0)} pads {st.get('pads')} "
                                f"dst_pad {st.get('dst_pad', 0)} tuning {tuning}")
            rounds += 1
            stripes_done += len(stripes)
            dirty_done += sum(w != CLEAN for w in want)
    finally:
        for k, v in defaults.items():
            engine.option(k, v)
    print(f"check fuzz: {rounds} batches, {stripes_done} stripes, {dirty_done} of them corrupted")
    assert rounds >= 3
