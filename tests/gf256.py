"""GF(2^8) for the Q parity tests: polynomial x^8+x^4+x^3+x^2+1 (0x11d),
generator g = 2 (the RAID-6 convention).  Tables are built here from the
polynomial; nothing is taken from the library under test.

    P[j] = XOR_k D_k[j]        Q[j] = XOR_k g^k * D_k[j]

with every source zero-padded to out_len."""
import numpy as np

POLY = 0x11D

EXP = np.zeros(510, dtype=np.uint8)
LOG = np.zeros(256, dtype=np.int32)
_x = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= POLY
del _x, _i


def gpow(e: int) -> int:
    """g^e for any integer e."""
    return int(EXP[e % 255])


def mul(a, b):
    """Product of two field elements or arrays of them (uint8)."""
    a = np.asarray(a, dtype=np.uint8)
    b = np.asarray(b, dtype=np.uint8)
    out = EXP[(LOG[a] + LOG[b]) % 255]
    return np.where((a == 0) | (b == 0), np.uint8(0), out).astype(np.uint8)


def div(a: int, b: int) -> int:
    assert b != 0
    return 0 if a == 0 else int(EXP[(int(LOG[a]) - int(LOG[b])) % 255])


def padded(chunks, out_len):
    """[len(chunks)][out_len] uint8: every chunk cut or zero-padded to out_len
    (None: a missing source)."""
    rows = np.zeros((len(chunks), out_len), dtype=np.uint8)
    for k, c in enumerate(chunks):
        if c is not None:
            n = min(len(c), out_len)
            rows[k, :n] = np.asarray(c, dtype=np.uint8)[:n]
    return rows


def p_of(chunks, out_len):
    rows = padded(chunks, out_len)
    return np.bitwise_xor.reduce(rows, axis=0) if len(chunks) else np.zeros(out_len, np.uint8)


def q_sum(chunks, out_len):
    """Q by the definition: the sum of g^k * D_k."""
    rows = padded(chunks, out_len)
    q = np.zeros(out_len, dtype=np.uint8)
    for k in range(len(chunks)):
        q ^= mul(rows[k], np.uint8(gpow(k)))
    return q


def q_horner(chunks, out_len):
    """Q in Horner form: q = 0; for k = n-1 .. 0: q = 2*q ^ D_k."""
    rows = padded(chunks, out_len)
    q = np.zeros(out_len, dtype=np.uint8)
    for k in range(len(chunks) - 1, -1, -1):
        q = mul(q, np.uint8(2)) ^ rows[k]
    return q


def mul2_packed(x):
    """2*x on four packed field elements per uint32 -- the kernel's formula."""
    x = np.asarray(x, dtype=np.uint32)
    m = x & np.uint32(0x80808080)
    return (((x << np.uint32(1)) & np.uint32(0xFEFEFEFE)) ^
            (((m << np.uint32(1)) - (m >> np.uint32(7))) & np.uint32(0x1D1D1D1D))).astype(np.uint32)


def recover_two(survivors, p, q, x, y, out_len):
    """D_x, D_y of a stripe whose members x < y are lost (survivors: the stripe's
    chunks with None at x and y), from P and Q."""
    ps = p ^ p_of(survivors, out_len)
    qs = q ^ q_sum(survivors, out_len)
    gyx = gpow(y - x)
    d = gyx ^ 1
    a, b = div(gyx, d), div(gpow(-x), d)
    dx = mul(ps, np.uint8(a)) ^ mul(qs, np.uint8(b))
    return dx, ps ^ dx


def recover_one_from_q(survivors, q, x, out_len):
    """D_x when member x and P are lost: g^(-x) * Qs."""
    qs = q ^ q_sum(survivors, out_len)
    return mul(qs, np.uint8(gpow(-x)))


def q_target(locations: int, ntargets: int) -> int:
    """Restatement of bcp_q_target."""
    p = locations >> 56
    if not 1 <= ntargets <= 56 or p == 0xFF or p >= ntargets or (locations >> p) & 1:
        return -1
    for i in range(1, ntargets):
        t = (p + i) % ntargets
        if not (locations >> t) & 1:
            return t
    return -1
