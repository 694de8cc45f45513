// bcp_pq.hip -- P + Q parity over GF(2^8) for gfx950.
//
// Field: polynomial x^8+x^4+x^3+x^2+1 (0x11d), generator g = 2 (the RAID-6
// convention).  For a stripe of sources D_0 .. D_{n-1} in position order,
// each zero-padded to out_len:
//   P[j] = XOR_k D_k[j]            Q[j] = XOR_k g^k * D_k[j]
// Q is evaluated in Horner form, q = 0; for k = n-1 .. 0: q = 2*q ^ D_k, on
// four packed bytes of a dword at a time (mul2): no multiply, no table, no
// LDS.  One pass over the sources yields both.
//
// Five forms of that pass:
//   GEN    the epilogue stores Q, and P when the stripe has a P address;
//   SOLVE  the sources are the survivors (lost positions have len 0 and
//          contribute 2*q steps only), the P and Q bodies are loaded with the
//          first sources and XORed in, which makes the accumulators the
//          syndromes Ps and Qs; the epilogue stores D_x = ca*Ps ^ cb*Qs and
//          D_y = Ps ^ D_x, each truncated to its own length.  ca, cb are
//          per-stripe constants from the host (P lost: ca = 0, cb = g^-x).
//   CHECK  SOLVE's prologue and pass over a complete stripe (P body
//          required), so the accumulators are again Ps and Qs; nothing is
//          stored.  A clean tile ends on one ballot.  Otherwise the wave
//          locates every bad byte -- Ps only: P, Qs only: Q, both: the data
//          position k with g^k * Ps = Qs -- and commits first offset, counts
//          and member mask to the stripe's record (bcp_pq_check_result).
//   REPAIR CHECK's prologue, pass and clean path; the mismatch path also
//          corrects in place every bad byte whose member the stripe's mask
//          allows -- P ^= Ps, Q ^= Qs, D_k ^= Ps -- and counts the bytes it
//          fixed and the bytes it left (bcp_pq_repair_result).
//   VERIFY-REBUILD  SOLVE's prologue and pass with P present and exactly one
//          member x lost (the case SOLVE leaves to the XOR kernel): Ps is D_x
//          and is stored, cut to len_x; the residual Qs ^ g^x * Ps, zero where
//          the survivors, P and Q agree, is judged like CHECK's syndromes --
//          one ballot for a clean tile, else first offset and count to the
//          stripe's record (bcp_check_result).  Nothing is located or altered.
//
// All five also exist over window replay (pq_win_desc, pq_repair_win_desc,
// pq_rebuild_win_desc, the _win entry points): D_k is then the reference's replayed stream R_k of source
// k (bcp.h), which the kernel reads by remapping, per source and tile, the
// offset it loads from (pq_eff_off); outputs and bodies are addressed as before.
// A replayed byte is not tile-local, so windowed REPAIR writes a data byte only
// from its home tile (where its source is not replayed) and the host launches
// the tiles in phases, a source's echo tiles after its home tiles
// (bcp_pq_repair_win_phases); a located byte of a replayed source is left.
//
// Schedule and load shape are the descriptor fold's (bcp_kernels.hip): a
// device-wide atomicAdd-fed tile queue, wave-contiguous lanes, 16-byte
// non-temporal loads, every load of a group of four sources issued before its
// arithmetic.  Per tile and per source the coverage test is wave-uniform: a
// source covers the tile, misses it (a 2*q step without a load) or ends inside
// it (per-lane tail loads).  The runs keep the caller's order -- the position
// is the coefficient -- so the tile records are the host's (PqTile), not
// desc_tiles'.
#include "bcp_kernel_util.h"

namespace bcp {

// 2*x on four packed field elements.
__device__ __forceinline__ v4u mul2(v4u x) {
  const v4u m = x & 0x80808080u;
  return ((x << 1) & 0xfefefefeu) ^ (((m << 1) - (m >> 7)) & 0x1d1d1d1du);
}

// Window replay (the _win entry points): where source k's bytes for the tile at
// stripe offset `off` lie in the source.  Below lim = (lw_k + 1) * W the
// stream is the source itself (zero padded); from there on it replays the
// last readable window, base = lw_k * W, at the tile's offset in its own
// window, offw = off mod W.  Both records are the host's (PqWin, PqBatchWin);
// a source without replay has lim = UINT64_MAX.  Wave-uniform.
__device__ __forceinline__ uint64_t pq_eff_off(const_as<PqWin> *w, uint64_t off, uint64_t offw) {
  return off < w->lim ? off : w->base + offw;
}

// G consecutive sources run[0 .. G) of a stripe, folded highest position
// first: q = 2*q ^ D, p ^= D.  Every load of the group goes out before the
// arithmetic.
//
// WIN: source i is read at its effective offset eo(i) (pq_eff_off), the place
// the window replay takes this tile's bytes from; everything below that is
// `off` in the plain form -- covering test, loads, tail, miss -- is eo(i).
template <int G, int U, bool WIN>
__device__ __forceinline__ void pq_group(v4u (&p)[U], v4u (&q)[U], const_as<bcp_source> *run,
                                         const_as<PqWin> *wrun, uint64_t off, uint64_t offw, uint32_t T,
                                         uint32_t lane_off) {
  uint64_t ptr[G], len[G], weo[G];
  // (the plain form names `off` itself, so that its code is what it was before there was a windowed one)
  auto eo = [&](int i) -> uint64_t {
    if constexpr (WIN) return weo[i];
    else return off;
  };
  bool cover = true;
#pragma unroll
  for (int i = 0; i < G; i++) {
    ptr[i] = run[i].ptr;
    len[i] = run[i].len;
    if constexpr (WIN) weo[i] = pq_eff_off(wrun + i, off, offw);
    cover = cover && len[i] >= eo(i) + T;
  }
  v4u x[G][U];
  if (cover) {
#pragma unroll
    for (int i = 0; i < G; i++) {
      const glob<v4u_u> *s = gp<const v4u_u>(ptr[i] + eo(i) + lane_off);
#pragma unroll
      for (int u = 0; u < U; u++) x[i][u] = __builtin_nontemporal_load(s + u * 64);
    }
  } else {
#pragma unroll
    for (int i = 0; i < G; i++) {
      if (len[i] >= eo(i) + T) {
        const glob<v4u_u> *s = gp<const v4u_u>(ptr[i] + eo(i) + lane_off);
#pragma unroll
        for (int u = 0; u < U; u++) x[i][u] = __builtin_nontemporal_load(s + u * 64);
      } else if (len[i] <= eo(i)) {  // zero padding (also a (0, 0) source: never dereferenced)
#pragma unroll
        for (int u = 0; u < U; u++) x[i][u] = zero4();  // (never read: the 2*q step below)
      } else {
        gbyte *s = gp<const unsigned char>(ptr[i] + eo(i));
        const uint64_t left = len[i] - eo(i);  // < T: the source ends inside the tile
#pragma unroll
        for (int u = 0; u < U; u++) x[i][u] = load_src_tail(s, left, lane_off + u * 1024u);
      }
    }
    // a source that misses the tile is a 2*q step only (uniform branch)
#pragma unroll
    for (int i = G - 1; i >= 0; i--) {
      if (len[i] <= eo(i)) {
#pragma unroll
        for (int u = 0; u < U; u++) q[u] = mul2(q[u]);
      } else {
#pragma unroll
        for (int u = 0; u < U; u++) {
          q[u] = mul2(q[u]) ^ x[i][u];
          p[u] ^= x[i][u];
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = G - 1; i >= 0; i--)
#pragma unroll
    for (int u = 0; u < U; u++) {
      q[u] = mul2(q[u]) ^ x[i][u];
      p[u] ^= x[i][u];
    }
}

// r = c * x for a wave-uniform constant c: shift-and-add over the bits of c.
template <int U>
__device__ __forceinline__ void mulc_acc(v4u (&r)[U], const v4u (&x0)[U], uint32_t c) {
  v4u x[U];
#pragma unroll
  for (int u = 0; u < U; u++) x[u] = x0[u];
#pragma unroll
  for (int bit = 0; bit < 8; bit++) {
    if (c & (1u << bit)) {
#pragma unroll
      for (int u = 0; u < U; u++) r[u] ^= x[u];
    }
    if (bit < 7 && (c >> (bit + 1)) != 0) {
#pragma unroll
      for (int u = 0; u < U; u++) x[u] = mul2(x[u]);
    }
  }
}

// U vectors of this lane to d[0 .. left), tile-relative.
template <int U>
__device__ __forceinline__ void pq_store(uint64_t d, uint64_t left, uint32_t T, uint32_t lane_off, const v4u (&v)[U]) {
  if (left >= T) {
    glob<v4u_u> *o = gp<v4u_u>(d + lane_off);
#pragma unroll
    for (int u = 0; u < U; u++) __builtin_nontemporal_store(v[u], o + u * 64);
  } else {
    glob<unsigned char> *o = gp<unsigned char>(d);
#pragma unroll
    for (int u = 0; u < U; u++) store_tail(o, left, lane_off + u * 1024u, v[u]);
  }
}

// ---- CHECK form: what the syndromes say ---------------------------------
// Bit 7 of every non-zero byte of w.
__device__ __forceinline__ uint32_t nz_bytes(uint32_t w) {
  return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
}

// Bytes of the tile at or past `left` do not count (a source may be longer
// than out_len; the bodies' tail loads are zero there already).
template <int U>
__device__ __forceinline__ void pq_mask_tail(v4u (&v)[U], uint32_t left, uint32_t lane_off) {
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint32_t o = lane_off + (uint32_t)u * 1024u;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint32_t at = o + (uint32_t)c * 4u;
      const uint32_t n = left > at ? left - at : 0u;  // readable bytes of this dword
      v[u][c] &= n >= 4u ? 0xFFFFFFFFu : ((1u << (8u * n)) - 1u);
    }
  }
}

// Mismatch path, every lane of the wave: Ps and Qs of this lane's vectors
// (vector u at tile offset lane_off + u * 1024, tile at stripe offset off).
// k is searched with mul2 alone, t = g^k * Ps against Qs on the bytes where
// both are non-zero; g has order 255 > nsrc, so a byte matches at most one k
// and the bytes that never matched are counted, not tracked.  One vector at a
// time, the loop over k rolled: this path is rare and must set neither the
// kernel's register budget nor its code size.
template <int U>
__device__ __forceinline__ void pq_check_commit(bcp_pq_check_result *rec, const v4u (&ps)[U], const v4u (&qs)[U],
                                                uint32_t nsrc, uint64_t off, uint32_t lane_off) {
  uint32_t first = 0xFFFFFFFFu, np = 0, nq = 0, nboth = 0, nfound = 0;
  unsigned long long members = 0;
#pragma unroll
  for (int u = 0; u < U; u++) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint32_t hp = nz_bytes(ps[u][c]), hq = nz_bytes(qs[u][c]);
      np += (uint32_t)__builtin_popcount(hp);
      nq += (uint32_t)__builtin_popcount(hq);
      nboth += (uint32_t)__builtin_popcount(hp & hq);
      if (hp & ~hq) members |= BCP_PQ_BAD_P;
      if (hq & ~hp) members |= BCP_PQ_BAD_Q;
      if (hp | hq) {
        const uint32_t o = lane_off + (uint32_t)u * 1024u + (uint32_t)c * 4u + ((uint32_t)__builtin_ctz(hp | hq) >> 3);
        first = o < first ? o : first;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    v4u t = ps[u], both;
#pragma unroll
    for (int c = 0; c < 4; c++) both[c] = nz_bytes(ps[u][c]) & nz_bytes(qs[u][c]);
#pragma unroll 1
    for (uint32_t k = 0; k < nsrc; k++) {
      uint32_t hit = 0;
#pragma unroll
      for (int c = 0; c < 4; c++) hit += (uint32_t)__builtin_popcount(both[c] & ~nz_bytes(t[c] ^ qs[u][c]));
      if (hit) members |= 1ull << k;
      nfound += hit;
      t = mul2(t);
    }
  }
  if (nfound < nboth) members |= BCP_PQ_BAD_NOWHERE;
  unsigned long long f = first == 0xFFFFFFFFu ? ~0ull : off + first, cp = np, cq = nq;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long fo = __shfl_xor(f, o, 64);
    f = fo < f ? fo : f;
    cp += __shfl_xor(cp, o, 64);
    cq += __shfl_xor(cq, o, 64);
    members |= __shfl_xor(members, o, 64);
  }
  if ((threadIdx.x & 63u) == 0 && members) {
    __hip_atomic_fetch_min((unsigned long long *)&rec->first_bad, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add((unsigned long long *)&rec->p_bad, cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add((unsigned long long *)&rec->q_bad, cq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_or((unsigned long long *)&rec->members, members, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- REPAIR form: the same verdict, and the bytes put right ---------------
// The bytes of dword `val` (Ps or Qs) flagged in m (bit 7 per byte) XORed into
// the n (<= 4) writable bytes at `at`.  A byte of a member belongs to the one
// lane of the one tile that loaded it, so a plain read-modify-write is safe at
// any alignment.  Returns the bytes written.
__device__ __forceinline__ uint32_t pq_fix_bytes(uint64_t at, uint32_t m, uint32_t val, uint32_t n) {
  uint32_t done = 0;
  while (m) {
    const uint32_t b = (uint32_t)__builtin_ctz(m) >> 3;
    m &= m - 1u;
    if (b < n) {
      glob<unsigned char> *o = gp<unsigned char>(at + b);
      *o = (unsigned char)(*o ^ (unsigned char)(val >> (8u * b)));
      done++;
    }
  }
  return done;
}

// Sibling of pq_check_commit: the record's first four fields are the state as
// found; `allow` (the stripe's mask, bit layout of members) decides which
// members are written.  pbody, qbody: the bodies at stripe offset 0.  A byte
// that names position k at or past len_k (zero padding cannot be wrong), a
// position the mask leaves out, or no position at all, is left.
// WIN: so is a position whose source is replayed at this tile (off >= lim_k,
// wrun beside run): that byte's home is a tile of an earlier launch.  Where the
// source is not replayed its effective offset is `off`, so the address and the
// len test are the plain form's.
template <int U, bool WIN>
__device__ __forceinline__ void pq_repair_commit(bcp_pq_repair_result *rec, const v4u (&ps)[U], const v4u (&qs)[U],
                                                 const_as<bcp_source> *run, const_as<PqWin> *wrun, uint32_t nsrc,
                                                 unsigned long long allow, uint64_t pbody, uint64_t qbody,
                                                 uint64_t off, uint32_t lane_off) {
  uint32_t first = 0xFFFFFFFFu, np = 0, nq = 0, nboth = 0, nfound = 0, nfixed = 0, nleft = 0;
  unsigned long long members = 0;
#pragma unroll
  for (int u = 0; u < U; u++) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint32_t hp = nz_bytes(ps[u][c]), hq = nz_bytes(qs[u][c]);
      const uint64_t j = off + lane_off + (uint32_t)u * 1024u + (uint32_t)c * 4u;  // the dword's stripe offset
      np += (uint32_t)__builtin_popcount(hp);
      nq += (uint32_t)__builtin_popcount(hq);
      nboth += (uint32_t)__builtin_popcount(hp & hq);
      if (hp & ~hq) {  // (the tail is masked: every flagged byte lies below out_len)
        members |= BCP_PQ_BAD_P;
        if (allow & BCP_PQ_BAD_P) nfixed += pq_fix_bytes(pbody + j, hp & ~hq, ps[u][c], 4u);
        else nleft += (uint32_t)__builtin_popcount(hp & ~hq);
      }
      if (hq & ~hp) {
        members |= BCP_PQ_BAD_Q;
        if (allow & BCP_PQ_BAD_Q) nfixed += pq_fix_bytes(qbody + j, hq & ~hp, qs[u][c], 4u);
        else nleft += (uint32_t)__builtin_popcount(hq & ~hp);
      }
      if (hp | hq) {
        const uint32_t o = lane_off + (uint32_t)u * 1024u + (uint32_t)c * 4u + ((uint32_t)__builtin_ctz(hp | hq) >> 3);
        first = o < first ? o : first;
      }
    }
  }
  uint32_t nfixed_d = 0;
#pragma unroll
  for (int u = 0; u < U; u++) {
    v4u t = ps[u], both;
#pragma unroll
    for (int c = 0; c < 4; c++) both[c] = nz_bytes(ps[u][c]) & nz_bytes(qs[u][c]);
#pragma unroll 1
    for (uint32_t k = 0; k < nsrc; k++) {
      uint32_t hit = 0;
      bool may = (allow >> k) & 1ull;
      if constexpr (WIN) may = may && off < wrun[k].lim;
      const uint64_t ptr = run[k].ptr, len = run[k].len;  // uniform; a (0, 0) source has no byte below len
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const uint32_t h = both[c] & ~nz_bytes(t[c] ^ qs[u][c]);
        hit += (uint32_t)__builtin_popcount(h);
        const uint64_t j = off + lane_off + (uint32_t)u * 1024u + (uint32_t)c * 4u;
        if (h && may && len > j)
          nfixed_d += pq_fix_bytes(ptr + j, h, ps[u][c], len - j >= 4u ? 4u : (uint32_t)(len - j));
      }
      if (hit) members |= 1ull << k;
      nfound += hit;
      t = mul2(t);
    }
  }
  if (nfound < nboth) members |= BCP_PQ_BAD_NOWHERE;
  nleft += nboth - nfixed_d;
  nfixed += nfixed_d;
  unsigned long long f = first == 0xFFFFFFFFu ? ~0ull : off + first, cp = np, cq = nq, cf = nfixed, cl = nleft;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long fo = __shfl_xor(f, o, 64);
    f = fo < f ? fo : f;
    cp += __shfl_xor(cp, o, 64);
    cq += __shfl_xor(cq, o, 64);
    cf += __shfl_xor(cf, o, 64);
    cl += __shfl_xor(cl, o, 64);
    members |= __shfl_xor(members, o, 64);
  }
  if ((threadIdx.x & 63u) == 0 && members) {
    __hip_atomic_fetch_min((unsigned long long *)&rec->first_bad, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add((unsigned long long *)&rec->p_bad, cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add((unsigned long long *)&rec->q_bad, cq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_or((unsigned long long *)&rec->members, members, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add((unsigned long long *)&rec->fixed, cf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add((unsigned long long *)&rec->left, cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- VERIFY-REBUILD form: where Q does not agree with the rebuilt member ----
// Mismatch path, every lane of the wave: r = Qs ^ g^x * Ps of this lane's
// vectors, already cut to len_x.  The smallest bad offset and the number of bad
// bytes, reduced over the wave, one fetch_min and one fetch_add on the record.
template <int U>
__device__ __forceinline__ void pq_rebuild_commit(bcp_check_result *rec, const v4u (&r)[U], uint64_t off,
                                                  uint32_t lane_off) {
  uint32_t first = 0xFFFFFFFFu, nbad = 0;
#pragma unroll
  for (int u = 0; u < U; u++) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint32_t h = nz_bytes(r[u][c]);
      nbad += (uint32_t)__builtin_popcount(h);
      if (h) {
        const uint32_t o = lane_off + (uint32_t)u * 1024u + (uint32_t)c * 4u + ((uint32_t)__builtin_ctz(h) >> 3);
        first = o < first ? o : first;
      }
    }
  }
  unsigned long long f = first == 0xFFFFFFFFu ? ~0ull : off + first, cnt = nbad;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long fo = __shfl_xor(f, o, 64);
    f = fo < f ? fo : f;
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((threadIdx.x & 63u) == 0 && cnt) {
    __hip_atomic_fetch_min((unsigned long long *)&rec->first_bad, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add((unsigned long long *)&rec->bad_bytes, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

enum PqForm { kPqGen = 0, kPqSolve = 1, kPqCheck = 2, kPqRepair = 3, kPqRebuild = 4 };

// WIN: the windowed instantiations (PqBatchWin's two more tables, w); a stripe
// without a window in such a batch has lim = UINT64_MAX on every source and
// so keeps the plain semantics.  The bodies and the outputs are addressed
// with plain `off` in both.
// R: the form's record, bcp_pq_repair_result for REPAIR.
template <int U, PqForm F, bool WIN, class R>
__device__ __forceinline__ void pq_tile(const PqBatch &b, const PqWinTab &w, uint32_t t, R *res) {
  constexpr bool SOLVE = F == kPqSolve;
  constexpr uint32_t T = (uint32_t)kBlock * U * 16u;
  const_as<PqTile> *tr = cst(b.tiles) + t;
  const_as<PqStripe> *d = cst(b.stripes) + tr->stripe;
  const uint64_t off = (uint64_t)tr->sub * T;
  const_as<bcp_source> *run = cst(b.sources) + d->first_src;
  const_as<PqWin> *wrun = nullptr;  // per source, beside run
  uint64_t offw = 0;                // off mod W of a windowed stripe
  if constexpr (WIN) {
    wrun = cst(w.win) + d->first_src;
    offw = cst(w.offw)[t];
  }
  // this lane's vector u = 0 inside the tile; vector u is at + u * 1024
  const uint32_t lane_off = ((threadIdx.x >> 6) * (64u * U) + (threadIdx.x & 63u)) * 16u;
  const uint64_t out_left = d->out_len - off;  // > 0: the host cuts tiles below out_len only
  v4u p[U], q[U], qb[U];
#pragma unroll
  for (int u = 0; u < U; u++) p[u] = q[u] = qb[u] = zero4();
  if constexpr (F != kPqGen) {
    // the P and Q bodies: p starts as P, the Q body joins after the Horner pass
    const uint64_t pp = d->p;
    if (out_left >= T) {
      const glob<v4u_u> *s = gp<const v4u_u>(d->q + off + lane_off);
#pragma unroll
      for (int u = 0; u < U; u++) qb[u] = __builtin_nontemporal_load(s + u * 64);
      if (pp) {
        const glob<v4u_u> *s2 = gp<const v4u_u>(pp + off + lane_off);
#pragma unroll
        for (int u = 0; u < U; u++) p[u] = __builtin_nontemporal_load(s2 + u * 64);
      }
    } else {
      gbyte *s = gp<const unsigned char>(d->q + off);
#pragma unroll
      for (int u = 0; u < U; u++) qb[u] = load_src_tail(s, out_left, lane_off + u * 1024u);
      if (pp) {
        gbyte *s2 = gp<const unsigned char>(pp + off);
#pragma unroll
        for (int u = 0; u < U; u++) p[u] = load_src_tail(s2, out_left, lane_off + u * 1024u);
      }
    }
  }
  uint32_t k = d->nsrc;
  // the highest positions that miss the tile: q is still zero there, nothing to do
  if constexpr (WIN) {
    while (k > 0 && run[k - 1].len <= pq_eff_off(wrun + (k - 1), off, offw)) k--;
  } else {
    while (k > 0 && run[k - 1].len <= off) k--;
  }
  while (k >= 4) {
    k -= 4;
    pq_group<4, U, WIN>(p, q, run + k, wrun + k, off, offw, T, lane_off);
  }
  switch (k) {
    case 3: pq_group<3, U, WIN>(p, q, run, wrun, off, offw, T, lane_off); break;
    case 2: pq_group<2, U, WIN>(p, q, run, wrun, off, offw, T, lane_off); break;
    case 1: pq_group<1, U, WIN>(p, q, run, wrun, off, offw, T, lane_off); break;
    default: break;
  }
  if constexpr (F == kPqCheck || F == kPqRepair) {
#pragma unroll
    for (int u = 0; u < U; u++) q[u] ^= qb[u];  // p = Ps, q = Qs
    if (out_left < T) {  // the stripe's last tile (uniform)
      pq_mask_tail<U>(p, (uint32_t)out_left, lane_off);
      pq_mask_tail<U>(q, (uint32_t)out_left, lane_off);
    }
    v4u any = p[0] | q[0];
#pragma unroll
    for (int u = 1; u < U; u++) any |= p[u] | q[u];
    if (__ballot((any[0] | any[1] | any[2] | any[3]) != 0u) == 0) return;  // clean: no store, no atomic
    if constexpr (F == kPqRepair)
      pq_repair_commit<U, WIN>(res + tr->stripe, p, q, run, wrun, d->nsrc, d->allow, d->p, d->q, off, lane_off);
    else pq_check_commit<U>(res + tr->stripe, p, q, d->nsrc, off, lane_off);
  } else if constexpr (F == kPqRebuild) {
#pragma unroll
    for (int u = 0; u < U; u++) q[u] ^= qb[u];  // p = Ps = D_x, q = Qs
    const uint64_t left = d->len_x - off;       // > 0: the tiles cover [0, len_x) only
    mulc_acc<U>(q, p, d->ca);                   // q = r = Qs ^ g^x * Ps
    pq_store<U>(d->dx + off, left, T, lane_off, p);
    if (left < T) pq_mask_tail<U>(q, (uint32_t)left, lane_off);  // the stripe's last covered tile (uniform)
    v4u any = q[0];
#pragma unroll
    for (int u = 1; u < U; u++) any |= q[u];
    if (__ballot((any[0] | any[1] | any[2] | any[3]) != 0u) == 0) return;  // clean: no further store, no atomic
    pq_rebuild_commit<U>(res + tr->stripe, q, off, lane_off);
  } else if constexpr (SOLVE) {
#pragma unroll
    for (int u = 0; u < U; u++) q[u] ^= qb[u];  // p = Ps, q = Qs
    v4u dx[U];
#pragma unroll
    for (int u = 0; u < U; u++) dx[u] = zero4();
    mulc_acc<U>(dx, p, d->ca);
    mulc_acc<U>(dx, q, d->cb);
    const uint64_t len_x = d->len_x, len_y = d->len_y;
    if (len_x > off) pq_store<U>(d->dx + off, len_x - off, T, lane_off, dx);
    if (len_y > off) {
#pragma unroll
      for (int u = 0; u < U; u++) dx[u] ^= p[u];
      pq_store<U>(d->dy + off, len_y - off, T, lane_off, dx);
    }
  } else {
    pq_store<U>(d->q + off, out_left, T, lane_off, q);
    const uint64_t pp = d->p;
    if (pp) pq_store<U>(pp + off, out_left, T, lane_off, p);
  }
}

template <int U, PqForm F, bool WIN = false, class R>
__device__ __forceinline__ void pq_body(const PqBatch &b, R *res, const PqWinTab &w = PqWinTab{}) {
  // Work queue, one tile per grab (two LDS slots as in stream_body).
  __shared__ uint32_t next[2];
  if (threadIdx.x == 0) next[0] = queue_grab(b.ctr, b.base);
  __syncthreads();
  uint32_t t = __builtin_amdgcn_readfirstlane(next[0]);
  int slot = 0;
  while (t < b.ntiles) {
    pq_tile<U, F, WIN, R>(b, w, t, res);
    slot ^= 1;
    if (threadIdx.x == 0) next[slot] = queue_grab(b.ctr, b.base);
    __syncthreads();
    t = __builtin_amdgcn_readfirstlane(next[slot]);
  }
}

template <int U, bool SOLVE>
__global__ __launch_bounds__(kBlock) void pq_desc(PqBatch b) {
  pq_body<U, SOLVE ? kPqSolve : kPqGen>(b, (bcp_pq_check_result *)nullptr);
}

// The CHECK form (bcp_pq_check_stripes_async): same tiles, same queue, one
// record per stripe in res (initialised by pq_check_init before the launch).
template <int U>
__global__ __launch_bounds__(kBlock) void pq_check_desc(PqBatch b, bcp_pq_check_result *res) {
  pq_body<U, kPqCheck>(b, res);
}

// The REPAIR form (bcp_pq_repair_stripes_async): CHECK's batch, the stripes'
// masks in their records, one bcp_pq_repair_result per stripe (pq_repair_init).
template <int U>
__global__ __launch_bounds__(kBlock) void pq_repair_desc(PqBatch b, bcp_pq_repair_result *res) {
  pq_body<U, kPqRepair>(b, res);
}

// The windowed forms of all three (the _win entry points): one kernel per
// tile size and form, the form a template argument as above.
template <int U, int F>
__global__ __launch_bounds__(kBlock) void pq_win_desc(PqBatchWin b, bcp_pq_check_result *res) {
  pq_body<U, (PqForm)F, true>(b.b, res, b.w);
}

// Windowed REPAIR (bcp_pq_repair_stripes_win_async): one launch per phase over
// that phase's part of the tile and offw tables, in stream order.
template <int U>
__global__ __launch_bounds__(kBlock) void pq_repair_win_desc(PqBatchWin b, bcp_pq_repair_result *res) {
  pq_body<U, kPqRepair, true>(b.b, res, b.w);
}

// The VERIFY-REBUILD form (bcp_pq_rebuild_check_stripes_async and its _win
// namesake): SOLVE's batch with P present, one bcp_check_result per stripe
// (initialised by check_init before the launch).  Nothing is written in place,
// so the windowed one needs no phases.
template <int U>
__global__ __launch_bounds__(kBlock) void pq_rebuild_desc(PqBatch b, bcp_check_result *res) {
  pq_body<U, kPqRebuild>(b, res);
}

template <int U>
__global__ __launch_bounds__(kBlock) void pq_rebuild_win_desc(PqBatchWin b, bcp_check_result *res) {
  pq_body<U, kPqRebuild, true>(b.b, res, b.w);
}

__global__ __launch_bounds__(kBlock) void pq_check_init(bcp_pq_check_result *res, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) res[i] = bcp_pq_check_result{~0ull, 0ull, 0ull, 0ull};
}

__global__ __launch_bounds__(kBlock) void pq_repair_init(bcp_pq_repair_result *res, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) res[i] = bcp_pq_repair_result{~0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
}

hipError_t launch_pq(hipStream_t st, int grid, int vecs, bool solve, const PqBatch &b) {
  if (grid <= 0 || !pq_vecs_ok(vecs)) return hipErrorInvalidValue;
  if (vecs == 8) {
    if (solve) hipLaunchKernelGGL((pq_desc<8, true>), dim3(grid), dim3(kBlock), 0, st, b);
    else hipLaunchKernelGGL((pq_desc<8, false>), dim3(grid), dim3(kBlock), 0, st, b);
  } else {
    if (solve) hipLaunchKernelGGL((pq_desc<4, true>), dim3(grid), dim3(kBlock), 0, st, b);
    else hipLaunchKernelGGL((pq_desc<4, false>), dim3(grid), dim3(kBlock), 0, st, b);
  }
  return hipGetLastError();
}

hipError_t launch_pq_win(hipStream_t st, int grid, int vecs, int form, const PqBatchWin &b, bcp_pq_check_result *res) {
  if (grid <= 0 || !pq_vecs_ok(vecs) || form < 0 || form > 2 || (form == kPqCheck) != (res != nullptr))
    return hipErrorInvalidValue;
  const dim3 g(grid), bl(kBlock);
  if (vecs == 8) {
    if (form == kPqGen) hipLaunchKernelGGL((pq_win_desc<8, kPqGen>), g, bl, 0, st, b, res);
    else if (form == kPqSolve) hipLaunchKernelGGL((pq_win_desc<8, kPqSolve>), g, bl, 0, st, b, res);
    else hipLaunchKernelGGL((pq_win_desc<8, kPqCheck>), g, bl, 0, st, b, res);
  } else {
    if (form == kPqGen) hipLaunchKernelGGL((pq_win_desc<4, kPqGen>), g, bl, 0, st, b, res);
    else if (form == kPqSolve) hipLaunchKernelGGL((pq_win_desc<4, kPqSolve>), g, bl, 0, st, b, res);
    else hipLaunchKernelGGL((pq_win_desc<4, kPqCheck>), g, bl, 0, st, b, res);
  }
  return hipGetLastError();
}

hipError_t launch_pq_check_init(hipStream_t st, bcp_pq_check_result *res, uint32_t n) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(pq_check_init, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, res, n);
  return hipGetLastError();
}

hipError_t launch_pq_check(hipStream_t st, int grid, int vecs, const PqBatch &b, bcp_pq_check_result *res) {
  if (grid <= 0 || !pq_vecs_ok(vecs) || !res) return hipErrorInvalidValue;
  if (vecs == 8) hipLaunchKernelGGL((pq_check_desc<8>), dim3(grid), dim3(kBlock), 0, st, b, res);
  else hipLaunchKernelGGL((pq_check_desc<4>), dim3(grid), dim3(kBlock), 0, st, b, res);
  return hipGetLastError();
}

hipError_t launch_pq_repair_init(hipStream_t st, bcp_pq_repair_result *res, uint32_t n) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(pq_repair_init, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, res, n);
  return hipGetLastError();
}

hipError_t launch_pq_repair(hipStream_t st, int grid, int vecs, const PqBatch &b, bcp_pq_repair_result *res) {
  if (grid <= 0 || !pq_vecs_ok(vecs) || !res) return hipErrorInvalidValue;
  if (vecs == 8) hipLaunchKernelGGL((pq_repair_desc<8>), dim3(grid), dim3(kBlock), 0, st, b, res);
  else hipLaunchKernelGGL((pq_repair_desc<4>), dim3(grid), dim3(kBlock), 0, st, b, res);
  return hipGetLastError();
}

hipError_t launch_pq_repair_win(hipStream_t st, int grid, int vecs, const PqBatchWin &b, bcp_pq_repair_result *res) {
  if (grid <= 0 || !pq_vecs_ok(vecs) || !res) return hipErrorInvalidValue;
  if (vecs == 8) hipLaunchKernelGGL((pq_repair_win_desc<8>), dim3(grid), dim3(kBlock), 0, st, b, res);
  else hipLaunchKernelGGL((pq_repair_win_desc<4>), dim3(grid), dim3(kBlock), 0, st, b, res);
  return hipGetLastError();
}

hipError_t launch_pq_rebuild(hipStream_t st, int grid, int vecs, const PqBatch &b, bcp_check_result *res) {
  if (grid <= 0 || !pq_vecs_ok(vecs) || !res) return hipErrorInvalidValue;
  if (vecs == 8) hipLaunchKernelGGL((pq_rebuild_desc<8>), dim3(grid), dim3(kBlock), 0, st, b, res);
  else hipLaunchKernelGGL((pq_rebuild_desc<4>), dim3(grid), dim3(kBlock), 0, st, b, res);
  return hipGetLastError();
}

hipError_t launch_pq_rebuild_win(hipStream_t st, int grid, int vecs, const PqBatchWin &b, bcp_check_result *res) {
  if (grid <= 0 || !pq_vecs_ok(vecs) || !res) return hipErrorInvalidValue;
  if (vecs == 8) hipLaunchKernelGGL((pq_rebuild_win_desc<8>), dim3(grid), dim3(kBlock), 0, st, b, res);
  else hipLaunchKernelGGL((pq_rebuild_win_desc<4>), dim3(grid), dim3(kBlock), 0, st, b, res);
  return hipGetLastError();
}

}  // namespace bcp
