// bcp_kernel_util.h -- device helpers shared by the kernel files
// (bcp_kernels.hip, bcp_pq.hip): vector types, address-space casts, the
// byte-exact tail loads and stores, and the work queue's grab.
#pragma once

#include "bcp_internal.h"

namespace bcp {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef v4u v4u_u __attribute__((aligned(1)));  // unaligned 16-byte view

template <typename T>
__device__ __forceinline__ v4u ld_nt(const T *p) { return __builtin_nontemporal_load(p); }

// Descriptor tables (stripes, sources, tile prefixes) are never written while
// a kernel runs.  Reading them through the constant address space lets the
// compiler use scalar loads (s_load, own lgkm counter) for the uniform
// indices; through a generic pointer they become vector loads whose
// s_waitcnt vmcnt(0) drains the data loads in flight on every tile.
template <typename T>
using const_as = const __attribute__((address_space(4))) T;
template <typename T>
__device__ __forceinline__ const_as<T> *cst(const T *p) {
  return (const_as<T> *)(uintptr_t)p;
}

// Data pointers taken from descriptor tables are plain integers; without an
// address space the compiler emits flat loads, which also count on lgkmcnt,
// so every scalar-load wait would drain the whole data stream.  Cast them to
// the global address space.
template <typename T>
using glob = __attribute__((address_space(1))) T;
template <typename T>
__device__ __forceinline__ glob<T> *gp(uint64_t p) {
  return (glob<T> *)(uintptr_t)p;
}
__device__ __forceinline__ v4u zero4() { return v4u{0u, 0u, 0u, 0u}; }

// 16 bytes of source `p` (readable length len) at offset off, zero past len.
typedef glob<const unsigned char> gbyte;
__device__ __forceinline__ v4u ld16(gbyte *p) { return __builtin_nontemporal_load((const glob<v4u_u> *)p); }

// The one vector of a source that straddles its end: n (1..15) readable bytes
// at p, zeros after.  Static byte indices keep w[] in registers.
__device__ __forceinline__ v4u load_straddle(gbyte *p, uint32_t n) {
  unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t i = 0; i < 16; i++)
    if (i < n) w[i >> 2] |= (unsigned int)p[i] << (8 * (i & 3));
  return v4u{w[0], w[1], w[2], w[3]};
}

__device__ __forceinline__ uint32_t queue_grab(unsigned long long *ctr, unsigned long long base) {
  const unsigned long long v = atomicAdd(ctr, 1ull) - base;
  return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
}

__device__ __forceinline__ v4u load_src_tail(gbyte *p, uint64_t len, uint64_t off) {
  if (off + 16 <= len) return ld16(p + off);
  if (off >= len) return zero4();
  return load_straddle(p + off, (uint32_t)(len - off));
}

__device__ __forceinline__ void store_tail(glob<unsigned char> *d, uint64_t out_len, uint64_t off, v4u v) {
  if (off + 16 <= out_len) {
    __builtin_nontemporal_store(v, (glob<v4u_u> *)(d + off));
    return;
  }
  if (off >= out_len) return;
  const uint32_t n = (uint32_t)(out_len - off);
#pragma unroll
  for (uint32_t i = 0; i < 16; i++)
    if (i < n) d[off + i] = (unsigned char)(v[i >> 2] >> (8 * (i & 3)));
}

}  // namespace bcp
