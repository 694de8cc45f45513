// hipdouble.cpp -- a CPU stand-in for the device: the HIP runtime functions
// and the bcp::launch_* wrappers that the host-only object of bcp_engine.hip
// leaves undefined.  Test code (tools/hipdouble_pipeline.sh,
// tests/test_hipdouble_cpu.py): with it the engine's and the pipeline's host
// code runs unchanged on a machine without a GPU, under AddressSanitizer and
// ThreadSanitizer, against a "device" that checks every address it is handed
// and chooses the schedule.  Nothing here calls the real runtime.
//
//  memory    every allocation is host memory in a registry (base, size, kind,
//            owning device); a free first drains every stream, as the real
//            runtime does, then poisons and releases; an operation still
//            pending at the free that refers to the range is a finding
//  devices   two; hipSetDevice is per thread; a launch that touches a device
//            allocation (or memory registered without the portable flag) of
//            the other device is a finding, as are a launch on a stream that
//            is not of the thread's current device and an event recorded on a
//            stream of another device than the one it was created on -- how a
//            stream, event or allocation made under the wrong current device
//            shows
//  streams   one thread each, in order; events with HIP's semantics (never
//            recorded = complete); a copy from pinned memory reads its source
//            when it executes; schedules eager / lazy / seed=N (hipdouble.h)
//  launches  validated when enqueued (the arguments, and the tables: in place
//            where they lie in pinned memory, else from the pinned source of
//            their pending upload) and again when executed,
//            from the structures of bcp_internal.h as the device reads them;
//            *ctr == base is asserted and the counter advanced by the tiles
//            taken plus the grid; the result is computed byte by byte from the
//            staged tables (no sub_class, no count_tiles, no tile cutting)
// A finding is one line on stderr and one count (hipdouble_findings); nothing
// here aborts.
#include <hip/hip_runtime_api.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "bcp_internal.h"
#include "hipdouble.h"

using namespace bcp;
using Clock = std::chrono::steady_clock;

namespace {

// ---------------------------------------------------------------------------
// findings
// ---------------------------------------------------------------------------
std::atomic<long> g_findings{0};
std::atomic<long> g_ops{0};

void finding_v(std::set<std::string> *seen, const char *fmt, va_list ap) {
  char line[512];
  vsnprintf(line, sizeof line, fmt, ap);
  if (seen) {
    static std::mutex mu;  // an operation's enqueue and execution may run on two threads
    std::lock_guard<std::mutex> lk(mu);
    if (!seen->insert(line).second) return;  // the same finding of the same operation, seen at enqueue already
  }
  g_findings.fetch_add(1);
  fprintf(stderr, "hipdouble: FINDING %s\n", line);
}
void finding(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void finding(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  finding_v(nullptr, fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------------------
// schedule
// ---------------------------------------------------------------------------
enum Sched { kEager, kLazy, kSeed };
Sched g_sched = kEager;
uint64_t g_seed = 0;
std::chrono::microseconds g_lazy_timer(1500);  // HIPDOUBLE_LAZY_US: another one (the self-test's long one)
long g_launch_us = 0;   // HIPDOUBLE_LAUNCH_US: every launch stays on its stream at least this long
int g_devices = 2;      // HIPDOUBLE_DEVICES=1: one device, a pipeline's lanes wrap onto it as on a one-GPU machine
bool g_trace = false;  // HIPDOUBLE_TRACE: one line per allocation and free
std::once_flag g_sched_once;
void read_schedule() {
  std::call_once(g_sched_once, [] {
    g_trace = getenv("HIPDOUBLE_TRACE") != nullptr;
    if (const char *t = getenv("HIPDOUBLE_DEVICES")) g_devices = atoi(t) == 1 ? 1 : 2;
    if (const char *t = getenv("HIPDOUBLE_LAUNCH_US")) g_launch_us = atol(t);
    if (const char *t = getenv("HIPDOUBLE_LAZY_US")) g_lazy_timer = std::chrono::microseconds(atol(t));
    const char *v = getenv("HIPDOUBLE_SCHEDULE");
    if (!v || !strcmp(v, "eager")) return;
    if (!strcmp(v, "lazy")) {
      g_sched = kLazy;
    } else if (!strncmp(v, "seed=", 5)) {
      g_sched = kSeed;
      g_seed = strtoull(v + 5, nullptr, 10);
    } else {
      fprintf(stderr, "hipdouble: unknown HIPDOUBLE_SCHEDULE '%s', running eager\n", v);
    }
  });
}
uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// ---------------------------------------------------------------------------
// memory
// ---------------------------------------------------------------------------
enum Kind { kDevice, kPinned, kRegistered };
const char *const kKindName[] = {"device", "pinned host", "registered host"};
struct Alloc {
  uintptr_t base;
  size_t size;
  Kind kind;
  int dev;        // owning device; -1: every device reaches it (portable)
  bool owned;     // allocated here (freed here)
};
// Shared: lookups, and an operation for as long as it executes.  Exclusive:
// whoever adds or removes an allocation.
std::shared_mutex g_mem;
std::map<uintptr_t, Alloc> g_allocs;
thread_local int t_dev = 0;
thread_local hipError_t t_last = hipSuccess;

const Alloc *find_alloc(const void *p) {  // with g_mem held
  const uintptr_t a = (uintptr_t)p;
  auto it = g_allocs.upper_bound(a);
  if (it == g_allocs.begin()) return nullptr;
  --it;
  return a < it->second.base + it->second.size ? &it->second : nullptr;
}

struct Range {
  uintptr_t lo, hi;
};

// What one operation is checked in: its name, its stream's device, where its
// ranges are collected (enqueue) and which findings it has made already.
struct Ctx {
  const char *op;
  int dev;
  std::vector<Range> *ranges;
  std::set<std::string> *seen;
  std::pair<bool, uint64_t> *tables = nullptr;  // hash of the tables as read at enqueue (pinned ones), if they were
  bool ok = true;
  // Tables read in place must not change between the launch call and the launch.
  void same_tables(uint64_t h, bool exec) {
    if (!tables) return;
    if (!exec) {
      *tables = {true, h};
    } else if (tables->first && tables->second != h) {
      fail("%s: the tables it reads in place were rewritten between the launch call and its execution", op);
    }
  }
  void fail(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
    va_list ap;
    va_start(ap, fmt);
    finding_v(seen, fmt, ap);
    va_end(ap);
    ok = false;
  }
  // [p, p + n) lies in one live allocation that this device may reach.
  bool need(const void *p, uint64_t n, const char *what, long stripe = -1) {
    if (!n) return true;
    const Alloc *a = p ? find_alloc(p) : nullptr;
    if (!a) {
      fail("%s: stripe %ld: %s [%p, +%llu) lies in no live allocation", op, stripe, what, p, (unsigned long long)n);
      return false;
    }
    const uintptr_t end = (uintptr_t)p + n;
    if (end > a->base + a->size || end < (uintptr_t)p) {
      fail("%s: stripe %ld: %s [%p, +%llu) runs %llu bytes past its %s allocation [%p, +%zu)", op, stripe, what, p,
           (unsigned long long)n, (unsigned long long)(end - (a->base + a->size)), kKindName[a->kind], (void *)a->base,
           a->size);
      return false;
    }
    if (a->dev >= 0 && a->dev != dev && a->kind != kPinned) {
      fail("%s: stripe %ld: %s [%p, +%llu) belongs to device %d, the stream to device %d", op, stripe, what, p,
           (unsigned long long)n, a->dev, dev);
      return false;
    }
    if (ranges) ranges->push_back(Range{(uintptr_t)p, end});
    return true;
  }
};

bool host_resident(const void *p) {  // with g_mem held
  const Alloc *a = find_alloc(p);
  return a && a->kind != kDevice;
}

// The latest upload (one-row copy from pinned memory) into each device range.
// A launch whose tables are uploaded is enqueued while that copy may still be
// pending; its tables are then read, at the launch call, from the copy's pinned
// source, which the host filled on this same thread -- so a pending launch
// knows the slab ranges it will touch whether its tables travel or not.
struct Upload {
  uintptr_t hi, src;
};
std::mutex g_up_mu;
std::map<uintptr_t, Upload> g_uploads;  // by the destination's first byte
void forget_uploads(uintptr_t lo, uintptr_t hi, bool also_sources) {
  std::lock_guard<std::mutex> lk(g_up_mu);
  for (auto it = g_uploads.begin(); it != g_uploads.end();) {
    const uintptr_t n = it->second.hi - it->first;
    const bool hit = (it->first < hi && lo < it->second.hi) ||
                     (also_sources && it->second.src < hi && lo < it->second.src + n);
    it = hit ? g_uploads.erase(it) : std::next(it);
  }
}
template <typename T>
const T *staged(const T *p) {
  std::lock_guard<std::mutex> lk(g_up_mu);
  const uintptr_t a = (uintptr_t)p;
  auto it = g_uploads.upper_bound(a);
  if (it == g_uploads.begin()) return p;
  --it;
  return a < it->second.hi ? (const T *)(it->second.src + (a - it->first)) : p;
}

// ---------------------------------------------------------------------------
// streams and events
// ---------------------------------------------------------------------------
struct Stream;
struct Marker {  // one hipEventRecord
  Stream *owner = nullptr;
  uint64_t seq = 0;
  std::atomic<bool> done{false};
  Clock::time_point when;
};
std::mutex g_mk_mu;
std::condition_variable g_mk_cv;

struct Op {
  const char *name;
  uint64_t seq;
  std::function<void()> fn;
  std::vector<Range> ranges;
  Clock::time_point t_enq;
  unsigned delay_us;
};

struct Stream {
  int dev = 0;
  bool dead = false;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Op> q;  // the front is the one running, if any does
  uint64_t enq = 0, done = 0, urgent_upto = 0;
  bool stop = false;
  std::thread th;

  void loop() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return stop || !q.empty(); });
      if (q.empty()) return;
      Op &op = q.front();  // (push_back leaves references into a deque valid)
      if (g_sched == kLazy) {
        cv.wait_until(lk, op.t_enq + g_lazy_timer, [&] { return urgent_upto >= op.seq || stop; });
      } else if (g_sched == kSeed && op.delay_us) {
        lk.unlock();
        std::this_thread::sleep_for(std::chrono::microseconds(op.delay_us));
        lk.lock();
      }
      lk.unlock();
      op.fn();
      g_ops.fetch_add(1);
      lk.lock();
      q.pop_front();
      done++;
      cv.notify_all();
    }
  }
  void push(const char *name, std::vector<Range> ranges, std::function<void()> fn, uint64_t *seq_out = nullptr) {
    std::lock_guard<std::mutex> lk(mu);
    const uint64_t seq = ++enq;
    unsigned delay = 0;
    if (g_sched == kSeed) {
      const uint64_t r = splitmix(g_seed * 0x10001ull + (uintptr_t)this + seq * 0x9E37ull);
      delay = r & 1 ? (unsigned)((r >> 8) % 400u) : 0;  // half of the operations wait up to 0.4 ms
    }
    q.push_back(Op{name, seq, std::move(fn), std::move(ranges), Clock::now(), delay});
    if (seq_out) *seq_out = seq;
    cv.notify_all();
  }
  void kick(uint64_t seq) {  // somebody blocks on everything up to seq
    std::lock_guard<std::mutex> lk(mu);
    if (urgent_upto < seq) urgent_upto = seq;
    cv.notify_all();
  }
  void sync() {
    std::unique_lock<std::mutex> lk(mu);
    const uint64_t target = enq;
    if (urgent_upto < target) urgent_upto = target;
    cv.notify_all();
    cv.wait(lk, [&] { return done >= target; });
  }
};

struct Event {
  int dev = 0;
  std::mutex mu;
  std::shared_ptr<Marker> last;
};

std::mutex g_streams_mu;
std::vector<Stream *> g_streams;  // never shrinks: a destroyed stream stays (dead), markers may still name it
std::set<Event *> g_events;

Stream *as_stream(hipStream_t s, const char *op) {
  Stream *p = reinterpret_cast<Stream *>(s);
  std::lock_guard<std::mutex> lk(g_streams_mu);
  for (Stream *x : g_streams)
    if (x == p && !x->dead) return p;
  finding("%s: stream %p is not a live stream", op, (void *)s);
  return nullptr;
}
Event *as_event(hipEvent_t e, const char *op) {
  Event *p = reinterpret_cast<Event *>(e);
  std::lock_guard<std::mutex> lk(g_streams_mu);
  if (g_events.count(p)) return p;
  finding("%s: event %p is not a live event", op, (void *)e);
  return nullptr;
}

void drain_all() {
  std::vector<Stream *> live;
  {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    for (Stream *s : g_streams)
      if (!s->dead) live.push_back(s);
  }
  for (Stream *s : live) s->sync();
}

// The project's rule: nothing is freed while in use.  An operation still queued
// (or running) that names the range when the free is called breaks it, even
// though the drain below then lets it finish first.
void check_pending(const char *op, uintptr_t lo, uintptr_t hi) {
  std::vector<Stream *> live;
  {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    for (Stream *s : g_streams)
      if (!s->dead) live.push_back(s);
  }
  for (Stream *s : live) {
    std::lock_guard<std::mutex> lk(s->mu);
    for (const Op &o : s->q)
      for (const Range &r : o.ranges)
        if (r.lo < hi && lo < r.hi) {
          finding("%s: [%p, +%zu) is freed while %s (operation %llu of a stream of device %d) still refers to [%p, +%zu)",
                  op, (void *)lo, (size_t)(hi - lo), o.name, (unsigned long long)o.seq, s->dev, (void *)r.lo,
                  (size_t)(r.hi - r.lo));
          return;  // one finding per free
        }
  }
}

hipError_t add_alloc(void **out, size_t size, Kind kind) {
  read_schedule();
  if (!out) return hipErrorInvalidValue;
  void *p = nullptr;
  const size_t n = (size + 4095) / 4096 * 4096;  // page-aligned, whole pages: O_DIRECT reads land here
  if (posix_memalign(&p, 4096, n ? n : 4096) != 0) return hipErrorOutOfMemory;
  memset(p, 0xCB, n ? n : 4096);  // fresh memory holds no zeros by luck
  std::unique_lock<std::shared_mutex> lk(g_mem);
  g_allocs[(uintptr_t)p] = Alloc{(uintptr_t)p, size ? size : 1, kind, t_dev, true};
  *out = p;
  if (g_trace) fprintf(stderr, "hipdouble: alloc %s %zu bytes on device %d: %p\n", kKindName[kind], size, t_dev, p);
  return hipSuccess;
}

hipError_t drop_alloc(void *p, const char *op, bool want_owned) {
  if (!p) return hipSuccess;
  Alloc a;
  {
    std::shared_lock<std::shared_mutex> lk(g_mem);
    auto it = g_allocs.find((uintptr_t)p);
    if (it == g_allocs.end() || it->second.owned != want_owned) {
      finding("%s: %p is not the base of a live allocation of that kind", op, p);
      return hipErrorInvalidValue;
    }
    a = it->second;
  }
  if (g_trace) fprintf(stderr, "hipdouble: %s %s %zu bytes: %p\n", op, kKindName[a.kind], a.size, p);
  check_pending(op, a.base, a.base + a.size);
  drain_all();
  forget_uploads(a.base, a.base + a.size, true);
  std::unique_lock<std::shared_mutex> lk(g_mem);
  g_allocs.erase(a.base);
  if (a.owned) {
    memset((void *)a.base, 0xDD, a.size);
    free((void *)a.base);
  }
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// GF(2^8): polynomial 0x11d, generator 2, tables built from the polynomial
// (tests/gf256.py states the same)
// ---------------------------------------------------------------------------
struct Gf {
  uint8_t exp[510];
  int log[256];
  Gf() {
    unsigned x = 1;
    for (int i = 0; i < 255; i++) {
      exp[i] = exp[i + 255] = (uint8_t)x;
      log[x] = i;
      x <<= 1;
      if (x & 0x100) x ^= 0x11d;
    }
    log[0] = 0;
  }
  uint8_t mul(uint8_t a, uint8_t b) const { return a && b ? exp[(log[a] + log[b]) % 255] : 0; }
  uint8_t gpow(int e) const { return exp[((e % 255) + 255) % 255]; }
};
const Gf g_gf;

// ---------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------
std::atomic<unsigned long long *> g_last_ctr{nullptr};

// body(ctx, exec): exec false when enqueued, true when executed.
template <typename F>
hipError_t launch(hipStream_t st, const char *name, F body, bool kernel = true) {
  read_schedule();
  Stream *s = as_stream(st, name);
  if (!s) return hipErrorInvalidHandle;
  if (kernel && t_dev != s->dev)
    finding("%s: launched on a stream of device %d while the thread's current device is %d", name, s->dev, t_dev);
  auto seen = std::make_shared<std::set<std::string>>();
  auto tables = std::make_shared<std::pair<bool, uint64_t>>(false, 0);
  std::vector<Range> ranges;
  {
    std::shared_lock<std::shared_mutex> lk(g_mem);
    Ctx c{name, s->dev, &ranges, seen.get(), tables.get()};
    body(c, false);
  }
  const int dev = s->dev;
  s->push(name, std::move(ranges), [name, dev, seen, tables, body, kernel] {
    {
      std::shared_lock<std::shared_mutex> lk(g_mem);
      Ctx c{name, dev, nullptr, seen.get(), tables.get()};
      body(c, true);
    }
    // a slow device: the next batches are submitted while this one is still on its queue
    if (kernel && g_launch_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(g_launch_us));
  });
  return hipSuccess;
}

// The work-queue counter at the start of a launch, and after it.
void take_counter(Ctx &c, unsigned long long *ctr, unsigned long long base, unsigned long long advance) {
  if (!c.need(ctr, 8, "work-queue counter")) return;
  g_last_ctr.store(ctr);
  const unsigned long long v = __atomic_load_n(ctr, __ATOMIC_RELAXED);
  if (v != base)
    c.fail("%s: the work-queue counter is %llu when the launch starts, its base %llu", c.op, v, base);
  __atomic_store_n(ctr, base + advance, __ATOMIC_RELAXED);  // (back in step after a finding)
}

// The byte loops run uninstrumented (one check per byte would make a 10 MiB
// window take seconds under a sanitizer); what they are about to read or write
// is announced to the sanitizer as whole ranges instead, so a host thread that
// touches a slab while the "device" works on it is still a reported race, and
// memory the registry believes live but the allocator has freed still a report.
#if defined(__has_feature)
#if __has_feature(thread_sanitizer)
#define HD_TSAN 1
#endif
#if __has_feature(address_sanitizer)
#define HD_ASAN 1
#endif
#endif
#if defined(__SANITIZE_THREAD__)
#define HD_TSAN 1
#endif
#if defined(__SANITIZE_ADDRESS__)
#define HD_ASAN 1
#endif
#ifdef HD_TSAN
extern "C" void __tsan_read_range(void *addr, unsigned long size);
extern "C" void __tsan_write_range(void *addr, unsigned long size);
#endif
#ifdef HD_ASAN
extern "C" void *__asan_region_is_poisoned(void *beg, size_t size);
#endif
#define HD_RAW __attribute__((no_sanitize_address, no_sanitize_thread, noinline))

void will_read(const void *p, uint64_t n) {
  (void)p;
  if (!n) return;
#ifdef HD_TSAN
  __tsan_read_range(const_cast<void *>(p), n);
#endif
#ifdef HD_ASAN
  if (void *bad = __asan_region_is_poisoned(const_cast<void *>(p), n))
    finding("the registry holds [%p, +%llu) live, the allocator has %p poisoned", p, (unsigned long long)n, bad);
#endif
}
void will_write(void *p, uint64_t n) {
  (void)p;
  if (!n) return;
#ifdef HD_TSAN
  __tsan_write_range(p, n);
#endif
#ifdef HD_ASAN
  if (void *bad = __asan_region_is_poisoned(p, n))
    finding("the registry holds [%p, +%llu) live, the allocator has %p poisoned", p, (unsigned long long)n, bad);
#endif
}

// acc[j] ^= c * (stream of the source at j) for j < n, c through its product
// row (nullptr: c = 1).  The stream (bcp.h): the source zero padded, or with a
// window W (given as the last readable window's base and the offset `lim` from
// which it is replayed) the replay of that window.
HD_RAW void fold_stream(uint8_t *acc, const uint8_t *row, const uint8_t *p, uint64_t len, uint64_t base, uint64_t lim,
                        uint64_t n) {
  const uint64_t W = lim - base;
  for (uint64_t j = 0; j < n; j++) {
    uint64_t o = j;
    if (j >= lim) o = base + j % W;
    const uint8_t d = o < len ? p[o] : 0;
    acc[j] ^= row ? row[d] : d;
  }
}
HD_RAW void put_bytes(uint8_t *dst, const uint8_t *src, uint64_t n) {
  for (uint64_t j = 0; j < n; j++) dst[j] = src[j];
}
HD_RAW void zero_bytes(uint8_t *dst, uint64_t n) {
  for (uint64_t j = 0; j < n; j++) dst[j] = 0;
}
// fold against what is stored: the smallest differing j (UINT64_MAX: none) and their number
HD_RAW void diff_bytes(const uint8_t *a, const uint8_t *b, uint64_t n, uint64_t *first, uint64_t *count) {
  for (uint64_t j = 0; j < n; j++)
    if (a[j] != b[j]) {
      if (j < *first) *first = j;
      ++*count;
    }
}

struct XorStripe {
  uint64_t dst, out_len, window;
  std::vector<bcp_source> src;
};

// Ranges of a fold (or check) batch: every source, every output.
bool xor_ranges(Ctx &c, const std::vector<XorStripe> &v, const char *dst_what) {
  bool ok = true;
  for (size_t s = 0; s < v.size(); s++) {
    for (size_t k = 0; k < v[s].src.size(); k++)
      ok &= c.need((const void *)v[s].src[k].ptr, v[s].src[k].len, "source", (long)s);
    ok &= c.need((const void *)v[s].dst, v[s].out_len, dst_what, (long)s);
  }
  return ok;
}

void xor_fold_of(const XorStripe &x, std::vector<uint8_t> &out) {
  out.assign(x.out_len, 0);
  uint64_t longest = 0;
  for (const bcp_source &so : x.src) longest = so.len > longest ? so.len : longest;
  for (const bcp_source &so : x.src) {
    if (!so.len) continue;
    will_read((const void *)so.ptr, so.len);
    const uint64_t W = x.window, lw = W ? (so.len - 1) / W : 0;
    fold_stream(out.data(), nullptr, (const uint8_t *)so.ptr, so.len, W ? lw * W : 0, W ? (lw + 1) * W : ~0ull,
                x.out_len);
  }
  // with a window the replayed stream ends with the stripe's longest source
  if (x.window && longest < x.out_len) zero_bytes(out.data() + longest, x.out_len - longest);
}

void xor_store(const std::vector<XorStripe> &v) {
  std::vector<uint8_t> out;
  for (const XorStripe &x : v) {
    xor_fold_of(x, out);
    will_write((void *)x.dst, x.out_len);
    put_bytes((uint8_t *)x.dst, out.data(), x.out_len);
  }
}

// The tables of a descriptor batch, once their own ranges are known good.
bool desc_stripes(Ctx &c, const DescBatch &b, std::vector<XorStripe> &v) {
  bool ok = true;
  v.resize(b.nstripes);
  for (uint32_t s = 0; s < b.nstripes; s++) {
    const bcp_stripe &st = b.stripes[s];
    v[s] = XorStripe{st.dst, st.out_len, st.window, {}};
    if (!c.need(b.sources + st.first_src, (uint64_t)st.nsrc * sizeof(bcp_source), "source table", (long)s)) {
      ok = false;
      continue;
    }
    v[s].src.assign(b.sources + st.first_src, b.sources + st.first_src + st.nsrc);
  }
  return ok;
}

uint64_t fnv(uint64_t h, const void *p, size_t n) {
  const uint8_t *b = (const uint8_t *)p;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
  return h;
}
uint64_t desc_stamp(const DescBatch &b, const std::vector<XorStripe> &v) {
  uint64_t h = fnv(0xCBF29CE484222325ull, b.stripes, (size_t)b.nstripes * sizeof(bcp_stripe));
  for (const XorStripe &x : v) h = fnv(h, x.src.data(), x.src.size() * sizeof(bcp_source));
  h = fnv(h, b.tile_start, ((size_t)b.nstripes + 1) * sizeof(uint32_t));
  return fnv(h, &b.tile_bytes, sizeof b.tile_bytes);
}

bool desc_tables(Ctx &c, const DescBatch &b, bool with_ctr) {
  bool ok = true;
  if (with_ctr) ok &= c.need(b.ctr, 8, "work-queue counter");
  ok &= c.need(b.stripes, (uint64_t)b.nstripes * sizeof(bcp_stripe), "stripe table");
  ok &= c.need(b.tile_start, ((uint64_t)b.nstripes + 1) * sizeof(uint32_t), "tile starts");
  ok &= c.need(b.tiles, (uint64_t)b.ntiles * sizeof(DescTile), "tile records");
  return ok;
}

// desc_tiles, xor_desc and check_desc in one: which = 0, 1, 2.
void desc_body(Ctx &c, bool exec, int which, int grid, const DescBatch &b0, bcp_check_result *res) {
  bool ok = desc_tables(c, b0, which != 0);
  if (which == 2) ok &= c.need(res, (uint64_t)b0.nstripes * sizeof(*res), "result records");
  std::vector<XorStripe> v;
  // at the launch call, tables on their way to the device are read where the upload reads them
  DescBatch b = b0;
  if (!exec) b.stripes = staged(b0.stripes), b.sources = staged(b0.sources), b.tile_start = staged(b0.tile_start);
  const bool content =
      ok && (exec || (host_resident(b.stripes) && host_resident(b.sources) && host_resident(b.tile_start)));
  if (content && !exec) ok &= desc_tables(c, b, false);
  if (content && ok) {
    ok &= desc_stripes(c, b, v);
    if (b.tile_start[b.nstripes] != b.ntiles)
      c.fail("%s: tile_start[%u] = %u, the batch has %u tiles", c.op, b.nstripes, b.tile_start[b.nstripes], b.ntiles);
    // the cut itself is the code under test's; what holds for any cut: a stripe has no tile exactly when
    // it has no output, never more tiles than subtiles, and one per subtile under a window
    for (uint32_t s = 0; s < b.nstripes && ok; s++) {
      const uint64_t lo = b.tile_start[s], hi = b.tile_start[s + 1];
      const uint64_t nsub = (v[s].out_len + b.tile_bytes - 1) / b.tile_bytes;
      if (hi < lo || (hi == lo) != (nsub == 0) || hi - lo > nsub || (v[s].window && hi - lo != nsub))
        c.fail("%s: stripe %u: tiles [%llu, %llu) for %llu subtiles%s", c.op, s, (unsigned long long)lo,
               (unsigned long long)hi, (unsigned long long)nsub, v[s].window ? " under a window" : "");
    }
    ok &= xor_ranges(c, v, which == 2 ? "checked body" : "destination");
    if (ok) c.same_tables(desc_stamp(b, v), exec);
  }
  if (!exec) return;
  if (which != 0) take_counter(c, b.ctr, b.base, (unsigned long long)b.ntiles + (unsigned long long)grid);
  if (!ok || !c.ok) return;  // nothing is computed from what failed a check
  const uint64_t stamp = desc_stamp(b, v);
  if (which == 0) {
    for (uint32_t i = 0; i < b.ntiles; i++) {
      memset(&b.tiles[i], 0, sizeof(DescTile));
      b.tiles[i].dst = stamp ^ i;
      b.tiles[i].meta = 0xD0B1Eu;
    }
    return;
  }
  for (uint32_t i = 0; i < b.ntiles; i++)
    if (b.tiles[i].dst != (stamp ^ i) || b.tiles[i].meta != 0xD0B1Eu) {
      c.fail("%s: tile record %u of %u is not what desc_tiles wrote for these tables", c.op, i, b.ntiles);
      return;
    }
  if (which == 1) {
    xor_store(v);
    return;
  }
  std::vector<uint8_t> out;
  for (uint32_t s = 0; s < b.nstripes; s++) {
    xor_fold_of(v[s], out);
    will_read((const void *)v[s].dst, v[s].out_len);
    diff_bytes(out.data(), (const uint8_t *)v[s].dst, v[s].out_len, &res[s].first_bad, &res[s].bad_bytes);
  }
}

// ---- P + Q ---------------------------------------------------------------
struct PqView {
  PqStripe r;
  std::vector<bcp_source> src;
  std::vector<PqWin> win;       // windowed batch: per source
  std::vector<uint8_t> listed;  // subtile j of the stripe is in the tile table
};

// form 0 GEN, 1 SOLVE, 2 CHECK, 3 ranges only.  Tables, then (when they can be read) what they name.
bool pq_views(Ctx &c, bool exec, bool content, int vecs, int form, const PqBatch &b, const PqWinTab *w, const void *res,
              size_t res_size, std::vector<PqView> &v) {
  bool ok = c.need(b.ctr, 8, "work-queue counter");
  ok &= c.need(b.tiles, (uint64_t)b.ntiles * sizeof(PqTile), "tile table");
  if (w) ok &= c.need(w->offw, (uint64_t)b.ntiles * sizeof(uint64_t), "offw table");
  if (!ok || !content) return ok;
  const uint64_t T = desc_tile_bytes(vecs);
  uint32_t nstripes = 0;
  for (uint32_t t = 0; t < b.ntiles; t++) nstripes = b.tiles[t].stripe >= nstripes ? b.tiles[t].stripe + 1 : nstripes;
  ok &= c.need(b.stripes, (uint64_t)nstripes * sizeof(PqStripe), "stripe table");
  if (res) ok &= c.need(res, (uint64_t)nstripes * res_size, "result records");
  if (!ok) return false;
  v.resize(nstripes);
  for (uint32_t s = 0; s < nstripes; s++) {
    PqView &x = v[s];
    x.r = b.stripes[s];
    const PqStripe &r = x.r;
    if (!c.need(b.sources + r.first_src, (uint64_t)r.nsrc * sizeof(bcp_source), "source table", (long)s) ||
        (w && !c.need(w->win + r.first_src, (uint64_t)r.nsrc * sizeof(PqWin), "window table", (long)s))) {
      ok = false;
      continue;
    }
    x.src.assign(b.sources + r.first_src, b.sources + r.first_src + r.nsrc);
    if (w) x.win.assign(w->win + r.first_src, w->win + r.first_src + r.nsrc);
    for (uint32_t k = 0; k < r.nsrc; k++) ok &= c.need((const void *)x.src[k].ptr, x.src[k].len, "source", (long)s);
    if (form == 1 || form == 3) {  // 3: a form that is only range-checked; P where there is one
      if (r.p) ok &= c.need((const void *)r.p, r.out_len, "P body", (long)s);
      ok &= c.need((const void *)r.q, r.out_len, "Q body", (long)s);
      ok &= c.need((const void *)r.dx, r.len_x, "rebuilt member x", (long)s);
      ok &= c.need((const void *)r.dy, r.len_y, "rebuilt member y", (long)s);
    } else {
      if (r.p || form == 2) ok &= c.need((const void *)r.p, r.out_len, form ? "P body" : "P output", (long)s);
      ok &= c.need((const void *)r.q, r.out_len, form ? "Q body" : "Q output", (long)s);
    }
  }
  for (uint32_t t = 0; t < b.ntiles; t++) {
    PqView &x = v[b.tiles[t].stripe];
    const uint32_t sub = b.tiles[t].sub;
    if (x.listed.size() <= sub) x.listed.resize((size_t)sub + 1, 0);
    if (x.listed[sub]++) c.fail("%s: stripe %u: subtile %u is listed twice", c.op, b.tiles[t].stripe, sub);
    if (w) {
      // offw is (sub * T) mod W where a source of the stripe replays, 0 where none has a window
      uint64_t W = 0;
      for (const PqWin &pw : x.win)
        if (pw.lim != ~0ull) W = pw.lim - pw.base;
      const uint64_t want = W ? ((uint64_t)sub * T) % W : 0;
      if (W && w->offw[t] != want)
        c.fail("%s: stripe %u: offw[%u] = %llu, (sub * T) mod W is %llu", c.op, b.tiles[t].stripe, t,
               (unsigned long long)w->offw[t], (unsigned long long)want);
    }
  }
  if (ok) {
    uint64_t h = fnv(0xCBF29CE484222325ull, b.tiles, (size_t)b.ntiles * sizeof(PqTile));
    h = fnv(h, b.stripes, (size_t)nstripes * sizeof(PqStripe));
    for (const PqView &x : v) {
      h = fnv(h, x.src.data(), x.src.size() * sizeof(bcp_source));
      h = fnv(h, x.win.data(), x.win.size() * sizeof(PqWin));
    }
    if (w) h = fnv(h, w->offw, (size_t)b.ntiles * sizeof(uint64_t));
    c.same_tables(h, exec);
  }
  return ok && c.ok;
}

// One stripe's part of the SOLVE and CHECK forms, over the listed subtiles.
HD_RAW void pq_solve_bytes(const PqStripe &r, const uint8_t *P, const uint8_t *Q, uint64_t n, const uint8_t *listed,
                           uint64_t nlisted, uint64_t T, const uint8_t *row_a, const uint8_t *row_b) {
  const uint8_t *pb = (const uint8_t *)r.p, *qb = (const uint8_t *)r.q;
  uint8_t *dx = (uint8_t *)r.dx, *dy = (uint8_t *)r.dy;
  for (uint64_t j = 0; j < n; j++) {
    if (j / T >= nlisted || !listed[j / T]) continue;
    const uint8_t ps = (uint8_t)(P[j] ^ (pb ? pb[j] : 0)), qs = (uint8_t)(Q[j] ^ qb[j]);
    const uint8_t x = (uint8_t)(row_a[ps] ^ row_b[qs]);
    if (j < r.len_x) dx[j] = x;
    if (j < r.len_y) dy[j] = (uint8_t)(ps ^ x);
  }
}
HD_RAW void pq_check_bytes(const PqStripe &r, const uint8_t *P, const uint8_t *Q, uint64_t n, const uint8_t *listed,
                           uint64_t nlisted, uint64_t T, const uint8_t (*rows)[256], bcp_pq_check_result *o) {
  const uint8_t *pb = (const uint8_t *)r.p, *qb = (const uint8_t *)r.q;
  for (uint64_t j = 0; j < n; j++) {
    if (j / T >= nlisted || !listed[j / T]) continue;
    const uint8_t ps = (uint8_t)(P[j] ^ pb[j]), qs = (uint8_t)(Q[j] ^ qb[j]);
    if (!ps && !qs) continue;
    if (j < o->first_bad) o->first_bad = j;
    o->p_bad += ps != 0;
    o->q_bad += qs != 0;
    if (!qs) {
      o->members |= BCP_PQ_BAD_P;
    } else if (!ps) {
      o->members |= BCP_PQ_BAD_Q;
    } else {
      uint64_t bit = BCP_PQ_BAD_NOWHERE;
      for (uint32_t k = 0; k < r.nsrc; k++)
        if (rows[k][ps] == qs) bit = 1ull << k;  // g^k * Ps = Qs names position k
      o->members |= bit;
    }
  }
}
HD_RAW void put_listed(uint8_t *dst, const uint8_t *src, uint64_t n, const uint8_t *listed, uint64_t nlisted,
                       uint64_t T) {
  for (uint64_t j = 0; j < n; j++)
    if (j / T < nlisted && listed[j / T]) dst[j] = src[j];
}

void pq_compute(int vecs, int form, std::vector<PqView> &v, bool windowed, bcp_pq_check_result *res) {
  const uint64_t T = desc_tile_bytes(vecs);
  static uint8_t rows[256][256];  // rows[k][d] = g^k * d (built once; k < 255 is all a stripe can have)
  static std::once_flag once;
  std::call_once(once, [] {
    for (int k = 0; k < 256; k++)
      for (int d = 0; d < 256; d++) rows[k][d] = g_gf.mul(g_gf.gpow(k), (uint8_t)d);
  });
  std::vector<uint8_t> P, Q;
  for (size_t s = 0; s < v.size(); s++) {
    PqView &x = v[s];
    const PqStripe &r = x.r;
    uint64_t n = r.out_len;
    if (form == 1) n = r.len_x > r.len_y ? r.len_x : r.len_y;
    P.assign(n, 0);
    Q.assign(n, 0);
    for (uint32_t k = 0; k < r.nsrc; k++) {
      const bcp_source &so = x.src[k];
      if (!so.len) continue;
      uint64_t base = 0, lim = ~0ull;
      if (windowed) base = x.win[k].base, lim = x.win[k].lim;  // ({0, ~0}: never replayed)
      will_read((const void *)so.ptr, so.len);
      fold_stream(P.data(), nullptr, (const uint8_t *)so.ptr, so.len, base, lim, n);
      fold_stream(Q.data(), rows[k], (const uint8_t *)so.ptr, so.len, base, lim, n);
    }
    const uint8_t *listed = x.listed.data();
    const uint64_t nl = x.listed.size();
    if (form == 0) {
      if (r.p) will_write((void *)r.p, n), put_listed((uint8_t *)r.p, P.data(), n, listed, nl, T);
      will_write((void *)r.q, n);
      put_listed((uint8_t *)r.q, Q.data(), n, listed, nl, T);
    } else if (form == 1) {
      uint8_t row_a[256], row_b[256];
      for (int d = 0; d < 256; d++) {
        row_a[d] = g_gf.mul((uint8_t)r.ca, (uint8_t)d);
        row_b[d] = g_gf.mul((uint8_t)r.cb, (uint8_t)d);
      }
      if (r.p) will_read((const void *)r.p, n);
      will_read((const void *)r.q, n);
      will_write((void *)r.dx, r.len_x);
      will_write((void *)r.dy, r.len_y);
      pq_solve_bytes(r, P.data(), Q.data(), n, listed, nl, T, row_a, row_b);
    } else {
      will_read((const void *)r.p, n);
      will_read((const void *)r.q, n);
      pq_check_bytes(r, P.data(), Q.data(), n, listed, nl, T, rows, &res[s]);
    }
  }
}

hipError_t pq_launch(hipStream_t st, const char *name, int grid, int vecs, int form, const PqBatch &b,
                     const PqWinTab *wt, bcp_pq_check_result *res) {
  if (grid <= 0 || !pq_vecs_ok(vecs) || (form == 2 && !res)) return hipErrorInvalidValue;
  const bool windowed = wt != nullptr;
  const PqWinTab w = wt ? *wt : PqWinTab{nullptr, nullptr};
  return launch(st, name, [=](Ctx &c, bool exec) {
    std::vector<PqView> v;
    // at the launch call, tables on their way to the device are read where the upload reads them (desc_body)
    PqBatch e = b;
    PqWinTab ew = w;
    bool content = true;
    if (!exec) {
      e.stripes = staged(b.stripes), e.sources = staged(b.sources), e.tiles = staged(b.tiles);
      if (windowed) ew.win = staged(w.win), ew.offw = staged(w.offw);
      content = host_resident(e.stripes) && host_resident(e.sources) && host_resident(e.tiles) &&
                (!windowed || (host_resident(ew.win) && host_resident(ew.offw)));
      if (e.tiles != b.tiles) {  // the device's own copy is part of what the pending launch refers to
        c.need(b.tiles, (uint64_t)b.ntiles * sizeof(PqTile), "tile table");
        if (windowed) c.need(w.offw, (uint64_t)b.ntiles * sizeof(uint64_t), "offw table");
      }
    }
    const bool ok = pq_views(c, exec, content, vecs, form, e, windowed ? &ew : nullptr, form == 2 ? res : nullptr,
                             sizeof(bcp_pq_check_result), v);
    if (!exec) return;
    take_counter(c, b.ctr, b.base, (unsigned long long)b.ntiles + (unsigned long long)grid);
    if (ok && c.ok) pq_compute(vecs, form, v, windowed, res);
  });
}

// A form the stand-in does not compute: its ranges are checked, then the
// launch is refused, so nothing passes through it unnoticed.
hipError_t pq_refuse(hipStream_t st, const char *name, int vecs, const PqBatch &b, const PqWinTab *wt, const void *res,
                     size_t res_size) {
  read_schedule();
  Stream *s = as_stream(st, name);
  if (!s) return hipErrorInvalidHandle;
  std::shared_lock<std::shared_mutex> lk(g_mem);
  std::set<std::string> seen;
  Ctx c{name, s->dev, nullptr, &seen};
  std::vector<PqView> v;
  pq_views(c, false, host_resident(b.tiles) && host_resident(b.stripes), vecs, 3, b, wt, res, res_size, v);
  return hipErrorNotSupported;
}

hipError_t refuse_ranges(hipStream_t st, const char *name, std::initializer_list<std::pair<const void *, uint64_t>> rs) {
  read_schedule();
  Stream *s = as_stream(st, name);
  if (!s) return hipErrorInvalidHandle;
  std::shared_lock<std::shared_mutex> lk(g_mem);
  std::set<std::string> seen;
  Ctx c{name, s->dev, nullptr, &seen};
  for (const auto &r : rs) c.need(r.first, r.second, "buffer");
  return hipErrorNotSupported;
}

}  // namespace

// ---------------------------------------------------------------------------
// the launchers of bcp_internal.h
// ---------------------------------------------------------------------------
namespace bcp {

uint32_t stream_tiles_per_stripe(uint64_t chunk_bytes, int vecs) {
  // a tile is 256 lanes x vecs vectors of 16 bytes; a byte tail still takes a vector
  const uint64_t tile = 256ull * 16ull * (uint64_t)vecs;
  const uint64_t bytes = (chunk_bytes + 15) / 16 * 16;
  return (uint32_t)((bytes + tile - 1) / tile);
}

hipError_t launch_xor_stream(hipStream_t st, int grid, int vecs, bool gather, const StreamArgs &a0) {
  if (a0.ntiles == 0) return hipSuccess;
  if (grid <= 0 || !a0.tps || !a0.grab) return hipErrorInvalidValue;
  (void)vecs;
  const StreamArgs a1 = a0;
  return launch(st, gather ? "xor_stream (gather)" : "xor_stream", [=](Ctx &c, bool exec) {
    const uint32_t nstripes = a1.ntiles / a1.tps;
    const uint64_t len = (uint64_t)a1.vps * 16u + a1.tail;
    bool ok = c.need(a1.ctr, 8, "work-queue counter");
    std::vector<XorStripe> v;
    bool content = true;
    StreamArgs a = a1;
    if (gather) {
      ok &= c.need(a1.stripes, (uint64_t)nstripes * sizeof(bcp_stripe), "stripe table");
      // at the launch call, tables on their way to the device are read where the upload reads them (desc_body)
      if (!exec) a.stripes = staged(a1.stripes), a.sources = staged(a1.sources);
      content = ok && (exec || (host_resident(a.stripes) && host_resident(a.sources)));
      if (content && !exec) ok &= c.need(a.stripes, (uint64_t)nstripes * sizeof(bcp_stripe), "stripe table");
    }
    if (content) {
      v.resize(nstripes);
      for (uint32_t s = 0; s < nstripes; s++) {
        XorStripe &x = v[s];
        x.out_len = len;
        x.window = 0;
        if (gather) {
          const uint32_t first = a.dense ? s * a.nsrc : a.stripes[s].first_src;
          x.dst = a.stripes[s].dst;
          if (!c.need(a.sources + first, (uint64_t)a.nsrc * sizeof(bcp_source), "source table", (long)s)) {
            ok = false;
            continue;
          }
          for (uint32_t k = 0; k < a.nsrc; k++) x.src.push_back(bcp_source{a.sources[first + k].ptr, len});
        } else {
          x.dst = (uint64_t)a.dst + s * a.dst_stride;
          for (uint32_t k = 0; k < a.nsrc; k++)
            x.src.push_back(bcp_source{(uint64_t)a.src + s * a.stripe_stride + k * a.src_stride, len});
        }
      }
      ok &= xor_ranges(c, v, "destination");
      if (ok && gather) {
        uint64_t h = fnv(0xCBF29CE484222325ull, a.stripes, (size_t)nstripes * sizeof(bcp_stripe));
        for (const XorStripe &x : v) h = fnv(h, x.src.data(), x.src.size() * sizeof(bcp_source));
        c.same_tables(h, exec);
      }
    }
    if (!exec) return;
    take_counter(c, a.ctr, a.base, ((unsigned long long)a.ntiles + a.grab - 1) / a.grab + (unsigned long long)grid);
    if (ok && c.ok) xor_store(v);
  });
}

hipError_t launch_desc_tiles(hipStream_t st, const DescBatch &b0) {
  const DescBatch b = b0;
  return launch(st, "desc_tiles", [=](Ctx &c, bool exec) { desc_body(c, exec, 0, 0, b, nullptr); });
}

hipError_t launch_xor_desc(hipStream_t st, int grid, int vecs, const DescBatch &b0) {
  if (grid <= 0 || b0.tile_bytes != desc_tile_bytes(vecs)) return hipErrorInvalidValue;
  const DescBatch b = b0;
  return launch(st, "xor_desc", [=](Ctx &c, bool exec) { desc_body(c, exec, 1, grid, b, nullptr); });
}

hipError_t launch_check_init(hipStream_t st, bcp_check_result *res, uint32_t n) {
  return launch(st, "check_init", [=](Ctx &c, bool exec) {
    if (!c.need(res, (uint64_t)n * sizeof(*res), "result records") || !exec) return;
    for (uint32_t i = 0; i < n; i++) res[i] = bcp_check_result{UINT64_MAX, 0};
  });
}

hipError_t launch_check_desc(hipStream_t st, int grid, int vecs, const DescBatch &b0, bcp_check_result *res) {
  if (grid <= 0 || !res || b0.tile_bytes != desc_tile_bytes(vecs)) return hipErrorInvalidValue;
  const DescBatch b = b0;
  return launch(st, "check_desc", [=](Ctx &c, bool exec) { desc_body(c, exec, 2, grid, b, res); });
}

hipError_t launch_xor_desc_args(hipStream_t st, int grid, int vecs, const DescArgs &a0) {
  if (grid <= 0 || a0.nstripes > (uint32_t)kArgStripes) return hipErrorInvalidValue;
  const DescArgs a = a0;
  return launch(st, "xor_desc_args", [=](Ctx &c, bool exec) {
    std::vector<XorStripe> v(a.nstripes);
    bool ok = c.need(a.ctr, 8, "work-queue counter");
    for (uint32_t s = 0; s < a.nstripes; s++) {
      v[s] = XorStripe{a.dst[s], a.out_len[s], 0, {}};
      if ((uint64_t)a.first[s] + a.nsrc[s] > (uint64_t)kArgSources) {
        c.fail("%s: stripe %u: sources [%u, +%u) past the %d the arguments hold", c.op, s, a.first[s], a.nsrc[s],
               kArgSources);
        ok = false;
        continue;
      }
      for (uint32_t k = 0; k < a.nsrc[s]; k++)
        v[s].src.push_back(bcp_source{a.src_ptr[a.first[s] + k], a.src_len[a.first[s] + k]});
    }
    if (a.tile_start[a.nstripes] != a.ntiles)
      c.fail("%s: tile_start[%u] = %u, the batch has %u tiles", c.op, a.nstripes, a.tile_start[a.nstripes], a.ntiles);
    for (uint32_t s = 0; s < a.nstripes; s++) {  // this form has one tile per subtile
      const uint64_t T = desc_tile_bytes(vecs), nsub = (a.out_len[s] + T - 1) / T;
      if ((uint64_t)a.tile_start[s] + nsub != a.tile_start[s + 1])
        c.fail("%s: stripe %u: tiles [%u, %u) for %llu subtiles", c.op, s, a.tile_start[s], a.tile_start[s + 1],
               (unsigned long long)nsub);
    }
    ok &= xor_ranges(c, v, "destination");
    if (!exec) return;
    take_counter(c, a.ctr, a.base, (unsigned long long)a.ntiles + (unsigned long long)grid);
    if (ok && c.ok) xor_store(v);
  });
}

hipError_t launch_pq(hipStream_t st, int grid, int vecs, bool solve, const PqBatch &b) {
  return pq_launch(st, solve ? "pq_desc (solve)" : "pq_desc (gen)", grid, vecs, solve ? 1 : 0, b, nullptr, nullptr);
}

hipError_t launch_pq_win(hipStream_t st, int grid, int vecs, int form, const PqBatchWin &b, bcp_pq_check_result *res) {
  if (form < 0 || form > 2) return hipErrorInvalidValue;
  static const char *const name[3] = {"pq_win_desc (gen)", "pq_win_desc (solve)", "pq_win_desc (check)"};
  return pq_launch(st, name[form], grid, vecs, form, b.b, &b.w, res);
}

hipError_t launch_pq_check_init(hipStream_t st, bcp_pq_check_result *res, uint32_t n) {
  return launch(st, "pq_check_init", [=](Ctx &c, bool exec) {
    if (!c.need(res, (uint64_t)n * sizeof(*res), "result records") || !exec) return;
    for (uint32_t i = 0; i < n; i++) res[i] = bcp_pq_check_result{UINT64_MAX, 0, 0, 0};
  });
}

hipError_t launch_pq_check(hipStream_t st, int grid, int vecs, const PqBatch &b, bcp_pq_check_result *res) {
  return pq_launch(st, "pq_desc (check)", grid, vecs, 2, b, nullptr, res);
}

hipError_t launch_pq_repair_init(hipStream_t st, bcp_pq_repair_result *res, uint32_t n) {
  return refuse_ranges(st, "pq_repair_init", {{res, (uint64_t)n * sizeof(*res)}});
}
hipError_t launch_pq_repair(hipStream_t st, int, int vecs, const PqBatch &b, bcp_pq_repair_result *res) {
  return pq_refuse(st, "pq_repair_desc", vecs, b, nullptr, res, sizeof(*res));
}
hipError_t launch_pq_repair_win(hipStream_t st, int, int vecs, const PqBatchWin &b, bcp_pq_repair_result *res) {
  return pq_refuse(st, "pq_repair_win_desc", vecs, b.b, &b.w, res, sizeof(*res));
}
hipError_t launch_pq_rebuild(hipStream_t st, int, int vecs, const PqBatch &b, bcp_check_result *res) {
  return pq_refuse(st, "pq_rebuild_desc", vecs, b, nullptr, res, sizeof(*res));
}
hipError_t launch_pq_rebuild_win(hipStream_t st, int, int vecs, const PqBatchWin &b, bcp_check_result *res) {
  return pq_refuse(st, "pq_rebuild_win_desc", vecs, b.b, &b.w, res, sizeof(*res));
}

hipError_t launch_fold_ring(hipStream_t st, int, const RingArgs &a) {
  const uint64_t K = (uint64_t)a.kmask + 1;
  return refuse_ranges(st, "fold_ring",
                       {{a.host, K * sizeof(RingEntry)},
                        {a.done, K * kRingDoneStride * sizeof(unsigned long long)},
                        {a.closed, 8},
                        {a.stop, 4},
                        {a.state, sizeof(RingState)},
                        {a.claim, K * 8},
                        {a.cnt, K * 8},
                        {a.copy, K * sizeof(RingEntry)}});
}
hipError_t launch_fill_synthetic(hipStream_t st, int, char *dst, uint64_t bytes, uint64_t, uint64_t) {
  return refuse_ranges(st, "fill_synthetic", {{dst, bytes}});
}
hipError_t launch_xor_fold(hipStream_t st, int, const char *src, uint64_t bytes, uint32_t *out4) {
  return refuse_ranges(st, "xor_fold", {{src, bytes}, {out4, 16}});
}
hipError_t launch_compare(hipStream_t st, int, const char *a, const char *b, uint64_t bytes, unsigned long long *out) {
  return refuse_ranges(st, "compare", {{a, bytes}, {b, bytes}, {out, 8}});
}

}  // namespace bcp

// ---------------------------------------------------------------------------
// the HIP runtime functions the engine's host code calls
// ---------------------------------------------------------------------------
extern "C" {

hipError_t hipGetDeviceCount(int *count) {
  read_schedule();  // (the first call of every program here)
  if (!count) return hipErrorInvalidValue;
  *count = g_devices;
  return hipSuccess;
}

hipError_t hipSetDevice(int device) {
  if (device < 0 || device >= g_devices) return t_last = hipErrorInvalidDevice;
  t_dev = device;
  return hipSuccess;
}

hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600 *prop, int device) {
  if (!prop || device < 0 || device >= g_devices) return hipErrorInvalidDevice;
  memset(prop, 0, sizeof(*prop));
  snprintf(prop->name, sizeof prop->name, "hipdouble device %d", device);
  snprintf(prop->gcnArchName, sizeof prop->gcnArchName, "cpu");
  prop->multiProcessorCount = 8;  // small grids: the counter's advance differs visibly from the tile count
  return hipSuccess;
}

hipError_t hipDeviceGetAttribute(int *pi, hipDeviceAttribute_t attr, int device) {
  if (!pi || device < 0 || device >= g_devices) return hipErrorInvalidValue;
  *pi = attr == hipDeviceAttributeWallClockRate ? 100000 : 0;
  return hipSuccess;
}

hipError_t hipDeviceGetPCIBusId(char *bus, int len, int device) {
  if (!bus || len < 13 || device < 0 || device >= g_devices) return hipErrorInvalidValue;
  snprintf(bus, (size_t)len, "0000:%02x:00.0", device + 1);
  return hipSuccess;
}

const char *hipGetErrorString(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorNotReady: return "device not ready";
    case hipErrorNotSupported: return "operation not supported (hipdouble computes no such form)";
    case hipErrorInvalidHandle: return "invalid resource handle";
    default: return "hipdouble error";
  }
}

hipError_t hipGetLastError(void) {
  const hipError_t e = t_last;
  t_last = hipSuccess;
  return e;
}

hipError_t hipMalloc(void **ptr, size_t size) { return add_alloc(ptr, size, kDevice); }
hipError_t hipExtMallocWithFlags(void **ptr, size_t size, unsigned int) { return add_alloc(ptr, size, kDevice); }
hipError_t hipFree(void *ptr) { return drop_alloc(ptr, "hipFree", true); }
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int) { return add_alloc(ptr, size, kPinned); }
hipError_t hipHostFree(void *ptr) { return drop_alloc(ptr, "hipHostFree", true); }

hipError_t hipHostRegister(void *p, size_t n, unsigned int flags) {
  read_schedule();
  if (!p || !n) return hipErrorInvalidValue;
  std::unique_lock<std::shared_mutex> lk(g_mem);
  if (find_alloc(p) || find_alloc((char *)p + n - 1)) return t_last = hipErrorHostMemoryAlreadyRegistered;
  g_allocs[(uintptr_t)p] = Alloc{(uintptr_t)p, n, kRegistered, flags & hipHostRegisterPortable ? -1 : t_dev, false};
  return hipSuccess;
}

hipError_t hipHostUnregister(void *p) { return drop_alloc(p, "hipHostUnregister", false); }

hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int) {
  if (!dev) return hipErrorInvalidValue;
  std::shared_lock<std::shared_mutex> lk(g_mem);
  const Alloc *a = find_alloc(host);
  if (!a || a->kind == kDevice) return t_last = hipErrorInvalidValue;
  *dev = host;  // the kernels address host rows by their host address
  return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *out, unsigned int) {
  read_schedule();
  if (!out) return hipErrorInvalidValue;
  Stream *s = new Stream();
  s->dev = t_dev;
  s->th = std::thread(&Stream::loop, s);
  std::lock_guard<std::mutex> lk(g_streams_mu);
  g_streams.push_back(s);
  *out = reinterpret_cast<hipStream_t>(s);
  return hipSuccess;
}

hipError_t hipStreamDestroy(hipStream_t st) {
  Stream *s = as_stream(st, "hipStreamDestroy");
  if (!s) return hipErrorInvalidHandle;
  s->sync();
  {
    std::lock_guard<std::mutex> lk(s->mu);
    s->stop = true;
    s->cv.notify_all();
  }
  s->th.join();
  std::lock_guard<std::mutex> lk(g_streams_mu);
  s->dead = true;
  return hipSuccess;
}

hipError_t hipStreamQuery(hipStream_t st) {
  Stream *s = as_stream(st, "hipStreamQuery");
  if (!s) return hipErrorInvalidHandle;
  std::lock_guard<std::mutex> lk(s->mu);
  return s->done == s->enq ? hipSuccess : hipErrorNotReady;
}

hipError_t hipStreamSynchronize(hipStream_t st) {
  Stream *s = as_stream(st, "hipStreamSynchronize");
  if (!s) return hipErrorInvalidHandle;
  s->sync();
  return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *out, unsigned int) {
  read_schedule();
  if (!out) return hipErrorInvalidValue;
  Event *e = new Event();
  e->dev = t_dev;
  std::lock_guard<std::mutex> lk(g_streams_mu);
  g_events.insert(e);
  *out = reinterpret_cast<hipEvent_t>(e);
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *out) { return hipEventCreateWithFlags(out, 0); }

hipError_t hipEventDestroy(hipEvent_t ev) {
  Event *e = as_event(ev, "hipEventDestroy");
  if (!e) return hipErrorInvalidHandle;
  {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    g_events.erase(e);
  }
  delete e;  // (a pending record or wait holds its marker, not the event)
  return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) {
  Event *e = as_event(ev, "hipEventRecord");
  Stream *s = as_stream(st, "hipEventRecord");
  if (!e || !s) return hipErrorInvalidHandle;
  if (e->dev != s->dev) {
    finding("hipEventRecord: the event was created on device %d, the stream on device %d", e->dev, s->dev);
    return t_last = hipErrorInvalidHandle;
  }
  auto m = std::make_shared<Marker>();
  m->owner = s;
  {
    std::lock_guard<std::mutex> lk(e->mu);
    e->last = m;
  }
  s->push("event record", {}, [m] {
    std::lock_guard<std::mutex> lk(g_mk_mu);
    m->when = Clock::now();
    m->done.store(true);
    g_mk_cv.notify_all();
  }, &m->seq);
  return hipSuccess;
}

static std::shared_ptr<Marker> marker_of(Event *e) {
  std::lock_guard<std::mutex> lk(e->mu);
  return e->last;
}

static void wait_marker(const std::shared_ptr<Marker> &m) {
  if (m->done.load()) return;
  // the record's sequence number is set right after its push: read it under the owner's lock
  uint64_t seq;
  {
    std::lock_guard<std::mutex> lk(m->owner->mu);
    seq = m->seq ? m->seq : m->owner->enq;
  }
  m->owner->kick(seq);
  std::unique_lock<std::mutex> lk(g_mk_mu);
  g_mk_cv.wait(lk, [&] { return m->done.load(); });
}

hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned int) {
  Event *e = as_event(ev, "hipStreamWaitEvent");
  Stream *s = as_stream(st, "hipStreamWaitEvent");
  if (!e || !s) return hipErrorInvalidHandle;
  std::shared_ptr<Marker> m = marker_of(e);  // the record as of now; never recorded: nothing to wait for
  if (!m) return hipSuccess;
  s->push("event wait", {}, [m] { wait_marker(m); });
  return hipSuccess;
}

hipError_t hipEventQuery(hipEvent_t ev) {
  Event *e = as_event(ev, "hipEventQuery");
  if (!e) return hipErrorInvalidHandle;
  std::shared_ptr<Marker> m = marker_of(e);
  return !m || m->done.load() ? hipSuccess : hipErrorNotReady;
}

hipError_t hipEventSynchronize(hipEvent_t ev) {
  Event *e = as_event(ev, "hipEventSynchronize");
  if (!e) return hipErrorInvalidHandle;
  std::shared_ptr<Marker> m = marker_of(e);
  if (m) wait_marker(m);
  return hipSuccess;
}

hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
  Event *ea = as_event(a, "hipEventElapsedTime"), *eb = as_event(b, "hipEventElapsedTime");
  if (!ms || !ea || !eb) return hipErrorInvalidHandle;
  std::shared_ptr<Marker> ma = marker_of(ea), mb = marker_of(eb);
  if (!ma || !mb) return hipErrorInvalidHandle;
  if (!ma->done.load() || !mb->done.load()) return hipErrorNotReady;
  std::lock_guard<std::mutex> lk(g_mk_mu);
  *ms = std::chrono::duration<float, std::milli>(mb->when - ma->when).count();
  return hipSuccess;
}

// Copies.  Memory in the registry (device, pinned, registered) is read and
// written when the copy executes.  A host side that is not -- pageable memory
// -- makes the copy synchronous for the caller, as the real runtime stages it:
// a source is snapshot at the call, a destination is written before it returns.
static hipError_t copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows,
                            hipMemcpyKind kind, hipStream_t st, const char *name) {
  read_schedule();
  Stream *s = as_stream(st, name);
  if (!s) return hipErrorInvalidHandle;
  if (!width || !rows) return hipSuccess;
  bool src_reg, dst_reg;
  {
    std::shared_lock<std::shared_mutex> lk(g_mem);
    src_reg = find_alloc(src) != nullptr;
    dst_reg = find_alloc(dst) != nullptr;
  }
  const bool src_dev = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
  const bool dst_dev = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice;
  auto seen = std::make_shared<std::set<std::string>>();
  std::shared_ptr<std::vector<uint8_t>> snap;
  if (!src_reg && !src_dev) {  // pageable source: staged now
    snap = std::make_shared<std::vector<uint8_t>>(width * rows);
    for (size_t r = 0; r < rows; r++) memcpy(snap->data() + r * width, (const char *)src + r * spitch, width);
  }
  if (rows == 1 && kind == hipMemcpyHostToDevice && src_reg && dst_reg) {
    forget_uploads((uintptr_t)dst, (uintptr_t)dst + width, false);
    std::lock_guard<std::mutex> lk(g_up_mu);
    g_uploads[(uintptr_t)dst] = Upload{(uintptr_t)dst + width, (uintptr_t)src};
  }
  const int dev = s->dev;
  auto body = [=](Ctx &c) {
    bool ok = true;
    for (size_t r = 0; r < rows; r++) {
      if (src_reg || src_dev) ok &= c.need((const char *)src + r * spitch, width, "copy source", (long)r);
      if (dst_reg || dst_dev) ok &= c.need((char *)dst + r * dpitch, width, "copy destination", (long)r);
    }
    return ok;
  };
  std::vector<Range> ranges;
  {
    std::shared_lock<std::shared_mutex> lk(g_mem);
    Ctx c{name, dev, &ranges, seen.get()};
    body(c);
  }
  s->push(name, std::move(ranges), [=] {
    std::shared_lock<std::shared_mutex> lk(g_mem);
    Ctx c{name, dev, nullptr, seen.get()};
    if (!body(c)) return;
    for (size_t r = 0; r < rows; r++)
      memcpy((char *)dst + r * dpitch, snap ? (const char *)snap->data() + r * width : (const char *)src + r * spitch,
             width);
  });
  if (!dst_reg && !dst_dev) s->sync();  // pageable destination: the call returns with the bytes in place
  return hipSuccess;
}

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t st) {
  return copy_rows(dst, n, src, n, n, 1, kind, st, "hipMemcpyAsync");
}

hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                            hipMemcpyKind kind, hipStream_t st) {
  return copy_rows(dst, dpitch, src, spitch, width, height, kind, st, "hipMemcpy2DAsync");
}

hipError_t hipMemsetAsync(void *dst, int value, size_t n, hipStream_t st) {
  return launch(st, "hipMemsetAsync", [=](Ctx &c, bool exec) {
    if (c.need(dst, n, "memset destination") && exec) memset(dst, value, n);
  }, false);
}

// ---- the driver's side (hipdouble.h) ---------------------------------------
long hipdouble_findings(void) { return g_findings.load(); }
long hipdouble_ops(void) { return g_ops.load(); }
int hipdouble_bump_counter(long delta) {
  unsigned long long *c = g_last_ctr.load();
  if (!c) return -1;
  drain_all();
  std::shared_lock<std::shared_mutex> lk(g_mem);
  if (!find_alloc(c)) return -1;
  __atomic_fetch_add(c, (unsigned long long)delta, __ATOMIC_RELAXED);
  return 0;
}

}  // extern "C"
