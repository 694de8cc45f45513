// Proves the CPU stand-in for the device (tests/native/hipdouble/): the
// engine's public entry points are driven with one seeded mistake per run,
// and the stand-in must answer with exactly that mistake's finding -- or, for
// the deferred copy, with the bytes that show the schedule really defers.
// Where the engine accepts the mistake, a correct batch follows on the same
// queue and must come out right with no further finding.
//
//   hipdouble_selftest <case>
//     src_past        a source whose len runs one byte past its allocation
//     dst_past        a destination that ends one byte past its allocation
//     cross_device    a buffer of device 1 folded on a queue of device 0
//     free_pending    a buffer freed with hipFree itself while a launch that
//                     reads it is pending (lazy)
//     free_pending_uploaded  the same with the launch's tables uploaded, not read
//                     in place: the launch is known to read the buffer before
//                     its tables have reached the device
//     pinned_rewrite  a pinned buffer rewritten between bcp_h2d_async and the
//                     copy's execution (lazy): the device gets the new bytes
//     counter_bump    the work-queue counter bumped by one between two launches
// Prints "selftest <case>: findings=N want=M ... OK" and exits 0, or FAILED / 1.
#include <hip/hip_runtime_api.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bcp.h"
#include "hipdouble/hipdouble.h"

static int fails = 0;
#define MUST(expr)                                                         \
  do {                                                                     \
    const int rc_ = (expr);                                                \
    if (rc_) {                                                             \
      fprintf(stderr, "selftest: %s = %d (%s)\n", #expr, rc_, bcp_strerror(rc_)); \
      exit(2);                                                             \
    }                                                                      \
  } while (0)

struct Dev {
  bcp_engine *eng = nullptr;
  bcp_queue *q = nullptr;
  explicit Dev(int device) {
    MUST(bcp_engine_create(device, &eng));
    MUST(bcp_queue_create(eng, &q));
  }
  std::vector<void *> owned;
  ~Dev() {
    bcp_queue_sync(q);
    for (void *p : owned) bcp_dev_free(eng, p);
    bcp_queue_destroy(q);
    bcp_engine_destroy(eng);
  }
  uint8_t *alloc(size_t n) {
    void *p = nullptr;
    MUST(bcp_dev_alloc(eng, n, &p));
    owned.push_back(p);
    return (uint8_t *)p;
  }
  void forget(void *p) {
    for (void *&o : owned)
      if (o == p) o = nullptr;
  }
  void upload(uint8_t *d, const std::vector<uint8_t> &h) {
    MUST(bcp_h2d_async(q, d, h.data(), h.size()));  // pageable source: staged at the call
  }
  std::vector<uint8_t> download(const uint8_t *d, size_t n) {
    std::vector<uint8_t> h(n);
    MUST(bcp_d2h_async(q, h.data(), d, n));
    MUST(bcp_queue_sync(q));
    return h;
  }
};

static std::vector<uint8_t> pattern(size_t n, unsigned seed) {
  std::vector<uint8_t> v(n);
  unsigned x = seed * 2654435761u + 1;
  for (size_t i = 0; i < n; i++) {
    x = x * 1664525u + 1013904223u;
    v[i] = (uint8_t)(x >> 24);
  }
  return v;
}

// dst = a ^ b over n bytes on d.q; sources and dst as given (lengths may lie).
static int fold2(Dev &d, uint8_t *dst, uint64_t out_len, const uint8_t *a, uint64_t la, const uint8_t *b, uint64_t lb) {
  const bcp_stripe st = {(uint64_t)dst, out_len, 0, 2, 0};
  const bcp_source so[2] = {{(uint64_t)a, la}, {(uint64_t)b, lb}};
  return bcp_xor_stripes_async(d.q, &st, 1, so, 2);
}

// A correct batch on the same queue: right bytes, and it adds no finding.
static void clean_batch(Dev &d) {
  const size_t n = 5000;
  const long before = hipdouble_findings();
  uint8_t *a = d.alloc(n), *b = d.alloc(n), *o = d.alloc(n);
  const std::vector<uint8_t> ha = pattern(n, 11), hb = pattern(n, 12);
  d.upload(a, ha);
  d.upload(b, hb);
  MUST(fold2(d, o, n, a, n, b, n - 7));
  const std::vector<uint8_t> got = d.download(o, n);
  for (size_t j = 0; j < n; j++)
    if (got[j] != (uint8_t)(ha[j] ^ (j < n - 7 ? hb[j] : 0))) {
      fprintf(stderr, "selftest: the clean batch is wrong at byte %zu\n", j);
      fails++;
      break;
    }
  if (hipdouble_findings() != before) {
    fprintf(stderr, "selftest: the clean batch made %ld findings\n", hipdouble_findings() - before);
    fails++;
  }
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <case>\n", argv[0]);
    return 2;
  }
  const char *c = argv[1];
  const bool lazy = !strncmp(c, "free_pending", 12) || !strcmp(c, "pinned_rewrite");
  setenv("HIPDOUBLE_SCHEDULE", lazy ? "lazy" : "eager", 1);
  if (lazy) setenv("HIPDOUBLE_LAZY_US", "300000", 1);  // nothing runs by timer while the mistake is made
  long want = 1;
  {
    Dev d(0);
    const size_t n = 4096;  // a whole allocation
    if (!strcmp(c, "src_past")) {
      uint8_t *a = d.alloc(n), *b = d.alloc(2 * n), *o = d.alloc(2 * n);
      d.upload(a, pattern(n, 1));
      d.upload(b, pattern(2 * n, 2));
      MUST(fold2(d, o, n + 1, a, n + 1, b, n + 1));
      MUST(bcp_queue_sync(d.q));
      clean_batch(d);
    } else if (!strcmp(c, "dst_past")) {
      uint8_t *a = d.alloc(2 * n), *b = d.alloc(2 * n), *o = d.alloc(n);
      d.upload(a, pattern(2 * n, 1));
      d.upload(b, pattern(2 * n, 2));
      MUST(fold2(d, o, n + 1, a, n + 1, b, n + 1));
      MUST(bcp_queue_sync(d.q));
      clean_batch(d);
    } else if (!strcmp(c, "cross_device")) {
      Dev other(1);
      uint8_t *a = other.alloc(n), *b = d.alloc(n), *o = d.alloc(n);
      other.upload(a, pattern(n, 1));
      MUST(bcp_queue_sync(other.q));
      d.upload(b, pattern(n, 2));
      MUST(fold2(d, o, n, a, n, b, n));
      MUST(bcp_queue_sync(d.q));
      clean_batch(d);
      clean_batch(other);
    } else if (!strncmp(c, "free_pending", 12)) {
      if (strcmp(c, "free_pending")) MUST(bcp_set_option(d.eng, "table_host_max", 0));
      uint8_t *a = d.alloc(n), *b = d.alloc(n), *o = d.alloc(n);
      d.upload(a, pattern(n, 1));
      d.upload(b, pattern(n, 2));
      MUST(bcp_queue_sync(d.q));         // the uploads are done: only the launch will refer to a
      MUST(fold2(d, o, n, a, n, b, n));  // pending: nobody blocks on it yet
      if (hipFree(a) != hipSuccess) fails++;  // not bcp_dev_free: the runtime's own entry point
      d.forget(a);
      MUST(bcp_queue_sync(d.q));
      clean_batch(d);
    } else if (!strcmp(c, "pinned_rewrite")) {
      want = 0;
      void *h = nullptr;
      MUST(bcp_host_alloc(d.eng, n, &h));
      uint8_t *dv = d.alloc(n);
      const std::vector<uint8_t> first = pattern(n, 1), second = pattern(n, 2);
      memcpy(h, first.data(), n);
      MUST(bcp_h2d_async(d.q, dv, h, n));
      memcpy(h, second.data(), n);  // the mistake: the copy has not run yet
      const std::vector<uint8_t> got = d.download(dv, n);
      if (got == first) {
        fprintf(stderr, "selftest: the device has the bytes as enqueued: the lazy schedule did not defer the copy\n");
        fails++;
      } else if (got != second) {
        fprintf(stderr, "selftest: the device has neither the first nor the second pattern\n");
        fails++;
      }
      MUST(bcp_host_free(d.eng, h));
      clean_batch(d);
    } else if (!strcmp(c, "counter_bump")) {
      clean_batch(d);  // a launch: the stand-in now knows the queue's counter
      if (hipdouble_findings() != 0 || hipdouble_bump_counter(1) != 0) fails++;
      uint8_t *a = d.alloc(n), *b = d.alloc(n), *o = d.alloc(n);
      d.upload(a, pattern(n, 1));
      d.upload(b, pattern(n, 2));
      MUST(fold2(d, o, n, a, n, b, n));
      MUST(bcp_queue_sync(d.q));
      clean_batch(d);
    } else {
      fprintf(stderr, "selftest: unknown case '%s'\n", c);
      return 2;
    }
  }
  const long got = hipdouble_findings();
  if (got != want) fails++;
  printf("selftest %s: findings=%ld want=%ld %s\n", c, got, want, fails ? "FAILED" : "OK");
  return fails ? 1 : 0;
}
