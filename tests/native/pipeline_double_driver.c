/* The batched pipeline on the CPU stand-in for the device
 * (tests/native/hipdouble/, tools/hipdouble_pipeline.sh,
 * tests/test_hipdouble_cpu.py): loopback stores, the pipeline's run, rebuild
 * and verify_q paths, and every parity file, Q file, verdict and rebuilt chunk
 * checked against a CPU computation written here (XOR and window replay by
 * windows, Q in Horner form with a shift-and-reduce doubling: nothing shared
 * with the library or the stand-in).  No device is touched; the schedule of
 * the stand-in's streams comes from HIPDOUBLE_SCHEDULE.
 *
 *   pipeline_double_driver <a|b|c|d> <root>
 *
 *  a  9 targets, 60 files of 2..8 holders, chunks of 1 byte .. 1 MiB; slabs of
 *     4 MiB, 2 io threads, 2 slots; COPY and DIRECT; gen, then target 3 lost
 *     and rebuilt
 *  b  16 targets, 26 files of width 1..15 (64 KiB .. 3 MiB, odd lengths, one
 *     chunk missing at generation time) and two past the window; gen with Q;
 *     slabs of 1 MiB, 4 io threads, 2 slots, 2 devices; four chunks flipped,
 *     bcp_pipeline_verify_q: the verdicts land on those four items
 *  c  one pipeline run three times over stores whose largest item and whose
 *     batches' descriptor tables and tile counts grow (4 slots, launches
 *     slowed, so batches overlap on the device): the slots are freed and
 *     reallocated between runs, the engine's ring slots and tile records grow
 *     while earlier batches are still on the queue
 *  d  an item above the 10 MiB window, with P only and with Q over the
 *     replayed streams (bcp_pipeline_set_q_windowed), then scrubbed */
#define _GNU_SOURCE
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "bcp_task.h"
#include "hipdouble/hipdouble.h"

#define MAXT 16
#define KiB 1024u
#define MiB (1024u * 1024u)
#define WINDOW ((uint64_t)BCP_WINDOW_BYTES)

typedef struct {
    char name[64];
    uint64_t loc;            /* holders | P << 56 */
    int p, q;                /* parity target, Q target (-1: none) */
    int n;                   /* holders */
    int holder[MAXT];        /* ascending */
    size_t len[MAXT];        /* by position */
    uint8_t *data[MAXT];
} file_t;

static const char *root;
static int NT;
static file_t *files;
static bcp_work_item *items;
static int nfiles;
static int bad;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

/* The driver's own byte loops (chunk contents, expected bodies) are not code
 * under test: uninstrumented, so a sanitizer build spends its time in the
 * library. */
#define PLAIN __attribute__((no_sanitize("address", "thread"), noinline))

PLAIN static void fill_random(uint8_t *d, size_t n)
{
    size_t j = 0;
    for (; j + 8 <= n; j += 8) {
        const uint64_t r = rnd();
        memcpy(d + j, &r, 8);
    }
    for (uint64_t r = rnd(); j < n; j++, r >>= 8)
        d[j] = (uint8_t)r;
}

static void mkdirs(const char *p)
{
    char tmp[640];
    snprintf(tmp, sizeof tmp, "%s", p);
    for (char *s = tmp + 1; *s; s++)
        if (*s == '/') {
            *s = 0;
            mkdir(tmp, 0755);
            *s = '/';
        }
    mkdir(tmp, 0755);
}

static void write_file(const char *path, const uint8_t *d, size_t n)
{
    char dir[640];
    snprintf(dir, sizeof dir, "%s", path);
    *strrchr(dir, '/') = 0;
    mkdirs(dir);
    int fd = open(path, O_CREAT | O_WRONLY | O_TRUNC, 0644);
    if (fd < 0) {
        perror(path);
        exit(2);
    }
    for (size_t off = 0; off < n;) {
        ssize_t w = write(fd, d + off, n - off);
        if (w <= 0) {
            perror(path);
            exit(2);
        }
        off += (size_t)w;
    }
    close(fd);
}

static uint8_t *read_file(const char *path, size_t *n)
{
    int fd = open(path, O_RDONLY);
    *n = 0;
    if (fd < 0)
        return NULL;
    struct stat sb;
    fstat(fd, &sb);
    uint8_t *b = malloc((size_t)sb.st_size + 1);
    size_t got = 0;
    while (got < (size_t)sb.st_size) {
        ssize_t r = read(fd, b + got, (size_t)sb.st_size - got);
        if (r <= 0)
            break;
        got += (size_t)r;
    }
    close(fd);
    *n = got;
    return b;
}

static void problem(const char *what, const char *name)
{
    fprintf(stderr, "MISMATCH: %s: %s\n", what, name);
    bad++;
}

/* The rule of bcp_q_target, restated: the first of P+1, P+2, ... that is
 * neither a holder nor P. */
static int q_target_of(uint64_t holders, int p)
{
    for (int i = 1; i < NT; i++) {
        const int t = (p + i) % NT;
        if (!(holders >> t & 1))
            return t;
    }
    return -1;
}

/* A store of nf files: holder sets and lengths from the caller's arrays. */
static void store_begin(int nt, int nf)
{
    NT = nt;
    nfiles = 0;
    files = calloc((size_t)nf, sizeof *files);
    items = calloc((size_t)nf, sizeof *items);
    char path[640];
    for (int t = 0; t < NT; t++) {
        snprintf(path, sizeof path, "%s/st%d/parity", root, t);
        mkdirs(path);
        snprintf(path, sizeof path, "%s/st%d/parityq", root, t);
        mkdirs(path);
        snprintf(path, sizeof path, "%s/st%d/chunks", root, t);
        mkdirs(path);
    }
}

static void store_free(void)
{
    for (int i = 0; i < nfiles; i++)
        for (int k = 0; k < files[i].n; k++)
            free(files[i].data[k]);
    free(files);
    free(items);
    files = NULL;
    items = NULL;
}

static char *chunk_path(char *buf, size_t cap, const file_t *f, int k)
{
    snprintf(buf, cap, "%s/st%d/chunks/%s", root, f->holder[k], f->name);
    return buf;
}

/* holders: bit set; lens in ascending holder order */
static file_t *store_add(const char *name, uint64_t holders, int p, const size_t *lens)
{
    file_t *f = &files[nfiles];
    char path[640];
    snprintf(f->name, sizeof f->name, "%s", name);
    f->p = p;
    f->loc = holders | ((uint64_t)p << 56);
    f->q = q_target_of(holders, p);
    for (int t = 0; t < NT; t++)
        if (holders >> t & 1) {
            const int k = f->n++;
            f->holder[k] = t;
            f->len[k] = lens[k];
            f->data[k] = malloc(lens[k] + 1);
            fill_random(f->data[k], lens[k]);
            write_file(chunk_path(path, sizeof path, f, k), f->data[k], lens[k]);
        }
    items[nfiles].path = f->name;
    items[nfiles].fi.timestamp = 1LL << 40;
    items[nfiles].fi.locations = f->loc;
    nfiles++;
    return f;
}

/* ---- the expected bodies ------------------------------------------------ */
static size_t max_len(const file_t *f)
{
    size_t m = 0;
    for (int k = 0; k < f->n; k++)
        m = f->len[k] > m ? f->len[k] : m;
    return m;
}

/* The stream of member k over [0, n): its chunk window by window; past its
 * last readable window that window again (the sender never refills its buffer
 * after the end of the file), zeros where the chunk has no byte.  n at most
 * one window: the chunk zero padded. */
static uint8_t *stream_of(const file_t *f, int k, size_t n)
{
    uint8_t *r = calloc(n + 1, 1);
    const size_t len = f->len[k];
    if (!len)
        return r;
    if (n <= WINDOW) {
        memcpy(r, f->data[k], len < n ? len : n);
        return r;
    }
    const size_t last = (len - 1) / WINDOW; /* its last readable window */
    for (size_t w = 0; w * WINDOW < n; w++) {
        const size_t from = (w <= last ? w : last) * WINDOW;
        size_t have = len - from < WINDOW ? len - from : WINDOW;
        if (w * WINDOW + have > n)
            have = n - w * WINDOW;
        memcpy(r + w * WINDOW, f->data[k] + from, have);
    }
    return r;
}

/* p ^= r and q = 2q ^ r over n bytes: doubling is times g = 2, reduced by
 * x^8+x^4+x^3+x^2+1 */
PLAIN static void horner_step(uint8_t *p, uint8_t *q, const uint8_t *r, size_t n)
{
    for (size_t j = 0; j < n; j++) {
        p[j] ^= r[j];
        q[j] = (uint8_t)((uint8_t)(q[j] << 1) ^ (q[j] & 0x80 ? 0x1d : 0) ^ r[j]);
    }
}

/* P and Q bodies over the members' streams (Q in Horner form: q = 2q ^ D_k
 * from the last position down). */
static void bodies_of(const file_t *f, uint8_t **p_out, uint8_t **q_out)
{
    const size_t n = max_len(f);
    uint8_t *p = calloc(n + 1, 1), *q = calloc(n + 1, 1);
    for (int k = f->n - 1; k >= 0; k--) {
        uint8_t *r = stream_of(f, k, n);
        horner_step(p, q, r, n);
        free(r);
    }
    *p_out = p;
    *q_out = q;
}

/* A parity file: u64 sizes in ascending holder order, then the body. */
static void check_parity_file(const file_t *f, const char *dir, int target, const uint8_t *body, const char *what)
{
    char path[640];
    const size_t n = max_len(f), hdr = 8 * (size_t)f->n;
    snprintf(path, sizeof path, "%s/st%d/%s/%s", root, target, dir, f->name);
    size_t got_n = 0;
    uint8_t *got = read_file(path, &got_n);
    int ok = got && got_n == hdr + n;
    for (int k = 0; ok && k < f->n; k++) {
        uint64_t h;
        memcpy(&h, got + 8 * k, 8);
        ok = h == (uint64_t)f->len[k];
    }
    if (ok && memcmp(got + hdr, body, n)) {
        size_t j = 0;
        while (got[hdr + j] == body[j])
            j++;
        fprintf(stderr, "  first wrong byte at %zu of %zu\n", j, n);
        ok = 0;
    }
    if (!ok) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s, %s file of target %d (%zu bytes, expected %zu)", what, dir, target, got_n,
                 hdr + n);
        problem(msg, f->name);
    }
    free(got);
}

/* q_mode: 0 no Q file may exist, 1 Q for the items inside the window, 2 Q for all */
static void check_parity(const char *what, int q_mode)
{
    char path[640];
    for (int i = 0; i < nfiles; i++) {
        const file_t *f = &files[i];
        uint8_t *p, *q;
        bodies_of(f, &p, &q);
        check_parity_file(f, "parity", f->p, p, what);
        const int has_q = f->q >= 0 && (q_mode == 2 || (q_mode == 1 && max_len(f) <= WINDOW));
        if (has_q) {
            check_parity_file(f, "parityq", f->q, q, what);
        } else if (f->q >= 0) {
            snprintf(path, sizeof path, "%s/st%d/parityq/%s", root, f->q, f->name);
            if (access(path, F_OK) == 0)
                problem("a Q file that should not exist", f->name);
        }
        free(p);
        free(q);
    }
}

static void lose_target(int victim)
{
    char path[640];
    for (int i = 0; i < nfiles; i++)
        for (int k = 0; k < files[i].n; k++)
            if (files[i].holder[k] == victim)
                unlink(chunk_path(path, sizeof path, &files[i], k));
}

static void check_target(int victim, const char *what)
{
    char path[640];
    for (int i = 0; i < nfiles; i++)
        for (int k = 0; k < files[i].n; k++)
            if (files[i].holder[k] == victim) {
                size_t got_n = 0;
                uint8_t *got = read_file(chunk_path(path, sizeof path, &files[i], k), &got_n);
                if (!got || got_n != files[i].len[k] || memcmp(got, files[i].data[k], got_n))
                    problem(what, files[i].name);
                free(got);
            }
}

static void must(int rc, int errors, const char *what)
{
    if (rc || errors) {
        fprintf(stderr, "FAILED: %s: rc=%d (%s) errors=%d\n", what, rc, bcp_strerror(rc), errors);
        printf("FAILED: %s\n", what);
        fprintf(stderr, "hipdouble: %ld findings\n", hipdouble_findings());
        exit(1);
    }
}

static size_t log_uniform(size_t lo, size_t hi)
{
    /* lo * 2^u, u uniform over the octaves between lo and hi */
    double o = 0;
    for (size_t x = lo; x < hi; x *= 2)
        o += 1;
    const double u = (double)(rnd() % 100000) / 100000.0 * o;
    double v = (double)lo;
    for (int i = 0; i < (int)u; i++)
        v *= 2;
    v *= 1.0 + (u - (int)u);
    return v > (double)hi ? hi : (size_t)v;
}

/* w distinct targets of nt, as a bit set */
static uint64_t pick_targets(int nt, int w)
{
    uint64_t s = 0;
    while (w > 0) {
        const int t = (int)(rnd() % (uint64_t)nt);
        if (!(s >> t & 1)) {
            s |= 1ull << t;
            w--;
        }
    }
    return s;
}

static int pick_p(int nt, uint64_t holders)
{
    for (;;) {
        const int t = (int)(rnd() % (uint64_t)nt);
        if (!(holders >> t & 1))
            return t;
    }
}

/* ---- a ------------------------------------------------------------------ */
static int by_path(const void *x, const void *y)
{
    return strcmp(((const bcp_work_item *)x)->path, ((const bcp_work_item *)y)->path);
}

static void scenario_a(void)
{
    enum { VICTIM = 3 };
    store_begin(9, 60);
    for (int i = 0; i < 60; i++) {
        char name[64];
        size_t lens[MAXT];
        const int w = 2 + (int)(rnd() % 7); /* 2..8 holders */
        const uint64_t h = pick_targets(9, w);
        for (int k = 0; k < w; k++) {
            lens[k] = log_uniform(1, MiB);
            if (rnd() % 8 == 0)
                lens[k] = MiB - rnd() % 3; /* the top of the range is reached */
        }
        snprintf(name, sizeof name, "m%d/chunk%d", i % 5, i);
        store_add(name, h, pick_p(9, h), lens);
    }
    const int modes[2] = {BCP_READ_COPY, BCP_READ_DIRECT};
    for (int m = 0; m < 2; m++) {
        bcp_pipeline_opts o = {0, (size_t)4 << 20, 2, 2, 1, modes[m]};
        bcp_pipeline *pl = NULL;
        bcp_run_stats st;
        char what[64];
        must(bcp_pipeline_create(&o, &pl), 0, "pipeline_create");
        snprintf(what, sizeof what, "a: gen, read mode %d", modes[m]);
        must(bcp_pipeline_run(pl, root, NT, items, (size_t)nfiles, NULL, &st), st.errors, what);
        check_parity(what, 0);
        lose_target(VICTIM);
        snprintf(what, sizeof what, "a: rebuild of target %d, read mode %d", VICTIM, modes[m]);
        /* the rebuild takes the items as a DB scan gives them, in key order */
        bcp_work_item *sorted = malloc((size_t)nfiles * sizeof *sorted);
        memcpy(sorted, items, (size_t)nfiles * sizeof *sorted);
        qsort(sorted, (size_t)nfiles, sizeof *sorted, by_path);
        must(bcp_pipeline_rebuild(pl, root, NT, VICTIM, sorted, (size_t)nfiles, NULL, NULL, &st), st.errors, what);
        free(sorted);
        check_target(VICTIM, what);
        bcp_pipeline_destroy(pl);
    }
    store_free();
}

/* ---- b ------------------------------------------------------------------ */
static void flip(const file_t *f, int k, size_t off)
{
    char path[640];
    struct stat sb;
    chunk_path(path, sizeof path, f, k);
    int fd = open(path, O_RDWR);
    uint8_t b;
    if (fd < 0 || fstat(fd, &sb) || pread(fd, &b, 1, (off_t)off) != 1) {
        perror(path);
        exit(2);
    }
    b ^= 0x5A;
    if (pwrite(fd, &b, 1, (off_t)off) != 1) {
        perror(path);
        exit(2);
    }
    const struct timespec tv[2] = {sb.st_atim, sb.st_mtim}; /* the scrub takes a newer chunk for a stale item */
    futimens(fd, tv);
    close(fd);
}

static void scenario_b(void)
{
    store_begin(16, 28);
    for (int i = 0; i < 26; i++) {
        char name[64];
        size_t lens[MAXT];
        const int w = i % 15 + 1;
        const uint64_t h = pick_targets(16, w);
        for (int k = 0; k < w; k++)
            lens[k] = log_uniform(64 * KiB, w <= 4 ? 3 * MiB : 400 * KiB) | 1;
        if (i == 5)
            lens[1] = 0; /* width 6: its second holder's chunk never existed */
        snprintf(name, sizeof name, "v/%d/c%02d", i % 5, i);
        file_t *f = store_add(name, h, pick_p(16, h), lens);
        if (i == 5) {
            char path[640];
            unlink(chunk_path(path, sizeof path, f, 1));
        }
    }
    const size_t big_a[2] = {10485760, 26214405}, big_b[3] = {11 * MiB + 3, 70 * KiB + 1, 12 * MiB + 5};
    store_add("big/a", 1ull << 0 | 1ull << 1, 4, big_a);
    store_add("big/b", 1ull << 1 | 1ull << 2 | 1ull << 3, 0, big_b);

    bcp_pipeline_opts o = {0, (size_t)1 << 20, 4, 2, 2, BCP_READ_COPY};
    bcp_pipeline *pl = NULL;
    bcp_run_stats st;
    must(bcp_pipeline_create(&o, &pl), 0, "pipeline_create");
    bcp_pipeline_set_q_parity(pl, 1);
    must(bcp_pipeline_run(pl, root, NT, items, (size_t)nfiles, NULL, &st), st.errors, "b: gen with Q");
    bcp_pipeline_set_q_parity(pl, 0);
    check_parity("b: gen with Q", 1);

    const int picks[4] = {0, 14, 20, nfiles - 1};
    for (int j = 0; j < 4; j++)
        flip(&files[picks[j]], 0, 4097 + (size_t)picks[j]);
    bcp_verify_q_item *res = calloc((size_t)nfiles, sizeof *res);
    bcp_verify_q_stats vs;
    bcp_pipeline_timing tm;
    must(bcp_pipeline_verify_q(pl, root, NT, items, (size_t)nfiles, res, NULL, NULL, NULL, &vs), vs.v.errors,
         "b: verify_q");
    bcp_pipeline_last_timing(pl, &tm);
    if (tm.batches < 4)
        problem("b: fewer than 4 batches", "verify_q");
    for (int i = 0; i < nfiles; i++) {
        const file_t *f = &files[i];
        int picked = 0;
        for (int j = 0; j < 4; j++)
            picked |= picks[j] == i;
        const int has_q = f->q >= 0 && max_len(f) <= WINDOW;
        const bcp_verify_q_item *r = &res[i];
        int ok = r->q_state == (uint32_t)(has_q ? BCP_QSTATE_CHECKED : BCP_QSTATE_NONE);
        if (!picked) {
            ok = ok && r->status == BCP_VERIFY_OK;
        } else {
            ok = ok && r->status == BCP_VERIFY_MISMATCH && r->first_bad == 4097 + (uint64_t)i;
            if (has_q)
                ok = ok && r->culprit == BCP_CULPRIT_DATA && r->target == f->holder[0] && r->p_bad == 1 && r->q_bad == 1;
            else
                ok = ok && r->culprit == BCP_CULPRIT_MANY && r->target == -1 && r->q_bad == 0;
        }
        if (!ok) {
            fprintf(stderr, "  status %u q_state %u culprit %u target %d first_bad %llu p_bad %llu q_bad %llu\n", r->status,
                    r->q_state, r->culprit, r->target, (unsigned long long)r->first_bad, (unsigned long long)r->p_bad,
                    (unsigned long long)r->q_bad);
            problem(picked ? "b: verdict of a flipped item" : "b: verdict of an untouched item", f->name);
        }
    }
    if (vs.v.mismatch != 4 || vs.v.ok != (uint64_t)nfiles - 4 || vs.culprit_data != 2 || vs.culprit_many != 2)
        problem("b: counts", "verify_q");
    free(res);
    bcp_pipeline_destroy(pl);
    store_free();
}

/* ---- c ------------------------------------------------------------------ */
static void scenario_c(void)
{
    /* per run, in this order: the largest item, wide (the slabs grow to it, so
     * it is a batch of its own); a second wide item and medium ones that fill
     * the next batch's output slab (past 16 stripes: the batch goes through a
     * ring slot, and with the stand-in's launches slowed it is still on the
     * queue when the next batch comes); then many tiny items, one batch whose
     * descriptor tables outgrow the ring slots and, in the last run, whose
     * tiles outgrow the tile-record buffers */
    static const int ntiny[3] = {300, 1500, 4500};
    static const size_t large[3] = {100 * KiB, 600 * KiB, 1536 * KiB};
    const char *base = root;
    setenv("HIPDOUBLE_LAUNCH_US", "10000", 0);
    /* 4 slots: on one lane with 2, a batch is submitted only after the one
     * before it has been written, so no two are ever on the device together */
    bcp_pipeline_opts o = {0, (size_t)2 << 20, 2, 4, 1, BCP_READ_COPY};
    bcp_pipeline *pl = NULL;
    must(bcp_pipeline_create(&o, &pl), 0, "pipeline_create");
    for (int run = 0; run < 3; run++) {
        char sub[600], what[64], name[64];
        snprintf(sub, sizeof sub, "%s/run%d", base, run);
        root = sub;
        store_begin(9, ntiny[run] + 62);
        size_t lens[MAXT];
        for (int k = 0; k < 8; k++)
            lens[k] = large[run] - rnd() % 5000;
        store_add("large", 0xFF, 8, lens);
        for (int k = 0; k < 8; k++)
            lens[k] = 80 * KiB - rnd() % 5000;
        store_add("second", 0xFF, 8, lens);
        for (int i = 0; i < 60; i++) {
            lens[0] = 32 * KiB - rnd() % 1000;
            lens[1] = 16 * KiB + rnd() % 1000;
            snprintf(name, sizeof name, "med/%d", i);
            store_add(name, 1ull << (i % 4) | 1ull << 5, 6, lens);
        }
        for (int i = 0; i < ntiny[run]; i++) {
            lens[0] = 1 + rnd() % 64;
            snprintf(name, sizeof name, "t%d/%d", i % 7, i);
            store_add(name, 1ull << (i % 8), 8, lens);
        }
        bcp_run_stats st;
        snprintf(what, sizeof what, "c: run %d", run);
        must(bcp_pipeline_run(pl, root, NT, items, (size_t)nfiles, NULL, &st), st.errors, what);
        check_parity(what, 0);
        store_free();
    }
    root = base;
    bcp_pipeline_destroy(pl);
}

/* ---- d ------------------------------------------------------------------ */
static void scenario_d(void)
{
    store_begin(6, 8);
    size_t lens[MAXT];
    for (int i = 0; i < 6; i++) {
        char name[64];
        const int w = 1 + i % 4;
        const uint64_t h = pick_targets(5, w);
        for (int k = 0; k < w; k++)
            lens[k] = log_uniform(1, 512 * KiB);
        snprintf(name, sizeof name, "n/%d", i);
        store_add(name, h, 5, lens);
    }
    /* past the window: the longest member replays nothing, the first replays
     * its second window, the short one its only window */
    lens[0] = WINDOW + 70001;
    lens[1] = 300 * KiB + 1;
    lens[2] = 2 * WINDOW + 4097;
    store_add("big/w", 1ull << 0 | 1ull << 2 | 1ull << 3, 4, lens);
    for (int q = 0; q < 2; q++) {
        bcp_pipeline_opts o = {0, (size_t)4 << 20, 2, 2, 1, BCP_READ_COPY};
        bcp_pipeline *pl = NULL;
        bcp_run_stats st;
        must(bcp_pipeline_create(&o, &pl), 0, "pipeline_create");
        if (q) {
            bcp_pipeline_set_q_parity(pl, 1);
            bcp_pipeline_set_q_windowed(pl, 1);
        }
        const char *what = q ? "d: gen with Q over the window" : "d: gen, P only";
        must(bcp_pipeline_run(pl, root, NT, items, (size_t)nfiles, NULL, &st), st.errors, what);
        check_parity(what, q ? 2 : 0);
        if (q) {
            bcp_verify_q_item *res = calloc((size_t)nfiles, sizeof *res);
            bcp_verify_q_stats vs;
            must(bcp_pipeline_verify_q(pl, root, NT, items, (size_t)nfiles, res, NULL, NULL, NULL, &vs), vs.v.errors,
                 "d: verify_q");
            for (int i = 0; i < nfiles; i++)
                if (res[i].status != BCP_VERIFY_OK || res[i].q_state != BCP_QSTATE_CHECKED)
                    problem("d: verdict of a clean item", files[i].name);
            free(res);
        }
        bcp_pipeline_destroy(pl);
    }
    store_free();
}

int main(int argc, char **argv)
{
    if (argc < 3 || strlen(argv[1]) != 1 || !strchr("abcd", argv[1][0])) {
        fprintf(stderr, "usage: %s <a|b|c|d> <store root>\n", argv[0]);
        return 2;
    }
    root = argv[2];
    rng_state ^= (uint64_t)argv[1][0] * 0x100000001B3ull;
    switch (argv[1][0]) {
    case 'a': scenario_a(); break;
    case 'b': scenario_b(); break;
    case 'c': scenario_c(); break;
    default: scenario_d(); break;
    }
    bcp_task_shutdown();
    const long nf = hipdouble_findings();
    printf("hipdouble: %ld findings, %ld operations\n", nf, hipdouble_ops());
    printf("%s: %d problems\n", bad ? "FAILED" : "OK", bad);
    return bad || nf ? 1 : 0;
}
