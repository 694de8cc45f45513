/*
 * bcp_pipeline.c -- batched end-to-end parity generation on one node.
 *
 * The per-task protocol (bcp_task.c) moves one stripe per round trip; this
 * is the throughput form of the same computation for loopback stores, where
 * every chunk file is local: stripes are batched into pinned slabs and the
 * device does one descriptor-kernel launch per batch (SURVEY.md §7 "hard
 * parts": batching vs the per-task interface).
 *
 *   io pool (reads first)     chunk files -> pinned input slab   [slot s]
 *   h2d queue                 pinned -> device slab, event H
 *   compute queue             wait H, xor_desc over the batch, event K
 *   d2h queue                 wait K, parity bodies -> pinned output slab, event D
 *   io pool (the same)        wait D, parity files = u64 sizes[n] + body
 *
 * Slots are recycled round-robin, so batch b+1 is read while batch b is on
 * the device and batch b-1 is being written; H2D and D2H run on their own
 * queues beside the kernel (PCIe is full duplex).  With ndevices > 1 the
 * batches go round-robin to the node's GPUs (each with its own engine, queues
 * and slots; stripes are independent, so nothing crosses GPUs): PCIe, not the
 * kernel, bounds this path, and every GPU brings its own link.
 *
 * Output files are byte-identical to parity_generator's
 * (task_processing.c:146-226): header in ascending storage-target order, then
 * the windowed XOR (replay semantics past one 10 MiB window); a missing chunk
 * counts as size 0 / zeros; an item with no holders unlinks its parity chunk.
 *
 * Rebuild mode (bcp_pipeline_rebuild) is the same machinery with do_file's
 * roles (rebuild/main.c:40-89, task_processing.c:146-174,228-230,263-280):
 * the sources are the surviving chunks plus the parity body (read after the
 * u64 header), max_cs = max(header), and the lost chunk is written to the
 * victim's chunks directory truncated to header[index of the victim];
 * survivors newer than FileInfo.timestamp go to the corrupt list.
 *
 * Verify mode (bcp_pipeline_verify, the scrub) reads instead of writing: the
 * sources of an item are its chunks (lengths from the parity header) and, last,
 * the parity body; the device compares the fold of the chunks with the body
 * where it lies in the input slab (bcp_check_stripes_async), 16 bytes per item
 * come back in the output slab, and the completion stage turns them into
 * verdicts.  No write jobs, nothing under the store changes.  With Q
 * (bcp_pipeline_verify_q) an item whose Q file is in order gets one more
 * source row, the Q body, and its stripe goes in a launch of its own per batch
 * (bcp_pq_check_stripes_async): 32 bytes come back, the syndromes' verdict.
 * A repair run (bcp_pipeline_repair_q) is that run with one more stage in the
 * batch's completion, before the slot is released: the MISMATCH items the
 * policy admits go through bcp_pq_repair_stripes_async and a second check on
 * the slot's device slab, on a queue of the completion thread's own, and the
 * blocks that changed are patched into the files (repair_batch).  Items past
 * the window are admitted only under bcp_pipeline_set_repair_windowed; their
 * stripes carry the window and both calls are the _win entry points'.
 *
 * Q parity (bcp_pipeline_set_q_parity, bcp_pipeline_rebuild2; bcp_task.h): a
 * task may have a second output, placed after the first in the output slab
 * and written by a second write job -- the Q body of a gen task (file
 * <root>/st<q>/parityq/<path>, same header), or the second chunk of a rebuild
 * from P and Q.  Those tasks' stripes go in a launch of their own per batch
 * (bcp_pq_stripes_async / bcp_pq_recover_stripes_async, sources in holder
 * order) beside the batch's bcp_xor_stripes_async.  An item past the window
 * has no Q unless bcp_pipeline_set_q_windowed is on; then its stripe carries
 * the window and the launch is the _win entry point's (Q over the replayed
 * streams, the P body still the reference's).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <linux/magic.h>
#include <sys/mman.h>
#include <sys/vfs.h>
#include <sys/stat.h>
#include <sys/uio.h>
#include <time.h>
#include <unistd.h>

#include "bcp_host.h"
#include "bcp_runner.h"

#define ROW 256u
#define PAGE 4096u
#define WINDOW ((uint64_t)BCP_WINDOW_BYTES)
#define RUP(x) (((x) + ROW - 1) / ROW * ROW)
#define RUP_PAGE(x) (((x) + PAGE - 1) / PAGE * PAGE)

static double now_s(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + (double)t.tv_nsec * 1e-9;
}

/* ---- a small job pool ---------------------------------------------------
 * Jobs are intrusive: every argument struct starts with a `job`, and the
 * caller owns its storage (arrays sized before a run starts), so pushing a
 * job cannot fail half way through a batch and leave a latch that never
 * reaches zero. */
typedef struct job {
    struct job *next;
    void (*fn)(struct job *);
} job;

typedef struct {
    pthread_mutex_t lock;
    pthread_cond_t cv;
    job *head, *tail;
    job *hhead, *htail;   /* taken first (pool_push_hi) */
    int stop;
    int nthreads;
    pthread_t *th;
} pool;

static void *pool_main(void *p)
{
    pool *P = p;
    for (;;) {
        pthread_mutex_lock(&P->lock);
        while (!P->head && !P->hhead && !P->stop)
            pthread_cond_wait(&P->cv, &P->lock);
        job *j = P->hhead ? P->hhead : P->head;
        if (!j) {
            pthread_mutex_unlock(&P->lock);
            return NULL;
        }
        if (j == P->hhead) {
            P->hhead = j->next;
            if (!P->hhead)
                P->htail = NULL;
        } else {
            P->head = j->next;
            if (!P->head)
                P->tail = NULL;
        }
        pthread_mutex_unlock(&P->lock);
        j->fn(j);
    }
}

static void pool_stop(pool *P);

/* All n threads or none: a partial start joins what it started. */
static int pool_start(pool *P, int n)
{
    memset(P, 0, sizeof(*P));
    pthread_mutex_init(&P->lock, NULL);
    pthread_cond_init(&P->cv, NULL);
    P->th = calloc((size_t)n, sizeof(pthread_t));
    if (!P->th) {
        pthread_mutex_destroy(&P->lock);
        pthread_cond_destroy(&P->cv);
        return -ENOMEM;
    }
    for (int i = 0; i < n; i++) {
        if (pthread_create(&P->th[i], NULL, pool_main, P) != 0) {
            pool_stop(P);
            return -EAGAIN;
        }
        P->nthreads++;
    }
    return 0;
}

static void pool_push(pool *P, job *j, void (*fn)(job *))
{
    j->fn = fn;
    j->next = NULL;
    pthread_mutex_lock(&P->lock);
    if (P->tail)
        P->tail->next = j;
    else
        P->head = j;
    P->tail = j;
    pthread_cond_signal(&P->cv);
    pthread_mutex_unlock(&P->lock);
}

/* The same, ahead of every job pushed with pool_push. */
static void pool_push_hi(pool *P, job *j, void (*fn)(job *))
{
    j->fn = fn;
    j->next = NULL;
    pthread_mutex_lock(&P->lock);
    if (P->htail)
        P->htail->next = j;
    else
        P->hhead = j;
    P->htail = j;
    pthread_cond_signal(&P->cv);
    pthread_mutex_unlock(&P->lock);
}

static void pool_stop(pool *P)
{
    pthread_mutex_lock(&P->lock);
    P->stop = 1;
    pthread_cond_broadcast(&P->cv);
    pthread_mutex_unlock(&P->lock);
    for (int i = 0; i < P->nthreads; i++)
        pthread_join(P->th[i], NULL);
    free(P->th);
    pthread_mutex_destroy(&P->lock);
    pthread_cond_destroy(&P->cv);
}

/* countdown latch */
typedef struct {
    pthread_mutex_t lock;
    pthread_cond_t cv;
    long left;
    double t_zero;        /* when the count reached zero */
} latch;

static void latch_init(latch *l, long n)
{
    pthread_mutex_init(&l->lock, NULL);
    pthread_cond_init(&l->cv, NULL);
    l->left = n;
    l->t_zero = n ? 0.0 : now_s();
}
static void latch_down(latch *l)
{
    pthread_mutex_lock(&l->lock);
    if (--l->left == 0) {
        l->t_zero = now_s();
        pthread_cond_broadcast(&l->cv);
    }
    pthread_mutex_unlock(&l->lock);
}
static void latch_wait(latch *l)
{
    pthread_mutex_lock(&l->lock);
    while (l->left > 0)
        pthread_cond_wait(&l->cv, &l->lock);
    pthread_mutex_unlock(&l->lock);
}
static void latch_destroy(latch *l)
{
    pthread_mutex_destroy(&l->lock);
    pthread_cond_destroy(&l->cv);
}

/* ---- plan --------------------------------------------------------------- */
typedef struct {
    const char *path;
    int p;                               /* output target: P (gen) or the victim (rebuild) */
    int n;                               /* sources */
    int holders[MAX_STORAGE_TARGETS];    /* source targets, ascending */
    int rebuild;                         /* 1: rebuild task */
    int parity_src;                      /* rebuild: index of the parity body among the sources */
    int64_t timestamp;                   /* rebuild: FileInfo.timestamp (corrupt check) */
    uint64_t size[MAX_STORAGE_TARGETS];  /* source lengths at stat time (0 = missing);
                                            gen: also the parity header */
    uint64_t src_off[MAX_STORAGE_TARGETS];/* file offset of the source data (parity body: 8n) */
    uint64_t max_cs;
    uint64_t out_len;                    /* gen: max_cs; rebuild: header[victim index] */
    uint64_t in_off[MAX_STORAGE_TARGETS];/* offsets in the input slab (page layout, DIRECT:
                                            of the file's first byte, page-aligned; the data
                                            then starts src_off further) */
    uint64_t out_off;                    /* offset in the output slab */
    int batch;
    int prealloc;                        /* posix_fallocate the output first (not where the
                                            output target's directory is tmpfs: do_write) */
    int verify;                          /* 1: verify task; sources 0..n-2 are the chunks, n-1 the
                                            parity body (parity_src) */
    size_t item;                         /* verify: index of the work item */
    uint32_t status;                     /* verify: BCP_VERIFY_* or VERIFY_PENDING */
    uint64_t first_bad, bad_bytes;       /* verify: the device's record */
    /* verify with Q (bcp_pipeline_verify_q): vq = 1, q_st the item's Q target
     * (-1: none); after the stat phase q_state, and for a CHECKED task the Q
     * body as source q_src behind the P body */
    int vq;
    uint32_t q_state;
    uint64_t q_bad, members;             /* vq, CHECKED: the rest of the record (p_bad is bad_bytes) */
    struct timespec mtime[MAX_STORAGE_TARGETS]; /* verify: mtime of source k's file at stat time (repair) */
    uint64_t allow;                      /* repair: the members that may be written */
    /* Q parity.  gen: q_st is the item's Q target when the run writes its Q
     * file (-1: none).  rebuild2: pq = 1 recovers the victim from Q alone (P is
     * lost too), pq = 2 both victims (p, p2) from P and Q; the sources are then
     * the survivors, ascending, src_pos[k] their position among the item's
     * `width` holders, followed by the P body (pq = 2, parity_src) and the Q
     * body (q_src). */
    int q_st;
    int pq;
    int p2;                              /* pq = 2: the second victim */
    int width;                           /* pq: holders of the item = header entries */
    int lost_pos[2];                     /* pq: positions of the victims */
    int src_pos[MAX_STORAGE_TARGETS];    /* pq: position of survivor k */
    int q_src;                           /* pq: index of the Q body among the sources */
    int unrecov;                         /* pq, after the stat phase: cannot be recovered */
    int has2;                            /* a second output: the Q body (gen), the second chunk (pq = 2) */
    uint64_t out_len2;
    int prealloc2;
    uint64_t header[MAX_STORAGE_TARGETS];/* pq: the sizes header of the parity files */
} task;

#define VERIFY_PENDING 0xFFu             /* passed the stat phase: to be read and compared */

/* Where source k is read from: 0 the chunks directory, 1 the parity directory
 * and 2 the Q parity directory (both after the u64 header). */
static const char *const k_dir[3] = {"chunks", "parity", "parityq"};
static int src_kind(const task *t, int k)
{
    if ((t->pq || (t->vq && t->q_state == BCP_QSTATE_CHECKED)) && k == t->q_src)
        return 2;
    return (t->rebuild || t->verify) && k == t->parity_src;
}

/* Bytes a task takes in the output slab; a second output follows the first
 * at the next multiple of 256. */
static uint64_t out_off2(const task *t)
{
    return t->out_off + (t->out_len + 255u) / 256u * 256u;
}

static uint64_t out_span(const task *t)
{
    if (t->verify)
        return t->vq ? sizeof(bcp_pq_check_result) : sizeof(bcp_check_result);
    return (t->out_len + 255u) / 256u * 256u + (t->has2 ? (t->out_len2 + 255u) / 256u * 256u : 0);
}

typedef struct {
    job j;                               /* first: the pool's link */
    const char *root;
    task *t;
    latch *done;
    int corrupt_fd;                      /* rebuild: corrupt list (or -1) */
    int q_win;                           /* windowed items have Q too (bcp_pipeline_set_q_windowed) */
} stat_arg;

typedef struct {
    uint8_t *h_in, *h_out;
    void *d_in, *d_out;
    size_t in_cap, out_cap;
    bcp_event *ev_h, *ev_k, *ev_d;
    latch reads, writes;
    int busy;             /* writes of the previous batch pending */
} slot;



/* One read job: bytes [off, off + len) of source k's data, into dst (its
 * place in the slab + off).  Sources are read in pieces of at most PIECE
 * bytes, so a batch's big chunks spread over the io threads instead of one
 * thread finishing a 4 MiB chunk while the others idle.  DIRECT mode: off and
 * len are of the file itself (page-aligned, the page layout puts the file's
 * first byte at a page of the slab), read with O_DIRECT. */
#define PIECE ((uint64_t)1 << 20)
typedef struct {
    job j;
    const char *root;
    task *t;
    int k;                /* source */
    uint64_t off, len;
    uint8_t *dst;
    uint64_t *bytes;      /* accumulated under lock: {data bytes, of them read with O_DIRECT,
                             DIRECT pieces read through the page cache instead} */
    latch *done;
    int direct;
    int *errors;          /* verify: counts sources that could not be read to their end (or NULL) */
} read_arg;

static uint64_t pieces_of(uint64_t size)
{
    return (size + PIECE - 1) / PIECE;
}

/* Read jobs of source k: PIECE-sized pieces of its data, or (DIRECT) of the
 * file prefix up to the data's end, page-rounded. */
static uint64_t read_extent(const task *t, int k, int direct)
{
    if (!t->size[k])
        return 0;
    return direct ? RUP_PAGE(t->src_off[k] + t->size[k]) : t->size[k];
}

/* A repair run's policy, results and counts (bcp_pipeline_repair_q); only the
 * completion thread touches them while the run is on. */
typedef struct repair_ctx {
    int mode, dry_run;
    int windowed;           /* bcp_pipeline_set_repair_windowed: windowed items are admitted */
    uint32_t max_members;
    bcp_repair_q_item *res; /* per work item: repair, bytes_fixed */
    int list_fd;            /* the repaired list (or -1) */
    uint64_t files_written, bytes_written, launches;
    int errors;
} repair_ctx;

typedef struct {
    job j;
    const char *root;
    task *t;
    const uint8_t *body;
    latch *done;
    FILE *log;
    int *errors;
    int prealloc;         /* posix_fallocate first (not on tmpfs: see do_write) */
    int second;           /* the task's second output (Q file / second rebuilt chunk) */
} write_arg;

typedef struct {
    job j;
    slot *S;
    const char *root;
    task *tasks;
    write_arg *wa;        /* two per task of the run (the second: task.has2) */
    size_t first, last;
    pool *io;
    FILE *log;
    int *errors;
    int *dev_rc;
    struct repair_ctx *rp; /* a repair run (or NULL), and what its stage needs of the batch's lane */
    bcp_engine *eng;
    bcp_queue *qr;
    int dir;
} complete_arg;

static pthread_mutex_t g_stat_lock = PTHREAD_MUTEX_INITIALIZER;

static void chunk_file(char *buf, size_t cap, const char *root, int st, const char *dir, const char *path)
{
    snprintf(buf, cap, "%s/st%d/%s/%s", root, st, dir, path);
}

/* Corrupt list line (task_processing.c:54-60, 268-271), written whole. */
static void push_corrupt(int fd, const char *path)
{
    if (fd < 0)
        return;
    size_t len = strlen(path);
    char *line = malloc(len + 2);
    if (!line)
        return;
    memcpy(line, path, len);
    line[len] = '\n';
    ssize_t w = write(fd, line, len + 1);
    (void)w;
    free(line);
}

static void do_stat(job *p)
{
    stat_arg *a = (stat_arg *)p;
    task *t = a->t;
    char fn[4352];
    t->max_cs = 0;
    if (t->verify) {
        /* the parity header and size, every holder's chunk as it is now;
         * precedence STALE, NO_PARITY, SIZE */
        const int n = t->n - 1;
        uint64_t header[MAX_STORAGE_TARGETS] = {0};
        uint64_t fsize = 0;
        int have = 0, stale = 0, resized = 0;
        struct stat st;
        chunk_file(fn, sizeof(fn), a->root, t->holders[n], "parity", t->path);
        int fd = open(fn, O_RDONLY);
        if (fd >= 0) {
            if (fstat(fd, &st) == 0) {
                fsize = (uint64_t)st.st_size;
                t->mtime[n] = st.st_mtim;
            }
            have = fsize >= (uint64_t)n * 8u && pread(fd, header, (size_t)n * 8u, 0) == (ssize_t)((size_t)n * 8u);
            close(fd);
        }
        for (int k = 0; k < n; k++)
            if (header[k] > t->max_cs)
                t->max_cs = header[k];
        for (int k = 0; k < n; k++) {
            chunk_file(fn, sizeof(fn), a->root, t->holders[k], "chunks", t->path);
            uint64_t cur = 0;
            if (stat(fn, &st) == 0) {
                cur = (uint64_t)st.st_size;
                stale |= st.st_mtime > t->timestamp;
                t->mtime[k] = st.st_mtim;
            }
            resized |= cur != header[k];
            t->size[k] = header[k];
            t->src_off[k] = 0;
        }
        t->src_off[n] = (uint64_t)n * 8u;
        t->size[n] = t->max_cs;
        t->out_len = t->max_cs;
        t->status = stale                                                 ? BCP_VERIFY_STALE
                    : !have || fsize != (uint64_t)n * 8u + t->max_cs ? BCP_VERIFY_NO_PARITY
                    : resized                                             ? BCP_VERIFY_SIZE
                                                                          : VERIFY_PENDING;
        if (t->vq && t->status == VERIFY_PENDING) {
            /* the Q state: by rule none, or a file in order beside P's */
            t->q_state = BCP_QSTATE_NONE;
            if (t->q_st >= 0 && (t->max_cs <= WINDOW || a->q_win)) {
                uint64_t hq[MAX_STORAGE_TARGETS] = {0};
                uint64_t qsize = 0;
                int qhave = 0;
                chunk_file(fn, sizeof(fn), a->root, t->q_st, "parityq", t->path);
                fd = open(fn, O_RDONLY);
                if (fd >= 0) {
                    if (fstat(fd, &st) == 0) {
                        qsize = (uint64_t)st.st_size;
                        t->mtime[t->n] = st.st_mtim;
                    }
                    qhave = qsize >= (uint64_t)n * 8u && pread(fd, hq, (size_t)n * 8u, 0) == (ssize_t)((size_t)n * 8u);
                    close(fd);
                }
                if (qhave && qsize == (uint64_t)n * 8u + t->max_cs && memcmp(hq, header, (size_t)n * 8u) == 0) {
                    t->q_state = BCP_QSTATE_CHECKED;
                    t->q_src = t->n;
                    t->holders[t->n] = t->q_st;
                    t->src_off[t->n] = (uint64_t)n * 8u;
                    t->size[t->n] = t->max_cs;
                    t->n++;
                } else {
                    t->q_state = BCP_QSTATE_BAD;
                }
            }
        }
        latch_down(a->done);
        return;
    }
    if (t->pq) {
        /* rebuild2 from Q (and P): the parity files' headers and sizes decide
         * whether the item can be recovered at all */
        const int w = t->width;
        uint64_t hq[MAX_STORAGE_TARGETS] = {0};
        int ok = 1;
        for (int pass = 0; pass < 2; pass++) {
            const int k = pass ? t->q_src : t->parity_src;
            if (k < 0)
                continue;
            uint64_t *h = pass ? hq : t->header;
            uint64_t fsize = 0, m = 0;
            struct stat st;
            chunk_file(fn, sizeof(fn), a->root, t->holders[k], k_dir[src_kind(t, k)], t->path);
            int fd = open(fn, O_RDONLY);
            int have = 0;
            if (fd >= 0) {
                if (fstat(fd, &st) == 0)
                    fsize = (uint64_t)st.st_size;
                have = fsize >= (uint64_t)w * 8u && pread(fd, h, (size_t)w * 8u, 0) == (ssize_t)((size_t)w * 8u);
                close(fd);
            }
            for (int j = 0; j < w; j++)
                if (h[j] > m)
                    m = h[j];
            ok = ok && have && fsize == (uint64_t)w * 8u + m;
        }
        if (t->parity_src < 0)
            memcpy(t->header, hq, sizeof(hq));
        else
            ok = ok && memcmp(t->header, hq, (size_t)w * 8u) == 0;
        for (int j = 0; j < w; j++)
            if (t->header[j] > t->max_cs)
                t->max_cs = t->header[j];
        ok = ok && (t->max_cs <= WINDOW || a->q_win); /* windowed items have no Q without the switch */
        for (int k = 0; k < t->n; k++) {
            struct stat st;
            if (k == t->parity_src || k == t->q_src) {
                t->src_off[k] = (uint64_t)w * 8u;
                t->size[k] = ok ? t->max_cs : 0;
                continue;
            }
            chunk_file(fn, sizeof(fn), a->root, t->holders[k], "chunks", t->path);
            t->src_off[k] = 0;
            t->size[k] = 0;
            if (stat(fn, &st) == 0) {
                t->size[k] = (uint64_t)st.st_size > t->max_cs ? t->max_cs : (uint64_t)st.st_size;
                if (st.st_mtime > t->timestamp)
                    push_corrupt(a->corrupt_fd, t->path);
            }
        }
        t->out_len = t->header[t->lost_pos[0]];
        t->out_len2 = t->pq == 2 ? t->header[t->lost_pos[1]] : 0;
        t->unrecov = !ok;
        latch_down(a->done);
        return;
    }
    if (!t->rebuild) {
        for (int k = 0; k < t->n; k++) {
            chunk_file(fn, sizeof(fn), a->root, t->holders[k], "chunks", t->path);
            struct stat st;
            t->size[k] = stat(fn, &st) == 0 ? (uint64_t)st.st_size : 0;
            t->src_off[k] = 0;
            if (t->size[k] > t->max_cs)
                t->max_cs = t->size[k];
        }
        t->out_len = t->max_cs;
        if (t->q_st >= 0 && t->max_cs > WINDOW && !a->q_win) {
            /* windowed: P only; a Q file from an earlier, smaller state goes */
            chunk_file(fn, sizeof(fn), a->root, t->q_st, "parityq", t->path);
            unlink(fn);
            t->q_st = -2;
        }
        t->has2 = t->q_st >= 0;
        t->out_len2 = t->max_cs;
        latch_down(a->done);
        return;
    }
    /* rebuild: survivors as they are now; the parity holder contributes its
     * stored header (sizes at generation) and the body after it */
    uint64_t header[MAX_STORAGE_TARGETS] = {0};
    const int n = t->n;
    for (int k = 0; k < n; k++) {
        struct stat st;
        if (k == t->parity_src) {
            chunk_file(fn, sizeof(fn), a->root, t->holders[k], "parity", t->path);
            int fd = open(fn, O_RDONLY);
            uint64_t fsize = 0;
            if (fd >= 0) {
                if (fstat(fd, &st) == 0)
                    fsize = (uint64_t)st.st_size;
                ssize_t r = pread(fd, header, (size_t)n * 8u, 0); /* a short header reads as zeros */
                (void)r;
                close(fd);
            }
            t->src_off[k] = (uint64_t)n * 8u;
            t->size[k] = fsize > t->src_off[k] ? fsize - t->src_off[k] : 0;
        } else {
            chunk_file(fn, sizeof(fn), a->root, t->holders[k], "chunks", t->path);
            t->src_off[k] = 0;
            if (stat(fn, &st) == 0) {
                t->size[k] = (uint64_t)st.st_size;
                if (st.st_mtime > t->timestamp)
                    push_corrupt(a->corrupt_fd, t->path);
            } else {
                t->size[k] = 0;
            }
        }
    }
    for (int k = 0; k < n; k++)
        if (header[k] > t->max_cs)
            t->max_cs = header[k];
    /* the victim's index in the header: survivors (and the victim) below it */
    int idx = 0;
    for (int k = 0; k < n; k++)
        if (k != t->parity_src && t->holders[k] < t->p)
            idx++;
    t->out_len = header[idx];
    /* sources longer than max_cs are only read up to it (data_to_send) */
    for (int k = 0; k < n; k++)
        if (t->size[k] > t->max_cs)
            t->size[k] = t->max_cs;
    latch_down(a->done);
}

static void do_read(job *p)
{
    read_arg *a = (read_arg *)p;
    task *t = a->t;
    const uint64_t want = a->len;
    const uint64_t foff = a->direct ? a->off : t->src_off[a->k] + a->off; /* file offset of dst[0] */
    uint64_t got = 0;
    int direct = 0, fell_back = 0;
    if (want) {
        char fn[4352];
        chunk_file(fn, sizeof(fn), a->root, t->holders[a->k], k_dir[src_kind(t, a->k)], t->path);
        int fd = -1;
        if (a->direct) {
            fd = open(fn, O_RDONLY | O_DIRECT);
            direct = fd >= 0;
            fell_back = !direct;
        }
        if (fd < 0)
            fd = open(fn, O_RDONLY);
        if (fd >= 0) {
            if (!direct)
                posix_fadvise(fd, (off_t)foff, (off_t)want, POSIX_FADV_SEQUENTIAL);
            while (got < want) {
                ssize_t r = pread(fd, a->dst + got, (size_t)(want - got), (off_t)(foff + got));
                if (direct && r > 3000 && bcpi_inject_hit(BCP_INJECT_DIRECT_READ)) {
                    /* (failure injection) short before the end: what the read
                     * did deliver past the cut is spoilt, the fallback must
                     * read it again */
                    memset(a->dst + got + 3000, 0xA5, (size_t)r - 3000);
                    r = 3000;
                }
                if (r > 0)
                    got += (uint64_t)r;
                struct stat sb;
                if (direct && (r < 0 || (got % PAGE && got < want && fstat(fd, &sb) == 0 &&
                                         (uint64_t)sb.st_size > foff + got))) {
                    /* refused (EINVAL: alignment the filesystem wants bigger,
                     * EFAULT: memory it cannot pin) or short before the end
                     * of the file: the rest of the piece through the page cache */
                    close(fd);
                    fd = open(fn, O_RDONLY);
                    direct = 0;
                    fell_back = 1;
                    if (fd < 0)
                        break;
                    continue;
                }
                if (r <= 0 || (direct && got % PAGE))
                    break; /* end of file (an O_DIRECT read ends short there) */
            }
            if (fd >= 0)
                close(fd);
        }
    }
    /* the source's data inside this piece; what the file no longer holds is
     * zero padded, as chunk_sender does (:302-303) */
    const uint64_t d_lo = a->direct ? t->src_off[a->k] : foff;
    const uint64_t d_hi = a->direct ? d_lo + t->size[a->k] : foff + want;
    const uint64_t lo = d_lo > foff ? d_lo : foff;
    const uint64_t hi = d_hi < foff + want ? d_hi : foff + want;
    const uint64_t have = foff + got;
    uint64_t data = 0;
    if (hi > lo) {
        const uint64_t z = have > lo ? have : lo;
        if (z < hi)
            memset(a->dst + (z - foff), 0, (size_t)(hi - z));
        data = (have < hi ? have : hi) > lo ? (have < hi ? have : hi) - lo : 0;
    }
    pthread_mutex_lock(&g_stat_lock);
    if (a->errors && hi > lo && have < hi)
        (*a->errors)++; /* shorter than at stat time, or unreadable: compared as zeros */
    a->bytes[0] += data;
    if (a->direct) {
        if (fell_back)
            a->bytes[2]++;
        else
            a->bytes[1] += data;
    }
    pthread_mutex_unlock(&g_stat_lock);
    latch_down(a->done);
}

static void mkdir_parents(char *fn)
{
    for (char *q = fn + 1; *q; q++)
        if (*q == '/') {
            *q = 0;
            mkdir(fn, S_IRWXU);
            *q = '/';
        }
}

static void do_write(job *p)
{
    write_arg *a = (write_arg *)p;
    task *t = a->t;
    char fn[4352];
    /* the second output: the Q file of a gen task, the second chunk of a
     * two-victim rebuild */
    const int out_st = !a->second ? t->p : t->rebuild ? t->p2 : t->q_st;
    const uint64_t out_len = a->second ? t->out_len2 : t->out_len;
    chunk_file(fn, sizeof(fn), a->root, out_st, t->rebuild ? "chunks" : a->second ? "parityq" : "parity", t->path);
    /* directories only when the file cannot be created (mkdir_for_file,
     * task_processing.c:30-40, does every level first: a lookup per level
     * per file).  (Overwriting an existing file in place instead of
     * O_TRUNC, to reuse its page-cache pages, measured no different:
     * profiles/r04/pipeline/lib_ab_overwrite_in_place_r4r.jsonl.) */
    int fd = open(fn, O_CREAT | O_WRONLY | O_TRUNC, S_IRUSR | S_IWUSR);
    if (fd < 0 && errno == ENOENT) {
        mkdir_parents(fn);
        fd = open(fn, O_CREAT | O_WRONLY | O_TRUNC, S_IRUSR | S_IWUSR);
    }
    int bad = fd < 0;
    if (!bad) {
        /* gen: u64 sizes header + body; rebuild: the chunk itself */
        const size_t hdr = t->rebuild ? 0 : 8u * (size_t)t->n;
        uint64_t total = hdr + out_len;
        /* The reference reserves the file's space first (task_processing.c:186):
         * on a disk that keeps it in one extent and fails early when full.  On
         * tmpfs it makes the kernel allocate and ZERO every page before the
         * write fills it again -- one more pass over the parity bytes for
         * nothing -- so it is skipped there (the file is the same). */
        if (total && a->prealloc)
            posix_fallocate(fd, 0, (off_t)total);
        struct iovec iov[2] = {{t->size, hdr}, {(void *)a->body, (size_t)out_len}};
        uint64_t done = 0;
        int idx = total ? 0 : 2; /* an empty rebuilt chunk: nothing to write */
        while (idx < 2 && !bad) {
            ssize_t w = writev(fd, iov + idx, 2 - idx);
            if (w <= 0) {
                bad = 1;
                break;
            }
            done += (uint64_t)w;
            size_t left = (size_t)w;
            while (idx < 2 && left >= iov[idx].iov_len) {
                left -= iov[idx].iov_len;
                idx++;
            }
            if (idx < 2) {
                iov[idx].iov_base = (uint8_t *)iov[idx].iov_base + left;
                iov[idx].iov_len -= left;
            }
        }
        (void)done;
        close(fd);
    }
    if (bad) {
        pthread_mutex_lock(&g_stat_lock);
        (*a->errors)++;
        if (a->log)
            fprintf(a->log, "bcp_pipeline: writing parity '%s' failed: %s\n", fn, strerror(errno));
        pthread_mutex_unlock(&g_stat_lock);
    }
    latch_down(a->done);
}

/* Completion stage (one thread, batches in order): wait for the batch's D2H,
 * then hand its parity files to the io pool (behind every queued read). */
/* ---- scrub repair: the stage between a batch's records and its slot's release */
static uint64_t data_off(const task *t, int k, int page_layout);

#define REPAIR_PENDING 0xFFu /* admitted by the policy: in the repair launch */

/* Size a verify task's source file had at stat time: a chunk is its header
 * entry, a parity file the header and the body. */
static uint64_t repair_fsize(const task *t, int k)
{
    return t->src_off[k] + t->size[k];
}

static void push_repaired(int fd, const char *path, int kind, int target, uint64_t bytes)
{
    static const char *const name[3] = {"data", "p", "q"};
    if (fd < 0)
        return;
    const size_t cap = strlen(path) + 64;
    char *line = malloc(cap);
    if (!line)
        return;
    const int len = snprintf(line, cap, "%s\t%s\t%d\t%llu\n", path, name[kind], target, (unsigned long long)bytes);
    ssize_t w = write(fd, line, (size_t)len);
    (void)w;
    free(line);
}

/* Write back the allowed members of one repaired, re-checked item: the slab
 * still holds each file as read (was), the device the corrected bytes (now).
 * Returns the item's BCP_REPAIRED_* verdict. */
static uint32_t repair_write_back(const complete_arg *a, const task *t)
{
    repair_ctx *R = a->rp;
    int src[MAX_STORAGE_TARGETS], ns = 0;
    char fn[4352];
    for (int k = 0; k < t->parity_src; k++)
        if (t->allow >> k & 1)
            src[ns++] = k;
    if (t->allow & BCP_PQ_BAD_P)
        src[ns++] = t->parity_src;
    if (t->allow & BCP_PQ_BAD_Q)
        src[ns++] = t->q_src;
    /* a file that changed under the scrub leaves the whole item alone */
    for (int i = 0; i < ns; i++) {
        const int k = src[i];
        struct stat st;
        chunk_file(fn, sizeof(fn), a->root, t->holders[k], k_dir[src_kind(t, k)], t->path);
        if (stat(fn, &st) != 0)
            return errno == ENOENT ? BCP_REPAIRED_CHANGED : BCP_REPAIRED_FAILED;
        if ((uint64_t)st.st_size != repair_fsize(t, k) || st.st_mtim.tv_sec != t->mtime[k].tv_sec ||
            st.st_mtim.tv_nsec != t->mtime[k].tv_nsec)
            return BCP_REPAIRED_CHANGED;
    }
    for (int i = 0; i < ns; i++) {
        const int k = src[i], kind = src_kind(t, k);
        const uint64_t off = data_off(t, k, a->dir), len = t->size[k];
        uint8_t *was = malloc(len ? len : 1);
        if (!was)
            return BCP_REPAIRED_FAILED;
        memcpy(was, a->S->h_in + off, len);
        int rc = bcp_d2h_async(a->qr, a->S->h_in + off, (const uint8_t *)a->S->d_in + off, (size_t)len);
        if (!rc)
            rc = bcp_queue_sync(a->qr);
        uint64_t bw = 0;
        chunk_file(fn, sizeof(fn), a->root, t->holders[k], k_dir[kind], t->path);
        if (!rc)
            rc = bcp_patch_file(fn, t->src_off[k], was, a->S->h_in + off, len, repair_fsize(t, k), &t->mtime[k], &bw);
        free(was);
        if (bw) {
            R->files_written++;
            R->bytes_written += bw;
            push_repaired(R->list_fd, t->path, kind, t->holders[k], bw);
        }
        if (rc == -ESTALE)
            return BCP_REPAIRED_CHANGED;
        if (rc) {
            if (a->log)
                fprintf(a->log, "bcp_pipeline: repair of '%s' failed: %s\n", fn, bcp_strerror(rc));
            return BCP_REPAIRED_FAILED;
        }
    }
    return BCP_REPAIRED_DONE;
}

/* The batch's MISMATCH items after their records are in: the policy on the
 * host, then one repair launch and one check launch over the admitted stripes
 * where they lie in the slot's device slab, then the write-back. */
static void repair_batch(const complete_arg *a)
{
    repair_ctx *R = a->rp;
    size_t n = 0, nsrc = 0;
    for (size_t i = a->first; i < a->last; i++) {
        task *t = &a->tasks[i];
        if (t->status != BCP_VERIFY_MISMATCH)
            continue;
        bcp_repair_q_item *v = &R->res[t->item];
        v->repair = BCP_REPAIRED_UNLOCATED;
        if (!t->vq || t->q_state != BCP_QSTATE_CHECKED || (t->max_cs > WINDOW && !R->windowed))
            continue;
        const bcp_pq_check_result r = {t->first_bad, t->bad_bytes, t->q_bad, t->members};
        const int vd = bcp_pq_repair_verdict(&r, (uint32_t)t->parity_src, R->mode, R->max_members, &t->allow);
        if (vd == BCP_VERDICT_POLICY)
            v->repair = BCP_REPAIRED_POLICY;
        if (vd != BCP_VERDICT_REPAIR)
            continue;
        v->repair = REPAIR_PENDING;
        n++;
        nsrc += (size_t)t->parity_src;
    }
    if (!n)
        return;
    const size_t rec = sizeof(bcp_pq_repair_result) + sizeof(bcp_pq_check_result);
    bcp_stripe *st = malloc(n * sizeof(*st));
    bcp_source *so = malloc((nsrc ? nsrc : 1) * sizeof(*so));
    uint64_t *qb = malloc(2 * n * sizeof(*qb)), *al = qb ? qb + n : NULL;
    uint8_t *h = malloc(n * rec);
    void *d = NULL;
    int rc = st && so && qb && h ? bcp_dev_alloc(a->eng, n * rec, &d) : -ENOMEM;
    if (!rc) {
        uint32_t j = 0, s = 0;
        int win = 0; /* a windowed stripe among them: the _win entry points, which take a mixed batch */
        for (size_t i = a->first; i < a->last; i++) {
            const task *t = &a->tasks[i];
            if (t->status != BCP_VERIFY_MISMATCH || R->res[t->item].repair != REPAIR_PENDING)
                continue;
            const int nfold = t->parity_src;
            st[j] = (bcp_stripe){(uint64_t)a->S->d_in + data_off(t, nfold, a->dir), t->out_len, s, (uint32_t)nfold,
                                 t->max_cs > WINDOW ? WINDOW : 0};
            win |= t->max_cs > WINDOW;
            qb[j] = (uint64_t)a->S->d_in + data_off(t, t->q_src, a->dir);
            al[j] = t->allow;
            for (int k = 0; k < nfold; k++)
                so[s++] = (bcp_source){(uint64_t)a->S->d_in + data_off(t, k, a->dir), t->size[k]};
            j++;
        }
        bcp_pq_repair_result *d_rep = d;
        bcp_pq_check_result *d_chk = (bcp_pq_check_result *)(d_rep + n);
        if (!(rc = win ? bcp_pq_repair_stripes_win_async(a->qr, st, (uint32_t)n, so, s, qb, al, d_rep)
                       : bcp_pq_repair_stripes_async(a->qr, st, (uint32_t)n, so, s, qb, al, d_rep)) &&
            !(rc = win ? bcp_pq_check_stripes_win_async(a->qr, st, (uint32_t)n, so, s, qb, d_chk)
                       : bcp_pq_check_stripes_async(a->qr, st, (uint32_t)n, so, s, qb, d_chk)) &&
            !(rc = bcp_d2h_async(a->qr, h, d, n * rec)))
            rc = bcp_queue_sync(a->qr);
        R->launches++;
    }
    const bcp_pq_repair_result *rep = (const bcp_pq_repair_result *)h;
    const bcp_pq_check_result *chk = rep ? (const bcp_pq_check_result *)(rep + n) : NULL;
    size_t j = 0;
    for (size_t i = a->first; i < a->last; i++) {
        const task *t = &a->tasks[i];
        bcp_repair_q_item *v = &R->res[t->item];
        if (t->status != BCP_VERIFY_MISMATCH || v->repair != REPAIR_PENDING)
            continue;
        if (rc)
            v->repair = BCP_REPAIRED_FAILED;
        else if (rep[j].left)
            v->repair = BCP_REPAIRED_UNLOCATED;
        else if (chk[j].members || rep[j].members != t->members) /* nothing reaches a disk unverified */
            v->repair = BCP_REPAIRED_FAILED;
        else
            v->repair = R->dry_run ? BCP_REPAIRED_DRY : repair_write_back(a, t);
        if (v->repair == BCP_REPAIRED_DONE || v->repair == BCP_REPAIRED_DRY)
            v->bytes_fixed = rep[j].fixed;
        R->errors += v->repair == BCP_REPAIRED_FAILED;
        j++;
    }
    if (rc && a->log)
        fprintf(a->log, "bcp_pipeline: repair launch failed: %s\n", bcp_strerror(rc));
    if (d)
        bcp_dev_free(a->eng, d);
    free(st);
    free(so);
    free(qb);
    free(h);
}

static void do_complete(job *p)
{
    /* The run frees its job arrays once every write of the batch has counted
     * down, which may be before this function returns: copy what it needs
     * and touch neither `a` nor a pushed write job after handing it over. */
    const complete_arg a = *(complete_arg *)p;
    int rc = bcp_event_sync(a.S->ev_d);
    if (a.first < a.last && a.tasks[a.first].verify) {
        /* verify: the batch's records are its result; no writes */
        if (rc) {
            pthread_mutex_lock(&g_stat_lock);
            *a.dev_rc = rc;
            pthread_mutex_unlock(&g_stat_lock);
        }
        latch *done = &a.S->writes;
        for (size_t i = a.first; i < a.last; i++) {
            task *t = &a.tasks[i];
            if (!rc && t->vq && t->q_state == BCP_QSTATE_CHECKED) {
                const bcp_pq_check_result *r = (const bcp_pq_check_result *)(a.S->h_out + t->out_off);
                t->first_bad = r->first_bad;
                t->bad_bytes = r->p_bad;
                t->q_bad = r->q_bad;
                t->members = r->members;
                t->status = r->members ? BCP_VERIFY_MISMATCH : BCP_VERIFY_OK;
            } else if (!rc) {
                const bcp_check_result *r = (const bcp_check_result *)(a.S->h_out + t->out_off);
                t->first_bad = r->first_bad;
                t->bad_bytes = r->bad_bytes;
                t->status = r->bad_bytes ? BCP_VERIFY_MISMATCH : BCP_VERIFY_OK;
            }
        }
        if (!rc && a.rp)
            repair_batch(&a); /* before the slot is released: it corrects in the slot's slabs */
        for (size_t i = a.first; i < a.last; i++)
            latch_down(done);
        return;
    }
    if (rc) {
        pthread_mutex_lock(&g_stat_lock);
        *a.dev_rc = rc;
        pthread_mutex_unlock(&g_stat_lock);
        for (size_t i = a.first; i < a.last; i++)
            for (int o = 0; o <= a.tasks[i].has2; o++)
                latch_down(&a.S->writes);
    } else {
        for (size_t i = a.first; i < a.last; i++) {
            /* (has2 read before the first job is handed over: see above) */
            const int has2 = a.tasks[i].has2;
            const uint64_t off2 = out_off2(&a.tasks[i]);
            const int pre2 = a.tasks[i].prealloc2;
            write_arg *w = &a.wa[2 * i];
            *w = (write_arg){{0}, a.root, &a.tasks[i], a.S->h_out + a.tasks[i].out_off, &a.S->writes, a.log, a.errors,
                             a.tasks[i].prealloc, 0};
            if (has2)
                w[1] = (write_arg){{0}, a.root, &a.tasks[i], a.S->h_out + off2, &a.S->writes, a.log, a.errors, pre2, 1};
            pool_push(a.io, &w->j, do_write);
            if (has2)
                pool_push(a.io, &w[1].j, do_write);
        }
    }
}

static int slot_alloc(bcp_engine *e, slot *s, size_t in_cap, size_t out_cap)
{
    int rc;
    memset(s, 0, sizeof(*s));
    if ((rc = bcp_host_alloc(e, in_cap, (void **)&s->h_in)) || (rc = bcp_host_alloc(e, out_cap, (void **)&s->h_out)) ||
        (rc = bcp_dev_alloc(e, in_cap, &s->d_in)) || (rc = bcp_dev_alloc(e, out_cap, &s->d_out)) ||
        (rc = bcp_event_create(e, &s->ev_h)) || (rc = bcp_event_create(e, &s->ev_k)) ||
        (rc = bcp_event_create(e, &s->ev_d)))
        return rc;
    s->in_cap = in_cap;
    s->out_cap = out_cap;
    return 0;
}

static void slot_free(bcp_engine *e, slot *s)
{
    bcp_host_free(e, s->h_in);
    bcp_host_free(e, s->h_out);
    bcp_dev_free(e, s->d_in);
    bcp_dev_free(e, s->d_out);
    if (s->ev_h)
        bcp_event_destroy(s->ev_h);
    if (s->ev_k)
        bcp_event_destroy(s->ev_k);
    if (s->ev_d)
        bcp_event_destroy(s->ev_d);
}

/* One GPU of the pipeline: engine, h2d / compute / d2h queues, slots. */
typedef struct {
    bcp_engine *eng;
    bcp_queue *qh, *qk, *qd;
    bcp_queue *qr;        /* a repair run's launches and copies (completion thread); created by the first such run */
    slot *slots;
} dev_lane;

struct bcp_pipeline {
    bcp_pipeline_opts o;
    int read_mode;      /* BCP_READ_AUTO (decided per run), COPY or DIRECT */
    int ndev;
    dev_lane *dev;
    pool io, completer; /* io: 2 x io_threads threads, chunk reads ahead of parity writes */
    int pools;
    size_t in_cap, out_cap;
    bcp_stripe *st;
    bcp_source *so;
    bcp_stripe *st2;    /* the batch's P + Q stripes (a launch of their own) */
    bcp_source *so2;
    uint64_t *qd;
    bcp_pq_lost *lost;
    size_t desc_cap;    /* stripes the descriptor arrays hold */
    int q_on;           /* bcp_pipeline_set_q_parity */
    int q_win;          /* bcp_pipeline_set_q_windowed */
    int repair_win;     /* bcp_pipeline_set_repair_windowed */
    uint64_t q_written, q_no_target, q_windowed; /* of the last run */
    repair_ctx *repair; /* during a repair run (bcp_pipeline_repair_q) */
    uint8_t *r2_unrec;  /* during a rebuild2 run: per item, 1 = unrecoverable after the stat phase */
    bcp_pipeline_timing last; /* of the last run */
};

int bcp_pipeline_last_timing(const bcp_pipeline *pl, bcp_pipeline_timing *out)
{
    if (!pl || !out)
        return -EINVAL;
    *out = pl->last;
    return 0;
}

static void free_slots(bcp_pipeline *pl)
{
    for (int d = 0; d < pl->ndev; d++) {
        dev_lane *L = &pl->dev[d];
        if (!L->slots)
            continue;
        for (int s = 0; s < pl->o.nslots; s++)
            slot_free(L->eng, &L->slots[s]);
        free(L->slots);
        L->slots = NULL;
    }
}

int bcp_pipeline_destroy(bcp_pipeline *pl)
{
    if (!pl)
        return -EINVAL;
    /* only the pools that started (pool_start is all or nothing) */
    if (pl->pools & 2)
        pool_stop(&pl->completer);
    if (pl->pools & 1)
        pool_stop(&pl->io);
    if (pl->dev) {
        /* queues first (each synchronises its streams): no copy or kernel may
         * still use a slot when its memory goes */
        for (int d = 0; d < pl->ndev; d++) {
            dev_lane *L = &pl->dev[d];
            if (L->qh)
                bcp_queue_destroy(L->qh);
            if (L->qk)
                bcp_queue_destroy(L->qk);
            if (L->qd)
                bcp_queue_destroy(L->qd);
            if (L->qr)
                bcp_queue_destroy(L->qr);
            L->qh = L->qk = L->qd = L->qr = NULL;
        }
        free_slots(pl);
        for (int d = 0; d < pl->ndev; d++)
            if (pl->dev[d].eng)
                bcp_engine_destroy(pl->dev[d].eng);
        free(pl->dev);
    }
    free(pl->st);
    free(pl->so);
    free(pl->st2);
    free(pl->so2);
    free(pl->qd);
    free(pl->lost);
    free(pl);
    return 0;
}

static int ensure_slots(bcp_pipeline *pl, size_t in_cap, size_t out_cap)
{
    if (pl->dev[0].slots && in_cap <= pl->in_cap && out_cap <= pl->out_cap)
        return 0;
    free_slots(pl);
    in_cap = in_cap > pl->in_cap ? in_cap : pl->in_cap;
    out_cap = out_cap > pl->out_cap ? out_cap : pl->out_cap;
    for (int d = 0; d < pl->ndev; d++) {
        dev_lane *L = &pl->dev[d];
        L->slots = calloc((size_t)pl->o.nslots, sizeof(slot));
        if (!L->slots)
            return -ENOMEM;
        for (int s = 0; s < pl->o.nslots; s++) {
            int rc = slot_alloc(L->eng, &L->slots[s], in_cap, out_cap);
            if (rc)
                return rc;
        }
    }
    pl->in_cap = in_cap;
    pl->out_cap = out_cap;
    return 0;
}

/* CPUs this process may use: its affinity mask, capped by the cgroup's CPU
 * quota (v2 cpu.max, else v1 cfs). */
static int usable_cpus(void)
{
    cpu_set_t set;
    int n = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 0;
    if (n <= 0)
        n = (int)sysconf(_SC_NPROCESSORS_ONLN);
    long long q = -1, per = 0;
    FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r");
    if (f) {
        char qs[32];
        if (fscanf(f, "%31s %lld", qs, &per) == 2 && strcmp(qs, "max"))
            q = atoll(qs);
        fclose(f);
    } else if ((f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"))) {
        if (fscanf(f, "%lld", &q) != 1)
            q = -1;
        fclose(f);
        if ((f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r"))) {
            if (fscanf(f, "%lld", &per) != 1)
                per = 0;
            fclose(f);
        }
    }
    if (q > 0 && per > 0) {
        const long long c = (q + per / 2) / per;
        if (c >= 1 && c < n)
            n = (int)c;
    }
    return n > 0 ? n : 1;
}

int bcp_pipeline_create(const bcp_pipeline_opts *opts_in, bcp_pipeline **out)
{
    if (!out)
        return -EINVAL;
    *out = NULL;
    bcp_pipeline_opts o = {0, 256u << 20, 0, 4, 1, BCP_READ_AUTO};
    if (opts_in)
        o = *opts_in;
    /* 2 was the MAP read mode (ABI 2), removed in ABI 3: never chosen by
     * AUTO and level with or behind COPY */
    if (o.read_mode != BCP_READ_AUTO && o.read_mode != BCP_READ_COPY && o.read_mode != BCP_READ_DIRECT)
        return -EINVAL;
    if (o.read_mode == BCP_READ_AUTO) { /* stays AUTO (decided per run) unless the env names a mode */
        const char *env = getenv("BCP_PIPELINE_READ");
        o.read_mode = !env                     ? BCP_READ_AUTO
                      : !strcmp(env, "copy")   ? BCP_READ_COPY
                      : !strcmp(env, "direct") ? BCP_READ_DIRECT
                                               : BCP_READ_AUTO;
    }
    if (o.ndevices < 1)
        o.ndevices = 1;
    /* io threads 0 = auto: 8 per GPU, and the io pool twice that (reads and
     * writes share it, below).  One GPU's PCIe link takes what ~8 threads
     * copy out of the page cache (8 + 8 beat 16 + 16 on a 16-CPU share,
     * profiles/r02/protocol/pipeline_io_threads_ab_r2e4.jsonl), and every
     * further GPU brings its own link and its own CPU share -- but never more
     * than half the CPUs this process may run on, so the pool has no more
     * threads than CPUs: beyond that they only measure oversubscription. */
    if (o.io_threads == 0) {
        const int half = usable_cpus() / 2;
        o.io_threads = 8 * o.ndevices;
        if (o.io_threads > half)
            o.io_threads = half > 2 ? half : 2;
    }
    int ndev_vis = 0;
    bcp_device_count(&ndev_vis);
    if (o.device < 0 || o.ndevices > 64)
        return -EINVAL;
    if (o.slab_bytes < (1u << 20))
        o.slab_bytes = 1u << 20;
    if (o.io_threads < 1)
        o.io_threads = 1;
    if (o.io_threads > 64)
        o.io_threads = 64;
    if (o.nslots < 2)
        o.nslots = 2;
    if (o.nslots > 8)
        o.nslots = 8;
    bcp_pipeline *pl = calloc(1, sizeof(*pl));
    if (!pl)
        return -ENOMEM;
    pl->o = o;
    pl->read_mode = o.read_mode; /* AUTO: COPY or DIRECT, chosen per run (auto_read_mode) */
    int rc = 0;
    pl->dev = calloc((size_t)o.ndevices, sizeof(dev_lane));
    if (!pl->dev) {
        free(pl);
        return -ENOMEM;
    }
    pl->ndev = o.ndevices;
    for (int d = 0; d < pl->ndev; d++) {
        dev_lane *L = &pl->dev[d];
        /* devices wrap modulo the visible count: more lanes than GPUs runs
         * several lanes per GPU (how the multi-device path is tested on one) */
        const int dev = ndev_vis > 0 ? (o.device + d) % ndev_vis : o.device + d;
        if ((rc = bcp_engine_create(dev, &L->eng)) || (rc = bcp_queue_create(L->eng, &L->qh)) ||
            (rc = bcp_queue_create(L->eng, &L->qk)) || (rc = bcp_queue_create(L->eng, &L->qd)))
            goto fail;
    }
    /* One io pool of 2 x io_threads threads reads chunks and writes parity
     * files, reads first: the reads feed the link, a batch's writes only gate
     * its slot's reuse four batches later, and where the host's CPU time
     * bounds the run a thread never idles in one pool while the other has
     * work.  (Separate pools, writes first and push order measured within the
     * box-to-box spread of this order on six boxes and were removed in r05:
     * profiles/r04/pipeline/shared_io_ab*.jsonl) */
    if ((rc = pool_start(&pl->io, 2 * o.io_threads)))
        goto fail;
    pl->pools |= 1;
    if ((rc = pool_start(&pl->completer, 1)))
        goto fail;
    pl->pools |= 2;
    if ((rc = ensure_slots(pl, o.slab_bytes, o.slab_bytes)))
        goto fail;
    *out = pl;
    return 0;
fail:
    bcp_pipeline_destroy(pl);
    return rc;
}

static int pipeline_exec(bcp_pipeline *pl, const char *store_root, task *tasks, size_t nt, int corrupt_fd,
                         FILE *log, bcp_run_stats *stats, double t0, bcp_verify_item *vres,
                         bcp_verify_q_item *qres);

/* Bytes source k of t takes in the input slab: its data at 256-byte pitch
 * (COPY), or the whole file prefix up to the data's end at page pitch (DIRECT:
 * files are read from offset 0 into page-aligned slab offsets, the rebuild
 * parity body sits 8n in). */
static uint64_t span_of(const task *t, int k, int page_layout)
{
    if (!page_layout)
        return RUP(t->size[k]);
    return t->size[k] ? RUP_PAGE(t->src_off[k] + t->size[k]) : 0;
}

/* Where source k's data starts, relative to the slab. */
static uint64_t data_off(const task *t, int k, int page_layout)
{
    return t->in_off[k] + (page_layout ? t->src_off[k] : 0);
}

int bcp_pipeline_run(bcp_pipeline *pl, const char *store_root, int ntargets, const bcp_work_item *items,
                     size_t nitems, FILE *log, bcp_run_stats *stats)
{
    if (!pl || !store_root || ntargets < 1 || ntargets > MAX_STORAGE_TARGETS || (nitems && !items))
        return -EINVAL;
    double t0 = now_s();
    int rc = 0;

    /* validate everything before touching any file */
    for (size_t i = 0; i < nitems; i++) {
        uint64_t loc = items[i].fi.locations;
        int P = GET_P(loc);
        if ((uint64_t)P == NO_P)
            continue;
        if (!items[i].path || P >= ntargets || TEST_BIT(loc, P) || ((loc & L_MASK) >> ntargets))
            return -EINVAL;
    }
    /* tasks: skip NO_P, unlink deletes now (no data moves for them) */
    task *tasks = calloc(nitems ? nitems : 1, sizeof(task));
    if (!tasks)
        return -ENOMEM;
    size_t nt = 0;
    for (size_t i = 0; i < nitems; i++) {
        uint64_t loc = items[i].fi.locations;
        int P = GET_P(loc);
        if ((uint64_t)P == NO_P)
            continue;
        if (!bcpi_path_ok(items[i].path, (size_t)-1)) { /* as process_task: refused, skipped */
            if (log)
                fprintf(log, "bcp_pipeline: refusing '%s': not a path inside the store\n", items[i].path);
            continue;
        }
        const int qt = pl->q_on ? bcp_q_target(loc, ntargets) : -1;
        if ((loc & L_MASK) == 0) {
            char fn[4352];
            chunk_file(fn, sizeof(fn), store_root, P, "parity", items[i].path);
            unlink(fn);
            if (qt >= 0) {
                chunk_file(fn, sizeof(fn), store_root, qt, "parityq", items[i].path);
                unlink(fn);
            }
            continue;
        }
        task *t = &tasks[nt++];
        t->path = items[i].path;
        t->p = P;
        t->q_st = qt;
        for (int k = 0; k < MAX_STORAGE_TARGETS; k++)
            if (TEST_BIT(loc, k))
                t->holders[t->n++] = k;
    }
    rc = pipeline_exec(pl, store_root, tasks, nt, -1, log, stats, t0, NULL, NULL);
    free(tasks);
    if (stats)
        stats->refused = bcpr_count_refused(items, nitems, -1);
    return rc;
}

/* One batch between queueing its reads and submitting it. */
typedef struct {
    size_t first, last;        /* tasks */
    uint64_t in_used;          /* input bytes */
    int reads_live;            /* S->reads initialised and not yet waited for */
    dev_lane *L;
    slot *S;
} bstate;

/* AUTO's read path for one run: COPY where the chunks are in memory anyway
 * (tmpfs / ramfs, or a sample of the run's sources mostly resident in the
 * page cache -- just written, or read before), DIRECT for a cold store on a
 * disk, where O_DIRECT lets the storage device fill the slabs without a CPU
 * copy (1.1-1.4x).  The sample: the first 16 MiB of one
 * source in each of up to 64 tasks spread over the run, mincore() on a
 * mapping of it. */
/* Filesystem of every storage target's directory a run touches, looked up
 * once per run: <root>/st<k>/{chunks,parity} are often separate mounts, so
 * the choices below are made per target, never from the store root. */
typedef struct {
    signed char mem[MAX_STORAGE_TARGETS][3]; /* [k][0 chunks, 1 parity, 2 parityq]: 1 tmpfs / ramfs, 0 not, -1 unknown yet */
} fs_kinds;

static int dir_in_memory(fs_kinds *fk, const char *root, int k, int kind)
{
    signed char *m = &fk->mem[k][kind];
    if (*m < 0) {
        char dn[4352];
        snprintf(dn, sizeof(dn), "%s/st%d/%s", root, k, k_dir[kind]);
        struct statfs sf;
        *m = statfs(dn, &sf) == 0 && (sf.f_type == TMPFS_MAGIC || sf.f_type == RAMFS_MAGIC);
    }
    return *m;
}

/* AUTO's read path for one run: COPY where the chunks are in memory anyway
 * (every source directory of the run on tmpfs / ramfs, or a sample of the
 * run's sources mostly resident in the page cache -- just written, or read
 * before), DIRECT for a cold store on a disk, where O_DIRECT lets the storage
 * device fill the slabs without a CPU copy (1.1-1.4x).
 * The sample: the first 16 MiB of one source in each of up to 64 tasks spread
 * over the run, mincore() on a mapping of it. */
static int auto_read_mode(const char *root, const task *tasks, size_t nt, fs_kinds *fk)
{
    int all_mem = 1;
    for (size_t i = 0; i < nt && all_mem; i++)
        for (int k = 0; k < tasks[i].n && all_mem; k++)
            all_mem = dir_in_memory(fk, root, tasks[i].holders[k], src_kind(&tasks[i], k));
    if (all_mem)
        return BCP_READ_COPY;
    const uint64_t cap = (uint64_t)16 << 20;
    unsigned char *vec = malloc(cap / PAGE);
    if (!vec)
        return BCP_READ_COPY;
    uint64_t pages = 0, resident = 0;
    char fn[4352];
    for (size_t i = 0; i < nt; i += nt / 64 + 1) {
        const task *t = &tasks[i];
        for (int k = 0; k < t->n; k++) {
            if (!t->size[k])
                continue;
            chunk_file(fn, sizeof(fn), root, t->holders[k], k_dir[src_kind(t, k)], t->path);
            const uint64_t len = t->src_off[k] + t->size[k] < cap ? t->src_off[k] + t->size[k] : cap;
            int fd = open(fn, O_RDONLY);
            if (fd < 0)
                continue;
            void *m = mmap(NULL, (size_t)len, PROT_READ, MAP_SHARED, fd, 0);
            close(fd);
            if (m == MAP_FAILED)
                continue;
            const uint64_t np = (len + PAGE - 1) / PAGE;
            if (mincore(m, (size_t)len, vec) == 0) {
                pages += np;
                for (uint64_t q = 0; q < np; q++)
                    resident += vec[q] & 1;
            }
            munmap(m, (size_t)len);
            break; /* one source per sampled task */
        }
    }
    free(vec);
    return pages && resident * 2 < pages ? BCP_READ_DIRECT : BCP_READ_COPY;
}

/* Stat, batch and stream the tasks through the slots (both read paths).
 * Takes no ownership of tasks.  vres or qres: verify run (every task a verify
 * task; qres: with Q, every task vq): the verdicts of the work items, written
 * here for every task. */
static int pipeline_exec(bcp_pipeline *pl, const char *store_root, task *tasks, size_t nt, int corrupt_fd,
                         FILE *log, bcp_run_stats *stats, double t0, bcp_verify_item *vres,
                         bcp_verify_q_item *qres)
{
    fs_kinds fk;
    memset(&fk, -1, sizeof(fk));
    const int nslots = pl->o.nslots;
    int rc = 0, errors = 0, dev_rc = 0;
    uint64_t rd[3] = {0, 0, 0}, bytes_written = 0, ntasks = 0; /* rd: see read_arg.bytes */
    const double t_stat = now_s();
    memset(&pl->last, 0, sizeof(pl->last)); /* a run that fails early reports zeros, not the previous run */

    /* 1. stat every chunk (parallel) */
    {
        latch l;
        latch_init(&l, (long)nt);
        stat_arg *args = calloc(nt ? nt : 1, sizeof(stat_arg));
        if (!args) {
            latch_destroy(&l);
            return -ENOMEM;
        }
        for (size_t i = 0; i < nt; i++) {
            /* a run writes Q only with Q on; rebuild2 and verify_q read what is there */
            const int q_win = pl->q_win && (pl->q_on || tasks[i].rebuild || tasks[i].verify);
            args[i] = (stat_arg){{0}, store_root, &tasks[i], &l, corrupt_fd, q_win};
            pool_push(&pl->io, &args[i].j, do_stat);
        }
        latch_wait(&l);
        latch_destroy(&l);
        free(args);
    }
    const int verify = vres != NULL || qres != NULL;
    if (verify) {
        /* only the items that passed the stat phase are read and compared:
         * the others' verdicts stand, their tasks drop out (order kept) */
        size_t w = 0;
        for (size_t i = 0; i < nt; i++) {
            if (tasks[i].status != VERIFY_PENDING) {
                if (qres)
                    qres[tasks[i].item].status = tasks[i].status;
                else
                    vres[tasks[i].item].status = tasks[i].status;
                continue;
            }
            if (w != i)
                tasks[w] = tasks[i];
            w++;
        }
        nt = w;
    }
    if (pl->r2_unrec) {
        /* rebuild2: the items that cannot be recovered drop out (order kept);
         * nothing is read or written for them */
        size_t w = 0;
        for (size_t i = 0; i < nt; i++) {
            if (tasks[i].unrecov) {
                pl->r2_unrec[tasks[i].item] = 1;
                continue;
            }
            if (w != i)
                tasks[w] = tasks[i];
            w++;
        }
        nt = w;
    }
    /* the reference reserves every output's space first (task_processing.c:186),
     * except where that output's directory is tmpfs / ramfs (do_write) */
    for (size_t i = 0; i < nt && !verify; i++) {
        tasks[i].prealloc = !dir_in_memory(&fk, store_root, tasks[i].p, !tasks[i].rebuild);
        if (tasks[i].rebuild)
            tasks[i].has2 = tasks[i].pq == 2;
        if (tasks[i].has2)
            tasks[i].prealloc2 = !dir_in_memory(&fk, store_root, tasks[i].rebuild ? tasks[i].p2 : tasks[i].q_st,
                                                tasks[i].rebuild ? 0 : 2);
    }
    /* Q files of the run (bcp_pipeline_q_stats) */
    pl->q_written = pl->q_no_target = pl->q_windowed = 0;
    for (size_t i = 0; i < nt && pl->q_on && !verify; i++)
        if (!tasks[i].rebuild) {
            pl->q_written += tasks[i].q_st >= 0;
            pl->q_no_target += tasks[i].q_st == -1;
            pl->q_windowed += tasks[i].q_st == -2;
        }

    /* 2. plan batches: inputs at 256-byte pitch (DIRECT: page pitch), outputs
     * at 256 */
    const int mode = pl->read_mode == BCP_READ_AUTO ? auto_read_mode(store_root, tasks, nt, &fk) : pl->read_mode;
    const int dir = mode == BCP_READ_DIRECT; /* page layout */
    size_t in_cap = pl->in_cap, out_cap = pl->out_cap;
    for (size_t i = 0; i < nt; i++) {
        uint64_t in = 0;
        for (int k = 0; k < tasks[i].n; k++)
            in += span_of(&tasks[i], k, dir);
        if (in > in_cap)
            in_cap = (size_t)in;
        if (out_span(&tasks[i]) > out_cap)
            out_cap = (size_t)out_span(&tasks[i]);
    }
    if ((rc = ensure_slots(pl, in_cap, out_cap))) {
        return rc;
    }
    in_cap = pl->in_cap;
    out_cap = pl->out_cap;
    /* A small job (a changelog round's subset) cut at slab capacity makes a
     * few big batches: on ndev GPUs (batches go round-robin) most devices
     * would idle -- a 1 GiB round is 4 batches of 256 MiB for 8 GPUs.  Aim
     * for >= 4 batches per slot and device, >= 16 MiB each, never above the
     * slab (the largest task still fits, ensure_slots above).  On one GPU
     * this changed nothing measurable (r2av: the round's pipeline 48 ms vs
     * 46 before). */
    uint64_t plan_in = in_cap;
    {
        uint64_t total_in = 0, max_in = 0;
        for (size_t i = 0; i < nt; i++) {
            uint64_t in = 0;
            for (int k = 0; k < tasks[i].n; k++)
                in += span_of(&tasks[i], k, dir);
            total_in += in;
            max_in = in > max_in ? in : max_in;
        }
        const uint64_t want = (uint64_t)4 * (uint64_t)nslots * (uint64_t)pl->ndev;
        uint64_t per = total_in / want + 1;
        per = per < ((uint64_t)16 << 20) ? ((uint64_t)16 << 20) : per;
        plan_in = per < plan_in ? per : plan_in;
        plan_in = plan_in < max_in ? max_in : plan_in;
    }
    /* Ramps.  Once the reads outrun the link, the run is the host-to-device
     * copies back to back plus what cannot overlap them: the first batch's
     * reads before the first copy, and after the last copy the last batch's
     * kernel, D2H and parity writes.  Both scale with the batch, so batches
     * start at RAMP_MIN and double (a batch holds at most what the run has
     * consumed so far, per device) and end halving (at most half of what
     * remains, per device): r03 timing showed 6-10 ms of a 51 ms config-1
     * run spent in the drain behind 160 MiB batches. */
    const uint64_t RAMP_MIN = (uint64_t)16 << 20;
    uint64_t total_in_all = 0;
    for (size_t i = 0; i < nt; i++)
        for (int k = 0; k < tasks[i].n; k++)
            total_in_all += span_of(&tasks[i], k, dir);
    int nbatches = 0;
    {
        uint64_t in_used = 0, out_used = 0, consumed = 0, limit = plan_in;
        for (size_t i = 0; i < nt; i++) {
            task *t = &tasks[i];
            uint64_t in = 0;
            for (int k = 0; k < t->n; k++)
                in += span_of(t, k, dir);
            if (i == 0 || in_used + in > limit || out_used + out_span(t) > out_cap) {
                nbatches++;
                consumed += in_used;
                in_used = out_used = 0;
                const uint64_t up = consumed / (uint64_t)pl->ndev;
                const uint64_t down = (total_in_all - consumed) / (2u * (uint64_t)pl->ndev);
                limit = up < down ? up : down;
                limit = limit < RAMP_MIN ? RAMP_MIN : limit;
                limit = limit > plan_in ? plan_in : limit;
            }
            t->batch = nbatches - 1;
            for (int k = 0; k < t->n; k++) {
                t->in_off[k] = in_used;
                in_used += span_of(t, k, dir);
            }
            t->out_off = out_used;
            out_used += out_span(t);
        }
    }
    if (pl->desc_cap < nt) {
        free(pl->st);
        free(pl->so);
        free(pl->st2);
        free(pl->so2);
        free(pl->qd);
        free(pl->lost);
        pl->st = malloc((nt ? nt : 1) * sizeof(bcp_stripe));
        pl->so = malloc((nt ? nt : 1) * MAX_STORAGE_TARGETS * sizeof(bcp_source));
        /* the batch's P + Q stripes (gen with Q, rebuild2) go in a launch of their own */
        pl->st2 = malloc((nt ? nt : 1) * sizeof(bcp_stripe));
        pl->so2 = malloc((nt ? nt : 1) * MAX_STORAGE_TARGETS * sizeof(bcp_source));
        pl->qd = malloc((nt ? nt : 1) * sizeof(uint64_t));
        pl->lost = malloc((nt ? nt : 1) * sizeof(bcp_pq_lost));
        pl->desc_cap = (pl->st && pl->so && pl->st2 && pl->so2 && pl->qd && pl->lost) ? nt : 0;
        if (!pl->desc_cap) {
            return -ENOMEM;
        }
    }
    bcp_stripe *st = pl->st;
    bcp_source *so = pl->so;
    /* every job of the run, before the first one is queued: a read job per
     * piece of every source, a write job per task, a completion per batch */
    size_t nreads_all = 0;
    for (size_t i = 0; i < nt; i++)
        for (int k = 0; k < tasks[i].n; k++)
            nreads_all += (size_t)pieces_of(read_extent(&tasks[i], k, dir));
    read_arg *ra = calloc(nreads_all ? nreads_all : 1, sizeof(read_arg));
    write_arg *wa = calloc(nt ? 2 * nt : 1, sizeof(write_arg));
    complete_arg *cargs = calloc(nbatches ? (size_t)nbatches : 1, sizeof(complete_arg));
    bstate *bs = calloc(nbatches ? (size_t)nbatches : 1, sizeof(bstate));
    if (!ra || !wa || !cargs || !bs) {
        free(ra);
        free(wa);
        free(cargs);
        free(bs);
        return -ENOMEM;
    }
    size_t rnext = 0;
    bcp_pipeline_timing tm = {0};
    tm.stat = now_s() - t_stat;
    tm.batches = (uint32_t)nbatches;

    /* 3. stream the batches through the slots.  Batch b+1's reads are
     * queued before the host waits for batch b's, so the io threads go from
     * one batch to the next without idling at a batch's last chunks; b is on
     * the device meanwhile and earlier batches are being written (4 slots by
     * default: a slot's parity writes gate its reuse). */
    {
        size_t first = 0;
        for (int b = 0; b < nbatches; b++) {
            bs[b].first = first;
            while (first < nt && tasks[first].batch == b)
                first++;
            bs[b].last = first;
        }
    }
    int started = 0; /* batches whose reads are queued */
    for (int b = 0; b < nbatches && !rc; b++) {
        /* queue batch b+1's reads into its slot (after the slot's previous
         * batch has been written), ahead of every queued parity write */
        for (; started < nbatches && started <= b + 1; started++) {
            bstate *B = &bs[started];
            B->L = &pl->dev[started % pl->ndev];
            B->S = &B->L->slots[(started / pl->ndev) % nslots];
            double tw = now_s();
            if (B->S->busy) { /* writes of batch started - nslots still running */
                latch_wait(&B->S->writes);
                latch_destroy(&B->S->writes);
                B->S->busy = 0;
            }
            tm.slot_wait += now_s() - tw;
            uint64_t in_used = 0;
            long nreads = 0;
            for (size_t i = B->first; i < B->last; i++)
                for (int k = 0; k < tasks[i].n; k++) {
                    const uint64_t end = tasks[i].in_off[k] + span_of(&tasks[i], k, dir);
                    if (end > in_used)
                        in_used = end;
                    nreads += (long)pieces_of(read_extent(&tasks[i], k, dir));
                }
            B->in_used = in_used;
            latch_init(&B->S->reads, nreads);
            B->reads_live = 1;
            for (size_t i = B->first; i < B->last; i++)
                for (int k = 0; k < tasks[i].n; k++) {
                    const uint64_t e = read_extent(&tasks[i], k, dir);
                    uint8_t *d = B->S->h_in + (dir ? tasks[i].in_off[k] : data_off(&tasks[i], k, dir));
                    for (uint64_t o = 0; o < e; o += PIECE) {
                        read_arg *a = &ra[rnext++];
                        *a = (read_arg){{0}, store_root, &tasks[i], k, o, e - o < PIECE ? e - o : PIECE, d + o, rd,
                                        &B->S->reads, dir, verify ? &errors : NULL};
                        pool_push_hi(&pl->io, &a->j, do_read);
                    }
                }
            tm.read_jobs += (uint32_t)nreads;
        }
        bstate *B = &bs[b];
        dev_lane *L = B->L;
        slot *S = B->S;
        const uint64_t in_used = B->in_used;
        const size_t first = B->first, last = B->last;
        const double t_wait0 = now_s();
        latch_wait(&S->reads);
        latch_destroy(&S->reads);
        B->reads_live = 0;
        const double ts = now_s();
        tm.read_wait += ts - t_wait0; /* blocked on this batch's reads */
        uint32_t ns = 0, nsrc = 0, ns2 = 0, nsrc2 = 0;
        uint64_t out_used = 0;
        long nwrites = 0;
        int recover = 0;
        int win2 = 0; /* a windowed stripe among the P + Q ones: the _win entry points */
        /* verify with Q: the batch's syndrome records first, then the P check's */
        uint64_t nchk = 0;
        for (size_t i = first; i < last && qres; i++)
            nchk += tasks[i].q_state == BCP_QSTATE_CHECKED;
        for (size_t i = first; i < last; i++) {
            task *t = &tasks[i];
            nwrites += 1 + t->has2;
            if (t->vq && t->q_state == BCP_QSTATE_CHECKED) {
                /* dst and qd are the P and Q bodies in the input slab (only
                 * read), the sources the chunks in holder order */
                const int nfold = t->parity_src;
                t->out_off = (uint64_t)ns2 * sizeof(bcp_pq_check_result);
                pl->st2[ns2] = (bcp_stripe){(uint64_t)S->d_in + data_off(t, nfold, dir), t->out_len, nsrc2, (uint32_t)nfold,
                                            t->max_cs > WINDOW ? WINDOW : 0};
                win2 |= t->max_cs > WINDOW;
                pl->qd[ns2] = (uint64_t)S->d_in + data_off(t, t->q_src, dir);
                for (int k = 0; k < nfold; k++)
                    pl->so2[nsrc2++] = (bcp_source){(uint64_t)S->d_in + data_off(t, k, dir), t->size[k]};
                ns2++;
                if (t->out_off + sizeof(bcp_pq_check_result) > out_used)
                    out_used = t->out_off + sizeof(bcp_pq_check_result);
                continue;
            }
            if (t->vq) {
                t->out_off = nchk * sizeof(bcp_pq_check_result) + (uint64_t)ns * sizeof(bcp_check_result);
                if (t->out_off + sizeof(bcp_check_result) > out_used)
                    out_used = t->out_off + sizeof(bcp_check_result);
            }
            if (t->pq) {
                /* the survivors in position order, the victims' positions empty */
                recover = 1;
                bcp_pq_lost *l = &pl->lost[ns2];
                memset(l, 0, sizeof(*l));
                l->p = t->parity_src >= 0 ? (uint64_t)S->d_in + data_off(t, t->parity_src, dir) : 0;
                l->q = (uint64_t)S->d_in + data_off(t, t->q_src, dir);
                l->x = (uint32_t)t->lost_pos[0];
                l->y = t->pq == 2 ? (uint32_t)t->lost_pos[1] : BCP_PQ_NONE;
                l->dst_x = (uint64_t)S->d_out + t->out_off;
                l->len_x = t->out_len;
                l->dst_y = (uint64_t)S->d_out + out_off2(t);
                l->len_y = t->out_len2;
                pl->st2[ns2] = (bcp_stripe){0, t->max_cs, nsrc2, (uint32_t)t->width, t->max_cs > WINDOW ? WINDOW : 0};
                win2 |= t->max_cs > WINDOW;
                for (int j = 0; j < t->width; j++)
                    pl->so2[nsrc2 + j] = (bcp_source){0, 0};
                for (int k = 0; k < t->n; k++)
                    if (k != t->parity_src && k != t->q_src)
                        pl->so2[nsrc2 + t->src_pos[k]] = (bcp_source){(uint64_t)S->d_in + data_off(t, k, dir), t->size[k]};
                nsrc2 += (uint32_t)t->width;
                ns2++;
                if (t->out_off + out_span(t) > out_used)
                    out_used = t->out_off + out_span(t);
                continue;
            }
            if (t->has2) {
                /* gen with a Q file: P and Q in one pass, sources in holder order */
                pl->st2[ns2] = (bcp_stripe){(uint64_t)S->d_out + t->out_off, t->out_len, nsrc2, (uint32_t)t->n,
                                            t->max_cs > WINDOW ? WINDOW : 0};
                win2 |= t->max_cs > WINDOW;
                pl->qd[ns2] = (uint64_t)S->d_out + out_off2(t);
                for (int k = 0; k < t->n; k++)
                    pl->so2[nsrc2++] = (bcp_source){(uint64_t)S->d_in + data_off(t, k, dir), t->size[k]};
                ns2++;
                if (t->out_off + out_span(t) > out_used)
                    out_used = t->out_off + out_span(t);
                continue;
            }
            /* verify: dst is the parity body in the input slab (only read), the
             * sources are the chunks before it */
            const int nfold = verify ? t->parity_src : t->n;
            const uint64_t dst = verify ? (uint64_t)S->d_in + data_off(t, nfold, dir) : (uint64_t)S->d_out + t->out_off;
            st[ns] = (bcp_stripe){dst, t->out_len, nsrc, (uint32_t)nfold, t->max_cs > WINDOW ? WINDOW : 0};
            for (int k = 0; k < nfold; k++)
                so[nsrc++] = (bcp_source){(uint64_t)S->d_in + data_off(t, k, dir), t->size[k]};
            ns++;
            if (!t->vq && t->out_off + out_span(t) > out_used)
                out_used = t->out_off + out_span(t);
        }
        /* device: H2D (side queue) -> kernel -> D2H (side queue) */
        if ((in_used && (rc = bcp_h2d_async(L->qh, S->d_in, S->h_in, (size_t)in_used))) ||
            (rc = bcp_event_record(S->ev_h, L->qh)) || (rc = bcp_queue_wait_event(L->qk, S->ev_h)) ||
            (rc = verify ? bcp_check_stripes_async(L->qk, st, ns, so, nsrc,
                                                   (bcp_check_result *)((uint8_t *)S->d_out +
                                                                        nchk * sizeof(bcp_pq_check_result)))
                         : bcp_xor_stripes_async(L->qk, st, ns, so, nsrc)) ||
            (ns2 && !win2 &&
             (rc = qres      ? bcp_pq_check_stripes_async(L->qk, pl->st2, ns2, pl->so2, nsrc2, pl->qd,
                                                          (bcp_pq_check_result *)S->d_out)
                   : recover ? bcp_pq_recover_stripes_async(L->qk, pl->st2, ns2, pl->so2, nsrc2, pl->lost)
                             : bcp_pq_stripes_async(L->qk, pl->st2, ns2, pl->so2, nsrc2, pl->qd))) ||
            (ns2 && win2 &&
             (rc = qres      ? bcp_pq_check_stripes_win_async(L->qk, pl->st2, ns2, pl->so2, nsrc2, pl->qd,
                                                              (bcp_pq_check_result *)S->d_out)
                   : recover ? bcp_pq_recover_stripes_win_async(L->qk, pl->st2, ns2, pl->so2, nsrc2, pl->lost)
                             : bcp_pq_stripes_win_async(L->qk, pl->st2, ns2, pl->so2, nsrc2, pl->qd))) ||
            (rc = bcp_event_record(S->ev_k, L->qk)) ||
            (rc = bcp_queue_wait_event(L->qd, S->ev_k)) ||
            (rc = bcp_d2h_async(L->qd, S->h_out, S->d_out, (size_t)out_used)) ||
            (rc = bcp_event_record(S->ev_d, L->qd)))
            break;
        /* writes start once the batch's D2H is done (completion thread); the
         * host moves on to batch b+1 meanwhile */
        latch_init(&S->writes, verify ? (long)(last - first) : nwrites);
        S->busy = 1;
        complete_arg *ca = &cargs[b];
        *ca = (complete_arg){{0}, S, store_root, tasks, wa, first, last, &pl->io, log, &errors, &dev_rc,
                             qres ? pl->repair : NULL, L->eng, L->qr, dir};
        pool_push(&pl->completer, &ca->j, do_complete);
        for (size_t i = first; i < last && !verify; i++)
            bytes_written += (tasks[i].rebuild ? 0 : 8u * (uint64_t)tasks[i].n) + tasks[i].out_len +
                             (!tasks[i].has2         ? 0
                              : tasks[i].rebuild ? tasks[i].out_len2
                                                 : 8u * (uint64_t)tasks[i].n + tasks[i].out_len2);
        ntasks += last - first;
        tm.submit += now_s() - ts;
    }
    /* a failed submission leaves batch b+1's reads queued: let them finish
     * before the slab and the jobs go away */
    for (int b = 0; b < started; b++)
        if (bs[b].reads_live) {
            latch_wait(&bs[b].S->reads);
            latch_destroy(&bs[b].S->reads);
            bs[b].reads_live = 0;
        }
    free(bs);
    const double td = now_s();
    for (int d = 0; d < pl->ndev; d++)
        for (int s = 0; s < nslots; s++) {
            slot *S = &pl->dev[d].slots[s];
            if (S->busy) {
                latch_wait(&S->writes);
                latch_destroy(&S->writes);
                S->busy = 0;
            }
        }
    /* after a failed submission part of a batch may still be on the device:
     * nothing of this run stays in flight on the slots past its return */
    for (int d = 0; d < pl->ndev; d++) {
        dev_lane *L = &pl->dev[d];
        const int s1 = bcp_queue_sync(L->qh), s2 = bcp_queue_sync(L->qk), s3 = bcp_queue_sync(L->qd);
        if (!rc && !dev_rc)
            dev_rc = s1 ? s1 : s2 ? s2 : s3;
    }
    /* every job has run: the writes latched above, the completions before them */
    free(ra);
    free(wa);
    free(cargs);
    tm.drain = now_s() - td;
    tm.read_mode = mode;
    tm.direct_bytes = rd[1];
    tm.direct_fallbacks = (uint32_t)rd[2];
    pl->last = tm;
    if (!rc && dev_rc)
        rc = dev_rc;
    for (size_t i = 0; i < nt && qres; i++) {
        const task *t = &tasks[i];
        bcp_verify_q_item *v = &qres[t->item];
        if (t->status == VERIFY_PENDING) { /* its batch never came back */
            v->status = BCP_VERIFY_SKIPPED;
            errors++;
            continue;
        }
        v->status = t->status;
        v->q_state = t->q_state;
        if (t->status != BCP_VERIFY_MISMATCH)
            continue;
        v->first_bad = t->first_bad;
        v->p_bad = t->bad_bytes;
        v->culprit = BCP_CULPRIT_MANY; /* the P check alone names nobody */
        if (t->q_state == BCP_QSTATE_CHECKED) {
            const bcp_pq_check_result r = {t->first_bad, t->bad_bytes, t->q_bad, t->members};
            int pos = -1;
            v->q_bad = t->q_bad;
            v->culprit = (uint32_t)bcp_pq_culprit(&r, &pos);
            v->target = v->culprit == BCP_CULPRIT_DATA && pos < t->parity_src ? t->holders[pos]
                        : v->culprit == BCP_CULPRIT_P                         ? t->p
                        : v->culprit == BCP_CULPRIT_Q                         ? t->q_st
                                                                              : -1;
        }
    }
    for (size_t i = 0; i < nt && vres; i++) {
        bcp_verify_item *v = &vres[tasks[i].item];
        if (tasks[i].status == VERIFY_PENDING) { /* its batch never came back */
            v->status = BCP_VERIFY_SKIPPED;
            errors++;
            continue;
        }
        v->status = tasks[i].status;
        if (tasks[i].status == BCP_VERIFY_MISMATCH) {
            v->first_bad = tasks[i].first_bad;
            v->bad_bytes = tasks[i].bad_bytes;
        }
    }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->seconds = now_s() - t0;
        stats->tasks = ntasks;
        stats->bytes_read = rd[0];
        stats->bytes_written = bytes_written;
        stats->errors = errors;
    }
    return rc;
}

int bcp_pipeline_rebuild(bcp_pipeline *pl, const char *store_root, int ntargets, int rebuild_target,
                         const bcp_work_item *items, size_t nitems, const char *corrupt_list_path, FILE *log,
                         bcp_run_stats *stats)
{
    if (!pl || !store_root || ntargets < 2 || ntargets > MAX_STORAGE_TARGETS || rebuild_target < 0 ||
        rebuild_target >= ntargets || (nitems && !items))
        return -EINVAL;
    double t0 = now_s();
    for (size_t i = 0; i < nitems; i++) {
        uint64_t loc = items[i].fi.locations;
        int P = GET_P(loc);
        if ((uint64_t)P == NO_P)
            continue;
        if (!items[i].path || P >= ntargets || TEST_BIT(loc, P) || ((loc & L_MASK) >> ntargets))
            return -EINVAL;
    }
    int corrupt_fd = -1;
    if (corrupt_list_path) {
        corrupt_fd = open(corrupt_list_path, O_WRONLY | O_CREAT | O_TRUNC | O_APPEND, S_IRUSR | S_IWUSR);
        if (corrupt_fd < 0)
            return -errno;
    }
    task *tasks = calloc(nitems ? nitems : 1, sizeof(task));
    if (!tasks) {
        if (corrupt_fd >= 0)
            close(corrupt_fd);
        return -ENOMEM;
    }
    size_t nt = 0;
    for (size_t i = 0; i < nitems; i++) {
        const FileInfo *fi = &items[i].fi;
        const int P = GET_P(fi->locations);
        /* do_file's skip rules (rebuild/main.c:48-51) */
        if ((uint64_t)P == NO_P || P == rebuild_target || !TEST_BIT(fi->locations, rebuild_target))
            continue;
        if (!bcpi_path_ok(items[i].path, (size_t)-1)) { /* as process_task: refused, skipped */
            if (log)
                fprintf(log, "bcp_pipeline: refusing '%s': not a path inside the store\n", items[i].path);
            continue;
        }
        task *t = &tasks[nt++];
        t->path = items[i].path;
        t->p = rebuild_target;
        t->q_st = -1;
        t->rebuild = 1;
        t->timestamp = fi->timestamp;
        /* sources: the surviving holders and the parity holder, ascending
         * (the re-roled locations of rebuild/main.c:55-60) */
        const uint64_t src = ((fi->locations & L_MASK) | (UINT64_C(1) << P)) & ~(UINT64_C(1) << rebuild_target);
        t->parity_src = -1;
        for (int k = 0; k < MAX_STORAGE_TARGETS; k++)
            if (TEST_BIT(src, k)) {
                if (k == P)
                    t->parity_src = t->n;
                t->holders[t->n++] = k;
            }
    }
    int rc = pipeline_exec(pl, store_root, tasks, nt, corrupt_fd, log, stats, t0, NULL, NULL);
    free(tasks);
    if (stats)
        stats->refused = bcpr_count_refused(items, nitems, rebuild_target);
    if (corrupt_fd >= 0)
        close(corrupt_fd);
    return rc;
}

int bcp_pipeline_verify(bcp_pipeline *pl, const char *store_root, int ntargets, const bcp_work_item *items,
                        size_t nitems, bcp_verify_item *results, const char *bad_list_path, FILE *log,
                        bcp_verify_stats *stats)
{
    if (!pl || !store_root || ntargets < 1 || ntargets > MAX_STORAGE_TARGETS || (nitems && !items))
        return -EINVAL;
    double t0 = now_s();
    for (size_t i = 0; i < nitems; i++) {
        uint64_t loc = items[i].fi.locations;
        int P = GET_P(loc);
        if ((uint64_t)P == NO_P)
            continue;
        if (!items[i].path || P >= ntargets || TEST_BIT(loc, P) || ((loc & L_MASK) >> ntargets))
            return -EINVAL;
    }
    bcp_verify_item *res = results ? results : calloc(nitems ? nitems : 1, sizeof(*res));
    task *tasks = calloc(nitems ? nitems : 1, sizeof(task));
    int bad_fd = -1, rc = 0;
    if (!res || !tasks) {
        rc = -ENOMEM;
        goto out;
    }
    if (bad_list_path) {
        bad_fd = open(bad_list_path, O_WRONLY | O_CREAT | O_TRUNC | O_APPEND, S_IRUSR | S_IWUSR);
        if (bad_fd < 0) {
            rc = -errno;
            goto out;
        }
    }
    uint64_t refused = 0;
    size_t nt = 0;
    for (size_t i = 0; i < nitems; i++) {
        const FileInfo *fi = &items[i].fi;
        const int P = GET_P(fi->locations);
        res[i] = (bcp_verify_item){BCP_VERIFY_SKIPPED, 0, UINT64_MAX, 0};
        if ((uint64_t)P == NO_P || (fi->locations & L_MASK) == 0)
            continue;
        if (!bcpi_path_ok(items[i].path, (size_t)-1)) {
            if (log)
                fprintf(log, "bcp_pipeline: refusing '%s': not a path inside the store\n", items[i].path);
            refused++;
            continue;
        }
        task *t = &tasks[nt++];
        t->path = items[i].path;
        t->p = P;
        t->q_st = -1;
        t->verify = 1;
        t->item = i;
        t->timestamp = fi->timestamp;
        for (int k = 0; k < MAX_STORAGE_TARGETS; k++)
            if (TEST_BIT(fi->locations, k))
                t->holders[t->n++] = k;
        t->parity_src = t->n; /* the body: the last source, held by P */
        t->holders[t->n++] = P;
    }
    bcp_run_stats rs = {0};
    rc = pipeline_exec(pl, store_root, tasks, nt, -1, log, &rs, t0, res, NULL);
    bcp_verify_stats vs = {0};
    vs.items = nitems;
    vs.refused = refused;
    vs.bytes_read = rs.bytes_read;
    vs.errors = rs.errors + (rc != 0);
    for (size_t i = 0; i < nitems; i++) {
        switch (res[i].status) {
        case BCP_VERIFY_OK: vs.ok++; break;
        case BCP_VERIFY_STALE: vs.stale++; break;
        case BCP_VERIFY_NO_PARITY: vs.no_parity++; break;
        case BCP_VERIFY_SIZE: vs.size++; break;
        case BCP_VERIFY_MISMATCH: vs.mismatch++; break;
        default: vs.skipped++; break;
        }
        /* the bad list after the run, in item order */
        if (res[i].status == BCP_VERIFY_NO_PARITY || res[i].status == BCP_VERIFY_SIZE ||
            res[i].status == BCP_VERIFY_MISMATCH)
            push_corrupt(bad_fd, items[i].path);
    }
    vs.seconds = now_s() - t0;
    if (stats)
        *stats = vs;
out:
    if (bad_fd >= 0)
        close(bad_fd);
    free(tasks);
    if (res != results)
        free(res);
    return rc;
}

/* One line of the culprit list, written whole. */
static void push_culprit(int fd, const char *path, uint32_t culprit, int target)
{
    static const char *const kind[] = {"many", "data", "p", "q", "many"};
    if (fd < 0)
        return;
    const size_t cap = strlen(path) + 32;
    char *line = malloc(cap);
    if (!line)
        return;
    const int len = snprintf(line, cap, "%s\t%s\t%d\n", path, kind[culprit <= BCP_CULPRIT_MANY ? culprit : 0], target);
    ssize_t w = write(fd, line, (size_t)len);
    (void)w;
    free(line);
}

int bcp_pipeline_verify_q(bcp_pipeline *pl, const char *store_root, int ntargets, const bcp_work_item *items,
                          size_t nitems, bcp_verify_q_item *results, const char *bad_list_path,
                          const char *culprit_list_path, FILE *log, bcp_verify_q_stats *stats)
{
    if (!pl || !store_root || ntargets < 1 || ntargets > MAX_STORAGE_TARGETS || (nitems && !items))
        return -EINVAL;
    double t0 = now_s();
    for (size_t i = 0; i < nitems; i++) {
        uint64_t loc = items[i].fi.locations;
        int P = GET_P(loc);
        if ((uint64_t)P == NO_P)
            continue;
        if (!items[i].path || P >= ntargets || TEST_BIT(loc, P) || ((loc & L_MASK) >> ntargets))
            return -EINVAL;
    }
    bcp_verify_q_item *res = results ? results : calloc(nitems ? nitems : 1, sizeof(*res));
    task *tasks = calloc(nitems ? nitems : 1, sizeof(task));
    int bad_fd = -1, culprit_fd = -1, rc = 0;
    if (!res || !tasks) {
        rc = -ENOMEM;
        goto out;
    }
    if (bad_list_path) {
        bad_fd = open(bad_list_path, O_WRONLY | O_CREAT | O_TRUNC | O_APPEND, S_IRUSR | S_IWUSR);
        if (bad_fd < 0) {
            rc = -errno;
            goto out;
        }
    }
    if (culprit_list_path) {
        culprit_fd = open(culprit_list_path, O_WRONLY | O_CREAT | O_TRUNC | O_APPEND, S_IRUSR | S_IWUSR);
        if (culprit_fd < 0) {
            rc = -errno;
            goto out;
        }
    }
    uint64_t refused = 0;
    size_t nt = 0;
    for (size_t i = 0; i < nitems; i++) {
        const FileInfo *fi = &items[i].fi;
        const int P = GET_P(fi->locations);
        res[i] = (bcp_verify_q_item){BCP_VERIFY_SKIPPED, BCP_QSTATE_NONE, BCP_CULPRIT_NONE, -1, UINT64_MAX, 0, 0};
        if ((uint64_t)P == NO_P || (fi->locations & L_MASK) == 0)
            continue;
        if (!bcpi_path_ok(items[i].path, (size_t)-1)) {
            if (log)
                fprintf(log, "bcp_pipeline: refusing '%s': not a path inside the store\n", items[i].path);
            refused++;
            continue;
        }
        task *t = &tasks[nt++];
        t->path = items[i].path;
        t->p = P;
        t->q_st = bcp_q_target(fi->locations, ntargets);
        t->vq = 1;
        t->q_state = BCP_QSTATE_NONE;
        t->verify = 1;
        t->item = i;
        t->timestamp = fi->timestamp;
        for (int k = 0; k < MAX_STORAGE_TARGETS; k++)
            if (TEST_BIT(fi->locations, k))
                t->holders[t->n++] = k;
        t->parity_src = t->n; /* the P body, held by P; a Q body follows it (do_stat) */
        t->holders[t->n++] = P;
    }
    bcp_run_stats rs = {0};
    rc = pipeline_exec(pl, store_root, tasks, nt, -1, log, &rs, t0, NULL, res);
    bcp_verify_q_stats vs;
    memset(&vs, 0, sizeof(vs));
    vs.v.items = nitems;
    vs.v.refused = refused;
    vs.v.bytes_read = rs.bytes_read;
    vs.v.errors = rs.errors + (rc != 0);
    for (size_t i = 0; i < nitems; i++) {
        const bcp_verify_q_item *v = &res[i];
        const int compared = v->status == BCP_VERIFY_OK || v->status == BCP_VERIFY_MISMATCH;
        switch (v->status) {
        case BCP_VERIFY_OK: vs.v.ok++; break;
        case BCP_VERIFY_STALE: vs.v.stale++; break;
        case BCP_VERIFY_NO_PARITY: vs.v.no_parity++; break;
        case BCP_VERIFY_SIZE: vs.v.size++; break;
        case BCP_VERIFY_MISMATCH: vs.v.mismatch++; break;
        default: vs.v.skipped++; break;
        }
        if (compared) {
            vs.q_checked += v->q_state == BCP_QSTATE_CHECKED;
            vs.q_none += v->q_state == BCP_QSTATE_NONE;
            vs.q_bad += v->q_state == BCP_QSTATE_BAD;
        }
        /* both lists after the run, in item order */
        if (v->status == BCP_VERIFY_NO_PARITY || v->status == BCP_VERIFY_SIZE || v->status == BCP_VERIFY_MISMATCH ||
            (compared && v->q_state == BCP_QSTATE_BAD))
            push_corrupt(bad_fd, items[i].path);
        if (v->status == BCP_VERIFY_MISMATCH) {
            vs.culprit_data += v->culprit == BCP_CULPRIT_DATA;
            vs.culprit_p += v->culprit == BCP_CULPRIT_P;
            vs.culprit_q += v->culprit == BCP_CULPRIT_Q;
            vs.culprit_many += v->culprit == BCP_CULPRIT_MANY;
            push_culprit(culprit_fd, items[i].path, v->culprit, v->target);
        }
    }
    vs.v.seconds = now_s() - t0;
    if (stats)
        *stats = vs;
out:
    if (bad_fd >= 0)
        close(bad_fd);
    if (culprit_fd >= 0)
        close(culprit_fd);
    free(tasks);
    if (res != results)
        free(res);
    return rc;
}

/* The scrub with repair: bcp_pipeline_verify_q's run with the repair stage in
 * its completions (repair_batch), so the verdicts and both lists are that
 * function's own. */
int bcp_pipeline_repair_q(bcp_pipeline *pl, const char *store_root, int ntargets, const bcp_work_item *items,
                          size_t nitems, int mode, uint32_t max_members, int dry_run, bcp_repair_q_item *results,
                          const char *bad_list_path, const char *culprit_list_path, const char *repaired_list_path,
                          FILE *log, bcp_repair_q_stats *stats)
{
    if (!pl || (mode != BCP_REPAIR_PARITY && mode != BCP_REPAIR_ALL) || max_members < 1)
        return -EINVAL;
    int rc = 0;
    for (int d = 0; d < pl->ndev && !rc; d++)
        if (!pl->dev[d].qr)
            rc = bcp_queue_create(pl->dev[d].eng, &pl->dev[d].qr);
    if (rc)
        return rc;
    bcp_repair_q_item *res = results ? results : calloc(nitems ? nitems : 1, sizeof(*res));
    bcp_verify_q_item *vq = calloc(nitems ? nitems : 1, sizeof(*vq));
    repair_ctx R = {mode, dry_run != 0, pl->repair_win, max_members, res, -1, 0, 0, 0, 0};
    if (!res || !vq) {
        rc = -ENOMEM;
        goto out;
    }
    memset(res, 0, (nitems ? nitems : 1) * sizeof(*res));
    if (repaired_list_path) {
        R.list_fd = open(repaired_list_path, O_WRONLY | O_CREAT | O_TRUNC | O_APPEND, S_IRUSR | S_IWUSR);
        if (R.list_fd < 0) {
            rc = -errno;
            goto out;
        }
    }
    bcp_repair_q_stats rs;
    memset(&rs, 0, sizeof(rs));
    pl->repair = &R;
    rc = bcp_pipeline_verify_q(pl, store_root, ntargets, items, nitems, vq, bad_list_path, culprit_list_path, log, &rs.q);
    pl->repair = NULL;
    if (rc == -EINVAL || rc == -ENOMEM) /* (refused before anything ran: no verdicts) */
        goto out;
    for (size_t i = 0; i < nitems; i++) {
        bcp_repair_q_item *v = &res[i];
        v->status = vq[i].status;
        v->q_state = vq[i].q_state;
        v->culprit = vq[i].culprit;
        v->target = vq[i].target;
        v->first_bad = vq[i].first_bad;
        v->p_bad = vq[i].p_bad;
        v->q_bad = vq[i].q_bad;
        if (v->status != BCP_VERIFY_MISMATCH)
            v->repair = BCP_REPAIRED_NONE;
        else if (v->repair == BCP_REPAIRED_NONE || v->repair == REPAIR_PENDING) { /* its repair stage never ran */
            v->repair = BCP_REPAIRED_FAILED;
            R.errors++;
        }
        rs.none += v->repair == BCP_REPAIRED_NONE;
        rs.done += v->repair == BCP_REPAIRED_DONE;
        rs.dry += v->repair == BCP_REPAIRED_DRY;
        rs.policy += v->repair == BCP_REPAIRED_POLICY;
        rs.unlocated += v->repair == BCP_REPAIRED_UNLOCATED;
        rs.changed += v->repair == BCP_REPAIRED_CHANGED;
        rs.failed += v->repair == BCP_REPAIRED_FAILED;
    }
    rs.q.v.errors += R.errors;
    rs.files_written = R.files_written;
    rs.bytes_written = R.bytes_written;
    rs.repair_launches = R.launches;
    if (stats)
        *stats = rs;
out:
    if (R.list_fd >= 0)
        close(R.list_fd);
    free(vq);
    if (res != results)
        free(res);
    return rc;
}

int bcp_pipeline_set_q_parity(bcp_pipeline *pl, int on)
{
    if (!pl || (on != 0 && on != 1))
        return -EINVAL;
    pl->q_on = on;
    return 0;
}

int bcp_pipeline_set_q_windowed(bcp_pipeline *pl, int on)
{
    if (!pl || (on != 0 && on != 1))
        return -EINVAL;
    pl->q_win = on;
    return 0;
}

int bcp_pipeline_set_repair_windowed(bcp_pipeline *pl, int on)
{
    if (!pl || (on != 0 && on != 1))
        return -EINVAL;
    pl->repair_win = on;
    return 0;
}

int bcp_pipeline_q_stats(const bcp_pipeline *pl, uint64_t *written, uint64_t *no_target, uint64_t *windowed)
{
    if (!pl)
        return -EINVAL;
    if (written)
        *written = pl->q_written;
    if (no_target)
        *no_target = pl->q_no_target;
    if (windowed)
        *windowed = pl->q_windowed;
    return 0;
}

int bcp_pipeline_rebuild2(bcp_pipeline *pl, const char *store_root, int ntargets, int target_a, int target_b,
                          const bcp_work_item *items, size_t nitems, const char *corrupt_list_path,
                          const char *lost_list_path, FILE *log, bcp_run_stats *stats, bcp_rebuild2_stats *st2)
{
    if (!pl || !store_root || ntargets < 2 || ntargets > MAX_STORAGE_TARGETS || target_a < 0 || target_a >= ntargets ||
        target_b < 0 || target_b >= ntargets || target_a == target_b || (nitems && !items))
        return -EINVAL;
    double t0 = now_s();
    for (size_t i = 0; i < nitems; i++) {
        uint64_t loc = items[i].fi.locations;
        int P = GET_P(loc);
        if ((uint64_t)P == NO_P)
            continue;
        if (!items[i].path || P >= ntargets || TEST_BIT(loc, P) || ((loc & L_MASK) >> ntargets))
            return -EINVAL;
    }
    int corrupt_fd = -1, lost_fd = -1, rc = 0;
    task *tasks = NULL;
    uint8_t *unrec = NULL, *kind = NULL; /* per item: unrecoverable; 1 xor, 2 q, 3 pq task */
    if (corrupt_list_path) {
        corrupt_fd = open(corrupt_list_path, O_WRONLY | O_CREAT | O_TRUNC | O_APPEND, S_IRUSR | S_IWUSR);
        if (corrupt_fd < 0)
            return -errno;
    }
    if (lost_list_path) {
        lost_fd = open(lost_list_path, O_WRONLY | O_CREAT | O_TRUNC | O_APPEND, S_IRUSR | S_IWUSR);
        if (lost_fd < 0) {
            rc = -errno;
            goto out;
        }
    }
    tasks = calloc(nitems ? nitems : 1, sizeof(task));
    unrec = calloc(nitems ? nitems : 1, 1);
    kind = calloc(nitems ? nitems : 1, 1);
    if (!tasks || !unrec || !kind) {
        rc = -ENOMEM;
        goto out;
    }
    const uint64_t lmask = (UINT64_C(1) << target_a) | (UINT64_C(1) << target_b);
    uint64_t refused = 0;
    size_t nt = 0;
    for (size_t i = 0; i < nitems; i++) {
        const FileInfo *fi = &items[i].fi;
        const uint64_t loc = fi->locations;
        const int P = GET_P(loc);
        const uint64_t lostH = loc & L_MASK & lmask;
        /* do_file's skip rules (rebuild/main.c:48-51) for either target */
        if ((uint64_t)P == NO_P || !lostH)
            continue;
        if (!bcpi_path_ok(items[i].path, (size_t)-1)) { /* as process_task: refused, skipped */
            if (log)
                fprintf(log, "bcp_pipeline: refusing '%s': not a path inside the store\n", items[i].path);
            refused++;
            continue;
        }
        const int two = lostH == lmask;
        const int p_lost = P == target_a || P == target_b;
        task *t = &tasks[nt];
        memset(t, 0, sizeof(*t));
        t->path = items[i].path;
        t->item = i;
        t->q_st = -1;
        t->rebuild = 1;
        t->timestamp = fi->timestamp;
        t->parity_src = -1;
        t->q_src = -1;
        if (!two && !p_lost) {
            /* one victim, P present: bcp_pipeline_rebuild's task for it */
            const int victim = TEST_BIT(lostH, target_a) ? target_a : target_b;
            const uint64_t src = ((loc & L_MASK) | (UINT64_C(1) << P)) & ~(UINT64_C(1) << victim);
            t->p = victim;
            for (int k = 0; k < MAX_STORAGE_TARGETS; k++)
                if (TEST_BIT(src, k)) {
                    if (k == P)
                        t->parity_src = t->n;
                    t->holders[t->n++] = k;
                }
            kind[i] = 1;
            nt++;
            continue;
        }
        /* Q is needed */
        const int qt = bcp_q_target(loc, ntargets);
        if (qt < 0) {
            unrec[i] = 1;
            continue;
        }
        t->pq = two ? 2 : 1;
        int nlost = 0;
        for (int k = 0; k < MAX_STORAGE_TARGETS; k++)
            if (TEST_BIT(loc & L_MASK, k)) {
                if (TEST_BIT(lostH, k)) {
                    if (nlost == 0)
                        t->p = k;
                    else
                        t->p2 = k;
                    t->lost_pos[nlost++] = t->width;
                } else {
                    t->src_pos[t->n] = t->width;
                    t->holders[t->n++] = k;
                }
                t->width++;
            }
        if (two) {
            t->parity_src = t->n;
            t->holders[t->n++] = P;
        }
        t->q_src = t->n;
        t->holders[t->n++] = qt;
        kind[i] = two ? 3 : 2;
        nt++;
    }
    pl->r2_unrec = unrec;
    rc = pipeline_exec(pl, store_root, tasks, nt, corrupt_fd, log, stats, t0, NULL, NULL);
    pl->r2_unrec = NULL;
    bcp_rebuild2_stats r2 = {0, 0, 0, 0};
    for (size_t i = 0; i < nitems; i++) {
        if (unrec[i]) {
            r2.unrecoverable++;
            push_corrupt(lost_fd, items[i].path); /* (the same one-line-per-path format) */
        } else if (kind[i] == 1) {
            r2.xor_items++;
        } else if (kind[i] == 2) {
            r2.q_items++;
        } else if (kind[i] == 3) {
            r2.pq_items++;
        }
    }
    if (st2)
        *st2 = r2;
    if (stats)
        stats->refused = refused;
out:
    free(tasks);
    free(unrec);
    free(kind);
    if (corrupt_fd >= 0)
        close(corrupt_fd);
    if (lost_fd >= 0)
        close(lost_fd);
    return rc;
}

int bcp_pipeline_gen(const char *store_root, int ntargets, const bcp_work_item *items, size_t nitems,
                     const bcp_pipeline_opts *opts, FILE *log, bcp_run_stats *stats)
{
    bcp_pipeline *pl = NULL;
    int rc = bcp_pipeline_create(opts, &pl);
    if (rc)
        return rc;
    rc = bcp_pipeline_run(pl, store_root, ntargets, items, nitems, log, stats);
    bcp_pipeline_destroy(pl);
    return rc;
}
