/*
 * bcp.h -- C ABI of the MI355X chunk-XOR parity engine (libbcp.so).
 *
 * Drop-in boundary for the arithmetic seam of runefriborg/beegfs-chunk-parity:
 *
 *   static void xor_parity(uint8_t *restrict dst, size_t nbytes,
 *                          const uint8_t *data, int nsources);
 *       -- src/beegfs-raid5/common/task_processing.c:96-109
 *
 * which the P role (parity_generator, task_processing.c:117-245) calls once
 * per 10 MiB window.  This ABI replaces it with
 *   (1) bcp_xor_parity(): the same signature and semantics, on the GPU;
 *   (2) an engine/queue lifecycle (one queue = one HIP stream pair, one per
 *       lane thread, gen/main.c:821-845 runs 12 lanes per rank);
 *   (3) batched asynchronous submission of stripe descriptors, because one
 *       512 KiB x 8 stripe is ~1 us of HBM time -- far below a launch;
 *   (4) query / wait on completion, and HIP-event timing for the bench.
 *
 * Conventions: plain C types only; every function returns 0 or a negative
 * errno value (-EINVAL, -ENOMEM, -ENODEV, -EIO, -EAGAIN); nothing throws
 * across the ABI.  An engine is thread-safe; a queue belongs to one thread
 * at a time.  There is no CPU fallback: without a usable gfx950 device every
 * compute entry point returns -ENODEV.
 *
 * Semantics of every XOR entry point (bit-exact with the reference,
 * SURVEY.md §8(a)):
 *   out[j] = XOR_k  src_k'[j]         for 0 <= j < out_len
 * where src_k'[j] = src_k[j] if j < len_k else 0 (zero padding), except when
 * a stripe carries window W != 0: then byte j of window w = j / W of a source
 * with last readable window lw_k = (len_k - 1) / W and w > lw_k replays
 * window lw_k (chunk_sender never refills its buffer after EOF,
 * task_processing.c:291-308, quirk A3-q1).  len_k = 0 always reads zeros.
 * The replayed stream ends with the longest source, as the reference's parity
 * body does: with a window, out[j] = 0 for j >= max_k len_k.
 */
#ifndef BCP_H
#define BCP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (r06): the resident fold ring (bcp_ring_*) and the P role's fold
 * through it (bcp_task.h, bcp_task_set_fold_ring) added.  Later additions
 * under 4 (nothing existing changed): the parity scrub's
 * bcp_check_stripes_async / bcp_check_result, and the "last_desc_form"
 * value 3; Q parity's bcp_pq_stripes_async / bcp_pq_recover_stripes_async /
 * bcp_pq_lost / bcp_q_target, the "last_desc_form" values 4 and 5 and the
 * option "pq_blocks_per_cu"; the Q-aware scrub's
 * bcp_pq_check_stripes_async / bcp_pq_check_result / bcp_pq_culprit and the
 * "last_desc_form" value 6; Q parity over window replay,
 * bcp_pq_stripes_win_async / bcp_pq_recover_stripes_win_async /
 * bcp_pq_check_stripes_win_async and the "last_desc_form" values 7, 8 and 9;
 * the scrub repair's bcp_pq_repair_stripes_async / bcp_pq_repair_result /
 * bcp_pq_repair_verdict / bcp_patch_file and the "last_desc_form" value 10;
 * the repair over window replay, bcp_pq_repair_stripes_win_async /
 * bcp_pq_repair_win_phases, the "last_desc_form" value 11, the read-only
 * key "last_pq_repair_phases" and bcp_task.h's
 * bcp_pipeline_set_repair_windowed; the verified rebuild's
 * bcp_pq_rebuild_check_stripes_async / bcp_pq_rebuild_check_stripes_win_async,
 * and the "last_desc_form" values 12 and 13; the parity restore's rule,
 * BCP_PQ_KEEP_P / BCP_PQ_KEEP_Q and bcp_task.h's bcp_restore_plan.
 * 3 (r05): the pipeline's MAP read mode (BCP_READ_MAP), its
 * bcp_pipeline_timing fields and bcp_host_register_dma_src removed.
 * 2 (r04): bcp_task.h's bcp_run_stats gained `refused`, bcp_pipeline_opts
 * `read_mode`, bcp_pipeline_timing the MAP fields; bcp_host_register_dma_src
 * added.  Since 1 (r03): fold modes ZERO_COPY, STAGED, STREAMED and
 * DEVICE_ROWS, bcp_dev_alloc_hostwrite and the engine keys they used were
 * removed, and the default window padding became BCP_PAD_AUTO
 * ("ABI history"). */
#define BCP_ABI_VERSION 4
#define BCP_MAX_SOURCES 56                  /* MAX_STORAGE_TARGETS, common.h:18 */
#define BCP_WINDOW_BYTES (10u * 1024u * 1024u) /* FILE_TRANSFER_BUFFER_SIZE, task_processing.c:20 */

typedef struct bcp_engine bcp_engine;
typedef struct bcp_queue bcp_queue;

/* One source of a stripe: device address and readable length in bytes. */
typedef struct bcp_source {
    uint64_t ptr;
    uint64_t len;
} bcp_source;

/* One stripe: out[0..out_len) = XOR of sources[first_src .. first_src+nsrc).
 * window = 0 for plain zero padding, or the transfer window (normally
 * BCP_WINDOW_BYTES, must be a multiple of 16) when the stream exceeded one
 * window and the reference's replay semantics apply. */
typedef struct bcp_stripe {
    uint64_t dst;
    uint64_t out_len;
    uint32_t first_src;
    uint32_t nsrc;
    uint64_t window;
} bcp_stripe;

/* ---- library / device ------------------------------------------------- */
int bcp_abi_version(void);
/* Number of visible HIP devices (0 without a GPU; never fails for that). */
int bcp_device_count(int *count);
/* Human-readable message for a return code. */
const char *bcp_strerror(int rc);

/* ---- engine lifecycle ------------------------------------------------- */
/* Create an engine bound to `device` (HIP ordinal). */
int bcp_engine_create(int device, bcp_engine **out);
int bcp_engine_destroy(bcp_engine *eng);
/* Device properties the bench reports: CU count and the name string. */
int bcp_engine_info(bcp_engine *eng, int *num_cus, char *name, size_t name_cap);
/* PCI bus id of the engine's device ("dddd:bb:dd.f"): identifies the physical
 * GPU across processes whatever HIP_VISIBLE_DEVICES renumbers (bench.py counts
 * distinct devices with it, so ranks sharing a GPU are not reported as more
 * GPUs).  -EINVAL if bus_id_cap is too small. */
int bcp_engine_pci_bus_id(bcp_engine *eng, char *bus_id, size_t bus_id_cap);

/* ---- queues (one in-order HIP stream each) ----------------------------- */
/* Work on one queue runs in submission order.  Overlap (copy beside compute)
 * comes from using two queues ordered by events, as the pipeline does. */
int bcp_queue_create(bcp_engine *eng, bcp_queue **out);
int bcp_queue_destroy(bcp_queue *q);
/* Block until everything submitted to q has finished. */
int bcp_queue_sync(bcp_queue *q);
/* 0 if idle, -EAGAIN if work is pending. */
int bcp_queue_query(bcp_queue *q);

/* ---- completion handles (HIP events) ---------------------------------- */
typedef struct bcp_event bcp_event;
int bcp_event_create(bcp_engine *eng, bcp_event **out);
int bcp_event_destroy(bcp_event *ev);
/* Mark the current tail of q; later bcp_queue_wait_event() / bcp_event_sync()
 * see everything submitted to q before this call. */
int bcp_event_record(bcp_event *ev, bcp_queue *q);
/* Make later work on q wait (on the device) for ev. */
int bcp_queue_wait_event(bcp_queue *q, bcp_event *ev);
/* Host wait; bcp_event_query: 0 done, -EAGAIN pending. */
int bcp_event_sync(bcp_event *ev);
int bcp_event_query(bcp_event *ev);

/* ---- memory ----------------------------------------------------------- */
int bcp_dev_alloc(bcp_engine *eng, size_t bytes, void **dptr);
int bcp_dev_free(bcp_engine *eng, void *dptr);
/* Pinned (page-locked) host memory for staging (registered huge-page memory
 * by default, option host_registered). */
int bcp_host_alloc(bcp_engine *eng, size_t bytes, void **hptr);
/* Pinned host memory that kernels read and write in place over PCIe
 * (coherent, mapped at the same address on the device): the P role's window
 * rows and parity blocks (bcp_task.c, the fold server's shared arena), which
 * the fold reads and writes in place.  Free with bcp_host_free. */
int bcp_host_alloc_mapped(bcp_engine *eng, size_t bytes, void **hptr);
int bcp_host_free(bcp_engine *eng, void *hptr);
/* Register caller-owned host memory (e.g. a shared mapping other processes
 * write) so kernels read and write it in place at the same address, like
 * bcp_host_alloc_mapped memory; -EIO if the device cannot address it at its
 * host address.  Unregister before the memory is unmapped or reused. */
int bcp_host_register(bcp_engine *eng, void *hptr, size_t bytes);
int bcp_host_unregister(bcp_engine *eng, void *hptr);
/* Async copies, in order on q. */
int bcp_h2d_async(bcp_queue *q, void *dst, const void *src, size_t bytes);
int bcp_d2h_async(bcp_queue *q, void *dst, const void *src, size_t bytes);
int bcp_d2d_async(bcp_queue *q, void *dst, const void *src, size_t bytes);
/* Pitched H2D: `rows` rows of `row_bytes`, host pitch hpitch, device pitch dpitch. */
int bcp_h2d_2d_async(bcp_queue *q, void *dst, size_t dpitch, const void *src,
                     size_t hpitch, size_t row_bytes, size_t rows);
int bcp_memset_async(bcp_queue *q, void *dst, int value, size_t bytes);

/* ---- XOR kernels (device pointers, asynchronous on q) ------------------ */
/* Uniform stripes: src is [nstripes][nsrc][chunk_bytes] contiguous, dst is
 * [nstripes][chunk_bytes].  Any alignment / length is accepted; 16-byte
 * aligned pointers with chunk_bytes % 16 == 0 take the streaming fast path. */
int bcp_xor_uniform_async(bcp_queue *q, void *dst, const void *src,
                          uint64_t nstripes, uint32_t nsrc,
                          uint64_t chunk_bytes);
/* Same, but sources given by a stride: source k of stripe s starts at
 * src + s*stripe_stride + k*src_stride; output s at dst + s*dst_stride. */
int bcp_xor_strided_async(bcp_queue *q, void *dst, uint64_t dst_stride,
                          const void *src, uint64_t stripe_stride,
                          uint64_t src_stride, uint64_t nstripes,
                          uint32_t nsrc, uint64_t chunk_bytes);
/* Descriptor batch (variable lengths, zero padding, rebuild truncation,
 * window replay).  Host arrays are copied before return. */
int bcp_xor_stripes_async(bcp_queue *q, const bcp_stripe *stripes,
                          uint32_t nstripes, const bcp_source *sources,
                          uint32_t nsources);

/* One record per stripe of a check batch (bcp_check_stripes_async). */
typedef struct bcp_check_result {
    uint64_t first_bad;   /* smallest j in [0, out_len) with fold[j] != dst[j]; UINT64_MAX if none */
    uint64_t bad_bytes;   /* number of such j (bytes, not vectors) */
} bcp_check_result;
/* Compare instead of store: for every stripe, what bcp_xor_stripes_async would
 * write to [dst, dst+out_len) against what is there.  dst is only read.
 * results_dev: nstripes records in device memory (bcp_dev_alloc), fully
 * written by this call's work for every stripe -- {UINT64_MAX, 0} for a clean
 * one, also for out_len == 0 and for batches with no tile at all.  Both
 * fields are exact.  Nothing is read outside [dst, dst+out_len). */
int bcp_check_stripes_async(bcp_queue *q, const bcp_stripe *stripes,
                            uint32_t nstripes, const bcp_source *sources,
                            uint32_t nsources, bcp_check_result *results_dev);

/* ---- P + Q parity over GF(2^8) ----------------------------------------- */
/* Field: polynomial x^8+x^4+x^3+x^2+1 (0x11d), generator g = 2 (the RAID-6
 * convention of Linux md).  For a stripe of nsrc sources in position order
 * k = 0 .. nsrc-1, each zero-padded to out_len as above:
 *   P[j] = XOR_k D_k[j]        Q[j] = XOR_k g^k * D_k[j]      0 <= j < out_len
 * There is no window replay here (a replayed P is not the plain XOR, which
 * the two-loss algebra needs): window != 0 is -EINVAL.  This holds for
 * bcp_pq_stripes_async, bcp_pq_recover_stripes_async and
 * bcp_pq_check_stripes_async; their _win namesakes further down define both
 * parities over the replayed streams instead. */
/* P and Q of every stripe.  stripes[s].dst = P body (0: P is not written),
 * q_dst[s] = Q body (required); both out_len bytes.  Source k of the stripe's
 * run has coefficient g^k (position order is kept); window must be 0. */
int bcp_pq_stripes_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                         const bcp_source *sources, uint32_t nsources, const uint64_t *q_dst);

#define BCP_PQ_NONE 0xFFFFFFFFu
typedef struct bcp_pq_lost {
    uint64_t p;            /* P body, out_len readable bytes; 0: P is lost too (then y must be NONE) */
    uint64_t q;            /* Q body, out_len readable bytes; required */
    uint32_t x, y;         /* lost positions, x < y < nsrc; y = BCP_PQ_NONE: only x */
    uint64_t dst_x, len_x; /* first len_x (<= out_len) bytes of member x are written */
    uint64_t dst_y, len_y;
} bcp_pq_lost;
/* Recover up to two lost members of every stripe from the survivors and the
 * parities: two data members from P and Q, or one data member from Q alone
 * when P is lost too.  stripes[s]: the survivors in position order, lost
 * positions with len 0; dst is ignored.  (p != 0 with y = NONE is plain
 * RAID-5: -EINVAL, use bcp_xor_stripes_async.)  -EINVAL also for a lost
 * position whose source has len != 0 and for len_x or len_y above out_len. */
int bcp_pq_recover_stripes_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                                 const bcp_source *sources, uint32_t nsources, const bcp_pq_lost *lost);
/* Verified rebuild: the one combination the call above refuses.  Exactly one
 * data member x is lost and P and Q both survive, so P alone gives the member
 * and Q, otherwise idle, vouches for it.  With Ps = P ^ XOR_{k != x} D_k and
 * Qs = Q ^ XOR_{k != x} g^k * D_k over the survivors:
 *   dst_x[j] = Ps[j]                            0 <= j < len_x
 *   byte j < len_x is bad when Qs[j] != g^x * Ps[j]
 * lost[s]: p and q required (out_len readable bytes each, only read), x lost
 * (its source has len 0), y = BCP_PQ_NONE; len_x <= out_len, dst_x required
 * when len_x > 0; anything else -EINVAL, as is a window.  The bytes written
 * are what bcp_xor_stripes_async writes over the survivors and P, whatever the
 * record says: the call reports, it does not alter.  results_dev: nstripes
 * bcp_check_result records in device memory, fully written by this call's work
 * for every stripe -- {UINT64_MAX, 0} for a clean one, also for len_x == 0 and
 * for batches with no tile at all; first_bad is the smallest bad j, bad_bytes
 * their number, both exact.  A fault confined to one member at offset j < len_x
 * -- a survivor, P or Q -- always makes j bad (g has order 255); it cannot be
 * located while x is missing.  Only [0, len_x) is read and judged: nothing is
 * read outside [body, body+out_len) or a source's len, nothing is written
 * outside [dst_x, dst_x+len_x) and the records. */
int bcp_pq_rebuild_check_stripes_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                                       const bcp_source *sources, uint32_t nsources, const bcp_pq_lost *lost,
                                       bcp_check_result *results_dev);

/* Parity restore: one of a complete item's two parity files is lost, the other
 * survives and is the only witness of what the members held when both were
 * written.  Which of the two is kept (bcp_task.h, bcp_restore_plan): */
#define BCP_PQ_KEEP_P 1u /* P is the witness, Q is to be written */
#define BCP_PQ_KEEP_Q 2u /* Q is the witness, P is to be written */
/* With Ps = P ^ XOR_k D_k and Qs = Q ^ XOR_k g^k * D_k over the complete
 * stripe, the kept parity agrees with the members at byte j when Ps[j] == 0
 * (keep P) or Qs[j] == 0 (keep Q).  A fault confined to one member at offset j
 * -- a data member (e in Ps, g^k * e in Qs) or the kept parity (e) -- always
 * shows there, never zero.  Which member is wrong cannot be told from one
 * syndrome.  Two members wrong at one offset can cancel (e in D_a and in D_b
 * leaves Ps clean; e_a, e_b with g^a * e_a = g^b * e_b leave Qs clean). */

/* One record per stripe of a syndrome check (bcp_pq_check_stripes_async).
 * With Ps = P ^ XOR_k D_k and Qs = Q ^ XOR_k g^k * D_k, a byte j is bad when
 * Ps[j] or Qs[j] is non-zero, and names its member: Ps only, P; Qs only, Q;
 * both, the data position k < nsrc with g^k * Ps[j] = Qs[j] (unique: g has
 * order 255), or nowhere when there is no such k. */
#define BCP_PQ_BAD_P        (1ull << 56)
#define BCP_PQ_BAD_Q        (1ull << 57)
#define BCP_PQ_BAD_NOWHERE  (1ull << 58)
typedef struct bcp_pq_check_result {
    uint64_t first_bad;  /* smallest j in [0,out_len) with Ps[j] or Qs[j] != 0; UINT64_MAX if none */
    uint64_t p_bad;      /* bytes with Ps != 0 */
    uint64_t q_bad;      /* bytes with Qs != 0 */
    uint64_t members;    /* OR over the bad bytes: bit k<56 data position k, BAD_P, BAD_Q, BAD_NOWHERE */
} bcp_pq_check_result;
/* Syndromes of every stripe against its P and Q bodies, nothing stored but the
 * records.  stripes[s].dst = P body, q_body[s] = Q body: both required when
 * out_len > 0, out_len readable bytes, only read.  Sources in position order,
 * lost or missing members with len 0; window must be 0.  results_dev:
 * nstripes records in device memory, fully written by this call's work for
 * every stripe -- {UINT64_MAX, 0, 0, 0} for a clean one, also for out_len == 0
 * and for batches with no tile at all.  All four fields are exact.  Nothing is
 * read outside [body, body+out_len) or outside a source's len. */
int bcp_pq_check_stripes_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                               const bcp_source *sources, uint32_t nsources,
                               const uint64_t *q_body, bcp_pq_check_result *results_dev);

/* One record per stripe of a repair (bcp_pq_repair_stripes_async): the four
 * fields of bcp_pq_check_result with the same meaning -- the state as found,
 * before anything was corrected -- and two byte counts.  fixed + left is the
 * number of j with Ps[j] or Qs[j] non-zero. */
typedef struct bcp_pq_repair_result {
    uint64_t first_bad, p_bad, q_bad, members;
    uint64_t fixed;      /* bad bytes corrected in place */
    uint64_t left;       /* bad bytes not touched */
} bcp_pq_repair_result;
/* bcp_pq_check_stripes_async that also corrects, in place in device memory,
 * the bad bytes whose member allow[s] (nstripes masks, required; bit layout of
 * `members`) admits.  For a bad byte j < out_len:
 *   Ps != 0, Qs == 0: P[j] ^= Ps when allow has BAD_P;
 *   Ps == 0, Qs != 0: Q[j] ^= Qs when allow has BAD_Q;
 *   both != 0:        D_k[j] ^= Ps for the k < nsrc with g^k * Ps = Qs, when
 *                     allow has bit k and j < len_k;
 * every other bad byte is left: no such k, a member the mask leaves out, or
 * j at or past len_k (zero padding cannot be wrong; a (0, 0) source is never
 * dereferenced).  Validation is the check's, window must be 0.  The sources
 * and both bodies are written as well as read, so across the whole batch they
 * must not overlap one another: a byte corrected for one stripe must not be a
 * byte another stripe, or another member of the same stripe, reads.  Nothing
 * is written at or past len_k or out_len.  results_dev: nstripes records,
 * fully written, {UINT64_MAX, 0, 0, 0, 0, 0} for a clean stripe.  The
 * correction is single-error per byte offset: two members wrong at the same j
 * can name a third ("Scrub repair"). */
int bcp_pq_repair_stripes_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                                const bcp_source *sources, uint32_t nsources, const uint64_t *q_body,
                                const uint64_t *allow, bcp_pq_repair_result *results_dev);
/* ---- P + Q over window replay ------------------------------------------ */
/* The three entry points above for stripes with a window W.  The replayed
 * stream of source k (quirk A3-q1, see the top of this file) is a function of
 * that source alone: with D_k' = D_k zero-padded and lw_k = (len_k - 1) / W,
 *   R_k[j] = D_k'[j]                     for j <  (lw_k + 1) * W
 *   R_k[j] = D_k'[lw_k * W + j mod W]    for j >= (lw_k + 1) * W
 *   R_k    = 0 everywhere                for len_k = 0
 * and, for 0 <= j < out_len,
 *   P[j] = XOR_k R_k[j]        Q[j] = XOR_k g^k * R_k[j].
 * P is what bcp_xor_stripes_async writes for the same stripe when out_len is
 * the longest len_k, the reference's parity body.  The whole algebra above
 * holds over the R_k: the syndromes over the survivors' replayed streams give
 * R_x and R_y, and the first len_x bytes of R_x are D_x.  Survivors replay to
 * out_len whether or not the longest member is among them.
 * Signatures, validation and results are the namesakes', except that
 * stripes[s].window may be 0 (that stripe: R_k = D_k', exactly the namesake's
 * semantics) or a non-zero multiple of 32768; any other window is -EINVAL.  A
 * batch may mix windows. */
int bcp_pq_stripes_win_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                             const bcp_source *sources, uint32_t nsources, const uint64_t *q_dst);
int bcp_pq_recover_stripes_win_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                                     const bcp_source *sources, uint32_t nsources, const bcp_pq_lost *lost);
/* The record is bcp_pq_check_result unchanged, with Ps = P ^ XOR_k R_k and
 * Qs = Q ^ XOR_k g^k * R_k: first_bad, p_bad and q_bad are offsets and counts
 * in the replayed streams, so one wrong byte of D_k counts once for every place
 * below out_len it is replayed to, and names position k at each of them. */
int bcp_pq_check_stripes_win_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                                   const bcp_source *sources, uint32_t nsources,
                                   const uint64_t *q_body, bcp_pq_check_result *results_dev);
/* bcp_pq_rebuild_check_stripes_async with Ps and Qs over the survivors'
 * replayed streams: dst_x = R_x cut to len_x, which is D_x; an offset below
 * len_x that a survivor's wrong byte is replayed to counts like its home. */
int bcp_pq_rebuild_check_stripes_win_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                                           const bcp_source *sources, uint32_t nsources, const bcp_pq_lost *lost,
                                           bcp_check_result *results_dev);

/* The repair over window replay.  One wrong byte of D_k in its last readable
 * window shows at its home offset j and at every echo j + W, j + 2W, ... below
 * out_len, each in another tile, so the tiles run in phases, one launch per
 * phase in order on q:
 *   thresholds  the distinct T_k = (lw_k + 1) * W over the positions k with
 *               bit k in allow, len_k > 0 and T_k < out_len: E_1 < ... < E_m;
 *   phase       of the tile at stripe offset off: #{i : E_i <= off}.  W is a
 *               multiple of the largest tile, so no tile straddles a threshold;
 *               a stripe with window 0, or without such a k, is all phase 0;
 *   launches    1 + the largest phase of the batch.
 * bcp_pq_repair_win_phases is that rule (pure host arithmetic, no device): for
 * stripe s with its own source run (run[k] is position k; s->first_src is not
 * used) it writes the first min(m, cap) thresholds, ascending, to bounds and
 * returns m + 1, the number of phases.  -EINVAL for a null s, a null run with
 * nsrc > 0, null bounds with cap > 0, a window that is neither 0 nor a multiple
 * of 32768, and nsrc > BCP_MAX_SOURCES. */
int bcp_pq_repair_win_phases(const bcp_stripe *s, const bcp_source *run, uint64_t allow, uint64_t *bounds,
                             uint32_t cap);
/* bcp_pq_repair_stripes_async over the replayed streams R_k.  Signature and
 * validation are its own, except that stripes[s].window may be 0 or a non-zero
 * multiple of 32768 and a batch may mix them; a batch without any window is
 * the namesake's launch.  The rules are the namesake's with Ps and Qs over the
 * R_k and one more clause: a byte that names position k is written, as
 * D_k[j] ^= Ps, only by a tile at which source k is not replayed (off <
 * T_k, where R_k[j] is D_k'[j] itself, so j < len_k is the same test); at a
 * tile where k is replayed the byte is left.  P and Q are addressed with the
 * stream offset.  A byte of D_k is thus written only by its home tile and read
 * again only by k's echo tiles, which lie in a later phase: the result does
 * not depend on timing.  A member the mask leaves out is never written.
 * The record is the state as found by each phase: a corrected data byte counts
 * once, at its home -- its echoes are clean by the time their phase runs -- so
 * p_bad and q_bad are at most bcp_pq_check_stripes_win_async's for the same
 * stripe, and equal when nothing corrected had an echo; first_bad and members
 * equal the check's whenever every stream offset has at most one wrong member;
 * fixed + left is the number of bad bytes the phases saw.  For a data member
 * outside the mask every echo counts in p_bad, q_bad and left, as the check
 * counts them.  The namesake's limit holds: two members wrong at one stream
 * offset can name a third, and the record's members may then differ from a
 * check's made before.  Across the whole batch no two members may overlap.
 * Nothing is written at or past len_k or out_len. */
int bcp_pq_repair_stripes_win_async(bcp_queue *q, const bcp_stripe *stripes, uint32_t nstripes,
                                    const bcp_source *sources, uint32_t nsources, const uint64_t *q_body,
                                    const uint64_t *allow, bcp_pq_repair_result *results_dev);

/* Which single member a record blames (pure host arithmetic, no device,
 * bcp_pq_host.c).  Returns the kind, or -EINVAL for a null record;
 * *position (may be null) is the data position for DATA, else -1. */
#define BCP_CULPRIT_NONE 0   /* members == 0 */
#define BCP_CULPRIT_DATA 1   /* exactly one bit k < 56: *position = k */
#define BCP_CULPRIT_P    2
#define BCP_CULPRIT_Q    3
#define BCP_CULPRIT_MANY 4   /* more than one bit, or BAD_NOWHERE: not a single-member fault */
int bcp_pq_culprit(const bcp_pq_check_result *r, int *position);

/* Which members of a record a repair may write under a policy (pure host
 * arithmetic).  mode: BCP_REPAIR_PARITY, only P and Q; BCP_REPAIR_ALL, data
 * members too.  Returns BCP_VERDICT_REPAIR with *allow = the record's member
 * bits, or, with *allow = 0, BCP_VERDICT_CLEAN (members == 0),
 * BCP_VERDICT_UNLOCATED (BAD_NOWHERE is set, or a data bit at or above nsrc)
 * or BCP_VERDICT_POLICY (more than max_members member bits, or a data bit
 * under PARITY).  -EINVAL for a null record or allow, or a mode that is
 * neither. */
#define BCP_REPAIR_PARITY 1
#define BCP_REPAIR_ALL    2
#define BCP_VERDICT_CLEAN     0
#define BCP_VERDICT_REPAIR    1
#define BCP_VERDICT_UNLOCATED 2
#define BCP_VERDICT_POLICY    3
int bcp_pq_repair_verdict(const bcp_pq_check_result *r, uint32_t nsrc, int mode, uint32_t max_members,
                          uint64_t *allow);
/* Patch a file in place from two images of its body: every 4 KiB block of
 * [0, len) (block boundaries relative to the body) in which now[] differs from
 * was[] is pwritten from now[] at file offset body_off + block, clipped to len.
 * The file is opened and fstat'ed first: a size other than expect_size or an
 * mtime other than *expect_mtime is -ESTALE and nothing is written.  After the
 * last pwrite and an fdatasync, futimens puts back the atime and mtime that
 * fstat showed.  Nothing is created, truncated or resized (-EINVAL when
 * body_off + len exceeds the size).  *bytes_written (may be null) is the sum
 * of the blocks written; no differing block is success with 0 and the file is
 * not written at all.  Other failures are -errno (-ENOENT for a missing file). */
struct timespec;
int bcp_patch_file(const char *path, uint64_t body_off, const void *was, const void *now, uint64_t len,
                   uint64_t expect_size, const struct timespec *expect_mtime, uint64_t *bytes_written);

/* Storage target of an item's Q file (pure host arithmetic, no device):
 * `locations` as in bcp_task.h's FileInfo (bits 0..55 chunk holders, bits
 * 56..63 the parity target P).  The first of P+1, P+2, ... (mod ntargets)
 * that is neither a holder nor P; -1 when there is none, when the item has no
 * valid P (NO_P, P a holder, P >= ntargets) and for ntargets outside
 * 1..BCP_MAX_SOURCES. */
int bcp_q_target(uint64_t locations, int ntargets);

/* ---- resident fold ring ------------------------------------------------ */
/* One kernel launch that stays on the device and folds stripes published
 * into a ring of descriptors in pinned host memory: no launch and no stream
 * sync per stripe.  For callers that fold one small stripe at a time from
 * many threads -- the P role's windows, task_processing.c:203-226, 12 lanes
 * per rank (gen/main.c:821-889) -- where a launch + sync per window is the
 * bound.  Same semantics as bcp_xor_stripes_async for one stripe with
 * window 0 (sources and output anywhere the device can address: pinned
 * mapped host memory or device memory; any alignment and length).
 *
 * The launch starts on the first submission and ends by itself after
 * idle_us without one (it is relaunched on the next); bcp_ring_destroy ends
 * it at once.  While it is live it holds 1 + `workers` workgroups of the
 * device, and HIP calls that wait for the whole device (hipFree,
 * hipHostUnregister, device synchronisation) wait until it idles out.
 * A ring is thread-safe: any thread may submit and wait. */
typedef struct bcp_ring bcp_ring;
/* workers: worker workgroups (0 = default 64, at most 4096); idle_us: idle
 * time before the launch ends (0 = default 5000, at most 10 s). */
int bcp_ring_create(bcp_engine *eng, int workers, int idle_us, bcp_ring **out);
/* Publish stripe (window must be 0; nsrc <= BCP_MAX_SOURCES; out_len <=
 * 255 x 512 KiB) with its sources[0 .. nsrc) (stripe->first_src is ignored).
 * Returns at once with a handle for bcp_ring_wait / _query; blocks only while
 * the ring is full.  The caller keeps sources and output untouched until the
 * handle completes. */
int bcp_ring_submit(bcp_ring *r, const bcp_stripe *stripe, const bcp_source *sources, uint64_t *handle);
/* Block until the stripe behind handle is folded and visible to the host;
 * -EIO if the ring's launch failed. */
int bcp_ring_wait(bcp_ring *r, uint64_t handle);
/* 0 done, -EAGAIN pending, -EIO failed. */
int bcp_ring_query(bcp_ring *r, uint64_t handle);
/* Stops the launch (pending stripes are folded first) and frees the ring;
 * every handle must have been waited for. */
int bcp_ring_destroy(bcp_ring *r);
/* How waiters wait: spin spin_us, then sleep sleep_us between looks (0:
 * sched_yield); defaults from the engine options ring_spin_us /
 * ring_sleep_us (4 / 10). */
int bcp_ring_set_wait(bcp_ring *r, int spin_us, int sleep_us);
/* Pieces published (a stripe is cut into 512 KiB pieces) and launches made
 * since the ring was created. */
int bcp_ring_stats(bcp_ring *r, uint64_t *pieces, uint64_t *launches);

/* ---- drop-in for xor_parity (task_processing.c:96-109) ----------------- */
/* Host pointers, synchronous, same contract as the reference: dst gets
 * XOR of the nsources rows of `data` ([nsources][nbytes]).  nsources is
 * 1..BCP_MAX_SOURCES (-EINVAL otherwise: the P role never folds zero rows,
 * it unlinks the parity chunk instead, task_processing.c:141-144).  Runs on a
 * process-wide engine (device from $BCP_DEVICE, default 0) and a per-thread
 * queue with pinned staging; returns -ENODEV without a GPU. */
int bcp_xor_parity(uint8_t *dst, size_t nbytes, const uint8_t *data,
                   int nsources);

/* ---- verification / synthetic data (device) --------------------------- */
/* Fill with the splitmix64 byte stream: byte b = byte (b&7) of
 * splitmix64(seed + (byte_offset + b)/8).  Same stream as the oracle's
 * oracle_fill_synthetic, so checks need no bulk host copy. */
int bcp_dev_fill_synthetic_async(bcp_queue *q, void *dst, uint64_t bytes,
                                 uint64_t seed, uint64_t byte_offset);
/* XOR-fold of a buffer into 16 bytes (out16_dev is device memory). */
int bcp_dev_xor_fold_async(bcp_queue *q, const void *src, uint64_t bytes,
                           void *out16_dev);
/* Count of differing bytes between two device buffers into *out_dev (u64). */
int bcp_dev_compare_async(bcp_queue *q, const void *a, const void *b,
                          uint64_t bytes, void *out_dev);

/* ---- timing (HIP events on the queue's stream) ------------------------- */
int bcp_queue_mark(bcp_queue *q, int slot);           /* slot 0..63 */
int bcp_queue_elapsed_ms(bcp_queue *q, int slot_from, int slot_to,
                         float *ms);

/* Tuning knobs for the fast path (bench / autotune only; 0 = default). */
int bcp_set_tuning(bcp_engine *eng, int blocks_per_cu, int vecs_per_thread);
/* Named knob (unknown keys and out-of-range values: -EINVAL):
 *  uniform streaming kernel: "blocks_per_cu" (1..32, default 1),
 *   "vecs_per_thread" (1, 2, 4, 8; 0 = the default: 8, or 4 / 2 for batches
 *   of few tiles), "stream_grid" (explicit workgroup count; 0 = the default,
 *   blocks_per_cu on 29 of every 32 CUs), "table_host_max" (bytes: a
 *   pointer table up to this size is read from pinned host memory instead of
 *   being copied first; default 4096);
 *  descriptor kernel (mixed sizes, windows, unaligned): "desc_blocks_per_cu"
 *   (0 = the default, one per CU; 1..32), "desc_vecs_per_thread" (1, 2, 4,
 *   8, 16; 0 = by batch size; 16 = 64 KiB subtiles, batches through
 *   desc_tiles only -- small batches in the kernel arguments use 8),
 *   "desc_grid" (explicit workgroup count; 0 = default), "desc_args_max"
 *   (batches of at most this many stripes, 0..16, travel in the kernel
 *   arguments; default 16), "desc_table_host_max" (as table_host_max;
 *   default 131072), "desc_reuse_records" (1: a batch resubmitted on a ring
 *   slot with byte-identical staged tables reuses that slot's tile records;
 *   default 0, an A/B knob);
 *  P + Q kernel (bcp_pq_*): tiles of "desc_vecs_per_thread" vectors per lane
 *   where that is 4 or 8 (else by batch size), "pq_blocks_per_cu" workgroups
 *   per CU (1..8, default 2), or "desc_grid" workgroups when that is set;
 *  resident fold ring: "ring_spin_us" (a waiter spins this long, default 4)
 *   and "ring_sleep_us" (then sleeps this long between looks, default 10;
 *   0 = sched_yield instead);
 *  memory: "contiguous_alloc" (1: bcp_dev_alloc requests physically
 *   contiguous memory for buffers of 64 MiB and more; default 0),
 *   "host_registered" (bcp_host_alloc / bcp_host_alloc_mapped: 1 = ordinary
 *   huge-page memory registered with HIP, the default -- CPU copies into and
 *   out of it run at malloc speed; 0 = hipHostMalloc; env
 *   BCP_HOST_REGISTERED).
 * The kernels' schedule (device-wide tile work queue), register budgets and
 * load windows are fixed: the alternatives lost the r01-r03 sweeps
 * (DESIGN.md section 4). */
int bcp_set_option(bcp_engine *eng, const char *key, int value);
/* Current value of a named knob (same keys), or of the engine's latest
 * launch: "last_stream_vecs" (vecs_per_thread of the streaming kernel),
 * "last_desc_vecs" and "last_desc_form" (descriptor kernel: 1 = desc_tiles +
 * xor_desc, 2 = xor_desc_args, 3 = desc_tiles + the check kernel of
 * bcp_check_stripes_async, 4 = the P + Q kernel of bcp_pq_stripes_async,
 * 5 = its recovery form, bcp_pq_recover_stripes_async, 6 = its syndrome
 * form, bcp_pq_check_stripes_async, 7 / 8 / 9 = the windowed kernels of
 * bcp_pq_stripes_win_async / bcp_pq_recover_stripes_win_async /
 * bcp_pq_check_stripes_win_async, taken by a batch with a windowed stripe,
 * 10 = the repair form, bcp_pq_repair_stripes_async, 11 = its windowed
 * kernel, taken by a bcp_pq_repair_stripes_win_async batch with a windowed
 * stripe, 12 = the verified-rebuild form,
 * bcp_pq_rebuild_check_stripes_async, 13 = its windowed kernel, taken by a
 * bcp_pq_rebuild_check_stripes_win_async batch with a windowed stripe), and
 * "last_pq_repair_phases": the launches the latest
 * bcp_pq_repair_stripes_win_async call made (1 for a batch without a window,
 * 0 for one without a tile). */
int bcp_get_option(bcp_engine *eng, const char *key, int *value);
/* Timer slots for bcp_queue_mark / bcp_queue_elapsed_ms. */
#define BCP_TIMER_SLOTS 64

#ifdef __cplusplus
}
#endif

#endif /* BCP_H */
