/* bcp_pq_host.c -- host-only pieces of Q parity (no device needed). */
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "bcp.h"
#include "bcp_task.h"

/* The Q file of an item lives on the first target after P (cyclically) that
 * holds neither a chunk of the item nor its P. */
int bcp_q_target(uint64_t locations, int ntargets) {
    if (ntargets < 1 || ntargets > MAX_STORAGE_TARGETS) return -1;
    const int p = GET_P(locations);
    if (p >= ntargets || TEST_BIT(locations, p)) return -1; /* NO_P (0xFF) is above every target */
    for (int i = 1; i < ntargets; i++) {
        const int t = (p + i) % ntargets;
        if (!TEST_BIT(locations, t)) return t;
    }
    return -1;
}

/* Which of an item's parity files were lost with the targets, and which
 * survivor is kept as the witness (bcp_task.h). */
int bcp_restore_plan(uint64_t locations, int ntargets, int target_a, int target_b, int q_on, int windowed_no_q,
                     int *p_lost, int *q_lost, uint32_t *keep) {
    if (ntargets < 1 || ntargets > MAX_STORAGE_TARGETS) return -EINVAL;
    if (target_a < 0 || target_a >= ntargets || target_b < -1 || target_b >= ntargets || target_b == target_a)
        return -EINVAL;
    const int p = GET_P(locations);
    const int qt = q_on && !windowed_no_q ? bcp_q_target(locations, ntargets) : -1;
    const int pl = p < ntargets && (p == target_a || p == target_b); /* NO_P (0xFF) is above every target */
    const int ql = qt >= 0 && (qt == target_a || qt == target_b);
    if (p_lost) *p_lost = pl;
    if (q_lost) *q_lost = ql;
    if (keep) *keep = pl && !ql && qt >= 0 ? BCP_PQ_KEEP_Q : ql && !pl ? BCP_PQ_KEEP_P : 0u;
    return 0;
}

/* The single member a syndrome record blames, if it blames one. */
int bcp_pq_culprit(const bcp_pq_check_result *r, int *position) {
    if (!r) return -EINVAL;
    if (position) *position = -1;
    const uint64_t m = r->members;
    if (!m) return BCP_CULPRIT_NONE;
    if ((m & (m - 1)) || (m & BCP_PQ_BAD_NOWHERE)) return BCP_CULPRIT_MANY;
    if (m == BCP_PQ_BAD_P) return BCP_CULPRIT_P;
    if (m == BCP_PQ_BAD_Q) return BCP_CULPRIT_Q;
    if (m >> BCP_MAX_SOURCES) return BCP_CULPRIT_MANY; /* bits above 58 are no member */
    if (position) *position = __builtin_ctzll(m);
    return BCP_CULPRIT_DATA;
}

/* Which members a repair may write (bcp.h). */
int bcp_pq_repair_verdict(const bcp_pq_check_result *r, uint32_t nsrc, int mode, uint32_t max_members,
                          uint64_t *allow) {
    if (!r || !allow || (mode != BCP_REPAIR_PARITY && mode != BCP_REPAIR_ALL)) return -EINVAL;
    *allow = 0;
    const uint64_t m = r->members;
    if (!m) return BCP_VERDICT_CLEAN;
    const uint64_t data = m & ((1ull << BCP_MAX_SOURCES) - 1);
    const uint64_t known = data | (m & (BCP_PQ_BAD_P | BCP_PQ_BAD_Q));
    if (m != known) return BCP_VERDICT_UNLOCATED; /* BAD_NOWHERE, or a bit that is no member */
    if (nsrc < BCP_MAX_SOURCES && (data >> nsrc)) return BCP_VERDICT_UNLOCATED;
    if ((uint32_t)__builtin_popcountll(known) > max_members) return BCP_VERDICT_POLICY;
    if (data && mode == BCP_REPAIR_PARITY) return BCP_VERDICT_POLICY;
    *allow = known;
    return BCP_VERDICT_REPAIR;
}

/* The phase thresholds of a windowed repair (bcp.h): the distinct
 * T_k = (lw_k + 1) * W below out_len of the non-empty members the mask admits,
 * ascending.  At most nsrc of them, kept sorted by insertion. */
int bcp_pq_repair_win_phases(const bcp_stripe *s, const bcp_source *run, uint64_t allow, uint64_t *bounds,
                             uint32_t cap) {
    if (!s || (s->nsrc && !run) || (cap && !bounds)) return -EINVAL;
    if (s->nsrc > BCP_MAX_SOURCES || s->window % 32768u != 0) return -EINVAL;
    const uint64_t W = s->window;
    uint64_t e[BCP_MAX_SOURCES];
    uint32_t m = 0;
    for (uint32_t k = 0; W && k < s->nsrc; k++) {
        const uint64_t len = run[k].len;
        if (!(allow >> k & 1) || !len) continue;
        const uint64_t lw = (len - 1) / W;
        if (!s->out_len || lw >= (s->out_len - 1) / W) continue; /* T_k >= out_len (so T_k cannot wrap below) */
        const uint64_t t = (lw + 1) * W;
        uint32_t i = 0;
        while (i < m && e[i] < t) i++;
        if (i < m && e[i] == t) continue;
        memmove(e + i + 1, e + i, (m - i) * sizeof(*e));
        e[i] = t;
        m++;
    }
    for (uint32_t i = 0; i < m && i < cap; i++) bounds[i] = e[i];
    return (int)m + 1;
}

/* In-place patch of the blocks that differ (bcp.h): decisions 1-3 of
 * INTEGRATION.md, "Scrub repair". */
#define PATCH_BLOCK 4096u
int bcp_patch_file(const char *path, uint64_t body_off, const void *was, const void *now, uint64_t len,
                   uint64_t expect_size, const struct timespec *expect_mtime, uint64_t *bytes_written) {
    if (bytes_written) *bytes_written = 0;
    if (!path || !expect_mtime || (len && (!was || !now))) return -EINVAL;
    const int fd = open(path, O_WRONLY | O_CLOEXEC);
    if (fd < 0) return -errno;
    struct stat sb;
    int rc = 0;
    uint64_t total = 0;
    if (fstat(fd, &sb) != 0) {
        rc = -errno;
    } else if ((uint64_t)sb.st_size != expect_size || sb.st_mtim.tv_sec != expect_mtime->tv_sec ||
               sb.st_mtim.tv_nsec != expect_mtime->tv_nsec) {
        rc = -ESTALE;
    } else if (body_off > expect_size || len > expect_size - body_off) {
        rc = -EINVAL;
    }
    const unsigned char *a = (const unsigned char *)was, *b = (const unsigned char *)now;
    for (uint64_t o = 0; !rc && o < len; o += PATCH_BLOCK) {
        const uint64_t n = len - o < PATCH_BLOCK ? len - o : PATCH_BLOCK;
        if (!memcmp(a + o, b + o, n)) continue;
        uint64_t done = 0;
        while (done < n) {
            const ssize_t w = pwrite(fd, b + o + done, n - done, (off_t)(body_off + o + done));
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) {
                rc = w < 0 ? -errno : -EIO;
                break;
            }
            done += (uint64_t)w;
        }
        total += done;
    }
    if (total) { /* also after a failed write: what was written keeps the old times */
        if (fdatasync(fd) != 0 && !rc) rc = -errno;
        const struct timespec tv[2] = {sb.st_atim, sb.st_mtim};
        if (futimens(fd, tv) != 0 && !rc) rc = -errno;
    }
    if (close(fd) != 0 && !rc) rc = -errno;
    if (bytes_written) *bytes_written = total;
    return rc;
}
