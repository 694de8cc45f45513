/* bcp_pq_host.c -- host-only pieces of Q parity (no device needed). */
#include <errno.h>

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
