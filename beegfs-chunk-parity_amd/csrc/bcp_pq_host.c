/* bcp_pq_host.c -- host-only pieces of Q parity (no device needed). */
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
