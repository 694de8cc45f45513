/* hipdouble.h -- what a driver may ask of the CPU stand-in for the HIP runtime
 * and the kernel launchers (hipdouble.cpp).  Test code: never part of
 * libbcp.so.  The schedule comes from the environment, read at the first call:
 *   HIPDOUBLE_SCHEDULE=eager   every operation runs as soon as stream order allows
 *   HIPDOUBLE_SCHEDULE=lazy    an operation runs when somebody blocks on it, or
 *                              after a short timer (so polling never livelocks)
 *   HIPDOUBLE_SCHEDULE=seed=N  per-operation delays from generator N
 * Further knobs: HIPDOUBLE_LAZY_US (lazy's timer, default 1500),
 * HIPDOUBLE_LAUNCH_US (every launch stays on its stream at least this long: a
 * slow device, so that later batches are submitted beside it; default 0),
 * HIPDOUBLE_DEVICES (1: one device instead of two, so that a pipeline's lanes
 * wrap onto it), HIPDOUBLE_TRACE (one line on stderr per allocation and free). */
#ifndef HIPDOUBLE_H
#define HIPDOUBLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Findings so far.  Each was also one line on stderr ("hipdouble: FINDING ..."). */
long hipdouble_findings(void);
/* Operations (copies, memsets, launches, event records and waits) executed. */
long hipdouble_ops(void);
/* Adds delta to the work-queue counter the latest launch used: the mistake
 * "a kernel starts with the counter off its base", for the self-test. */
int hipdouble_bump_counter(long delta);

#ifdef __cplusplus
}
#endif

#endif
