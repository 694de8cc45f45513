/*
 * bcp_tool.c -- command-line front end (bin/bcp) over libbcp.so for
 * loopback stores <root>/st<k>/{chunks,parity,db}: the single-node
 * counterpart of the reference's programs.
 *
 *   bcp find-all-chunks <chunks_dir>
 *       bp-find-all-chunks: the record stream on stdout.
 *   bcp parity-gen --complete|--partial [--pipeline|--protocol|--procs] [--fold MODE]
 *                  [--read PATH] [--lanes N] [--force] [--changelog DIR] [--q] [--q-windowed]
 *                  <store_root> <ntargets>
 *       beegfs-parity-gen + bp-parity-gen (src/beegfs-parity-gen:1-135,
 *       gen/main.c): target bookkeeping, phase 1 from a scan of every
 *       target (--complete) or from record files DIR/st<k> (--partial,
 *       default DIR = <root>/changelog), then one round against the
 *       persistent state.  Engines (byte-identical output):
 *         --pipeline (default): the batched pipeline on every visible GPU --
 *           the faster engine for local stores;
 *         --protocol: the per-rank protocol (process_task, 12 lanes per rank,
 *           ranks as threads) -- the reference's interface;
 *         --procs: the same with one process per target, as under mpirun.
 *       --fold picks the protocol P role's GPU fold: pipelined (default) or
 *       batched; --read the pipeline's read path (bcp_pipeline_opts.read_mode):
 *       auto (default: copy for stores in memory, direct for a cold store on a
 *       disk), copy, or direct (O_DIRECT into the pinned slabs); --read with
 *       --protocol / --procs and --fold with the pipeline are refused (usage):
 *       each names a path the other engines do not have.  A --complete over
 *       an existing state needs --force and first
 *       deletes the old parity data and DBs (the script's clean_old,
 *       :94-108, :120-126).  On success <root>/last-gen-timestamp.
 *       --q (pipeline only; usage with --protocol / --procs): also write the Q
 *       parity files <root>/st<q>/parityq/<path> (bcp_pipeline_set_q_parity).
 *       --q-windowed (implies --q): also for items past the 10 MiB window
 *       (bcp_pipeline_set_q_windowed).  A --q run without it removes those
 *       items' Q files, so a store that uses it uses it in every run.
 *   bcp parity-rebuild [--pipeline|--protocol|--procs] [--fold MODE] [--read PATH] [--lanes N]
 *                      [--db DIR] [--corrupt FILE] [--also TARGET] [--lost FILE] [--q-windowed]
 *                      <store_root> <ntargets> <target>
 *       beegfs-parity-rebuild + bp-parity-rebuild (rebuild/main.c), through
 *       the batched pipeline (default), the per-rank protocol (--protocol)
 *       or rank processes (--procs).  --also TARGET (pipeline only): a second
 *       target is lost too; chunks are rebuilt from P, from Q or from both
 *       (bcp_pipeline_rebuild2), the paths that cannot be go to --lost FILE and
 *       the exit status is then 1.  --q-windowed (with --also): items past the
 *       window have Q files too and are recovered like the others.
 *   bcp parity-verify [--db DIR] [--bad FILE] [--read PATH] [--q [--culprits FILE] [--q-windowed]
 *                     [--repair parity|all [--repair-members N] [--dry-run] [--repaired FILE]
 *                     [--repair-windowed]]] <store_root> <ntargets>
 *       The scrub (no counterpart in the reference): for every item of the
 *       database (default <root>/st0/db) the batched pipeline reads the chunks
 *       and the parity body and compares them on the device
 *       (bcp_pipeline_verify); nothing under the store is written.  One
 *       summary line; --bad FILE lists the paths whose parity is missing,
 *       has the wrong size or differs.  Exit 0 when nothing is NO_PARITY, SIZE
 *       or MISMATCH, nothing was refused and no read or device error occurred
 *       (stale items -- chunks modified since the last round -- are clean).
 *       --q: the scrub with Q (bcp_pipeline_verify_q): an item's Q file is
 *       read and checked in the same pass, and a mismatch names the one file
 *       that is wrong -- a chunk, P or Q -- where the syndromes allow.  A
 *       second summary line has the Q states and the culprits; --culprits FILE
 *       gets one line "path<TAB>data|p|q|many<TAB>target" per mismatch; --bad
 *       also lists the items whose Q file is missing or out of order, and
 *       those make the exit status 1 too.  --q-windowed (with --q): items
 *       past the window are expected to have a Q file and are checked with it.
 *       --repair parity|all (with --q; without it a usage error, exit 2): the
 *       scrub also corrects what the syndromes blame (bcp_pipeline_repair_q) --
 *       `parity` only P and Q files, `all` chunks too -- in items that blame
 *       at most --repair-members N (default 1) files, and writes back the
 *       4 KiB blocks that changed, file times restored.  --dry-run corrects
 *       and re-checks on the device and writes nothing; --repaired FILE gets
 *       "path<TAB>data|p|q<TAB>target<TAB>bytes" per file written.  A third
 *       summary line has the repair counts.  The first two lines and the lists
 *       describe the store as found; the exit status is 0 when every mismatch
 *       was repaired and nothing else is wrong (with --dry-run: as without
 *       --repair).  --repair-windowed (with --repair and --q-windowed; without
 *       either a usage error, exit 2): items past the window are repaired too
 *       (bcp_pipeline_set_repair_windowed); without it they are reported and
 *       left as they are.
 *
 * Items whose path would leave the store (absolute, "..") are skipped and
 * counted as refused; a run with refused items exits 1.
 *
 * Exit status 0 on success, 1 on any error (message on stderr).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <ftw.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "bcp_task.h"

static int usage(void)
{
    fputs("usage: bcp find-all-chunks <chunks_dir>\n"
          "       bcp parity-gen --complete|--partial [--pipeline|--protocol|--procs] [--fold MODE] [--read PATH]\n"
          "                      [--lanes N] [--force] [--changelog DIR] [--q] [--q-windowed] <store_root> <ntargets>\n"
          "       bcp parity-rebuild [--pipeline|--protocol|--procs] [--fold MODE] [--read PATH] [--lanes N]\n"
          "                          [--db DIR] [--corrupt FILE] [--also TARGET] [--lost FILE] [--q-windowed]\n"
          "                          <store_root> <ntargets> <target>\n"
          "       bcp parity-verify [--db DIR] [--bad FILE] [--read PATH] [--q [--culprits FILE] [--q-windowed]\n"
          "                         [--repair parity|all [--repair-members N] [--dry-run] [--repaired FILE]\n"
          "                         [--repair-windowed]]] <store_root> <ntargets>\n"
          "       engine: --pipeline (default: batched pipeline on every GPU) | --protocol (per-rank\n"
          "               process_task, ranks as threads) | --procs (ranks as processes)\n"
          "       MODE (protocol P-role fold): pipelined (default) | batched\n"
          "       PATH (pipeline read path): auto (default: copy in memory, direct for cold disk stores) | copy |\n"
          "            direct (O_DIRECT)\n"
          "       --read applies to the pipeline only, --fold to --protocol / --procs only\n"
          "       --q (also write Q parity files) and --also TARGET (a second lost target; --lost FILE lists\n"
          "            what cannot be rebuilt) apply to the pipeline only\n"
          "       parity-verify --q also reads and checks the Q files and names the wrong file of a mismatch;\n"
          "            --culprits FILE (with --q only) lists path, data|p|q|many and the storage target\n"
          "            --repair parity|all (with --q only) corrects in place what the syndromes blame: P and Q files,\n"
          "            or chunks too; at most N files per item (default 1); --dry-run writes nothing; --repaired FILE\n"
          "            lists path, data|p|q, target and bytes per file written; --repair-windowed (with --repair and\n"
          "            --q-windowed only) also repairs items past the 10 MiB window, which are otherwise reported\n"
          "       --q-windowed (pipeline only): Q files for items past the 10 MiB window too; parity-gen (implies\n"
          "            --q; a --q run without it removes those Q files), parity-rebuild --also, parity-verify --q\n",
          stderr);
    return 1;
}

static int g_read_mode = BCP_READ_AUTO;

static int read_mode_arg(const char *s)
{
    if (!strcmp(s, "auto"))
        return BCP_READ_AUTO;
    if (!strcmp(s, "copy"))
        return BCP_READ_COPY;
    if (!strcmp(s, "direct"))
        return BCP_READ_DIRECT;
    return -1;
}

static int fold_mode_arg(const char *s)
{
    if (!strcmp(s, "batched"))
        return BCP_FOLD_BATCHED;
    if (!strcmp(s, "pipelined"))
        return BCP_FOLD_PIPELINED;
    return -1;
}

/* The batched pipeline on every visible GPU (each brings its own PCIe link;
 * io threads scale with them).  job_bytes (0: unknown) sizes the slabs: the
 * pipeline cuts a run into batches of at most job / (4 x slots x GPUs)
 * anyway, so bigger slabs would only be pinned and zeroed for nothing -- the
 * setup of a one-shot run (a config-1 --complete: 2 GiB of slabs, 0.25-0.38 s
 * of a 0.6 s process, profiles/r05/pipeline/c1_cli_r5e.jsonl).  Slabs still
 * grow to a stripe that does not fit. */
static int pipeline_on_all_gpus(bcp_pipeline **pl, uint64_t job_bytes)
{
    int ndev = 0;
    bcp_device_count(&ndev);
    const uint64_t devs = ndev > 0 ? (uint64_t)ndev : 1, full = (uint64_t)256 << 20, least = (uint64_t)16 << 20;
    uint64_t slab = full;
    if (job_bytes) {
        slab = job_bytes / (4 * 4 * devs) + 1;
        slab = (slab + least - 1) / least * least;
        slab = slab < least ? least : slab > full ? full : slab;
    }
    const bcp_pipeline_opts o = {0, (size_t)slab, 0, 4, (int)devs, g_read_mode};
    return bcp_pipeline_create(&o, pl);
}

/* Bytes a --complete run stages: the chunk bytes the scan's records announce
 * plus a page per chunk (DIRECT reads place every source at page pitch).
 * Only a --complete run's records are its whole input: a --partial run reads
 * every holder's chunk of each changed stripe, which the changelog's records
 * do not list, so it keeps the library's default slabs (0). */
static uint64_t job_bytes_of(const bcp_eventset *es, int complete)
{
    if (!complete)
        return 0;
    uint64_t total = 0;
    const size_t n = bcp_eventset_count(es);
    for (size_t i = 0; i < n; i++) {
        const char *p;
        int64_t ts;
        uint64_t m, d, sz = 0;
        if (bcp_eventset_get(es, i, &p, &ts, &m, &d, &sz) == 0)
            total += sz + 4096;
    }
    return total;
}

static int fail(const char *what, int rc)
{
    fprintf(stderr, "bcp: %s: %s\n", what, strerror(rc < 0 ? -rc : rc));
    return 1;
}

static int rm_visit(const char *p, const struct stat *sb, int flag, struct FTW *ftw)
{
    (void)sb;
    (void)flag;
    if (ftw->level == 0)
        return 0; /* keep the directory itself */
    return remove(p) != 0 && errno != ENOENT;
}

static int clear_dir(const char *dir)
{
    struct stat sb;
    if (stat(dir, &sb) != 0)
        return errno == ENOENT ? 0 : -errno;
    return nftw(dir, rm_visit, 64, FTW_DEPTH | FTW_PHYS) == 0 ? 0 : -EIO;
}

static int cmd_find(int argc, char **argv)
{
    if (argc != 1)
        return usage();
    int rc = bcp_scan_chunks(argv[0], STDOUT_FILENO, NULL);
    return rc ? fail("find-all-chunks", rc) : 0;
}

static double now_s(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + (double)t.tv_nsec * 1e-9;
}

static int cmd_gen(int argc, char **argv)
{
    const double t_start = now_s();
    int complete = -1, engines = 0, use_pipeline = 1, use_procs = 0, lanes = 12, force = 0, read_arg = 0, fold_arg = 0;
    int q_parity = 0, q_windowed = 0;
    const char *changelog = NULL;
    int i = 0;
    for (; i < argc && argv[i][0] == '-'; i++) {
        if (!strcmp(argv[i], "--complete"))
            complete = 1;
        else if (!strcmp(argv[i], "--partial"))
            complete = 0;
        else if (!strcmp(argv[i], "--pipeline"))
            engines++, use_pipeline = 1;
        else if (!strcmp(argv[i], "--protocol"))
            engines++, use_pipeline = 0;
        else if (!strcmp(argv[i], "--procs"))
            engines++, use_pipeline = 0, use_procs = 1;
        else if (!strcmp(argv[i], "--fold") && i + 1 < argc) {
            fold_arg = 1;
            if (fold_mode_arg(argv[++i]) < 0 || bcp_task_set_fold_mode(fold_mode_arg(argv[i])) < 0)
                return usage();
        }
        else if (!strcmp(argv[i], "--read") && i + 1 < argc) {
            read_arg = 1;
            if ((g_read_mode = read_mode_arg(argv[++i])) < 0)
                return usage();
        }
        else if (!strcmp(argv[i], "--force"))
            force = 1;
        else if (!strcmp(argv[i], "--q"))
            q_parity = 1;
        else if (!strcmp(argv[i], "--q-windowed"))
            q_parity = q_windowed = 1;
        else if (!strcmp(argv[i], "--lanes") && i + 1 < argc)
            lanes = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--changelog") && i + 1 < argc)
            changelog = argv[++i];
        else
            return usage();
    }
    if (complete < 0 || argc - i != 2 || engines > 1 || (read_arg && !use_pipeline) || (fold_arg && use_pipeline) ||
        (q_parity && !use_pipeline))
        return usage();
    const char *root = argv[i];
    const int ntargets = atoi(argv[i + 1]);
    if (ntargets < 1 || ntargets > MAX_STORAGE_TARGETS || lanes < 1 || lanes > 64)
        return usage();
    char p[4096];
    snprintf(p, sizeof(p), "%s/run_data", root);
    int rc = bcp_check_targets(root, ntargets, p, stderr);
    if (rc)
        return fail("storage targets", rc);
    char ts_path[4096];
    snprintf(ts_path, sizeof(ts_path), "%s/last-gen-timestamp", root);
    struct stat sb;
    if (complete && stat(ts_path, &sb) == 0) {
        if (!force) {
            fputs("bcp: a complete run has already been done; --force deletes all existing parity data\n", stderr);
            return 1;
        }
        for (int k = 0; k < ntargets; k++) {
            snprintf(p, sizeof(p), "%s/st%d/parity", root, k);
            if ((rc = clear_dir(p)))
                return fail("removing old parity data", rc);
            snprintf(p, sizeof(p), "%s/st%d/parityq", root, k);
            if ((rc = clear_dir(p)))
                return fail("removing old parity data", rc);
            snprintf(p, sizeof(p), "%s/st%d/db", root, k);
            if ((rc = clear_dir(p)))
                return fail("removing old parity databases", rc);
        }
    }
    const time_t started = time(NULL);
    const double t_phase1 = now_s();
    bcp_eventset *es = NULL;
    if ((rc = bcp_eventset_create(&es)))
        return fail("event set", rc);
    uint64_t nrec = 0;
    for (int k = 0; k < ntargets && !rc; k++) {
        if (complete) {
            uint64_t n = 0;
            snprintf(p, sizeof(p), "%s/st%d/chunks", root, k);
            rc = bcp_eventset_scan(es, k, p, &n);
            nrec += n;
        } else {
            if (changelog)
                snprintf(p, sizeof(p), "%s/st%d", changelog, k);
            else
                snprintf(p, sizeof(p), "%s/changelog/st%d", root, k);
            if (stat(p, &sb) == 0)
                rc = bcp_eventset_feed_file(es, k, p);
        }
    }
    if (rc) {
        bcp_eventset_destroy(es);
        return fail(complete ? "scanning chunks" : "reading changelog", rc);
    }
    printf("Total number of events found: %8zu\n", bcp_eventset_count(es));
    const double t_round = now_s();
    double t_setup = t_round;
    bcp_run_stats st;
    memset(&st, 0, sizeof(st));
    size_t planned = 0;
    if (use_pipeline) {
        bcp_pipeline *pl = NULL;
        rc = pipeline_on_all_gpus(&pl, job_bytes_of(es, complete == 1));
        t_setup = now_s();
        if (!rc && q_parity)
            rc = bcp_pipeline_set_q_parity(pl, 1);
        if (!rc && q_windowed)
            rc = bcp_pipeline_set_q_windowed(pl, 1);
        if (!rc)
            rc = bcp_gen_round_pipeline(pl, root, ntargets, es, NULL, stderr, &st, &planned);
        if (pl)
            bcp_pipeline_destroy(pl);
    } else if (use_procs) {
        rc = bcp_gen_round_procs(root, ntargets, es, NULL, lanes, stderr, &st, &planned);
    } else {
        rc = bcp_gen_round(root, ntargets, es, NULL, lanes, stderr, &st, &planned);
        bcp_task_shutdown();
    }
    bcp_eventset_destroy(es);
    if (rc)
        return fail("parity generation", rc);
    const double t_end = now_s();
    printf("worklist %zu items, %llu tasks, %.3f s, %.1f MiB read, %.1f MiB written, %d rank errors, "
           "%llu refused (%s)\n",
           planned, (unsigned long long)st.tasks, st.seconds, st.bytes_read / 1048576.0,
           st.bytes_written / 1048576.0, st.errors, (unsigned long long)st.refused,
           use_pipeline ? "pipeline" : use_procs ? "rank processes" : "protocol");
    /* stage timings, as the reference's rank 0 prints them (gen/main.c:920-928) */
    printf("timings: init %.3f s, phase1 %.3f s, engine setup %.3f s, round %.3f s (run %.3f s), total %.3f s\n",
           t_phase1 - t_start, t_round - t_phase1, t_setup - t_round, t_end - t_setup, st.seconds, t_end - t_start);
    if (st.refused)
        fprintf(stderr, "bcp: %llu item(s) refused: paths outside the store have no parity\n",
                (unsigned long long)st.refused);
    if (st.errors || st.refused)
        return 1;
    FILE *f = fopen(ts_path, "w");
    if (!f)
        return fail("last-gen-timestamp", errno);
    fprintf(f, "%lld\n", (long long)started);
    fclose(f);
    (void)nrec;
    return 0;
}

static int cmd_rebuild(int argc, char **argv)
{
    const char *db = NULL, *corrupt = NULL, *lost = NULL;
    int engines = 0, use_pipeline = 1, use_procs = 0, read_arg = 0, fold_arg = 0, also = -1, also_arg = 0;
    int q_windowed = 0;
    int i = 0;
    for (; i < argc && argv[i][0] == '-'; i++) {
        if (!strcmp(argv[i], "--db") && i + 1 < argc)
            db = argv[++i];
        else if (!strcmp(argv[i], "--corrupt") && i + 1 < argc)
            corrupt = argv[++i];
        else if (!strcmp(argv[i], "--lost") && i + 1 < argc)
            lost = argv[++i];
        else if (!strcmp(argv[i], "--also") && i + 1 < argc) {
            char *end = NULL;
            also = (int)strtol(argv[++i], &end, 10);
            if (!*argv[i] || *end || also < 0)
                return usage();
            also_arg = 1;
        } else if (!strcmp(argv[i], "--q-windowed"))
            q_windowed = 1;
        else if (!strcmp(argv[i], "--pipeline"))
            engines++, use_pipeline = 1;
        else if (!strcmp(argv[i], "--protocol"))
            engines++, use_pipeline = 0;
        else if (!strcmp(argv[i], "--procs"))
            engines++, use_pipeline = 0, use_procs = 1;
        else if (!strcmp(argv[i], "--fold") && i + 1 < argc) {
            fold_arg = 1;
            if (fold_mode_arg(argv[++i]) < 0 || bcp_task_set_fold_mode(fold_mode_arg(argv[i])) < 0)
                return usage();
        } else if (!strcmp(argv[i], "--read") && i + 1 < argc) {
            read_arg = 1;
            if ((g_read_mode = read_mode_arg(argv[++i])) < 0)
                return usage();
        } else if (!strcmp(argv[i], "--lanes") && i + 1 < argc) {
            if (bcp_task_set_rebuild_lanes(atoi(argv[++i])) < 0) /* (the reference rebuilds with one) */
                return usage();
        } else
            return usage();
    }
    if (argc - i != 3 || engines > 1 || (read_arg && !use_pipeline) || (fold_arg && use_pipeline))
        return usage();
    const char *root = argv[i];
    const int ntargets = atoi(argv[i + 1]), target = atoi(argv[i + 2]);
    if ((also_arg || lost || q_windowed) && (!use_pipeline || !also_arg || also == target || also >= ntargets))
        return usage();
    bcp_run_stats st;
    bcp_rebuild2_stats st2;
    memset(&st, 0, sizeof(st));
    memset(&st2, 0, sizeof(st2));
    int rc;
    if (use_pipeline || use_procs) {
        char dp[4096];
        if (!db) {
            int from = 0; /* the first target that is not lost */
            while (from == target || from == also)
                from++;
            snprintf(dp, sizeof(dp), "%s/st%d/db", root, from);
            db = dp;
        }
        struct stat sb;
        bcp_pdb *pdb = NULL;
        bcp_work_item *items = NULL;
        size_t n = 0;
        rc = stat(db, &sb) == 0 ? 0 : -errno;
        if (!rc)
            rc = bcp_pdb_open(db, DB_VERSION, &pdb);
        if (!rc) {
            rc = bcp_pdb_items(pdb, &items, &n);
            bcp_pdb_close(pdb);
        }
        if (!rc && use_procs) {
            rc = bcp_rebuild_run_procs(root, ntargets, target, items, n, corrupt, stderr, &st);
        } else if (!rc) {
            bcp_pipeline *pl = NULL;
            rc = pipeline_on_all_gpus(&pl, 0);
            if (!rc && q_windowed)
                rc = bcp_pipeline_set_q_windowed(pl, 1);
            if (!rc)
                rc = also_arg ? bcp_pipeline_rebuild2(pl, root, ntargets, target, also, items, n, corrupt, lost, stderr,
                                                      &st, &st2)
                              : bcp_pipeline_rebuild(pl, root, ntargets, target, items, n, corrupt, stderr, &st);
            if (pl)
                bcp_pipeline_destroy(pl);
        }
        bcp_pdb_items_free(items);
    } else {
        rc = bcp_rebuild_run_db(root, ntargets, target, db, corrupt, stderr, &st);
        bcp_task_shutdown();
    }
    if (rc)
        return fail("rebuild", rc);
    printf("rebuilt target %d: %llu tasks, %.3f s, %.1f MiB read, %.1f MiB written, %d rank errors, "
           "%llu refused (%s)\n",
           target, (unsigned long long)st.tasks, st.seconds, st.bytes_read / 1048576.0,
           st.bytes_written / 1048576.0, st.errors, (unsigned long long)st.refused,
           use_pipeline ? "pipeline" : use_procs ? "rank processes" : "protocol");
    if (also_arg)
        printf("also target %d: %llu items from P, %llu from Q, %llu from P and Q, %llu unrecoverable\n", also,
               (unsigned long long)st2.xor_items, (unsigned long long)st2.q_items, (unsigned long long)st2.pq_items,
               (unsigned long long)st2.unrecoverable);
    return (st.errors || st.refused || st2.unrecoverable) ? 1 : 0;
}

static int cmd_verify(int argc, char **argv)
{
    const char *db = NULL, *bad = NULL, *culprits = NULL, *repaired = NULL;
    int i = 0, with_q = 0, q_windowed = 0, repair = 0, dry_run = 0, bad_repair = 0, repair_windowed = 0;
    long members = 1;
    for (; i < argc && argv[i][0] == '-'; i++) {
        if (!strcmp(argv[i], "--db") && i + 1 < argc)
            db = argv[++i];
        else if (!strcmp(argv[i], "--bad") && i + 1 < argc)
            bad = argv[++i];
        else if (!strcmp(argv[i], "--culprits") && i + 1 < argc)
            culprits = argv[++i];
        else if (!strcmp(argv[i], "--q"))
            with_q = 1;
        else if (!strcmp(argv[i], "--q-windowed"))
            q_windowed = 1;
        else if (!strcmp(argv[i], "--repair") && i + 1 < argc) {
            i++;
            repair = !strcmp(argv[i], "parity") ? BCP_REPAIR_PARITY : !strcmp(argv[i], "all") ? BCP_REPAIR_ALL : 0;
            bad_repair |= !repair;
        } else if (!strcmp(argv[i], "--repair-members") && i + 1 < argc) {
            char *end;
            members = strtol(argv[++i], &end, 10);
            bad_repair |= *end || members < 1 || members > MAX_STORAGE_TARGETS + 2;
        } else if (!strcmp(argv[i], "--dry-run"))
            dry_run = 1;
        else if (!strcmp(argv[i], "--repair-windowed"))
            repair_windowed = 1;
        else if (!strcmp(argv[i], "--repaired") && i + 1 < argc)
            repaired = argv[++i];
        else if (!strcmp(argv[i], "--read") && i + 1 < argc) {
            if ((g_read_mode = read_mode_arg(argv[++i])) < 0)
                return usage();
        } else
            return usage();
    }
    if (bad_repair || (repair && !with_q) || ((members != 1 || dry_run || repaired) && !repair) ||
        (repair_windowed && (!repair || !q_windowed))) {
        usage();
        return 2;
    }
    if (argc - i != 2 || ((culprits || q_windowed) && !with_q))
        return usage();
    const char *root = argv[i];
    const int ntargets = atoi(argv[i + 1]);
    if (ntargets < 1 || ntargets > MAX_STORAGE_TARGETS)
        return usage();
    char dp[4096];
    if (!db) {
        snprintf(dp, sizeof(dp), "%s/st0/db", root);
        db = dp;
    }
    struct stat sb;
    bcp_pdb *pdb = NULL;
    bcp_work_item *items = NULL;
    size_t n = 0;
    bcp_verify_stats vs;
    bcp_verify_q_stats qs;
    bcp_repair_q_stats rs;
    memset(&vs, 0, sizeof(vs));
    memset(&qs, 0, sizeof(qs));
    memset(&rs, 0, sizeof(rs));
    int rc = stat(db, &sb) == 0 ? 0 : -errno;
    if (!rc)
        rc = bcp_pdb_open(db, DB_VERSION, &pdb);
    if (!rc) {
        rc = bcp_pdb_items(pdb, &items, &n);
        bcp_pdb_close(pdb);
    }
    if (!rc) {
        bcp_pipeline *pl = NULL;
        rc = pipeline_on_all_gpus(&pl, 0);
        if (!rc && q_windowed)
            rc = bcp_pipeline_set_q_windowed(pl, 1);
        if (!rc && repair_windowed)
            rc = bcp_pipeline_set_repair_windowed(pl, 1);
        if (!rc && repair) {
            rc = bcp_pipeline_repair_q(pl, root, ntargets, items, n, repair, (uint32_t)members, dry_run, NULL, bad,
                                       culprits, repaired, stderr, &rs);
            qs = rs.q;
            vs = qs.v;
        } else if (!rc && with_q) {
            rc = bcp_pipeline_verify_q(pl, root, ntargets, items, n, NULL, bad, culprits, stderr, &qs);
            vs = qs.v;
        } else if (!rc)
            rc = bcp_pipeline_verify(pl, root, ntargets, items, n, NULL, bad, stderr, &vs);
        if (pl)
            bcp_pipeline_destroy(pl);
    }
    bcp_pdb_items_free(items);
    if (rc)
        return fail("parity-verify", rc);
    printf("verified %llu items: %llu ok, %llu stale, %llu no parity, %llu wrong size, %llu mismatch, %llu skipped "
           "(%llu refused), %d errors, %.3f s, %.1f MiB read\n",
           (unsigned long long)vs.items, (unsigned long long)vs.ok, (unsigned long long)vs.stale,
           (unsigned long long)vs.no_parity, (unsigned long long)vs.size, (unsigned long long)vs.mismatch,
           (unsigned long long)vs.skipped, (unsigned long long)vs.refused, vs.errors, vs.seconds,
           vs.bytes_read / 1048576.0);
    if (with_q)
        printf("q files: %llu checked, %llu none, %llu bad; culprits: %llu data, %llu p, %llu q, %llu many\n",
               (unsigned long long)qs.q_checked, (unsigned long long)qs.q_none, (unsigned long long)qs.q_bad,
               (unsigned long long)qs.culprit_data, (unsigned long long)qs.culprit_p,
               (unsigned long long)qs.culprit_q, (unsigned long long)qs.culprit_many);
    if (repair) {
        printf("repair (%s%s): %llu done, %llu dry, %llu policy, %llu unlocated, %llu changed, %llu failed; "
               "%llu files, %llu bytes written, %llu launches\n",
               repair == BCP_REPAIR_ALL ? "all" : "parity", dry_run ? ", dry run" : "", (unsigned long long)rs.done,
               (unsigned long long)rs.dry, (unsigned long long)rs.policy, (unsigned long long)rs.unlocated,
               (unsigned long long)rs.changed, (unsigned long long)rs.failed, (unsigned long long)rs.files_written,
               (unsigned long long)rs.bytes_written, (unsigned long long)rs.repair_launches);
        if (!dry_run) /* a mismatch that was repaired is no longer one */
            return (vs.no_parity || qs.q_bad || vs.size || vs.mismatch != rs.done || vs.refused || vs.errors) ? 1 : 0;
    }
    return (vs.no_parity || qs.q_bad || vs.size || vs.mismatch || vs.refused || vs.errors) ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 2)
        return usage();
    if (!strcmp(argv[1], "find-all-chunks"))
        return cmd_find(argc - 2, argv + 2);
    if (!strcmp(argv[1], "parity-gen"))
        return cmd_gen(argc - 2, argv + 2);
    if (!strcmp(argv[1], "parity-rebuild"))
        return cmd_rebuild(argc - 2, argv + 2);
    if (!strcmp(argv[1], "parity-verify"))
        return cmd_verify(argc - 2, argv + 2);
    return usage();
}
