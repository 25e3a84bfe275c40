/* peaksegdisk_hip.h -- C ABI of libpeaksegdisk_hip.so, the MI355X-native drop-in for
 * PeakSegDisk's PeakSegFPOP hot path.
 *
 * Plain C types only (pointers, sizes, ints, doubles).  Each entry point cites the
 * reference interface it replaces; INTEGRATION.md shows the bindings (R `.C` glue, ctypes).
 */
#ifndef PEAKSEGDISK_HIP_H
#define PEAKSEGDISK_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------- */
/* 1..11: identical to /root/reference/src/PeakSegFPOPLog.h:3-13 */
#define ERROR_PENALTY_NOT_FINITE 1
#define ERROR_PENALTY_NEGATIVE 2
#define ERROR_UNABLE_TO_OPEN_BEDGRAPH 3
#define ERROR_NOT_ENOUGH_COLUMNS 4
#define ERROR_NON_INTEGER_DATA 5
#define ERROR_INCONSISTENT_CHROMSTART_CHROMEND 6
#define ERROR_WRITING_COST_FUNCTIONS 7
#define ERROR_WRITING_LOSS_OUTPUT 8
#define ERROR_NO_DATA 9
#define ERROR_PENALTY_NOT_NUMERIC 10
#define ERROR_WRITING_SEGMENTS_OUTPUT 11
/* additions of this implementation (the reference reports "error code %d" for them) */
#define ERROR_NO_HIP_DEVICE 12     /* no MI355X visible: there is no CPU fallback */
#define ERROR_DEVICE_SOLVER 13     /* kernel reported a failure; see peakseg_hip_last_error() */
#define ERROR_DEVICE_MEMORY 14     /* arena / tables do not fit in HBM (or in PEAKSEG_HIP_MAX_BYTES) */
#define ERROR_SEARCH_ARGUMENTS 15  /* PeakSegFPOP_sequential_search: bad arguments / row capacity */
#define ERROR_SEARCH_TOO_MANY_PEAKS 16 /* peaks.int exceeds the maximum for the data; the text of
                                          R/sequentialSearch_dir.R:57-66 is in peakseg_hip_last_error() */
#define ERROR_DENSE_ARGUMENTS 17   /* dense counts that cannot be solved: 2^31 or more bases, a
                                      negative count, counts that sum to 2^53 or more, 2^30 or more
                                      runs; the contig and the reason are in peakseg_hip_last_error() */
#define ERROR_READS_ARGUMENTS 18   /* aligned reads that cannot be piled up: an empty or negative
                                      extent, bases_counted not 0/1, a NULL or misaligned array, a
                                      read with chromStart >= chromEnd or a negative count, counts
                                      that sum to 2^31 or more in a contig; the contig, the read and
                                      the reason are in peakseg_hip_last_error() */

#define ERROR_LABEL_ARGUMENTS 19   /* labels that cannot be counted: a negative number of labels, a
                                      NULL or misaligned array, a label with chromStart >= chromEnd
                                      or an annotation code outside 0..3; the contig, the label's
                                      index and the reason are in peakseg_hip_last_error() */

#define ERROR_FEATURE_ARGUMENTS 20 /* coverage statistics that cannot be computed: a negative number
                                      of ranks or more than peakseg_hip_coverage_stats_max_ranks, a
                                      rank outside 0 .. bases - 1 of its contig; the contig and the
                                      rank are in peakseg_hip_last_error() */

#define ERROR_FIT_ARGUMENTS 21     /* a penalty model that cannot be fitted: a shape outside the
                                      limits, a feature that is not finite, a NaN limit, lo > hi, a
                                      row with both limits infinite, a fold outside [0, F) or one
                                      that leaves no training row, regularizations that are negative
                                      or do not increase, a gram_lambda_max, threshold or
                                      max_iterations that is not positive; the argument and the row
                                      are in peakseg_hip_last_error().  The Python layer raises the
                                      same status when no regularization has all its fits converged */
#define ERROR_REGION_ARGUMENTS 22  /* regions or groups that cannot be served: a negative number of
                                      regions or groups, a NULL or misaligned array, a region with
                                      chromStart >= chromEnd, a problem in a group outside
                                      -1 .. n_groups - 1; the contig and the region, or the problem,
                                      are in peakseg_hip_last_error() */
#define ERROR_HELDOUT_ARGUMENTS 23 /* pairs that cannot be scored: a negative number of pairs, a NULL
                                      or misaligned array, a problem or contig out of range, a scale
                                      that is not finite and positive, a contig that has not the
                                      bases of its problem's contig; the pair is in
                                      peakseg_hip_last_error().  Fold sets: a number of folds that is
                                      not 2, 4 or 8, a base whose count exceeds
                                      peakseg_hip_fold_max_count() */
#define ERROR_STRAND_ARGUMENTS 24  /* stranded reads that cannot be served: a strand that is neither
                                      +1 nor -1, a NULL strand array with reads present, max_shift
                                      below 0 or above peakseg_hip_xcorr_max_shift(), a
                                      fragment_length below 1, an extent with hi <= lo; the contig and
                                      the read, or the argument, are in peakseg_hip_last_error() */
#define ERROR_DEDUP_ARGUMENTS 25   /* a duplicate removal or compaction that cannot be served: keep
                                      below 1, an unknown `by`, five_prime without strands, 2^31 or
                                      more rows in one call, an output that overlaps an input; the
                                      argument is in peakseg_hip_last_error() */

/* ---- environment ---------------------------------------------------------------------
 * PEAKSEG_HIP_DEVICE            GPU used by the file-level entry points (default 0); one process
 *                               per GPU sets it from its rank
 * PEAKSEG_HIP_DEVICES=all|0,1,..  fan-out inside one process (takes precedence over
 *                               PEAKSEG_HIP_DEVICE): PeakSegFPOP_disk_batch, PeakSegFPOP_dir_batch
 *                               and the search batches (PeakSegFPOP_sequential_search_batch,
 *                               PeakSegFPOP_parallel_search_batch) deal their dynamic programs
 *                               (the search batches: their directories) to one shard per listed device,
 *                               longest predicted first, and solve each shard in a problem set of its
 *                               own on a host thread of its own; an id listed twice gets two sets,
 *                               one after the other.  PeakSegFPOP_disk and
 *                               PeakSegFPOP_sequential_search use the first listed device.  A
 *                               malformed list or an id that is not visible: the dynamic programs
 *                               get ERROR_NO_HIP_DEVICE and no shard runs.  Unset or empty: one set
 *                               on PEAKSEG_HIP_DEVICE's device, as without this knob
 * PEAKSEG_HIP_MAX_BYTES         cap on the HBM one problem set (one shard's) may hold (suffix
 *                               K/M/G/T); several processes can then share one GPU (R's future
 *                               workers)
 * PEAKSEG_HIP_PIECES_PER_FUNCTION  arena estimate, pieces per stored cost function (default 7):
 *                               picks the arena's chunk and block sizes; the arena itself grows
 *                               block by block WHILE the kernel runs (a host thread maps ahead of
 *                               what the waves have taken), up to nine tenths of the free HBM or
 *                               PEAKSEG_HIP_MAX_BYTES
 * PEAKSEG_HIP_NO_LIVE_GROWTH=1  map what the estimate asks for at creation and nothing under a
 *                               running kernel: a solve that needs more parks its problems, adds
 *                               blocks and resumes them where they stopped
 * PEAKSEG_HIP_SPILL_CAP / _SPILL_SLOTS  capacity (pieces per list, at most 32767) and initial
 *                               number of slots of the HBM spill pool for functions that outgrow LDS
 * PEAKSEG_HIP_CHECKPOINT=K / PEAKSEG_HIP_NO_CHECKPOINT=1  force / forbid the checkpointed store
 * PEAKSEG_HIP_CKPT_OVERFLOW     initial size (pieces) of the pool that holds checkpoints of functions
 *                               too long for a checkpoint slot (adversarial data)
 * PEAKSEG_HIP_NO_PARK=1         rerun a set that ran out of arena instead of resuming its problems
 * PEAKSEG_HIP_NO_VMM=1          arena blocks from hipMalloc instead of the HIP virtual-memory calls
 *                               (same growth, nothing is ever copied)
 * PEAKSEG_HIP_ARENA_BLOCK_LOG2  tests: log2 of the pieces per arena block (default 19-24)
 * PEAKSEG_HIP_VARIANT=lat|thr|pk  force a build of the forward kernel
 * PEAKSEG_HIP_NO_PACKED=1       the launch planner never picks the packed build (pk)
 * PEAKSEG_HIP_RATES=lat,thr     diagnostic: data points per second per problem the launch planner
 *                               assumes for the latency / throughput build (default: measured by
 *                               this process's earlier solves, else 96000,58000)
 * PEAKSEG_HIP_TIMING=1          phase timings of the file-level calls and of the creation of a
 *                               problem set (the pile-up of reads and the dense encoder's launches included) on
 *                               stderr */

/* ---- the reference's boundary -------------------------------------------------------- */

/* Replaces `int PeakSegFPOP_disk(char*, char*, char*)`
 * (/root/reference/src/PeakSegFPOPLog.h:15, PeakSegFPOPLog.cpp:143-463): same arguments,
 * same status codes, same validation order, byte-identical
 * <bedGraph>_penalty=<pen>_segments.bed / _loss.tsv files.  The dynamic program runs on the
 * GPU and the cost-function store lives in HBM; db_file_name is still opened (status 7 if
 * that fails, as the reference) and is left as a sparse file of exactly the size the
 * reference's database would have, so callers that report its size keep working. */
int PeakSegFPOP_disk(char *bedGraph_file_name, char *penalty_str, char *db_file_name);

/* Additive batch form of the same call for penalty grids: problem i is
 * (bedGraph_files[i], penalty_strs[i], db_files[i]); every distinct bedGraph file is parsed
 * and uploaded once, all dynamic programs run concurrently (one workgroup each), and the
 * output files are byte-identical to n separate PeakSegFPOP_disk calls.  status_out[i]
 * receives each problem's status; the return value is the first non-zero one (0 if none). */
int PeakSegFPOP_disk_batch(int n_problems, char **bedGraph_files, char **penalty_strs,
                           char **db_files, int *status_out);

/* PeakSegFPOP_dir for a batch of (problem directory, penalty string) pairs
 * (/root/reference/R/PeakSegFPOP_dir.R:64-117 over R/PeakSegFPOP_file.R:57-86): pairs whose
 * coverage.bedGraph_penalty=<pen>_{segments.bed,loss.tsv,timing.tsv} files exist and pass the
 * reference's consistency test are skipped (cached_out[i] = 1); the rest are solved in one
 * PeakSegFPOP_disk_batch (default database name, removed afterwards) and get their _timing.tsv
 * (penalty, megabytes = size of the reference's database / 2^20, seconds = the problem's share
 * of the batch's wall time).  Returns the first non-zero status (0 if none). */
int PeakSegFPOP_dir_batch(int n_problems, char **problem_dirs, char **penalty_strs,
                          int *status_out, int *cached_out);

/* One model visited by the penalty search: a row of sequentialSearch_dir's $others. */
typedef struct {
  char penalty_str[40];  /* paste(penalty): names the result files of this model */
  double penalty;        /* loss.tsv column 1 */
  double total_loss;     /* loss.tsv column 7 */
  int peaks, segments, bases;
  int iteration;         /* 1-based */
  int under_peaks, over_peaks; /* peaks of the bracket when the model was requested; INT_MIN = NA */
  int cached;            /* result files were reused, no dynamic program ran */
} psd_search_row;

/* sequentialSearch_dir(problem.dir, peaks.int) (/root/reference/R/sequentialSearch_dir.R:22-103)
 * next to the solver: the same loop, the same penalties (R's 15-significant-digit paste() of
 * each secant step) and the same files as the reference leaves behind for every model --
 * PeakSegFPOP_dir's cache included -- but coverage.bedGraph is parsed and uploaded once and the
 * arena is reused from one penalty to the next.  rows[0..*n_rows) are the models in the order
 * they were requested (iteration 1: "0" then "Inf"); *chosen_row is the returned model.
 * Status: 0, a solver status, ERROR_SEARCH_TOO_MANY_PEAKS or ERROR_SEARCH_ARGUMENTS. */
int PeakSegFPOP_sequential_search(const char *problem_dir, int peaks_int, int verbose,
                                  int row_capacity, psd_search_row *rows, int *n_rows,
                                  int *chosen_row);

/* The same search over several problem directories at once (additive: the reference runs one
 * R process per directory, /root/reference/R/sequentialSearch_dir.R:34-38 with a `future`
 * plan).  Every directory follows its own search -- the penalties, files and rows are those
 * of PeakSegFPOP_sequential_search on that directory alone -- but the models the searches ask
 * for in the same iteration are computed in one launch (PeakSegFPOP_dir_batch), so a set of
 * contigs is searched in about the time of its longest search.  rows: n_dirs x row_capacity
 * (directory d at rows + d*row_capacity); n_rows, chosen_row, status_out: one per directory
 * (a directory whose search fails keeps its status and the others go on).  Returns the first
 * non-zero status. */
int PeakSegFPOP_sequential_search_batch(int n_dirs, char **problem_dirs, const int *peaks_int,
                                        int verbose, int row_capacity, psd_search_row *rows,
                                        int *n_rows, int *chosen_row, int *status_out);

/* A penalty search that asks for `width` models per round instead of one (additive; the
 * sequential entries above keep the reference's exact penalty sequence).  Round 1 is the
 * reference's: penalties "0" and "Inf" and the max.peaks check.  Every later round requests,
 * first, the reference's secant penalty of the bracket (under, over) at its start and, after it,
 * up to width-1 penalties strictly inside the bracket, placed by a pure function of the bracket
 * rows, the target and width; all of a round's models are computed in ONE
 * PeakSegFPOP_dir_batch call, which deals them over PEAKSEG_HIP_DEVICES when that is set.  The
 * secant model decides as the reference's one model does (peaks equal to a bracket end's: no
 * model lies between, the search ends with `under`); otherwise every model of the round may
 * narrow the bracket, and a model with exactly peaks_int peaks ends the search (the one with the
 * largest penalty if several have).  The chosen model never has more peaks than asked.  Every row
 * leaves the reference's three files and consistent files are reused (cached = 1).  rows: the
 * models in the order requested, `iteration` = the round, under_peaks / over_peaks = the bracket
 * at the round's start.  width: 1 = the sequence of PeakSegFPOP_sequential_search, 0 = the
 * default (8), at most 256.  A round whose launch reports ERROR_DEVICE_MEMORY is repeated for
 * its missing models at half the width, which the rest of the search keeps.
 * peakseg_hip_last_fanout* describe the last round's PeakSegFPOP_dir_batch.
 * Status: 0, a solver status, ERROR_SEARCH_TOO_MANY_PEAKS or ERROR_SEARCH_ARGUMENTS. */
int PeakSegFPOP_parallel_search(const char *problem_dir, int peaks_int, int width, int verbose,
                                int row_capacity, psd_search_row *rows, int *n_rows,
                                int *chosen_row);

/* The parallel search over several problem directories in lockstep: all models every active
 * directory wants in a round go into one PeakSegFPOP_dir_batch call, and each directory ends
 * with the rows and files of PeakSegFPOP_parallel_search on that directory alone.  Arrays as for
 * PeakSegFPOP_sequential_search_batch; a directory listed twice is refused, a failing directory
 * keeps its status and the others go on.  Under PEAKSEG_HIP_DEVICES the directories are dealt
 * to one shard per listed device, as the sequential batch deals them.  Returns the first
 * non-zero status. */
int PeakSegFPOP_parallel_search_batch(int n_dirs, char **problem_dirs, const int *peaks_int,
                                      int width, int verbose, int row_capacity,
                                      psd_search_row *rows, int *n_rows, int *chosen_row,
                                      int *status_out);

/* The text the reference's glue passes to Rf_error for a status
 * (/root/reference/src/interface.cpp:16-55); returns buf; empty string for status 0. */
char *PeakSegFPOP_status_message(int status, const char *bedGraph, const char *penalty,
                                 const char *db, char *buf, size_t buf_len);

/* Where "problem: %d items on line %d" goes (the reference Rprintf()s it,
 * PeakSegFPOPLog.cpp:181).  NULL restores the default (stdout).  It is only ever called on the
 * thread that called the entry point: the shard threads of PEAKSEG_HIP_DEVICES hand their lines
 * to it, complete lines at a time, each directory's in their order. */
void peakseg_hip_set_print(void (*print)(const char *text));

/* What PEAKSEG_HIP_DEVICES did in the calling thread's last file-level call.  Returns S, the
 * number of shards (the length of the device list), or 0 when that call did not fan out (knob
 * unset or bad, a single-program entry point, or no dynamic program to deal).  Per shard, up to
 * `capacity` of them: its device, the dynamic programs it solved and the seconds its problem
 * sets existed (creation, solve, results, destruction; any array may be NULL).  After the join
 * the calling thread's peakseg_hip_last_error() holds the first failing shard's text and
 * peakseg_hip_last_warning() the first shard warning, in shard order. */
int peakseg_hip_last_fanout(int capacity, int *shard_device, int *shard_programs,
                            double *shard_seconds);
/* For each of the first n entries of that call in input order (a problem; a directory for the
 * search batch): the shard that solved it, or -1 where none did (a cache hit, a trivial model, a
 * failure before the dynamic program, or no fan-out).  A duplicated entry reports the shard of
 * its first copy.  Returns the number of entries of that call. */
int peakseg_hip_last_fanout_entries(int n, int *shard_of);

/* ---- device-resident problem sets (penalty x contig grids, benchmarking) ------------ */

typedef struct psd_problem_set psd_problem_set;

typedef struct {
  int status;             /* 0, or ERROR_DEVICE_* */
  int kernel_status;      /* PST_* detail from the kernel */
  int n_segments;
  int n_peaks;
  int n_equality_constraints;
  int max_intervals;
  unsigned long long total_intervals;
  double best_cost;       /* mean penalized cost (loss.tsv column 6) */
  int n_serial_env;       /* diagnostics: min-envelope calls replayed sequentially */
  int step_reached;
  int spill_steps;        /* data points processed with the piece lists spilled to HBM */
} psd_result;

int peakseg_hip_device_count(void);
/* shader clock of a device in kHz, 0 when unknown */
int peakseg_hip_device_clock_khz(int device);
/* text of the calling thread's last FAILURE (statuses >= 12 carry their detail here) */
const char *peakseg_hip_last_error(void);
/* Something worth knowing about the calling thread's last problem-set solve although it
 * succeeded (e.g. the mixed launch's wait for its latency-build workgroups ran into its bound);
 * "" when there is nothing.  Never part of an error message. */
const char *peakseg_hip_last_warning(void);

/* Upload contigs (count = 4th bedGraph column, weight = chromEnd-chromStart) and the
 * problem list to HBM and allocate the arena (arena_pieces = 0: sized automatically and
 * grown on demand).  One problem = one (contig, penalty) dynamic program. */
int peakseg_hip_problem_set_create(int device, int n_contigs, const int *contig_n_bins,
                                   const int *const *contig_count,
                                   const int *const *contig_weight, int n_problems,
                                   const int *problem_contig, const double *problem_penalty,
                                   unsigned long long arena_pieces, psd_problem_set **out);

/* The same set from DENSE coverage: contig c is contig_n_bases[c] int32 counts, one per base, and
 * the run-length encoding happens on the device (three launches per call however many contigs it
 * has; a run starts at a contig's first base and wherever a count differs from the one before
 * it).  counts_on_device = 0: contig_counts[] are host arrays, uploaded and freed again after the
 * encoding; 1: they are device addresses (multiples of 4) on `device`, read in place -- by
 * launches on the null stream, so after everything the caller has queued there -- and not
 * referred to after the call returns.  From there on the set is one of
 * peakseg_hip_problem_set_create: contig_n_bins = the runs, count = the run's count, weight = its
 * length; every call below works on it.  In addition it keeps run_end[] (offset of each run's last
 * base + 1 from the contig's first base), which peakseg_hip_problem_set_pack_segments needs, and
 * it knows its trivial models (penalty +Inf, or a contig whose counts are all equal: the
 * reference's one-segment branch, PeakSegFPOPLog.cpp:224-243): solve launches only the other
 * problems, and result / segments / pack_tables / pack_segments / loss serve the closed form.
 * Checks, in this order: penalties (NaN: ERROR_PENALTY_NOT_FINITE, negative:
 * ERROR_PENALTY_NEGATIVE, +Inf is allowed); a contig without bases: ERROR_NO_DATA, with 2^31 or
 * more: ERROR_DENSE_ARGUMENTS; the device: ERROR_NO_HIP_DEVICE (there is no host encoder); what
 * the encoder finds -- a negative count, counts that sum to 2^53 or more (the reference's double
 * accumulation would round), 2^30 or more runs in a contig: ERROR_DENSE_ARGUMENTS. */
int peakseg_hip_problem_set_create_dense(int device, int n_contigs,
                                         const long long *contig_n_bases,
                                         const int *const *contig_counts, int counts_on_device,
                                         int n_problems, const int *problem_contig,
                                         const double *problem_penalty,
                                         unsigned long long arena_pieces, psd_problem_set **out);

/* The same set from ALIGNED READS: contig c has n_reads[c] reads, read i covering the bases
 * [read_start[c][i], read_end[c][i]) read_count[c][i] times (read_count NULL, or NULL for a contig:
 * every read counts 1), in any order.  The coverage of the contig's extent
 * [extent_start[c], extent_end[c]) is piled up on the device -- +count where a read starts, -count
 * where it ends, prefix sum; four launches per call however many contigs it has -- into a buffer
 * of one int32 per base, which the dense encoder reads in place and which is freed when the
 * encoding ends.  bases_counted = 0: every base of a read counts; 1: only its last base
 * (the interval [end - 1, end)).  A read is clipped to the extent; one that misses it adds nothing;
 * a contig with no read inside its extent has all-zero coverage (the one-segment model).
 * reads_on_device = 0: the arrays are host arrays, uploaded; 1: device addresses (multiples of 4) on
 * `device`, read in place by launches on the null stream and not referred to after the call.
 * From the encoder on the set is one of peakseg_hip_problem_set_create_dense, with base 0 of contig
 * c at extent_start[c]: pass that as first_chromStart for genomic coordinates.
 * Checks, in this order: penalties (as above); n_contigs <= 0: ERROR_NO_DATA; what the host sees --
 * extent_end <= extent_start, extent_start < 0, bases_counted not 0/1, a NULL array where
 * n_reads > 0, n_reads < 0, a device address that is no multiple of 4: ERROR_READS_ARGUMENTS; the
 * device: ERROR_NO_HIP_DEVICE; what the pile-up finds -- a read with start >= end or a negative
 * count (the first such read of the contig is named), good reads' counts that sum to 2^31 or more
 * in a contig (a coverage value could overflow; reads outside the extent count too):
 * ERROR_READS_ARGUMENTS, and nothing further is launched; then what the encoder refuses
 * (ERROR_DENSE_ARGUMENTS). */
int peakseg_hip_problem_set_create_reads(int device, int n_contigs, const long long *n_reads,
                                         const int *const *read_start, const int *const *read_end,
                                         const int *const *read_count, int reads_on_device,
                                         const int *extent_start, const int *extent_end,
                                         int bases_counted, int n_problems, const int *problem_contig,
                                         const double *problem_penalty,
                                         unsigned long long arena_pieces, psd_problem_set **out);

/* Run forward DP + backtrack for every problem of the set; inputs are already resident.
 * *forward_ms = duration of the kernel, measured with HIP events on the stream it runs on.
 * Each workgroup decodes its segmentation right after its last data point, inside the same
 * kernel, so there is no separate backtrack launch: *backtrack_ms is always 0. */
int peakseg_hip_problem_set_solve(psd_problem_set *set, float *forward_ms, float *backtrack_ms);

int peakseg_hip_problem_set_result(psd_problem_set *set, int problem, psd_result *out);

/* Segment table of one problem in the reference's output order (last segment first):
 * seg_start[r] = index of the data point whose chromEnd starts segment r (-1: the first
 * chromStart), seg_mean[r] = segment mean.  Returns the number of rows, or -1. */
int peakseg_hip_problem_set_segments(psd_problem_set *set, int problem, int capacity,
                                     int *seg_start, double *seg_mean);

/* Debug/parity aid: write one problem's in-HBM cost-function store in the byte layout of
 * the reference's DiskVector file (PeakSegFPOPLog.cpp:12-34,76-141); chromEnd[] supplies
 * the per-function chromEnd field. */
int peakseg_hip_problem_set_export_db(psd_problem_set *set, int problem, const int *chromEnd,
                                      const char *path);

/* Which build of the forward kernel the last solve used: "lat" (latency build: helper waves,
 * one workgroup per CU; sets of at most one problem per CU), "thr" (throughput build:
 * 4 workgroups per CU, 64-piece lists), "pk" (packed build: 6 workgroups per CU, 40-piece lists;
 * problems whose functions outgrow them go on, from the data point reached, on a wider build),
 * or "lat+thr" / "lat+pk" (a set that oversubscribes the chip with contigs of unequal length: its
 * longest problems on the latency build, the rest packed, concurrently).  The planner takes
 * the build it predicts to finish the set first; same results whichever it is.
 * PEAKSEG_HIP_VARIANT=lat|thr|pk overrides the choice, PEAKSEG_HIP_NO_PACKED=1 excludes pk. */
const char *peakseg_hip_problem_set_kernel_build(psd_problem_set *set);

/* bytes of HBM held by the set (arena + tables) */
unsigned long long peakseg_hip_problem_set_bytes(psd_problem_set *set);

/* 0 when every cost function is kept in HBM (the reference's store, in memory), K > 0 when the
 * set uses the checkpointed store: only a checkpoint every K data points is kept and the
 * decoding recomputes the blocks it walks through (chosen automatically when the full store
 * would not fit; PEAKSEG_HIP_CHECKPOINT=K forces it, PEAKSEG_HIP_NO_CHECKPOINT=1 forbids it). */
int peakseg_hip_problem_set_checkpoint_interval(psd_problem_set *set);

/* bytes of the arena the last solve handed out (whole chunks) */
unsigned long long peakseg_hip_problem_set_arena_bytes_used(psd_problem_set *set);

/* How the last solve went: kernel launches (1 unless a store ran out between launches: blocks
 * are added to the arena and the problems it had parked are resumed, finished problems are never
 * repeated; growth UNDER the kernel does not count, see peakseg_hip_problem_set_arena_stats) and
 * the data points its launches worked through (the sum of the problems' lengths when nothing
 * was repeated). */
int peakseg_hip_problem_set_solve_stats(psd_problem_set *set, int *launches,
                                        unsigned long long *steps_run);

/* The arena of the set (include/../csrc/fpop_types.h): pieces per block, blocks mapped now, and
 * how many of them the last solve mapped WHILE its kernels ran (0 with
 * PEAKSEG_HIP_NO_LIVE_GROWTH=1, with an explicit arena size and for the checkpointed store). */
int peakseg_hip_problem_set_arena_stats(psd_problem_set *set, unsigned long long *block_pieces,
                                        int *blocks, int *blocks_added_live);

/* How often the last solve parked a problem (the arena had run out; the problem was resumed
 * after more had been mapped) and how many pieces of the overflow pool -- where a parked
 * problem keeps functions too long for its park slot -- those parks took. */
int peakseg_hip_problem_set_park_stats(psd_problem_set *set, int *parks,
                                       unsigned long long *overflow_pool_pieces);

/* ---- The packed results of a set over a history of calls ---------------------------------------
 * Every pack_* function below keeps its result in device tables of the set, which grow to what the
 * largest call so far needed and are never shrunk; its ..._download copies the result of the LAST
 * call to host arrays and returns -1 when nothing is packed.  What ends a packed result, for every
 * pack_* / ..._download pair (tests/test_gpu_resident_tables.py holds each sentence):
 *   the same function, called again   Always, also when that call is refused for its arguments or
 *       for memory: after a refusal nothing is packed, and the next good call is a first call.
 *   peakseg_hip_problem_set_solve     Every result that describes the set's models or was made
 *       from them: pack_tables, pack_segments, pack_segment_stats, pack_label_errors,
 *       pack_peak_clusters, pack_joint_peaks, pack_joint_path, pack_joint_label_errors and
 *       pack_heldout_loss.  From the solve to the next pack call their downloads return -1 and
 *       their device addresses must not be read: no download serves the models of the solve
 *       before.  (pack_joint_peaks and pack_joint_path on GIVEN windows read no model; a solve ends
 *       their results all the same.)  pack_region_stats and pack_coverage_stats read the contigs
 *       only: a solve leaves their results as they are, bit for bit.
 *   another pack_* function           Nothing: every function has tables of its own, and a call
 *       leaves every other function's result and device addresses as they are.  Two exceptions.
 *       pack_joint_path ends what pack_joint_label_errors packed (the label errors are those of
 *       the path).  pack_joint_peaks and pack_joint_path WITHOUT windows take the clusters of their
 *       groups for windows: they pack those clusters exactly as pack_peak_clusters(the same
 *       first_chromStart and groups) would, IN ITS PLACE -- afterwards
 *       packed_peak_clusters_download gives the whole cluster table and matrix of the joint call's
 *       groups, never a mixture with an earlier pack_peak_clusters; when the clusters cannot be
 *       packed, nothing is.
 * Refusals and memory.  A call whose arguments the host can check -- counts, groups, ranks,
 * penalties, and every entry of arrays given in host memory -- is refused before anything is
 * allocated: peakseg_hip_problem_set_bytes is what it was.  Arrays in device memory are checked by
 * the call's first launch, which needs the call's first-level tables.  The functions that return
 * -ERROR_DEVICE_MEMORY ask whether their tables fit (PEAKSEG_HIP_MAX_BYTES, free memory) before
 * they allocate them; a call that needs no more than its tables already hold is never refused for
 * memory.  Growth frees a table before it allocates the larger one, so a set allowed exactly what
 * it held at the end of a history can repeat that history. */

/* Pack the segment tables of a solved set at their exact sizes, IN HBM: problem p's rows
 * (rows_out[p] of them, n_problems entries, host) follow problem p-1's.  Returns the total
 * number of rows, -1 on failure.  *start_dev / *mean_dev receive the device addresses of the
 * packed arrays (valid until the set is solved again or destroyed): what the multi-GPU gather
 * hands to RCCL without a host round trip (peaksegdisk_amd/parallel.py);
 * peakseg_hip_problem_set_packed_download copies them to host arrays of that many rows, and returns
 * -1 when the set has been solved again since the last pack call.  No other pack_* function
 * touches them. */
long long peakseg_hip_problem_set_pack_tables(psd_problem_set *set, long long *rows_out,
                                              const int **start_dev, const double **mean_dev);
int peakseg_hip_problem_set_packed_download(psd_problem_set *set, int *start_out, double *mean_out);

/* The reference's segments table of every problem of a solved set made from dense counts, packed
 * IN HBM like pack_tables (one launch, a workgroup per problem): row r of a problem has
 * chromStart = seg_start < 0 ? first : first + run_end[seg_start], chromEnd = the row before's
 * chromStart (row 0: first + the contig's bases) and its mean; its status is its parity (even:
 * background, odd: peak).  first_chromStart: one per CONTIG, NULL = zeros.  Returns the total
 * number of rows, -1 on failure (a set that was not made from dense counts has no run_end[]).
 * The device addresses stay valid until the set is solved again or destroyed, whatever other pack_*
 * function is called; ..._download copies the columns and returns -1 when the set has been solved
 * again since the last pack call, or that call failed. */
long long peakseg_hip_problem_set_pack_segments(psd_problem_set *set, const int *first_chromStart,
                                                long long *rows_out, const int **chromStart_dev,
                                                const int **chromEnd_dev, const double **mean_dev);
int peakseg_hip_problem_set_packed_segments_download(psd_problem_set *set, int *chromStart_out,
                                                     int *chromEnd_out, double *mean_out);

/* What every row of that segments table holds, from the runs resident in HBM: four more columns,
 * packed in the same row order and at the same row offsets as pack_segments' three.  Row r of a
 * problem covers the runs seg_start[r] + 1 ... seg_start[r - 1] of its contig (row 0: to the
 * contig's last run; seg_start < 0: from run 0), and of those runs
 *   sum          int64  the sum of count[i] * weight[i]: the reads under the segment
 *   max          int32  the largest count[i]
 *   summitStart  int32  first + run_end[i] - weight[i]   of the FIRST run in genomic order whose
 *   summitEnd    int32  first + run_end[i]               count equals max
 * with first = first_chromStart of the contig (one per CONTIG, NULL = zeros; the same 32-bit
 * check as pack_segments).  Integer arithmetic only: the columns are the same whatever the
 * schedule.  A solved set made from dense counts only (-1 and an error text otherwise).  Returns
 * the total number of rows, -1 on failure; rows_out[p] (n_problems entries, host, may be NULL)
 * receives problem p's row count.  The device addresses stay valid until the set is solved again
 * or destroyed, whatever other pack_* function is called; ..._download copies the columns (any may
 * be NULL) to host arrays of that many rows and returns -1 when the set has been solved again since
 * the last pack call, or that call failed. */
long long peakseg_hip_problem_set_pack_segment_stats(psd_problem_set *set, const int *first_chromStart,
                                                     long long *rows_out, const long long **sum_dev,
                                                     const int **max_dev, const int **summitStart_dev,
                                                     const int **summitEnd_dev);
int peakseg_hip_problem_set_packed_segment_stats_download(psd_problem_set *set, long long *sum_out,
                                                          int *max_out, int *summitStart_out,
                                                          int *summitEnd_out);
/* the tile of that launch: runs one workgroup folds (tests aim at its boundaries) */
int peakseg_hip_segment_stats_tile_runs(void);
/* milliseconds (HIP events) of the calling thread's last pack_segment_stats: zeroing and launches */
int peakseg_hip_segment_stats_last_ms(float *ms);

/* The label errors of every problem of a solved set made from dense counts or reads, counted on
 * the device from the resident segment tables (the PeakError convention; coordinates are BED
 * coordinates, 0-based and half-open).  A label is [chromStart, chromEnd) with an annotation code:
 * 0 noPeaks, 1 peakStart, 2 peakEnd, 3 peaks; a peak is an odd row [ps, pe) of the segments table.
 *   noPeaks, peaks  count = peaks with ps < chromEnd && chromStart < pe
 *   peakStart       count = peaks with chromStart <= ps < chromEnd
 *   peakEnd         count = peaks with chromStart < pe <= chromEnd
 * false positive: noPeaks with count >= 1, peakStart / peakEnd with count >= 2; false negative:
 * peaks / peakStart / peakEnd with count == 0.  Labels come in any order, may overlap, and may lie
 * partly or wholly outside the contig.
 * first_chromStart: one per CONTIG, NULL = zeros (the check of pack_segments).  n_labels[c]: the
 * labels of contig c; label_start / label_end / label_annotation: per contig an int32 array of that
 * many entries (not read where n_labels[c] == 0); labels_on_device != 0: the arrays are device
 * addresses (multiples of 4) and are read in place, else host memory that the library uploads.
 * rows_out[p] (n_problems entries, host, may be NULL) receives problem p's row count: its contig's
 * label count.  The packed columns count / fp / fn (int32) hold the problems' rows one problem
 * after the other, in the order of the labels as given; totals holds five int32 per problem:
 * errors, fp, fn, possible_fp (labels that are not peaks), possible_fn (labels that are not
 * noPeaks).  Integer arithmetic only: the same whatever the schedule.
 * Returns the total number of rows; -1 for a set that is not solved or was not made from dense
 * counts; -ERROR_LABEL_ARGUMENTS for what that status names (host arrays are checked on the host,
 * device arrays by the first launch, after which nothing further is launched); the text is in
 * peakseg_hip_last_error.  The device addresses stay valid until the set is solved again, this
 * function is called again, or the set is destroyed, whatever other pack_* function is called;
 * ..._download copies the columns and the totals (any may be NULL) to host arrays and returns -1
 * when there is nothing packed: after a solve, and after a refused call. */
long long peakseg_hip_problem_set_pack_label_errors(
    psd_problem_set *set, const int *first_chromStart, const long long *n_labels,
    const int *const *label_start, const int *const *label_end, const int *const *label_annotation,
    int labels_on_device, long long *rows_out, const int **count_dev, const int **fp_dev,
    const int **fn_dev, const int **totals_dev);
int peakseg_hip_problem_set_packed_label_errors_download(psd_problem_set *set, int *count_out,
                                                         int *fp_out, int *fn_out, int *totals_out);
/* milliseconds (HIP events) of the calling thread's last pack_label_errors: zeroing and launches */
int peakseg_hip_label_errors_last_ms(float *ms);

/* Order statistics and moments of the per-base coverage of every contig of a set made from dense
 * counts or reads, computed on the device from the resident runs: the inputs of a penalty-learning
 * regression (quartiles, mean, sd, bases, runs).  A contig's runs (count_i, weight_i), i < R, stand
 * for the vector x that repeats count_i weight_i times; B = sum of weight_i < 2^31 is its bases.
 *   order statistic  for a 0-based rank r in [0, B): x_(r) is the smallest v with
 *                    sum over count_i <= v of weight_i  >  r, which is sort(x)[r]
 *   moments          six words per contig: bases B, runs R, S1 = sum weight_i count_i, and
 *                    S2 = sum weight_i count_i^2 (up to 2^84) as three sums that each stay below
 *                    2^63: with count = ch 2^16 + cl,  Q0 = sum w cl^2, Q1 = sum w cl ch,
 *                    Q2 = sum w ch^2, and S2 = Q0 + 2^17 Q1 + 2^32 Q2
 * n_ranks: ranks per contig, 0 (moments only) to peakseg_hip_coverage_stats_max_ranks(); ranks:
 * host array, contig c's ranks are ranks[c * n_ranks ...], in any order, repeats allowed.  value
 * (int32, n_contigs * n_ranks) receives the order statistics in the order of the ranks, moments
 * (n_contigs * 6) the words {bases, runs, S1, Q0, Q1, Q2}.  Integer arithmetic only: the same
 * whatever the schedule, and exact for every count in [0, 2^31) and every weight.  The set may be
 * solved or not, and the call leaves what a solve made (the segment tables, the packed columns)
 * as it is.  The number of launches does not depend on the number of contigs: one for the
 * moments and two per 8-bit digit up to the highest one that is not zero in the whole set (counts
 * below 256: one digit pass; full-range counts: four).
 * Returns n_contigs * n_ranks; -1 for a set that was not made from dense counts or reads;
 * -ERROR_FEATURE_ARGUMENTS for n_ranks < 0 or above the maximum and for a rank outside [0, bases)
 * of its contig, which the host checks before anything is launched; the text is in
 * peakseg_hip_last_error.  The device addresses stay valid until this function is called again or
 * the set is destroyed -- across a solve and across every other pack_* function; ..._download
 * copies value and moments (either may be NULL) to host arrays and returns -1 when there is
 * nothing packed (no call yet, or the last call refused). */
long long peakseg_hip_problem_set_pack_coverage_stats(psd_problem_set *set, int n_ranks,
                                                      const long long *ranks, const int **value_dev,
                                                      const unsigned long long **moments_dev);
int peakseg_hip_problem_set_packed_coverage_stats_download(psd_problem_set *set, int *value_out,
                                                           unsigned long long *moments_out);
/* the tile of those launches: runs one workgroup reads (tests aim at its boundaries) */
int peakseg_hip_coverage_stats_tile_runs(void);
/* the largest n_ranks of one call (at least 10) */
int peakseg_hip_coverage_stats_max_ranks(void);
/* milliseconds (HIP events) of the calling thread's last pack_coverage_stats: zeroing and launches */
int peakseg_hip_coverage_stats_last_ms(float *ms);
/* the digit passes the calling thread's last pack_coverage_stats launched (0: moments only) */
int peakseg_hip_coverage_stats_last_passes(int *digit_passes);

/* The coverage of caller-chosen regions of every contig of a set made from dense counts or reads,
 * computed on the device from the resident runs (what bigWigAverageOverBed does for a bigWig).
 * A region is [chromStart, chromEnd) in BED coordinates; contig c covers
 * [first_chromStart[c], first_chromStart[c] + bases).  Regions come in any order, may overlap one
 * another, and may lie partly or wholly outside their contig.  Per region:
 *   bases  int32  the bases of the region that lie inside the contig
 *   sum    int64  the sum of the per-base counts over those bases: sum of count_i x |run_i in the
 *                 region|; a run cut by an edge of the region counts with the cut length only
 *   max    int32  the largest count_i of a run that meets the region; 0 where bases == 0
 * first_chromStart: one per CONTIG, NULL = zeros (the check of pack_segments).  n_regions[c]: the
 * regions of contig c; region_start / region_end: per contig an int32 array of that many entries
 * (not read where n_regions[c] == 0); regions_on_device != 0: the arrays are device addresses
 * (multiples of 4) and are read in place, else host memory that the library uploads.  rows_out[c]
 * (n_contigs entries, host, may be NULL) receives contig c's row count, n_regions[c].  The packed
 * columns hold the contigs' regions one contig after the other, in the order given.  Integer
 * arithmetic only: the same whatever the schedule.  The set may be solved or not, and the call
 * leaves what a solve made (the segment tables, the packed columns) as it is.  Three launches,
 * however many contigs and regions there are (peaksegdisk_amd/csrc/region_stats.h).
 * Returns the total number of rows; -1 for a set that was not made from dense counts or reads;
 * -ERROR_REGION_ARGUMENTS for what that status names (host arrays are checked on the host, device
 * arrays by the first launch, after which nothing further is launched); the text is in
 * peakseg_hip_last_error.  The device addresses stay valid until this function is called again or
 * the set is destroyed -- across a solve and across every other pack_* function (the cluster
 * matrix, the joint peaks and the held-out loss fold with tables of their own); ..._download
 * copies the columns (any may be NULL) to host arrays and returns -1 when there is nothing packed
 * (no call yet, or the last call refused). */
long long peakseg_hip_problem_set_pack_region_stats(
    psd_problem_set *set, const int *first_chromStart, const long long *n_regions,
    const int *const *region_start, const int *const *region_end, int regions_on_device,
    long long *rows_out, const int **bases_dev, const long long **sum_dev, const int **max_dev);
int peakseg_hip_problem_set_packed_region_stats_download(psd_problem_set *set, int *bases_out,
                                                         long long *sum_out, int *max_out);
/* the tile of the fold: runs one workgroup folds for one region at a time, laid over the contig's
 * 16-byte aligned range as pack_segment_stats' tiles are (tests aim at its boundaries) */
int peakseg_hip_region_stats_tile_runs(void);
/* the workgroups of the fold launch of the calling thread's last pack_region_stats or
 * pack_peak_clusters (0 before the first): eight per compute unit, or the call's upper bound on its
 * (region, tile) items where that is smaller.  A workgroup takes the items blockIdx.x,
 * blockIdx.x + grid, ...: tests size their work lists from it, read-only */
long long peakseg_hip_region_stats_last_fold_grid(void);
/* milliseconds (HIP events) of the calling thread's last pack_region_stats: the launches */
int peakseg_hip_region_stats_last_ms(float *ms);

/* Which peaks of several models are the same peak, and what every model has under each of them:
 * the consensus peaks of the samples of a genomic region (PeakSegPipeline's clusterPeaks) and the
 * cluster-by-sample matrix that differential analysis starts from.  For a SOLVED set made from
 * dense counts or reads.  group[p] (n_problems entries, host) is in [-1, n_groups): -1 keeps
 * problem p out.  The members of a group are its problems in increasing problem index; a group may
 * be empty.  A member's peaks are the odd rows [ps, pe) of its segments table in genomic
 * coordinates (its contig's first_chromStart added; a model of one segment has none); members of
 * one group may have different first_chromStart and lengths, and may share a contig.
 *   clusters  two peaks overlap when ps_a < pe_b && ps_b < pe_a (abutting peaks do not); the
 *             clusters of a group are the connected components of that relation over all peaks of
 *             all its members.  Four int32 per cluster: clusterStart (the smallest ps), clusterEnd
 *             (the largest pe), peaks (the peaks joined), samples (the members with a peak in it).
 *             Packed group after group, within a group in INCREASING clusterStart -- the segments
 *             tables themselves are in decreasing order
 *   matrix    for a group of m members and k clusters k x m entries, cluster-major, the members in
 *             member order, group after group: m_peaks (int32, the member's peaks with
 *             ps < clusterEnd && clusterStart < pe) and m_bases / m_sum / m_max: the three columns
 *             of pack_region_stats with the cluster as a region of the member's contig
 * clusters_out[g], members_out[g] (n_groups entries, host, may be NULL) receive k and m of group g.
 * Integer arithmetic only: the same whatever the schedule.  The number of launches does not depend
 * on the numbers of problems, groups, members or peaks; the groups' cluster counts are downloaded
 * once in between (peaksegdisk_amd/csrc/peak_clusters.h).
 * Returns the total number of clusters; -1 for a set that is not solved or was not made from dense
 * counts; -ERROR_REGION_ARGUMENTS for n_groups < 0 or a group value outside [-1, n_groups), with
 * the problem named; -ERROR_DEVICE_MEMORY for a matrix that does not fit (PEAKSEG_HIP_MAX_BYTES or
 * the device), said before anything of it is written; the text is in peakseg_hip_last_error.  The
 * device addresses stay valid until the set is solved again, this function is called again,
 * pack_joint_peaks or pack_joint_path is called WITHOUT windows (they pack the clusters of their
 * own groups in this function's tables, as this function would), or the set is destroyed;
 * ..._download copies the columns (any may be NULL) to host arrays and returns -1 when there is
 * nothing packed: after a solve, after a refused call of this function, and after such a joint call
 * whose clusters could not be packed. */
long long peakseg_hip_problem_set_pack_peak_clusters(
    psd_problem_set *set, const int *first_chromStart, int n_groups, const int *group,
    long long *clusters_out, long long *members_out, const int **clusterStart_dev,
    const int **clusterEnd_dev, const int **peaks_dev, const int **samples_dev, const int **m_peaks_dev,
    const int **m_bases_dev, const long long **m_sum_dev, const int **m_max_dev);
int peakseg_hip_problem_set_packed_peak_clusters_download(
    psd_problem_set *set, int *clusterStart_out, int *clusterEnd_out, int *peaks_out, int *samples_out,
    int *m_peaks_out, int *m_bases_out, long long *m_sum_out, int *m_max_out);
/* milliseconds (HIP events) of the calling thread's last pack_peak_clusters: from its first launch
 * to its last, the download of the groups' cluster counts included */
int peakseg_hip_peak_clusters_last_ms(float *ms);

/* One common peak per window for all members of a group (PeakSegPipeline's PeakSegJoint step): the
 * final peak calls of a project with several samples, which samples carry each peak, and the
 * likelihood gains a differential analysis ranks by.  For a set made from dense counts or reads;
 * group[] and the members as for pack_peak_clusters; member i has the extent
 * [first_i, first_i + bases_i).
 *   windows   n_windows[g] windows per group (host), window_start[g] / window_end[g] their int32
 *             arrays (host, or with windows_on_device != 0 device addresses, read in place; one
 *             call takes one kind).  With n_windows == NULL the call first runs pack_peak_clusters
 *             on the resident tables (a SOLVED set) and window c of a group is its cluster c widened
 *             by its own width on either side: [clusterStart - w, clusterEnd + w),
 *             w = clusterEnd - clusterStart, in 64 bits.  A given window needs no solve.
 *             A window is clipped to the intersection of the extents of all members of its group:
 *             [ws, we), W = we - ws.  W < 3, or a group without members: no joint peak.
 *   sums      C_i(x, y): the sum of member i's per-base counts over [x, y), exact int64;
 *             T_i = C_i(ws, we)
 *   gain      of a candidate (s, e), ws < s < e < we: L1 = s - ws, L2 = e - s, L3 = we - e and
 *             S1, S2, S3 the member's sums over them.  The member is FEASIBLE iff S2 L1 > S1 L2 and
 *             S2 L3 > S3 L2 (exact products).  t(S, L) = 0 for S = 0, else
 *             double(S) * log(double(S) / double(L)) with the log of peakseg_detmath.h, a correctly
 *             rounded division and conversions that round to nearest;
 *             gain_i(s, e) = ((t(S1, L1) + t(S2, L2)) + t(S3, L3)) - t(T_i, W): the Poisson loss of
 *             the flat model minus that of the three-segment model
 *   G(s, e)   the sum over the feasible members, in member order, of max(0, gain_i(s, e) - penalty)
 *   search    level 0: b the smallest power of two with n = ceil(W / b) <= 64; candidates
 *             s = ws + i b, e = ws + j b, 1 <= i < j <= n - 1.  While b > 1: b' = b / 2, candidates
 *             s = s* + p b', e = e* + q b' for p, q in -4 .. 4 with ws < s < e < we around the choice
 *             (s*, e*) so far, then b = b'.  At every level the choice is the candidate with the
 *             largest G, among equals the smallest s, then the smallest e (an exact comparison: the
 *             schedule decides nothing).  A best G of 0 at level 0: no joint peak.  Otherwise the
 *             peak is the last level's choice, objective its G, levels the levels run.
 *   per window, group after group: windowStart, windowEnd (the clipped window; windowEnd =
 *             windowStart where nothing is left), peakStart, peakEnd (-1: no joint peak; then
 *             objective, samples_up, levels and the window's matrix entries are 0), samples_up,
 *             levels (int32) and objective (double)
 *   per (window, member), window-major as the cluster matrix: m_gain (double; 0 where the member is
 *             infeasible at the peak), m_up (int32; 1 iff feasible and gain > penalty; samples_up is
 *             their sum), m_sum (int64, S2), m_bases (int32, L2)
 * windows_out[g], members_out[g] (n_groups entries, host, may be NULL) receive the windows and the
 * members of group g.  All windows advance through the levels in lockstep: the number of launches
 * depends on the widest window's log2 b only (peaksegdisk_amd/csrc/joint_peaks.h); a head of 16
 * bytes is downloaded once after the first launch.
 * Returns the total number of windows; -1 for a set that was not made from dense counts, or is not
 * solved where n_windows == NULL; -ERROR_REGION_ARGUMENTS for a penalty that is negative or NaN, a
 * bad group (as pack_peak_clusters), a negative n_windows[g], a NULL or misaligned array, or a given
 * window with start >= end, with the group and the window named (host arrays are checked on the
 * host, device arrays by the first launch); -ERROR_DEVICE_MEMORY when the call's tables do not fit
 * (PEAKSEG_HIP_MAX_BYTES or the device), said before anything of them is allocated.
 * n_windows == NULL replaces what pack_peak_clusters packed: the call packs the clusters of ITS
 * groups at ITS first_chromStart in pack_peak_clusters' tables -- columns and matrix, as that
 * function would -- and packed_peak_clusters_download then gives those (or -1, when the cluster
 * step was refused); with given windows the cluster tables are not touched.  The device
 * addresses stay valid until the set is solved again (also where the windows were given), this
 * function is called again, or the set is destroyed; ..._download copies the columns (any may be
 * NULL) and returns -1 when nothing is packed. */
long long peakseg_hip_problem_set_pack_joint_peaks(
    psd_problem_set *set, const int *first_chromStart, int n_groups, const int *group, double penalty,
    const long long *n_windows, const int *const *window_start, const int *const *window_end,
    int windows_on_device, long long *windows_out, long long *members_out,
    const int **windowStart_dev, const int **windowEnd_dev, const int **peakStart_dev,
    const int **peakEnd_dev, const double **objective_dev, const int **samples_up_dev,
    const int **levels_dev, const double **m_gain_dev, const int **m_up_dev,
    const long long **m_sum_dev, const int **m_bases_dev);
int peakseg_hip_problem_set_packed_joint_peaks_download(
    psd_problem_set *set, int *windowStart_out, int *windowEnd_out, int *peakStart_out,
    int *peakEnd_out, double *objective_out, int *samples_up_out, int *levels_out, double *m_gain_out,
    int *m_up_out, long long *m_sum_out, int *m_bases_out);
/* milliseconds (HIP events) of the calling thread's last pack_joint_peaks: from its first launch to
 * its last, the download of the head included (the cluster step of n_windows == NULL is not) */
int peakseg_hip_joint_peaks_last_ms(float *ms);

/* pack_joint_peaks at n_penalties penalties in one call: model (p, w) is exactly what
 * pack_joint_peaks returns for window w at penalties[p], bit for bit, in every column; all the
 * definitions above hold unchanged per penalty (feasibility, t, gain, G added in member order, the
 * three-key choice, the levels).  What does not depend on the penalty -- the bins of level 0 and
 * their fold, the prefix sums, t(T, W), the feasibility test and the gain of every (candidate,
 * member) -- is computed once per window; from level 1 on every penalty refines its own choice, and
 * a penalty without a peak idles.
 *   penalties 1 <= n_penalties <= peakseg_hip_joint_path_max_penalties() (16) doubles >= 0 (host), in
 *             any order; repeats, 0 and +Inf (no joint peak anywhere) are allowed
 *   layout    penalty-major: the per-window columns at p * windows + w (windows: the value
 *             returned), the per-(window, member) columns at p * entries + entry (entries: the sum
 *             over the groups of windows_out[g] * members_out[g])
 * The other arguments, and the refusals, are pack_joint_peaks's; -ERROR_REGION_ARGUMENTS also for
 * n_penalties out of range and for a penalty that is negative or NaN, with its index named;
 * -ERROR_DEVICE_MEMORY, before anything is allocated, when the tables -- n_penalties times those of
 * pack_joint_peaks, 18 n_penalties (at least 64) regions per entry, and for groups of more than 64
 * members 2048 doubles per (window, penalty) -- do not fit.  The number of launches is that of one
 * pack_joint_peaks: it depends on the widest window's levels only, not on n_penalties
 * (peaksegdisk_amd/csrc/joint_path.h).
 * The call keeps buffers of its own: a later pack_joint_peaks does not touch what it packed, nor
 * does it touch what pack_joint_peaks packed.  n_windows == NULL replaces what pack_peak_clusters
 * packed by the clusters of this call's groups, exactly as pack_joint_peaks does.  The call ends
 * what pack_joint_label_errors packed, also when it is refused.  The device addresses stay valid
 * until the set is solved again (also where the windows were given), this function is called
 * again, or the set is destroyed; ..._download copies the columns (any may be NULL; n_penalties
 * times as many entries each) and returns -1 when nothing is packed. */
int peakseg_hip_joint_path_max_penalties(void);
long long peakseg_hip_problem_set_pack_joint_path(
    psd_problem_set *set, const int *first_chromStart, int n_groups, const int *group,
    int n_penalties, const double *penalties, const long long *n_windows,
    const int *const *window_start, const int *const *window_end, int windows_on_device,
    long long *windows_out, long long *members_out, const int **windowStart_dev,
    const int **windowEnd_dev, const int **peakStart_dev, const int **peakEnd_dev,
    const double **objective_dev, const int **samples_up_dev, const int **levels_dev,
    const double **m_gain_dev, const int **m_up_dev, const long long **m_sum_dev,
    const int **m_bases_dev);
int peakseg_hip_problem_set_packed_joint_path_download(
    psd_problem_set *set, int *windowStart_out, int *windowEnd_out, int *peakStart_out,
    int *peakEnd_out, double *objective_out, int *samples_up_out, int *levels_out, double *m_gain_out,
    int *m_up_out, long long *m_sum_out, int *m_bases_out);
/* milliseconds (HIP events) of the calling thread's last pack_joint_path: from its first launch to
 * its last, the download of the head included (the cluster step of n_windows == NULL is not) */
int peakseg_hip_joint_path_last_ms(float *ms);

/* The label errors of every model of the set's packed joint path (-1 without one), counted on the
 * device from its columns, in integers only: the same result whatever the schedule.
 *   labels    n_labels[q] labels per PROBLEM (host) and label_start[q] / label_end[q] /
 *             label_annotation[q], int32 arrays (host, or with labels_on_device != 0 device
 *             addresses, read in place; one call takes one kind), in genomic coordinates, the ones
 *             the joint peaks are in; annotation codes 0 noPeaks, 1 peakStart, 2 peakEnd, 3 peaks
 *   peaks     of problem q in model p: the joint peaks [peakStart, peakEnd) of the windows w of q's
 *             group with peakStart >= 0 and m_up[p, w, member of q] == 1.  Every window's peak
 *             counts, also where the peaks of two given windows overlap or coincide.  A problem in
 *             no group has no peaks in any model.
 *   counted   count, fp and fn of a label by the relations and rules of pack_label_errors
 *   per (penalty, label), penalty-major, within a penalty problem after problem in the order given:
 *             count, fp, fn (int32)
 *   per (penalty, problem): errors, fp, fn, possible_fp, possible_fn (int32, 5 per entry)
 *   per penalty: the same five as int64
 * Returns the number of labels of one penalty; -ERROR_LABEL_ARGUMENTS as pack_label_errors, with
 * the problem and the label named (host arrays are checked on the host, device arrays by the first
 * launch).  Two launches, however many penalties, problems, labels and windows
 * (peaksegdisk_amd/csrc/joint_labels.h).  The device addresses stay valid until the set is solved
 * again (the path is gone with it: the function returns -1 until the next pack_joint_path), the
 * next pack_joint_path, this function is called again, or the set is destroyed; no other pack_*
 * function touches them.  ..._download copies the columns (any may be NULL) and returns -1 when
 * nothing is packed. */
long long peakseg_hip_problem_set_pack_joint_label_errors(
    psd_problem_set *set, const long long *n_labels, const int *const *label_start,
    const int *const *label_end, const int *const *label_annotation, int labels_on_device,
    const int **count_dev, const int **fp_dev, const int **fn_dev, const int **problem_totals_dev,
    const long long **model_totals_dev);
int peakseg_hip_problem_set_packed_joint_label_errors_download(
    psd_problem_set *set, int *count_out, int *fp_out, int *fn_out, int *problem_totals_out,
    long long *model_totals_out);
/* milliseconds (HIP events) of the calling thread's last pack_joint_label_errors */
int peakseg_hip_joint_label_errors_last_ms(float *ms);

/* The Poisson loss of a solved model on ANOTHER contig of the same set: what a penalty chosen by
 * thinning is scored with (the model is fitted on some of the sampling units, the other contig holds
 * the units that were held out).  The set is one made by create_dense or create_reads and is
 * solved.  A PAIR is (problem p, contig c, scale a): contig c must have exactly as many bases as
 * p's own contig, and positions are base offsets from each contig's first base.  Rows
 * k = 0 .. S - 1 of p's segments table have [start_k, end_k) and mean_k, the doubles that
 * peakseg_hip_problem_set_pack_segments reports; B_k = end_k - start_k; Y_k is the `sum` that
 * peakseg_hip_problem_set_pack_region_stats gives for that region on contig c, an exact int64.
 * With x_k = a * mean_k the term of row k is
 *     x_k * B_k - Y_k * psd_log(x_k)   if Y_k > 0 and mean_k > 0,
 *     x_k * B_k                         if Y_k == 0 (no logarithm is taken),
 *     +Inf                              if mean_k == 0 and Y_k > 0 (counted in zero_mean_rows),
 * and loss = sum over k of term_k.  Every product and difference is rounded once (the library is
 * built with -ffp-contract=off); psd_log is the logarithm of include/peakseg_detmath.h.  The order
 * of the additions is fixed and depends on S only: with T = 256, the sum s_t of t = 0 .. T - 1 takes
 * the terms of rows t, t + T, t + 2 T, ... in that order, starting from 0; within every group of 64
 * consecutive t, for d = 32, 16, 8, 4, 2, 1 in turn, s_t += s_(t + d) for the t whose place in the
 * group is below 64 - d (all of them from the values before the step); then
 * loss = ((s_0 + s_64) + s_128) + s_192.  No floating-point atomics are used: the same pairs give
 * the same bytes on every run.  Per pair the call gives loss (double), rows (int32, S), bases
 * (int64, the sum of B_k), sum (int64, the sum of Y_k) and zero_mean_rows (int32).  A problem whose
 * solve reported a failure has no rows, as in pack_segments: its loss is 0 and its rows are 0.
 *
 * problem / contig (int32) and scale (double): n_pairs entries each, in host memory or
 * (pairs_on_device != 0) in the set's device memory, where they are read in place; pairs may
 * repeat and come in any order.  The *_dev outputs (any may be NULL) receive the device addresses
 * of the five columns, one entry per pair in the order given; they are valid until the set is
 * solved again (the columns score the models of the solve before: nothing in the library reads
 * them across a solve, and the download refuses), the next pack_heldout_loss, or destroy.  The call
 * leaves the segment tables and every other packed buffer as they are.  The number of launches does
 * not depend on the pairs or the rows.
 * Returns n_pairs; -1 for a set that was not made from dense counts or reads or is not solved, and
 * for a device failure; -ERROR_HELDOUT_ARGUMENTS for a negative n_pairs, a NULL or misaligned
 * array, an index out of range, a scale that is not finite and positive, or a contig whose bases
 * differ: peakseg_hip_last_error() names the pair.  Host arrays are checked on the host before
 * anything is allocated or launched; device arrays are checked by the first launch, after which
 * nothing further is launched.  -ERROR_DEVICE_MEMORY when the call's buffers do not fit in free HBM
 * or PEAKSEG_HIP_MAX_BYTES: asked before anything is allocated (device arrays: the rows' buffers
 * are asked about once the first launch has counted the rows, before any of them is allocated). */
long long peakseg_hip_problem_set_pack_heldout_loss(
    psd_problem_set *set, long long n_pairs, const int *problem, const int *contig,
    const double *scale, int pairs_on_device, const double **loss_dev, const int **rows_dev,
    const long long **bases_dev, const long long **sum_dev, const int **zero_mean_rows_dev);
/* the five columns of the last pack_heldout_loss to host arrays of n_pairs entries (any may be
 * NULL); 0, or -1 when nothing is packed -- no call yet, the last call refused, or the set solved
 * again since -- or a copy fails */
int peakseg_hip_problem_set_packed_heldout_loss_download(psd_problem_set *set, double *loss_out,
                                                         int *rows_out, long long *bases_out,
                                                         long long *sum_out, int *zero_mean_rows_out);
/* milliseconds (HIP events) of the calling thread's last pack_heldout_loss: its launches */
int peakseg_hip_heldout_loss_last_ms(float *ms);

/* Fold sets: the sampling units of every input contig split at random into `folds` = K folds on the
 * device (thinning), and the set of all train and test contigs.  K is 2, 4 or 8 and
 * bits = log2 K; any other value is ERROR_HELDOUT_ARGUMENTS.  The random words are splitmix64,
 *     splitmix64(s, i):  z = s + (i + 1) * 0x9E3779B97F4A7C15;
 *                        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                        z = (z ^ (z >> 27)) * 0x94D049BB133111EB;   z ^ (z >> 31)
 * in 64-bit arithmetic that wraps (peaksegdisk_amd/synthetic.py has the same function): with
 * s_i = seed ^ ((i + 1) * 0xD1B54A32D192ED03) for input contig i, h = splitmix64(s_i, index) and
 * word_j = splitmix64(h, j).
 *   dense units  index is the base's offset in its contig.  Unit u < n of a base with the count n
 *                takes field u mod per_word of word_(u div per_word), where per_word = 64 div bits
 *                fields of `bits` bits are counted from the low end of a word; the field's value is
 *                the unit's fold.  (K = 2: the base's count in fold 1 is a popcount.)  The K counts
 *                t_f of a base sum to n.  A count above peakseg_hip_fold_max_count() = 2^20 is
 *                refused with ERROR_HELDOUT_ARGUMENTS, the contig and the base in the text: a
 *                choice, which bounds the words a base takes at 2^20 / 21.
 *   reads        index is the read's place in the caller's arrays.  The read's fold is the top
 *                `bits` bits of word_0; its optional count goes whole to that fold.
 * The set's layout is the same for both: input contig i and fold f give contig (i K + f) 2 (train:
 * every unit that is not in fold f) and (i K + f) 2 + 1 (test: the units in fold f), both with the
 * input's bases (reads: its extent); problem (i K + f) P + j is the train contig of (i, f) at
 * penalties[j], j < P = n_penalties; test contigs carry no problem.  From here on the set is one
 * of create_dense / create_reads.  The other arguments and statuses are those of the parents; host
 * arrays are checked on the host, where the input's contig is named (device arrays: a read that
 * cannot be piled up is named by the pile-up with the fold contig it met it in). */
int peakseg_hip_problem_set_create_dense_folds(int device, int n_contigs,
                                               const long long *contig_n_bases,
                                               const int *const *contig_counts, int counts_on_device,
                                               int n_penalties, const double *penalties,
                                               unsigned long long arena_pieces, int folds,
                                               unsigned long long seed, psd_problem_set **out);
int peakseg_hip_problem_set_create_reads_folds(
    int device, int n_contigs, const long long *n_reads, const int *const *read_start,
    const int *const *read_end, const int *const *read_count, int reads_on_device,
    const int *extent_start, const int *extent_end, int bases_counted, int n_penalties,
    const double *penalties, unsigned long long arena_pieces, int folds, unsigned long long seed,
    psd_problem_set **out);
/* the largest count of a base that create_dense_folds splits: 2^20 */
int peakseg_hip_fold_max_count(void);
/* milliseconds (HIP events) of the calling thread's last fold kernel (dense or reads) */
int peakseg_hip_fold_units_last_ms(float *ms);

/* The fits of a penalty-learning regression (the model that penalty_model= takes): interval
 * regression with the squared hinge of margin 1, an L1 penalty on the weights and an unpenalised
 * intercept, for every regularization of a path and every fold of a cross-validation, in one launch
 * of one workgroup per problem.  The call is not tied to a problem set.
 *   rows      n (2 to 2^20 - 1), each with p (0 to peakseg_hip_penalty_fit_max_features())
 *             standardised features, x_std[j * n + i] for feature j of row i (feature-major), and the
 *             target [lo[i], hi[i]] in log(penalty); lo = -inf or hi = +inf is allowed, not both
 *   folds     fold[i] in [0, n_folds), n_folds = F from 1 to 16.  Problem (f, k), f < F, trains on the
 *             rows whose fold is not f with reg[k] and is validated on the rows of fold f; problem
 *             (F, k) trains on all rows and is validated on them.  F = 1: no validation -- the
 *             all-rows problem alone runs (every fold[i] is 0) and n_reg must be 1
 *   reg       n_reg (1 to 256) increasing regularizations, none negative
 *   objective (1/|S|) sum over the training rows S of phi(f_i - lo_i) + phi(hi_i - f_i)
 *             + reg |w|_1, with f_i = b + w . x_i and phi(z) = (z - 1)^2 for z < 1, else 0
 *   solver    accelerated proximal gradient from w = 0, b = 0 with the constant step
 *             |S| / (4 gram_lambda_max) and a restart of the momentum; gram_lambda_max bounds the
 *             largest eigenvalue of [X 1]'[X 1] over all rows from above (the caller computes it)
 *   stopping  c = max(|dF/db|, max_j c_j) <= threshold, with c_j = |g_j + reg sign(w_j)| where
 *             w_j != 0 and max(0, |g_j| - reg) where w_j = 0, g the gradient of the smooth part at the
 *             weights returned; evaluated every 8 iterations and after max_iterations
 * The outputs (any may be NULL) have one entry per problem, problem (f, k) at f * n_reg + k, in all
 * (F + 1) * n_reg of them -- n_reg when F = 1: weights_out p + 1 doubles each, the intercept last, in
 * standardised units; iterations_out; criterion_out, the c of the weights returned; converged_out, 1
 * or 0 (max_iterations reached with c above threshold); incorrect_out, the validation rows whose
 * prediction lies outside their interval; hinge_out, the sum of phi(f_i - lo_i) + phi(hi_i - f_i)
 * over the validation rows.  Every floating-point sum has an order fixed by (n, p): two calls with
 * the same arguments return the same bits.
 * Returns 0; ERROR_FIT_ARGUMENTS with the argument and the row in peakseg_hip_last_error, checked on
 * the host before anything is launched; then ERROR_NO_HIP_DEVICE.  Everything the call allocates on
 * the device is freed before it returns. */
int peakseg_hip_penalty_fit(int device, int n, int p, const double *x_std, const double *lo,
                            const double *hi, const int *fold, int n_folds, int n_reg,
                            const double *reg, double gram_lambda_max, double threshold,
                            int max_iterations, double *weights_out, int *iterations_out,
                            double *criterion_out, int *converged_out, long long *incorrect_out,
                            double *hinge_out);
/* milliseconds (HIP events) of the calling thread's last penalty_fit: zeroing and the launch, the
 * upload excluded */
int peakseg_hip_penalty_fit_last_ms(float *ms);
/* the largest p of one call */
int peakseg_hip_penalty_fit_max_features(void);

/* Where a round of the parallel penalty search looks besides its secant penalty: up to `extras`
 * penalties between over_penalty (the bracket's smaller penalty, 0 allowed) and under_penalty (its
 * larger one, +Inf allowed) into out[extras]; returns how many.  The caller keeps what survives
 * the 15-digit string strictly inside the bracket. */
int peakseg_hip_search_place_penalties(double under_penalty, double over_penalty, double secant,
                                       int extras, double *out);

/* The ten fields of the reference's loss.tsv row of one solved problem, in its order and with its
 * arithmetic: penalty, segments, peaks, bases, bedGraph.lines, mean.pen.cost, total.loss,
 * equality.constraints, mean.intervals, max.intervals.  0 or -1. */
int peakseg_hip_problem_set_loss(psd_problem_set *set, int problem, double *out);

/* Shader cycles a problem's workgroup ran in the last launch that worked on it (0 when
 * unknown); with the device's clock, data points / cycles is the problem's rate: the dealing of
 * problems to ranks is sized from it. */
long long peakseg_hip_problem_set_cycles(psd_problem_set *set, int problem);
/* Data points per second one problem advanced at in this process's last clean solves on the
 * latency build (a CU per problem) and on the throughput build (a full chip). */
void peakseg_hip_measured_rates(double *lat_rate, double *thr_rate);

/* Tests: the bound on the number of polls of a wait between the waves of a workgroup, and (in
 * builds with -DPSD_SPIN_STATS, 0 otherwise) the largest poll count a problem's waves saw. */
long long peakseg_hip_spin_limit(void);
int peakseg_hip_problem_set_max_spin(psd_problem_set *set, int problem);
/* Tests: in builds with -DPSD_LOOP_STATS, for each chain wave (up, then down) the data points of
 * the problem's last launch that the latency kernel took inside its inner loop of the usual data
 * point, those its general code took, and the entries into the inner loop: out[6], returns 6.
 * Every other build counts nothing and returns 0. */
int peakseg_hip_problem_set_loop_stats(psd_problem_set *set, int problem, int *out);

/* Change one problem's penalty in place (the contig stays resident, the arena is reused by the
 * next solve): what the penalty search does between its dynamic programs.  0 or -1. */
int peakseg_hip_problem_set_set_penalty(psd_problem_set *set, int problem, double penalty);

void peakseg_hip_problem_set_destroy(psd_problem_set *set);

/* Tests: parse a bedGraph file the way PeakSegFPOP_disk does (use_fast != 0: byte scanner with
 * sscanf fallback; 0: the reference's sscanf format on every line) and return the status, the
 * number of data lines and a hash of everything parsed. */
int peakseg_hip_parse_probe(const char *path, int use_fast, int *n_lines,
                            unsigned long long *hash);

/* Tests: the dense encoder alone.  Arguments as peakseg_hip_problem_set_create_dense; per contig
 * runs_out / min_out / max_out / sum_out, and the concatenated count / weight / run_end arrays
 * (any may be NULL).  Statuses as the creator's, without the penalties. */
int peakseg_hip_dense_encode_probe(int device, int n_contigs, const long long *n_bases,
                                   const int *const *counts, int counts_on_device,
                                   long long *runs_out, int *count_out, int *weight_out,
                                   int *run_end_out, int *min_out, int *max_out,
                                   long long *sum_out);
/* the encoder's tile: bases one workgroup encodes (tests aim at its boundaries) */
int peakseg_hip_dense_tile_bases(void);
/* milliseconds (HIP events) of the three launches of the calling thread's last encoding */
int peakseg_hip_dense_last_encode_ms(float *count_ms, float *scan_ms, float *scatter_ms);

/* Tests and coverage_from_reads: the pile-up alone, and the encoding of it when any of runs_out /
 * count_out / weight_out / run_end_out is given.  The read arguments as
 * peakseg_hip_problem_set_create_reads; coverage_out (host, the sum of the extents' bases, or NULL)
 * receives the contigs' coverage one after the other, the other four what
 * peakseg_hip_dense_encode_probe gives.  Statuses as the creator's, without the penalties. */
int peakseg_hip_reads_pileup_probe(int device, int n_contigs, const long long *n_reads,
                                   const int *const *read_start, const int *const *read_end,
                                   const int *const *read_count, int reads_on_device,
                                   const int *extent_start, const int *extent_end, int bases_counted,
                                   int *coverage_out, long long *runs_out, int *count_out,
                                   int *weight_out, int *run_end_out);
/* milliseconds (HIP events) of the calling thread's last pile-up: zeroing and scatter_kernel; the
 * three launches of the prefix sum */
int peakseg_hip_reads_last_pileup_ms(float *scatter_ms, float *scan_ms);

/* Stranded single-end reads: the strand cross-correlation of the reads' 5'
 * ends in exact integers, and the extension of reads to a fragment length.  Neither call is tied to
 * a problem set.
 *   input    per contig the int32 arrays chromStart, chromEnd and the optional count as
 *            peakseg_hip_problem_set_create_reads takes them, an int8 array strand with +1 or -1 per
 *            read, and the extent [lo, hi), B = hi - lo
 *   tags     the 5' base of a plus read is chromStart, of a minus read chromEnd - 1.  p[i] is the sum
 *            of the counts of the plus reads whose 5' base is lo + i, m[i] the same for minus reads,
 *            0 <= i < B.  A read whose 5' base lies outside the extent is no tag; its count still
 *            goes into the contig's sum of counts, which must stay below 2^31 -- then
 *            sum p x sum m < 2^62 and every sum below fits 64 bits
 *   table    for s = 0 .. S = max_shift one row of six int64:
 *              pairs                max(B - s, 0)
 *              sum_plus, sq_plus    sum of p[i], of p[i]^2 over i < B - s
 *              sum_minus, sq_minus  sum of m[i], of m[i]^2 over i >= s
 *              cross                sum of p[i] m[i + s] over i < B - s
 *            Integer adds commute: the table does not depend on the schedule, and a repeated call
 *            gives the same bytes.  S is at most peakseg_hip_xcorr_max_shift() = 1023
 *   correlation  (formed by the caller from the exact integers; peaksegdisk_amd does it in Python
 *            integers)  num = pairs cross - sum_plus sum_minus, vx = pairs sq_plus - sum_plus^2,
 *            vy = pairs sq_minus - sum_minus^2, r = num / (sqrt(vx) sqrt(vy)), NaN where vx <= 0 or
 *            vy <= 0.  The pooled table of several contigs is the column-wise sum of their tables
 *            (pooled sums may pass 2^63: not in int64)
 *   estimate among the shifts of [min_shift, max_shift] with a finite r the largest r, among equal r
 *            the smallest shift, compared exactly: the sign of num first, then num_a^2 vx_b vy_b
 *            against num_b^2 vx_a vy_a.  fragment_length = shift + 1: a fragment [f, f + d) has its
 *            plus tag at f and its minus tag at f + d - 1
 *   extension  to the length d >= 1: a plus read becomes [chromStart, chromStart + d), a minus read
 *            [chromEnd - d, chromEnd), formed in 64 bits and clamped into int32.  Nothing is clipped
 *            to an extent: the pile-up does that afterwards, as for any read
 * strand_xcorr: table_out is host memory, n_contigs x (max_shift + 1) x 6 int64, contig-major.
 * extend: fragment_length has one entry per contig; out_start / out_end are on the side of the
 * inputs (host arrays for host reads, device arrays for device reads; they may be the inputs
 * themselves); after a refusal their contents are undefined.
 * Checks, in this order: n_contigs <= 0: ERROR_NO_DATA; what the host sees of the reads --
 * n_reads < 0, a NULL chromStart / chromEnd with n_reads > 0, an int32 device address that is no
 * multiple of 4 (a strand array may begin at any byte): ERROR_READS_ARGUMENTS, a NULL strand array
 * with n_reads > 0: ERROR_STRAND_ARGUMENTS; max_shift or fragment_length out of range, hi <= lo:
 * ERROR_STRAND_ARGUMENTS; lo < 0: ERROR_READS_ARGUMENTS; the device: ERROR_NO_HIP_DEVICE; whether
 * the call's buffers fit in free HBM and PEAKSEG_HIP_MAX_BYTES, asked before anything is allocated:
 * ERROR_DEVICE_MEMORY; then what the first launch finds -- the first read of a contig with
 * chromStart >= chromEnd or a negative count: ERROR_READS_ARGUMENTS, with a strand that is neither
 * +1 nor -1: ERROR_STRAND_ARGUMENTS, a contig whose counts sum to 2^31 or more:
 * ERROR_READS_ARGUMENTS -- with the contig and the read in peakseg_hip_last_error(), and nothing
 * further is launched. */
int peakseg_hip_reads_strand_xcorr(int device, int n_contigs, const long long *n_reads,
                                   const int *const *read_start, const int *const *read_end,
                                   const int *const *read_count,
                                   const signed char *const *read_strand, int reads_on_device,
                                   const int *extent_start, const int *extent_end, int max_shift,
                                   long long *table_out);
int peakseg_hip_reads_extend(int device, int n_contigs, const long long *n_reads,
                             const int *const *read_start, const int *const *read_end,
                             const signed char *const *read_strand, int reads_on_device,
                             const int *fragment_length, int *const *out_start, int *const *out_end);
/* the largest max_shift of one call: 1023 (1024 shifts, four per thread of a workgroup of 256) */
int peakseg_hip_xcorr_max_shift(void);
/* milliseconds (HIP events) of the calling thread's last strand_xcorr: zeroing and tags_kernel;
 * xcorr_kernel and edges_kernel */
int peakseg_hip_reads_last_xcorr_ms(float *tags_ms, float *xcorr_ms);

/* Duplicate removal of aligned reads: the first `keep` units of every key
 * survive, in input order, in exact integers.  Neither call is tied to a problem set.
 *   input    per contig the reads i = 0 .. n - 1 in input order: int32 chromStart[i] < chromEnd[i]
 *            (negative coordinates are legal, as in the pile-up), an optional int32 count[i] >= 0
 *            (absent: every read counts 1) and an optional int8 strand[i] of +1 or -1.  c(i) is the
 *            count of read i: a row is a multiplicity
 *   key      by = 0 (fragment): (chromStart, chromEnd, strand), the strand +1 for every read when no
 *            strand array is given -- paired-end fragments, reads used as they are.  by = 1
 *            (five_prime): (5' base, strand), the 5' base chromStart of a plus read and chromEnd - 1
 *            of a minus read; a strand array is required -- the rule for single-end reads.  Keys are
 *            compared within a contig only
 *   marking  with keep in 1 .. 2^31 - 1:
 *              before(i)    = sum of c(j) over j < i with key(j) = key(i)
 *              out_count(i) = min(c(i), max(keep - before(i), 0))
 *            The result depends on grouping and input order only, never on how keys are ordered
 *            among themselves
 *   summary  per contig four int64: reads = sum of c(i), kept = sum of out_count(i), rows_kept =
 *            #{i: out_count(i) > 0}, distinct = #{i: c(i) > 0 and before(i) = 0}, the keys with at
 *            least one unit.  Everything is integer; a repeated call gives the same bytes
 * dedup: out_count[c] (n_reads[c] int32) is on the side of the inputs -- host arrays for host reads,
 * device arrays for device reads -- and must not overlap any input; summary_out is host memory,
 * 4 x n_contigs.  read_strand may be NULL for by = 0.
 * compact: writes the rows with keep_count > 0 of every contig, in order, to out_start / out_end /
 * out_count (the value of keep_count) and, with read_strand given, out_strand -- room for n_reads[c]
 * rows each, on the side of the inputs, overlapping no input -- and the rows written per contig to
 * rows_out (host).  Usable on its own, for instance to drop rows of count 0.
 * Checks, in this order: n_contigs <= 0: ERROR_NO_DATA; n_reads NULL or negative:
 * ERROR_READS_ARGUMENTS; 2^31 or more rows in the call, an unknown by, keep < 1, five_prime without
 * strands: ERROR_DEDUP_ARGUMENTS; a NULL array of a contig with reads or an int32 device address that
 * is no multiple of 4 (a strand array may begin at any byte): ERROR_READS_ARGUMENTS, a NULL strand
 * array next to given ones: ERROR_STRAND_ARGUMENTS; an output that overlaps an input:
 * ERROR_DEDUP_ARGUMENTS; the device: ERROR_NO_HIP_DEVICE; whether the call's buffers fit in free HBM
 * and PEAKSEG_HIP_MAX_BYTES, asked before anything is allocated: ERROR_DEVICE_MEMORY; then what the
 * first launch finds -- the first read of a contig with chromStart >= chromEnd or a negative count:
 * ERROR_READS_ARGUMENTS, with a strand that is neither +1 nor -1: ERROR_STRAND_ARGUMENTS, a contig
 * whose counts sum to 2^31 or more (the pile-up's rule; what makes before(i) fit int32):
 * ERROR_READS_ARGUMENTS -- with the contig and the read in peakseg_hip_last_error(), and nothing
 * further is launched.  A refused call has written nothing to its outputs. */
int peakseg_hip_reads_dedup(int device, int n_contigs, const long long *n_reads,
                            const int *const *read_start, const int *const *read_end,
                            const int *const *read_count, const signed char *const *read_strand,
                            int reads_on_device, int by, int keep, int *const *out_count,
                            long long *summary_out);
int peakseg_hip_reads_compact(int device, int n_contigs, const long long *n_reads,
                              const int *const *read_start, const int *const *read_end,
                              const signed char *const *read_strand, int reads_on_device,
                              const int *const *keep_count, int *const *out_start,
                              int *const *out_end, int *const *out_count,
                              signed char *const *out_strand, long long *rows_out);
/* rows of a workgroup of a sort pass, and the workgroups one trip of the table scan covers: what the
 * tests build their sizes on */
int peakseg_hip_dedup_block_rows(void);
int peakseg_hip_dedup_scan_span(void);
/* milliseconds (HIP events) of the calling thread's last dedup: zeroing and keys_kernel; the sort's
 * passes; the three launches of the runs -- and the number of passes the keys' mask chose */
int peakseg_hip_reads_last_dedup_ms(float *keys_ms, float *sort_ms, float *runs_ms);
int peakseg_hip_reads_last_dedup_passes(void);

/* Tests: the cluster kernels alone, on caller-given peaks of the members of ONE group, without any
 * solve.  n_peaks[m]: the peaks of member m; peak_start[m] / peak_end[m]: host int32 arrays, sorted
 * and disjoint (peak_end[i] <= peak_start[i + 1]), coordinates in [0, 2^31).  clusterStart_out /
 * clusterEnd_out / peaks_out / samples_out (room for one entry per peak: there are no more clusters
 * than peaks) receive the cluster table in increasing clusterStart, m_peaks_out (clusters x
 * n_members entries, cluster-major; room for peaks x n_members) the matrix' peaks column; any may
 * be NULL.  Returns the clusters; -ERROR_REGION_ARGUMENTS for lists that are not as said (the member
 * and the peak are in peakseg_hip_last_error), -ERROR_NO_HIP_DEVICE, or -1. */
long long peakseg_hip_peak_clusters_probe(int device, int n_members, const long long *n_peaks,
                                          const int *const *peak_start, const int *const *peak_end,
                                          int *clusterStart_out, int *clusterEnd_out, int *peaks_out,
                                          int *samples_out, int *m_peaks_out);

/* Tests: R's paste() of a double (15 significant digits) as the penalty search and the timing
 * files format numbers; returns the length. */
int peakseg_hip_paste_double(double x, char *buf, size_t buf_len);

/* diagnostic builds (-DPSD_PROFILE): per-wave cycle counters of the forward kernel; -1 in
 * normal builds */
int peakseg_hip_problem_set_profile(psd_problem_set *set, int problem, long long *out);

/* y[i] = exp(x[i]) (op 0) or log(x[i]) (op 1) evaluated on the device with the library's
 * deterministic math (include/peakseg_detmath.h); op 2: y[i] = psd_div(x[i], x[n + i]) (x holds
 * n numerators, then n divisors), op 3: the same quotients by the compiler's own fp64 division
 * sequence, which psd_div repairs; tests compare with the host build. */
int peakseg_hip_math_probe(int op, int n, const double *x, double *y);

/* Tests: one form of include/peakseg_detmath_core.h on the device, element by element, with one set
 * of constants.  form: 0 psd_exp, 1 psd_log, 2 psd_exp2, 3 psd_log2, 4 psd_exp2_log, 5 psd_exp_nb,
 * 6 psd_log_nb, 7 psd_log_wild_nb; set: 0 the plain constants (throughput and packed builds), 1 the
 * constants in vector registers (latency build).  x0, x1, z: n arguments each (x1 for the forms of
 * two exp / two log, z the log's argument of psd_exp2_log; NULL where the form reads none: zeros);
 * y0, y1, lz: n results each (zeros where the form has none), rare: the record of the _nb forms,
 * 0 before every element's call (0 for the other forms); any output may be NULL.  Returns 0,
 * ERROR_NO_HIP_DEVICE, or -1 for a form, a set or an n out of range, before anything is launched. */
int peakseg_hip_math_forms_probe(int form, int set, int n, const double *x0, const double *x1,
                                 const double *z, double *y0, double *y1, double *lz, int *rare);

#ifdef __cplusplus
}
#endif
#endif
