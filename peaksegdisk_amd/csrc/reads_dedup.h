/* reads_dedup.h -- duplicate removal of aligned reads on the device, in exact integers: the first
 * `keep` units of every key survive, in input order (the contract is in include/peaksegdisk_hip.h;
 * DESIGN.md section 20).
 *
 * A read's key is (contig, strand, a, b): (chromStart, chromEnd) for a, b by fragment, (5' base, 0)
 * by 5' end.  The rows of all contigs of a call are numbered g = 0 .. N - 1 in input order.  Every
 * launch is a whole pass over its data, and no workgroup ever waits for another:
 *   keys_kernel      the shape of reads::scatter_kernel: a workgroup per slice of SLICE reads of one
 *                    contig, a read per lane.  A bad read goes to the contig's 16-byte record as in
 *                    strand_xcorr.h (~index with the reason in the low bits, a 64-bit max), the sum
 *                    of the good counts by a 64-bit add.  A row's four key words (signed ones biased
 *                    to unsigned), its number g and its count go to flat arrays, and the OR over
 *                    rows of key XOR the call's first key to four mask words: the bits in which the
 *                    keys differ at all.
 *   the sort         a stable LSD radix sort of (key, g) by digits of 8 bits, over those of the 16
 *                    digits only in which the mask says the keys differ, and moving those of the
 *                    four key words only that differ.  A pass is three launches:
 *     hist_kernel    a workgroup per BLOCK_ROWS rows: its counts of the 256 digit values (LDS adds)
 *                    to the digit-major table [digit][workgroup], and to the 256 totals of the pass
 *                    by one add each -- both sums of ones, the same whatever the schedule.
 *     scan_kernel    a wave per digit value: the totals of the smaller values, then the exclusive
 *                    scan of its row of the table in trips of SCAN_SPAN workgroups, by shuffles.
 *     scatter_kernel a workgroup per BLOCK_ROWS rows again; wave w owns the rows 256 w .. 256 w + 255
 *                    of the block in four rounds of 64.  The peers of a lane -- the lanes of its
 *                    round with its digit -- come from eight ballots; its rank is the count of the
 *                    wave's earlier rounds (LDS, written by the wave's lowest peer alone) plus the
 *                    population count of the peers below it.  Wave bases are taken in wave order
 *                    through LDS, on top of the table's entry.  No atomic decides a position.
 *   the runs         in sorted order a row is a head when its key differs from its predecessor's, and
 *                    before(i) is the segmented exclusive prefix sum of the counts.  Stable sort:
 *                    sorted order is input order within a key.
 *     runs_kernel    a workgroup per RUN_ROWS sorted rows: the sum of its trailing run and whether
 *                    it holds a head.
 *     carry_kernel   one workgroup: the segmented scan of those aggregates.
 *     apply_kernel   the local scan again plus the carry: out_count = min(c, max(keep - before, 0))
 *                    to out_count[row] of the row's contig; kept, rows_kept and distinct to the
 *                    contig's summary by 64-bit adds (a wave whose rows are of one contig adds
 *                    once, to one of the summary's copies).  `reads` is the record's sum.
 *   compaction       flag_kernel (rows with keep_count > 0 per slice), slice_scan_kernel (a
 *                    workgroup per contig: exclusive scan of its slices' totals, and the contig's
 *                    rows), compact_kernel (rank by ballot, wave bases through LDS): stable.
 * Counts of a contig sum to less than 2^31 (refused otherwise), so before(i) and every trailing sum
 * fit 32 bits; prefix sums inside a workgroup are formed in unsigned arithmetic, which wraps, and
 * only differences of them are used.
 *
 * Algorithmic traffic for N rows, m moving key words (1 to 4), P passes and W = N / BLOCK_ROWS:
 * keys 8 N read (12 N with counts, + N with strands), 24 N written; per pass 4 N read by hist_kernel,
 * 1 KB x W of table written, read and rewritten by scan_kernel and read by scatter_kernel, and
 * 4 (m + 2) N read and 4 (m + 1) N written by scatter_kernel, the writes scattered in runs of a
 * digit; runs 2 x (20 N sorted rows + 4 N counts gathered by row number), 4 N written through the
 * row number, 3 atomics per wave; compaction 4 N + 4 N flags, 13 N read and 13 x kept rows written.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_READS_DEDUP_H
#define PSD_READS_DEDUP_H

#include "psd_platform.h"
#include "strand_xcorr.h"

namespace psd {
namespace dedup {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int SLICE = THREADS;               /* reads of a slice of keys_kernel and of the compaction */
constexpr int ROUNDS = 4;                    /* rows of a lane in a sort pass */
constexpr int WAVE_ROWS = WAVE * ROUNDS;     /* consecutive rows a wave owns */
constexpr int BLOCK_ROWS = THREADS * ROUNDS; /* rows of a workgroup of a sort pass */
constexpr int RUN_ROWS = THREADS;            /* sorted rows of a workgroup of the runs */
constexpr int SCAN_SPAN = WAVE;              /* workgroups of a trip of scan_kernel */
constexpr int DIGIT_BITS = 8, DIGITS = 1 << DIGIT_BITS;
constexpr int KEY_WORDS = 4; /* in rising significance: b, a, strand, contig */
constexpr int WORD_B = 0, WORD_A = 1, WORD_STRAND = 2, WORD_CONTIG = 3;
constexpr int MAX_PASSES = KEY_WORDS * 32 / DIGIT_BITS;
constexpr int BY_FRAGMENT = 0, BY_FIVE_PRIME = 1;
constexpr int SUMMARY = 4; /* reads, kept, rows_kept, distinct */
/* A contig's summary exists `copies` times on the device, each copy in a 128-byte line of its own,
 * and a workgroup of apply_kernel adds to the copy of its index modulo that: one line for all waves
 * of a long contig makes their atomics queue behind each other (measured: DESIGN.md section 20).  The
 * host adds the copies up. */
constexpr int SUMMARY_STRIDE = 16, SUMMARY_COPIES = 64;
constexpr int REASON_BITS = psd::xcorr::REASON_BITS;
constexpr int BAD_ORDER = psd::xcorr::BAD_ORDER, BAD_COUNT = psd::xcorr::BAD_COUNT,
              BAD_STRAND = psd::xcorr::BAD_STRAND;

static_assert(DIGITS == THREADS && DIGITS % WAVES == 0 && BLOCK_ROWS % RUN_ROWS == 0,
              "a thread per digit value, a wave per digit value");

#ifdef __clang__
#define PSD_DEDUP_UNROLL _Pragma("unroll")
#else
#define PSD_DEDUP_UNROLL _Pragma("GCC unroll 4")
#endif

typedef psd::reads::u64 u64;
typedef psd::reads::Check Check;

struct Contig {
  const int *start, *end, *count; /* the reads; count == nullptr: every read counts 1 */
  const signed char *strand;      /* +1 or -1 per read, at any byte; nullptr: every read is plus */
  int *out;                       /* out_count of the contig's rows */
  long long n_reads;
  long long slice_first; /* index of the contig's first slice */
  long long row_first;   /* number of its first row in the call */
};

struct Rows { /* one side of the sort's ping-pong: N entries each */
  unsigned *key[KEY_WORDS];
  unsigned *row;
};

struct CompactContig {
  const int *start, *end, *keep;
  const signed char *strand; /* nullptr: no strands */
  int *out_start, *out_end, *out_count;
  signed char *out_strand;
  long long n_reads, slice_first;
};

PSD_D unsigned biased(int v) { return (unsigned)v ^ 0x80000000u; }

PSD_D void make_key(int by, int s, int e, int d, int ci, unsigned (&k)[KEY_WORDS]) {
  const int five = d > 0 ? s : e - 1;
  k[WORD_B] = by == BY_FRAGMENT ? biased(e) : 0u;
  k[WORD_A] = biased(by == BY_FRAGMENT ? s : five);
  k[WORD_STRAND] = d > 0 ? 1u : 0u;
  k[WORD_CONTIG] = (unsigned)ci;
}

/* the inclusive prefix sum of x over the lanes of the wave; reached by all lanes */
PSD_D unsigned wave_scan(unsigned x) {
  const int lane = lane_id();
  for (int off = 1; off < WAVE; off <<= 1) {
    const unsigned o = (unsigned)shfl_i((int)x, lane >= off ? lane - off : lane);
    if (lane >= off) x += o;
  }
  return x;
}

PSD_D unsigned wave_sum(unsigned x) {
  const int lane = lane_id();
  for (int off = 32; off > 0; off >>= 1) x += (unsigned)shfl_i((int)x, lane ^ off);
  return x;
}

__global__ __launch_bounds__(THREADS) void keys_kernel(const Contig *contigs, const int *slice_contig,
                                                       int by, int first_contig, Rows rows, int *cnt,
                                                       Check *checks, unsigned *mask) {
  const long long slice = (long long)blockIdx.x;
  const int ci = slice_contig[slice];
  const Contig c = contigs[ci];
  const int lane = lane_id();
  const long long i = (slice - c.slice_first) * SLICE + (long long)threadIdx.x;
  u64 good = 0, bad = 0;
  unsigned diff[KEY_WORDS] = {0u, 0u, 0u, 0u};
  if (i < c.n_reads) {
    const int s = c.start[i], e = c.end[i];
    const int k = c.count ? c.count[i] : 1;
    const int d = c.strand ? (int)c.strand[i] : 1;
    const int why = s >= e ? BAD_ORDER : (k < 0 ? BAD_COUNT : (d != 1 && d != -1 ? BAD_STRAND : 0));
    if (why) {
      bad = psd::xcorr::check_key(i, why);
    } else {
      good = (u64)k;
      /* the call's first key: row 0 of its first contig that has a row */
      const Contig f = contigs[first_contig];
      unsigned first[KEY_WORDS], mine[KEY_WORDS];
      make_key(by, f.start[0], f.end[0], f.strand ? (int)f.strand[0] : 1, first_contig, first);
      make_key(by, s, e, d, ci, mine);
      const long long g = c.row_first + i;
      PSD_DEDUP_UNROLL
      for (int w = 0; w < KEY_WORDS; w++) {
        rows.key[w][g] = mine[w];
        diff[w] = mine[w] ^ first[w];
      }
      rows.row[g] = (unsigned)g;
      cnt[g] = k;
    }
  }
  PSD_DEDUP_UNROLL
  for (int w = 0; w < KEY_WORDS; w++) {
    for (int off = 32; off > 0; off >>= 1) diff[w] |= (unsigned)shfl_i((int)diff[w], lane ^ off);
    /* (a look first: almost every wave finds its bits set already, and a million ORs to one word
     * queue behind each other; a stale look costs an OR that changes nothing) */
    if (lane == 0 && (diff[w] & ~agent_load_u32(mask + w))) atomic_or_u32(mask + w, diff[w]);
  }
  PSD_LDS u64 w_good[WAVES], w_bad[WAVES];
  psd::xcorr::send_check(good, bad, w_good, w_bad, checks + ci);
}

__global__ __launch_bounds__(THREADS) void hist_kernel(const unsigned *word, int shift, long long n,
                                                       int n_blocks, unsigned *table, int *digit_total) {
  PSD_LDS unsigned hist[DIGITS];
  const int tid = (int)threadIdx.x;
  hist[tid] = 0u;
  __syncthreads();
  const long long base = (long long)blockIdx.x * BLOCK_ROWS + wave_id() * WAVE_ROWS + lane_id();
  for (int r = 0; r < ROUNDS; r++) {
    const long long g = base + r * WAVE;
    if (g < n) lds_add_u32(&hist[(word[g] >> shift) & (DIGITS - 1)], 1u);
  }
  __syncthreads();
  const unsigned h = hist[tid];
  table[(long long)tid * n_blocks + (long long)blockIdx.x] = h;
  if (h) atomic_add_i32(digit_total + tid, (int)h);
}

/* a wave per digit value, four to a workgroup: nothing goes through LDS and nobody waits */
__global__ __launch_bounds__(THREADS) void scan_kernel(unsigned *table, const int *digit_total,
                                                       int n_blocks) {
  const int lane = lane_id();
  const int digit = (int)blockIdx.x * WAVES + wave_id();
  if (digit_total[digit] == 0) return; /* no row has this value: nobody reads its (zero) entries */
  unsigned below = 0u;
  for (int d = lane; d < digit; d += WAVE) below += (unsigned)digit_total[d];
  unsigned running = wave_sum(below); /* the rows in front of the trip's first workgroup, sorted */
  unsigned *row = table + (long long)digit * n_blocks;
  for (int first = 0; first < n_blocks; first += SCAN_SPAN) {
    const int j = first + lane;
    const unsigned x = j < n_blocks ? row[j] : 0u;
    const unsigned incl = wave_scan(x);
    if (j < n_blocks) row[j] = running + incl - x;
    running += (unsigned)shfl_i((int)incl, WAVE - 1);
  }
}

/* `digit_word` is src.key[] of the pass's digit; the words of `move` (bit w: key word w) and the row
 * numbers go to dst */
__global__ __launch_bounds__(THREADS) void scatter_kernel(Rows src, Rows dst, int move,
                                                          const unsigned *digit_word, int shift,
                                                          long long n, int n_blocks,
                                                          const unsigned *table) {
  PSD_LDS unsigned w_count[WAVES][DIGITS];
  PSD_LDS unsigned w_base[WAVES][DIGITS];
  const int tid = (int)threadIdx.x, lane = lane_id(), wave = wave_id();
  for (int w = 0; w < WAVES; w++) w_count[w][tid] = 0u;
  __syncthreads();
  const long long base = (long long)blockIdx.x * BLOCK_ROWS + wave * WAVE_ROWS + lane;
  unsigned digit[ROUNDS], rank[ROUNDS];
  PSD_DEDUP_UNROLL
  for (int r = 0; r < ROUNDS; r++) {
    const long long g = base + r * WAVE;
    const bool valid = g < n;
    const unsigned d = valid ? (digit_word[g] >> shift) & (DIGITS - 1) : 0u;
    unsigned long long peers = ballot(valid);
    for (int bit = 0; bit < DIGIT_BITS; bit++) {
      const bool set = (d >> bit) & 1u;
      const unsigned long long with = ballot(valid && set);
      peers &= set ? with : ~with;
    }
    const unsigned before = (unsigned)popc64(peers & lanes_below(lane));
    const unsigned prior = valid ? w_count[wave][d] : 0u;
    wave_sync();
    if (valid && before == 0u) w_count[wave][d] = prior + (unsigned)popc64(peers);
    wave_sync();
    digit[r] = d;
    rank[r] = prior + before;
  }
  __syncthreads();
  unsigned at = table[(long long)tid * n_blocks + (long long)blockIdx.x];
  for (int w = 0; w < WAVES; w++) {
    w_base[w][tid] = at;
    at += w_count[w][tid];
  }
  __syncthreads();
  PSD_DEDUP_UNROLL
  for (int r = 0; r < ROUNDS; r++) {
    const long long g = base + r * WAVE;
    if (g >= n) continue;
    const long long to = (long long)(w_base[wave][digit[r]] + rank[r]);
    if (to >= n) continue; /* (never, with the table as scan_kernel leaves it) */
    PSD_DEDUP_UNROLL
    for (int w = 0; w < KEY_WORDS; w++)
      if ((move >> w) & 1) dst.key[w][to] = src.key[w][g];
    dst.row[to] = src.row[g];
  }
}

/* What the runs know of a sorted row inside its workgroup.  Reached by all threads. */
struct Run {
  unsigned before; /* the counts of the run's earlier rows in this workgroup */
  bool open;       /* the run began in an earlier workgroup: the carry is to be added */
  unsigned trail;  /* the workgroup's aggregate: the sum of its trailing run ... */
  bool any_head;   /* ... and whether a run begins in it */
  unsigned row, contig;
  int count;
  bool valid;
};

PSD_D Run local_run(const Rows &sorted, const int *cnt, long long n, unsigned *l_trail, int *l_head) {
  const int lane = lane_id(), wave = wave_id();
  const long long idx = (long long)blockIdx.x * RUN_ROWS + (long long)threadIdx.x;
  Run r;
  r.valid = idx < n;
  bool head = false;
  r.contig = 0u;
  PSD_DEDUP_UNROLL
  for (int w = 0; w < KEY_WORDS; w++) {
    const unsigned mine = r.valid ? sorted.key[w][idx] : 0u;
    if (r.valid && idx > 0 && mine != sorted.key[w][idx - 1]) head = true;
    if (w == WORD_CONTIG) r.contig = mine;
  }
  if (r.valid && idx == 0) head = true;
  r.row = r.valid ? sorted.row[idx] : 0u;
  r.count = r.valid ? cnt[r.row] : 0;
  const unsigned x = (unsigned)r.count;
  const unsigned incl = wave_scan(x), excl = incl - x;
  const unsigned long long heads = ballot(head);
  const unsigned long long mine = heads & (lanes_below(lane) | (1ull << lane));
  const unsigned from = (unsigned)shfl_i((int)excl, mine ? msb64(mine) : 0);
  r.before = mine ? excl - from : excl;
  r.open = mine == 0ull;
  const unsigned total = (unsigned)shfl_i((int)incl, WAVE - 1);
  const unsigned last = (unsigned)shfl_i((int)excl, heads ? msb64(heads) : 0);
  if (lane == 0) {
    l_trail[wave] = heads ? total - last : total;
    l_head[wave] = heads != 0ull;
  }
  __syncthreads();
  unsigned carry = 0u;
  bool seen = false;
  r.trail = 0u;
  r.any_head = false;
  for (int w = 0; w < WAVES; w++) {
    if (w == wave) {
      if (r.open) {
        r.before += carry;
        r.open = !seen;
      }
    }
    carry = l_head[w] ? l_trail[w] : carry + l_trail[w];
    seen = seen || l_head[w];
  }
  r.trail = carry;
  r.any_head = seen;
  return r;
}

__global__ __launch_bounds__(THREADS) void runs_kernel(Rows sorted, const int *cnt, long long n,
                                                       unsigned *agg_trail, int *agg_head) {
  PSD_LDS unsigned l_trail[WAVES];
  PSD_LDS int l_head[WAVES];
  const Run r = local_run(sorted, cnt, n, l_trail, l_head);
  if (threadIdx.x == 0) {
    agg_trail[blockIdx.x] = r.trail;
    agg_head[blockIdx.x] = r.any_head;
  }
}

/* One workgroup: carry[b] = the counts of the run that is open where workgroup b of the runs begins
 * (thread k takes the k-th share of the aggregates; the shape of reads::tile_scan_kernel). */
__global__ __launch_bounds__(THREADS) void carry_kernel(const unsigned *agg_trail, const int *agg_head,
                                                        long long n_blocks, unsigned *carry) {
  PSD_LDS unsigned s_sum[THREADS];
  PSD_LDS int s_head[THREADS];
  const int tid = (int)threadIdx.x;
  const long long share = (n_blocks + THREADS - 1) / THREADS;
  const long long a = tid * share < n_blocks ? tid * share : n_blocks;
  const long long b = a + share < n_blocks ? a + share : n_blocks;
  unsigned sum = 0u;
  int any = 0;
  for (long long t = a; t < b; t++) {
    sum = agg_head[t] ? agg_trail[t] : sum + agg_trail[t];
    any |= agg_head[t];
  }
  s_sum[tid] = sum;
  s_head[tid] = any;
  __syncthreads();
  unsigned open = 0u;
  for (int k = 0; k < tid; k++) open = s_head[k] ? s_sum[k] : open + s_sum[k];
  for (long long t = a; t < b; t++) {
    carry[t] = open;
    open = agg_head[t] ? agg_trail[t] : open + agg_trail[t];
  }
}

__global__ __launch_bounds__(THREADS) void apply_kernel(Rows sorted, const int *cnt, long long n,
                                                        const unsigned *carry, const Contig *contigs,
                                                        int keep, long long *summary, int copies,
                                                        int n_contigs) {
  PSD_LDS unsigned l_trail[WAVES];
  PSD_LDS int l_head[WAVES];
  const Run r = local_run(sorted, cnt, n, l_trail, l_head);
  const int lane = lane_id();
  const unsigned before = r.before + (r.open ? carry[blockIdx.x] : 0u); /* below 2^31 */
  const int room = keep - (int)before;
  const int out = r.count < room ? r.count : (room > 0 ? room : 0);
  unsigned kept = 0u, rows_kept = 0u, distinct = 0u;
  if (r.valid) {
    contigs[r.contig].out[(long long)r.row - contigs[r.contig].row_first] = out;
    kept = (unsigned)out;
    rows_kept = out > 0;
    distinct = r.count > 0 && before == 0u;
  }
  /* (the valid lanes of a wave are its first ones) */
  const unsigned first = (unsigned)shfl_i((int)r.contig, 0);
  const unsigned long long valid = ballot(r.valid), other = ballot(r.valid && r.contig != first);
  if (valid == 0ull) return;
  if (other == 0ull) {
    kept = wave_sum(kept);
    rows_kept = wave_sum(rows_kept);
    distinct = wave_sum(distinct);
    if (lane != 0) return;
  }
  long long *mine = summary + ((long long)((int)blockIdx.x % copies) * n_contigs + (long long)r.contig) *
                                  SUMMARY_STRIDE;
  if (r.valid && kept) atomic_add_i64(mine + 1, (long long)kept);
  if (r.valid && rows_kept) atomic_add_i64(mine + 2, (long long)rows_kept);
  if (r.valid && distinct) atomic_add_i64(mine + 3, (long long)distinct);
}

/* ---- compaction ---------------------------------------------------------------------------- */

__global__ __launch_bounds__(THREADS) void flag_kernel(const CompactContig *contigs,
                                                       const int *slice_contig, unsigned *slice_total) {
  PSD_LDS unsigned w_tot[WAVES];
  const long long slice = (long long)blockIdx.x;
  const CompactContig c = contigs[slice_contig[slice]];
  const long long i = (slice - c.slice_first) * SLICE + (long long)threadIdx.x;
  const unsigned long long flags = ballot(i < c.n_reads && c.keep[i] > 0);
  if (lane_id() == 0) w_tot[wave_id()] = (unsigned)popc64(flags);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned total = 0u;
    for (int w = 0; w < WAVES; w++) total += w_tot[w];
    slice_total[slice] = total;
  }
}

/* a workgroup per contig: the rows in front of each of its slices, and its rows */
__global__ __launch_bounds__(THREADS) void slice_scan_kernel(const CompactContig *contigs,
                                                             const unsigned *slice_total,
                                                             unsigned *slice_carry, long long *rows) {
  PSD_LDS unsigned s_sum[THREADS];
  const CompactContig c = contigs[blockIdx.x];
  const int tid = (int)threadIdx.x;
  const long long n_slices = (c.n_reads + SLICE - 1) / SLICE;
  const long long share = (n_slices + THREADS - 1) / THREADS;
  const long long a = tid * share < n_slices ? tid * share : n_slices;
  const long long b = a + share < n_slices ? a + share : n_slices;
  unsigned sum = 0u;
  for (long long t = a; t < b; t++) sum += slice_total[c.slice_first + t];
  s_sum[tid] = sum;
  __syncthreads();
  unsigned before = 0u;
  for (int k = 0; k < tid; k++) before += s_sum[k];
  for (long long t = a; t < b; t++) {
    slice_carry[c.slice_first + t] = before;
    before += slice_total[c.slice_first + t];
  }
  if (tid == THREADS - 1) rows[blockIdx.x] = (long long)before;
}

__global__ __launch_bounds__(THREADS) void compact_kernel(const CompactContig *contigs,
                                                          const int *slice_contig,
                                                          const unsigned *slice_carry) {
  PSD_LDS unsigned w_tot[WAVES];
  const long long slice = (long long)blockIdx.x;
  const CompactContig c = contigs[slice_contig[slice]];
  const int lane = lane_id(), wave = wave_id();
  const long long i = (slice - c.slice_first) * SLICE + (long long)threadIdx.x;
  const int k = i < c.n_reads ? c.keep[i] : 0;
  const unsigned long long flags = ballot(k > 0);
  if (lane == 0) w_tot[wave] = (unsigned)popc64(flags);
  __syncthreads();
  if (k <= 0) return;
  unsigned to = slice_carry[slice] + (unsigned)popc64(flags & lanes_below(lane));
  for (int w = 0; w < wave; w++) to += w_tot[w];
  c.out_start[to] = c.start[i];
  c.out_end[to] = c.end[i];
  c.out_count[to] = k;
  if (c.strand) c.out_strand[to] = c.strand[i];
}

}  // namespace dedup
}  // namespace psd
#endif
