/*
 * agx.h -- C-ABI of libagx.so: the MI355X (gfx950) drop-in for the two
 * anti-diagonal DP hot paths of AnteMarusic/Accelerating-Genomics:
 *
 *   - Smith-Waterman affine-gap score-only fill
 *       replaces the per-pair loop body of smithWaterman/antidiagonalSmithWaterman.c:254-348
 *       (and the kernel launch of smithWaterman/hipvers.cpp:470-483)
 *   - PairHMM forward recurrence
 *       replaces pairHMM() of pairHMM/antidiagsPairHMM.c:120-267 (fp64 semantics of
 *       pairHMM/pairHMMmatrix.c:41-66) as called from the batch loop :411-461
 *
 * The reference exposes no library API: its surface is two command lines and
 * one function seam.  This header is what a C host binds
 * instead; the drop-in command lines in accelerating-genomics_amd/host/ are
 * built on exactly these entry points.  Plain C99, plain pointers and sizes,
 * caller-owned buffers, int status (0 = AGX_OK, < 0 = error, text via
 * agx_last_error()).  A context and everything created from it belong to one
 * host thread at a time; distinct contexts may be used from distinct threads.
 *
 * There is no CPU fallback: every compute entry point fails with
 * AGX_E_NODEVICE when no HIP device is usable.
 */
#ifndef AGX_H
#define AGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_OK 0
#define AGX_E_ARG (-1)      /* bad argument (NULL pointer, negative count, inconsistent offsets) */
#define AGX_E_NODEVICE (-2) /* no usable HIP device / ordinal out of range */
#define AGX_E_HIP (-3)      /* a HIP runtime call failed; agx_last_error() has the HIP text */
#define AGX_E_NOMEM (-4)    /* host or device allocation failed */
#define AGX_E_SYMBOL (-5)   /* a sequence contains byte 0x00, reserved as the padding symbol */
#define AGX_E_LIMIT (-6)    /* a length exceeds what the kernels support (see AGX_*_MAX_*) */
#define AGX_E_IO (-7)       /* parser: file cannot be opened / is malformed */
#define AGX_E_INTERNAL (-8) /* a result failed the library's own cross-check (agx_sw_batch_hits); agx_last_error() says which */

/* Smith-Waterman: the shorter sequence of a pair is laid across lanes, at most
 * 64 lanes x AGX_SW_MAX_COLS_PER_LANE columns; the longer one streams.  (The
 * reference CLI cannot produce lines of 1000 bytes or more,
 * antidiagonalSmithWaterman.c:44; hipvers.cpp:40 allows 10000.)  Batches whose
 * shorter sides all fit 64 x 40 = 2560 columns run the packed kernel; a batch
 * with a longer one runs the int32 kernel with its wide classes. */
#define AGX_SW_MAX_COLS_PER_LANE 160
#define AGX_SW_MAX_SHORT_LEN (64 * AGX_SW_MAX_COLS_PER_LANE)
/* PairHMM: haplotype across lanes, read streams.  Up to 64 lanes x AGX_PHMM_MAX_COLS_PER_LANE
 * columns a pair is filled in one pass; longer haplotypes (the reference's line buffer allows
 * 5000, antidiagsPairHMM.c:8,353) are filled in stripes of 1536 columns by one wavefront. */
#define AGX_PHMM_MAX_COLS_PER_LANE 32
#define AGX_PHMM_MAX_HAP_LEN 16384
#define AGX_PHMM_MAX_READ_LEN 4096

/* ------------------------------------------------------------------ runtime */

typedef struct agx_ctx agx_ctx; /* one device + one HIP stream + reusable workspaces */

const char *agx_version(void);
const char *agx_last_error(void); /* thread-local, never NULL */
int agx_device_count(void);       /* >= 0; 0 when HIP reports no device */
/* Marketing name of a device, as hipvers.cpp:388-391 prints it; empty string on failure. */
int agx_device_name(int device, char *buf, size_t buf_len);

int agx_ctx_create(int device, agx_ctx **out);
/* Batches keep their context alive: a context may be destroyed before the batches created from it
 * (its streams and memory pools go with the last of them). */
void agx_ctx_destroy(agx_ctx *ctx);
int agx_ctx_device(const agx_ctx *ctx);
/* The hipStream_t all launches of this context go to (as void*).  A host that
 * already owns a stream (e.g. PyTorch's current stream) may install it. */
void *agx_ctx_stream(const agx_ctx *ctx);
int agx_ctx_set_stream(agx_ctx *ctx, void *hip_stream);
int agx_ctx_sync(agx_ctx *ctx);
/* Options.  The library reads no environment variable; whatever a host wants changed it sets here. */
#define AGX_OPT_SW_KERNEL 1 /* which Smith-Waterman fill runs; all give identical scores */
#define AGX_SW_KERNEL_AUTO 0          /* packed int16 x 2 when the batch's value range allows, else int32 */
#define AGX_SW_KERNEL_INT32 1         /* one pair per lane group, int32 state (BASELINE config 2 as worded) */
#define AGX_SW_KERNEL_PACKED_SIGNED 2 /* two pairs per lane group, signed int16 halves */
#define AGX_SW_KERNEL_PACKED_BIASED 3 /* two pairs per lane group, biased unsigned halves (the default where it fits) */
#define AGX_OPT_SW_PLANNER 2 /* where the Smith-Waterman planner's per-pair passes run; same records, same scores */
#define AGX_SW_PLANNER_AUTO 0   /* on the device for large mixed batches of the packed biased fill, else on the host */
#define AGX_SW_PLANNER_HOST 1   /* always on the host (threaded) */
#define AGX_SW_PLANNER_DEVICE 2 /* on the device whenever the batch-level rules allow it, whatever the batch size */
#define AGX_OPT_PHMM_TRAINS 3 /* read trains in the packed float PairHMM fill (AGX_PHMM_F32_FMA); same results bit for bit */
#define AGX_PHMM_TRAINS_AUTO 0 /* two reads of a region share their lane groups where the batch is large enough for it to pay */
#define AGX_PHMM_TRAINS_OFF 1  /* every read drains before the next enters (the schedule of rounds 1 and 2) */
#define AGX_PHMM_TRAINS_ON 2   /* wherever two reads can share a group, whatever the batch size */
#define AGX_OPT_SW_TRACE_BYTES 4 /* agx_sw_batch_cigars: device memory one chunk of traced pairs may take, direction words and operation
                                  * slots together; default 1 GiB, a value below 1 is AGX_E_ARG ("Alignment itself" below) */
int agx_ctx_set_option(agx_ctx *ctx, int key, int64_t value);
/* Brings the HIP runtime and the process-wide contexts of these devices up (the ones agx_*_devices / agx_*_multi /
 * agx_pairHMM use) without computing anything: about 0.2 s that a host can spend on another thread while it
 * parses its input (both drop-in command lines do).  devices == NULL: devices 0 .. n_devices-1, n_devices <= 0: all. */
int agx_warmup_devices(const int *devices, int n_devices);
/* Page-locked host memory.  Batches built from buffers allocated here are uploaded by DMA straight from
 * the caller's memory (about twice the rate of pageable memory, and asynchronously).  Optional: every
 * entry point accepts ordinary malloc'ed buffers. */
void *agx_host_alloc(size_t bytes); /* NULL on failure */
void agx_host_free(void *p);
/* HIP-event stopwatch on the context's stream (used by bench.py for the roofline figures). */
int agx_ctx_timer_start(agx_ctx *ctx);
int agx_ctx_timer_stop(agx_ctx *ctx, float *elapsed_ms); /* second event + wait + elapsed */
/* The same stopwatch in two halves, for timing a launch inside a longer host-timed step without an extra
 * wait: mark() records the second event and returns at once; elapsed() (after whatever synchronised the
 * stream, e.g. agx_sw_batch_scores) reads the time between the two events. */
int agx_ctx_timer_mark(agx_ctx *ctx);
int agx_ctx_timer_elapsed(agx_ctx *ctx, float *elapsed_ms);

/* ----------------------------------------------------------- Smith-Waterman */

/*
 * Input layout (host memory): sequence k is bases[off[k] .. off[k]+len[k]);
 * pair p aligns sequences 2p and 2p+1 -- the file order of
 * antidiagonalSmithWaterman.c:216-227.  Sequences are raw symbols: the caller
 * decides whether a trailing '\n' belongs to them (the reference CLI keeps it,
 * antidiagonalSmithWaterman.c:229-247; agx_sw_text does the same).  Scoring is
 * the reference's compile-time constants (:40-43): match +1, mismatch -1,
 * gap open -3, gap extend -1.  scores[p] = max over the matrix, >= 0, int32,
 * bit-exact with the reference.
 */
typedef struct agx_sw_batch agx_sw_batch; /* a scheduled batch resident in HBM */

typedef struct agx_sw_info {
    int64_t n_pairs;
    int64_t cells;        /* sum len_a*len_b over pairs, as given (sentinels included) */
    int64_t padded_cells; /* lane-steps x columns actually issued (>= cells) */
    int64_t input_bytes;  /* bytes of the packed device image the kernels read */
    int32_t n_launches;   /* kernel launches per agx_sw_batch_launch() */
    int32_t n_waves;      /* wavefronts over all launches */
    int32_t planned_on_device; /* 1 = the per-pair passes of the planner ran as kernels (AGX_OPT_SW_PLANNER) */
    int32_t reserved;
} agx_sw_info;

/* Scoring of the fill (8f n3: the reference's GPU variants carry these as kernel arguments but
 * ignore them, hipvers.cpp:214).  Values are ADDED to the score, as in the reference's macros
 * (antidiagonalSmithWaterman.c:40-43): the first cell of a gap costs gap_open + gap_extend, every
 * further one gap_extend.  Limits: 1 <= match <= 12, match - 128 <= mismatch <= 0,
 * -1000 <= gap_open, gap_extend <= 0 (scores then fit the kernel's int16 lanes: 12 * 2560 < 32767). */
typedef struct agx_sw_scoring {
    int32_t match, mismatch, gap_open, gap_extend;
} agx_sw_scoring;
/* The reference's compile-time constants: +1, -1, -3, -1. */
#define AGX_SW_SCORING_REFERENCE {1, -1, -3, -1}

/* Validate, pick the lane tiling per pair, pack and copy to the device.  Blocking.
 * ctx may be NULL: the batch is then only planned on the host (no device needed); it answers
 * agx_sw_batch_info() and every other call on it fails with AGX_E_NODEVICE. */
int agx_sw_batch_create(agx_ctx *ctx, const uint8_t *bases, const uint64_t *off, const uint32_t *len,
                        int64_t n_pairs, agx_sw_batch **out);
/* Same with caller-chosen scoring (NULL = the reference's).  Only the reference scoring is pinned
 * against the reference program; other settings are checked against the oracle's parametrised Gotoh. */
int agx_sw_batch_create_scored(agx_ctx *ctx, const agx_sw_scoring *scoring, const uint8_t *bases, const uint64_t *off,
                               const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* Substitution matrix (the reference has no such mode -- its kernel's scoring
 * arguments are ignored, hipvers.cpp:214 -- so results are checked against the oracle's Gotoh with the
 * same matrix: "parity unpinned").  code[] maps an input byte to a symbol number 0..n_symbols-1, or
 * 0xff for bytes outside the alphabet (such input fails with AGX_E_SYMBOL); score[a][b] is added on
 * the diagonal move and must be symmetric (the shorter sequence of a pair is laid across the lanes
 * whichever came first).  Gaps as in agx_sw_scoring.  Shorter side <= 2560 in this mode. */
#define AGX_SW_MATRIX_MAX_SYMBOLS 32
typedef struct agx_sw_matrix {
    int32_t n_symbols; /* 1..32 */
    int32_t gap_open, gap_extend; /* -1000..0 each */
    uint8_t code[256];
    int8_t score[AGX_SW_MATRIX_MAX_SYMBOLS][AGX_SW_MATRIX_MAX_SYMBOLS];
} agx_sw_matrix;
int agx_sw_batch_create_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, const uint8_t *bases, const uint64_t *off,
                               const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* Enqueue the fill on the context's stream; scores stay in HBM.  Asynchronous. */
int agx_sw_batch_launch(agx_sw_batch *b);
/* Wait for the batch's last launch -- and for everything the library queued on the context's stream behind it -- and copy the
 * scores out in the caller's pair order.  After agx_sw_batch_bind_scores has changed where the scores go (an array bound,
 * unbound or replaced by another), the call fails with AGX_E_ARG until the batch has been launched again: the last launch wrote
 * to the place named before, so neither the caller's array nor the batch's own holds what this call would promise. */
int agx_sw_batch_scores(agx_sw_batch *b, int32_t *scores);
/* Optional: name the page-locked array (agx_host_alloc, n_pairs ints) the scores are wanted in BEFORE launching.  A batch
 * whose records are in file order (a uniform batch: fixed-length reads) then lets every launch write its scores there
 * itself -- one PCIe write per wavefront, no copy kernel behind the fill -- and agx_sw_batch_scores(b, the same pointer)
 * only waits.  Other batches keep the copy; scores == NULL unbinds.  The array must stay valid while it is bound.
 * Bind, then launch, then fetch: a change of the binding after a launch leaves that launch's scores where they were, and
 * agx_sw_batch_scores refuses (AGX_E_ARG) until the next launch.  Binding the array that is bound already changes nothing. */
int agx_sw_batch_bind_scores(agx_sw_batch *b, int32_t *scores);
int agx_sw_batch_info(const agx_sw_batch *b, agx_sw_info *info);
void agx_sw_batch_destroy(agx_sw_batch *b);

/*
 * Alignment coordinates: where the best local alignment ends and begins (no traceback: the span is what bounds one).
 * For pair p, a = sequence 2p (the query), b = sequence 2p+1 (the target), raw bytes as given, a trailing '\n'
 * included if the caller passed one.  H[i][j] is the local-alignment matrix with i a 0-based position in b and j a
 * 0-based position in a.  All positions are inclusive and in the caller's coordinates.
 *   score            = max over H, what agx_sw_batch_scores returns
 *   (b_end, a_end)   = among the cells with H == score the one with the smallest b_end, among those the smallest a_end
 *   (b_begin, a_begin) = among the alignments of that score ending in the end cell the one that begins latest in b,
 *                      among those latest in a; equally: the end cell, by the rule above, of a[a_end..0] against
 *                      b[b_end..0] (both prefixes reversed), mapped back
 *   score == 0 (no matching symbol, or an empty sequence): all four positions are -1.
 * An align batch lays a across the lanes whichever sequence is shorter, so its limits are on the roles, not on
 * "shorter/longer": len(a) <= AGX_SW_ALIGN_MAX_QUERY_LEN (64 lanes x 40 columns), len(b) <= AGX_SW_ALIGN_MAX_TARGET_LEN;
 * a longer sequence fails the create with AGX_E_LIMIT.  scoring == NULL: the reference's constants.
 */
typedef struct agx_sw_hit {
    int32_t score, a_begin, a_end, b_begin, b_end;
} agx_sw_hit;
#define AGX_SW_ALIGN_ENDS 1  /* score + end cell; begins are -1 */
#define AGX_SW_ALIGN_SPANS 2 /* score + end cell + begin cell (a second fill over the reversed prefixes) */
#define AGX_SW_ALIGN_MAX_QUERY_LEN 2560
#define AGX_SW_ALIGN_MAX_TARGET_LEN 65535
/* Resident batch like agx_sw_batch_create_scored; agx_sw_batch_launch (re)launches its fill, agx_sw_batch_scores returns
 * its scores, agx_sw_batch_bind_scores is accepted and ignored.  A SPANS batch keeps a host copy of the sequences.
 * ctx may be NULL: plan only. */
int agx_sw_batch_create_align(agx_ctx *ctx, const agx_sw_scoring *scoring, int what, const uint8_t *bases, const uint64_t *off,
                              const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* Waits for the launched fill and writes one hit per pair in the caller's pair order.  A SPANS batch runs its begin pass
 * here and checks that the reverse fill reproduces every forward score (AGX_E_INTERNAL otherwise: no span is returned that
 * the library cannot vouch for).  AGX_E_ARG on a batch that was not created by agx_sw_batch_create_align. */
int agx_sw_batch_hits(agx_sw_batch *b, agx_sw_hit *hits);
/* One-shot: create_align + launch + hits + destroy. */
int agx_sw_align(agx_ctx *ctx, const agx_sw_scoring *scoring, int what, const uint8_t *bases, const uint64_t *off,
                 const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits);

/*
 * Alignment modes: the same fill with other boundaries -- global, fit and extension alignment, score and coordinates,
 * still without a traceback.  a = sequence 2p (query), la = len(a); b = sequence 2p+1 (target), lb = len(b); the first
 * cell of a gap costs gap_open + gap_extend, every further cell gap_extend.
 * D[i][j], 0 <= i <= lb, 0 <= j <= la, is the best score of an alignment of a[0..j) with b[s..i); it may end in any
 * state (match, gap in a, gap in b).  D[0][0] = 0; D[0][j] = gap_open + j gap_extend for j > 0; the left column D[i][0],
 * i > 0, is gap_open + i gap_extend when the start is pinned (s = 0) and 0 when the target start is free (any s <= i).
 * There is NO zero floor: scores may be negative.
 * Results are the caller's 0-based inclusive coordinates, a_end = j - 1, b_end = i - 1; -1 = nothing of that sequence
 * consumed; an empty range is begin 0, end -1.
 *   mode                  start              score                             end cell
 *   AGX_SW_MODE_LOCAL     --                 exactly agx_sw_batch_create_align's
 *   AGX_SW_MODE_GLOBAL    pinned             D[lb][la]                         (lb-1, la-1)
 *   AGX_SW_MODE_FIT       target start free  max_i D[i][la], i = 0..lb         a_end = la-1, b_end = smallest such i, minus 1
 *   AGX_SW_MODE_EXTEND    pinned             max_{i,j} D[i][j] incl. D[0][0],  smallest i, then smallest j among the maxima;
 *                                            so >= 0                           score 0: a_end = b_end = -1
 *   AGX_SW_MODE_EXTEND_QUERY pinned          max_i D[i][la]                    a_end = la-1, b_end = smallest such i, minus 1
 * AGX_SW_ALIGN_ENDS leaves the begins at -1.  AGX_SW_ALIGN_SPANS fills them: GLOBAL, EXTEND, EXTEND_QUERY begin at
 * a_begin = b_begin = 0 (EXTEND with score 0 keeps -1 for all four, as in the local rule; no second fill).  FIT:
 * a_begin = 0 and b_begin = the LATEST start s among the alignments of that score that consume b through b_end (0 when
 * b_end = -1), found by a second fill -- reversed a against reversed b[0..b_end] in mode EXTEND_QUERY, whose score must
 * equal the forward one (AGX_E_INTERNAL naming the pair otherwise).
 * Pairs with an empty side have their answers from the formulas above (GLOBAL with la = 0: gap_open + lb gap_extend).
 * Limits are those of align batches; agx_sw_batch_scores returns the mode's score.  A mode outside 0..4: AGX_E_ARG.
 */
#define AGX_SW_MODE_LOCAL 0
#define AGX_SW_MODE_GLOBAL 1
#define AGX_SW_MODE_FIT 2
#define AGX_SW_MODE_EXTEND 3
#define AGX_SW_MODE_EXTEND_QUERY 4
/* agx_sw_batch_create_align / agx_sw_align with a mode (those two mean AGX_SW_MODE_LOCAL).  ctx may be NULL: plan only. */
int agx_sw_batch_create_align_mode(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, const uint8_t *bases,
                                   const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
int agx_sw_align_mode(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, const uint8_t *bases, const uint64_t *off,
                      const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits);

/* Align batches under a substitution matrix (agx_sw_matrix, validated as by agx_sw_batch_create_matrix; NULL: AGX_E_ARG).
 * The contract is that of "Alignment coordinates" and "Alignment modes" above in every mode, with the diagonal move adding
 * score[code[a_j]][code[b_i]] in place of match / mismatch; a byte outside the alphabet fails with AGX_E_SYMBOL naming the pair.
 * A diagonal score may be <= 0 even for identical symbols, so: a LOCAL or EXTEND score of 0 means "nothing consumed" (all four
 * positions -1), whatever the sequences hold; GLOBAL, FIT and EXTEND_QUERY scores may be negative.  The batch behaves as
 * agx_sw_batch_create_align_mode's does (launch, scores, hits, bind_scores ignored, limits; ctx may be NULL: plan only). */
int agx_sw_batch_create_align_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int what, const uint8_t *bases,
                                     const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_matrix + launch + hits + destroy. */
int agx_sw_align_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int what, const uint8_t *bases, const uint64_t *off,
                        const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits);

/*
 * Alignment statistics: matches and aligned pairs of the reported alignment, still without a traceback.
 * For a pair, let score, a_begin..a_end, b_begin..b_end be exactly what an AGX_SW_ALIGN_SPANS batch of the same mode and
 * scoring reports.  Among the alignments that attain `score` and consume exactly a[a_begin..a_end] and b[b_begin..b_end],
 * take the one with the most matches, among those the one with the most pairs:
 *   pairs   = its diagonal moves (an a symbol aligned with a b symbol)
 *   matches = the pairs of identical input bytes; under a matrix, of identical symbol codes, whatever that entry scores
 * Nothing consumed gives {0, 0}: a LOCAL or EXTEND score of 0, an empty side (GLOBAL included), b_end = -1.
 * Everything else is the caller's arithmetic.  With ca = a_end - a_begin + 1 and cb = b_end - b_begin + 1:
 *   alignment columns = ca + cb - pairs   (so "most pairs" is "fewest columns")
 *   mismatches        = pairs - matches
 *   gap cells         = ca + cb - 2 pairs
 *   identity          = matches / columns
 * The number of gap OPENS is not reported (it is not determined under a matrix or with gap_open = 0).
 * The query limit of a stats batch is AGX_SW_STATS_MAX_QUERY_LEN (the widest lane classes are not built with statistics);
 * a longer query fails the create with AGX_E_LIMIT.  The target limit stays AGX_SW_ALIGN_MAX_TARGET_LEN.
 */
typedef struct agx_sw_stat {
    int32_t matches, pairs;
} agx_sw_stat;
#define AGX_SW_STATS_MAX_QUERY_LEN 1792 /* 64 lanes x 28 columns */
/* A stats batch is an AGX_SW_ALIGN_SPANS batch of `mode` that can also answer agx_sw_batch_stats.  Exactly one way of scoring:
 * matrix != NULL (then scoring must be NULL: AGX_E_ARG otherwise), else scoring, else the reference's constants.
 * agx_sw_batch_launch (re)launches, agx_sw_batch_scores returns the mode's score, agx_sw_batch_hits what a SPANS batch returns,
 * agx_sw_batch_bind_scores is accepted and ignored.  ctx may be NULL: plan only. */
int agx_sw_batch_create_align_stats(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, const uint8_t *bases,
                                    const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* Waits for the launched fill and writes one stat (and, hits != NULL, one hit) per pair in the caller's pair order.  Every stat
 * is checked before it is returned -- 0 <= matches <= pairs <= min(ca, cb), and under match/mismatch scoring the score minus
 * matches, mismatches and gap cells must be a whole number of gap opens between "1 if there is a gap cell" and "one per gap
 * cell" -- AGX_E_INTERNAL naming the pair otherwise: no stat is returned that the library cannot vouch for.
 * AGX_E_ARG on a batch that was not created by agx_sw_batch_create_align_stats. */
int agx_sw_batch_stats(agx_sw_batch *b, agx_sw_hit *hits /* may be NULL */, agx_sw_stat *stats);
/* One-shot: create_align_stats + launch + stats + destroy. */
int agx_sw_align_stats(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, const uint8_t *bases,
                       const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits /* may be NULL */, agx_sw_stat *stats);

/*
 * Alignment itself: the CIGAR of every pair of an align batch, from a traced fill of the reported span.
 * For a pair, let score, a_begin..a_end, b_begin..b_end be exactly what an AGX_SW_ALIGN_SPANS batch of the same mode and
 * scoring reports.  x = a[a_begin..a_end], length ca, is the query; y = b[b_begin..b_end], length cb, the target; w(i,j) is
 * what the diagonal move adds for y[i-1], x[j-1] (match / mismatch, or the matrix entry); o = gap_open + gap_extend,
 * e = gap_extend.  Whatever the mode, the reported alignment is a GLOBAL alignment of x with y.  Pinned Gotoh, for
 * 0 <= i <= cb, 0 <= j <= ca:
 *   H[0][0] = 0;  H[0][j] = gap_open + j e (j > 0);  H[i][0] = gap_open + i e (i > 0);  E[0][j] = F[i][0] = -infinity
 *   E[i][j] = max(H[i-1][j] + o, E[i-1][j] + e)      (consumes a target symbol only: D)
 *   F[i][j] = max(H[i][j-1] + o, F[i][j-1] + e)      (consumes a query symbol only:  I)
 *   H[i][j] = max(H[i-1][j-1] + w(i,j), E[i][j], F[i][j])
 * H[cb][ca] == score always holds.  The CIGAR is the path found by walking back from (cb, ca) in state H; the tie rule
 * prefers the diagonal, then D, then I, and opens a gap before it extends one:
 *   state H, i > 0 and j > 0:  if H[i][j] == H[i-1][j-1] + w(i,j) emit '=' or 'X' and go to (i-1, j-1) in state H;
 *                              otherwise, if H[i][j] == E[i][j], go to state E at the same cell; otherwise to state F there.
 *   state E at (i, j):         emit D.  If E[i-1][j] + e > H[i-1][j] + o (strictly) stay in E at (i-1, j), otherwise go to
 *                              H at (i-1, j).
 *   state F at (i, j):         emit I.  Stay in F at (i, j-1) only on strict F[i][j-1] + e > H[i][j-1] + o, otherwise go to
 *                              H at (i, j-1).
 *   state H with i == 0:       emit j x I and stop.       state H with j == 0:  emit i x D and stop.
 * The emitted operations are reversed and equal neighbours merged into maximal runs.  An operation is
 * uint32_t = length << 4 | op with the BAM codes below.  '=' means identical input bytes; under a matrix identical symbol
 * codes, whatever that entry scores -- the rule `matches` uses in the stats contract.
 * Answered without a fill: nothing consumed gives zero operations (a LOCAL or EXTEND score of 0, both sides empty);
 * ca == 0 < cb gives cb D; cb == 0 < ca gives ca I (GLOBAL with an empty side, FIT / EXTEND_QUERY with b_end = -1).
 * Soft clips are the caller's arithmetic from the hit.
 * Relation to the stats ("Alignment statistics"): the CIGAR is ONE optimal alignment of the span, the stats describe the
 * optimal alignment with the most matches.  So sum('=') <= matches, and where they are equal sum('=' + 'X') <= pairs.
 * Limits: the query of a cigar batch is at most AGX_SW_CIGAR_MAX_QUERY_LEN (a longer one fails the create with AGX_E_LIMIT, in
 * every mode), the target AGX_SW_ALIGN_MAX_TARGET_LEN.
 * Memory: the traced fill writes four bits per cell of the span.  agx_sw_batch_cigars cuts the traced pairs into chunks in
 * the caller's order: a chunk takes pairs until the next one would pass AGX_OPT_SW_TRACE_BYTES (directions and operation
 * slots together, counted by a bound that does not depend on the plan), and always at least one.  The largest pair the
 * limits admit (2048 x 65 535) needs about 67 MB of directions plus its slot, so no pair is refused for size.  The block is
 * returned to the context's pool after every chunk: a resident batch holds none of it between calls.
 */
#define AGX_CIGAR_INS 1
#define AGX_CIGAR_DEL 2
#define AGX_CIGAR_EQ 7
#define AGX_CIGAR_DIFF 8
#define AGX_SW_CIGAR_MAX_QUERY_LEN 2048 /* 64 lanes x 32 columns (the four widest lane classes are not built with the trace) */
typedef struct agx_sw_cigar_info { /* of the last agx_sw_batch_cigars on this batch */
    int64_t n_traced;              /* pairs that needed a traced fill (ca > 0 and cb > 0) */
    int64_t trace_cells;           /* sum ca*cb over them */
    int64_t trace_bytes_peak;      /* largest device block held for directions + operation slots at one time */
    int32_t n_chunks, reserved;
} agx_sw_cigar_info;
/* A cigar batch is an AGX_SW_ALIGN_SPANS batch of `mode` that can also answer agx_sw_batch_cigars.  Exactly one way of scoring,
 * as agx_sw_batch_create_align_stats.  launch, scores, hits, bind_scores (accepted and ignored) behave as on a stats batch;
 * agx_sw_batch_stats on it is AGX_E_ARG (the two do not combine).  ctx may be NULL: plan only. */
int agx_sw_batch_create_align_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, const uint8_t *bases,
                                    const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* Waits for the launched fill.  Writes hits (may be NULL) and op_off[0..n_pairs] always; pair p's operations are
 * ops[op_off[p] .. op_off[p+1]).  ops == NULL is the sizing call: AGX_OK with op_off filled.  ops != NULL with
 * ops_cap < op_off[n_pairs]: AGX_E_ARG, the message names the count needed, ops is left untouched.  The result is kept in the
 * batch until the next launch or the destroy, so the sizing call followed by the real one costs one computation.
 * Every CIGAR is checked on the host before it is returned: the traced fill's corner score equals the hit's score, the
 * operations consume exactly ca and cb, every '=' and 'X' agrees with the symbols, no two neighbouring runs share an op,
 * and rescoring the operations (o for the first cell of a run of I or D, e for each further one) gives the score --
 * AGX_E_INTERNAL naming the pair otherwise: no CIGAR is returned that the library cannot vouch for.
 * AGX_E_ARG on a batch that was not created by agx_sw_batch_create_align_cigar. */
int agx_sw_batch_cigars(agx_sw_batch *b, agx_sw_hit *hits /* may be NULL */, uint64_t *op_off, uint32_t *ops, uint64_t ops_cap);
int agx_sw_batch_cigar_info(const agx_sw_batch *b, agx_sw_cigar_info *info);
/* One-shot: create_align_cigar + launch + cigars + destroy.  ops_cap >= sum(len) always suffices. */
int agx_sw_align_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, const uint8_t *bases,
                       const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits /* may be NULL */, uint64_t *op_off,
                       uint32_t *ops, uint64_t ops_cap);

/*
 * Banded alignment: global and extension alignment of long, similar pairs.  Only the cells within a fixed distance of the main
 * diagonal are filled: the cost is length x band, and NEITHER side has a column limit.  a, b, la, lb, D[i][j] (pinned start, no
 * zero floor) and the gap costs are those of "Alignment modes".  A batch has one half-width band = w >= 0; a cell (i, j) is
 * inside the band iff dlo <= j - i <= dhi:
 *   mode                 dlo                    dhi                    score                              end cell
 *   AGX_SW_MODE_GLOBAL   min(0, la - lb) - w    max(0, la - lb) + w    D[lb][la]                          (lb-1, la-1)
 *   AGX_SW_MODE_EXTEND   -w                     +w                     max over the in-band cells,        smallest i, then smallest j among
 *                                                                      D[0][0] = 0 included, so >= 0      the maxima; score 0: all four -1
 * The GLOBAL band is widened by the length difference: both corners are inside and connected, so a global score is always finite.
 * Cells outside the band do not exist: H = E = F = -infinity there and nothing is read from them.  Of row 0 and column 0 only
 * the in-band parts exist: D[0][j] = gap_open + j gap_extend for 0 < j <= dhi, D[i][0] likewise for 0 < i <= -dlo; E is
 * -infinity on row 0 and F in column 0.  Begins are what a pinned-start AGX_SW_ALIGN_SPANS batch reports: 0 (an empty range is
 * begin 0, end -1; EXTEND with score 0 keeps -1 for all four); there is no second fill.  A pair with an empty side is answered
 * by the formulas without a fill: GLOBAL with la = 0 gives gap_open + lb gap_extend, both sides empty 0, EXTEND 0.
 * A band wide enough to hold the whole matrix reports exactly what agx_sw_align_mode(..., AGX_SW_ALIGN_SPANS, ...) reports for
 * the same mode and scoring: that is so for w >= min(la, lb) in GLOBAL and for w >= max(la, lb) in EXTEND.
 * Limits: la, lb <= AGX_SW_BAND_MAX_LEN on BOTH sides, and width = dhi - dlo + 1 <= AGX_SW_BAND_MAX_WIDTH (64 lanes x 32
 * diagonals): |la - lb| + 2w + 1 in GLOBAL, 2w + 1 in EXTEND.  A pair beyond either fails the create with AGX_E_LIMIT, the
 * message names the pair.  band < 0: AGX_E_ARG.  LOCAL, FIT and EXTEND_QUERY have a free start or a column capture; a band
 * around the main diagonal means nothing for them without a diagonal offset: AGX_E_ARG, as for a mode outside 0..4 (they are
 * served by "Banded alignment around a diagonal" below).
 * scoring: agx_sw_scoring with its limits, NULL = the reference's constants.  Byte 0x00 is refused (AGX_E_SYMBOL) as elsewhere.
 * Deliberately left out: no substitution matrix (a band under a matrix is "Banded alignment around a diagonal under a
 * substitution matrix" below, whose EXTEND with diag == NULL is this entry's EXTEND band; GLOBAL with the widening is not offered
 * under a matrix) and no statistics; CIGARs come from a banded cigar batch ("CIGARs for banded batches" below), not from this one.
 * The batch behaves like the other align batches: agx_sw_batch_launch (re)launches, agx_sw_batch_scores returns the mode's
 * score, agx_sw_batch_hits the hits in the caller's pair order, agx_sw_batch_bind_scores is accepted and ignored;
 * agx_sw_batch_stats and agx_sw_batch_cigars return AGX_E_ARG.  ctx may be NULL: plan only.  In agx_sw_info, cells stays
 * sum la*lb as given and padded_cells is lane-steps x diagonals per lane actually issued.
 */
#define AGX_SW_BAND_MAX_LEN 65535
#define AGX_SW_BAND_MAX_WIDTH 2048
int agx_sw_batch_create_align_band(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases,
                                   const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band + launch + hits + destroy. */
int agx_sw_align_band(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases, const uint64_t *off,
                      const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits);

/*
 * CIGARs for banded batches: the alignment itself for the pairs only the band can align.  A banded cigar batch is a banded
 * batch (mode GLOBAL or EXTEND, half-width band = w; the same limits, scoring, hits and errors) that also answers
 * agx_sw_batch_cigars and agx_sw_batch_cigar_info.
 * Spans: for a pair, score, a_end and b_end are exactly what the banded batch of the same mode, band and scoring reports;
 * begins are 0.  x = a[0..a_end], length ca, is the query; y = b[0..b_end], length cb, the target.
 * Band: the CIGAR is a path inside the pair's band, the one the score was computed in --
 *   GLOBAL: dlo = min(0, la - lb) - w, dhi = max(0, la - lb) + w;   EXTEND: dlo = -w, dhi = +w.
 * The EXTEND band is NOT widened by ca - cb: a wider band could hold a better path to the end cell than the one that was scored
 * (|ca - cb| <= w holds because the end cell is in the band).  Cells outside the band do not exist: H = E = F = -infinity.
 * Recurrence and tie rule are those of "Alignment itself" over the in-band cells only, row 0 and column 0 existing only inside
 * the band: in state H prefer the diagonal, then E (D), then F (I); stay in a gap only on a strict E[i-1][j] + e > H[i-1][j] + o,
 * likewise for F; state H with i == 0 emits j x I, with j == 0 i x D.  Whatever the mode, the reported alignment is a global
 * alignment of x with y inside the band.  Operations, BAM codes, run merging, the sizing call, ops_cap, keeping the answer until
 * the next launch, agx_sw_cigar_info, chunking by AGX_OPT_SW_TRACE_BYTES in the caller's order (always at least one pair per
 * chunk) and returning the block to the pool after every chunk are as on a cigar batch; trace_cells is the number of in-band
 * cells (1 <= i <= cb, 1 <= j <= ca) of the traced spans.
 * Answered without a fill, as there: nothing consumed (EXTEND score 0, both sides empty) gives zero operations; ca == 0 < cb
 * gives cb D, cb == 0 < ca gives ca I (for a GLOBAL pair with an empty side the band holds that run by construction).
 * Every CIGAR is checked on the host before it is returned: the checks of agx_sw_batch_cigars, the traced fill's corner score
 * against the hit's, and after every operation dlo <= j - i <= dhi -- AGX_E_INTERNAL naming the pair otherwise.
 * Wide band: a band wide enough to hold the whole matrix returns exactly what agx_sw_align_cigar returns for the same mode and
 * scoring, hit for hit and operation for operation: w >= min(la, lb) in GLOBAL, w >= max(la, lb) in EXTEND.
 * No new limit.  The traced fill writes four bits per in-band cell, step-major: a pair whose band is tiled as G lanes of K
 * diagonals (G K >= dhi - dlo + 1, K one of 4, 8, 16, 32, all four built with the trace) takes (cb + G) x G x ceil(K / 8) dwords.
 * The largest pair the band admits, 65 535 rows x 2048 diagonals, is (65 535 + 64) x 64 x 4 dwords = 67.2 MB of directions plus
 * its slot of ca + cb words, so no pair is refused for size.
 * Unchanged: a plain banded batch keeps answering agx_sw_batch_cigars with AGX_E_ARG; agx_sw_batch_stats on a banded cigar
 * batch is AGX_E_ARG.  ctx may be NULL: plan only.
 */
int agx_sw_batch_create_align_band_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases,
                                         const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band_cigar + launch + cigars + destroy.  ops_cap >= sum(len) always suffices. */
int agx_sw_align_band_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases, const uint64_t *off,
                            const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits /* may be NULL */, uint64_t *op_off, uint32_t *ops,
                            uint64_t ops_cap);
/* Host only, no device.  What one traced pair of a banded cigar batch counts against AGX_OPT_SW_TRACE_BYTES: the directions of
 * its cb rows in the tiling of `width` = dhi - dlo + 1 diagonals that takes the most, plus its slot; it does not depend on the
 * plan.  0 for a width outside 1..AGX_SW_BAND_MAX_WIDTH. */
uint64_t agx_sw_band_cigar_bytes_bound(int32_t width, uint32_t ca, uint32_t cb);
/* Host only: 1 if the path of ops[0..n_ops) from (0, 0) keeps dlo <= j - i <= dhi after every operation (and starts inside),
 * 0 if it leaves the band or holds an operation other than I, D, = and X.  The band check of agx_sw_batch_cigars. */
int agx_sw_cigar_in_band(const uint32_t *ops, uint64_t n_ops, int32_t dlo, int32_t dhi);

/*
 * Banded alignment around a diagonal: all five modes inside a band around a caller-given diagonal, e.g. a 10 000-base read placed
 * in a 60 000-base window near where a seed chain says it lies (FIT at diag = minus the expected start).  a, b, la, lb, D[i][j],
 * the gap costs, the zero floor of LOCAL, the tie rules and the coordinates are those of "Alignment coordinates" and "Alignment
 * modes"; what = AGX_SW_ALIGN_ENDS or AGX_SW_ALIGN_SPANS.
 * Band: for pair p, with c = diag[p] (diag == NULL: 0 for every pair) and w = band, a cell (i, j) is inside the band iff
 *   dlo = c - w <= j - i <= dhi = c + w,
 * exactly, in every mode: it is never widened (the GLOBAL widening of "Banded alignment" stays that entry's).  Cells outside the
 * band do not exist: H = E = F = -infinity there and nothing is read from them; of row 0 and column 0 only the in-band parts
 * exist.  band < 0: AGX_E_ARG.  2w + 1 > AGX_SW_BAND_MAX_WIDTH (w > 1023): AGX_E_LIMIT.  |c| > AGX_SW_BAND_MAX_LEN + w:
 * AGX_E_ARG naming the pair.  la, lb <= AGX_SW_BAND_MAX_LEN (AGX_E_LIMIT naming the pair).
 * Boundaries, by the recurrence over the in-band cells:
 *   pinned modes (GLOBAL, EXTEND, EXTEND_QUERY)  D[0][0] = 0; D[0][j] and D[i][0] are the gap-initialised values where the in-band
 *                                                chain from (0, 0) reaches them (0 < j <= dhi, 0 < i <= -dlo)
 *   FIT                                          D[i][0] = 0 for every in-band (i, 0), 0 <= i <= lb; row 0 as in the pinned modes,
 *                                                so it exists beyond (0, 0) only if (0, 0) is inside the band
 *   LOCAL                                        the zero floor in every in-band cell
 * What the band must hold -- otherwise the create fails with AGX_E_ARG and the message names the pair:
 *   AGX_SW_MODE_GLOBAL        dlo <= 0 <= dhi and dlo <= la - lb <= dhi
 *   AGX_SW_MODE_EXTEND        dlo <= 0 <= dhi
 *   AGX_SW_MODE_EXTEND_QUERY  dlo <= 0 <= dhi and dhi >= la - lb
 *   AGX_SW_MODE_FIT           dlo <= 0 and dhi >= la - lb   (an in-band cell in column 0 and one in column la, rows 0..lb)
 *   AGX_SW_MODE_LOCAL         nothing: with no in-band cell at 1 <= i <= lb, 1 <= j <= la the pair scores 0 without a fill
 * Under these conditions every score is finite: the band clipped to the matrix is convex, so a monotone path inside it joins a
 * start cell to an end cell.  The conditions are checked for every pair, those with an empty side included; such pairs are then
 * answered by the formulas of "Alignment modes" without a fill (LOCAL: score 0, all four positions -1).
 * Results: score and end cell follow the mode's rule, taken over in-band cells only --
 *   LOCAL, EXTEND          the maximum (EXTEND: D[0][0] = 0 included), then the smallest b_end, then the smallest a_end; a score
 *                          of 0 gives all four positions -1
 *   FIT, EXTEND_QUERY      the maximum of D[i][la] over the in-band i in 0..lb, with the smallest such i: a_end = la - 1, b_end = i - 1
 *   GLOBAL                 D[lb][la]
 * AGX_SW_ALIGN_ENDS leaves the begins at -1.  AGX_SW_ALIGN_SPANS: the pinned modes begin at 0 (EXTEND with score 0 keeps -1).
 * LOCAL: the begin cell is the contract's -- latest in b, then latest in a -- among the alignments INSIDE THE BAND of that score
 * that end in the end cell; it is found by a second banded LOCAL fill of the reversed prefixes a[a_end..0], b[b_end..0] around
 * the mirror image of the band, centre (a_end + 1) - (b_end + 1) - c, the same w.  FIT: a_begin = 0 and b_begin = the latest
 * start among the in-band alignments of that score that consume b through b_end (0 when b_end = -1; b_end + 1 when the latest
 * one consumes nothing of b: all of a in one gap along row b_end + 1), found by a second banded EXTEND_QUERY fill of reversed a
 * against reversed b[0..b_end] around centre la - (b_end + 1) - c.  In both the reverse score must equal the forward one:
 * AGX_E_INTERNAL naming the pair otherwise.
 * Equivalences:
 *   a band that holds the whole matrix (c - w <= -lb and c + w >= la) reports exactly what agx_sw_align_mode reports for the same
 *       mode, `what` and scoring;
 *   EXTEND with diag == NULL reports what agx_sw_align_band(AGX_SW_MODE_EXTEND) reports for the same band;
 *   GLOBAL with c = 0 on pairs with la == lb reports what agx_sw_align_band(AGX_SW_MODE_GLOBAL) reports.
 * Cost: the band touches the rows max(0, -dhi) .. min(lb, la - dlo) only, and only those are filled: a read of 2000 in a window of
 * 65 535 costs about 2000 x width.  In agx_sw_info, cells stays sum la*lb as given, padded_cells is what is issued.
 * The batch behaves like a banded batch: agx_sw_batch_launch (re)launches, agx_sw_batch_scores returns the mode's score,
 * agx_sw_batch_hits the hits in the caller's pair order, agx_sw_batch_bind_scores is accepted and ignored, agx_sw_batch_info
 * works; agx_sw_batch_stats and agx_sw_batch_cigars return AGX_E_ARG.  ctx may be NULL: plan only.  scoring and byte 0x00 as in
 * "Banded alignment".  Unchanged: agx_sw_batch_create_align_band still refuses LOCAL, FIT and EXTEND_QUERY with AGX_E_ARG.
 * CIGARs come from "CIGARs for batches banded around a diagonal" below, z-drop termination of EXTEND from "Z-drop for banded
 * extension", substitution matrices from "Banded alignment around a diagonal under a substitution matrix", matches and aligned
 * pairs from "Statistics for batches banded around a diagonal".
 */
int agx_sw_batch_create_align_band_diag(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, int32_t band,
                                        const int32_t *diag /* n_pairs, or NULL = 0 for every pair */, const uint8_t *bases,
                                        const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band_diag + launch + hits + destroy. */
int agx_sw_align_band_diag(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, int32_t band, const int32_t *diag,
                           const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits);

/*
 * CIGARs for batches banded around a diagonal: the alignment itself for a read placed in its window.  The batch is a batch of
 * "Banded alignment around a diagonal" with what = AGX_SW_ALIGN_SPANS -- any of the five modes, the same band c - w .. c + w per
 * pair, the same conditions on what the band must hold, limits, trimmed rows, hits and errors -- that also answers
 * agx_sw_batch_cigars and agx_sw_batch_cigar_info.
 * Per pair: hits[p] is exactly what the band-diag SPANS batch of the same mode, band, diag and scoring reports.  The CIGAR consumes
 * a[a_begin..a_end] and b[b_begin..b_end].  Its path, run from the begin cell (b_begin, a_begin), stays within
 * dlo <= j - i <= dhi of the FULL matrix (dlo = c - w, dhi = c + w); seen from the span, whose cell (i', j') is
 * (b_begin + i', a_begin + j'), that is the band dlo - delta .. dhi - delta with delta = a_begin - b_begin, the same width.  It
 * rescores to `score`.  Among such paths it is the one the tie rule of "CIGARs for banded batches" picks, applied to the global
 * alignment of the span inside that band: in state H prefer the diagonal, then E (D), then F (I); a gap extends only on a strict
 * improvement.  Cells outside the band do not exist.
 * Lone cases: a span with one empty side gives a lone run, ca I or cb D (ca = a_end - a_begin + 1, cb = b_end - b_begin + 1) --
 * FIT's b_begin = b_end + 1 (all of a in one gap along row b_end + 1) included -- and that run is checked against the band like
 * any other path.  A pair with no aligned symbol (a LOCAL pair of score 0, or one whose band misses the matrix; an empty pair)
 * has no operations; its text form is "*".
 * Equivalences: a band that holds the whole matrix returns exactly what agx_sw_align_cigar returns for the same mode and
 * scoring; EXTEND with diag == NULL what agx_sw_align_band_cigar(AGX_SW_MODE_EXTEND) returns for the same band; GLOBAL with
 * c = 0 on pairs with la == lb what agx_sw_align_band_cigar(AGX_SW_MODE_GLOBAL) returns.
 * agx_sw_batch_cigars uploads no sequence byte: the traced fill of a span starts inside the batch's resident image, wherever
 * the span begins.  Operations, BAM codes, run merging, the sizing call, ops_cap, keeping the answer until the
 * next launch, chunking under AGX_OPT_SW_TRACE_BYTES (agx_sw_band_cigar_bytes_bound(2w + 1, ca, cb) per traced pair, a pair
 * beyond the budget alone in its chunk), agx_sw_cigar_info and the host's check of every CIGAR before it leaves (AGX_E_INTERNAL
 * naming the pair) are as in "CIGARs for banded batches".  ctx may be NULL: plan only.
 * Unchanged: a plain band-diag batch keeps answering agx_sw_batch_cigars with AGX_E_ARG; agx_sw_batch_stats on this batch gives
 * AGX_E_ARG.  Substitution matrices come from "Banded alignment around a diagonal under a substitution matrix" below; matches
 * and aligned pairs without a traceback from "Statistics for batches banded around a diagonal".
 */
int agx_sw_batch_create_align_band_diag_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band,
                                              const int32_t *diag /* n_pairs, or NULL = 0 for every pair */, const uint8_t *bases,
                                              const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band_diag_cigar + launch + cigars + destroy.  ops_cap >= sum(len) always suffices. */
int agx_sw_align_band_diag_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag,
                                 const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits,
                                 uint64_t *op_off, uint32_t *ops, uint64_t ops_cap);

/*
 * Banded alignment around a diagonal under a substitution matrix: protein extension around a seed diagonal under BLOSUM62, DNA
 * under an IUPAC or transition/transversion matrix, any query beyond AGX_SW_ALIGN_MAX_QUERY_LEN under a matrix -- the batches of
 * "Banded alignment around a diagonal" and of "CIGARs for batches banded around a diagonal" with an agx_sw_matrix in place of
 * the agx_sw_scoring.
 * Base contract: everything is as in those two sections -- the band c - w <= j - i <= c + w per pair (never widened), the table
 * of what the band must hold per mode, boundaries, result and tie rules, the begin pass of LOCAL and FIT under
 * AGX_SW_ALIGN_SPANS, trimmed rows, limits (la, lb <= AGX_SW_BAND_MAX_LEN, w <= 1023, |c| <= AGX_SW_BAND_MAX_LEN + w), error
 * codes and messages, the empty-side formulas, plan-only batches with ctx == NULL, launch and relaunch, agx_sw_batch_scores,
 * _hits, _info, bind_scores accepted and ignored, and on the cigar batch agx_sw_batch_cigars and _cigar_info with their chunking
 * under AGX_OPT_SW_TRACE_BYTES and agx_sw_band_cigar_bytes_bound.  The one difference: the diagonal move adds
 * score[code[a_j]][code[b_i]], and the gap costs are the matrix's gap_open and gap_extend.
 * Matrix: validated as agx_sw_batch_create_align_matrix validates it -- NULL, n_symbols outside 1..32, an asymmetric matrix or a
 * code that is neither 0xff nor below n_symbols: AGX_E_ARG; a gap cost outside -1000..0: AGX_E_LIMIT -- and before anything
 * else that can fail (mode, what, band, the pairs), also when ctx == NULL.
 * Symbols: a byte outside the alphabet (code 0xff) fails the create with AGX_E_SYMBOL naming the lowest such pair among the
 * pairs that are filled; all of b is checked, the rows the band leaves out included.  Byte 0x00 is a symbol like any other if
 * the matrix maps it.  As in the base contract the check belongs to the image build, so a plan-only batch does not make it.
 * Score zero: as in "Align batches under a substitution matrix" a diagonal score may be <= 0 even for identical symbols, so a
 * LOCAL or EXTEND score of 0 means "nothing consumed" -- all four positions -1, no operations -- whatever the sequences hold;
 * GLOBAL, FIT and EXTEND_QUERY scores may be negative.
 * CIGARs: '=' means identical symbol CODES, whatever that entry scores -- two bytes mapped to one code, such as upper and lower
 * case, are '=' -- and 'X' any other aligned pair.  The host's check of every CIGAR rescores under the matrix.
 * Range: entries are int8 and a path has at most 65 535 diagonal moves, so every score lies within -1.4e8 .. 8.4e6 (DESIGN.md
 * 4.1l has the bound for the intermediate values).
 * Equivalences:
 *   a band that holds the whole matrix (c - w <= -lb and c + w >= la) reports what agx_sw_align_matrix reports in the same mode
 *       and `what`, and its cigar batch what agx_sw_align_cigar reports with the matrix;
 *   a matrix over ACGT whose entries restate a supported scoring -- `match` on the diagonal, `mismatch` elsewhere, the scoring's
 *       gaps -- reports, on sequences over the bytes it maps to those four codes, what agx_sw_align_band_diag and
 *       agx_sw_align_band_diag_cigar report under that scoring on the same sequences with identical bytes for identical codes,
 *       hit for hit and operation for operation.
 * Both kinds of batch return AGX_E_ARG from agx_sw_batch_stats and agx_sw_batch_zdrop_stops, the batch without CIGARs also from
 * agx_sw_batch_cigars.
 * Deliberately left out: statistics on banded batches under a matrix, z-drop under a matrix, and a matrix for agx_sw_batch_create_align_band
 * (EXTEND with diag == NULL here is its EXTEND band; its GLOBAL band, widened by the length difference, is not offered).
 */
int agx_sw_batch_create_align_band_diag_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int what, int32_t band,
                                               const int32_t *diag /* n_pairs, or NULL = 0 for every pair */, const uint8_t *bases,
                                               const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band_diag_matrix + launch + hits + destroy. */
int agx_sw_align_band_diag_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int what, int32_t band, const int32_t *diag,
                                  const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits);
int agx_sw_batch_create_align_band_diag_matrix_cigar(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int32_t band,
                                                     const int32_t *diag /* n_pairs, or NULL = 0 for every pair */, const uint8_t *bases,
                                                     const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band_diag_matrix_cigar + launch + cigars + destroy.  ops_cap >= sum(len) always suffices. */
int agx_sw_align_band_diag_matrix_cigar(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int32_t band, const int32_t *diag,
                                        const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                                        agx_sw_hit *hits /* may be NULL */, uint64_t *op_off, uint32_t *ops, uint64_t ops_cap);

/*
 * Z-drop for banded extension: AGX_SW_MODE_EXTEND inside a band around a diagonal that stops extending once the alignment has
 * fallen apart -- a read whose tail is junk (a chimera, an adapter, the far side of a structural variant) neither pays for all of
 * its rows nor picks up an unrelated high-scoring stretch further down the band.
 * Everything is as in "Banded alignment around a diagonal", mode AGX_SW_MODE_EXTEND: the band dlo = c - w <= j - i <= dhi = c + w,
 * the admission rule dlo <= 0 <= dhi, limits, scoring and the symbol rules, diag == NULL meaning 0.  One batch-wide integer
 * `zdrop` is added.
 * The rule: let last = min(lb, la - dlo), the last row with an in-band cell.  For row i, R(i) is the maximum of D[i][j] over the
 * in-band j in 0..la and c(i) the smallest j that attains it.  The running best starts as B = D[0][0] = 0 at (bi, bj) = (0, 0).
 * For i = 1, 2, .., last in order:
 *   if R(i) > B: B = R(i), (bi, bj) = (i, c(i)); the drop test is not made in such a row;
 *   otherwise, if B - R(i) > zdrop + |gap_extend| * |(i - bi) - (c(i) - bj)|, strictly, the extension TERMINATES AT ROW i: later
 *   rows do not exist for this pair.
 * This is ksw2's ksw_extz rule stated over rows; the second term forgives the extension cost of one long gap since the best cell.
 * Reporting: the hit is B with end cell (bi - 1, bj - 1); score 0 keeps all four positions at -1; under AGX_SW_ALIGN_SPANS the
 * begins are 0, as for EXTEND.  Per pair the library also reports stop = i - 1 for the terminating row i -- the index in b of the
 * last row looked at -- and -1 when the fill ran through, which includes pairs with an empty side and pairs of score 0 that
 * never dropped.
 * Limits: 0 <= zdrop <= AGX_SW_ZDROP_MAX, AGX_E_ARG outside.  Under the supported scorings and lengths B - R(i) <= 7.9e5 + 1.32e8
 * and the right side stays below 2^31, so nothing wraps and zdrop = AGX_SW_ZDROP_MAX never fires.
 * Equivalences: with zdrop = AGX_SW_ZDROP_MAX the hits equal those of agx_sw_align_band_diag(AGX_SW_MODE_EXTEND) for the same
 * band, diag, `what` and scoring, and every stop is -1; with a band that holds the whole matrix as well they equal those of
 * agx_sw_align_mode(AGX_SW_MODE_EXTEND).  Example under the reference scoring (1, -1, -3, -1), w = 4, c = 0: a = AAAATTTTTTTT,
 * b = AAAACCCCCCCC gives the hit (4, 0, 3, 0, 3) for every zdrop, stop = 4 + zdrop for zdrop = 0..7 and stop = -1 from 8 on.
 * `mode` is kept in the signatures: anything but AGX_SW_MODE_EXTEND is AGX_E_ARG for now.
 * A z-drop batch behaves like a band-diag batch in every other respect: launch and relaunch, agx_sw_batch_scores, _hits and
 * _info, agx_sw_batch_bind_scores accepted and ignored, agx_sw_batch_stats AGX_E_ARG, ctx == NULL a plan-only batch.
 * agx_sw_batch_zdrop_stops waits for the launched fill like agx_sw_batch_hits; on any other kind of batch it is AGX_E_ARG.  It
 * checks -1 <= stop < lb and stop >= b_end for every pair (AGX_E_INTERNAL naming the pair).
 * The cigar batch is a batch of "CIGARs for batches banded around a diagonal" whose hits come from the z-drop fill: the reported
 * end cell is an in-band cell reached from (0, 0) inside the band, so the traced fill of the span, the band-aware walk and the
 * host's checks apply unchanged.
 * Deliberately left out: a z-drop for the unbanded EXTEND of agx_sw_align_mode, a z-drop under a substitution matrix, and an
 * X-drop variant.
 */
#define AGX_SW_ZDROP_MAX 1000000000
int agx_sw_batch_create_align_band_zdrop(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, int32_t band,
                                         const int32_t *diag /* n_pairs, or NULL = 0 for every pair */, int32_t zdrop,
                                         const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                                         agx_sw_batch **out);
/* One-shot: create_align_band_zdrop + launch + hits + stops + destroy. */
int agx_sw_align_band_zdrop(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, int32_t band, const int32_t *diag,
                            int32_t zdrop, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                            agx_sw_hit *hits, int32_t *stops /* n_pairs; may be NULL */);
int agx_sw_batch_zdrop_stops(agx_sw_batch *b, int32_t *stops /* n_pairs */);
int agx_sw_batch_create_align_band_zdrop_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag,
                                               int32_t zdrop, const uint8_t *bases, const uint64_t *off, const uint32_t *len,
                                               int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band_zdrop_cigar + launch + cigars + stops + destroy. */
int agx_sw_align_band_zdrop_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag, int32_t zdrop,
                                  const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits,
                                  int32_t *stops /* may be NULL */, uint64_t *op_off, uint32_t *ops, uint64_t ops_cap);

/*
 * Statistics for batches banded around a diagonal: matches and aligned pairs of a banded alignment without a traceback -- the
 * identity filter for long reads ("keep reads above 90 %"), which an unbanded stats batch cannot serve beyond
 * AGX_SW_STATS_MAX_QUERY_LEN and a cigar batch serves only at the price of a traced fill and a walk.
 * For a pair, let score, a_begin..a_end, b_begin..b_end be exactly what an AGX_SW_ALIGN_SPANS batch of
 * agx_sw_batch_create_align_band_diag reports for the same mode, scoring, band and diag.  Consider the alignments that run
 * through IN-BAND CELLS ONLY (dlo = c - w <= j - i <= dhi = c + w of the full matrix, after every operation), attain `score`, and
 * consume exactly a[a_begin..a_end] and b[b_begin..b_end].  Among these take the one with the most matches, and among those the
 * one with the most pairs; pairs, matches and the caller's arithmetic (columns, mismatches, gap cells, identity) are those of
 * "Alignment statistics".  Nothing consumed gives {0, 0}: a LOCAL or EXTEND score of 0 (a LOCAL band that misses the matrix
 * included), an empty side, b_end = -1, and FIT's empty range b_begin = b_end + 1 (all of a in one gap).
 * The CIGAR of "CIGARs for batches banded around a diagonal" is ONE of these alignments, the one its tie rule picks; its count of
 * '=' and of '=' + 'X' is therefore lexicographically <= (matches, pairs), with equality where the optimal in-band path is unique.
 * The batch: an AGX_SW_ALIGN_SPANS batch of "Banded alignment around a diagonal" -- the same band conditions per mode, limits,
 * trimmed rows and errors naming the pair; agx_sw_batch_launch, _scores, _hits and _info behave the same,
 * agx_sw_batch_bind_scores is accepted and ignored, ctx may be NULL: plan only -- that also answers agx_sw_batch_stats(b, hits,
 * stats).  Every stat is checked before it is returned by the rule of agx_sw_batch_stats (0 <= matches <= pairs <= min(ca, cb);
 * the score minus matches, mismatches and gap cells is a whole number of gap opens within its bounds): AGX_E_INTERNAL naming the
 * pair otherwise.
 * No new limit: every lane class of the banded fill is built with statistics, so the widest band stays AGX_SW_BAND_MAX_WIDTH.
 * Unchanged: agx_sw_batch_stats on a plain band-diag, cigar, z-drop or matrix batch keeps returning AGX_E_ARG, and this batch
 * returns AGX_E_ARG from agx_sw_batch_cigars and agx_sw_batch_zdrop_stops.
 * Deliberately left out: statistics under a substitution matrix, with a z-drop, and for agx_sw_batch_create_align_band with its
 * GLOBAL widening; the number of gap opens, as in "Alignment statistics".
 */
int agx_sw_batch_create_align_band_diag_stats(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band,
                                              const int32_t *diag /* n_pairs, or NULL = 0 for every pair */, const uint8_t *bases,
                                              const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band_diag_stats + launch + stats + destroy. */
int agx_sw_align_band_diag_stats(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag,
                                 const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                                 agx_sw_hit *hits /* may be NULL */, agx_sw_stat *stats);

/*
 * Banded alignment around a diagonal under two-piece gap costs: the gap model of long-read aligners (minimap2's -O4,24 -E2,1,
 * the recurrence of its ksw2_extd2).  A gap of L >= 1 symbols scores
 *     max(gap_open + L gap_extend, gap_open2 + L gap_extend2)
 * -- one piece steep for short gaps, one shallow for long ones; no setting of one piece gives both.  As a recurrence over the
 * in-band cells: E1 and F1 use piece 1, E2 and F2 piece 2, each exactly like E and F of "Banded alignment around a diagonal";
 * H = max(diagonal move, E1, F1, E2, F2), and LOCAL adds the zero floor.
 * Scoring: match, mismatch as agx_sw_scoring; each of the four gap numbers lies in -1000 .. 0 (AGX_E_LIMIT otherwise, as
 * agx_sw_scoring).  No ordering between the pieces is required.  scoring == NULL is AGX_E_ARG: a second piece has no reference
 * default.
 * Everything else is "Banded alignment around a diagonal", verbatim: the band c - w <= j - i <= c + w, never widened; the table
 * "what the band must hold"; the boundaries per mode, where the gap-initialised row 0 and column 0 carry the two-piece cost of
 * their gap; the limits; the result and tie rules (they depend on scores only: which piece a gap was scored by never enters);
 * the SPANS rules -- begins of LOCAL and FIT from a second banded fill of the reversed prefixes around the mirrored diagonal,
 * under the same two pieces, whose score must equal the forward one, AGX_E_INTERNAL naming the pair otherwise --; byte 0x00
 * refused (AGX_E_SYMBOL naming the pair); ctx == NULL: plan only.  The plan (lane tiling, waves, records, image) is that of the
 * agx_sw_batch_create_align_band_diag batch on the same pairs, band and diag.
 * Pairs with an empty side are answered without a fill by the mode's formulas with the two-piece cost: GLOBAL with la = 0 scores
 * max(gap_open + lb gap_extend, gap_open2 + lb gap_extend2).
 * The batch behaves like a batch banded around a diagonal for agx_sw_batch_launch, _scores, _hits and _info;
 * agx_sw_batch_bind_scores is accepted and ignored; agx_sw_batch_stats, _cigars and _zdrop_stops return AGX_E_ARG.
 * Equivalences: if piece 2 never beats piece 1 for any L >= 1 (identical pieces; gap_open2 <= gap_open and gap_extend2 <=
 * gap_extend), the hits are exactly those of agx_sw_align_band_diag under {match, mismatch, gap_open, gap_extend}; the same
 * with the pieces swapped.  A band that holds the whole matrix, under such pieces, therefore reports what agx_sw_align_mode does.
 * CIGARs under two pieces: "CIGARs for batches banded around a diagonal under two-piece gap costs", below.
 * Deliberately left out: a z-drop, a substitution matrix and statistics under two pieces, and a two-piece
 * agx_sw_batch_create_align_band with its GLOBAL widening.
 */
typedef struct agx_sw_scoring_dual {
    int32_t match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2;
} agx_sw_scoring_dual;
int agx_sw_batch_create_align_band_diag_dual(agx_ctx *ctx, const agx_sw_scoring_dual *scoring, int mode, int what, int32_t band,
                                             const int32_t *diag /* n_pairs, or NULL = 0 for every pair */, const uint8_t *bases,
                                             const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band_diag_dual + launch + hits + destroy. */
int agx_sw_align_band_diag_dual(agx_ctx *ctx, const agx_sw_scoring_dual *scoring, int mode, int what, int32_t band, const int32_t *diag,
                                const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits);

/*
 * CIGARs for batches banded around a diagonal under two-piece gap costs: the alignment itself for the caller who places a long
 * read in its window under the gap model above.  One-piece CIGARs are no substitute: no one-piece setting reproduces the
 * two-piece path.
 * The batch is the AGX_SW_ALIGN_SPANS batch of "Banded alignment around a diagonal under two-piece gap costs" in any of the five
 * modes -- the same hits, band conditions, limits, errors, empty-side formulas, plan; ctx == NULL: plan only -- which also answers
 * agx_sw_batch_cigars and agx_sw_batch_cigar_info exactly as the batch of "CIGARs for batches banded around a diagonal" does: the
 * CIGAR consumes a[a_begin..a_end] and b[b_begin..b_end]; run from the begin cell it stays within dlo <= j - i <= dhi of the full
 * matrix after every operation; lone runs, "*" (no operations), ops_cap, the chunks under AGX_OPT_SW_TRACE_BYTES and
 * AGX_E_INTERNAL naming the pair behave as there.  No new limit: every lane class of the banded fill has its traced two-piece
 * build, so the widest band stays AGX_SW_BAND_MAX_WIDTH, and no pair is refused for its size (the largest, 65 535 rows in 2048
 * diagonals, takes about 134 MB of directions: eight bits a cell).
 * Rescoring is under the LITERAL cost: every maximal run of I or of D of length L counts max(gap_open + L gap_extend, gap_open2 +
 * L gap_extend2), '=' match, 'X' mismatch, and the total equals `score`; the host checks that before a CIGAR leaves.  Why it
 * holds although the walk may join a piece-1 stretch of L1 and a piece-2 stretch of L2 of the same direction into one run: with
 * p(L) = open + L extend and opens <= 0, p1(L1) + p2(L2) is at most max(p1(L1 + L2), p2(L1 + L2)) -- if extend >= extend2 then
 * p1(L1) + p2(L2) <= p1(L1) + open2 + L2 extend <= p1(L1 + L2), else p1(L1) + p2(L2) <= open + L1 extend2 + p2(L2) <= p2(L1 + L2);
 * by induction for any number of stretches -- so the walked path's cost under the recurrence, which is
 * `score`, is <= its literal cost; the literal optimum inside the band is the recurrence's optimum (every literal path is a path
 * of the recurrence with each run in its better piece, and by the inequality no path of the recurrence beats its own literal
 * cost), so the literal cost of the walked path, a path inside the band, is <= `score`.  Both: equal.
 * Tie rule, on the global alignment of the span inside the moved band (dlo' = c - w - delta, dhi' = c + w - delta, delta =
 * a_begin - b_begin) under both pieces, walked back from the span's end cell in state H:
 *   in H     prefer the diagonal move ('=' or 'X') where it attains H; else E (a D) if max(E1, E2) >= max(F1, F2), else F (an I);
 *            within the direction piece 1 if its value is >= piece 2's, else piece 2
 *   in Ep    emit D and move up; stay in Ep only where piece p's extension is STRICTLY better than opening from H of the cell
 *            above under piece p:  Ep(i - 1, j) + extend_p > H(i - 1, j) + open_p + extend_p;  otherwise return to H
 *   in Fp    the same to the left with I
 *   H with i = 0 emits j x I, with j = 0 i x D.
 * Equivalences: if piece 2 never beats piece 1 for any L >= 1 (identical pieces; gap_open2 <= gap_open and gap_extend2 <=
 * gap_extend), hits and operations are exactly those of agx_sw_align_band_diag_cigar under {match, mismatch, gap_open,
 * gap_extend}.  If piece 1 is STRICTLY worse for every L >= 1 (gap_open + gap_extend < gap_open2 + gap_extend2 and gap_extend <=
 * gap_extend2), they are exactly those under {match, mismatch, gap_open2, gap_extend2}.  Where piece 1 merely ties piece 2 for
 * some L the preference for piece 1 may pick another gap length of the same score: no equality is claimed there.
 * Unchanged: the plain two-piece batch keeps answering agx_sw_batch_cigars, _stats and _zdrop_stops with AGX_E_ARG; this batch
 * refuses _stats and _zdrop_stops with AGX_E_ARG.
 * Deliberately left out: a z-drop, a substitution matrix and statistics under two pieces, and a two-piece
 * agx_sw_batch_create_align_band with its GLOBAL widening.
 */
int agx_sw_batch_create_align_band_diag_dual_cigar(agx_ctx *ctx, const agx_sw_scoring_dual *scoring, int mode, int32_t band,
                                                   const int32_t *diag /* n_pairs, or NULL = 0 for every pair */, const uint8_t *bases,
                                                   const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out);
/* One-shot: create_align_band_diag_dual_cigar + launch + cigars + destroy. */
int agx_sw_align_band_diag_dual_cigar(agx_ctx *ctx, const agx_sw_scoring_dual *scoring, int mode, int32_t band, const int32_t *diag,
                                      const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits,
                                      uint64_t *op_off, uint32_t *ops, uint64_t ops_cap);
/* Host only, no device.  What one traced pair of such a batch counts against AGX_OPT_SW_TRACE_BYTES: eight bits a cell in the
 * lane class that needs the most for `width` diagonals and cb rows, plus its operation slot of ca + cb words.  0 if width is
 * outside 1 .. AGX_SW_BAND_MAX_WIDTH.  (agx_sw_band_cigar_bytes_bound is unchanged.) */
uint64_t agx_sw_band_dual_cigar_bytes_bound(int32_t width, uint32_t ca, uint32_t cb);
/* Host only, no device.  A permanent entry of the ABI, for callers who want to validate a CIGAR they hold (one they edited, or
 * one from another aligner) against a score under two-piece costs, and for the project's own tests of the check below -- the
 * library applies it to every CIGAR of the batch above before agx_sw_batch_cigars returns.
 * The host's check of one CIGAR under the literal two-piece cost: 1 if the n_ops operations are
 * well-formed runs (I, D, =, X; positive lengths; no two equal neighbours), consume exactly x[0..ca) and y[0..cb), every '=' / 'X'
 * is true of the symbols and the total is `score`; else 0 (also for a NULL argument that is needed). */
int agx_sw_cigar_rescore_dual(const agx_sw_scoring_dual *scoring, const uint32_t *ops, uint64_t n_ops, const uint8_t *x, uint32_t ca,
                              const uint8_t *y, uint32_t cb, int32_t score);

/* Host only, no device.  How the traced fill of a span starts inside a banded batch's resident image.  The image holds the
 * query a behind `fpad` bytes and the rows b[row0 .. row0 + rows) behind one byte, packed for a fill from row0 in the band
 * dlo .. dhi COUNTED FROM row0 (j - (i - row0)) on `lanes` lanes per pair.  For a hit with a non-empty span on both sides the
 * record says where the fill of that span reads: */
typedef struct agx_sw_band_span {
    uint32_t ca, cb;   /* the span: columns (query symbols), rows (target symbols) */
    uint32_t x_bytes;  /* bytes in front of a[a_begin] behind the image's query: fpad + a_begin */
    uint32_t y_dwords; /* whole dwords the target's offset moves on by: (s - phase) / 4, s = b_begin - row0 */
    uint32_t phase;    /* s mod 4: the fill runs its step counter as t - phase, and b[b_begin] is byte 1 + phase behind the moved offset */
    int32_t dlo, dhi;  /* the band in span coordinates: both limits moved by s - a_begin, the width unchanged */
    uint32_t steps;    /* cb + lanes + phase */
} agx_sw_band_span;
/* AGX_E_ARG (nothing written) if a side of the span is empty, the span does not lie in the image (a_end >= la, b_begin < row0,
 * b_end >= row0 + rows), lanes is outside 1..64, or its begin or end cell is outside the band. */
int agx_sw_band_span_record(uint32_t la, uint32_t rows, uint32_t row0, uint32_t fpad, int32_t dlo, int32_t dhi, int32_t lanes,
                            const agx_sw_hit *hit, agx_sw_band_span *out);

/* One-shot: create + launch + scores + destroy. */
int agx_sw_score(agx_ctx *ctx, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                 int32_t *scores);
/* Same, sharded by cells over `n_devices` devices (<= 0: all visible), one host
 * thread and context per device, no collective.  The per-device contexts and
 * their memory pools are created on first use and kept for later calls. */
int agx_sw_score_multi(int n_devices, const uint8_t *bases, const uint64_t *off, const uint32_t *len,
                       int64_t n_pairs, int32_t *scores);
/* Same with an explicit device list: shard k runs on devices[k].  An ordinal may appear several times
 * (several shards then share that GPU, each with its own context and stream).  Callable from several host
 * threads at once: calls take turns on each (device, shard slot) context. */
int agx_sw_score_devices(const int *devices, int n_devices, const uint8_t *bases, const uint64_t *off, const uint32_t *len,
                         int64_t n_pairs, int32_t *scores);
/* The cut rule of the two calls above, on the host alone: cut[0..n_shards] with shard k = pairs
 * [cut[k], cut[k+1]), contiguous and balanced by sum(len_a * len_b + 1). */
int agx_sw_shard_cuts(const uint32_t *len, int64_t n_pairs, int n_shards, int64_t *cut);

/* ------------------------------------------------------------------ PairHMM */

/*
 * Input layout (host memory), mirroring the reference's regions ("batches",
 * antidiagsPairHMM.c:371-461): read r has length read_off[r+1]-read_off[r]
 * and five byte tracks at that offset (bases, base/insertion/deletion/gcp
 * qualities, Phred+33 characters exactly as in the text file); haplotype h is
 * hap_bases[hap_off[h] .. hap_off[h+1]).  Region g pairs reads
 * [region_read[g], region_read[g+1]) with haplotypes
 * [region_hap[g], region_hap[g+1]).  Results are written region by region,
 * read-major, haplotype-minor -- the order of the reference's output file.
 */
typedef struct agx_phmm_desc {
    const uint8_t *read_bases, *q_base, *q_ins, *q_del, *q_gcp;
    const uint64_t *read_off; /* n_reads + 1 */
    uint32_t n_reads;
    const uint8_t *hap_bases;
    const uint64_t *hap_off; /* n_haps + 1 */
    uint32_t n_haps;
    const uint32_t *region_read; /* n_regions + 1 */
    const uint32_t *region_hap;  /* n_regions + 1 */
    uint32_t n_regions;
} agx_phmm_desc;

/* Arithmetic of the recurrence. */
#define AGX_PHMM_F64 0      /* double, reference expression order, no FMA contraction:
                               the raw sum is bit-identical to pairHMMmatrix.c */
#define AGX_PHMM_F64_FMA 1  /* double with FMA contraction (<= 1e-12 relative on log10) */
#define AGX_PHMM_F32 2      /* float with initial constant FLT_MAX/16 (BASELINE config 3);
                               pairs whose float sum falls below AGX_PHMM_F32_RESCUE are
                               recomputed with AGX_PHMM_F64 on the device */
#define AGX_PHMM_F32_FMA 3  /* float, two haplotypes per lane group on packed FMA instructions: the fastest
                               mode; <= 1e-6 relative on log10 like AGX_PHMM_F32 but not bit-identical to a
                               plain float evaluation; same double rescue of underflowing pairs */
#define AGX_PHMM_F32_RESCUE 1e-28f
/* OR-able into `precision` (8f n4, default off): mismatch prior Qr/3 as GATK's PairHMM uses, instead
 * of the reference's Qr (antidiagsPairHMM.c:111-113).  Not a behaviour of the
 * reference: checked against the oracle's own restatement only. */
#define AGX_PHMM_GATK_PRIOR 0x100

typedef struct agx_phmm_batch agx_phmm_batch;

typedef struct agx_phmm_info {
    int64_t n_pairs;
    int64_t cells;        /* sum R*H */
    int64_t padded_cells; /* lane-steps x columns issued */
    int64_t input_bytes;
    int32_t n_launches;
    int32_t n_waves;
    int64_t n_rescued;    /* F32 only: pairs recomputed in double by the last launch+results */
} agx_phmm_info;

/* ctx may be NULL: plan only, as for agx_sw_batch_create. */
int agx_phmm_batch_create(agx_ctx *ctx, const agx_phmm_desc *d, int precision, agx_phmm_batch **out);
int agx_phmm_batch_launch(agx_phmm_batch *b);
/* log10_lik[k] = log10(sum_k) - log10(C), C = DBL_MAX/16 (FLT_MAX/16 for F32), both log10 taken by the
 * host libm in double exactly as antidiagsPairHMM.c:242; raw_sum (may be NULL) receives sum_k. */
int agx_phmm_batch_results(agx_phmm_batch *b, double *log10_lik, double *raw_sum);
/* Optional, the PairHMM counterpart of agx_sw_batch_bind_scores: name the page-locked array (agx_host_alloc, n_pairs
 * doubles) the log10 likelihoods are wanted in BEFORE launching.  An AGX_PHMM_F32_FMA batch in output order (one read and
 * haplotype length throughout, every pair with work) then lets its fill compute log10(sum) - log10(C) and write it there
 * itself -- no log10 kernel behind the fill -- and agx_phmm_batch_results(b, the same pointer, NULL) only waits, unless a
 * pair went to the double rescue plan.  Other batches keep the usual path; NULL unbinds. */
int agx_phmm_batch_bind_results(agx_phmm_batch *b, double *log10_lik);
int agx_phmm_batch_info(const agx_phmm_batch *b, agx_phmm_info *info);
void agx_phmm_batch_destroy(agx_phmm_batch *b);

int agx_phmm_forward(agx_ctx *ctx, const agx_phmm_desc *d, int precision, double *log10_lik);
int agx_phmm_forward_multi(int n_devices, const agx_phmm_desc *d, int precision, double *log10_lik);
/* Explicit device list, as agx_sw_score_devices. */
int agx_phmm_forward_devices(const int *devices, int n_devices, const agx_phmm_desc *d, int precision, double *log10_lik);
/* The cut rule: cut[0..n_shards] in REGIONS (whole regions stay together), balanced by
 * (read bytes x haplotype bytes + 1) per region. */
int agx_phmm_shard_cuts(const agx_phmm_desc *d, int n_shards, uint32_t *cut);

/*
 * The reference's only function-level seam, same argument list as
 * antidiagsPairHMM.c:120 (M/X/Y scratch is accepted and ignored; *likelihood is
 * overwritten with the log10 value, i.e. started from 0 -- SURVEY.md Q8).
 * Qr/Qi/Qd/Qg are probabilities, not Phred characters.  Runs one pair on
 * device 0 through a process-wide lazily created context; returns nothing, as
 * the reference does: on failure *likelihood = NaN and agx_last_error() is set.
 * Callable from several host threads at once: calls take turns with each other
 * and with the shards of agx_*_devices / agx_*_multi on (device 0, slot 0),
 * whose context this is.
 */
void agx_pairHMM(double *likelihood, double *M, double *X, double *Y, char *R, char *H, int read_len,
                 int haplotype_len, double *Qr, double *Qi, double *Qd, double *Qg);

/* ------------------------------------------------------------- text front end */

/*
 * Readers for the reference's two input formats, producing the flat layouts
 * above (n1 in SURVEY.md 8f).  They follow the reference's reading rules,
 * including its quirks: SW header = number of sequence LINES, fgets with a
 * 1000-byte buffer (longer lines split), newline kept as a symbol, loop ends
 * at the first missing line (antidiagonalSmithWaterman.c:201-227); PairHMM
 * read length = (strlen(line)-4)/5 (antidiagsPairHMM.c:418).
 */
typedef struct agx_sw_text {
    int32_t line_num;   /* header value as atoi() reads it */
    int64_t n_pairs;    /* pairs the reference loop would score */
    uint8_t *bases;
    uint64_t *off;      /* 2*n_pairs */
    uint32_t *len;      /* 2*n_pairs */
    char *dangling;     /* first line of an unpaired trailing pair (the reference echoes it, :225) or NULL */
} agx_sw_text;

int agx_sw_text_read(const char *path, int line_buf /* 0 = reference's 1000 */, agx_sw_text **out);
void agx_sw_text_free(agx_sw_text *t);

/* The same reader in pieces, so a host can score one chunk while the next is being parsed
 * (host/antidiagonalSmithWaterman.c does).  open reads the header; every next() returns a fresh
 * agx_sw_text object, which the caller frees, with up to max_pairs further pairs -- offsets relative to that
 * chunk's bases -- and `dangling` on the chunk that met an unpaired last line; done() turns 1 once
 * the reference's loop would have ended (header count reached or input exhausted). */
typedef struct agx_sw_reader agx_sw_reader;
int agx_sw_reader_open(const char *path, int line_buf, agx_sw_reader **out);
int32_t agx_sw_reader_line_num(const agx_sw_reader *r);
/* how many host threads read and scan a chunk of a regular file (default 0 = the library's thread pool; 1 = the
 * calling thread alone) */
void agx_sw_reader_set_threads(agx_sw_reader *r, int n_threads);
int agx_sw_reader_next(agx_sw_reader *r, int64_t max_pairs, agx_sw_text **out);
int agx_sw_reader_done(const agx_sw_reader *r);
void agx_sw_reader_close(agx_sw_reader *r);

typedef struct agx_phmm_text {
    agx_phmm_desc desc; /* points into storage owned by this object */
    int64_t n_pairs;
    int32_t n_regions_seen; /* header lines read, for the "#batch:" chatter */
    int32_t truncated;      /* 1 = a region ended early, 2 = a header with a negative haplotype count: the reference exits
                             * with failure there ("Error reading haplotypes." / "Memory allocation failed for haplotypes array") */
} agx_phmm_text;

int agx_phmm_text_read(const char *path, agx_phmm_text **out);
void agx_phmm_text_free(agx_phmm_text *t);

/* The same reader in pieces of whole regions -- the reference's batch loop, antidiagsPairHMM.c:371-433,484-489 --
 * so a host can have region k+1 parsed while region k is on the device and region k-1 is printed
 * (host/antidiagsPairHMM.c does).  Every next() returns a fresh agx_phmm_text, which the caller frees, holding the
 * regions up to the first one that brings it to max_pairs pairs (at least one region; indices and offsets
 * relative to the chunk); n_regions_seen counts the header lines read for it and `truncated` marks the chunk
 * that met a region cut short (the reader is done then, as the reference exits there). */
typedef struct agx_phmm_reader agx_phmm_reader;
int agx_phmm_reader_open(const char *path, agx_phmm_reader **out);
int agx_phmm_reader_next(agx_phmm_reader *r, int64_t max_pairs, agx_phmm_text **out);
int agx_phmm_reader_done(const agx_phmm_reader *r);
void agx_phmm_reader_close(agx_phmm_reader *r);

#ifdef __cplusplus
}
#endif
#endif /* AGX_H */
