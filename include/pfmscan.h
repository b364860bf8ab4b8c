/*
 * pfmscan.h -- C ABI of libpfmscan: MI355X (gfx950) sliding-window PFM scanner.
 *
 * This is the drop-in boundary for rnascan's per-position log-odds scoring
 * path.  Every entry point names the reference interface it replaces (paths
 * are relative to the upstream morrislab/rnascan checkout, v0.10.2).  Plain
 * pointers and sizes only; no C++ or torch types.  Loaded with ctypes
 * (rnascan_amd/_lib.py); INTEGRATION.md shows the stub a reference maintainer
 * would add.
 *
 * Conventions
 *   - every function returns a status (0 = PFMSCAN_OK, negative = error class);
 *     the message is read with pfmscan_last_error().  Foreign letters are never
 *     an error: they score NaN, as `ok = 0` does in _pwm.c:61-66.
 *   - the caller owns every buffer it passes; the library never frees caller
 *     memory and never returns memory the caller must free.  Device scratch is
 *     owned by the ctx, PSSM tables by the motif object.
 *   - a ctx is bound to one device and may be used by one host thread at a
 *     time; use one ctx per device / per thread.  No global mutable state: the
 *     host-only entry points (FASTA / profile text / TSV, no ctx) may be called
 *     from any number of threads, their message (pfmscan_last_error(NULL)) is
 *     thread-local.
 *   - a `_dev` entry point works on the `stream` it is given: its memsets,
 *     table uploads, count read-backs and helper kernels are issued there.
 *     A ctx's device scratch and a library's threshold table are per-call
 *     state, not per-stream state: calls on one ctx or one library must be
 *     issued in ONE stream order, or be ordered by the caller (an event
 *     between the streams).  Two streams that run calls of the same ctx side
 *     by side share its scratch.
 *   - positions are 0-based at this level; rnascan's 1-based inclusive
 *     Start/End (rnascan.py:264-271, :311) are made in the table layer.
 *
 * The packed record stream
 *   Records are concatenated into one stream of n_pos positions; every record
 *   is followed by exactly ONE separator position whose code is PFMSCAN_SEP.
 *     codes    uint8 [n_pos]      letter index 0..6, or PFMSCAN_SEP (7) for a
 *                                 separator or any letter outside the alphabet.
 *                                 Generic-alphabet scans (pfmscan_scan_letters_f64_*,
 *                                 pfmscan_hits_letters_f64_*, the second stream of
 *                                 pfmscan_hits_pair_*) read bits 0..2 only: the host may keep
 *                                 the letter's CASE in bit 3 (structure strings are reported as
 *                                 written, rnascan.py:186-197, :272)
 *     profile  float/double [n_pos][7] row-major averaged-structure profile
 *                                 (rnascan.py:296-297 after `del struct['PO']`),
 *                                 columns already paired with the PSSM's; the
 *                                 separator row may hold anything finite
 *   A window is named by the stream position of its first letter.  Windows that
 *   touch a separator (i.e. would cross a record end) or the end of the stream
 *   get a NaN sequence score, so they can never be hits; out arrays are
 *   position-aligned (length n_pos), record r's windows are
 *   [off_r, off_r + L_r - m + 1).  Base pointers must be 16-byte aligned.
 */
#ifndef PFMSCAN_H
#define PFMSCAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFMSCAN_ABI_VERSION 27   /* 27: pfmscan_expect_pair_joint_dev / _staged / _merged_staged (the 4 x 7 table per column); the posterior
                                  * site map (pfmscan_footprint_*), the table on averaged-structure profiles (pfmscan_expect_profile_joint_*)
                                  * and the threshold-free mutagenesis (pfmscan_mutocc_*) only ADD entry points and keep the number, which
                                  * the suite pins at 27 */
#define PFMSCAN_NCODE   8      /* columns of a letter table */
#define PFMSCAN_SEP     7      /* separator / foreign-letter code */
#define PFMSCAN_NSTRUCT 7      /* columns of a structure profile / structure PSSM */
#define PFMSCAN_MAX_M   64     /* widest PFM of the tuned kernels and of PFM libraries (pfmscan_library_create) */
#define PFMSCAN_MAX_WIDTH 4096 /* widest PFM accepted by pfmscan_motif_create / pfmscan_pwm_calculate: the reference's loops take
                                  any width (_pwm.c:34-68, rnascan.py:302-307).  Above PFMSCAN_MAX_M: letters-only scans run a
                                  slab-tiled kernel (the table through LDS 64 rows at a time), scans with a structure part the
                                  profile kernel up to 180 rows and a plain one-thread-per-window kernel beyond -- same results */
#define PFMSCAN_SITE_GROUP 4096 /* most hits of one group of the site profiles (pfmscan_site_groups) */
#define PFMSCAN_SITE_LIMBS 66   /* 64-bit limbs of one cell of a long accumulator (pfmscan_site_sums_lib_*) */
#define PFMSCAN_SITE_JOINT_COLS 64 /* columns of one LDS tile of the letter-pair counts (pfmscan_site_joint_*) */

#define PFMSCAN_OK          0
#define PFMSCAN_E_BADARG   -1  /* NULL / negative / inconsistent argument   -> ValueError */
#define PFMSCAN_E_BADSHAPE -2  /* width out of range, misaligned pointer     -> ValueError (_pwm.c:96-113) */
#define PFMSCAN_E_OOM      -3  /* host or device allocation failed           -> MemoryError (_pwm.c:27-31) */
#define PFMSCAN_E_HIP      -4  /* HIP runtime error (message has the detail) -> RuntimeError */
#define PFMSCAN_E_CAPACITY -5  /* hit buffer too small; *n_hits = required   -> retry */

#define PFMSCAN_PROFILE_NONE 0
#define PFMSCAN_PROFILE_F32  1
#define PFMSCAN_PROFILE_F64  2

typedef struct pfmscan_ctx pfmscan_ctx;
typedef struct pfmscan_motif pfmscan_motif;

int pfmscan_abi_version(void);

/* Context bound to HIP device `device` (>= 0).  Fails with PFMSCAN_E_HIP when no
 * gfx950 device is visible -- there is no CPU fallback behind this ABI. */
int pfmscan_ctx_create(int device, pfmscan_ctx **out);
void pfmscan_ctx_destroy(pfmscan_ctx *ctx);
/* Last error text of `ctx`; ctx == NULL reads the calling thread's last
 * ctx-less error (a failed pfmscan_ctx_create).  Never NULL. */
const char *pfmscan_last_error(const pfmscan_ctx *ctx);
int pfmscan_device_info(const pfmscan_ctx *ctx, int *n_cu, int64_t *hbm_bytes,
                        char *name, int name_cap);
int pfmscan_synchronize(pfmscan_ctx *ctx);

/* ---- PSSM operands -------------------------------------------------------
 * Replaces the per-call list-of-lists -> ndarray conversion of
 * ExtendedPositionSpecificScoringMatrix._calculate (matrix.py:57-60) and the
 * `pm = pd.DataFrame(pm)` of scan_averaged_structure (rnascan.py:298-300):
 * the tables are uploaded once.
 *   letter_table  double [m][8] or NULL: log-odds per letter code; every column
 *                 that is not a letter of the alphabet (always column 7) must be
 *                 NaN.  RNA: columns A,C,G,U = sorted(alphabet.letters)
 *                 (matrix.py:57), i.e. the column order of _pwm.c:45-60.
 *   struct_pssm   double [m][7] or NULL: log-odds for the 7 profile columns,
 *                 paired with the profile's column order by the caller.
 * At least one must be given; both share the width m (rnascan.py:422-423 joins
 * on Start AND End, so unequal widths can never produce a combined hit). */
int pfmscan_motif_create(pfmscan_ctx *ctx, const double *letter_table,
                         const double *struct_pssm, int m, pfmscan_motif **out);
void pfmscan_motif_destroy(pfmscan_motif *motif);

/* ---- (iii) of SURVEY 8b: the reference's native entry point ----------------
 * Replaces `_pwm.calculate(sequence, matrix)` (_pwm.c:72-121, loop :34-68):
 * ASCII sequence of length s (A/a C/c G/g T/t/U/u; anything else poisons the
 * windows covering it), matrix double [m][4] in A,C,G,U column order ->
 * out float [s-m+1] = (float)(fp64 sequential sum).  s < m writes nothing.
 * Host buffers; runs on the ctx's device. */
int pfmscan_pwm_calculate(pfmscan_ctx *ctx, const char *sequence, int64_t s,
                          const double *matrix, int64_t m, float *out);

/* ---- all-scores over a packed stream, device-resident ----------------------
 * Replaces the window loops of `pssm.search` -> `calculate` (rnascan.py:263,
 * matrix.py:68-81, _pwm.c:34-68) and of scan_averaged_structure
 * (rnascan.py:302-307) for every record of the stream in one pass.
 *   d_codes / d_profile / d_out_* are DEVICE pointers (hipMalloc or torch).
 *   d_out_seq    float  [n_pos] or NULL: (float)(fp64 sequential sum), NaN for
 *                windows covering a foreign letter / separator / stream end
 *   d_out_struct double [n_pos] or NULL: sum_j nan_to_num(dot(profile[p+j], pssm[j]))
 *                in fp64 (rnascan.py:306); NaN for p + m > n_pos
 *   stream       hipStream_t, NULL = the ctx's own stream.  Asynchronous. */
int pfmscan_scan_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                     const uint8_t *d_codes, const void *d_profile,
                     int profile_dtype, int64_t n_pos, float *d_out_seq,
                     double *d_out_struct, void *stream);

/* Generic-alphabet letter scan with fp64 output: replaces
 * ExtendedPositionSpecificScoringMatrix._py_calculate (matrix.py:25-43), which
 * keeps Python floats (no float32 cast) and gives NaN on an unknown letter. */
int pfmscan_scan_letters_f64_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                                 const uint8_t *d_codes, int64_t n_pos,
                                 double *d_out, void *stream);

/* ---- thresholded hits over a packed stream, device-resident ----------------
 * Replaces `score > threshold` of pssm.search (rnascan.py:263; strict, NaN and
 * -inf never pass), `if score > minscore` (rnascan.py:310) and, when the motif
 * has both parts, the inner join of combine() (rnascan.py:422-423):
 *   hit  <=>  (no letter table  or seq(p)    > thr_seq)
 *         and (no struct pssm   or struct(p) > thr_struct)
 * The structure compare is taken on the value the reference's arithmetic gives (rnascan.py:306: every product and
 * every addition rounded, k ascending): a window whose fast score lies within 24 m 2^-53 1024 sum|pssm| of thr_struct
 * is scored again in that order before the compare, and that score is reported (this holds for profile entries up to
 * 1024 in magnitude; they are probabilities).  The same in every hits entry point of this header.
 * Hits are appended in no particular order:
 *   d_hit_pos int64 [capacity], d_hit_seq float [capacity] (or NULL),
 *   d_hit_struct double [capacity] (or NULL), d_hit_count: one uint64 the
 *   caller zeroes before the call; afterwards it holds the TOTAL number of
 *   hits, which may exceed capacity (only the first `capacity` are stored). */
int pfmscan_hits_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                     const uint8_t *d_codes, const void *d_profile,
                     int profile_dtype, int64_t n_pos, double thr_seq,
                     double thr_struct, int64_t capacity, int64_t *d_hit_pos,
                     float *d_hit_seq, double *d_hit_struct,
                     uint64_t *d_hit_count, void *stream);

/* Same contract and arguments as pfmscan_hits_dev, but SYNCHRONISES `stream` and may take
 * two passes: when the motif has both parts and thr_seq is finite, the letters kernel
 * (1 byte per position) runs over everything and the structure score is computed only at
 * its hits (k_struct_at), because a combined hit needs BOTH thresholds (rnascan.py:422-433)
 * and the letter side is selective at real thresholds.  Falls back to the fused pass when
 * more than 1/32 of the windows pass the letter threshold.  Same hits, same scores. */
int pfmscan_hits_adaptive_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                              const uint8_t *d_codes, const void *d_profile,
                              int profile_dtype, int64_t n_pos, double thr_seq,
                              double thr_struct, int64_t capacity, int64_t *d_hit_pos,
                              float *d_hit_seq, double *d_hit_struct,
                              uint64_t *d_hit_count, void *stream);

/* ---- host-buffer forms ------------------------------------------------------
 * Same contracts with HOST pointers: the ctx stages H2D into its own device
 * scratch, launches, copies back and synchronises. */
int pfmscan_scan_host(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                      const uint8_t *codes, const void *profile,
                      int profile_dtype, int64_t n_pos, float *out_seq,
                      double *out_struct);
int pfmscan_scan_letters_f64_host(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                                  const uint8_t *codes, int64_t n_pos, double *out);
/* Hits come back sorted by position.  PFMSCAN_E_CAPACITY: *n_hits holds a capacity
 * that suffices (>= the number of hits), nothing was written to the hit arrays. */
int pfmscan_hits_host(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                      const uint8_t *codes, const void *profile,
                      int profile_dtype, int64_t n_pos, double thr_seq,
                      double thr_struct, int64_t capacity, int64_t *hit_pos,
                      float *hit_seq, double *hit_struct, int64_t *n_hits);

/* Hits of a host-resident stream of ANY length with bounded device scratch (a memory-mapped packed
 * profile store is handed over as is; replaces the per-record `pd.read_table` + scan of rnascan.py:296-310 and the
 * file fan-out of :351-366).  The stream is cut into chunks of chunk_positions (0 = 2^24) positions; the upload of
 * chunk k+1 (copy stream) runs beside the scan of chunk k (two alternating device buffers), every chunk is one fused
 * hits launch, hits come back sorted by stream position.  Same results and same capacity protocol as
 * pfmscan_hits_host; nothing stays staged afterwards. */
int pfmscan_hits_pipeline_host(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                               const uint8_t *codes, const void *profile,
                               int profile_dtype, int64_t n_pos, int64_t chunk_positions,
                               double thr_seq, double thr_struct, int64_t capacity,
                               int64_t *hit_pos, float *hit_seq, double *hit_struct,
                               int64_t *n_hits);

/* ---- staged stream: upload once, scan with many motifs ------------------------
 * (multi-PFM libraries, SURVEY 8f N1: the reference reloads and rescans everything
 * per PFM file).  pfmscan_stage copies a packed stream into the ctx's device scratch
 * and keeps it there; the *_staged calls run one motif over it without any H2D.
 * codes / profile may be NULL when no motif that will be used needs them.  The host
 * forms above are exactly stage + *_staged. */
int pfmscan_stage(pfmscan_ctx *ctx, const uint8_t *codes, const void *profile,
                  int profile_dtype, int64_t n_pos);
/* positions of the stream staged in `ctx` (what pfmscan_scan_staged writes per output array), -1 when nothing is
 * staged.  pfmscan_scan_host / pfmscan_hits_host / pfmscan_pwm_calculate / the pipeline restage or unstage: size the
 * out arrays from THIS, not from what was passed to an earlier pfmscan_stage. */
int64_t pfmscan_staged_positions(const pfmscan_ctx *ctx);
int pfmscan_scan_staged(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                        float *out_seq, double *out_struct);
int pfmscan_hits_staged(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                        double thr_seq, double thr_struct, int64_t capacity,
                        int64_t *hit_pos, float *hit_seq, double *hit_struct,
                        int64_t *n_hits);

/* ---- combined hits with a joint threshold on LogOdds.SeqStruct -----------------------------------
 * combine() (rnascan.py:416-434) ends the combined table with LogOdds.SeqStruct = LogOdds.Seq + LogOdds.Struct, the sum
 * of the two PRINTED columns, but only ever filters on each side alone (the two tables it joins were thresholded
 * separately).  These entry points add the joint filter.  The motif must have BOTH parts (else PFMSCAN_E_BADARG):
 *   hit <=> seq(p) > thr_seq  and  struct(p) > thr_struct                       (as pfmscan_hits_*; either may be -inf)
 *           and  (double)round3(seq(p)) + struct(p) > thr_sum                   (strict; a NaN sum never passes)
 * with round3(x) = np.round(float32 x, 3) = rint(x * 1000f) / 1000f in IEEE float32 -- the printed LogOdds.Seq
 * (rnascan.py:273) -- and one rounded fp64 addition: exactly the printed LogOdds.SeqStruct of an averaged-structure scan.
 * A window whose sum lies within a rigorous band of thr_sum is decided on -- and reports -- the structure score taken in
 * the reference's rounded order, as near thr_struct (csrc/pfmscan_exact.hpp).  thr_sum = -inf gives exactly the hits of
 * the plain call; NaN is PFMSCAN_E_BADARG.  Hit arrays, count, capacity protocol and ordering: as the pfmscan_hits_*
 * counterpart.  _dev is ONE fused pass, asynchronous on `stream`, and never synchronises; _staged / _host take the
 * candidate-then-verify route of pfmscan_hits_staged when thr_seq is finite and selective (the joint filter then runs
 * in the verify pass); _pipeline_host is one fused pass per chunk. */
int pfmscan_hits_sum_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                         const uint8_t *d_codes, const void *d_profile,
                         int profile_dtype, int64_t n_pos, double thr_seq,
                         double thr_struct, double thr_sum, int64_t capacity, int64_t *d_hit_pos,
                         float *d_hit_seq, double *d_hit_struct,
                         uint64_t *d_hit_count, void *stream);
int pfmscan_hits_sum_staged(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                            double thr_seq, double thr_struct, double thr_sum, int64_t capacity,
                            int64_t *hit_pos, float *hit_seq, double *hit_struct,
                            int64_t *n_hits);
int pfmscan_hits_sum_host(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                          const uint8_t *codes, const void *profile,
                          int profile_dtype, int64_t n_pos, double thr_seq,
                          double thr_struct, double thr_sum, int64_t capacity, int64_t *hit_pos,
                          float *hit_seq, double *hit_struct, int64_t *n_hits);
int pfmscan_hits_sum_pipeline_host(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                                   const uint8_t *codes, const void *profile,
                                   int profile_dtype, int64_t n_pos, int64_t chunk_positions,
                                   double thr_seq, double thr_struct, double thr_sum, int64_t capacity,
                                   int64_t *hit_pos, float *hit_seq, double *hit_struct,
                                   int64_t *n_hits);

/* ---- thresholded hits of a generic-alphabet letter scan, score in fp64 -------------------------
 * (`rnascan -q pfm structs.fa`.)  Replaces `pm.search(seq, threshold=minscore)` (rnascan.py:263) over
 * ExtendedPositionSpecificScoringMatrix._py_calculate (matrix.py:25-43) for an alphabet that is not a nucleotide
 * alphabet: the score is the sequential fp64 sum (Python floats, NO float32 cast), an unknown letter makes the window
 * NaN, hit <=> score > thr (strict: NaN and -inf never pass, not even at thr = -inf).  Letters-only motif, up to 7
 * letters (codes 0..6).  Finite thresholds and widths up to 32 run an integer prefilter with one-sided rounding
 * (k_letters_cred8) and the exact sum for its survivors; otherwise every window gets the exact sum.
 *   d_hit_pos int64 [capacity], d_hit_score double [capacity]; d_hit_count: one uint64 the caller zeroes, afterwards
 *   the TOTAL number of hits (only the first `capacity` are stored).  Hits in no particular order; asynchronous. */
int pfmscan_hits_letters_f64_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                                 const uint8_t *d_codes, int64_t n_pos, double thr,
                                 int64_t capacity, int64_t *d_hit_pos, double *d_hit_score,
                                 uint64_t *d_hit_count, void *stream);
/* Staged (pfmscan_stage with codes) and host-buffer forms: hits sorted by position, capacity protocol of
 * pfmscan_hits_host. */
int pfmscan_hits_letters_f64_staged(pfmscan_ctx *ctx, const pfmscan_motif *motif, double thr,
                                    int64_t capacity, int64_t *hit_pos, double *hit_score,
                                    int64_t *n_hits);
int pfmscan_hits_letters_f64_host(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                                  const uint8_t *codes, int64_t n_pos, double thr,
                                  int64_t capacity, int64_t *hit_pos, double *hit_score,
                                  int64_t *n_hits);

/* ---- two code streams: sequence letters AND structure letters in one call --------------------
 * (`rnascan -p pfm -q pfm seqs.fa structs.fa`, rnascan.py:119-123.)  Replaces the two scan_main passes and the
 * inner join of combine() (rnascan.py:416-434): codes = the RNA stream scored by motif_seq as in pfmscan_hits_dev
 * (float32 of the fp64 sum, _pwm.c:34-68), codes2 = the structure letters of the SAME records in the same layout
 * (same offsets, separators at the same positions) scored by motif_struct as in pfmscan_hits_letters_f64_dev.
 *   hit <=> seq(p) > thr_seq and struct(p) > thr_struct            (both strict)
 * Both motifs are letters-only and share the width m (the join is on Start AND End).  For a finite, selective thr_seq on a
 * PFM up to 32 wide this is ONE launch: the integer-prefiltered letters kernel scores the structure letters of its own
 * survivors (k_letters_cred<.., PAIR>).  Otherwise the sequence letters pass runs over everything and the structure
 * letters are read at its hits only (k_letters_at), which synchronises `stream` in between.
 * Hit arrays and count as in pfmscan_hits_dev (d_hit_struct = the fp64 structure score). */
int pfmscan_hits_pair_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif_seq,
                          const pfmscan_motif *motif_struct, const uint8_t *d_codes,
                          const uint8_t *d_codes2, int64_t n_pos, double thr_seq,
                          double thr_struct, int64_t capacity, int64_t *d_hit_pos,
                          float *d_hit_seq, double *d_hit_struct, uint64_t *d_hit_count,
                          void *stream);
/* A second code stream beside the one staged by pfmscan_stage (same n_pos); forgotten by the next pfmscan_stage. */
int pfmscan_stage_codes2(pfmscan_ctx *ctx, const uint8_t *codes2, int64_t n_pos);
int pfmscan_hits_pair_staged(pfmscan_ctx *ctx, const pfmscan_motif *motif_seq,
                             const pfmscan_motif *motif_struct, double thr_seq, double thr_struct,
                             int64_t capacity, int64_t *hit_pos, float *hit_seq,
                             double *hit_struct, int64_t *n_hits);
int pfmscan_hits_pair_host(pfmscan_ctx *ctx, const pfmscan_motif *motif_seq,
                           const pfmscan_motif *motif_struct, const uint8_t *codes,
                           const uint8_t *codes2, int64_t n_pos, double thr_seq, double thr_struct,
                           int64_t capacity, int64_t *hit_pos, float *hit_seq, double *hit_struct,
                           int64_t *n_hits);

/* ---- two code streams with a joint threshold on the printed LogOdds.SeqStruct -----------------
 * (`rnascan -p pfm -q pfm seqs.fa structs.fa --min-seqstruct T`.)  In this mode BOTH printed columns are rounded to three
 * places before combine() adds them (rnascan.py:273, :416-434): LogOdds.Seq is np.round of a float32, LogOdds.Struct is
 * Python's round(x, 3) of a double.  Arguments of pfmscan_hits_pair_* plus thr_sum:
 *   hit <=> seq(p) > thr_seq  and  struct(p) > thr_struct                      (as pfmscan_hits_pair_*; either may be -inf;
 *                                                                               NaN and -inf scores never pass)
 *           and  (double) round3(seq(p)) + round3d(struct(p))  >  thr_sum      (strict; one rounded fp64 addition)
 * with round3 as in pfmscan_hits_sum_* and round3d(x) = round(x, 3) of a double, bit for bit what pfmscan_round_decimals
 * gives (csrc/pfmscan_exact.hpp).  The reported scores are the unrounded ones, as from pfmscan_hits_pair_*.  thr_sum = -inf
 * gives exactly the hits of the plain call; NaN is PFMSCAN_E_BADARG.
 * Where it is decided (rnascan.py:273, :416-434):  a finite thr_seq takes the routes of pfmscan_hits_pair_dev with the
 * predicate in the exact stage (k_letters_cred<.., PAIR, SUM>: one launch, no synchronisation; else a letters pass and
 * k_letters_at<SUM>, which synchronises `stream` in between, exactly where pfmscan_hits_pair_dev may).  thr_seq = -inf with a
 * finite thr_sum is ONE asynchronous launch: for widths up to 32 an integer prefilter adds the credits of BOTH streams into one
 * 16-bit sum with the joint threshold folded in and only its survivors get the two exact sums (k_pair_cred_sum); wider PFMs,
 * tables with a +inf cell and thresholds that more than 1/32 of the windows would survive take both exact letter sums of every
 * window (k_pair_sum_dense).  A finite thr_seq too dense for the sequence credits alone tries the joint credits before the two launches.
 * Hit arrays, count, capacity protocol and ordering: as the pfmscan_hits_pair_* counterpart. */
int pfmscan_hits_pair_sum_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif_seq,
                              const pfmscan_motif *motif_struct, const uint8_t *d_codes,
                              const uint8_t *d_codes2, int64_t n_pos, double thr_seq,
                              double thr_struct, double thr_sum, int64_t capacity,
                              int64_t *d_hit_pos, float *d_hit_seq, double *d_hit_struct,
                              uint64_t *d_hit_count, void *stream);
int pfmscan_hits_pair_sum_staged(pfmscan_ctx *ctx, const pfmscan_motif *motif_seq,
                                 const pfmscan_motif *motif_struct, double thr_seq,
                                 double thr_struct, double thr_sum, int64_t capacity,
                                 int64_t *hit_pos, float *hit_seq, double *hit_struct,
                                 int64_t *n_hits);
int pfmscan_hits_pair_sum_host(pfmscan_ctx *ctx, const pfmscan_motif *motif_seq,
                               const pfmscan_motif *motif_struct, const uint8_t *codes,
                               const uint8_t *codes2, int64_t n_pos, double thr_seq,
                               double thr_struct, double thr_sum, int64_t capacity,
                               int64_t *hit_pos, float *hit_seq, double *hit_struct,
                               int64_t *n_hits);
/* The route the last pfmscan_hits_pair_sum_* call of this ctx took (NONE: thr_sum was -inf, or no such call yet). */
#define PFMSCAN_PAIR_ROUTE_NONE      0
#define PFMSCAN_PAIR_ROUTE_FUSED     1   /* k_letters_cred<.., PAIR, SUM>: one launch */
#define PFMSCAN_PAIR_ROUTE_TWO_PHASE 2   /* sequence letters pass, then k_letters_at<SUM> at its hits */
#define PFMSCAN_PAIR_ROUTE_DENSE     3   /* k_pair_sum_dense: both exact sums of every window */
#define PFMSCAN_PAIR_ROUTE_CREDITS   4   /* k_pair_cred_sum: one integer credit sum over both streams, exact sums for its survivors */
int pfmscan_pair_sum_route(const pfmscan_ctx *ctx);
/* Diagnostics (host only, no ctx): out[i] = round3d(in[i]) as the kernels compute it (rnascan.py:273 on a Python float);
 * and the two steps of the joint decision for n windows that passed both single thresholds: maybe[i] = the cheap superset
 * test, passes[i] = the exact predicate behind it (0 / 1), *margin0 = the constant part of the test's margin for thr_sum. */
int pfmscan_debug_round3d(const double *in, int64_t n, double *out);
/* The joint credit tables k_pair_cred_sum uses for one pair ([m][8] tables, m <= 32) and one thr_sum: credits_seq /
 * credits_struct uint16 [m][8] (the joint threshold folded into row 0 of credits_seq; "bit 15 of the sum over both clear" =>
 * the printed sum cannot exceed thr_sum), *quantum and *slack in score units (slack = 2 m quanta, one-sided), *thr_joint =
 * thr_sum minus the margin of the cheap test, *survive = the predicted share of surviving windows for uniform letters,
 * *mode 1: used; 2: dense (survive > 1/32: the exact kernel instead); 3: switched off (+inf cell, letters beyond ROUND3_SAFE,
 * non-finite quantum: quantum = slack = inf, credits 0). */
int pfmscan_debug_pair_credits(const double *letters_seq, const double *letters_struct, int m, double thr_sum,
                               uint16_t *credits_seq, uint16_t *credits_struct, double *quantum, double *slack,
                               double *thr_joint, double *survive, int *mode);
int pfmscan_debug_pair_sum_test(const float *seq, const double *st, int64_t n, double thr_sum,
                                uint8_t *maybe, uint8_t *passes, double *margin0);

/* ---- multi-PFM libraries: every motif in ONE pass (BASELINE config 5) ----------
 * The reference loads one PFM file per run (load_motif, rnascan.py:217-218), scans only the first
 * motif of its dict (rnascan.py:262) and would re-read every sequence and profile per motif,
 * although it ships a multi-PFM format (pfmutil.py:89-133).  A library object holds n motifs of one
 * width m:
 *   letter_tables  double [n][m][8], each as in pfmscan_motif_create; the alphabet must be the 4 codes
 *                  0..3 (columns 4..7 NaN) -- otherwise PFMSCAN_E_BADSHAPE, scan such motifs one by one
 *   struct_pssms   double [n][m][7] or NULL: motif k's structure PSSM, paired with letter table k
 * Hit of motif k at window p (same filter as pfmscan_hits_dev, per motif):
 *   seq_k(p) > thr_seq[k]  and  (no structure PSSMs or struct_k(p) > thr_struct[k])
 * i.e. pssm.search's strict `>` (rnascan.py:263), `score > minscore` (:310) and combine()'s inner
 * join (:422-423) for the pair (sequence motif k, structure motif k).  Scores are the same numbers the
 * single-motif entry points give (float32 of the sequential fp64 sum; fp64 per-row nan_to_num sum).
 * thr_seq / thr_struct are HOST arrays of n doubles; thr_seq must be > -inf (at -inf every window is a hit:
 * use the all-scores entry points).
 *
 * STRUCTURE-ONLY libraries: letter_tables == NULL with struct_pssms given (`rnascan -q library avgdir/`; the reference
 * would call scan_averaged_structure, rnascan.py:293-315, once per motif and re-read every profile each time).  Every
 * motif is scored in ONE pass over the profile (k_profile_lib): the tile's rows are staged in LDS once, the motifs'
 * PSSM rows stream through the scalar cache, any library size is one pass.  Hit of motif k at window p:
 * struct_k(p) > thr_struct[k] (rnascan.py:310); thr_seq and the codes are ignored (may be NULL), hit_seq comes back NaN.
 * No codes means no separators: the caller drops windows that run over a record end, as for a structure-only motif. */
typedef struct pfmscan_library pfmscan_library;
int pfmscan_library_create(pfmscan_ctx *ctx, const double *letter_tables,
                           const double *struct_pssms, int n_motifs, int m,
                           pfmscan_library **out);
void pfmscan_library_destroy(pfmscan_library *lib);
/* passes the library needs (motifs that fit the 160 KB of LDS at once), the largest one-sided slack of the
 * integer prefilter at the last thresholds in score units (NaN before the first scan, inf when a motif with
 * +inf / NaN log-odds sums runs without prefilter); any pointer may be NULL */
int pfmscan_library_info(const pfmscan_library *lib, int *n_motifs, int *m, int *n_passes,
                         int *motifs_per_pass, double *max_eps);
/* How the last scan of this library ran, through any pfmscan_library_hits* form (all three 0 before the first scan):
 * *n_launches = the scan kernel's launches (a chunked or > 2^31-position scan: over all chunks / spans),
 * *n_team_launches = those that ran several passes of a seq + struct library side by side as teams of one launch (long
 * streams only; 0 for structure-only and letter libraries), *max_teams = the most passes in one launch (1: one after the
 * other).  Host only; any pointer may be NULL. */
int pfmscan_library_last_launches(const pfmscan_library *lib, int *n_launches, int *n_team_launches,
                                  int *max_teams);
/* Device-resident form, asynchronous on `stream` WHILE THE THRESHOLDS REPEAT: a
 * call whose thresholds differ from the previous call's on this library (the
 * first call included) synchronises `stream` once before it rewrites the
 * library's threshold and credit tables -- the previous scan may still be
 * reading them -- and uploads the new ones on `stream`; the scan itself is
 * asynchronous again.  The same holds for pfmscan_library_hits_letters_dev.
 * Hits in no particular order:
 *   d_hit_pos int64 [capacity], d_hit_motif int32 [capacity] (motif index 0..n-1),
 *   d_hit_seq float [capacity] or NULL, d_hit_struct double [capacity] or NULL,
 *   d_hit_count: one uint64 (need not be zeroed); afterwards the TOTAL number of hits.  A value
 *   above capacity means the hit arrays are incomplete: call again with at least that capacity (the value
 *   is then the total or more: the hit arrays are 256 regions that must each hold their part, and hits
 *   that crowd into some of them -- the passes of a large library differ in their hit counts -- need more
 *   room than their number). */
int pfmscan_library_hits_dev(pfmscan_ctx *ctx, pfmscan_library *lib,
                             const uint8_t *d_codes, const void *d_profile,
                             int profile_dtype, int64_t n_pos, const double *thr_seq,
                             const double *thr_struct, int64_t capacity,
                             int64_t *d_hit_pos, int32_t *d_hit_motif, float *d_hit_seq,
                             double *d_hit_struct, uint64_t *d_hit_count, void *stream);
/* Staged / host-buffer forms (see pfmscan_stage): hits come back sorted by (position, motif index).
 * PFMSCAN_E_CAPACITY: *n_hits holds a capacity that suffices, nothing was written. */
int pfmscan_library_hits_staged(pfmscan_ctx *ctx, pfmscan_library *lib,
                                const double *thr_seq, const double *thr_struct,
                                int64_t capacity, int64_t *hit_pos, int32_t *hit_motif,
                                float *hit_seq, double *hit_struct, int64_t *n_hits);
int pfmscan_library_hits_host(pfmscan_ctx *ctx, pfmscan_library *lib,
                              const uint8_t *codes, const void *profile, int profile_dtype,
                              int64_t n_pos, const double *thr_seq, const double *thr_struct,
                              int64_t capacity, int64_t *hit_pos, int32_t *hit_motif,
                              float *hit_seq, double *hit_struct, int64_t *n_hits);

/* pfmscan_hits_pipeline_host for libraries: a host-resident stream of ANY length (a memory-mapped packed profile store and
 * the codes of its records: the whole of config 5's input) with bounded device scratch; chunks of chunk_positions (0 = 2^24)
 * positions, the upload of chunk k+1 beside the scan of chunk k, hits sorted by (position, motif index).  Same results and
 * capacity protocol as pfmscan_library_hits_host; nothing stays staged afterwards. */
int pfmscan_library_hits_pipeline_host(pfmscan_ctx *ctx, pfmscan_library *lib,
                                       const uint8_t *codes, const void *profile, int profile_dtype,
                                       int64_t n_pos, int64_t chunk_positions, const double *thr_seq,
                                       const double *thr_struct, int64_t capacity, int64_t *hit_pos,
                                       int32_t *hit_motif, float *hit_seq, double *hit_struct, int64_t *n_hits);

/* ---- libraries with a joint threshold on LogOdds.SeqStruct: decided in the library kernel ---------------------------------
 * The joint filter of pfmscan_hits_sum_* -- the printed LogOdds.SeqStruct of combine() (rnascan.py:416-434) -- for every
 * pair of a multi-PFM library (pfmutil.py:89-133) in ONE pass (k_library<.., SUM>).  The library must have letter tables AND
 * structure PSSMs and be scanned over profile rows (else PFMSCAN_E_BADARG).  Hit of pair k at window p <=>
 *   seq_k(p) > thr_seq[k]  and  struct_k(p) > thr_struct[k]  and  (double)round3(seq_k(p)) + struct_k(p) > thr_sum[k]
 * exactly as pfmscan_hits_sum_* decides it for pair k alone (strict; same near-band re-score, same reported scores).
 * thr_sum: HOST array of n doubles; NaN is PFMSCAN_E_BADARG; thr_sum[k] = -inf for every k runs the plain kernels and
 * returns the plain call's hits bit for bit.  thr_seq[k] MAY be -inf here: the kernel's integer prefilter is built for
 *   thr_eff[k] = max(thr_seq[k], thr_sum[k] - (an upper bound on struct_k) - rounding terms)      (csrc/pfmscan_exact.hpp),
 * a superset filter -- the exact pass still compares with thr_seq, thr_struct and thr_sum themselves.  The bound is
 * row_sum_max times the sum of the PSSM's non-negative row maxima; it holds when every profile row a scorable window touches
 * (every row not under code 7) is finite, non-negative and sums to at most row_sum_max -- what
 * pfmscan_profile_row_bound_* measures.  A motif with a +inf PSSM cell, or row_sum_max = INFINITY, is not tightened
 * (thr_eff = thr_seq); a motif whose thr_eff is -inf gives PFMSCAN_E_BADARG with pfmscan_library_hits_*'s message before
 * anything is written.
 *   _dev     takes row_sum_max from the CALLER: a promise about the rows (INFINITY promises nothing).  A false promise costs
 *            hits: windows over rows that break it may be dropped without any error.  Asynchronous under the conditions of
 *            pfmscan_library_hits_dev (the cached tables are keyed on thr_eff and thr_sum too); reads nothing home.
 *   _staged, _host  take no promise: they measure the staged stream's row bound themselves (once per staging).
 * Hit arrays, counts, ordering and the capacity protocol: as the pfmscan_library_hits_* counterpart.  There is no pipeline
 * form (the bound is needed for the whole stream before its first chunk is scanned), and letter libraries keep filtering
 * finished rows. */
int pfmscan_library_hits_sum_dev(pfmscan_ctx *ctx, pfmscan_library *lib,
                                 const uint8_t *d_codes, const void *d_profile,
                                 int profile_dtype, int64_t n_pos, const double *thr_seq,
                                 const double *thr_struct, const double *thr_sum, double row_sum_max,
                                 int64_t capacity, int64_t *d_hit_pos, int32_t *d_hit_motif,
                                 float *d_hit_seq, double *d_hit_struct, uint64_t *d_hit_count,
                                 void *stream);
int pfmscan_library_hits_sum_staged(pfmscan_ctx *ctx, pfmscan_library *lib,
                                    const double *thr_seq, const double *thr_struct,
                                    const double *thr_sum, int64_t capacity, int64_t *hit_pos,
                                    int32_t *hit_motif, float *hit_seq, double *hit_struct,
                                    int64_t *n_hits);
int pfmscan_library_hits_sum_host(pfmscan_ctx *ctx, pfmscan_library *lib,
                                  const uint8_t *codes, const void *profile, int profile_dtype,
                                  int64_t n_pos, const double *thr_seq, const double *thr_struct,
                                  const double *thr_sum, int64_t capacity, int64_t *hit_pos,
                                  int32_t *hit_motif, float *hit_seq, double *hit_struct,
                                  int64_t *n_hits);
/* The row bound of a profile stream: the largest fp64 row sum (columns 0..6 ascending, float32 rows widened first) over the
 * positions whose code (bits 0-2) is not 7 -- rows under separators and foreign letters are skipped, every window covering one
 * scores NaN on the sequence side -- or +inf when such a row holds a NaN, an infinite or a negative entry; 0 when no row
 * counts.  One defined bit pattern (a maximum does not depend on the order).  d_codes may be NULL: every row counts.
 * _dev writes one double to d_out, asynchronous on `stream`; _staged returns the staged stream's value, cached until the
 * next pfmscan_stage.  Both keep their per-workgroup partials in scratch the ctx owns (as every entry point does, see the
 * top of this file): ONE row-bound call in flight per ctx -- a second one on another stream, or a pfmscan_library_hits_sum_staged
 * / _host beside a _dev call, would share the partials and may return a wrong (too small) bound, which costs hits.  The first
 * _dev call of a ctx allocates that scratch (a few KB, one synchronous hipMalloc); every later one is asynchronous. */
int pfmscan_profile_row_bound_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const void *d_profile,
                                  int profile_dtype, int64_t n_pos, double *d_out, void *stream);
int pfmscan_profile_row_bound_staged(pfmscan_ctx *ctx, double *row_sum_max);
/* Diagnostic (host only, no device needed): thr_eff_out[k] = the letters threshold the prefilter of
 * pfmscan_library_hits_sum_* is built for (see above): letter_tables [n][m][8], struct_pssms [n][m][7], thr_seq / thr_sum /
 * thr_eff_out [n].  The letter tables are those of pfmscan_library_create: a 4-letter alphabet, columns 4..7 NaN (else
 * PFMSCAN_E_BADARG, as for NaN thresholds or a NaN row_sum_max).  Every window whose three predicates hold has (double)seq > thr_eff; tests check that by brute force. */
int pfmscan_library_sum_thresholds(const double *letter_tables, const double *struct_pssms,
                                   int n_motifs, int m, const double *thr_seq,
                                   const double *thr_sum, double row_sum_max, double *thr_eff_out);

/* ---- LETTER libraries: the structure side as letter strings (SURVEY 8f N1 x N4) -----------------------------------
 * The reference scans structure FASTA files (`-q pfm structs.fa`, and `-p pfm -q pfm seqs.fa structs.fa`;
 * rnascan.py:119-133) with _py_calculate (matrix.py:25-43: sequential sum of Python floats -- fp64, no float32 cast -- NaN
 * on an unknown letter), one PFM per run (rnascan.py:262), though it ships a multi-PFM format (pfmutil.py:89-133).
 *   struct_tables double [n][m][8]: letter tables of an alphabet of up to 7 letters (codes 0..6; column 7, the foreign
 *   code / separator, must be NaN; unused columns NaN).
 *   seq_tables == NULL: a STRUCTURE-LETTER library over ONE 8-code stream (`rnascan -q library structs.fa`), m <= 32.
 *     Hit of motif k at window p <=> score_k(p) > thr_struct[k] (fp64 compare, strict: NaN and -inf never pass); the
 *     score comes back in hit_struct, hit_seq is NaN / not written; thr_seq is ignored (may be NULL).  One pass per
 *     128 motifs at w = 12: single-letter integer credits for eight motifs per 16-byte table entry (k_library8), exact
 *     fp64 re-score of the survivors.
 *   seq_tables double [n][m][8] (4-letter alphabet): a TWO-FASTA library over two code streams of the same layout (the
 *     sequences and the structure strings of the same records), m <= 64.  Hit of pair k at window p <=>
 *     (double)(float)seq_k(p) > thr_seq[k] on the first stream AND struct_k(p) > thr_struct[k] on the second -- the inner
 *     join of combine() (rnascan.py:416-434).  k_library's prefilter on the sequence side; its survivors get the fp64
 *     letter score of the second stream.
 * Thresholds must be finite on the prefiltered side (thr_struct resp. thr_seq > -inf).  Scores are the numbers
 * pfmscan_hits_letters_f64_* / pfmscan_hits_pair_* give for each motif (pair) alone.  Scanned through
 * pfmscan_library_hits_staged (stage the stream with pfmscan_stage, the second one with pfmscan_stage_codes2) or the
 * two entry points below; d_codes2 / codes2 are NULL for a structure-letter library. */
int pfmscan_library_create_letters(pfmscan_ctx *ctx, const double *seq_tables,
                                   const double *struct_tables, int n_motifs, int m,
                                   pfmscan_library **out);
int pfmscan_library_hits_letters_dev(pfmscan_ctx *ctx, pfmscan_library *lib,
                                     const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos,
                                     const double *thr_seq, const double *thr_struct, int64_t capacity,
                                     int64_t *d_hit_pos, int32_t *d_hit_motif, float *d_hit_seq,
                                     double *d_hit_struct, uint64_t *d_hit_count, void *stream);
int pfmscan_library_hits_letters_host(pfmscan_ctx *ctx, pfmscan_library *lib,
                                      const uint8_t *codes, const uint8_t *codes2, int64_t n_pos,
                                      const double *thr_seq, const double *thr_struct, int64_t capacity,
                                      int64_t *hit_pos, int32_t *hit_motif, float *hit_seq,
                                      double *hit_struct, int64_t *n_hits);
/* Two-FASTA LIBRARIES with joint thresholds (rnascan.py:273, :416-434): pfmscan_library_hits_letters_dev / _host for a library made
 * by pfmscan_library_create_letters with both parts, plus thr_sum [n] (one T per pair; all -inf = the plain call).  The predicate
 * of pfmscan_hits_pair_sum_* sits in phase B of the one-pass library kernel (k_library<.., uint8_t, true, SUM>); phase A's credits
 * are built for thr_eff[k] = max(thr_seq[k], thr_sum[k] - U2[k] - margins), U2 = the sum of the row maxima of the pair's structure
 * table, so thr_seq[k] may be -inf as long as thr_eff[k] is finite (else PFMSCAN_E_BADARG: scan that pair with
 * pfmscan_hits_pair_sum_*).  pfmscan_library_letters_sum_thresholds (host only): tables [n][m][8] and thresholds -> thr_eff [n],
 * -inf where the route is closed (a +inf cell in the structure table or a +inf / NaN letter cell beside thr_seq = -inf, thr_sum = -inf). */
int pfmscan_library_hits_letters_sum_dev(pfmscan_ctx *ctx, pfmscan_library *lib, const uint8_t *d_codes,
                                         const uint8_t *d_codes2, int64_t n_pos, const double *thr_seq,
                                         const double *thr_struct, const double *thr_sum, int64_t capacity,
                                         int64_t *d_hit_pos, int32_t *d_hit_motif, float *d_hit_seq,
                                         double *d_hit_struct, uint64_t *d_hit_count, void *stream);
int pfmscan_library_hits_letters_sum_host(pfmscan_ctx *ctx, pfmscan_library *lib, const uint8_t *codes,
                                          const uint8_t *codes2, int64_t n_pos, const double *thr_seq,
                                          const double *thr_struct, const double *thr_sum, int64_t capacity,
                                          int64_t *hit_pos, int32_t *hit_motif, float *hit_seq,
                                          double *hit_struct, int64_t *n_hits);
int pfmscan_library_letters_sum_thresholds(const double *letter_tables, const double *struct_tables, int n_motifs,
                                           int m, const double *thr_seq, const double *thr_sum, double *thr_eff);

/* Diagnostics (host only, no device needed): the unsigned two-letter credit table the prefilters use for ONE motif
 * (letter_table double [m][8], 4-letter alphabet) at threshold thr_seq: credits uint16 [ceil(m/2)][16], entry index
 * c0 | c1 << 2, with `bits` = 16 (k_letters_cred; k_library for PFMs wider than 16), 10 (k_library up to width 16:
 * three credits per dword, twelve motifs per 16-byte table entry) or 0 (what k_library uses at this width).  A window
 * whose credits sum modulo 2^bits has bit (bits - 1) clear cannot be a hit; *slack = how far below the threshold a kept
 * window's score may lie (score units). */
int pfmscan_debug_credit_table(const double *letter_table, int m, double thr_seq, int bits,
                               uint16_t *credits, double *slack);

/* The same for the single-letter credits k_library8 uses for ONE motif of a structure-letter library (pfmscan_library_create_letters
 * without sequence tables): credits uint16 [4 ceil(m/4)][8] -- the width padded to a multiple of 4 with rows of full credit --
 * 16-bit sums, bit 15 clear = the window cannot be a hit (matrix.py:25-43 score, strict `>` of rnascan.py:263); m <= 32. */
int pfmscan_debug_library8_credits(const double *letter_table, int m, double thr, uint16_t *credits, double *slack);

/* The same for the SINGLE-letter credit table of the generic-alphabet hits kernel (k_letters_cred8, PFMs up to width 32,
 * letter_table double [m][8] with up to 7 letters): credits uint16 [m][8], entry index = the letter code; NaN and -inf
 * cells and the foreign code get no credit.  *mode = 1: the kernel uses the table; 2: more than 1/32 of the windows would
 * survive it, the exact kernel runs instead; 3: no prefilter possible (+inf cells).  A window whose credits sum modulo 2^16
 * has bit 15 clear cannot be a hit (fp64 score > thr, matrix.py:25-43). */
int pfmscan_debug_credit8_table(const double *letter_table, int m, double thr, uint16_t *credits, int *mode);

/* How the `_host` / `pfmscan_stage` / pipeline entry points move host memory to the device.
 *   PFMSCAN_UPLOAD_RUNTIME (default): hipMemcpyAsync from the caller's pages; the runtime pins them in place, which
 *     reaches the PCIe rate for ordinary (anonymous) memory.
 *   PFMSCAN_UPLOAD_STAGED: transfers of 256 MB and more are cut into 64-MiB pieces that a pool of host threads copies
 *     into pinned buffers while the DMA engine moves the previous piece.  For a source that is a FILE MAPPING (a packed
 *     profile store, rnascan/pfmutil.py:61-87 converted once) the page faults are then taken in parallel instead of
 *     inside the runtime's copy: 32 -> 56 GB/s on a page-cache-warm 4 GB store.
 * The mode stays set until changed. */
#define PFMSCAN_UPLOAD_RUNTIME 0
#define PFMSCAN_UPLOAD_STAGED  1
int pfmscan_set_upload_mode(pfmscan_ctx *ctx, int mode);
/* Tell the staged uploader that the host range [base, base + length) is a read-only MAPPING of `path` starting at byte
 * `file_offset` of that file (what numpy.memmap / mmap give the caller for a packed profile store).  A staged transfer
 * whose source lies inside the range then READS THE FILE (pread into the pinned buffers) instead of touching the mapping:
 * no page faults, no page-table entries to build and to tear down again -- unmapping an 8.4 GB store that was uploaded
 * through its mapping costs up to 0.2 s of munmap at exit on a box whose tmpfs / page cache has no huge pages.  The bytes
 * are the same either way.  length == 0 (path may be NULL) forgets the range: do that BEFORE unmapping it.  At most 8
 * ranges per context; a ninth replaces the oldest. */
int pfmscan_upload_source_file(pfmscan_ctx *ctx, const void *base, size_t length, const char *path, int64_t file_offset);
/* The same, for a caller that recorded fstat's st_dev / st_ino / st_size of the file WHEN IT MAPPED IT: the range is only
 * registered when `path` still names that file (a store re-packed by atomic rename in the meantime would otherwise be
 * read in the mapping's place); PFMSCAN_E_BADARG otherwise, and uploads keep reading the mapping. */
int pfmscan_upload_source_file_checked(pfmscan_ctx *ctx, const void *base, size_t length, const char *path,
                                       int64_t file_offset, int64_t st_dev, int64_t st_ino, int64_t st_size);

/* ---- dot-bracket structures -> structure-context letters ------------------------------------------------------
 * Replaces scripts/parse_secondary_structure.cpp (parse(), :65-221, and the line loop of its main(), :235-261): the
 * separate binary that turns folding output such as `((..((...))..))` into the EHTBLRM letters every structure-letter
 * mode reads.  Input: a packed stream in the layout above whose letters are dot-bracket codes
 *     '.' = 0, '(' = 1, ')' = 2, any other byte = 3          (PFMSCAN_SEP after every record)
 * (pfmscan_fasta_encode with that LUT).  Output: the same layout, each position the code of its context letter through
 * `map` (7 entries, the caller's codes of E H T B L R M, each 0..6; {0,1,2,3,4,5,6} for the order EHTBLRM),
 * PFMSCAN_SEP at separators, case bit clear -- what the letter scans (pfmscan_hits_letters_f64_*, pfmscan_hits_pair_*,
 * letter libraries) read.  The rules (a run of dots [a, b) between brackets k = a - 1 and m = b, p[] = partner):
 *     '(' -> L, ')' -> R;  a run at either end of its record -> E;  '(' .. ')' -> H;  ')' .. '(' -> M inside a pair,
 *     E outside;  '(' .. '(' or ')' .. ')' -> B when p[m] + 1 == p[k], else T -- except that such a run becomes M when it
 *     ends at p[j] - 1 or starts at p[m'] + 1 for a ')' at j followed by a '(' or by a multiloop run whose next bracket
 *     is m'.
 * Deviation: the reference reads past the end of an unbalanced string and drops characters it does not know; here a
 * stream with an unbalanced record, a byte outside "().", or no separator at its end is REJECTED: PFMSCAN_E_BADARG,
 * *first_bad = the first stream position at which it is invalid (a depth below zero, a separator at depth above zero,
 * a code 3, or a last position that is not a separator), nothing is written.  A record of 2^31 positions or more:
 * PFMSCAN_E_BADSHAPE, *first_bad = its separator.  On success *first_bad = -1.
 * counts: the histogram of the written codes 0..6 (int64 [7]): compute_background's letter counts of the annotated
 * records (rnascan.py:440-465) without another pass.
 *
 * _dev: d_in and d_out are device buffers of n_pos bytes that must not overlap; d_counts a device int64 [7] or NULL.
 *   Asynchronous on `stream` (NULL: the ctx's stream) EXCEPT for the validity verdict: `stream` is synchronised once
 *   after the validation pass.  Device scratch (depth, partners, tile sums) belongs to the ctx. */
int pfmscan_dotbracket_annotate_dev(pfmscan_ctx *ctx, const uint8_t *d_in, uint8_t *d_out, int64_t n_pos,
                                    const uint8_t *map, int64_t *d_counts, int64_t *first_bad, void *stream);
/* Upload host dot-bracket codes and leave the ANNOTATED stream staged: which = 0 in the codes slot (as pfmscan_stage
 * with codes only; nothing is staged after an error), which = 1 as the second code stream (as pfmscan_stage_codes2: a
 * stream of the same n_pos must be staged).  Every *_staged letter entry point and pfmscan_library_hits_staged of a
 * letter library then scan it with no further H2D.  counts: host int64 [7] or NULL. */
int pfmscan_dotbracket_stage(pfmscan_ctx *ctx, const uint8_t *codes, int64_t n_pos, int which, const uint8_t *map,
                             int64_t *counts, int64_t *first_bad);
/* Host buffers in and out (out: n_pos bytes); leaves the staged stream alone.  counts: host int64 [7] or NULL. */
int pfmscan_dotbracket_annotate_host(pfmscan_ctx *ctx, const uint8_t *in, uint8_t *out, int64_t n_pos,
                                     const uint8_t *map, int64_t *counts, int64_t *first_bad);

/* ---- fragment structures -> averaged-structure profile rows ------------------------------------------------
 * Replaces the averaging of rnascan/average_structure.py, get_structure_probability_matrix_for_sequence (:44-99), as
 * scripts/run_folding (fold(), :60-70) runs it per record of length L > 50 (the skip, :63-65, is the caller's):
 *   fragment starts  i in range(-w/2, L - w/2, w - o) in Python 2 integer arithmetic (:47): -ceil(w/2) .. L - floor(w/2)
 *   fragment i       seq[max(i, 0) : i + w], folded (RNAfold -p, centroid structure: line 4, first ' ' field, :134-141)
 *                    and annotated to EHTBLRM (parse_secondary_structure, :76-83)
 *   alignment        '-' * i + letters + '-' * (L - (i + w)) (:89-92): the letters cover rows [max(i, 0), + their length)
 *   counts           B E H L M R T per row, gaps skipped (struct_pfm_from_aligned, :28-42)
 *   value            c / n in fp64, n = the fragments covering the row (norm_pfm, pfmutil.py:136-151), written with str()
 *                    (write_pfm, pfmutil.py:61-87) and read back by the scan with pandas (rnascan.py:296-297)
 * Here a row's value in column k is table[n (n + 1) / 2 + c] for the row's coverage n and count c, 0 <= c <= n <= n_max:
 * the caller's table -- pfmscan_profile_parse of repr(c / n) gives what a scan of the reference's text reads, c / n itself
 * what that text must show.  Rows come out in the packed-store layout (store.py): [n_rows][7] in B E H L M R T order, each
 * record's rec_len rows followed by one zero row; out_dtype PFMSCAN_PROFILE_F64, or F32 (the round-to-nearest cast).
 *
 * Tables (int64; rows are 0-based rows of `out`):
 *   fragment f   frag_off[f] = stream position of its first letter, frag_len[f] >= 1 letters, frag_row[f] = the output
 *                row of its first letter.  Sorted by record, then by frag_row.
 *   record r     rec_row[r] = its first row (rec_row[0] = 0, each record right after the previous one's zero row),
 *                rec_len[r] = its length, fragments [rec_frag[r], rec_frag[r + 1]) (rec_frag has n_rec + 1 entries,
 *                rec_frag[0] = 0, rec_frag[n_rec] = n_frag).  Every fragment lies inside its record.
 * Rejections (nothing counts as written; *first_bad and *bad_kind say where and what):
 *   PFMSCAN_AVG_UNCOVERED   a row of a record that no fragment covers: PFMSCAN_E_BADARG, *first_bad = the row (the
 *                           reference divides by zero there, norm_pfm)
 *   PFMSCAN_AVG_COVER       a row covered more than n_max times: PFMSCAN_E_BADSHAPE, *first_bad = the row
 *   PFMSCAN_AVG_BAD_TABLE   tables that break the rules above: PFMSCAN_E_BADARG, *first_bad = the record
 *   PFMSCAN_AVG_DOTBRACKET  (_host / _stage) an invalid dot-bracket fragment: as pfmscan_dotbracket_annotate_dev,
 *                           *first_bad = the stream position
 * The earliest row wins when several rows are rejected; a broken table (its earliest record) wins over every row, since
 * rows computed from it mean nothing.  n_max <= PFMSCAN_MAX_COVER.
 *
 * _dev: d_letters = annotated codes whose code IS the column (annotate with map {1, 2, 6, 0, 3, 5, 4}: E H T B L R M ->
 *   B E H L M R T columns); max_len >= every frag_len; all tables and the table of (n_max + 1)(n_max + 2) / 2 doubles are
 *   device buffers; d_out holds n_rows rows.  Asynchronous on `stream` (NULL: the ctx's) except for the verdict: `stream`
 *   is synchronised once.  Device scratch: 8 bytes per 256 rows.
 * _host: `codes` = the fragments' dot-bracket codes in the stream layout (dotbracket LUT, PFMSCAN_SEP after each), the
 *   tables and `table` on the host; uploads, annotates and averages, and copies the rows to `out` (host).  Device scratch
 *   ~ 2 n_pos + 24 n_frag + 24 n_rec bytes + the rows: the caller bounds it by batching records.
 * _stage: as _host, but the rows stay staged in the profile slot (as pfmscan_stage with a profile only; *n_rows = their
 *   number): pfmscan_scan_staged / pfmscan_hits_staged / pfmscan_library_hits_staged of structure motifs scan them with no
 *   H2D.  Nothing is staged after an error. */
#define PFMSCAN_MAX_COVER 1024
#define PFMSCAN_AVG_OK         0
#define PFMSCAN_AVG_DOTBRACKET 1
#define PFMSCAN_AVG_UNCOVERED  2
#define PFMSCAN_AVG_COVER      3
#define PFMSCAN_AVG_BAD_TABLE  4
int pfmscan_average_dev(pfmscan_ctx *ctx, const uint8_t *d_letters, int64_t n_letters, const int64_t *d_frag_off,
                        const int64_t *d_frag_len, const int64_t *d_frag_row, int64_t n_frag, int64_t max_len,
                        const int64_t *d_rec_row, const int64_t *d_rec_len, const int64_t *d_rec_frag, int64_t n_rec,
                        int64_t n_rows, const double *d_table, int n_max, void *d_out, int out_dtype, int64_t *first_bad,
                        int *bad_kind, void *stream);
int pfmscan_average_host(pfmscan_ctx *ctx, const uint8_t *codes, int64_t n_pos, const int64_t *frag_off,
                         const int64_t *frag_len, const int64_t *frag_row, int64_t n_frag, const int64_t *rec_row,
                         const int64_t *rec_len, const int64_t *rec_frag, int64_t n_rec, const double *table, int n_max,
                         void *out, int out_dtype, int64_t *first_bad, int *bad_kind);
int pfmscan_average_stage(pfmscan_ctx *ctx, const uint8_t *codes, int64_t n_pos, const int64_t *frag_off,
                          const int64_t *frag_len, const int64_t *frag_row, int64_t n_frag, const int64_t *rec_row,
                          const int64_t *rec_len, const int64_t *rec_frag, int64_t n_rec, const double *table, int n_max,
                          int out_dtype, int64_t *n_rows, int64_t *first_bad, int *bad_kind);
/* Fragment ids (host only, no ctx): the id spans of pfmscan_fasta_ids (id_off, id_len into buf) of fragments named as
 * run_folding names them, <id>_frag_<i> (average_structure.py:58) -> key_len[k] (the key is buf[id_off[k], + key_len[k]):
 * everything before the LAST "_frag_", at least one byte) and start[k] (the signed decimal after it: an optional '-' and
 * 1..18 digits, nothing else).  PFMSCAN_E_BADARG with *first_bad = the first id that does not parse. */
int pfmscan_fragment_ids(const uint8_t *buf, const int64_t *id_off, const int64_t *id_len, int64_t n, int64_t *key_len,
                         int64_t *start, int64_t *first_bad);

/* ---- averaged-structure profiles -> per-record column sums (the structure background of a profile input) ----------
 * compute_background (rnascan.py:440-465) counts the letters of the input records; `load_background` (:468-484) hands it
 * whatever the structure input is, and for an averaged-structure directory that is no FASTA file: the reference has no
 * background for its fourth mode.  For profiles the count of letter c is the sum of column c over every row of every
 * record (the expected number of that letter; for one-hot rows exactly compute_background's count).  These entry points
 * give the sums PER RECORD, double [n_rec][7] in the profile's column order; the caller adds the records up (math.fsum per
 * column: exactly rounded, so independent of batches, chunks and ranks) and applies (count + 1) / (7 + sum of counts).
 * A record's sums depend on that record's rows alone, in a fixed order of fp64 additions anchored at its first row
 * (float32 rows are widened first): rows in pieces of 2048; in a piece lane t of 256 adds rows t, t + 256, ... in order;
 * the 64 lanes of each of the four waves are folded as a[i] += a[i + s] for s = 32 .. 1; the waves as
 * ((w0 + w1) + w2) + w3; the pieces one after the other.  No atomics: the same input gives the same bits on every run.
 *   rec_off / rec_len  int64 [n_rec]: first row and length of every record, as pack.Stream / store.ProfileStore keep
 *                them: ascending, every record followed by at least one (separator) row that belongs to no record and
 *                is not read as data.  A table that breaks this: PFMSCAN_E_BADARG, *first_bad = -1.
 * Rejection: a cell of a record that is NaN, +-inf or negative makes a background meaningless (the scan itself keeps
 * accepting such cells, rnascan.py:306 nan_to_num): PFMSCAN_E_BADARG, *first_bad = the flat element index row * 7 +
 * column of the EARLIEST such cell of the stream; the sums are not to be used.  *first_bad = -1 on success.
 *
 * _dev: d_profile (16-byte aligned), the tables and d_sums are device buffers.  Asynchronous on `stream` (NULL: the
 *   ctx's) except for the verdict: `stream` is synchronised once.  Device scratch (56 bytes per piece) belongs to the ctx.
 * _host: a host stream of ANY length (a numpy array or a mapped packed store; through the ctx's upload mode, see
 *   pfmscan_set_upload_mode / pfmscan_upload_source_file) with bounded device scratch: it is cut at record boundaries into
 *   pieces of at most 2^24 rows (PFMSCAN_COLSUMS_CHUNK in the environment overrides; a longer record is a piece of its
 *   own), the upload of piece k + 1 runs beside the sums of piece k in two alternating buffers.  Leaves the staged
 *   stream alone.  sums: host double [n_rec][7].
 * _staged: the profile that pfmscan_stage / pfmscan_average_stage left on the device; rec_off, rec_len and sums on the
 *   host. */
int pfmscan_profile_colsums_dev(pfmscan_ctx *ctx, const void *d_profile, int profile_dtype, int64_t n_pos,
                                const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_sums,
                                int64_t *first_bad, void *stream);
int pfmscan_profile_colsums_host(pfmscan_ctx *ctx, const void *profile, int profile_dtype, int64_t n_pos,
                                 const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *sums,
                                 int64_t *first_bad);
int pfmscan_profile_colsums_staged(pfmscan_ctx *ctx, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                                   double *sums, int64_t *first_bad);

/* ---- site profiles: profile rows and letters summed under aligned hit windows ---------------------------------------
 * What the sites of a motif look like: the structural context under the hits of a sequence motif, the same over
 * flanks (the meta-profile), and the counts a site PFM is made from.  The reference builds its averaged profiles by
 * counting aligned context letters (average_structure.py:28-42) and normalising per position (pfmutil.py:136-151);
 * summing the profile rows under aligned hit windows is the same operation on hits.
 * Inputs: a packed stream (codes and / or profile rows [n_pos][7], float32 or float64), its record table rec_off /
 * rec_len (as pfmscan_profile_colsums_*), a hit list hit_pos[0..n_hits): stream positions of window starts, STRICTLY
 * ascending, every window [pos, pos + m) inside ONE record; width m >= 1, flank F >= 0, W = m + 2 F <=
 * PFMSCAN_MAX_WIDTH (else PFMSCAN_E_BADSHAPE).
 * Columns: column j in [0, W) of hit h is stream row x = hit_pos[h] - F + j.  It COUNTS only if x lies inside the hit's
 *   record; flank columns that hang over a record end are skipped, not read.
 * Groups: the hits of one record, in order, are cut into groups of at most PFMSCAN_SITE_GROUP hits, anchored at the
 *   record's first hit: a group is a function of that record's hits alone, whatever batch, chunk or rank holds it.
 * Per group the device produces
 *   sums   double [W][7] (with a profile): sums[j][c] = the sum of (double) profile[x][c] over the group's hits whose
 *          column j counts; float32 rows are widened first;
 *   counts uint32 [W][8] (with codes): counts[j][k] = the number of those hits with min(codes[x], 7) == k; bin 7 is a
 *          foreign letter inside the record.  The sum over k of counts[j][k] is the number of hits whose column j counts.
 * Order of additions inside a group (only additions, no FMA; a function of the group alone): wave v of a workgroup's
 *   four waves starts every cell at 0.0 and adds the group's hits v, v + 4, v + 8, ... in ascending order, skipping a
 *   hit whose column does not count; the group's cell is ((w0 + w1) + w2) + w3.  tests/sites_rules.py restates this in
 *   numpy and the kernels equal it bit for bit.  No atomics: the same input gives the same bits on every run.
 * The caller adds the groups of all records, batches and ranks with math.fsum per cell (exactly rounded, so independent
 *   of how the hits were cut) and the counts as int64; the site PFM's row j is sums[j][.] / (the row's sum), the letter
 *   row counts[j][letter] / (the sum over the alphabet's letters).
 * Rejection: a NaN, +-inf or negative profile cell UNDER A COUNTED COLUMN OF A HIT makes the result meaningless:
 *   PFMSCAN_E_BADARG, *first_bad = the smallest flat element index row * 7 + column among the cells touched; the sums
 *   are not to be used.  The same cell under no hit (or under a skipped flank column) is no error.  *first_bad = -1 on
 *   success and for every other error.
 *
 * pfmscan_site_groups: host only, no ctx (no message is left: the return code says it all).  Checks the record table
 *   (offsets and lengths >= 0, every record behind the one before it and its separator), that the hits ascend strictly
 *   and that every window lies inside one record: PFMSCAN_E_BADARG otherwise.  Fills grp_first [*n_grp + 1] (indices
 *   into hit_pos, the last one n_hits) and grp_rec [*n_grp].  capacity: room for that many groups (grp_first holds one
 *   entry more); PFMSCAN_E_CAPACITY with *n_grp = what suffices when there are more (nothing was written).
 * _dev: every buffer is a device buffer (d_codes or d_profile may be NULL, and with it d_counts / d_sums; d_profile
 *   8-byte aligned).  d_sums [n_grp][W][7], d_counts [n_grp][W][8].  The groups are the caller's: any table whose groups
 *   are at most PFMSCAN_SITE_GROUP hits of one record each and cover the hits in order is taken, one that is not (or hits
 *   that do not ascend, a window that leaves its record, a record outside the stream) gives PFMSCAN_E_BADARG with
 *   *first_bad = -1, decided on the device without a load outside the buffers.  Asynchronous on `stream` (NULL: the
 *   ctx's) except for the verdict: `stream` is synchronised once.  Device scratch (8 bytes per group) belongs to the ctx.
 * _staged: the stream that pfmscan_stage / pfmscan_average_stage left on the device (use_codes / use_profile say which
 *   parts to sum); hits, tables and outputs on the host.  It cuts the groups itself: capacity = the groups the outputs
 *   hold (grp_rec [capacity], sums [capacity][W][7], counts [capacity][W][8]), PFMSCAN_E_CAPACITY with *n_grp set when
 *   there are more.
 * _host: a host stream of ANY length (a numpy array or a mapped packed store; through the ctx's upload mode), cut at
 *   record boundaries into pieces of at most 2^24 rows (PFMSCAN_SITES_CHUNK in the environment overrides; a longer
 *   record is a piece of its own; a piece no hit lies in is not uploaded); the upload of piece k + 1 runs beside the
 *   sums of piece k in two alternating buffers.  Leaves the staged stream alone.  Otherwise as _staged. */
int pfmscan_site_groups(const int64_t *hit_pos, int64_t n_hits, const int64_t *rec_off, const int64_t *rec_len,
                        int64_t n_rec, int32_t m, int64_t capacity, int64_t *grp_first, int64_t *grp_rec, int64_t *n_grp);
int pfmscan_site_sums_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                          const int64_t *d_hit_pos, int64_t n_hits, const int64_t *d_grp_first, const int64_t *d_grp_rec,
                          int64_t n_grp, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, int32_t m,
                          int32_t flank, double *d_sums, uint32_t *d_counts, int64_t *first_bad, void *stream);
int pfmscan_site_sums_staged(pfmscan_ctx *ctx, int use_codes, int use_profile, const int64_t *hit_pos, int64_t n_hits,
                             const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int32_t m, int32_t flank,
                             int64_t capacity, int64_t *grp_rec, double *sums, uint32_t *counts, int64_t *n_grp,
                             int64_t *first_bad);
int pfmscan_site_sums_host(pfmscan_ctx *ctx, const uint8_t *codes, const void *profile, int profile_dtype, int64_t n_pos,
                           const int64_t *hit_pos, int64_t n_hits, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                           int32_t m, int32_t flank, int64_t capacity, int64_t *grp_rec, double *sums, uint32_t *counts,
                           int64_t *n_grp, int64_t *first_bad);

/* ---- site profiles of a library: exact per-motif sums in one pass -----------------------------------------------------
 * The site profile of EVERY motif of a multi-PFM library of one width m, from one pass over the stream: what
 * pfmscan_site_sums_* + math.fsum give for each motif alone, bit for bit, without bringing the group rows home.
 * Hit list: (hit_pos, hit_motif) over the n_motifs motifs.  The _dev form and pfmscan_site_groups_lib take it
 *   MOTIF-MAJOR: hit_motif does not descend, inside one motif the positions ascend strictly, every window
 *   [pos, pos + m) lies inside one record.  Columns, flank F, W = m + 2 F <= PFMSCAN_MAX_WIDTH, "a column counts" and
 *   the rejection rule are those of pfmscan_site_sums_* above.
 * Groups: the groups of motif k are what pfmscan_site_groups gives for motif k's hit list alone: at most
 *   PFMSCAN_SITE_GROUP consecutive hits of one (motif, record), anchored at that pair's first hit.
 * Group cell: as above -- lane-wave v of four starts at 0.0 and adds hits v, v + 4, ... in ascending order, the group's
 *   cell is ((w0 + w1) + w2) + w3; only additions, float32 rows widened first (tests/sites_rules.py).
 * Per-motif sum: for motif k and cell e = 7 j + c the LONG ACCUMULATOR holds EXACTLY the integer
 *   A = sum over the groups of motif k of (group cell value / 2^-1074); the values are finite and >= 0.
 *   Layout: uint64 acc[n_motifs][PFMSCAN_SITE_LIMBS][W * 7], A = sum over i of acc[k][i][e] * 2^(32 i).  Limbs are the
 *   slow index inside a motif: the 64 lanes of a wave (consecutive cells) add to contiguous addresses.
 *   A double v > 0 with exponent field E and fraction f: M = f, b = 0 if E == 0 (subnormal), else M = f | 2^52,
 *   b = E - 1; x = M << (b mod 32) < 2^85; its three 32-bit pieces are added to limbs b / 32, b / 32 + 1, b / 32 + 2.
 *   DBL_MAX reaches limb 65, hence 66 limbs.  Zero pieces and v == 0 add nothing.  (rnascan_amd/csrc/pfmscan_superacc.hpp,
 *   shared by host and device; tests/sites_lib_rules.py restates it in Python ints.)
 *   Integer additions do not depend on their order: the limbs are the same for every schedule, so the device adds
 *   with 64-bit integer atomics and the bits still do not depend on how the work was cut.  No float atomics.
 *   Headroom: a call adds fewer than 2^31 groups of fewer than 2^32 per limb: a RAW limb stays below 2^63.  An
 *   accumulator is NORMALISED when every limb but the top one is below 2^32; the top limb has room for 2^46 values of
 *   DBL_MAX.
 *   Rounding: pfmscan_site_acc_round takes A * 2^-1074 to the nearest double, ties to even, +inf beyond DBL_MAX: a
 *   motif's S[j][c] is bit for bit math.fsum over its group rows.
 * Counts: uint64 counts[n_motifs][W][8], the integer sums of the per-group counts.  Coverage comes from positions and
 *   record bounds on the host, per motif.
 * Rejection: a NaN, +-inf or negative cell under a counted column of a hit of ANY motif: PFMSCAN_E_BADARG, *first_bad
 *   = the smallest flat element index touched.  NOTE the difference from one pfmscan_site_sums_* run per motif, which
 *   fails only for the motifs whose hits touch the cell.  A group cell that overflows to +inf from finite cells:
 *   PFMSCAN_E_BADARG with *first_bad = -1 and a message that says so; a non-finite value is never decomposed.
 *
 * Host only, no ctx, no message (the return code says it all):
 * pfmscan_site_groups_lib: checks the motif-major list (motif indices in [0, n_motifs)) and the record table and cuts
 *   the groups: grp_first [*n_grp + 1] (indices into the list), grp_rec, grp_motif [*n_grp].  Capacity protocol and
 *   return codes of pfmscan_site_groups.
 * pfmscan_site_order_lib: order[i] = index, in the given list, of hit i of the motif-major list: a STABLE counting sort
 *   by motif, so a list in (position, motif) order -- as pfmscan_library_hits_* return hits -- becomes motif-major.
 *   An index outside [0, n_motifs): PFMSCAN_E_BADARG.
 * pfmscan_site_acc_add: dst (normalised) += src (raw or normalised) for n_acc accumulators of n_words_per_limb words
 *   per limb each (n_motifs and W * 7); dst is normalised again.  PFMSCAN_E_BADSHAPE if a top limb overflows.
 * pfmscan_site_acc_round: acc (raw or normalised) [n_acc][LIMBS][n_cells] -> out double [n_acc][n_cells].
 * pfmscan_site_acc_from_doubles: acc_one_cell [LIMBS] = the RAW sum of n < 2^31 values, each finite and >= 0
 *   (PFMSCAN_E_BADARG otherwise), by the device's decomposition.
 *
 * _dev: every buffer is a device buffer; the tables are the caller's (pfmscan_site_groups_lib makes them).  Zeroes
 *   d_acc [n_motifs][LIMBS][W * 7] / d_counts [n_motifs][W][8] itself and leaves this call's RAW sums there.  A table
 *   that is broken (groups that do not cover the hits in order, an empty group or one of more than PFMSCAN_SITE_GROUP
 *   hits, grp_motif descending or outside [0, n_motifs), positions not ascending inside a motif, a window outside its
 *   group's record, a record outside the stream): PFMSCAN_E_BADARG, *first_bad = -1, decided on the device without a
 *   load or an add outside the buffers.  Asynchronous on `stream` except for the verdict's one synchronise.  Device
 *   scratch (8 bytes per four groups) belongs to the ctx.
 * _staged: the staged stream; hits on the host AS pfmscan_library_hits_* RETURN THEM (any order that is ascending in
 *   position inside each motif); it reorders, cuts the groups and returns NORMALISED accumulators acc / counts on the host.
 * There is no pipeline (_host) form: the caller stages, as for pfmscan_library_hits_sum_staged. */
int pfmscan_site_groups_lib(const int64_t *hit_pos, const int32_t *hit_motif, int64_t n_hits, int32_t n_motifs,
                            const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int32_t m, int64_t capacity,
                            int64_t *grp_first, int64_t *grp_rec, int64_t *grp_motif, int64_t *n_grp);
int pfmscan_site_order_lib(const int64_t *hit_pos, const int32_t *hit_motif, int64_t n_hits, int32_t n_motifs, int64_t *order);
int pfmscan_site_acc_add(uint64_t *dst, const uint64_t *src, int64_t n_acc, int64_t n_words_per_limb);
int pfmscan_site_acc_round(const uint64_t *acc, int64_t n_acc, int64_t n_cells, double *out);
int pfmscan_site_acc_from_doubles(const double *values, int64_t n, uint64_t *acc_one_cell);
int pfmscan_site_sums_lib_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                              const int64_t *d_hit_pos, int64_t n_hits, const int64_t *d_grp_first, const int64_t *d_grp_rec,
                              const int64_t *d_grp_motif, int64_t n_grp, const int64_t *d_rec_off, const int64_t *d_rec_len,
                              int64_t n_rec, int32_t n_motifs, int32_t m, int32_t flank, uint64_t *d_acc, uint64_t *d_counts,
                              int64_t *first_bad, void *stream);
int pfmscan_site_sums_lib_staged(pfmscan_ctx *ctx, int use_codes, int use_profile, const int64_t *hit_pos, const int32_t *hit_motif,
                                 int64_t n_hits, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int32_t n_motifs,
                                 int32_t m, int32_t flank, uint64_t *acc, uint64_t *counts, int64_t *first_bad);

/* ---- site profiles on letter streams: letter and letter-pair counts under hits ------------------------------------------
 * The sites of motifs scanned over LETTER strings (`-p seqs.fa`, `-q structs.fa`, `-p -q seqs.fa structs.fa`): the
 * structure side is a code stream, not a profile, so the site PFM is the reference's own PFM builder on the hit windows --
 * struct_pfm_from_aligned counts the letters of aligned windows per position (average_structure.py:28-42) and norm_pfm
 * divides each row by its sum (pfmutil.py:136-151).  With two streams both letters of every position are known, and one
 * table serves every mode:
 *   joint  uint64 [n_motifs][W][8][8]      W = m + 2 F <= PFMSCAN_MAX_WIDTH (else PFMSCAN_E_BADSHAPE)
 *   joint[k][j][a][b] = the number of hits of motif k whose column j counts and has (codes[x] & 7) == a and
 *                       (codes2[x] & 7) == b,  x = hit_pos - F + j.
 * "A column counts" is what it is for pfmscan_site_sums_*: row x lies inside the hit's record; a flank column that hangs
 *   over a record end is skipped and not read.  The code is taken & 7, not min(code, 7): structure streams keep the
 *   input's case in bit 3 and a lower-case letter counts as its letter (the scores ignore the case, matrix.py:31); index 7
 *   is a foreign letter inside the record.  A stream that is absent (NULL / not used) has index 0 everywhere.
 * The marginals are the two count tables (struct_pfm_from_aligned's counts for the second stream), the sum over a column's
 *   cells its coverage: no second output.  Integer counting is exact and independent of order, so the device adds with
 *   LDS atomics and 64-bit integer global atomics and the table is a function of the input alone; no float atomics.
 * Hit list: (hit_pos, hit_motif) over n_motifs motifs of width m; hit_motif NULL: one motif (n_motifs >= 1).  Every
 *   window [pos, pos + m) lies inside ONE record of the record table rec_off / rec_len (records ascending, each behind
 *   the separator of the one before, as pfmscan_profile_colsums_*).  A hit's record is found ON THE DEVICE by binary
 *   search of rec_off: there are no group tables.
 * _dev: every buffer is a device buffer (d_codes or d_codes2 may be NULL, not both); the list is MOTIF-MAJOR (hit_motif
 *   does not descend), as for pfmscan_site_sums_lib_dev.  Zeroes d_joint itself.  A position outside the stream, a
 *   window that leaves its record, a motif index outside [0, n_motifs) or a motif smaller than the one before:
 *   PFMSCAN_E_BADARG, decided on the device without a load or an add outside the buffers; the table is then not to be
 *   used.  Asynchronous on `stream` (NULL: the ctx's) except for the verdict: `stream` is synchronised once.  Device
 *   scratch (8 bytes per workgroup) belongs to the ctx.  A workgroup owns a slice of the list (PFMSCAN_SITE_JOINT_SLICE in
 *   the environment overrides its length; the table does not depend on it) and counts PFMSCAN_SITE_JOINT_COLS columns at
 *   a time in LDS.
 * _staged: the stream that pfmscan_stage (use_codes) and pfmscan_stage_codes2 (use_codes2) left on the device; hits and
 *   record table on the host, the hits AS pfmscan_library_hits_* RETURN THEM ((position, motif) order; reordered with
 *   pfmscan_site_order_lib); joint comes home.
 * There is no pipeline (_host) form: a FASTA code stream is one byte per position and every letter scan stages it anyway,
 *   so the stream the hits came from is still on the device when they are counted. */
int pfmscan_site_joint_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos,
                           const int64_t *d_hit_pos, const int32_t *d_hit_motif, int64_t n_hits, const int64_t *d_rec_off,
                           const int64_t *d_rec_len, int64_t n_rec, int32_t n_motifs, int32_t m, int32_t flank, uint64_t *d_joint,
                           void *stream);
int pfmscan_site_joint_staged(pfmscan_ctx *ctx, int use_codes, int use_codes2, const int64_t *hit_pos, const int32_t *hit_motif,
                              int64_t n_hits, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int32_t n_motifs,
                              int32_t m, int32_t flank, uint64_t *joint);

/* ---- host ingest and output (no device needed; no context: errors via pfmscan_last_error(NULL)) ---------------
 * The two pieces of host work that dwarf the kernel at scale, in native code.
 *
 * FASTA bytes -> packed code stream.  Replaces SeqIO.parse + preprocess_seq + the per-record encode
 * (rnascan/rnascan.py:170-174, :177-204): a record starts at a line whose first byte is '>', the header is that
 * line without '>' and without trailing \r \n, the letters are every later line stripped of ASCII whitespace at
 * both ends with embedded blanks removed; bytes before the first header are ignored.
 *
 * pfmscan_fasta_index: one pass over `buf` (cut into one piece per thread at line starts, stitched afterwards).
 *   capacity == 0 (arrays may be NULL): only counts the records and
 *   returns PFMSCAN_E_CAPACITY with *n_records set (PFMSCAN_OK when there are none).  Otherwise fills, per record,
 *   hdr_off / hdr_len (header bytes), seq_off / seq_end (byte range of its sequence lines), n_letters.
 * pfmscan_fasta_encode: records [lo, hi) -> codes[sum(n_letters + 1)]: lut256[byte] per letter, `separator`
 *   after each record (stream layout above); offsets[i] = stream position of record lo + i.  n_threads <= 0:
 *   as many as the host offers, at most 16. */
/* pfmscan_count_bytes: counts[256] = how often each byte value occurs in buf (parallel).  Over a packed code stream this
 * is compute_background's letter count (rnascan/rnascan.py:444-457: Seq.count per letter over every record) in one pass:
 * codes 0..6 are the alphabet's letters as written in upper case, 8..14 the lower-case ones, 7 separators / foreign. */
int pfmscan_count_bytes(const uint8_t *buf, int64_t n, int64_t *counts /* [256] */, int n_threads);
/* pfmscan_fasta_lone_cr: *found = 1 when buf holds a carriage return that is not followed by a line feed (old-Mac line
 * ends: the reference's universal-newline reader breaks lines there, pfmscan_fasta_index at \n only -- the caller
 * parses such a file the slow way).  One parallel pass at memory speed over the WHOLE buffer. */
int pfmscan_fasta_lone_cr(const uint8_t *buf, int64_t n, int *found, int n_threads);
int pfmscan_fasta_index(const uint8_t *buf, int64_t n, int64_t capacity, int64_t *hdr_off,
                        int64_t *hdr_len, int64_t *seq_off, int64_t *seq_end, int64_t *n_letters,
                        int64_t *n_records, int n_threads);
 /* pfmscan_fasta_ids: the id of every record = the first whitespace-separated word of its header
  *   (id_off, id_len: byte span in buf); *all_ascii = 0 when some header holds a byte >= 0x80 (the caller then
  *   decodes the headers itself). */
int pfmscan_fasta_ids(const uint8_t *buf, const int64_t *hdr_off, const int64_t *hdr_len,
                      int64_t n_records, int64_t *id_off, int64_t *id_len, int *all_ascii);
 /* pfmscan_gather_spans: the bytes of n_spans (offset, length) spans of buf, each followed by `separator`, back to back
  *   in out (all ids or headers of a file as ONE buffer the caller splits); *n_bytes = the size needed / written. */
int pfmscan_gather_spans(const uint8_t *buf, const int64_t *spans, int64_t n_spans, int separator,
                         uint8_t *out, int64_t capacity, int64_t *n_bytes);
int pfmscan_fasta_encode(const uint8_t *buf, const int64_t *seq_off, const int64_t *seq_end,
                         const int64_t *n_letters, int64_t lo, int64_t hi, const uint8_t *lut256,
                         int separator, uint8_t *codes, int64_t *offsets, int n_threads);

/* Averaged-structure profile text (written by rnascan/pfmutil.py:61-87: a header line, then one row per position:
 * <position> TAB <n_cols numbers>) -> float64 [n_rows][n_cols], the first column dropped, exactly as the reference reads
 * it: `pd.read_table` then `del struct['PO']` (rnascan/rnascan.py:296-297).  pandas' default converter is NOT correctly
 * rounded (at most 17 digits, leading zeros included, then one multiplication or division by a power of ten; about
 * half of all 17-digit reprs come out one ulp off) and the reference computes with those values, so that converter is
 * restated here bit for bit (tests/test_ingest.py compares millions of fields with pandas itself).  The header line is
 * skipped (the caller reads the column letters from it).  PFMSCAN_E_BADSHAPE: something only pandas should judge (blank
 * lines, ragged rows, nan / inf tokens, quotes): parse the file with pandas instead.  PFMSCAN_E_CAPACITY: *n_rows set. */
int pfmscan_profile_parse(const char *buf, int64_t n, int n_cols, int64_t capacity_rows,
                          double *out, int64_t *n_rows);

/* Hit columns -> the bytes `DataFrame.to_csv(sep='\t', index=False)` writes for them (rnascan/rnascan.py:555-567,
 * Match_ID :329-332), without building the table: one descriptor per column, rows formatted in parallel.
 *   CONST    data = bytes, width = their length (the same field in every row)
 *   I64      data = int64 [n_rows]
 *   F32/F64  data = float / double [n_rows]: shortest digits that round-trip in that precision, positional for
 *            1e-4 <= |x| < 1e16 else d.ddde+XX (numpy's str / Python's repr); NaN = empty field, inf = "inf"
 *   INDEXED  data = int64 index [n_rows], aux = int64 offsets [n_values + 1] into blob: row r holds
 *            blob[offsets[i] .. offsets[i + 1]) for i = index[r]  (record ids, descriptions, motif ids; the
 *            caller has applied csv quoting to the values)
 *   FIXED    data = bytes [n_rows][width], trailing NULs dropped (numpy 'S' arrays)
 *   WINDOW   data = int64 stream positions [n_rows], aux = the code stream, blob = 16 letters: the `width` letters
 *            blob[code & 15] of the window at each position (the Sequence column; codes 8..15 = the letters of codes
 *            0..7 as the input wrote them in lower case, see "codes" above)
 *   SPAN     data = int64 index [n_rows], aux = int64 [n_values][2] (offset, length) into blob: row r holds those
 *            bytes of blob (ids / headers straight from the mapped FASTA), csv-quoted here when they hold a tab, a
 *            double quote or a line break
 * first_match_id >= 0 appends a last column counting up from it.  Every row ends in '\n'; no header line.
 * The rows are written by up to PFMSCAN_TSV_MAX_PIECES threads, each into its own slice of `out` (no intermediate
 * buffer, no copy): afterwards piece k is out[pieces[2k] .. pieces[2k] + pieces[2k + 1]) and the table is the
 * pieces in order, k = 0 .. *n_pieces - 1.  `capacity` must cover the longest the rows can get (a bound per numeric
 * column, the real lengths of the INDEXED / SPAN values of the rows at hand); *need holds that size
 * (PFMSCAN_E_CAPACITY when capacity is smaller: nothing was written). */
#define PFMSCAN_TSV_CONST   0
#define PFMSCAN_TSV_I64     1
#define PFMSCAN_TSV_F32     2
#define PFMSCAN_TSV_F64     3
#define PFMSCAN_TSV_INDEXED 4
#define PFMSCAN_TSV_FIXED   5
#define PFMSCAN_TSV_WINDOW  6
#define PFMSCAN_TSV_SPAN    7
#define PFMSCAN_TSV_MAX_PIECES 16
typedef struct pfmscan_tsv_column {
    int32_t kind;
    int32_t reserved;
    const void *data;
    const void *aux;
    const void *blob;
    int64_t width;
} pfmscan_tsv_column;
int pfmscan_tsv_format(const pfmscan_tsv_column *cols, int n_cols, int64_t n_rows,
                       int64_t first_match_id, char *out, int64_t capacity, int64_t *need,
                       int64_t *pieces /* [2 * PFMSCAN_TSV_MAX_PIECES] */, int *n_pieces,
                       int n_threads);

/* Match_ID for rows that were formatted without it (rnascan/rnascan.py:329-332 numbers the rows 1..n AFTER every worker's
 * table has been concatenated; here the ranks of a multi-GPU run format their own rows, and rank 0 numbers them while it
 * relays them in rank order): copies `in` to `out` with "\t<id>" inserted in front of every line end that is not inside a
 * double-quoted field, ids counting up from first_id.  *in_quotes carries the quote state from one block of a stream to the
 * next (0 at the start).  capacity >= n + 21 x (line ends in the block) always suffices; PFMSCAN_E_CAPACITY otherwise. */
int pfmscan_tsv_number(const char *in, int64_t n, int64_t first_id, char *out, int64_t capacity,
                       int64_t *n_out, int64_t *n_rows, int *in_quotes);

/* `round(score, 3)` of rnascan.py:273 for Python floats (the structure letter scores of matrix.py:25-43 are Python
 * floats): out[i] = the double nearest to the decimal with `decimals` (0..15) digits after the point that is nearest
 * to in[i]'s exact value, ties to even -- float.__round__, which numpy.round is not.  NaN / inf pass through. */
int pfmscan_round_decimals(const double *in, int64_t n, int decimals, double *out, int n_threads);

/* ---- measurement helper ------------------------------------------------------
 * Average device time in milliseconds of `iters` back-to-back pfmscan_scan_dev
 * launches, bracketed by hipEvents on the launch stream (after `warmup`
 * untimed launches).  Used by bench.py for the roofline figure. */
int pfmscan_time_scan_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif,
                          const uint8_t *d_codes, const void *d_profile,
                          int profile_dtype, int64_t n_pos, float *d_out_seq,
                          double *d_out_struct, void *stream, int warmup,
                          int iters, double *avg_ms);

/* ---- device arrays of one scan, placed together ------------------------------------
 * No counterpart in the reference (its arrays are numpy arrays in host memory: rnascan.py:296-301, matrix.py:59-62).
 * The arrays one all-scores scan walks in lock-step -- codes, profile rows, the two score arrays -- run up to 12 % faster
 * on MI355X when they lie in parts of HBM that do not share DRAM banks (rnascan_amd/csrc/pfmscan_place.hip).
 * pfmscan_place_alloc allocates n_arrays (1..8) device arrays of bytes[r] each TOGETHER: it takes chunks of physical memory
 * through the HIP virtual memory API, measures which chunks disturb each other, gives every array the chunks that disturb the
 * chunks the other arrays use at the same fraction of the pass least, and returns ptrs[r] (contiguous, 2 MB aligned, contents
 * undefined, usable like any device pointer with every *_dev entry point).  PFMSCAN_PLACE_PLAIN in `flags` (or in the
 * environment) skips the measurement.  pfmscan_place_note: one line about the last allocation (candidates, measured pair
 * times, weighted disturbance chosen / driver order).  Results of scans never depend on placement.
 *
 * COST IN ADDRESS SPACE, AND WHAT pfmscan_place_free DOES.  On ROCm 7.2 an address range that was unmapped, freed and handed
 * out again for other physical memory read back other bytes than were written (profiles/r4/placement/
 * ab_ranges_reused_corrupt.txt; rnascan_amd/csrc/pfmscan_place.hip has the analysis), so NO range this allocator reserves is
 * ever given back while the context lives:
 *   * a measured allocation reserves (candidates + needed chunks) x chunk size of address space -- ~60 GB for the headline
 *     scan's 12.3 GB (24 candidate chunks of 2 GB + the arrays), at most ~140 GB -- a plain one only the arrays' size;
 *   * pfmscan_place_free(ptrs[0]) synchronises the device and RETIRES the set: it stays mapped, memory included, and the
 *     next pfmscan_place_alloc of the same sizes and flags returns it as it is (no new range, no measurement: an
 *     allocate / scan / free loop costs nothing after its first round).  The two most recently retired sets keep their
 *     memory; an older one is unmapped and its memory released at once (its ranges stay reserved).  pfmscan_place_trim
 *     releases the memory of every retired set now.  pfmscan_ctx_destroy releases all memory;
 *   * a context may reserve 16 TB in all (an eighth of the 47-bit user address space: ~270 measured allocations of the
 *     headline's size with DIFFERENT sizes each time); beyond that pfmscan_place_alloc returns PFMSCAN_E_OOM and says why. */
#define PFMSCAN_PLACE_PLAIN 1
int pfmscan_place_alloc(pfmscan_ctx *ctx, int n_arrays, const int64_t *bytes, void **ptrs, int flags);
int pfmscan_place_free(pfmscan_ctx *ctx, void *first_array);
int pfmscan_place_trim(pfmscan_ctx *ctx);
const char *pfmscan_place_note(const pfmscan_ctx *ctx);

/* ---- in-silico mutagenesis: every single-letter change scored in one pass -------------------------------------
 * No counterpart in the reference: it would write a mutated FASTA and scan again (pssm.search, rnascan.py:263), once per
 * variant.  Over a packed RNA stream (codes 0..3 = A, C, G, U; anything >= 4 is foreign here, whatever the table holds in
 * columns 4..7) and the letters part T [m][8] of a motif, m <= PFMSCAN_MAX_M:
 *   score(s | p->a)  the value pfmscan_scan_dev would write at window s if codes[p] were a: 0.0 (double), += T[k][code(s+k)]
 *                    for k ascending, every addition rounded, then (float) (_pwm.c:34-68); NaN when the window holds a
 *                    foreign code or a separator, or runs past n_pos
 *   cover(p)         the starts s with max(0, p-m+1) <= s <= min(p, n_pos-m)
 *   best[p][a]       the greatest non-NaN score(s | p->a) over cover(p), compared as float32, reported bit for bit; ties go
 *                    to the LOWEST start; where[p][a] = p - s of that window; no non-NaN window: NaN and -1.  Column
 *                    a = codes[p] is the unmutated best ("ref").  A position whose code is >= 4 has NaN / -1 in all four
 *                    columns: a foreign letter cannot be substituted, a separator is never bridged.
 * pfmscan_mutmap_dev writes d_best float [n_pos][4] and, unless NULL, d_where int8 [n_pos][4] (16-byte aligned device
 * pointers); asynchronous on `stream` (NULL = the ctx's), never synchronises.  pfmscan_mutmap_staged: the same over the
 * stream staged by pfmscan_stage, HOST outputs, synchronises.
 * A motif without a letters part, or wider than PFMSCAN_MAX_M, is PFMSCAN_E_BADSHAPE; a NULL that is not allowed
 * PFMSCAN_E_BADARG. */
int pfmscan_mutmap_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif, const uint8_t *d_codes, int64_t n_pos,
                       float *d_best, int8_t *d_where, void *stream);
int pfmscan_mutmap_staged(pfmscan_ctx *ctx, const pfmscan_motif *motif, float *best, int8_t *where);
/* Only the changes that create or destroy a site at threshold thr leave the device: for a != codes[p]
 *   gain <=> best[p][a] > thr and not best[p][ref] > thr;   loss <=> the reverse        (strict compares of the float32 with
 *   the double thr, as score > minscore everywhere in this header: NaN and -inf never pass; a NaN thr is PFMSCAN_E_BADARG)
 * An event is key = 4 p + a, the ref best and the alt best (its kind follows from the two).  _dev appends in no particular
 * order: d_ev_key int64 [capacity], d_ev_ref / d_ev_alt float [capacity], d_ev_count one uint64 the caller zeroes, afterwards
 * the TOTAL number of events (only the first `capacity` are stored), as pfmscan_hits_dev; asynchronous, never synchronises.
 * _staged returns them sorted by key; PFMSCAN_E_CAPACITY: *n_events holds the capacity that suffices, nothing was written
 * to the event arrays (as pfmscan_hits_host). */
int pfmscan_mutmap_events_dev(pfmscan_ctx *ctx, const pfmscan_motif *motif, const uint8_t *d_codes, int64_t n_pos,
                              double thr, int64_t capacity, int64_t *d_ev_key, float *d_ev_ref, float *d_ev_alt,
                              uint64_t *d_ev_count, void *stream);
int pfmscan_mutmap_events_staged(pfmscan_ctx *ctx, const pfmscan_motif *motif, double thr, int64_t capacity,
                                 int64_t *ev_key, float *ev_ref, float *ev_alt, int64_t *n_events);
/* A list of n_var variants (position, alt letter) x n_motifs letter tables of one width m (HOST double [n_motifs][m][8] as in
 * pfmscan_library_create; the call uploads them onto `stream` into scratch of the ctx).  For variant v and motif q:
 *   ref[v][q] = best[pos][codes[pos]], alt[v][q] = best[pos][alt] of motif q's map above, ref_where / alt_where their `where`
 *   (either may be NULL).  alt == codes[pos] is allowed (the ref columns twice).  A variant whose position holds a code >= 4,
 *   lies outside [0, n_pos) or has alt > 3 gets NaN / -1 for every motif and reads nothing out of bounds.
 * d_var_pos int64 [n_var], d_var_alt uint8 [n_var], d_ref / d_alt float [n_var][n_motifs], the where arrays int8 of the same
 * shape: device pointers for _dev (asynchronous, never synchronises; libraries that do not fit the LDS at once run as motif
 * chunks of one launch), host pointers and the staged stream for _staged.  NULL letter_tables or m outside
 * 1 .. PFMSCAN_MAX_M: PFMSCAN_E_BADSHAPE. */
int pfmscan_variants_dev(pfmscan_ctx *ctx, const double *letter_tables, int n_motifs, int m, const uint8_t *d_codes,
                         int64_t n_pos, const int64_t *d_var_pos, const uint8_t *d_var_alt, int64_t n_var,
                         float *d_ref, float *d_alt, int8_t *d_ref_where, int8_t *d_alt_where, void *stream);
int pfmscan_variants_staged(pfmscan_ctx *ctx, const double *letter_tables, int n_motifs, int m,
                            const int64_t *var_pos, const uint8_t *var_alt, int64_t n_var, float *ref, float *alt,
                            int8_t *ref_where, int8_t *alt_where);

/* ---- occupancy: the summed likelihood ratio of every record under every motif ------------------------------------
 * No counterpart in the reference.  Threshold-free: a records x motifs matrix instead of a table of hits.
 *   R [m][8]      ratio table of a motif of width m <= PFMSCAN_MAX_M over n_letters letters (4: RNA codes 0..3, 7:
 *                 structure-letter codes 0..6).  For a letter with normalised background b > 0 and normalised, pseudocounted
 *                 probability p: R = p / b if that quotient is > 0, else +0.0 (the cell whose log-odds is -inf); for b == 0:
 *                 +inf if p > 0, else NaN -- the operands of the log-odds cell before its log.  Columns >= n_letters are NaN
 *                 and never read.  Every cell is +0.0, positive, +inf or NaN; never negative, never -0.0.
 *   term(s)       t = R[0][c_0], then t = t * R[k][c_k] for k = 1 .. m-1, every product rounded to double, never fused with
 *                 the addition that follows; c_k = codes[s + k] & 7 (a lower-case structure letter carries bit 3 and counts
 *                 as its letter).  A window that holds a code >= n_letters has NO term: it adds +0.0 and is not counted.
 *                 Otherwise IEEE as it falls: subnormals stay, 0 x inf is NaN, NaN and +inf poison / saturate the sum.
 *   occ[r][q]     the terms of record r's n_win = max(L - m + 1, 0) windows in order (skipped ones as +0.0), summed in a
 *                 left-aligned tree of fan-in PFMSCAN_OCC_FANIN: element j of level l+1 is a[32 j], then + a[32 j + 1], ...
 *                 over the children that exist, sequential, ascending, each rounded; until one value is left; n_win = 0
 *                 gives +0.0.  The tree is anchored at the record's first window: the bits do not depend on where the
 *                 record lies in the stream, on the batch or on the launch geometry.
 *   windows[r]    the number of windows of record r that have a term (width and codes only, not the motif).
 * ratio_tables: HOST double [n_motifs][m][8], uploaded into scratch of the ctx by the call.  Records: rec_off / rec_len
 * int64 [n_rec], ascending and disjoint inside [0, n_pos) (else PFMSCAN_E_BADARG); occ double [n_rec][n_motifs]; windows
 * int64 [n_rec] or NULL.  pfmscan_occupancy_dev: device pointers (d_codes 16-byte aligned), on the ctx's stream; it reads
 * the record table back and checks it before anything is launched (one synchronisation), then returns without waiting for
 * the kernels (pfmscan_synchronize).  pfmscan_occupancy_staged: the stream left by pfmscan_stage (which = 0) or
 * pfmscan_stage_codes2 (which = 1), HOST record table and outputs, synchronises.  Device scratch for the partial sums is
 * bounded (256 MB of block sums, or one motif's block sums of the longest record if that is more): records, then motifs,
 * run in passes.  m outside 1 .. PFMSCAN_MAX_M: PFMSCAN_E_BADSHAPE; n_letters not 4 or 7, a NULL that is needed:
 * PFMSCAN_E_BADARG; n_rec == 0 or n_motifs == 0: PFMSCAN_OK, nothing written. */
#define PFMSCAN_OCC_FANIN 32
int pfmscan_occupancy_dev(pfmscan_ctx *ctx, const double *ratio_tables, int n_motifs, int m, int n_letters,
                          const uint8_t *d_codes, int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len,
                          int64_t n_rec, double *d_occ, int64_t *d_windows);
int pfmscan_occupancy_staged(pfmscan_ctx *ctx, int which, const double *ratio_tables, int n_motifs, int m, int n_letters,
                             const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *occ, int64_t *windows);

/* ---- occupancy on averaged-structure profiles: marginal ratios -------------------------------------------------------
 * The occupancy above for a stream whose structure is a profile r [n_pos][7] (float or double rows) instead of letters:
 * the expected odds of a window, not 2 ** (expected log-odds), which is what a structure scan's score gives.
 * No transcendental, no tolerance; tests/occupancy_profile_rules.py restates it in numpy and the bits are compared.
 *   S [m][7]      structure table of a motif of width m <= PFMSCAN_MAX_M: odds ratios as pssm.odds makes them (+0.0,
 *                 positive, +inf or NaN), the columns arranged on the host in the profile's STORED column order, exactly as
 *                 scanner.struct_matrix arranges a PSSM for --pairing aligned or positional.
 *   d(x, k)       the marginal of row x under motif row k: d = r[x][0] * S[k][0], then d = d + r[x][c] * S[k][c] for
 *                 c = 1 .. 6, ascending in stored column order.  Every product and every addition is rounded to double;
 *                 nothing is fused.  float rows are widened first (exact).  No nan_to_num, no validity check: IEEE as it
 *                 falls -- 0 x inf is NaN, a NaN or negative profile cell goes where arithmetic takes it.
 *   term(s)       structure only (seq_tables NULL): t = d(s, 0), then t = t * d(s + k, k) for k = 1 .. m-1, each product
 *                 rounded; the codes are not read and every window inside the record has a term.
 *                 joint (seq_tables R [m][8] over the 4 RNA letters): first the letter chain of the occupancy above,
 *                 t = R[0][c_0], then t = t * R[k][c_k]; then t = t * d(s + k, k) for k = 0 .. m-1.  A window that holds a
 *                 code >= 4 has no term.  This is the ratio behind LogOdds.SeqStruct.
 *   occ, windows  as above, unchanged: n_win = max(L - m + 1, 0) windows in order, skipped ones as +0.0, the left-aligned
 *                 tree of fan-in PFMSCAN_OCC_FANIN anchored at the record's first window; windows[r] = the windows with a term, n_win in structure-only mode.  The separator row behind
 *                 a record is never read as data.
 * Every term and partial sum is +0.0, positive, +inf or NaN whenever the rows are non-negative; where they are not, the
 * rules still define the result operation by operation.  The bits depend on the row dtype and on the stored column order
 * and on nothing else: not on the batch, the position in the stream, the launch geometry, the scratch cap or the staged /
 * _dev form.
 * struct_tables: HOST double [n_motifs][m][7]; seq_tables: HOST double [n_motifs][m][8] or NULL; both are uploaded into
 * scratch of the ctx by the call.  pfmscan_occupancy_profile_dev: d_profile (and d_codes in joint mode; otherwise it may be
 * NULL and is not read) are device pointers, 16-byte aligned (else PFMSCAN_E_BADSHAPE), profile_dtype PFMSCAN_PROFILE_F32 or
 * _F64; record table, the one synchronisation, outputs and the bounded scratch as for pfmscan_occupancy_dev.
 * pfmscan_occupancy_profile_staged: the profile (and codes) left by pfmscan_stage, HOST record table and outputs,
 * synchronises.  seq_tables without codes, no staged profile, a bad profile_dtype, a NULL that is needed: PFMSCAN_E_BADARG;
 * m outside 1 .. PFMSCAN_MAX_M: PFMSCAN_E_BADSHAPE; n_rec == 0 or n_motifs == 0: PFMSCAN_OK, nothing written. */
int pfmscan_occupancy_profile_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                  const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                                  const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_occ,
                                  int64_t *d_windows);
int pfmscan_occupancy_profile_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs,
                                     int m, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *occ,
                                     int64_t *windows);

/* ---- expected counts: the letters under every window, weighted by the window's likelihood ratio --------------------
 * No counterpart in the reference.  The E-step of motif refinement: per record and motif a matrix [m][8] of
 * expected letter counts per motif column, with no threshold.  No transcendental, no tolerance; tests/expect_rules.py
 * restates it in numpy and the bits are compared.  Everything not said here is the occupancy above, unchanged: the ratio
 * table R [m][8], n_letters 4 or 7, c_k = codes[s + k] & 7, and "a window that holds a foreign code has no term".
 *   t_s, has_s    the term of window s of record r and whether it has one, exactly as for the occupancy.
 *   occ_r         the record's occupancy under the motif: the bits pfmscan_occupancy_dev gives.
 *   w_s           the weight of window s.  PFMSCAN_EXPECT_RATIO: w_s = t_s.  PFMSCAN_EXPECT_POSTERIOR: v = 1.0 / occ_r, one
 *                 rounded division per record and motif, and w_s = t_s * v, one rounded product per window, never
 *                 contracted (a division per window would give other bits); if occ_r is +0.0 (no window with a term, or
 *                 every term zero) every w_s of the record is +0.0.  That rule and the skipped windows are the only special
 *                 cases: subnormals stay, inf and NaN propagate into the record's cells.
 *   E_r[k][c]     for k < m, c < n_letters: the values x_s = (has_s && (codes[s + k] & 7) == c) ? w_s : +0.0 over the
 *                 record's n_win = max(L - m + 1, 0) windows in order, summed in the occupancy's left-aligned tree of fan-in
 *                 PFMSCAN_OCC_FANIN anchored at the record's first window.  Columns c >= n_letters are +0.0; n_win = 0 gives
 *                 +0.0 everywhere.  The bits do not depend on the batch, on where the record lies in the stream, on the
 *                 launch geometry or on the scratch cap.
 * exp double [n_rec][n_motifs][m][8]; occ double [n_rec][n_motifs] or NULL: the occupancy, the same bits as
 * pfmscan_occupancy_*; windows int64 [n_rec] or NULL, as there.  ratio_tables, the record table and its check (a table that
 * is not ascending, disjoint and inside the stream: PFMSCAN_E_BADARG before any kernel forms an address from it, nothing
 * written), the one synchronisation of the _dev form, `which` of the _staged form and the error codes are those of
 * pfmscan_occupancy_dev / _staged; a mode other than the two: PFMSCAN_E_BADARG.  Device scratch is bounded as there: block
 * sums of blocks x (motifs x m x n_letters) doubles under the same cap, records, then cells and motifs, run in passes. */
#define PFMSCAN_EXPECT_RATIO 0
#define PFMSCAN_EXPECT_POSTERIOR 1
int pfmscan_expect_dev(pfmscan_ctx *ctx, const double *ratio_tables, int n_motifs, int m, int n_letters, int mode,
                       const uint8_t *d_codes, int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len,
                       int64_t n_rec, double *d_exp, double *d_occ, int64_t *d_windows);
int pfmscan_expect_staged(pfmscan_ctx *ctx, int which, const double *ratio_tables, int n_motifs, int m, int n_letters,
                          int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp, double *occ,
                          int64_t *windows);

/* ---- expected counts on averaged-structure profiles: weighted row sums ---------------------------------------------
 * No counterpart in the reference.  The expected counts above for a stream whose structure is a profile r [n_pos][7]: per
 * record and motif the weighted sum of the profile's ROWS under every motif column -- the threshold-free form
 * of what the site profiles sum under hits; on one-hot rows it is the letters' expected count.  (The posterior of the letter
 * given the motif, r * S / d, is a different quantity and is not computed.)  No transcendental, no tolerance;
 * tests/expect_profile_rules.py restates it in numpy and the bits are compared.  Everything not said here is the occupancy
 * on averaged-structure profiles and the expected counts above, unchanged: S [m][7] in the profile's STORED column order,
 * R [m][8] over the 4 RNA letters, the marginal d(x, k) of 7 rounded products and 6 rounded additions (float rows widened
 * first), the tree of fan-in PFMSCAN_OCC_FANIN anchored at the record's first window (the first value of a block is copied,
 * not added to zero; a lone window is the record's sum as it is; every level is padded with +0.0 as the rules pad it), the
 * two modes, v = 1.0 / occ_r (one rounded division per record and motif), w_s = t_s * v (one rounded product per window), and
 * "occ_r == 0.0 makes every weight of the record +0.0".
 *   t_s, has_s    by the tables that are given (both NULL: PFMSCAN_E_BADARG):
 *                 struct_tables only: the structure-only chain of marginals; every window inside the record has a term, the
 *                   codes are not read; occ, windows are the bits of pfmscan_occupancy_profile_* (structure only).
 *                 both: the joint chain -- the letters, then m marginals; a window with a code >= 4 has no term; occ, windows
 *                   are the bits of pfmscan_occupancy_profile_* (joint).
 *                 seq_tables only: the letter chain over the 4 RNA letters; occ, windows are the bits of
 *                   pfmscan_occupancy_* / pfmscan_expect_*.
 *   exp_struct    double [n_rec][n_motifs][m][8], always.  For k < m, c < 7 (stored column order): the values
 *                 x_s = has_s ? w_s * r[s + k][c] : +0.0, one rounded product each, over the record's n_win = max(L - m + 1, 0)
 *                 windows in order, summed in the tree.  Column 7 is +0.0; n_win = 0 gives +0.0 everywhere.
 *   exp_seq       double [n_rec][n_motifs][m][8] or NULL; only where seq_tables is given (else PFMSCAN_E_BADARG).  The cell of
 *                 the expected counts above, x_s = (has_s && (codes[s + k] & 7) == c) ? w_s : +0.0 for c < 4, with this call's
 *                 weights; with seq_tables alone, bit for bit what pfmscan_expect_dev returns.
 * No nan_to_num, no validity check: IEEE as it falls.  A negative or NaN profile cell goes where arithmetic takes it, and
 * w * (-0.0) keeps its sign into the tree.  The separator row behind a record is never read as data.  The bits depend on the
 * row dtype and the stored column order and on nothing else: not on the batch, the position in the stream, the launch
 * geometry, the scratch cap or the _dev / _staged form.
 * Pointers, alignment, the record table and its check (PFMSCAN_E_BADARG before any kernel forms an address from it, nothing
 * written), the one synchronisation of the _dev form and the error codes are those of pfmscan_occupancy_profile_* and
 * pfmscan_expect_*; d_profile is needed in every mode, d_codes where seq_tables is given.  A bad mode or profile_dtype:
 * PFMSCAN_E_BADARG, outputs untouched.  Device scratch is bounded as there: records, then matrix rows (the 7 + 4 cells of a
 * row (motif, k) stay together) and with them motifs, run in passes. */
int pfmscan_expect_profile_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                               int mode, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                               const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_exp_struct,
                               double *d_exp_seq, double *d_occ, int64_t *d_windows);
int pfmscan_expect_profile_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                  int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp_struct,
                                  double *exp_seq, double *occ, int64_t *windows);

/* The expected nucleotide x context table per column on averaged-structure profiles (added under ABI 27).  The two
 * matrices above are the margins of one table: per record r, motif (pair) q and motif column k, how much of structural context c
 * lies under nucleotide a.  An averaged row has no letter to pair the nucleotide with, so the cell sums the row's cell itself.
 * Everything not said here is the contract above, unchanged.
 *   exp_joint[r][q][k][a][c], a < 4, c < 7 (STORED column order)   over the record's windows in order, the tree sum of
 *                 x_s = (has_s && (codes[s + k] & 7) == a) ? w_s * r[s + k][c] : +0.0
 *                 -- the one rounded product exp_struct makes of the same window, never fused -- with w_s and has_s those of
 *                 exp_struct of the same call (joint chain with both tables, letter chain with seq_tables only).
 *                 double [n_rec][n_motifs][m][4][8], column c = 7 of every row +0.0: a matrix of 4 m rows (row k * 4 + a) of 7
 *                 letters, which is how the tree, the merge (acc_joint uint64 [n_motifs][PFMSCAN_SITE_LIMBS][32 m], cell
 *                 (k * 4 + a) * 8 + c) and the command take it.  The codes are read: without seq_tables PFMSCAN_E_BADARG.
 * Where every code of a record is one known nucleotide a0, exp_joint[..][k][a0][:] is bit for bit exp_struct[..][k][:] of the same
 * call and every other a is +0.0.  On rows with a single 1.0, finite positive tables and the identity column order the table is
 * bit for bit exp_joint of pfmscan_expect_pair_joint_* on the letter codes argmax(row).  The sum over a agrees with exp_struct
 * only to rounding: the tree adds other values.
 * The three functions carry the argument lists of pfmscan_expect_profile_dev / _staged / _merged_staged plus the table's output
 * behind the two matrices'; their checks, the order of the checks, messages and return codes are the namesakes', except that any
 * of the three outputs may be NULL (not computed: the bits of the others do not depend on it).  All three NULL, or exp_joint or
 * exp_seq without seq_tables: PFMSCAN_E_BADARG, outputs untouched, nothing launched.  Calls without the table run the same
 * kernels on the same plan as before.  The table is four matrices wide: 32 m doubles per record and motif on the device; the
 * caller bounds it by the records of a call.  Scratch: a matrix row (motif, k) takes 7 + 4 + 28 doubles of a block; a pass then
 * holds whole motifs, as many as leave room for the blocks that fill the device. */
int pfmscan_expect_profile_joint_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                     int mode, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                                     const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_exp_struct,
                                     double *d_exp_seq, double *d_exp_joint, double *d_occ, int64_t *d_windows);
int pfmscan_expect_profile_joint_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                        int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp_struct,
                                        double *exp_seq, double *exp_joint, double *occ, int64_t *windows);

/* ---- occupancy and expected counts of two code streams: sequence letters AND structure letters ------------------------
 * No counterpart in the reference.  The occupancy and the expected counts above for the input mode `-p seq.pfm -q struct.pfm
 * seqs.fa structs.fa`, where the structure of a record is a letter string.  No transcendental, no tolerance;
 * tests/pair_rules.py restates it in numpy and the bits are compared.  Everything not said here is the occupancy and the
 * expected counts above, unchanged: the cells of the tables, c = code & 7, the left-aligned tree of fan-in PFMSCAN_OCC_FANIN
 * anchored at the record's first window, v = 1.0 / occ_r (one rounded division per record and pair), w_s = t_s * v (one
 * rounded product per window), "occ_r == +0.0 makes every weight +0.0", IEEE as it falls, nothing contracted.
 * Two streams of equal length n_pos share one record table: codes holds RNA codes (n_letters 4), codes2 structure-letter
 * codes (n_letters 7; a lower-case structure letter carries bit 3 and counts as its letter).  seq_tables R and struct_tables
 * S are HOST double [n_motifs][m][8], both made as the ratio table of the occupancy is made; pair q is (R_q, S_q), both of
 * width m.
 *   term(s)       t = R[0][a_0], then t = t * R[k][a_k] for k = 1 .. m-1, then t = t * S[k][b_k] for k = 0 .. m-1, where
 *                 a_k = codes[s + k] & 7 and b_k = codes2[s + k] & 7: 2 m - 1 rounded products, the letters first, then the
 *                 structure -- the order of the joint chain on averaged-structure profiles.  R[k][a] * S[k][b] is never
 *                 made on its own: a pre-multiplied 28-entry row is another rounding and not this contract.
 *   has(s)        every a_k < 4 and every b_k < 7.  Otherwise the window has no term: it adds +0.0 and is not counted.
 *   occ[r][q], windows[r]   as for the occupancy, over these terms.
 *   exp_seq[r][q][k][c], c < 4      the tree sum of (has_s && a_k == c) ? w_s : +0.0.
 *   exp_struct[r][q][k][c], c < 7   the tree sum of (has_s && b_k == c) ? w_s : +0.0.
 *                 Both matrices are double [n_rec][n_motifs][m][8], the other columns +0.0.  Either pointer may be NULL (that
 *                 matrix is not computed); both NULL: PFMSCAN_E_BADARG.
 * Exact multiplication by 1.0 gives two identities: with every cell of S equal to 1.0 and no foreign structure code, occ,
 * windows and exp_seq are bit for bit those of pfmscan_occupancy_* / pfmscan_expect_* on codes; with every cell of R equal to
 * 1.0 and no foreign sequence code, occ, windows and exp_struct are those of the single-stream calls on codes2 with
 * n_letters 7.  The bits depend on the codes and the tables and on nothing else: not on the batch, the record's place in the
 * stream, the launch geometry, the scratch cap or the _dev / _staged form.
 * The _dev forms take device pointers, both code streams 16-byte aligned (else PFMSCAN_E_BADSHAPE), on the ctx's stream; they
 * read the record table back and check it before any kernel forms an address from it (one synchronisation; a table that is
 * not ascending, disjoint and inside the stream: PFMSCAN_E_BADARG, nothing written), then return without waiting.  The
 * _staged forms read the streams left by pfmscan_stage and pfmscan_stage_codes2, take a HOST record table and outputs, and
 * synchronise.  A missing staged stream, a NULL that is needed or a bad mode: PFMSCAN_E_BADARG, outputs untouched; m outside
 * 1 .. PFMSCAN_MAX_M: PFMSCAN_E_BADSHAPE; n_rec == 0 or n_motifs == 0: PFMSCAN_OK, nothing written.  Device scratch is bounded
 * as above: records, then pairs (occupancy) or matrix rows (expected counts; the 4 + 7 cells of a row (pair, k) stay
 * together), run in passes. */
int pfmscan_occupancy_pair_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                               const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                               const int64_t *d_rec_len, int64_t n_rec, double *d_occ, int64_t *d_windows);
int pfmscan_occupancy_pair_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                  const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *occ, int64_t *windows);
int pfmscan_expect_pair_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                            const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                            const int64_t *d_rec_len, int64_t n_rec, double *d_exp_seq, double *d_exp_struct, double *d_occ,
                            int64_t *d_windows);
int pfmscan_expect_pair_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                               int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp_seq,
                               double *exp_struct, double *occ, int64_t *windows);

/* The expected letter-PAIR table per column (ABI 27).  The two matrices above are the margins of one table: per record r, pair q
 * and motif column k, how often nucleotide a lies over structure letter b under the weights.  It is neither the outer product of
 * the margins nor anything a thresholded command writes.  Everything not said here is the contract above, unchanged.
 *   exp_joint[r][q][k][a][b], a < 4, b < 7   the tree sum of (has_s && a_k == a && b_k == b) ? w_s : +0.0.
 *                 double [n_rec][n_motifs][m][4][8], column b = 7 of every row +0.0: a matrix of 4 m rows (row k * 4 + a) and 7
 *                 letters per pair, which is how the tree, the merge below (rows 4 m, acc_joint uint64 [n_motifs]
 *                 [PFMSCAN_SITE_LIMBS][32 m]) and the commands take it.
 * Where every code of codes2 in a record is one known letter b0, exp_joint[..][k][a][b0] is bit for bit exp_seq[..][k][a] (the
 * same windows in the same tree) and every other b is +0.0; the same with a constant nucleotide a0 against exp_struct.  With
 * every cell of R and S equal to 1.0, PFMSCAN_EXPECT_RATIO and no foreign code the table is the integer count of letter pairs
 * under every window: what pfmscan_site_joint_* counts when every window start is a hit.
 * The three functions carry the argument lists of pfmscan_expect_pair_dev / _staged / _merged_staged plus the table's output
 * behind the two matrices'; their checks, the order of the checks, messages and return codes are the namesakes'.  Any of the three
 * outputs may be NULL (not computed: the bits of the others do not depend on it); all three NULL: PFMSCAN_E_BADARG.  The table is
 * four matrices wide: 32 m doubles per record and pair on the device (3.2 GB for 4096 records x 256 pairs at m = 12); the caller
 * bounds it by the records of a call. */
int pfmscan_expect_pair_joint_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                  int mode, const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                                  const int64_t *d_rec_len, int64_t n_rec, double *d_exp_seq, double *d_exp_struct,
                                  double *d_exp_joint, double *d_occ, int64_t *d_windows);
int pfmscan_expect_pair_joint_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                     int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp_seq,
                                     double *exp_struct, double *exp_joint, double *occ, int64_t *windows);

/* ---- expected counts: the records added up on the device -------------------------------------------------------------------
 * No counterpart in the reference.  The three families of expected counts above leave one matrix [m][8] per record and motif;
 * a refinement step wants their sum over the records, which the commands used to make on the host with math.fsum.  These
 * entry points make the same sum on the device, exactly, in the LONG ACCUMULATOR of "site profiles of a library" above: its
 * layout (limbs the slow index inside a motif), its decomposition of a double into three 32-bit pieces
 * (rnascan_amd/csrc/pfmscan_superacc.hpp), its headroom rule, RAW and NORMALISED, and the host helpers pfmscan_site_acc_add /
 * _round / _from_doubles are used as they stand, with m * 8 cells per motif where a site profile has W * 7.  A sum of finite
 * doubles >= 0 held exactly and rounded once IS math.fsum of them: pfmscan_site_acc_round of these accumulators is bit for bit
 * what math.fsum gives cell by cell over the records; tests/expect_merge_rules.py restates it in Python ints.
 * Integer additions do not depend on their order: 64-bit integer atomics, no float atomics, no tolerance.
 *   d_exp   DEVICE double [n_rec][n_motifs][m][8]: what pfmscan_expect_dev, pfmscan_expect_profile_dev or
 *           pfmscan_expect_pair_dev wrote, either of their matrices.
 *   d_acc   DEVICE uint64 [n_motifs][PFMSCAN_SITE_LIMBS][m * 8]; cell e = 8 k + c of motif q is sum_i d_acc[q][i][e] * 2^(32 i).
 *   d_bad   DEVICE int64 [n_motifs][2]: [q][0] the smallest record index of this call with a NaN or +-inf cell of motif q,
 *           [q][1] the smallest with a cell < 0 (-inf is both); -1: none.
 *   zero_first != 0: d_acc is zeroed and d_bad set to -1 first.  zero_first == 0: the call adds to what is there, so the batches
 *           of a pass accumulate on the device and nothing goes home in between; an entry of d_bad that is >= 0 already stays
 *           if it is the smaller one.  The caller keeps the records of one accumulator below 2^31; the sums are left RAW.
 *   Cells   a NaN, +-inf or negative cell is never decomposed: it adds nothing and only sets d_bad.  +0.0 and -0.0 add nothing,
 *           and -0.0 is not negative (math.fsum([-0.0]) is 0.0).  Every other cell is added exactly.
 * pfmscan_expect_merge_dev is asynchronous on the ctx's stream and does not synchronise.  A NULL that is needed (d_acc, d_bad
 * with n_motifs > 0; d_exp with records too), a negative size or n_rec >= 2^31: PFMSCAN_E_BADARG; m outside 1 .. PFMSCAN_MAX_M:
 * PFMSCAN_E_BADSHAPE; n_rec == 0 or n_motifs == 0: PFMSCAN_OK, after zeroing if asked.
 *
 * _merged_staged: the _staged form of the same name with its matrices replaced by accumulators.  The pass runs into the ctx's
 * scratch as before, the merge runs over that scratch, and only the accumulators, bad, occ and windows come home.
 *   acc*    HOST uint64 [n_motifs][PFMSCAN_SITE_LIMBS][m * 8], NORMALISED in and out: this call's sums are ADDED with the
 *           arithmetic of pfmscan_site_acc_add (a top limb that overflows: PFMSCAN_E_BADSHAPE).  Zero them once, call per batch.
 *   bad*    HOST int64 [n_motifs][2] of THIS call: indices into this call's record table.
 *   occ, windows   as in the form each one mirrors, bit for bit; either may be NULL.
 * Which pointers are needed, the error codes and the order of the checks are those of the mirrored form, an accumulator where
 * it takes a matrix; an accumulator that is given needs its bad (PFMSCAN_E_BADARG).  pfmscan_expect_profile_merged_staged
 * takes acc_seq only with seq_tables; pfmscan_expect_pair_merged_staged takes either accumulator or both.  n_rec == 0 or
 * n_motifs == 0: PFMSCAN_OK, nothing written. */
int pfmscan_expect_merge_dev(pfmscan_ctx *ctx, const double *d_exp, int64_t n_rec, int n_motifs, int m, int zero_first,
                             uint64_t *d_acc, int64_t *d_bad);
int pfmscan_expect_merged_staged(pfmscan_ctx *ctx, int which, const double *ratio_tables, int n_motifs, int m, int n_letters,
                                 int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, uint64_t *acc,
                                 int64_t *bad, double *occ, int64_t *windows);
int pfmscan_expect_profile_merged_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs,
                                         int m, int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                                         uint64_t *acc_struct, uint64_t *acc_seq, int64_t *bad_struct, int64_t *bad_seq,
                                         double *occ, int64_t *windows);
int pfmscan_expect_pair_merged_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                      int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, uint64_t *acc_seq,
                                      uint64_t *acc_struct, int64_t *bad_seq, int64_t *bad_struct, double *occ, int64_t *windows);
/* with the letter-pair table (ABI 27): acc_joint HOST uint64 [n_motifs][PFMSCAN_SITE_LIMBS][32 m], cell (k * 4 + a) * 8 + b */
int pfmscan_expect_pair_joint_merged_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs,
                                            int m, int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                                            uint64_t *acc_seq, uint64_t *acc_struct, uint64_t *acc_joint, int64_t *bad_seq,
                                            int64_t *bad_struct, int64_t *bad_joint, double *occ, int64_t *windows);
/* with the nucleotide x context table of averaged-structure profiles: acc_joint as above, cell (k * 4 + a) * 8 + c, c in the
 * profile's STORED column order; any of the three accumulators may be NULL, not all */
int pfmscan_expect_profile_joint_merged_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs,
                                               int m, int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                                               uint64_t *acc_struct, uint64_t *acc_seq, uint64_t *acc_joint, int64_t *bad_struct,
                                               int64_t *bad_seq, int64_t *bad_joint, double *occ, int64_t *windows);

/* ---- posterior site map: the weight of every window and the coverage of every position ---------------------------------
 * No counterpart in the reference.  The fourth member of the threshold-free family: where in a record the
 * binding is, per position, without a threshold -m.  No transcendental, no tolerance; tests/footprint_rules.py restates it in
 * numpy and the bits are compared.  Everything not said here is the occupancy, the expected counts and the two-stream contract
 * above, unchanged: the ratio tables, c = code & 7, the term chain (letters first, then structure letters, 2 m - 1 rounded
 * products, never a pre-multiplied row), has_s, occ_r and windows[r], the weights (v = 1.0 / occ_r one rounded division per
 * record and motif, w_s = t_s * v one rounded product per window; occ_r == +0.0 makes every weight +0.0),
 * PFMSCAN_EXPECT_RATIO / _POSTERIOR, IEEE as it falls, nothing contracted.
 * Two maps per motif (or pair) q, each a plane double [n_motifs][n_pos] aligned with the stream; record r lies at off_r with
 * L positions and n_win = max(L - m + 1, 0) windows:
 *   start[q][off_r + s] = w_s for 0 <= s < n_win, +0.0 for the record's last min(m - 1, L) positions; a window without a term
 *                 is +0.0, as its weight already is.
 *   cover[q][off_r + i] for 0 <= i < L: c = +0.0, then for s = i - m + 1 .. i ascending c = c + (0 <= s < n_win ? w_s : +0.0),
 *                 every addition rounded and sequential: no sliding-window update (another rounding), no tree (at most
 *                 m <= 64 terms).  Weights are never -0.0, so the absent terms added as +0.0 change nothing.  In posterior mode
 *                 cover is P(position under the site | one site per record).
 * One argument list serves the three letter inputs: seq_tables alone (struct_tables NULL) reads d_codes over the 4 RNA
 * letters and never d_codes2; struct_tables alone reads d_codes2 over the 7 structure letters and never d_codes; both are the
 * pair.  A single-table call's weights are bit for bit those of pfmscan_expect_* on that stream; occ and windows those of
 * pfmscan_occupancy_* (or _pair_*).  The bits depend on the codes and the tables and on nothing else: not on the batch, the
 * record's place in the stream, the tiling, the launch geometry, whether the other map was asked for, or the _dev, _staged or
 * events form.
 * Maps: d_start or d_cover may be NULL (not computed), not both (PFMSCAN_E_BADARG); occ double [n_rec][n_motifs] and windows
 * int64 [n_rec] may be NULL.  In the _dev form positions that lie in no record of the table (separators, gaps, records the
 * table skips) are NOT written; in the _staged form they are +0.0.  The caller bounds the 16 * n_motifs * n_pos bytes of the
 * planes by the motifs and records of a call.
 * Events: a position with cover > thr (strict; NaN never passes; a NaN thr is PFMSCAN_E_BADARG) is key = q * n_pos + p with its
 * cover and its start.  The decision is taken in the kernel that makes cover: no plane is allocated anywhere.  Capacity, the
 * total count in d_ev_count (one uint64 the caller zeroes; only the first `capacity` events are stored), "unordered in _dev,
 * sorted by key in _staged" and "PFMSCAN_E_CAPACITY: *n_events holds the capacity that suffices, nothing was written" are
 * exactly those of pfmscan_mutmap_events_*.
 * The record-table check (before any kernel forms an address from it), the one synchronisation of the _dev forms, the error
 * codes, the order of the checks and the 16-byte alignment of the streams are those of pfmscan_expect_pair_*; the tables that
 * are given decide which streams are needed; both tables NULL: PFMSCAN_E_BADARG.
 * PFMSCAN_FOOTPRINT_SLOTS: a workgroup of the level-0 kernel makes this many consecutive windows of ONE record; its tile is
 * the last PFMSCAN_FOOTPRINT_SLOTS - (m - 1) of them as positions, the first m - 1 are the halo it makes again. */
#define PFMSCAN_FOOTPRINT_SLOTS 512
int pfmscan_footprint_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                          const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                          const int64_t *d_rec_len, int64_t n_rec, double *d_start, double *d_cover, double *d_occ,
                          int64_t *d_windows);
int pfmscan_footprint_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                             const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *start, double *cover,
                             double *occ, int64_t *windows);
int pfmscan_footprint_events_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                 int mode, const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos,
                                 const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double thr, int64_t capacity,
                                 int64_t *d_ev_key, double *d_ev_cover, double *d_ev_start, uint64_t *d_ev_count, double *d_occ,
                                 int64_t *d_windows);
int pfmscan_footprint_events_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                    int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double thr,
                                    int64_t capacity, int64_t *ev_key, double *ev_cover, double *ev_start, int64_t *n_events,
                                    double *occ, int64_t *windows);

/* ---- posterior site map on averaged-structure profiles -------------------------------------------------------------------
 * The two maps above for the project's main input (DESIGN.md 5l "on averaged-structure profiles"); entry points ADDED under
 * ABI 27.  tests/footprint_profile_rules.py composes the rule from the family's and the bits are compared.
 * Term and has: those of pfmscan_occupancy_profile_*, unchanged.  struct_tables HOST double [n_motifs][m][7] in the profile's
 * STORED column order, required (NULL: PFMSCAN_E_BADARG -- sequence weights over a profile's records are pfmscan_footprint_* on
 * the codes); the marginal of a row is 7 rounded products and 6 rounded additions, ascending, float rows widened first;
 * structure only every window inside the record has a term and the codes are not read; seq_tables HOST double [n_motifs][m][8]
 * or NULL chooses joint mode and then needs the codes: the letter chain first, then t = t * d(s + k, k) for k = 0 .. m - 1, and
 * a window that holds a code >= 4 has no term.  No nan_to_num, no validity check: negative cells, NaN and 0 * inf go where the
 * arithmetic takes them.  occ_r and windows[r] are the bits of pfmscan_occupancy_profile_* for the same tables.
 * Weight: that of pfmscan_expect_profile_*: the term (PFMSCAN_EXPECT_RATIO) or t_s * v, v = 1.0 / occ_r one rounded division
 * (PFMSCAN_EXPECT_POSTERIOR); occ_r == 0.0 makes every weight +0.0.  A NEGATIVE occ_r (negative cells are legal) does not: the
 * weights are t_s * v with v negative.
 * Maps: start and cover as above, with one difference in the wording: a weight here CAN be -0.0 or negative, and cover is
 * c = +0.0, then c = c + (0 <= s < n_win && has_s ? w_s : +0.0) for s = i - m + 1 .. i ascending with all m additions made and
 * rounded.  The separator row behind a record and the rows of its neighbours are never used as data.  The bits depend on the
 * row dtype, the stored column order, the codes and the tables and on nothing else: not on the batch, the record's place in
 * the stream, the tiling, which plane was asked for, or the form.
 * Everything else comes from an existing entry point.  From pfmscan_occupancy_profile_* / pfmscan_expect_profile_*: the checks
 * of the width, the profile_dtype, the mode and the sizes, their order and codes; "no profile is staged"; the 16-byte alignment
 * of d_profile (and d_codes in joint mode, PFMSCAN_E_BADSHAPE); the record table read back and checked before any kernel forms
 * an address from it (the one synchronisation of the _dev forms).  From pfmscan_footprint_*: both planes NULL and a NaN thr are
 * PFMSCAN_E_BADARG; the event buffers, key = q * n_pos + p, the capacity verdict, "unordered in _dev, sorted by key in
 * _staged"; positions in no record are unwritten in _dev and +0.0 in _staged.  n_rec == 0 or n_motifs == 0: PFMSCAN_OK, nothing
 * written.  Bad arguments launch nothing and leave the outputs untouched.
 * PFMSCAN_FOOTPRINT_PROFILE_SLOTS: a workgroup of the level-0 kernel makes this many consecutive windows of ONE record; its
 * tile is the last PFMSCAN_FOOTPRINT_PROFILE_SLOTS - (m - 1) of them as positions. */
#define PFMSCAN_FOOTPRINT_PROFILE_SLOTS 256
int pfmscan_footprint_profile_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                  int mode, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                                  const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_start,
                                  double *d_cover, double *d_occ, int64_t *d_windows);
int pfmscan_footprint_profile_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                     int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *start,
                                     double *cover, double *occ, int64_t *windows);
int pfmscan_footprint_profile_events_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs,
                                         int m, int mode, const uint8_t *d_codes, const void *d_profile, int profile_dtype,
                                         int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec,
                                         double thr, int64_t capacity, int64_t *d_ev_key, double *d_ev_cover, double *d_ev_start,
                                         uint64_t *d_ev_count, double *d_occ, int64_t *d_windows);
int pfmscan_footprint_profile_events_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs,
                                            int m, int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                                            double thr, int64_t capacity, int64_t *ev_key, double *ev_cover, double *ev_start,
                                            int64_t *n_events, double *occ, int64_t *windows);

/* ---- threshold-free mutagenesis: the occupancy change of every single-letter change --------------------------------------
 * No counterpart in the reference.  Where pfmscan_mutmap_* says what a letter change does to the best window at a threshold,
 * this says what it does to the SUM the threshold-free family reports; entry points ADDED under ABI 27.
 * tests/mutocc_rules.py restates the rule in numpy and the bits are compared.  seq_tables HOST double [n_motifs][m][8] of one
 * width, the ratio tables of pfmscan_occupancy_* over the 4 RNA letters; c = code & 7; record r lies at off_r with L positions.
 * The map, double [n_motifs][n_pos][4] aligned with the stream: for a position p = off_r + i whose code is a letter
 * (c_i < 4) and a letter a in 0 .. 3
 *   local[q][p][a]: x = +0.0, then for s = i - m + 1 .. i ascending x = x + u(s), every addition rounded; u(s) = +0.0 when
 *                 s < 0, s > L - m, or any OTHER position of window s holds a code >= 4; else the term of window s of the
 *                 stream in which position i holds a, made as the occupancy makes it: R[0][.], then * R[k][.] for k ascending,
 *                 every product rounded (the factors before i are shared by the four letters; the tail is multiplied per
 *                 letter left to right, never a suffix product).  IEEE as it falls, nothing contracted, no exp, no log.
 * local[q][p][c_i] is bit for bit the cover of pfmscan_footprint_* in PFMSCAN_EXPECT_RATIO mode on the same stream and table,
 * and local[q][p][a] that cover at p of the stream with a written at p.  A position inside a record whose code is >= 4 has
 * four NaN, as pfmscan_mutmap_* has.  In the _dev form positions in no record of the table are NOT written; in the _staged
 * form they are NaN.  d_local is 16-byte aligned (PFMSCAN_E_BADSHAPE) and required; occ double [n_rec][n_motifs] and windows
 * int64 [n_rec] are those of pfmscan_occupancy_* and may be NULL.
 * Events: with occ_r the record's occupancy under q, delta = local[a] - local[c_i] (one rounded subtraction) and
 * lim = frac * occ_r (one rounded product), a != c_i is an event when delta > lim (gain) or delta < -lim (loss), both strict:
 * NaN never passes.  A NaN or negative frac is PFMSCAN_E_BADARG.  An event is key = (q * n_pos + p) * 4 + a with
 * alt = local[q][p][a] and ref = local[q][p][c_i]; no map is allocated anywhere.  Capacity, the total count in d_ev_count
 * (one uint64 the caller zeroes; only the first `capacity` events are stored), "unordered in _dev, sorted by key in _staged"
 * and "PFMSCAN_E_CAPACITY: *n_events holds the capacity that suffices, nothing was written" are exactly those of
 * pfmscan_mutmap_events_*.
 * The record-table check (before any kernel forms an address from it), the one synchronisation of the _dev forms, the error
 * codes, the order of the checks and the 16-byte alignment of d_codes are those of pfmscan_footprint_*.  The bits depend on
 * the codes and the tables and on nothing else: not on the batch, the tiling, the width's kernel or the form.
 * PFMSCAN_MUTOCC_TILE: a workgroup of the kernel owns this many consecutive positions of ONE record. */
#define PFMSCAN_MUTOCC_TILE 512
int pfmscan_mutocc_dev(pfmscan_ctx *ctx, const double *seq_tables, int n_motifs, int m, const uint8_t *d_codes, int64_t n_pos,
                       const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_local, double *d_occ,
                       int64_t *d_windows);
int pfmscan_mutocc_staged(pfmscan_ctx *ctx, const double *seq_tables, int n_motifs, int m, const int64_t *rec_off,
                          const int64_t *rec_len, int64_t n_rec, double *local, double *occ, int64_t *windows);
int pfmscan_mutocc_events_dev(pfmscan_ctx *ctx, const double *seq_tables, int n_motifs, int m, const uint8_t *d_codes, int64_t n_pos,
                              const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double frac, int64_t capacity,
                              int64_t *d_ev_key, double *d_ev_alt, double *d_ev_ref, uint64_t *d_ev_count, double *d_occ,
                              int64_t *d_windows);
int pfmscan_mutocc_events_staged(pfmscan_ctx *ctx, const double *seq_tables, int n_motifs, int m, const int64_t *rec_off,
                                 const int64_t *rec_len, int64_t n_rec, double frac, int64_t capacity, int64_t *ev_key,
                                 double *ev_alt, double *ev_ref, int64_t *n_events, double *occ, int64_t *windows);

/* ---- multi-site model: the partition function over non-overlapping sites and its site posteriors -----------------------
 * No counterpart in the reference.  The family above rests on one site per record (the weights) or adds overlapping windows as
 * if all were bound at once (the occupancy).  Here a record holds ANY set of non-overlapping sites, the empty set included
 * (DESIGN.md 5n); entry points ADDED under ABI 27.  tests/multisite_rules.py restates the rule in numpy and the bits are
 * compared.  The tables, c = code & 7, the term chain t_s over one or two code streams, has_s and windows[r] are those of
 * pfmscan_footprint_*, unchanged; a window without a term has t_s = +0.0.  lam double [n_rec]: the activity of a site in
 * record r.  Record r has L positions, n_win = max(L - m + 1, 0) windows.  Every product and addition below is ONE rounded
 * fp64 operation, nothing is contracted, there is no exp and no log, IEEE as it falls:
 *   a_s     = t_s * lam_r                                                    (one product after the chain)
 *   F[0]    = 1.0;  F[i] = F[i-1] + (i >= m ? a[i-m] * F[i-m] : +0.0)        for i = 1 .. L;   z = F[L]  (1.0 when L < m)
 *   B[L]    = 1.0;  B[i] = B[i+1] + (i <= L - m ? a[i] * B[i+m] : +0.0)      for i = L - 1 .. 0
 *   v       = 1.0 / z                                                        (one rounded division per record and motif)
 *   start[q][off_r + s] = ((F[s] * a[s]) * B[s+m]) * v for 0 <= s < n_win, +0.0 for the record's last min(m - 1, L) positions
 *   cover[q][off_r + i]: the m ascending rounded additions of pfmscan_footprint_* over start; sites of one configuration do
 *                 not overlap, so it is P(position i is bound)
 *   nsites  = +0.0, then nsites = nsites + start[s] for s = n_win - 1 DOWN TO 0: the expected number of sites
 * No scaling: z <= prod (1 + a_s) overflows on long records with a large lam; an infinite or NaN z is returned as IEEE makes
 * it and the caller decides.  The bits depend on the codes, the tables and lam_r and on nothing else: not on the batch, the
 * record's place in the stream, its neighbours, the passes, which outputs were asked for, or the _dev, _staged or events form.
 * The argument list is that of pfmscan_footprint_* without mode, with lam (a DEVICE pointer in the _dev forms, a HOST pointer
 * in the _staged forms; NULL: PFMSCAN_E_BADARG, tested after the sizes) behind the record table.  d_start or d_cover may be
 * NULL, not both; z, nsites double [n_rec][n_motifs] and windows int64 [n_rec] may be NULL.  Positions in no record: unwritten
 * in _dev, +0.0 in _staged.  Events: the positions with cover > thr; key, capacity, the counter, "unordered in _dev, sorted in
 * _staged" and the capacity verdict are those of pfmscan_footprint_events_*.  The checks, their order, the record-table check
 * before any kernel forms an address from it (the one synchronisation of the _dev forms) and the alignment rules are those of
 * pfmscan_footprint_*.  Scratch: 16 bytes per position and motif of a pass; the library plans records and motifs into passes.
 * PFMSCAN_MULTISITE_SLOTS: the tile-parallel kernels' workgroup holds this many windows of ONE record; its tile is
 * PFMSCAN_MULTISITE_SLOTS - (m - 1) positions.  PFMSCAN_MULTISITE_CHUNK: the positions of a record a lane of the two serial
 * kernels holds in LDS at a time. */
#define PFMSCAN_MULTISITE_SLOTS 512
#define PFMSCAN_MULTISITE_CHUNK 28
int pfmscan_multisite_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                          const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                          const int64_t *d_rec_len, int64_t n_rec, const double *d_lam, double *d_start, double *d_cover, double *d_z,
                          double *d_nsites, int64_t *d_windows);
int pfmscan_multisite_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                             const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, const double *lam, double *start,
                             double *cover, double *z, double *nsites, int64_t *windows);
int pfmscan_multisite_events_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                 const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                                 const int64_t *d_rec_len, int64_t n_rec, const double *d_lam, double thr, int64_t capacity,
                                 int64_t *d_ev_key, double *d_ev_cover, double *d_ev_start, uint64_t *d_ev_count, double *d_z,
                                 double *d_nsites, int64_t *d_windows);
int pfmscan_multisite_events_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                    const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, const double *lam, double thr,
                                    int64_t capacity, int64_t *ev_key, double *ev_cover, double *ev_start, int64_t *n_events,
                                    double *z, double *nsites, int64_t *windows);

/* ---- multi-site model on averaged-structure profiles ------------------------------------------------------------------------
 * The model above for the project's main input (DESIGN.md 5n "on averaged-structure profiles"); entry points ADDED under ABI 27.
 * tests/multisite_profile_rules.py composes the rule from the family's and the bits are compared.
 * Term and has: those of pfmscan_occupancy_profile_* / pfmscan_footprint_profile_*, unchanged.  struct_tables HOST double
 * [n_motifs][m][7] in the profile's STORED column order, required (NULL: PFMSCAN_E_BADARG -- the model of a profile's letters is
 * pfmscan_multisite_* on the codes); the marginal of a row is 7 rounded products and 6 rounded additions, ascending, float rows
 * widened first; structure only every window inside the record has a term and the codes are not read; seq_tables HOST double
 * [n_motifs][m][8] or NULL chooses joint mode and then needs the codes: the letter chain first, then t = t * d(s + k, k) for
 * k = 0 .. m - 1, and a window that holds a code >= 4 has no term (t_s = +0.0).  windows[r]: the windows with a term.
 * Model: a_s = t_s * lam_r, F, B, z, v, start, cover and nsites exactly as pfmscan_multisite_* states them, the same kernels
 * over the same plane of activities.  No nan_to_num, no validity check: profile cells may be negative or not finite, and z,
 * start and cover are then what IEEE makes of the stated operations -- z can be <= 0.0, infinite or NaN, and the caller
 * decides.  The separator row behind a record and the rows of its neighbours are never used as data.  The bits depend on the
 * row dtype, the stored column order, the codes, the tables and lam_r and on nothing else: not on the batch, the record's place
 * in the stream, the tiling, the passes, which outputs were asked for, or the form.
 * The argument list is that of pfmscan_footprint_profile_* without mode, with lam double [n_rec] behind the record table (a
 * DEVICE pointer in the _dev forms, a HOST pointer in the _staged forms).  The checks of the width, the profile_dtype and the
 * sizes, their order and codes, "no profile is staged", the 16-byte alignment of d_profile (and d_codes in joint mode,
 * PFMSCAN_E_BADSHAPE) and the record table read back and checked before any kernel forms an address from it (the one
 * synchronisation of the _dev forms) are those of pfmscan_footprint_profile_*.  A NULL lam is PFMSCAN_E_BADARG, tested after
 * the sizes and struct_tables; d_start or d_cover may be NULL, not both (PFMSCAN_E_BADARG); z, nsites double [n_rec][n_motifs]
 * and windows int64 [n_rec] may be NULL; a NaN thr, the event buffers, key = q * n_pos + p, the capacity verdict and "unordered
 * in _dev, sorted by key in _staged" are those of pfmscan_multisite_events_*.  Positions in no record: unwritten in _dev, +0.0
 * in _staged.  n_rec == 0 or n_motifs == 0: PFMSCAN_OK, nothing written.  Bad arguments launch nothing and leave the outputs
 * untouched.  Scratch and passes: those of pfmscan_multisite_*. */
int pfmscan_multisite_profile_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                  const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                                  const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, const double *d_lam,
                                  double *d_start, double *d_cover, double *d_z, double *d_nsites, int64_t *d_windows);
int pfmscan_multisite_profile_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                     const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, const double *lam,
                                     double *start, double *cover, double *z, double *nsites, int64_t *windows);
int pfmscan_multisite_profile_events_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs,
                                         int m, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                                         const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, const double *d_lam,
                                         double thr, int64_t capacity, int64_t *d_ev_key, double *d_ev_cover, double *d_ev_start,
                                         uint64_t *d_ev_count, double *d_z, double *d_nsites, int64_t *d_windows);
int pfmscan_multisite_profile_events_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs,
                                            int m, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                                            const double *lam, double thr, int64_t capacity, int64_t *ev_key, double *ev_cover,
                                            double *ev_start, int64_t *n_events, double *z, double *nsites, int64_t *windows);

#ifdef __cplusplus
}
#endif
#endif /* PFMSCAN_H */
