/*
 * wfa_hip.h — C ABI of the MI355X-native batched wavefront aligner (libwfa_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of kcleal/pywfa: the calls that
 * pywfa's Cython host (pywfa/align.pyx) makes into the vendored WFA2-lib, i.e.
 *
 *   wavefront_aligner_new(&attributes)                       align.pyx:344,419   wfa.h:125-126
 *   wavefront_align(aligner, pattern, plen, text, tlen)      align.pyx:439       wfa.h:199-204
 *   wavefront_align_lambda(...)  (wildcard matching)         align.pyx:441-442   wfa.h:205-210
 *   wavefront_aligner_delete(aligner)                        align.pyx:881-883   wfa.h:129-130
 *   reads of aligner->cigar->{score,operations,begin_offset,end_offset}
 *            aligner->align_status.status                    align.pyx:443,461-467,737-786
 *   writes to aligner->{alignment_form,alignment_scope,heuristic,penalties,...}
 *                                                            align.pyx:469-729
 *
 * Every entry point below is plain C (pointers + sizes, no torch / HIP types in the
 * signatures; a stream is passed as an opaque void*).  The reference aligns ONE pair per
 * call on one CPU thread; the replacement aligns a BATCH of independent pairs per call on
 * one GPU, so the batch forms are additive while the config struct carries exactly the kwargs
 * of WavefrontAligner.__init__ (align.pyx:309-334).  How the pairs map onto the GPU is the
 * library's business and depends on the reads: SIXTY-FOUR alignments per wavefront (a lane
 * each) for short reads — the BASELINE C2 kernel; a measured departure from north_star's
 * "one alignment per workgroup", DESIGN.md §3.0 —, one alignment per wave for long reads
 * under a heuristic, one alignment per workgroup with the M / I / D wavefronts in LDS or in
 * LDS tiles for exact long reads.  Results never depend on the mapping.
 *
 * Error model: the reference calls exit(1) on invalid penalties / ends-free sizes
 * (wavefront_penalties.c:101-112, wavefront_align.c:95-101).  Here every function returns
 * WFA_HIP_OK (0) or a negative WFA_HIP_E* code and wfa_hip_last_error() gives the text.
 * Per-pair results use the reference's own status codes (wfa.h:46-51):
 *   0 completed, 1 partial (heuristically dropped), -100 max steps reached, -200 OOM, -300 unattainable.
 */
#ifndef WFA_HIP_H_
#define WFA_HIP_H_

#ifndef __HIPCC_RTC__   /* (the kernel headers include this file for the status codes, also when compiled by hipRTC) */
#include <stdint.h>
#include <stddef.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* distance_metric_t values of the reference (wavefront_penalties.h:42-48) */
#define WFA_DIST_INDEL     0
#define WFA_DIST_EDIT      1
#define WFA_DIST_LINEAR    2
#define WFA_DIST_AFFINE    3
#define WFA_DIST_AFFINE2P  4

#define WFA_SCOPE_SCORE    0   /* compute_score      (align.pyx:374-375) */
#define WFA_SCOPE_FULL     1   /* compute_alignment  (align.pyx:372-373) */

#define WFA_SPAN_END2END   0   /* alignment_end2end  (align.pyx:396-397) */
#define WFA_SPAN_ENDSFREE  1   /* alignment_endsfree (align.pyx:394-395) */

#define WFA_HEUR_NONE      0   /* wf_heuristic_none        (align.pyx:401-402) */
#define WFA_HEUR_ADAPTIVE  1   /* wf_heuristic_wfadaptive  (align.pyx:403-407) */
#define WFA_HEUR_XDROP     2   /* wf_heuristic_xdrop       (align.pyx:408-411) */

#define WFA_MEM_HIGH       0   /* wavefront_memory_high (explicit wavefront history)  */
#define WFA_MEM_MED        1   /* wavefront_memory_med  (same results as high)        */
#define WFA_MEM_LOW        2   /* wavefront_memory_low  (same results as high)        */
#define WFA_MEM_BIWFA      3   /* wavefront_memory_ultralow (BiWFA, wavefront_bialign.c) — without heuristic / free ends */

/* per-pair status codes, identical to the reference (wfa.h:46-51) */
#define WFA_STATUS_COMPLETED          0
#define WFA_STATUS_PARTIAL            1
#define WFA_STATUS_MAX_STEPS_REACHED  (-100)
#define WFA_STATUS_OOM                (-200)
#define WFA_STATUS_UNATTAINABLE        (-300)  /* BiWFA: no alignment under the configuration (wfa.h:51) */

/* library return codes */
#define WFA_HIP_OK            0
#define WFA_HIP_EINVAL       (-1)   /* invalid configuration / arguments (reference: exit(1)) */
#define WFA_HIP_ENOTSUP      (-2)   /* configuration outside the accelerated path             */
#define WFA_HIP_EDEVICE      (-3)   /* HIP runtime error (no GPU, launch failure, OOM)         */

/*
 * Configuration = kwargs of pywfa.WavefrontAligner.__init__ (align.pyx:309-334), as a POD.
 * Defaults (wfa_hip_config_default) are pywfa's: affine 0/4/6/2 (24/1), scope full,
 * span ends-free with all free ends 0, no heuristic, memory high, max_steps unlimited.
 */
typedef struct wfa_hip_config {
  int32_t distance;                /* WFA_DIST_*                                    */
  int32_t match;                   /* <= 0                                          */
  int32_t mismatch;                /* > 0                                           */
  int32_t gap_opening;             /* >= 0                                          */
  int32_t gap_extension;           /* > 0                                           */
  int32_t gap_opening2;            /* >= 0 (affine2p)                               */
  int32_t gap_extension2;          /* > 0  (affine2p)                               */
  int32_t scope;                   /* WFA_SCOPE_*                                   */
  int32_t span;                    /* WFA_SPAN_*                                    */
  int32_t pattern_begin_free;
  int32_t pattern_end_free;
  int32_t text_begin_free;
  int32_t text_end_free;
  int32_t heuristic;               /* WFA_HEUR_*                                    */
  int32_t min_wavefront_length;    /* adaptive                                      */
  int32_t max_distance_threshold;  /* adaptive                                      */
  int32_t steps_between_cutoffs;   /* adaptive, X-drop                              */
  int32_t xdrop;                   /* X-drop                                        */
  int32_t memory_mode;             /* WFA_MEM_*                                     */
  int32_t max_steps;               /* <= 0: unlimited (align.pyx:415-417)           */
  int32_t wildcard;                /* -1: none; else the byte that matches anything */
  int32_t reserved;                /* must be 0                                     */
} wfa_hip_config_t;

typedef struct wfa_hip_aligner wfa_hip_aligner_t;  /* replaces wavefront_aligner_t*      */
typedef struct wfa_hip_batch   wfa_hip_batch_t;    /* a batch of pairs resident in HBM   */

/* ---- library / device ------------------------------------------------------------------ */

/* ABI version of this header (bumped on any signature change). */
int wfa_hip_abi_version(void);
/* Number of visible HIP devices, or a negative WFA_HIP_E* code. */
int wfa_hip_device_count(void);
/* Text for the last error on this thread when no aligner handle exists (create failed). */
const char* wfa_hip_global_error(void);

/* ---- aligner handle -------------------------------------------------------------------- */

/* Fill *cfg with pywfa's defaults (align.pyx:309-334; wavefront_attributes.c:38-100). */
int wfa_hip_config_default(wfa_hip_config_t* cfg);
/* Validate like wavefront_penalties_set_* (wavefront_penalties.c:95-173) but return
 * WFA_HIP_EINVAL instead of exit(1). err (nullable) receives a message of at most errlen. */
int wfa_hip_config_validate(const wfa_hip_config_t* cfg, char* err, size_t errlen);

/* Replaces wavefront_aligner_new (wfa.h:125-126). device = HIP device ordinal.
 * Returns NULL on error (see wfa_hip_global_error). */
wfa_hip_aligner_t* wfa_hip_create(const wfa_hip_config_t* cfg, int device);
/* Replaces wavefront_aligner_delete (wfa.h:129-130). */
void wfa_hip_destroy(wfa_hip_aligner_t* aligner);
/* Replaces pywfa's property setters that poke C fields after construction
 * (align.pyx:469-729): swap in a new validated configuration. */
int wfa_hip_set_config(wfa_hip_aligner_t* aligner, const wfa_hip_config_t* cfg);
int wfa_hip_get_config(const wfa_hip_aligner_t* aligner, wfa_hip_config_t* cfg);
const char* wfa_hip_last_error(const wfa_hip_aligner_t* aligner);

/* ---- host-buffer batch alignment (the drop-in for N x wavefront_align) ------------------ */

/*
 * Align n independent (pattern, text) pairs; synchronous.
 *   seqs            ASCII bytes, compared raw like the reference (wavefront_sequences.c:250);
 *                   pair i uses seqs[p_off[i] .. +p_len[i]) and seqs[t_off[i] .. +t_len[i])
 *   score[i]        what aligner->cigar->score holds after wavefront_align (align.pyx:443)
 *   status[i]       what aligner->align_status.status holds (align.pyx:461-463)
 *   cigar_ops       (nullable unless scope=full) caller buffer; pair i owns the region
 *                   [cigar_off[i], cigar_off[i+1]) which must hold >= p_len[i]+t_len[i] bytes
 *   cigar_off       n+1 region starts (host-computed prefix sums)
 *   cigar_begin[i], cigar_len[i]
 *                   the op string cigar->operations[begin_offset:end_offset) of pair i is
 *                   cigar_ops[cigar_begin[i] .. +cigar_len[i])  (chars M X I D)
 * All buffers are borrowed for the call; outputs are caller-owned.
 * Inside: up to 4 096 short pairs take one launch on a pinned block (single calls of a pywfa-style loop: ~30 us); batches of
 * >= 256 k pairs are packed to 2 bits per base by host threads on their way into a pinned upload ring; everything else is
 * uploaded as it is and packed on the device.  The results are the same whichever way.
 */
int wfa_hip_align_batch(wfa_hip_aligner_t* aligner, int64_t n,
                        const uint8_t* seqs,
                        const int64_t* p_off, const int32_t* p_len,
                        const int64_t* t_off, const int32_t* t_len,
                        int32_t* score, int32_t* status,
                        uint8_t* cigar_ops, const int64_t* cigar_off,
                        int64_t* cigar_begin, int32_t* cigar_len);

/*
 * One pair per call — pywfa's own usage pattern: wavefront_align(text) against the cached pattern (align.pyx:421-443, one
 * wavefront_align / wavefront_align_lambda per call, wfa.h:199-210).  The result of wfa_hip_align_batch with n = 1 without its
 * arrays: `pattern` / `text` are the two ASCII sequences; `cigar_ops` (NULL for scope = score) receives plen + tlen bytes of which
 * [*cigar_begin, *cigar_begin + *cigar_len) are the alignment's ops.  Round 6: calls in a row are served without a kernel launch — a
 * one-wave kernel stays on the device and takes the pairs from a mailbox in pinned host memory (it leaves by itself after 2 ms without
 * a call, before any batch of this aligner, and when the aligner is destroyed; gap-affine shapes of the library, reads of up to 1 000
 * bases; anything else takes the single-launch path: the pair packed into a pinned block, one wave, a completion flag polled by the
 * host).  About 9 us per 150 bp call from C score-only, 16.5 us with the op string, against 1-2 us for the reference on a host core —
 * the library is batch-oriented, and a loop of single calls, while exact, is what wfa_hip_align_batch with many pairs replaces.
 * WFA_HIP_MAILBOX=0: a launch per call (13 / 21 us).
 */
int wfa_hip_align_pair(wfa_hip_aligner_t* aligner, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen,
                       int32_t* score, int32_t* status, uint8_t* cigar_ops, int64_t* cigar_begin, int32_t* cigar_len);

/*
 * The same call for a caller that already holds 2-bit reads (cf. wavefront_align_packed2bits, wfa.h:211-216,
 * wavefront_sequences.h:115): `packed` holds every sequence in the reference's packed form (wavefront_sequences.c:102-139:
 * four bases per byte, base j of a byte in bits 2j .. 2j+1, 'A' 0 / 'C' 1 / 'G' 2 / 'T' 3), a sequence of len bases being
 * (len + 3) / 4 bytes starting at its BYTE offset p_off[i] / t_off[i]; p_len / t_len stay in bases.  The results are those
 * of wfa_hip_align_batch on the decoded ASCII sequences (that is what the tests pin it against: the reference's own entry
 * reads only (len + 7) / 8 bytes per sequence, wavefront_sequences.c:112, and aligns uninitialised buffer bytes behind them).
 * A quarter of the bytes are read on the host; large batches are re-based to whole words by the upload workers on their way into the
 * pinned ring (round 6: the same bytes cross PCIe as for ASCII input).  A wildcard letter cannot be expressed: WFA_HIP_ENOTSUP.
 */
int wfa_hip_align_batch_packed2bits(wfa_hip_aligner_t* aligner, int64_t n,
                                    const uint8_t* packed,
                                    const int64_t* p_off, const int32_t* p_len,
                                    const int64_t* t_off, const int32_t* t_len,
                                    int32_t* score, int32_t* status,
                                    uint8_t* cigar_ops, const int64_t* cigar_off,
                                    int64_t* cigar_begin, int32_t* cigar_len);

/* ---- host helper: the text of cigar_print_pretty ------------------------------------------------- */

/*
 * What cigar_print_pretty prints (cigar.h:180-186, cigar.c:778-863; called by align.pyx:445-459) for the op string
 * ops[0 .. ops_len) (chars M X I D, i.e. cigar->operations[begin_offset .. end_offset)) of `pattern` against `text`: the
 * ALIGNMENT (runs incl. M), ETRACE (runs without M) and CIGAR (SAM style, X folded into M) lines and the three rows
 * PATTERN / marks / TEXT.  Written NUL-terminated into out[0 .. cap) (truncated if cap is too small, like snprintf);
 * returns the length of the whole text without the NUL, or WFA_HIP_EINVAL.  Host only, needs no GPU.
 */
int64_t wfa_hip_cigar_sprint_pretty(const uint8_t* ops, int64_t ops_len,
                                    const uint8_t* pattern, int32_t plen,
                                    const uint8_t* text, int32_t tlen,
                                    char* out, int64_t cap);

/* ---- host helper: the 2-bit packing the large-batch upload uses ----------------------------------- */

/*
 * Packs `len` ASCII bases into (len + 15) / 16 words: word w holds bases 16 w .. 16 w + 15, base j in bits 2 j .. 2 j + 1,
 * code (c >> 1) & 3 ('A' 0, 'C' 1, 'T' 2, 'G' 3), zero beyond the end — the layout the kernels read.  Host only, needs no
 * GPU.  wfa_hip_align_batch / wfa_hip_batch_create run it on several host threads for batches of >= 256 k pairs, so
 * that 2 bits per base cross PCIe instead of 8 (the reference has no counterpart: it reads the caller's bytes in place,
 * wavefront_sequences.c:153-250).  form: -1 = the best the CPU has; 0 plain C, 1 AVX2, 2 AVX-512BW (for tests; a form the
 * CPU lacks falls back to plain C).  Returns 1 if some byte is not one of ACGT (such a pair is aligned on its bytes),
 * 0 if none, WFA_HIP_EINVAL on bad arguments.
 */
int wfa_hip_pack_2bit(const uint8_t* seq, int32_t len, uint32_t* words, int form);

/*
 * The number of blob bytes a batch description reaches: max over pairs of p_off + p_len and t_off + t_len (host only,
 * several threads), or -1 if an offset or a length is negative or an argument is missing.  For bindings: the align /
 * create calls take the blob by pointer only, so a binding that knows the blob's size checks it against this first
 * (pywfa_amd/_native.py does; pywfa itself passes one str per call, align.pyx:432-437).
 */
int64_t wfa_hip_batch_extent(int64_t n, const int64_t* p_off, const int32_t* p_len, const int64_t* t_off, const int32_t* t_len);
/* The same for a batch of 2-bit reads (wfa_hip_align_batch_packed2bits): a sequence of len bases reaches (len + 3) / 4 bytes. */
int64_t wfa_hip_batch_extent_packed2bits(int64_t n, const int64_t* p_off, const int32_t* p_len, const int64_t* t_off, const int32_t* t_len);

/* ---- several devices of one node ------------------------------------------------ */

/*
 * Pairs are independent, so a batch shards over the GPUs of a node with no exchange step: contiguous shards
 * balanced by sum(p_len + t_len), one host thread + one aligner + one stream per device, results written into
 * disjoint slices of the caller's arrays; no collective.  (The reference has no counterpart: it aligns one pair per
 * call on one CPU thread.)
 */
typedef struct wfa_hip_multi wfa_hip_multi_t;

/* The shard planner alone (host only, needs no GPU): shard_begin[nshards + 1], shard s = pairs
 * [shard_begin[s], shard_begin[s + 1]).  Returns WFA_HIP_OK or WFA_HIP_EINVAL. */
int wfa_hip_plan_shards(int64_t n, const int32_t* p_len, const int32_t* t_len, int nshards, int64_t* shard_begin);

/* The host side of several devices (host only, needs no GPU): the threads ONE device's upload pipeline takes — 2-bit packing into its
 * pinned ring, and plain copies — when `sharers` aligners or processes feed GPUs from a host of `hw_threads` logical CPUs.  The
 * devices of a wfa_hip_multi_t count themselves; a one-process-per-GPU job says so through LOCAL_WORLD_SIZE (torch.distributed.run
 * exports it) or WFA_HIP_HOST_SHARE.  Returns WFA_HIP_OK or WFA_HIP_EINVAL. */
int wfa_hip_plan_host_threads(int sharers, int hw_threads, int* pack_threads, int* copy_threads);

/* What the upload pipeline of this aligner knows about the host, and what its last pipelined upload (a batch of >= 256 k pairs) did
 * (diagnostics for the PCIe-inclusive rate; no counterpart in the reference, whose aligner never leaves the host).  info[0..7]:
 * NUMA node of the device's PCIe slot (-1 unknown), CPUs of that node this process may use (0: no binding possible), binding mode
 * (WFA_HIP_NUMA: 0 never, 1 always, 2 only when the caller's input lives on the device's node), node of the caller's pages in the last
 * upload (-1 unknown), whether that upload's spawned workers were bound (the caller's own thread never is), packing threads, copy
 * threads, CPUs of the process.  n >= 8.  Returns WFA_HIP_OK or WFA_HIP_EINVAL. */
int wfa_hip_upload_info(const wfa_hip_aligner_t* aligner, int32_t* info, int n);

/* One aligner per entry of devices[] (an ordinal may repeat: several host threads then feed that device).
 * Returns NULL on error (see wfa_hip_global_error). */
wfa_hip_multi_t* wfa_hip_multi_create(const wfa_hip_config_t* cfg, const int* devices, int ndevices);
void wfa_hip_multi_destroy(wfa_hip_multi_t* multi);
int wfa_hip_multi_set_config(wfa_hip_multi_t* multi, const wfa_hip_config_t* cfg);
const char* wfa_hip_multi_last_error(const wfa_hip_multi_t* multi);
/* Same arguments and results as wfa_hip_align_batch; synchronous. */
int wfa_hip_multi_align_batch(wfa_hip_multi_t* multi, int64_t n,
                              const uint8_t* seqs,
                              const int64_t* p_off, const int32_t* p_len,
                              const int64_t* t_off, const int32_t* t_len,
                              int32_t* score, int32_t* status,
                              uint8_t* cigar_ops, const int64_t* cigar_off,
                              int64_t* cigar_begin, int32_t* cigar_len);

/* ---- HBM-resident batches (what bench.py times; inputs resident before the clock starts) -- */

/* Upload n pairs (same input arrays as above) as 2-bit codes (packed by host threads on their way into the pinned upload
 * ring for batches of >= 256 k pairs, by a device kernel otherwise).  The returned batch keeps sequences, per-pair metadata
 * and result arrays in HBM.  For short-read batches of >= 64 k pairs the call also runs the pilot that picks the first
 * stage of the cascade (up to three small launches on 8192 pairs sampled across the batch, each waited for).  The input
 * arrays are not read after the call returns; uploads still in flight then are ordered before any later run by the library
 * (whatever stream the run is given). */
wfa_hip_batch_t* wfa_hip_batch_create(wfa_hip_aligner_t* aligner, int64_t n,
                                      const uint8_t* seqs,
                                      const int64_t* p_off, const int32_t* p_len,
                                      const int64_t* t_off, const int32_t* t_len);
/* The same for 2-bit reads in the reference's packed form (see wfa_hip_align_batch_packed2bits). */
wfa_hip_batch_t* wfa_hip_batch_create_packed2bits(wfa_hip_aligner_t* aligner, int64_t n,
                                                  const uint8_t* packed,
                                                  const int64_t* p_off, const int32_t* p_len,
                                                  const int64_t* t_off, const int32_t* t_len);
void wfa_hip_batch_destroy(wfa_hip_batch_t* batch);
/* Enqueue the alignment kernels for the whole batch on `stream` (hipStream_t passed as
 * void*, NULL = the library's own stream) and return without waiting: in the steady state the call only enqueues (kernels,
 * memsets, event waits).  Exceptions, all one-off: the FIRST run of an aligner and any run that has to grow its workspace
 * allocate device memory (hipFree / hipMalloc synchronise the device, and may drain the aligner's block pool), and the first
 * run under penalties the library has no built-in kernels for compiles them (hipRTC, about a second per kernel; cached on
 * disk under ~/.cache/pywfa_amd or $WFA_HIP_RTC_CACHE). */
int wfa_hip_batch_run(wfa_hip_batch_t* batch, void* stream);
/* Wait for the last run of this batch. */
int wfa_hip_batch_sync(wfa_hip_batch_t* batch);
/* Copy results of the last run to host arrays (cigar_* nullable for scope=score). */
int wfa_hip_batch_results(wfa_hip_batch_t* batch, int32_t* score, int32_t* status,
                          uint8_t* cigar_ops, const int64_t* cigar_off,
                          int64_t* cigar_begin, int32_t* cigar_len);
/* Mean HIP-event time (ms) per run of the alignment kernels, over the runs enqueued since the
 * previous sync (events are recorded on the stream the kernels are launched on), and the number of
 * pairs one run hands to the dominant kernel (for bench.py's roofline line). */
int wfa_hip_batch_last_kernel_ms(wfa_hip_batch_t* batch, float* ms, int64_t* pairs);
/* Algorithmic HBM bytes of one run: 2-bit packed sequence bytes + 8 result bytes per pair
 * (+ CIGAR op bytes for scope=full), SURVEY.md §8(d). */
int64_t wfa_hip_batch_algorithmic_bytes(const wfa_hip_batch_t* batch);
/* Pairs the fast (register/LDS) kernel handed to the general kernel in the last run. */
int64_t wfa_hip_batch_fallback_pairs(const wfa_hip_batch_t* batch);

/* ---- result surface on the device ------------------------------------------ */

/*
 * What pywfa derives per pair in Python from cigar->operations after each call — the run-length
 * encoded `cigartuples` (align.pyx:759-786; op codes M=0 I=1 D=2 X=8) and the `locations`
 * (pattern_start, pattern_end, text_start, text_end; align.pyx:788-833) — for the whole batch of the
 * last scope=full run, computed on the GPU.
 *   step 1  wfa_hip_batch_rle_counts: run_count[n] and locations[4n]; returns the total number of runs
 *           (or a negative WFA_HIP_E* code)
 *   step 2  wfa_hip_batch_rle_runs: run_code[total], run_len[total] in pair order
 *           (pair i owns runs [sum(run_count[:i]), +run_count[i]))
 */
int64_t wfa_hip_batch_rle_counts(wfa_hip_batch_t* batch, int32_t* run_count, int32_t* locations);
int wfa_hip_batch_rle_runs(wfa_hip_batch_t* batch, uint8_t* run_code, int32_t* run_len);

/* ---- score matrices: every sequence of one set against every sequence of another, or of itself ---------- */

/*
 * Semantics.  Cross mode: pattern set P (m sequences) and text set T (n sequences); score[i][j] / status[i][j] are exactly what
 * wfa_hip_align_batch returns for the pair (P[i], T[j]) under the aligner's configuration at wfa_hip_cross_run with scope set to
 * score (whatever scope the aligner has: no op strings).  All-vs-all mode (T = NULL): the dense result is the full n x n cross product
 * of P with itself, diagonal included, every cell meaning the same.  Where the score is provably symmetric — no heuristic, and span
 * end-to-end or ends-free with pattern_begin_free == text_begin_free and pattern_end_free == text_end_free — only the cells j >= i are
 * aligned and mirrored; under wf-adaptive, X-drop or asymmetric free ends both orders are aligned.  Free ends larger than a sequence:
 * WFA_HIP_EINVAL (as wfa_hip_align_batch).
 *
 * Completed pairs: the list of (i, j, score) of every cell with status 0, in row-major order of (i, j); all-vs-all: the cells i < j
 * only.  Meant for runs under max_steps (clustering, de-duplication: the close pairs), it needs no m x n buffer on either side.
 *
 * Inside, the pair metadata of the cross product is generated on the device in bands of rows, each band aligned by the batch
 * cascade over the sets' packed words (each sequence is uploaded and packed once: m + n sequences cross PCIe, not m x n pairs).
 * WFA_HIP_CROSS_BAND (pairs per band, read when the aligner is created) caps the band size.
 */
typedef struct wfa_hip_seqset wfa_hip_seqset_t;  /* a set of sequences resident in HBM, 2-bit packed once */
typedef struct wfa_hip_cross  wfa_hip_cross_t;   /* the results of one cross run, resident in HBM       */

#define WFA_HIP_CROSS_DENSE      1   /* want: the m x n score / status matrices          */
#define WFA_HIP_CROSS_COMPLETED  2   /* want: the list of completed pairs                */
#define WFA_HIP_CROSS_TOPK       4   /* want: the k best cells of every row (wfa_hip_cross_run_k only) */
#define WFA_HIP_CROSS_MAX_K      64  /* the largest k of WFA_HIP_CROSS_TOPK              */

/* Upload n sequences (ASCII; sequence k = seqs[off[k] .. +len[k])) as the word table the kernels read, one word-aligned run per
 * sequence.  The set keeps the lengths on the host, a flag per sequence holding letters outside ACGT (such a sequence also keeps its
 * bytes, and its pairs are aligned on them, as in a batch; the host also keeps where those letters are, for windowed batches), and the aligner's wildcard at this call: a cross run under another
 * wildcard returns WFA_HIP_EINVAL.  The inputs are not read after the call returns.  Returns NULL on error (wfa_hip_last_error). */
wfa_hip_seqset_t* wfa_hip_seqset_create(wfa_hip_aligner_t* aligner, int64_t n, const uint8_t* seqs, const int64_t* off, const int32_t* len);
void wfa_hip_seqset_destroy(wfa_hip_seqset_t* set);

/* Run the cross product of `patterns` x `texts` (texts = NULL: all-vs-all of `patterns`); synchronous.  want = WFA_HIP_CROSS_DENSE
 * and / or WFA_HIP_CROSS_COMPLETED.  The sets must belong to `aligner`.  Returns NULL on error (wfa_hip_last_error). */
wfa_hip_cross_t* wfa_hip_cross_run(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts, int want);
/* Top-k per row.  For every row i of the score matrix, the k best of its eligible cells, best first.  Eligible: status 0 (the cells
 * the completed pairs list), and in all-vs-all mode every column j != i: the diagonal is excluded, and where the run mirrors (the rule
 * above) the cells j < i of row i are the aligned cells (j, i).  Best: the larger score as the score matrix holds it (so also for
 * match < 0, where scores are positive), ties to the smaller j; the result does not depend on band sizes or runs.  A row with fewer
 * than k eligible cells is padded with j = -1, score = INT32_MIN.  Reduced on the device band by band (csrc/wfa_cross.hpp): no m x n
 * buffer on either side unless WFA_HIP_CROSS_DENSE is also wanted.
 * wfa_hip_cross_run_k: as wfa_hip_cross_run, want any non-empty combination of WFA_HIP_CROSS_DENSE, _COMPLETED and _TOPK; k (read
 * only with WFA_HIP_CROSS_TOPK) in 1 .. WFA_HIP_CROSS_MAX_K, else WFA_HIP_EINVAL.  wfa_hip_cross_run refuses WFA_HIP_CROSS_TOPK. */
wfa_hip_cross_t* wfa_hip_cross_run_k(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts, int want, int k);
/* The top-k: m x k row-major int32 host arrays of columns and scores (needs WFA_HIP_CROSS_TOPK, else WFA_HIP_EINVAL). */
int wfa_hip_cross_topk(wfa_hip_cross_t* cross, int32_t* j, int32_t* score);
/* The dense results: m x n row-major int32 host arrays (needs WFA_HIP_CROSS_DENSE). */
int wfa_hip_cross_dense(wfa_hip_cross_t* cross, int32_t* score, int32_t* status);
/* The completed pairs: *count always; i / j / score (each *count entries) when not NULL (needs WFA_HIP_CROSS_COMPLETED). */
int wfa_hip_cross_completed(wfa_hip_cross_t* cross, int64_t* count, int32_t* i, int32_t* j, int32_t* score);
/* HIP-event time (ms) of the alignment kernels summed over the bands (the span wfa_hip_batch_last_kernel_ms times for a batch), and
 * the pairs aligned. */
int wfa_hip_cross_kernel_ms(wfa_hip_cross_t* cross, float* ms, int64_t* pairs);
void wfa_hip_cross_destroy(wfa_hip_cross_t* cross);

/* The band planner alone (host only, needs no GPU): bands of whole rows of the m x n rectangle (triangle = 0) or of the upper triangle
 * of an n x n square, columns j >= i (triangle = 1, m ignored), each of at most max_pairs pairs (a row longer than that is a band of
 * its own).  Writes the first row of every band and the end, row_begin[0 .. nbands], when row_begin is not NULL and cap >= nbands + 1.
 * Returns nbands, or WFA_HIP_EINVAL. */
int64_t wfa_hip_plan_cross_bands(int64_t m, int64_t n, int triangle, int64_t max_pairs, int64_t* row_begin, int64_t cap);

/* ---- indexed batches: a list of (i, j) index pairs over resident sequence sets ----------------------------- */

/* A resident batch whose pair q is (patterns[i[q]], texts[j[q]]); texts = NULL: both indices into `patterns`.  The result is an
 * ordinary batch: run / sync / results / rle_counts / rle_runs / last_kernel_ms / algorithmic_bytes / fallback_pairs / destroy work on
 * it unchanged, and pair q's score, status and op string are exactly what wfa_hip_align_batch returns for that pair under the
 * aligner's configuration at this call, scope included (scope full: op strings, in regions of plen + tlen bytes in list order, as a
 * batch's).  Results are in list order; duplicates, i == j and empty sequences are legal; npairs = 0 is a valid empty batch.  Eight
 * bytes per pair cross PCIe: the pair metadata and the pairs' words are laid out on the device from the sets' tables
 * (csrc/wfa_cross.hpp).
 * WFA_HIP_EINVAL (NULL, wfa_hip_last_error; nothing is launched): an index outside its set (the message names the first such
 * position), a set of another aligner or packed under another wildcard, free ends larger than a LISTED sequence (checked per listed
 * pair: a short sequence no pair names is harmless), more than 2^32 words of sets and slots ("split the list").
 * The index arrays are not read after the call returns, and the batch stays valid after either set is destroyed (it copies what it
 * needs of them on the device).  A set serves any number of indexed batches and cross runs, in any order. */
wfa_hip_batch_t* wfa_hip_batch_create_indexed(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts,
                                              int64_t npairs, const int32_t* i, const int32_t* j);

/* ---- windowed batches: windows of resident sequences, either strand, by index ------------------------------ */

/* A resident batch whose pair q is a window of patterns[i[q]] against a window of texts[j[q]] (texts = NULL: both indices into
 * `patterns`).  Pattern: bases [p_start[q], p_start[q] + p_len[q]) of patterns[i[q]], and where reverse[q] != 0 the reverse complement
 * of that window; text: bases [t_start[q], t_start[q] + t_len[q]) of texts[j[q]], never reversed.  A NULL start array means 0 for every
 * pair, a NULL length array "to the end of the sequence from the start", a NULL `reverse` every pair forward.  The complement on bytes
 * is A<->T, C<->G, a<->t, c<->g and every other byte unchanged (N stays N, a wildcard byte stays itself).
 * The result is an ordinary batch (run / sync / results / rle_counts / rle_runs / last_kernel_ms / algorithmic_bytes / fallback_pairs /
 * destroy work on it unchanged): pair q's score, status and op string are exactly what wfa_hip_align_batch returns for the two
 * materialised byte strings under the aligner's configuration at this call, scope included; op-string regions are p_len[q] + t_len[q]
 * bytes in list order, coordinates are relative to the windows (the caller adds the starts).  Duplicates, overlapping windows, empty
 * windows (length 0) and i == j are legal; npairs = 0 is a valid empty batch.  Up to 25 bytes per pair cross PCIe (8 with every
 * optional array NULL): the slots are gathered on the device from the sets' words (csrc/wfa_cross.hpp, k_windows.hip).
 * A pair is aligned on its bytes exactly when the wildcard is one of ACGT or one of its two WINDOWS holds a letter outside ACGT: the
 * windows of a reference with a few N runs that avoid the Ns take the 2-bit kernels (wfa_hip_batch_last_kernel_ms reports the count).
 * WFA_HIP_EINVAL (NULL, wfa_hip_last_error; nothing is launched): an index outside its set, a negative start or length, a window that
 * ends behind its sequence (the message names the first offending list position and its values), a set of another aligner or packed
 * under another wildcard, free ends larger than a LISTED WINDOW, more than 2^32 words of slots ("split the list").
 * The arrays are not read after the call returns.  The batch owns the slots of the listed windows and nothing else (no copy of a set,
 * whatever the sequences' lengths), and stays valid after either set is destroyed. */
wfa_hip_batch_t* wfa_hip_batch_create_windows(wfa_hip_aligner_t* aligner,
    const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts, int64_t npairs,
    const int32_t* i, const int32_t* j,
    const int32_t* p_start, const int32_t* p_len,     /* nullable */
    const int32_t* t_start, const int32_t* t_len,     /* nullable */
    const uint8_t* reverse);                          /* nullable */

/* Host only, needs no GPU: the (len + 15) / 16 words of the window [start, start + len) of a sequence in wfa_hip_pack_2bit's layout,
 * re-based to bit 0, reverse-complemented when reverse != 0 (a reversal of the 2-bit groups and code ^ 2), zero beyond `len` — what
 * the device gather stores in a slot, and wfa_hip_pack_2bit of the materialised ACGT string.  Only the words that hold a base of the
 * window are read.  Returns WFA_HIP_OK, or WFA_HIP_EINVAL on a negative start or length (or a NULL pointer with len > 0). */
int wfa_hip_window_2bit(const uint32_t* words, int64_t start, int32_t len, int reverse, uint32_t* out);

/* ---- reductions of the op strings on the device: per pair, and per text position --------------------------- */

/* Op letters are the library's: M and X consume one pattern base and one text base, D a pattern base only, I a text base only.  The
 * ALIGNED CORE of an op string is the span from its first M to its last M, inclusive (the ops outside it are the ends `locations`
 * strips, align.pyx:797-831 with a threshold of 1); an op string without an M has an empty core. */

/* Per-pair summary of the last scope=full run, for any resident batch (plain, packed2bits, indexed, windows): `summary` receives n
 * rows of WFA_HIP_SUMMARY_COLS int32, row-major.  Over the whole op string [cigar_begin, + cigar_len) of the pair:
 *   0..3  the numbers of M, X, I and D ops
 *   4, 5  the numbers of maximal runs of I, and of D
 *   6..9  pattern_start, pattern_end, text_start, text_end: exactly what wfa_hip_batch_rle_counts writes to `locations` for the pair
 *         (all zero for an empty pair or an empty op string)
 * A pair with an empty op string (heuristically dropped, step limit) has zeros in columns 0..5 too.  Waits for the last run like
 * wfa_hip_batch_rle_counts; one kernel (csrc/wfa_summary.hpp) and one download of 40 bytes per pair: no op string and no run-length
 * encoding crosses PCIe.  n = 0 is fine.  WFA_HIP_EINVAL: a batch of scope score or without a run ("... needs scope=full" / "... needs
 * a finished run"), a NULL `summary` with n > 0. */
#define WFA_HIP_SUMMARY_COLS 10
int wfa_hip_batch_summary(wfa_hip_batch_t* batch, int32_t* summary);

/* Host only, needs no GPU: the row wfa_hip_batch_summary writes for ONE pair, from its op string ops[0 .. ops_len) and its lengths.
 * Returns WFA_HIP_OK, or WFA_HIP_EINVAL on a negative length or a missing pointer. */
int wfa_hip_ops_summary(const uint8_t* ops, int64_t ops_len, int32_t plen, int32_t tlen, int32_t* out10);

/*
 * Pileup over a text set: the pairs of full-scope batches taken as READS (the pattern) aligned against windows of REFERENCES (the
 * texts of a resident set), counted per text base.  Per base WFA_HIP_PILEUP_COLS int32 counters:
 *   0..4  reads whose aligned base here is A, C, G, T, or anything else (N, a wildcard byte, lower case)
 *   5     reads that delete this base (op I: a text base the read lacks)
 *   6     reads that insert bases in front of this base (op D: read bases the text lacks; one count per maximal D run)
 *   7     reads that mismatch here (op X; also counted in 0..4 under the read's letter)
 * so the sum of columns 0..5 is the number of contributing reads whose aligned core covers the base.
 *
 * wfa_hip_pileup_create allocates the zeroed table for every base of `texts` in HBM: 32 BYTES PER TEXT BASE (a failed allocation:
 * NULL, WFA_HIP_EDEVICE, the message names the byte count).  COUNTERS ARE int32 AND NOT CHECKED FOR OVERFLOW.  The pileup copies the
 * set's lengths and prefix offsets: it stays valid after the set is destroyed.  A set of another aligner is refused (NULL).
 *
 * wfa_hip_pileup_add waits for the batch's last run, then adds its pairs: pair q is taken to be a read aligned against the text bases
 * [t_start[q], t_start[q] + tlen[q]) of texts[j[q]], tlen[q] being the batch's own text length of the pair (the caller guarantees that
 * the batch's text really was that window; the arrays given to wfa_hip_batch_create_windows are exactly this).  t_start NULL: 0 for
 * every pair.  Pair q contributes iff its status is 0 and (keep == NULL or keep[q] != 0).  Its op string is walked with a pattern
 * position v and a text position h, both from 0; only the ops of the aligned core add, to row g = t_start[q] + h:
 *   M  +1 to the column of pattern letter v                          then v, h advance
 *   X  +1 to the column of pattern letter v, +1 to column 7          then v, h advance
 *   I  +1 to column 5                                                then h advances
 *   D  +1 to column 6, once per maximal D run (at the g where the run starts: the text base behind the inserted read bases);  v advances
 * The pattern letter is the batch's: of a reverse-strand window the reverse complement, i.e. on the text's strand.  Any number of adds
 * accumulate into one table; integer adds make the result independent of their order and of how a list is split.  One kernel
 * (csrc/wfa_pileup.hpp, k_pileup.hip: a wave per pair, int32 atomics), 9 bytes per pair uploaded, nothing downloaded.
 * WFA_HIP_EINVAL, nothing launched (wfa_hip_last_error names the first offending list position and its values): a batch of another
 * aligner, of scope score or without a finished run; j[q] outside the set; a negative t_start[q]; t_start[q] + tlen[q] behind the end
 * of texts[j[q]].
 *
 * wfa_hip_pileup_read copies the rows [start, start + len) of sequence `seq` into counts (len x WFA_HIP_PILEUP_COLS, row-major);
 * WFA_HIP_EINVAL when the range leaves the sequence.  wfa_hip_pileup_clear zeroes the table (and drops the insertion log of a pileup
 * that tracks insertions, keeping that setting: "insertions" below; likewise the deletion log and the starts plane: "deletions" below).
 */
#define WFA_HIP_PILEUP_COLS 8   /* A, C, G, T, other, deleted, insertion-before, mismatch */
typedef struct wfa_hip_pileup wfa_hip_pileup_t;
wfa_hip_pileup_t* wfa_hip_pileup_create(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* texts);
int  wfa_hip_pileup_add(wfa_hip_pileup_t* pileup, wfa_hip_batch_t* batch,
                        const int32_t* j, const int32_t* t_start /* nullable: 0 */, const uint8_t* keep /* nullable: all */);
int  wfa_hip_pileup_read(wfa_hip_pileup_t* pileup, int32_t seq, int64_t start, int64_t len, int32_t* counts /* len x 8 */);
int  wfa_hip_pileup_clear(wfa_hip_pileup_t* pileup);
void wfa_hip_pileup_destroy(wfa_hip_pileup_t* pileup);

/* Host only, needs no GPU: ONE pair's contribution by the rule above, from its op string and its ASCII pattern bytes, added to the
 * window-relative rows rows[0 .. tlen) (tlen x WFA_HIP_PILEUP_COLS, row-major; not cleared).  Returns WFA_HIP_OK, or WFA_HIP_EINVAL on
 * a negative length, a missing pointer, or an op string that consumes more than plen pattern or tlen text bases (nothing is added). */
int wfa_hip_ops_pileup(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, int32_t tlen,
                       int32_t* rows /* tlen x 8, added to */);

/* ---- calls and sites: two reductions of a pileup against its reference set -------------------------------- */

/*
 * What a caller wants from a pileup is rarely the table: it is one byte per base (the consensus call) or the few rows where the reads
 * disagree with the reference.  Both are computed on the device from the table and the reference letters; 1 byte per base, or 32 bytes
 * per SITE, cross PCIe instead of 32 bytes per base.  Integers only.
 *
 * For base g of text j take the counters c0..c7 (the columns of WFA_HIP_PILEUP_COLS) and the reference byte b of that base:
 *   r     = col(b): 'A' 0, 'C' 1, 'G' 2, 'T' 3, every other byte 4 (lower case, N, a wildcard byte) — the mapping the pileup applies to
 *           read letters
 *   depth = c0 + ... + c5, summed in 64 bits (the site row holds its low 32 bits: counters are not checked for overflow)
 *
 * CALL (one byte per base), parameter min_depth >= 1.
 *   low 3 bits: 6 ("no call") when depth < min_depth; otherwise the column x in 0..5 with the greatest c[x]; among equal greatest
 *               columns r if it is one of them, else the smallest x.  So 0..3 are a base, 4 another letter, 5 "deleted here".
 *   bit 3 (8):  set when depth >= min_depth and 2 * c6 > depth: most covering reads insert in front of this base.
 *
 * SITE, parameters min_depth >= 1 and min_permille in 1..1000.  A base is considered only when depth >= min_depth.
 *   alt  = the column in 0..5 other than r with the greatest count, the smallest on a tie; A = c[alt]
 *   snv  = A >= 1 && 1000 * A >= min_permille * depth            (64-bit products)
 *   ins  = c6 >= 1 && 1000 * c6 >= min_permille * depth
 * The base is a site iff snv || ins.  Its row is WFA_HIP_SITE_COLS int32:
 *   j, pos, ref = r, alt (-1 when !snv), depth, ref_count = c[r], alt_count (A; 0 when !snv), ins_count = c6
 * Sites come out in ascending (j, pos), always: the order does not depend on scheduling, two calls give identical rows.
 *
 * A site says that, and how often, reads insert in front of a base; WHAT they insert is the allele row of "insertions" below, from a
 * pileup made to track them; per-strand counts and a diploid genotype per site: "strands and genotypes" below; base
 * qualities: "base qualities" below; a deletion of several bases as one event with its start and length: "deletions" below.
 * Out of scope: multi-base substitutions, genotypes and strand counts per deletion allele; more than one alternate allele per site,
 * ploidy other than 2, a Fisher or other strand statistic (the four counts are returned; the test is the caller's).
 *
 * The pileup keeps no reference letters and outlives its set, so both device calls take the set: the one the pileup was made over, or
 * one made again from the same sequences.  wfa_hip_pileup_calls writes out[0 .. len) for the rows [start, start + len) of sequence
 * seq.  wfa_hip_pileup_sites sets *count to the number of sites in the range (always the full number) and writes the first
 * min(*count, cap) rows (cap x 8 int32, row-major; rows behind them are not touched); cap = 0 with rows = NULL is the counting call;
 * seq = -1 takes every sequence, with start = 0 and len = -1.  Both wait for the aligner's stream, as wfa_hip_pileup_read does; len = 0
 * is fine.  Kernels: csrc/wfa_calls.hpp, k_calls.hip (calls: a thread per base; sites: count per chunk of bases, exclusive scan of
 * the chunk counts, scatter — no atomics; the chunk is WFA_HIP_CALLS_CHUNK bases, read per call).
 * WFA_HIP_EINVAL, nothing launched, nothing written (wfa_hip_last_error names the values): a set of another aligner; a set whose
 * number of sequences or any length differs from the pileup's (the first differing sequence and both lengths are named); a range that
 * leaves its sequence; min_depth < 1; min_permille outside 1..1000; cap < 0; a NULL `out` with len > 0, a NULL `count`, NULL `rows`
 * with cap > 0; seq = -1 with another start or len.
 */
#define WFA_HIP_SITE_COLS 8   /* j, pos, ref, alt, depth, ref_count, alt_count, ins_count */
int wfa_hip_pileup_calls(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                         int32_t min_depth, uint8_t* out /* len */);
int wfa_hip_pileup_sites(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                         int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows /* cap x 8, nullable */);

/* Host only, needs no GPU: the same two rules on `len` rows as wfa_hip_pileup_read returns them (counts: len x 8, row-major) and the
 * reference bytes ref[0 .. len) of those rows.  wfa_hip_sites_host numbers its rows j = seq, pos = start + row.  Returns WFA_HIP_OK,
 * or WFA_HIP_EINVAL (nothing written) on a negative len, a parameter out of range (as above) or a missing pointer. */
int wfa_hip_calls_host(const int32_t* counts, const uint8_t* ref, int64_t len, int32_t min_depth, uint8_t* out);
int wfa_hip_sites_host(const int32_t* counts, const uint8_t* ref, int64_t len, int32_t seq, int64_t start,
                       int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows);

/* ---- insertions: what the reads insert, one allele per reported row ---------------------------------------- */

/*
 * Column 6 counts THAT reads insert in front of a base.  A pileup that tracks insertions also keeps WHAT they insert, in a log on the
 * device, and reduces it there to one allele per row.  It is opt-in: a pileup that does not ask for it behaves, allocates and launches
 * exactly as before.  Integers only.
 *
 * RECORDS.  A pair contributes under exactly the conditions of wfa_hip_pileup_add (status 0, keep, its window inside its text).  Every
 * maximal D run of its aligned core that the add counts into column 6 is one record (g, n, letters):
 *   g        the global row t_start + h of text j: the row whose column 6 the run increments
 *   n        the run's length
 *   letters  col(pattern[v .. v + n)): 0..3 = A C G T, 4 = any other byte; the batch's pattern, so on the text's strand for a
 *            reverse window
 * So the number of records at a row equals that row's column 6.
 *
 * ALLELE OF A ROW.  The alleles are the distinct (n, letters) among the row's records, count(a) the multiplicity of allele a.  The
 * row's allele is the one with the greatest count; ties go to the smaller n, then to the lexicographically smaller column sequence.
 * The order is total: the result never depends on the order in which records were stored, added or split over adds.
 *
 * REPORTED ROWS, parameters min_depth >= 1 and min_permille in 0..1000; depth as in "calls and sites".  A row is reported iff
 * depth >= min_depth and
 *   min_permille > 0:   c6 >= 1 && 1000 * c6 >= min_permille * depth      (exactly the `ins` condition of SITE)
 *   min_permille == 0:  2 * c6 > depth                                    (exactly bit 3 of CALL)
 * Its row is WFA_HIP_INSERTION_COLS int32:
 *   j, pos, depth, ins_count (= c6), allele_count, allele_len, alleles (the number of distinct alleles), overflow
 * Rows come out in ascending (j, pos), always.  The alleles' letters follow in one byte array in row order, as ASCII A C G T N; row
 * r's letters start at the sum of allele_len of the rows before it.  A row whose ins_count exceeds WFA_HIP_INS_MAX_READS is still
 * reported, with overflow = 1 and allele_count = allele_len = alleles = 0: the limit (default 4096; read per call from the environment
 * variable of that name, as WFA_HIP_CALLS_CHUNK is; at least 1) bounds the work of the one wave that serves a row, a documented limit
 * like max_hits.
 *
 * wfa_hip_pileup_track_insertions turns tracking on or off.  Allowed only while the pileup is empty: fresh, or just after
 * wfa_hip_pileup_clear; otherwise WFA_HIP_EINVAL with a message.  wfa_hip_pileup_clear drops the log and keeps the setting.
 * wfa_hip_pileup_add, with tracking on, also appends the batch's records to the log: a count pass gives records and inserted bases per
 * pair, an exclusive scan places them, the two totals are downloaded, the log grows by doubling, then every pair writes its runs at
 * its scanned offset while the table is added to — no atomics for the log.  COST: ABOUT 24 BYTES PER RECORD AND 1 BYTE PER INSERTED
 * BASE in HBM until the pileup is cleared or destroyed, 16 bytes per pair of scratch during the add, one more pass over the op strings,
 * and the 16-byte download.  The log grows before anything is added: a failed growth returns WFA_HIP_EDEVICE, the message names the
 * byte count, and neither the table nor the log has changed.  wfa_hip_pileup_insertion_stats gives the records and the inserted bases
 * of the log (either pointer may be NULL); WFA_HIP_EINVAL on a pileup that does not track.
 *
 * wfa_hip_pileup_insertions follows the conventions of wfa_hip_pileup_sites: seq = -1 takes every sequence (start = 0, len = -1);
 * *count and *bases_count are always the full numbers (rows, and letters of all rows); only the first min(*count, cap) rows are
 * written, and only the letters of those rows that fit whole in bases_cap — nothing behind them is touched; cap = 0 and bases_cap = 0
 * with NULL rows and bases is the counting call.  Two calls give identical bytes.  Kernels: csrc/wfa_insertions.hpp, k_pileup.hip (the
 * record side), k_insertions.hip (rows selected by the chunk count / scan / scatter of the sites; a bucket per row sized from c6 by a
 * scan; records find their row by binary search; a wave per row picks the allele; a scan over allele_len places the letters).
 * WFA_HIP_EINVAL, nothing launched, nothing written: whatever wfa_hip_pileup_sites refuses (`texts` is taken and checked the same way
 * although the rule needs no letters, so the call shape matches), with min_permille in 0..1000; a pileup that does not track ("... was
 * not made to track insertions"); bases_cap < 0; a NULL count or bases_count; NULL bases with bases_cap > 0.
 *
 * Out of scope: multi-base substitutions, genotypes and strand counts per deletion allele ("deletions" below records deletion runs);
 * more than one alternate allele per site (here: per row), ploidy other than 2, a
 * Fisher or other strand statistic (the four counts are returned; the test is the caller's).  The log keeps no strand per record
 * ("strands and genotypes" below counts strands per base).  Reads that place the same inserted bases at
 * different rows of a repeat are different records at different rows: left-align the batch first ("left alignment" below), which puts
 * every gap at the left end of its repeat as far as the read's own window and its own mismatches allow.
 */
#define WFA_HIP_INSERTION_COLS 8   /* j, pos, depth, ins_count, allele_count, allele_len, alleles, overflow */
#define WFA_HIP_INS_MAX_READS 4096 /* the default of the limit; the environment variable of this name replaces it per call */
int wfa_hip_pileup_track_insertions(wfa_hip_pileup_t* pileup, int on);
int wfa_hip_pileup_insertion_stats(wfa_hip_pileup_t* pileup, int64_t* records, int64_t* bases);
int wfa_hip_pileup_insertions(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                              int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows /* cap x 8, nullable */,
                              int64_t bases_cap, int64_t* bases_count, uint8_t* bases /* bases_cap, nullable */);

/* Host only, needs no GPU.  wfa_hip_ops_insertions: ONE pair's records by the rule above, from its op string and its ASCII pattern
 * bytes: recs[r] = (h, n, offset), h window-relative (the row is t_start + h), offset the first of the record's n column bytes (0..4)
 * in cols.  *count and *cols_count are the full numbers; the first min(*count, cap) records are written, and of those the column bytes
 * of the records that fit whole in cols_cap; nothing behind them is touched.  Refused (WFA_HIP_EINVAL, nothing written): what
 * wfa_hip_ops_pileup refuses, a negative capacity, a NULL count, NULL recs / cols with a capacity > 0.
 * wfa_hip_insertions_host: the allele rule on `len` rows as wfa_hip_pileup_read returns them (counts: len x 8) and the records of
 * those rows: record r lies on row rec_row[r] (relative to the first of the len rows; records outside are skipped) and has the
 * rec_n[r] column bytes cols[rec_off[r] ..].  Rows are numbered j = seq, pos = start + row; outputs and capacities as
 * wfa_hip_pileup_insertions; WFA_HIP_INS_MAX_READS is read from the environment in the same way.  Refused (WFA_HIP_EINVAL, nothing
 * written): what wfa_hip_sites_host refuses (min_permille in 0..1000), a negative count or capacity, a missing pointer, a record whose
 * column bytes leave cols[0 .. ncols). */
int wfa_hip_ops_insertions(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, int32_t tlen, int64_t cap,
                           int64_t* count, int32_t* recs /* cap x 3 */, int64_t cols_cap, int64_t* cols_count, uint8_t* cols);
int wfa_hip_insertions_host(const int32_t* counts, int64_t len, int32_t seq, int64_t start, int32_t min_depth, int32_t min_permille,
                            int64_t nrec, const int64_t* rec_row, const int32_t* rec_n, const int64_t* rec_off, const uint8_t* cols,
                            int64_t ncols, int64_t cap, int64_t* count, int32_t* rows, int64_t bases_cap, int64_t* bases_count,
                            uint8_t* bases);

/* ---- deletions: what the reads delete, one deletion length per reported row -------------------------------- */

/*
 * Column 5 counts, per reference base, the reads that delete that base.  A pileup that tracks deletions also keeps every deletion as
 * ONE event with a start and a length, in a log on the device, and reduces it there to one length per row.  It is opt-in: a pileup
 * that does not ask for it behaves, allocates and launches exactly as before.  Integers only.  Op letters are WFA's: I is a text
 * base the read lacks.
 *
 * RECORDS.  A pair contributes under exactly the conditions of wfa_hip_pileup_add (status 0, keep, its window inside its text).  Every
 * maximal I run inside its aligned core (first M to last M) is one record (g, n):
 *   g        the global row t_start + h of text j of the run's first deleted base
 *   n        the run's length
 * A D run next to an I run neither breaks nor joins the I run.  Two facts follow:
 *   the number of records that COVER a row (g <= row < g + n) equals that row's column 5;
 *   the number of records that START at a row is at most that row's column 5.
 *
 * STARTS PLANE.  A pileup that tracks deletions keeps one more int32 plane next to the table: starts[g] is the number of records
 * that start at row g.  It is added to with integer adds, as the table is, so it does not depend on how a list is split or ordered.
 *
 * ALLELE OF A ROW.  The alleles are the distinct n among the records that start at the row, count(n) the multiplicity of n.  The
 * row's allele is the n with the greatest count; ties go to the smaller n.  The order is total: the result never depends on the order
 * in which records were stored, added or split over adds.
 *
 * REPORTED ROWS, parameters min_depth >= 1 and min_permille in 0..1000; depth as in "calls and sites", taken at row g; S = starts[g].
 * A row is reported iff depth >= min_depth and
 *   min_permille > 0:   S >= 1 && 1000 * S >= min_permille * depth      (64-bit products)
 *   min_permille == 0:  2 * S > depth
 * Its row is WFA_HIP_DELETION_COLS int32:
 *   j, pos, depth, del_count (= S), allele_count, allele_len, alleles (the number of distinct lengths), overflow
 * pos is the FIRST DELETED BASE, 0-based; VCF anchors a deletion one base earlier (POS = pos in VCF's 1-based numbering, REF = the
 * base in front of the deletion plus the allele_len deleted bases; the reference has the letters, the log keeps none).  Rows come out
 * in ascending (j, pos), always.  A row is selected by where it starts, so its deleted bases may reach past the queried range.  A row
 * with S > WFA_HIP_DEL_MAX_READS is still reported, with overflow = 1 and allele_count = allele_len = alleles = 0: the limit (default
 * 4096; read per call from the environment variable of that name, exactly as WFA_HIP_INS_MAX_READS is; at least 1) bounds the work of
 * the one wave that serves a row.
 *
 * wfa_hip_pileup_track_deletions turns tracking on or off.  Allowed only while the pileup is empty: fresh, or just after
 * wfa_hip_pileup_clear; otherwise WFA_HIP_EINVAL with a message.  Turning it on allocates the zeroed starts plane, 4 MORE BYTES PER TEXT
 * BASE; a failed allocation returns WFA_HIP_EDEVICE, the message names the byte count, and the pileup is unchanged and not tracking.
 * Turning it off frees the plane.  wfa_hip_pileup_clear drops the log, zeroes the plane and keeps the setting.  Tracking deletions does
 * not depend on insertions, strands or qualities, and goes with every form of the add: wfa_hip_pileup_add, _add_strands and _add_quals
 * make exactly their own adds to their tables — the table kernels are the ones a pileup without the log runs — and the deletion log
 * gets a pass of its own: a count pass gives records and deleted bases per pair, an exclusive scan places the records, the two totals
 * are downloaded, the log grows by doubling, the tables are added to, then every pair writes its records at its scanned offset and adds
 * 1 to starts[g] per record.  COST: 16 BYTES PER RECORD in HBM until the pileup is cleared or destroyed, the 4 bytes per text base of
 * the plane, 8 bytes of counts per pair (and the two 64-bit prefixes of the scans) of scratch during the add, one more pass over the op
 * strings, and the 16-byte download.  The log grows before anything is written: a failed growth returns WFA_HIP_EDEVICE, the message
 * names the byte count, and neither a table nor the log nor the plane has changed.  wfa_hip_pileup_deletion_stats gives the records
 * of the log and the sum of their lengths (either pointer may be NULL); wfa_hip_pileup_read_deletion_starts copies starts[] of the
 * rows [start, start + len) of sequence seq, as wfa_hip_pileup_read copies the table's; both WFA_HIP_EINVAL on a pileup that does not
 * track.
 *
 * wfa_hip_pileup_deletions follows the conventions of wfa_hip_pileup_insertions: seq = -1 takes every sequence (start = 0, len = -1);
 * *count is always the full number; only the first min(*count, cap) rows are written, and nothing behind them is touched; cap = 0
 * with rows = NULL is the counting call.  Two calls give identical bytes.  Kernels: csrc/wfa_deletions.hpp, k_deletions.hip (the record
 * side: a wave per pair, 64 ops per round, run starts from the I ballot and the last op of the round before, a run that crosses a
 * round boundary carried wave-uniformly; rows selected by the chunk count / scan / scatter of the sites; a bucket per row sized from S
 * by a scan; records find their row by binary search; a wave per row picks the length).  WFA_HIP_EINVAL, nothing launched, nothing
 * written: whatever wfa_hip_pileup_insertions refuses of these arguments (min_permille in 0..1000), and a pileup that does not track
 * ("... was not made to track deletions").
 *
 * Out of scope: multi-base substitutions; genotypes and strand counts per deletion allele; more than one allele per row.  Reads that
 * place the same deleted bases at different rows of a repeat are different records at different rows: left-align the batch first
 * ("left alignment" below), which puts every gap at the left end of its repeat as far as the read's own window and its own
 * mismatches allow.
 */
#define WFA_HIP_DELETION_COLS 8    /* j, pos, depth, del_count, allele_count, allele_len, alleles, overflow */
#define WFA_HIP_DEL_MAX_READS 4096 /* the default of the limit; the environment variable of this name replaces it per call */
int wfa_hip_pileup_track_deletions(wfa_hip_pileup_t* pileup, int on);
int wfa_hip_pileup_deletion_stats(wfa_hip_pileup_t* pileup, int64_t* records, int64_t* bases);
int wfa_hip_pileup_read_deletion_starts(wfa_hip_pileup_t* pileup, int32_t seq, int64_t start, int64_t len, int32_t* out /* len */);
int wfa_hip_pileup_deletions(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                             int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows /* cap x 8, nullable */);

/* Host only, needs no GPU.  wfa_hip_ops_deletions: ONE pair's records by the rule above, from its op string: recs[r] = (h, n), h
 * window-relative (the row is t_start + h).  *count is the full number; the first min(*count, cap) records are written, nothing behind
 * them is touched.  Refused (WFA_HIP_EINVAL, nothing written): a negative length or capacity, a missing pointer, an op string that
 * consumes more than plen pattern or tlen text bases.
 * wfa_hip_deletions_host: the allele rule on `len` rows as wfa_hip_pileup_read returns them (counts: len x 8), their starts as
 * wfa_hip_pileup_read_deletion_starts returns them (starts: len) and the records that start at those rows: record r starts at row
 * rec_row[r] (relative to the first of the len rows; records outside are skipped) and has length rec_n[r].  Rows are numbered j = seq,
 * pos = start + row; count, cap and rows as wfa_hip_pileup_deletions; WFA_HIP_DEL_MAX_READS is read from the environment in the same
 * way.  Refused (WFA_HIP_EINVAL, nothing written): what wfa_hip_sites_host refuses (min_permille in 0..1000), a negative count or
 * capacity, a missing pointer, a record of length below 1. */
int wfa_hip_ops_deletions(const uint8_t* ops, int64_t ops_len, int32_t plen, int32_t tlen, int64_t cap, int64_t* count,
                          int32_t* recs /* cap x 2: h, n */);
int wfa_hip_deletions_host(const int32_t* counts, const int32_t* starts, int64_t len, int32_t seq, int64_t start, int32_t min_depth,
                           int32_t min_permille, int64_t nrec, const int64_t* rec_row, const int32_t* rec_n, int64_t cap,
                           int64_t* count, int32_t* rows);

/* ---- strands and genotypes: per-strand counts, and a diploid genotype per variant site ---------------------- */

/*
 * A site seen on one strand only is the classic artefact every caller filters, and "0/1 or 1/1, and how sure" is the first thing a
 * caller asks of a site.  Both are integer reductions of data already resident.  Strand tracking is opt-in: a pileup that does not ask
 * for it behaves, allocates and launches exactly as before.  Integers only, 64-bit products.
 *
 * STRANDS.  wfa_hip_pileup_track_strands turns tracking on or off.  Allowed only while the pileup is empty: fresh, or just after
 * wfa_hip_pileup_clear; otherwise WFA_HIP_EINVAL with a message.  Turning it on allocates a second zeroed table, the FORWARD TABLE: the
 * same 8 planes, plane stride and layout (csrc/wfa_pileup.hpp), 32 MORE BYTES PER TEXT BASE; a failed allocation returns
 * WFA_HIP_EDEVICE, the message names the byte count, and the pileup is unchanged and not tracking.  Turning it off frees that table.
 * wfa_hip_pileup_clear keeps the setting and zeroes both tables.  Strand tracking and insertion tracking are independent; both may be
 * on, and the insertion log is the same either way (no strand per record).
 *
 * wfa_hip_pileup_add_strands does exactly what wfa_hip_pileup_add does to the table; in addition a pair with reverse[q] == 0 makes the
 * same adds to the same rows and columns of the forward table (reverse NULL: every pair is forward).  reverse is the strand array given
 * to wfa_hip_batch_create_windows; the letters counted are the batch's either way, i.e. on the text's strand.  Reverse counts are
 * total - forward and are never stored.  10 bytes per pair uploaded.  Its refusals are those of wfa_hip_pileup_add, and a pileup that
 * does not track strands.  wfa_hip_pileup_add on a pileup that tracks strands is refused, the message names this call.  Kernel:
 * k_pileup.hip, the table kernel (and its insertion-tracking form) compiled with a STRANDS flag: the strand is uniform over the wave
 * that serves a pair, a forward pair issues each atomicAdd twice.
 *
 * wfa_hip_pileup_read_strand is wfa_hip_pileup_read for one strand (0 forward, 1 reverse = total - forward, subtracted on the host):
 * the same checks, plus WFA_HIP_EINVAL for a strand outside {0, 1} and for a pileup that does not track strands.
 *
 * GENOTYPED SITES.  For base g take c0..c7, r, depth, alt, A = c[alt], snv and ins exactly as SITE ("calls and sites") defines them
 * and, on a tracking pileup, f0..f7 from the forward table and depth_fwd = f0 + ... + f5.  Parameters: min_depth >= 1, min_permille in
 * 1..1000, err_q in 1..60, min_alt_strand >= 0 (a value above 0 needs a tracking pileup).
 *   snv' = snv && f[alt] >= min_alt_strand && A - f[alt] >= min_alt_strand
 *   ins' = ins && f6 >= min_alt_strand && c6 - f6 >= min_alt_strand
 * (min_alt_strand == 0: snv' = snv, ins' = ins.)  A base of depth >= min_depth is reported iff snv' || ins'.
 *
 * GENOTYPE of an event with R reference reads and A alternate reads:
 *   L0 = err_q * A  (genotype 0/0)      L1 = 3 * (R + A)  (0/1)      L2 = err_q * R  (1/1)
 *   gt = the index of the smallest L, the smaller index on a tie;  gq = min(99, second smallest L - smallest L)
 * The 3 is 10 log10 2 rounded: under 0/1 every read had an even chance of showing either allele.  err_q is the phred-scaled cost of a
 * read that contradicts the genotype.  gq is a documented confidence, NOT a calibrated likelihood, as mapq is in "placement": no base
 * qualities, no mapping qualities, no prior enter it.  SNV event: R = c[r], A = c[alt].  Insertion event: A = c6,
 * R = max(0, depth - c6).
 *
 * Row, WFA_HIP_GENOTYPE_COLS int32:
 *   0..7    the site row: j, pos, ref, alt, depth, ref_count, alt_count, ins_count — with snv' in place of snv
 *   8..11   gt, gq (-1, -1 when !snv'), ins_gt, ins_gq (-1, -1 when !ins')
 *   12..15  depth_fwd (its low 32 bits), ref_fwd = f[r], alt_fwd (f[alt]; 0 when !snv'), ins_fwd = f6; all four -1 on a pileup that
 *           does not track strands
 * Rows come out in ascending (j, pos), always; two calls give identical bytes.  With min_alt_strand == 0, columns 0..7 of the rows are
 * byte for byte the rows of wfa_hip_pileup_sites with the same min_depth and min_permille.
 *
 * wfa_hip_pileup_genotypes follows the conventions of wfa_hip_pileup_sites: seq = -1 takes every sequence (start = 0, len = -1);
 * *count is always the full number; the first min(*count, cap) rows are written (cap x 16 int32; rows behind them are not touched);
 * cap = 0 with rows = NULL is the counting call.  Kernels: csrc/wfa_calls.hpp, k_calls.hip — the sites' chunk count / scan / scatter
 * (WFA_HIP_CALLS_CHUNK applies), no atomics; the forward planes are read only at bases that pass SITE; a row is four 16-byte stores.
 * WFA_HIP_EINVAL, nothing launched, nothing written (wfa_hip_last_error names the values): whatever wfa_hip_pileup_sites refuses;
 * err_q outside 1..60; min_alt_strand < 0; min_alt_strand > 0 on a pileup that does not track strands.
 *
 * Out of scope: multi-base substitutions, genotypes and strand counts per deletion allele ("deletions" above records deletion runs,
 * without a genotype); more than one alternate allele per site, ploidy other than 2, a Fisher or other strand statistic
 * (the four counts are returned; the test is the caller's).  Base qualities in the costs: "base qualities" below.
 */
#define WFA_HIP_GENOTYPE_COLS 16  /* the 8 of a site, gt, gq, ins_gt, ins_gq, depth_fwd, ref_fwd, alt_fwd, ins_fwd */
int wfa_hip_pileup_track_strands(wfa_hip_pileup_t* pileup, int on);
int wfa_hip_pileup_add_strands(wfa_hip_pileup_t* pileup, wfa_hip_batch_t* batch, const int32_t* j, const int32_t* t_start /* nullable: 0 */,
                               const uint8_t* keep /* nullable: all */, const uint8_t* reverse /* nullable: all forward */);
int wfa_hip_pileup_read_strand(wfa_hip_pileup_t* pileup, int32_t seq, int64_t start, int64_t len, int strand /* 0 forward, 1 reverse */,
                               int32_t* counts /* len x 8 */);
int wfa_hip_pileup_genotypes(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                             int32_t min_depth, int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap, int64_t* count,
                             int32_t* rows /* cap x 16, nullable */);

/* Host only, needs no GPU: the rule of the genotyped sites on `len` rows as wfa_hip_pileup_read returns them (counts: len x 8) and,
 * for a tracking pileup, as wfa_hip_pileup_read_strand returns them for strand 0 (counts_fwd: len x 8; NULL: not tracking, columns
 * 12..15 are -1), over the reference bytes ref[0 .. len).  Rows are numbered j = seq, pos = start + row; count, cap and rows as
 * wfa_hip_sites_host.  Refused (WFA_HIP_EINVAL, nothing written): what wfa_hip_sites_host refuses, err_q outside 1..60,
 * min_alt_strand < 0, min_alt_strand > 0 with counts_fwd NULL. */
int wfa_hip_genotypes_host(const int32_t* counts, const int32_t* counts_fwd /* nullable */, const uint8_t* ref, int64_t len, int32_t seq,
                           int64_t start, int32_t min_depth, int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap,
                           int64_t* count, int32_t* rows);

/* ---- base qualities: a quality filter, quality sums per base, quality-weighted genotypes ------------------- */

/*
 * A FASTQ record's fourth line says how far each base is to be trusted.  A pileup that tracks qualities leaves bases under a threshold
 * out and sums the qualities of those it counts, and the genotype of a site is then charged what its contradicting reads really
 * cost.  Everything here is opt-in: a pileup that does not ask for it behaves, allocates and launches exactly as before.
 *
 * QUALITY SET.  wfa_hip_qualset_create uploads one byte per base of the sequences of `reads`, RAW PHRED (0 .. WFA_HIP_MAX_QUALITY;
 * not phred + 33), once: entry k is quals[off[k] .. off[k] + len[k]) and belongs to sequence k of `reads`.  Refused (NULL,
 * WFA_HIP_EINVAL as far as an error code goes, nothing allocated; wfa_hip_last_error names the first offending entry): a set of
 * another aligner; a missing pointer; a negative offset; len[k] other than the length of sequence k; a value above 93.  The set keeps
 * the lengths and outlives `reads`.
 *
 * RULE.  The quality of pattern position v of pair q is the stored read's, seen through the pair's window: with r = i[q],
 * s = p_start[q] (NULL: 0) and n the pair's pattern length,
 *   Q(v)  = quals[r][reverse[q] ? s + n - 1 - v : s + v]            (the arrays given to wfa_hip_batch_create_windows are exactly these)
 *   Qc(v) = min(Q(v), quality_cap)
 * with the parameters min_base_quality in 0 .. 93 and quality_cap in 1 .. 93 of the add.  The walk is that of wfa_hip_pileup_add: the
 * same core, the same v, h and g.  ONE THING CHANGES: an M or X with Q(v) < min_base_quality adds NOTHING, no letter and no mismatch,
 * to any table.  I ops and D runs count as they do there, whatever the qualities.  So the sum of columns 0..5 is the number of
 * contributing reads whose aligned core covers the base WITH A BASE THAT PASSED THE FILTER OR WITH A DELETION, which is the depth the
 * calls, sites and genotypes then see.  ONE TABLE IS ADDED, the QUALITY TABLE: the same 8 planes, plane stride and layout, 32 MORE
 * BYTES PER TEXT BASE, int32 and not checked for overflow, as the counts are:
 *   M that passes   +Qc(v) to the letter's column
 *   X that passes   +Qc(v) to the letter's column and to column 7
 *   I               +min(Qc(v - 1), Qc(v)) to column 5: the read bases on either side of the text base the read lacks (an index outside
 *                   [0, n) is left out of the min; the core's first and last M make at least one exist)
 *   D run           +Qc(v) of its first inserted base to column 6, at the row where the run is counted
 * With min_base_quality = 0 the count table is byte for byte that of wfa_hip_pileup_add on the same list.
 *
 * wfa_hip_pileup_track_qualities turns tracking on or off, only while the pileup is empty, as wfa_hip_pileup_track_strands; on
 * allocates the zeroed quality table (a failed allocation: WFA_HIP_EDEVICE, the message names the byte count, the pileup unchanged),
 * off frees it.  wfa_hip_pileup_clear keeps the setting and zeroes the table.  Quality, strand and insertion tracking are independent.
 *
 * wfa_hip_pileup_add_quals is the add of a pileup that tracks qualities, with or without strands: `reverse` is the strand array in
 * both (it orients the qualities, and with strand tracking a pair with reverse[q] == 0 repeats its count adds, filter included, in
 * the forward table; there is no forward quality table).  The insertion log is unaffected: records are written whatever the
 * qualities.  WFA_HIP_EINVAL, nothing launched (the message names the first offending list position): whatever wfa_hip_pileup_add
 * refuses; a pileup that does not track qualities; a quality set of another aligner; a missing i; i[q] outside the set; a negative
 * p_start[q]; p_start[q] + plen[q] behind the read's end; min_base_quality outside 0..93; quality_cap outside 1..93.
 * wfa_hip_pileup_add and wfa_hip_pileup_add_strands on a pileup that tracks qualities are refused, the message names this call.
 * Kernel: k_pileup.hip, the table kernel compiled with a QUALS flag: one byte load per lane (two on an I), ascending over the wave
 * for a forward pair, descending for a reverse one, and one more atomicAdd per add.  18 bytes per pair uploaded.
 *
 * wfa_hip_pileup_read_quality is wfa_hip_pileup_read for the quality table (the same checks, and a pileup that does not track).
 *
 * QUALITY-WEIGHTED GENOTYPES.  wfa_hip_pileup_genotypes_quals takes the arguments of wfa_hip_pileup_genotypes and has its SITE
 * selection, min_alt_strand filter, row layout, count / scan / scatter and order.  Only the three costs of an event change, qsum being
 * the base's row of the quality table:
 *   SNV or deletion event:  L0 = qsum[alt]      L1 = 3 * (R + A)      L2 = qsum[r]
 *   insertion event:        L0 = qsum[6]        L1 = 3 * (R + A)      L2 = err_q * R
 * (R, A as in GENOTYPE.)  A read that does not insert has no base to take a quality from, so the insertion's L2 keeps the constant.
 * 64-bit arithmetic, gq capped at 99.  The quality planes are read only at bases that are reported.  Refused as
 * wfa_hip_pileup_genotypes, and on a pileup that does not track qualities.
 *
 * Out of scope: mapping qualities in the costs, a prior, recalibration; of the multi-base events, substitutions and
 * a genotype or strand counts per deletion allele (deletion runs themselves: "deletions" above).
 */
#define WFA_HIP_MAX_QUALITY 93
typedef struct wfa_hip_qualset wfa_hip_qualset_t;  /* the base qualities of a sequence set, resident in HBM */
wfa_hip_qualset_t* wfa_hip_qualset_create(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* reads, const uint8_t* quals, const int64_t* off,
                                          const int32_t* len);
void wfa_hip_qualset_destroy(wfa_hip_qualset_t* quals);
int wfa_hip_pileup_track_qualities(wfa_hip_pileup_t* pileup, int on);
int wfa_hip_pileup_add_quals(wfa_hip_pileup_t* pileup, wfa_hip_batch_t* batch, const int32_t* j, const int32_t* t_start /* nullable: 0 */,
                             const uint8_t* keep /* nullable: all */, const uint8_t* reverse /* nullable: all forward */,
                             const wfa_hip_qualset_t* quals, const int32_t* i, const int32_t* p_start /* nullable: 0 */,
                             int32_t min_base_quality, int32_t quality_cap);
int wfa_hip_pileup_read_quality(wfa_hip_pileup_t* pileup, int32_t seq, int64_t start, int64_t len, int32_t* qsums /* len x 8 */);
int wfa_hip_pileup_genotypes_quals(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                   int32_t min_depth, int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap,
                                   int64_t* count, int32_t* rows /* cap x 16, nullable */);

/* Host only, needs no GPU: ONE pair's contribution by the rule above, as wfa_hip_ops_pileup: quals[0 .. plen) are the qualities of
 * pattern[0 .. plen) in the window's order (already reversed for a reverse pair); rows and qrows (tlen x 8 each) are added to.
 * WFA_HIP_EINVAL, nothing added: what wfa_hip_ops_pileup refuses, a quality above 93, a parameter out of range. */
int wfa_hip_ops_pileup_quals(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, int32_t tlen, const uint8_t* quals,
                             int32_t min_base_quality, int32_t quality_cap, int32_t* rows /* tlen x 8, added to */,
                             int32_t* qrows /* tlen x 8, added to */);

/* Host only: wfa_hip_genotypes_host with the costs above; qsums: len x 8, the rows wfa_hip_pileup_read_quality returns. */
int wfa_hip_genotypes_quals_host(const int32_t* counts, const int32_t* qsums, const int32_t* counts_fwd /* nullable */, const uint8_t* ref,
                                 int64_t len, int32_t seq, int64_t start, int32_t min_depth, int32_t min_permille, int32_t err_q,
                                 int32_t min_alt_strand, int64_t cap, int64_t* count, int32_t* rows);

/* ---- left alignment: gaps at the left end of their repeat, where VCF puts them ----------------------------- */

/*
 * WFA's backtrace leaves a gap at the RIGHT end of a homopolymer or tandem repeat; VCF, and every tool and truth set that follows it,
 * puts it at the LEFT end.  Left alignment is a pure rewrite of the op string of a status-0 pair, done before the string is reduced, so
 * that summaries, pileups, sites and insertion rows report a gap where a caller expects it, and reads that stopped at different places
 * of one repeat agree as far as their own letters allow.
 *
 * INPUT.  The op string and the pair's own letters P[0 .. plen) and T[0 .. tlen): the batch's letters, so a reverse-strand window is
 * already on the text's strand.
 * CORE.  The aligned core: first M (index `first`) .. last M (index `last`).  Without an M nothing changes.
 * RUNS.  The maximal gap runs (I runs and D runs) that lie wholly inside (first, last), taken in ascending op order over the string as
 * already rewritten.
 * SHIFT.  A run of kind c occupies ops [a, a + L); x is the position in S when the run starts, with S = T and x = h for I, S = P and
 * x = v for D.  While a - 1 > first, ops[a - 1] == 'M' and S[x - 1] == S[x + L - 1] (byte equality; no wildcard rule):
 *     ops[a - 1] = c, ops[a + L - 1] = 'M', then a and x decrease by one.
 * MERGE.  If the run has moved at least once, a - 1 > first and ops[a - 1] == c, the run in front of it and this one are one run from
 * here on: a goes to the start of that earlier run, L grows by its length, x drops by its length, and SHIFT goes on with the larger L.
 * STOP.  Anything else in front of the run stops it: an X, a gap of the other kind, the core's first M.
 *
 * What follows from the rule:
 *   - the string keeps its length, its count of every letter, its `first` and its `last`, so `locations` (and with them the interval
 *     a placement sees) do not change;
 *   - every M still pairs equal letters;
 *   - applying the rule twice gives the bytes of applying it once;
 *   - the reported score stays WFA's and is NOT recomputed: under gap-affine and gap-affine-2p a shift costs nothing; a merge (which
 *     the one-component metrics produce) can only improve the score of the string.
 * Out of scope: moving a gap through a mismatch; joint realignment across reads; re-scoring; normalising against anything but the
 * pair's own window (a gap cannot move left of the window or of the core's first M).
 *
 * wfa_hip_batch_left_align waits for the batch's last run and rewrites the op strings of its status-0 pairs in place, in the batch's
 * device buffer; nothing crosses PCIe but the two counters.  Everything read from the batch afterwards sees the rewritten strings:
 * wfa_hip_batch_results, wfa_hip_batch_rle_counts / _rle_runs, wfa_hip_batch_summary, wfa_hip_pileup_add, wfa_hip_placer_add.  The
 * run-length encoding the batch may hold is dropped (call wfa_hip_batch_rle_counts again).  A new wfa_hip_batch_run brings WFA's own
 * strings back.  stats (nullable): [0] the runs that moved, [1] the merges, summed over the batch; a second call changes nothing and
 * reports zeros.  Kernel: csrc/wfa_leftalign.hpp, k_leftalign.hip (a wave per pair; a pair without a gap inside its core is left
 * without a store).  WFA_HIP_EINVAL, nothing launched: what wfa_hip_batch_summary refuses (a batch of scope score, or without a
 * finished run).
 */
int wfa_hip_batch_left_align(wfa_hip_batch_t* batch, int64_t* stats /* nullable; [0] runs moved, [1] merges */);

/* Host only, needs no GPU: the rule for ONE pair, in place, from its op string and its ASCII pattern and text bytes.  Returns
 * WFA_HIP_OK, or WFA_HIP_EINVAL with nothing changed on a negative length, a missing pointer, or an op string that does not consume
 * exactly plen pattern and tlen text bases. */
int wfa_hip_ops_left_align(uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen,
                           int64_t* stats /* nullable; [0] runs moved, [1] merges */);

/* ---- SAM fields: POS, soft clips, a SAM CIGAR, NM and MD per pair ---------------------------------------- */

/*
 * What a batch returns about an alignment is in WFA's vocabulary: op letters M X I D with D meaning "the read inserts" and I meaning
 * "the read deletes" (the opposite of SAM), coordinates relative to a window, free ends as leading or trailing gap ops, no NM and no
 * MD.  These entries turn the op string and the text letters the batch holds into the per-read fields a SAM record wants.
 *
 * INPUT.  One pair gives its op string, its status, plen and tlen, and its own text letters T[0 .. tlen): the batch's letters, so a
 * reverse-strand window is already on the text's strand, which is SAM's convention for SEQ.  Op letters are the library's: M and X
 * consume a pattern base and a text base, D a pattern base only, I a text base only.
 * FLAGS.  WFA_HIP_SAM_EQX writes = and X instead of folding both into M.  WFA_HIP_SAM_CORE makes the anchors M only; without it the
 * anchors are M and X.
 * SPAN.  f is the first anchor op, l the last.  A pair whose status is not 0, whose op string is empty, or that has no anchor op is
 * UNMAPPED: its row is {-1, 0, 0, 0, 0, 0, 0, 0} and both of its strings are empty.  Without WFA_HIP_SAM_CORE the span runs from the
 * first to the last op that pairs two bases, as whole-read aligners write it; with it the span is the aligned core of `locations`,
 * pos is `locations`' text_start, and the clips take the outer mismatches.
 * ROW.  WFA_HIP_SAM_COLS int32:
 *   0  pos         the X and I ops before f: 0-based and window-relative (a SAM writer adds the window's start and 1)
 *   1  ref_len     the M, X and I ops in [f, l]
 *   2  clip_left   the X and D ops before f
 *   3  clip_right  the X and D ops after l
 *   4  nm          the X, I and D ops in [f, l]
 *   5  cigar_len   the byte length of the CIGAR string
 *   6  md_len      the byte length of the MD string
 *   7  query_len   the M, X and D ops in [f, l]
 * so that clip_left + query_len + clip_right == plen and pos + ref_len <= tlen.
 * CIGAR.  clip_left and S when clip_left is not zero; then the maximal runs of the span after the mapping M -> M (= under EQX),
 * X -> M (X under EQX), D -> I, I -> D, each as its decimal length and its letter (a run is maximal AFTER the mapping: without EQX,
 * MMXM is 4M); then clip_right and S when clip_right is not zero.  Text ops outside the span only move pos.
 * MD.  The form of samtools calmd, [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*: walk the span with `run`, the M ops since the last event.  An X at
 * text offset h emits run and the letter T[h], and run = 0.  The first op of a maximal I run (maximal in the op string) emits run, ^
 * and its letter, and run = 0; every further I of that run emits its letter.  D ops emit nothing and do not break run.  The end emits
 * run.  A zero run is therefore always written.  Letters are the bytes the batch holds for the text base: ACGT from the 2-bit words,
 * the stored byte for a pair on the byte path.  There is no wildcard rule: an M is a match whatever the letters are.
 * Examples (ops, T, flags: CIGAR, MD):
 *   MMXMIIMDM    ACGTACGT  none  4M2D1M1I1M      2G1^AC2       row 0, 8, 0, 0, 4, 10, 7, 7
 *   MMXMIIMDM    ACGTACGT  EQX   2=1X1=2D1=1I1=  2G1^AC2
 *   DDIIIMMMXMD  ACGTACGT  none  2S5M1S          3G1           pos 3, ref_len 5, nm 1
 *   XMMMX        ACGTA     none  5M              0A3A0         nm 2
 *   XMMMX        ACGTA     CORE  1S3M1S          3             pos 1, nm 0
 *   MIIDIIXM     ACGTACG   none  1M2D1I2D2M      1^CG0^TA0C1
 * Out of scope: FLAG, RNEXT, PNEXT and TLEN (integer arithmetic on the rows of a placement plus these columns); writing SAM or BAM;
 * hard clips; these fields on placements, pileups and host-buffer batches; feeding unclipped ends to the duplicate marker; lower-case
 * or wildcard letters in MD beyond "the stored byte".
 *
 * Two steps, like wfa_hip_batch_rle_counts / _rle_runs, over the last run of a resident batch (after a wfa_hip_batch_left_align: over
 * the rewritten strings):
 *   step 1  wfa_hip_batch_sam_counts: rows[n x 8], and the bytes of all CIGAR and of all MD strings
 *   step 2  wfa_hip_batch_sam_strings: the two blobs; pair q's strings start at the prefix sums of columns 5 and 6 of the rows
 * The offsets are made on the device and stay there; the flags of step 1 hold for step 2.  WFA_HIP_EINVAL, nothing launched: what
 * wfa_hip_batch_summary refuses (a batch of scope score, or without a finished run), unknown flag bits, a missing output, and step 2
 * without a step 1 since the batch's last run or left alignment.  n = 0 is fine.  Kernels: csrc/wfa_sam.hpp, k_sam.hip (a wave per
 * pair, two passes around a 64-bit scan).  wfa_hip_batch_sam_kernel_ms: the HIP-event time of both passes of the last two calls.
 */
#define WFA_HIP_SAM_COLS 8
#define WFA_HIP_SAM_EQX  1
#define WFA_HIP_SAM_CORE 2
int wfa_hip_batch_sam_counts(wfa_hip_batch_t* batch, int flags, int32_t* rows /* n x 8 */, int64_t* cigar_bytes, int64_t* md_bytes);
int wfa_hip_batch_sam_strings(wfa_hip_batch_t* batch, uint8_t* cigar /* cigar_bytes */, uint8_t* md /* md_bytes */);
int wfa_hip_batch_sam_kernel_ms(wfa_hip_batch_t* batch, float* ms);

/* Host only, needs no GPU: the rule for ONE pair, from its op string and its ASCII text: row8, and cigar[0 .. row8[5]) and
 * md[0 .. row8[6]).  Returns WFA_HIP_OK, or WFA_HIP_EINVAL with nothing written when a buffer is too small, a pointer is missing, a
 * flag bit is unknown, or the op string does not consume exactly plen pattern and tlen text bases. */
int wfa_hip_ops_sam(const uint8_t* ops, int64_t ops_len, const uint8_t* text, int32_t tlen, int32_t plen, int flags,
                    int32_t* row8, uint8_t* cigar, int64_t cigar_cap, uint8_t* md, int64_t md_cap);

/* ---- placement: one row per read from the hits of any number of batches ---------------------------------- */

/*
 * The seed and chain queries give up to n candidate windows per read and a windowed batch aligns them all; what a mapper wants next is
 * where each read GOES: its best hit, how far the runner-up at another place is behind, and which hits are merely the same place found
 * twice.  The hits are recorded on the device where the batches lie, grouped by read and reduced there; 32 bytes per read and 1 byte
 * per hit cross PCIe.  Integers only.
 *
 * HIT.  One aligned pair: its read i and text j, its strand `reverse` (0 or 1), score and status, a text interval [ts, te) in
 * coordinates of text j, and its HIT NUMBER: its position in the order of the adds (the first add first, list order within an add).
 * ELIGIBLE.  status == 0 && score >= min_score.  min_score = INT32_MIN keeps every hit of status 0.
 * PRIMARY of a read: its eligible hit of greatest score; on a tie the smallest hit number.
 * SAME LOCUS.  Eligible hit h is at the locus of the primary p iff h != p, j_h == j_p, reverse_h == reverse_p, and
 *     ov = min(te_h, te_p) - max(ts_h, ts_p)   has   ov > 0 && 2 * ov >= min(te_h - ts_h, te_p - ts_p)        (64-bit)
 * so a hit with an empty interval (te <= ts) is never at the same locus, and neither is p at one's.
 * RUNNER-UP.  `second` is the greatest score among the eligible hits that are neither p nor at p's locus; `ties` the number of those
 * whose score equals p's.
 * MAPPING QUALITY.  60 when there is no runner-up; otherwise min(60, 60 * (score_p - second) / full_gap), the product and the floor
 * division in 64 bits, full_gap >= 1: a tie gives 0, a runner-up full_gap or more behind gives 60.  It is a documented confidence, not a
 * calibrated probability; score, second and ties are returned so that a caller can apply a rule of their own.
 *
 * PER READ WFA_HIP_PLACE_COLS int32: hit (the primary's hit number), score, second (INT32_MIN without a runner-up), mapq, hits (the
 * read's eligible hits), ties, text_start, text_end (the primary's [ts, te)).  A read without an eligible hit gets
 * -1, INT32_MIN, INT32_MIN, 0, 0, 0, 0, 0.
 * PER HIT one byte: 0 not eligible, 1 eligible at another locus, 2 at the locus of the primary, 3 the primary.
 *
 * INTERVAL OF A BATCH'S PAIR q, with t0 = t_start[q] (0 when t_start is NULL).  Scope full: [t0 + loc_ts, t0 + loc_te), loc_ts and
 * loc_te being exactly columns 8 and 9 of wfa_hip_batch_summary for the pair: the aligned core; for an op string without an M
 * loc_te <= loc_ts, an empty interval.  Scope score: the whole window [t0, t0 + tlen[q]), tlen[q] the batch's own text length.
 *
 * CLIPS.  Every hit also carries two integers, lead and trail: the bases of the read that the aligned core leaves out on either side.
 * For a pair whose op string has an M, lead is the number of pattern-consuming ops (X and D) in front of the first M and trail the
 * number behind the last M, each saturated at WFA_HIP_CLIP_MAX = 65 535.  A pair with no M, an empty op string, plen == 0 or
 * tlen == 0 has lead = trail = 0, and so has every pair under scope score.  The UNCLIPPED INTERVAL of a hit is
 *     us = ts - lead,   ue = te + trail                                                                  (64-bit)
 * where the read's first and last base would land if the clipped ends were laid down without gaps; us may be negative and ue beyond
 * its text for a read that hangs over an end.  For a mapped pair under wfa_hip_batch_sam_counts with WFA_HIP_SAM_CORE (Python:
 * sam=True, clip_mismatches=True), whose pos is relative to the window's start t0, lead == clip_left and trail == clip_right below
 * the cap, so us == t0 + pos - clip_left and ue == t0 + pos + ref_len + clip_right.  The clips share the record's last word: a hit
 * stays 37 bytes.  wfa_hip_placer_add fills them on the device from the walk that gives the interval; wfa_hip_placer_add_hits_clips
 * takes them from host arrays (either NULL: 0; a negative value is refused, one above the cap saturated), wfa_hip_placer_add_hits
 * gives 0.  wfa_hip_placer_read_clips downloads lead and trail of all hits so far (wfa_hip_placer_count int32 each, 32 bytes per
 * hit cross PCIe): for tests, and for a SAM writer that wants the chosen hit's soft clips.  wfa_hip_ops_clips (host only, no GPU)
 * states the rule for one op string.  Placement, pairing and rescue never read them; "duplicates" may.
 *
 * wfa_hip_placer_create: a placer over reads 0 .. nreads - 1 (nreads >= 0), without hits.  37 BYTES PER HIT AND 36 PER READ in HBM
 * (csrc/wfa_place.hpp), the records grown by doubling; a failed allocation: WFA_HIP_EDEVICE, the message names the byte count.
 * wfa_hip_placer_add waits for the batch's last run, as wfa_hip_pileup_add does, and appends its pairs as hits: pair q is a hit of
 * read i[q] on text j[q] from t_start[q], on the strand reverse[q] != 0 (the arrays given to wfa_hip_batch_create_windows are exactly
 * these; reverse NULL: forward).  One kernel; 13 bytes per pair uploaded, nothing downloaded.  The batch may be destroyed afterwards:
 * a list too long for one batch is added chunk by chunk.
 * wfa_hip_placer_add_hits appends n hits from host arrays (reverse nullable), for hits aligned elsewhere.
 * wfa_hip_placer_run groups and reduces ALL hits added so far: rows receives nreads x WFA_HIP_PLACE_COLS int32, row-major; flags,
 * when not NULL, wfa_hip_placer_count bytes.  It may be called again with other parameters (the grouping is kept), and adds after a
 * run are legal: the next run sees every hit.  Rows and flags depend on the hits alone, never on scheduling: two runs give identical
 * bytes.  Kernels: csrc/wfa_place.hpp, k_place.hip (count per read, exclusive scan, scatter; then a wave per read).  A READ WITH A VERY
 * LARGE GROUP OF HITS IS SERVED BY ONE WAVE; that is the design, not a defect: groups come from n <= WFA_HIP_SEED_MAX_N candidates.
 * wfa_hip_placer_count: the hits so far.  wfa_hip_placer_clear drops them (the capacity stays).  wfa_hip_placer_kernel_ms: the
 * HIP-event time of the last run's kernels (0 before the first).
 * WFA_HIP_EINVAL, nothing launched, nothing appended (wfa_hip_last_error names the first offending position and its values): a batch
 * of another aligner or without a finished run; i[q] outside [0, nreads); a negative j[q], t_start[q] or text_start[q];
 * text_end[q] < text_start[q]; full_gap < 1; more than 2^31 - 1 hits in all; a NULL pointer where an array is needed.
 */
#define WFA_HIP_PLACE_COLS 8   /* hit, score, second, mapq, hits, ties, text_start, text_end */
typedef struct wfa_hip_placer wfa_hip_placer_t;
wfa_hip_placer_t* wfa_hip_placer_create(wfa_hip_aligner_t* aligner, int64_t nreads);
int  wfa_hip_placer_add(wfa_hip_placer_t* placer, wfa_hip_batch_t* batch, const int32_t* i, const int32_t* j,
                        const int32_t* t_start /* nullable: 0 */, const uint8_t* reverse /* nullable: forward */);
int  wfa_hip_placer_add_hits(wfa_hip_placer_t* placer, int64_t n, const int32_t* i, const int32_t* j, const uint8_t* reverse /* nullable */,
                             const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end);
#define WFA_HIP_CLIP_MAX 65535   /* lead and trail saturate here */
int  wfa_hip_placer_add_hits_clips(wfa_hip_placer_t* placer, int64_t n, const int32_t* i, const int32_t* j,
                                   const uint8_t* reverse /* nullable */, const int32_t* score, const int32_t* status,
                                   const int32_t* text_start, const int32_t* text_end, const int32_t* lead /* nullable: 0 */,
                                   const int32_t* trail /* nullable: 0 */);
int  wfa_hip_placer_read_clips(wfa_hip_placer_t* placer, int32_t* lead /* nhits */, int32_t* trail /* nhits */);
/* Host only, needs no GPU: lead and trail of one op string (ops_len bytes of M, X, I, D) of a pair of plen pattern and tlen text
 * bases.  WFA_HIP_EINVAL for a NULL output, a negative length or NULL ops with ops_len > 0. */
int  wfa_hip_ops_clips(const uint8_t* ops, int64_t ops_len, int32_t plen, int32_t tlen, int32_t* lead, int32_t* trail);
int  wfa_hip_placer_run(wfa_hip_placer_t* placer, int32_t min_score, int32_t full_gap, int32_t* rows /* nreads x 8 */,
                        uint8_t* flags /* nhits, nullable */);
int64_t wfa_hip_placer_count(const wfa_hip_placer_t* placer);
int  wfa_hip_placer_clear(wfa_hip_placer_t* placer);
int  wfa_hip_placer_kernel_ms(const wfa_hip_placer_t* placer, float* ms);
void wfa_hip_placer_destroy(wfa_hip_placer_t* placer);

/* Host only, needs no GPU: the rule above in plain C++ over arrays of nhits hits in hit-number order (reverse nullable: forward):
 * what wfa_hip_placer_add_hits + wfa_hip_placer_run give.  Returns WFA_HIP_OK, or WFA_HIP_EINVAL (nothing written; msg, when not NULL,
 * receives up to msg_cap bytes: the device entries' message) for a negative count, a hit the device entries refuse, full_gap < 1 or
 * a missing array. */
int wfa_hip_place_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse, const int32_t* score,
                       const int32_t* status, const int32_t* text_start, const int32_t* text_end, int32_t min_score, int32_t full_gap,
                       int32_t* rows /* nreads x 8 */, uint8_t* flags /* nhits, nullable */, char* msg, size_t msg_cap);

/* ---- pairing: one row per fragment of two reads from the hits of a placer ---------------------------------- */

/*
 * Short reads come in pairs, and the mate is the strongest placement evidence there is: a read inside an exact repeat has mapq 0 on
 * its own, whichever copy its mate sits next to.  The join of the two mates' hits is made where the records lie, after the group and
 * place passes of the same placer; 48 bytes per fragment and 1 byte per hit cross PCIe.  Integers only, nothing depends on scheduling.
 *
 * HIT, ELIGIBLE, PRIMARY, SAME LOCUS and the single-end row are those of "placement"; se(r) is read r's single-end row under the same
 * min_score and full_gap, and a hit's single-end flag its byte there.
 * FRAGMENT.  Fragment f is two distinct reads, mate1[f] and mate2[f]; with both arrays NULL, mate1[f] = 2 f and mate2[f] = 2 f + 1,
 * and 2 * nfrag <= nreads.  A read belongs to at most one fragment.  Reads in no fragment are untouched by the pairing: their
 * pair_flags equal their single-end flags.
 * PAIRING.  (h, g), h an eligible hit of mate 1 and g an eligible hit of mate 2.  It is PROPER iff
 *     j_h == j_g && reverse_h != reverse_g;
 *     te_h > ts_h && te_g > ts_g (both intervals non-empty);
 *     with F the one of reverse == 0 and R the other:  ts_F <= ts_R && te_F <= te_R  (the mates face each other, neither extends
 *     past the other);
 *     min_insert <= te_R - ts_F <= max_insert                                                                     (64-bit)
 * with 0 <= min_insert <= max_insert.  `insert` of a pairing is te_R - ts_F; its PAIR SCORE is score_h + score_g in 64 bits, saturated
 * to [INT32_MIN + 1, INT32_MAX] where it is returned as int32 (nowhere else).
 * BEST.  The proper pairing of greatest pair score; on a tie the smallest hit number of h, then of g.
 * PROPER FRAGMENT.  proper = 1 iff both mates have an eligible hit, a proper pairing exists and
 *     pairscore(best) + unpaired >= se(mate1).score + se(mate2).score                                   (64-bit, unpaired >= 0)
 * `unpaired` being the number of score points a mapper gives up to keep the mates together.  When proper, the CHOSEN hits are (h, g)
 * of the best pairing; otherwise the single-end primaries, -1 where there is none.
 * SAME PLACE.  A proper pairing (h', g') is at the place of the chosen (h, g) iff (h' == h or h' is at h's locus by the SAME LOCUS
 * test with h in the role of p) and the same holds for g' and g.
 * RUNNER-UP.  `second` is the greatest pair score among the proper pairings not at the chosen place, `ties` the number of those whose
 * pair score equals the chosen one's (0 when proper = 0).  `pairings` is the number of proper pairings, the chosen one included; it is
 * reported even when proper = 0.
 * PAIR MAPQ.  60 without a runner-up; otherwise min(60, 60 * (pairscore - second) / full_gap), a 64-bit floor division on the
 * unsaturated values; 0 when proper = 0.
 * MATE MAPQ.  When proper, for mate m with chosen hit c: max(pair mapq, se(m).mapq) if c's single-end flag is 3 or 2 (c is that read's
 * own primary or at its locus), else the pair mapq.  When not proper, se(m).mapq.
 * OVERFLOW.  With E1, E2 the column `hits` of the two single-end rows: a fragment with E1 * E2 > WFA_HIP_PAIR_MAX_PAIRINGS is not
 * joined and gets overflow = 1, proper = 0, pairings = 0.  The bound is why A FRAGMENT IS SERVED BY ONE WAVE can stay the design: at
 * most WFA_HIP_PAIR_MAX_PAIRINGS / 64 rounds of eligible pairings a pass.
 *
 * PER FRAGMENT WFA_HIP_PAIR_COLS int32: hit1, hit2 (the chosen hits), proper, score, second, mapq, mapq1, mapq2, insert, pairings,
 * ties, overflow.  score and second are INT32_MIN when proper = 0, second is INT32_MIN without a runner-up, insert is 0 when
 * proper = 0.
 * PER HIT one byte, pair_flags: the single-end flag relative to the CHOSEN hit c of its read: 3 = c, 2 = eligible at c's locus,
 * 1 = eligible elsewhere, 0 = not eligible.
 *
 * wfa_hip_placer_run_pairs groups ALL hits added so far (the grouping is shared with wfa_hip_placer_run), reduces every read as
 * wfa_hip_placer_run does and then joins every fragment: one wave per fragment over the slots of the two groups (csrc/wfa_place.hpp).
 * rows (nreads x WFA_HIP_PLACE_COLS), flags and pair_flags (wfa_hip_placer_count bytes each) are nullable; pair_rows receives
 * nfrag x WFA_HIP_PAIR_COLS int32.  8 bytes per fragment are uploaded (none for interleaved mates), 48 per fragment downloaded plus the
 * nullable outputs asked for.  It may be called before, after or between calls of wfa_hip_placer_run and adds, under the same rules;
 * wfa_hip_placer_kernel_ms then covers the pair kernel too.  Two runs give identical bytes.
 * WFA_HIP_EINVAL, nothing launched, nothing written (wfa_hip_last_error names the first offending position and its values): what
 * wfa_hip_placer_run refuses; nfrag < 0; min_insert < 0, max_insert < min_insert or unpaired < 0; a mate outside [0, nreads);
 * mate1[f] == mate2[f]; a read named by two fragments; exactly one of mate1 / mate2 NULL; 2 * nfrag > nreads with both NULL; a NULL
 * pair_rows with nfrag > 0.
 */
#define WFA_HIP_PAIR_COLS 12   /* hit1, hit2, proper, score, second, mapq, mapq1, mapq2, insert, pairings, ties, overflow */
#define WFA_HIP_PAIR_MAX_PAIRINGS 65536
int  wfa_hip_placer_run_pairs(wfa_hip_placer_t* placer, int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert,
                              int32_t unpaired, int64_t nfrag, const int32_t* mate1 /* nullable */, const int32_t* mate2 /* nullable */,
                              int32_t* rows /* nreads x 8, nullable */, uint8_t* flags /* nhits, nullable */,
                              int32_t* pair_rows /* nfrag x 12 */, uint8_t* pair_flags /* nhits, nullable */);

/* Host only, needs no GPU: the rule above in plain C++ over arrays of nhits hits in hit-number order (reverse nullable: forward): what
 * wfa_hip_placer_add_hits + wfa_hip_placer_run_pairs give.  Returns WFA_HIP_OK, or WFA_HIP_EINVAL (nothing written; msg as for
 * wfa_hip_place_host) for whatever wfa_hip_place_host refuses and for the refusals of wfa_hip_placer_run_pairs. */
int wfa_hip_pair_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse, const int32_t* score,
                      const int32_t* status, const int32_t* text_start, const int32_t* text_end, int32_t min_score, int32_t full_gap,
                      int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag, const int32_t* mate1 /* nullable */,
                      const int32_t* mate2 /* nullable */, int32_t* rows /* nreads x 8, nullable */, uint8_t* flags /* nhits, nullable */,
                      int32_t* pair_rows /* nfrag x 12 */, uint8_t* pair_flags /* nhits, nullable */, char* msg, size_t msg_cap);

/* ---- rescue: the window in which a lost mate must lie, from its anchored partner ---------------------------- */

/*
 * The pairing joins the hits it is given.  A fragment whose one mate was never aligned at its true place (a repeat masked by the seed
 * index, too many errors for the seeds, an overflowed seed list) has no proper pairing, however well the other mate is anchored.  The
 * anchored mate, the orientation rule and the insert bounds say where the lost mate must lie; this rule turns them into a window list
 * in the shape wfa_hip_batch_create_windows takes, made where the records lie: 32 bytes per window cross PCIe.  Integers only, 64-bit
 * arithmetic, nothing depends on scheduling.  The terms of "placement" and "pairing" keep their meaning.
 *
 * Inputs: a placer's hits; the parameters of wfa_hip_placer_run_pairs (min_score, full_gap, min_insert, max_insert, unpaired, nfrag,
 * mate1, mate2); len(r), the length of read r in a pattern set; tlen(j), the length of text j in a text set; pad >= 0, min_len >= 0
 * and anchor_mapq in 0 .. 60.
 * RESCUED FRAGMENT.  Fragment f whose pair row under those parameters has proper == 0 && pairings == 0 && overflow == 0.
 * ANCHOR.  For a rescued fragment take mate m = 1, then m = 2, and let a be the single-end primary of mate m (se(m).hit).  Mate m is
 * an anchor iff a >= 0, a's interval is non-empty (te_a > ts_a) and se(m).mapq >= anchor_mapq.  The other mate o then gets ONE window
 * on text j_a, on the strand 1 - reverse_a:
 *     anchor forward (reverse_a == 0; o must be the reverse hit, whose end lies in [ts_a + min_insert, ts_a + max_insert]):
 *         lo = ts_a + min_insert - len(o) - pad,    hi = ts_a + max_insert + pad
 *     anchor reverse (reverse_a == 1; o is the forward hit, whose start lies in [te_a - max_insert, te_a - min_insert]):
 *         lo = te_a - max_insert - pad,             hi = te_a - min_insert + len(o) + pad
 *     in both cases clipped, lo = max(lo, 0), hi = min(hi, tlen(j_a)); the window is made iff hi - lo >= max(min_len, 1) and is
 *     dropped otherwise.
 * A fragment yields 0, 1 or 2 windows: both mates may anchor, for instance when the two single-end primaries lie on different texts.
 * LIST ORDER.  Ascending fragment number; within a fragment the window anchored by mate 1 comes before the one anchored by mate 2.
 * PER WINDOW WFA_HIP_RESCUE_COLS int32 (32 bytes): i (the read to align, mate o), j, text_start (= lo), text_len (= hi - lo), reverse,
 * fragment, anchor (the anchor's hit number) and a spare that is 0.  The first five are exactly the arrays
 * wfa_hip_batch_create_windows takes; the pattern window is the whole read.
 * WHAT RESCUE DOES NOT DO.  It does not rescue a fragment that has proper pairings but lost to its single-end primaries.  It uses no
 * anchor other than the primary.  It does not dedupe against hits the other mate already has: the same-locus rule of the next pair run
 * absorbs those.
 *
 * wfa_hip_placer_rescue runs group, place and pair on the device exactly as wfa_hip_placer_run_pairs does, downloads none of their
 * outputs, and makes the list there (csrc/wfa_place.hpp, k_rescue.hip: a thread per (fragment, anchoring mate) decides, an exclusive
 * scan of the 0 / 1 decisions gives every window its position, a second pass stores the rows; no atomics, the order comes from the
 * scan: two calls give identical bytes).  *count receives the full number of windows and rows the first min(*count, cap) of them
 * (cap x WFA_HIP_RESCUE_COLS int32, row-major; rows behind them are not touched; cap = 0 with rows = NULL is the counting call), the
 * convention of wfa_hip_pileup_sites.  Only the count and those rows are downloaded.  wfa_hip_placer_kernel_ms then covers the rescue
 * kernels too.  A placer keeps, on the host, the hits at which the j it was given rises above all before: the last is the greatest j, and
 * the first with j >= the number of texts is the first hit of the list outside the text set, the one wfa_hip_rescue_host names.
 * WFA_HIP_EINVAL, nothing launched, nothing written (wfa_hip_last_error names the first offending position and its values): what
 * wfa_hip_placer_run_pairs refuses (pair_rows aside); a NULL set or a set of another aligner; a pattern set with fewer sequences than
 * the placer has reads; a hit whose j is not below the number of texts; a negative pad, min_len or cap; anchor_mapq outside 0 .. 60;
 * a NULL count; NULL rows with cap > 0.
 */
#define WFA_HIP_RESCUE_COLS 8   /* i, j, text_start, text_len, reverse, fragment, anchor, spare */
int  wfa_hip_placer_rescue(wfa_hip_placer_t* placer, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts, int32_t min_score,
                           int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag,
                           const int32_t* mate1 /* nullable */, const int32_t* mate2 /* nullable */, int32_t pad, int32_t min_len,
                           int32_t anchor_mapq, int64_t cap, int64_t* count, int32_t* rows /* cap x 8, nullable */);

/* Host only, needs no GPU: the rule above in plain C++ over the arrays wfa_hip_pair_host takes, read_len[nreads] and
 * text_len[ntexts]: what wfa_hip_placer_add_hits + wfa_hip_placer_rescue give.  *count receives the full number of windows,
 * min(*count, cap) rows are written.  Returns WFA_HIP_OK, or WFA_HIP_EINVAL (nothing written; msg as for wfa_hip_place_host) for
 * whatever wfa_hip_pair_host refuses (pair_rows aside); a negative pad, min_len, cap, ntexts, read_len or text_len; anchor_mapq
 * outside 0 .. 60; a hit whose j >= ntexts; a missing pointer (read_len with nreads > 0, text_len with ntexts > 0, count, rows with
 * cap > 0). */
int wfa_hip_rescue_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse, const int32_t* score,
                        const int32_t* status, const int32_t* text_start, const int32_t* text_end, int32_t min_score, int32_t full_gap,
                        int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag, const int32_t* mate1 /* nullable */,
                        const int32_t* mate2 /* nullable */, const int32_t* read_len, int64_t ntexts, const int32_t* text_len,
                        int32_t pad, int32_t min_len, int32_t anchor_mapq, int64_t cap, int64_t* count,
                        int32_t* rows /* cap x 8, nullable */, char* msg, size_t msg_cap);

/* ---- duplicates: the fragments and reads that lie at one place with the same ends, one representative each --- */

/*
 * PCR copies of one fragment land at the same place with the same ends, and every copy adds to a pileup's counts as if it were an
 * independent read: a polymerase error copied ten times looks like ten observations.  This rule groups the placed fragments and reads
 * by (text, strand, ends) where the records lie and names one representative per group; 16 bytes per read and per fragment cross
 * PCIe.  Integers only, 64-bit where sums occur, nothing depends on scheduling.  The terms of "placement" and "pairing" keep their
 * meaning.
 *
 * Inputs: a placer's hits; the parameters of wfa_hip_placer_run_pairs (min_score, full_gap, min_insert, max_insert, unpaired, nfrag,
 * mate1, mate2); tlen(j), the length of text j in a text set.
 * UNITS.  After group, place and pair under those parameters:
 *     PAIR UNIT f: fragment f whose pair row has proper == 1.  h and g are its chosen hits, F the one with reverse == 0 and R the
 *         other.  Key = (j, ts_F, te_R, first), `first` being 1 when F is mate 1's hit and 2 otherwise: F1R2 and F2R1 fragments with
 *         the same ends are different molecules.  Score = the pair row's score (the saturated int32).  Bucket position b = ts_F.
 *     READ UNIT r: a read that is in no fragment, or a mate of a fragment with proper == 0, whose single-end row has hit >= 0 and a
 *         non-empty primary interval (te > ts).  Key = (j, reverse, p5), p5 = ts for a forward primary and te - 1 for a reverse one:
 *         the 5' end, so reverse reads of different lengths that end at the same base are one group.  Score = the single-end score.
 *         b = p5.
 *     Everything else is no unit: a read without an eligible hit, a read whose primary interval is empty, a fragment that is not
 *     proper.  The mates of a pair unit are not read units.  A pair unit and a read unit are never in one group.
 * GROUP.  The units of one kind with equal keys.  Its REPRESENTATIVE is the unit of greatest score, on a tie the one with the smallest
 * unit number (fragment number or read number).
 * BUCKET.  All units, of either kind, with the same (j, b).
 * OVERFLOW.  A bucket with more than WFA_HIP_DUP_MAX_BUCKET units is not resolved: each of its units is alone and carries
 * overflow = 1 (the convention of WFA_HIP_INS_MAX_READS).  A unit whose b lies outside [0, tlen(j)) is alone with overflow = 0: on
 * core coordinates only hits added through wfa_hip_placer_add_hits with invented intervals can have one; on unclipped coordinates
 * (below) a real read that hangs over an end of its text has one.  A unit whose key coordinate does not fit int32 is alone with
 * overflow = 0 too; only invented intervals can have one.
 * ROWS.  WFA_HIP_DUP_COLS int32 (16 bytes) each: rep, size, dup, overflow.  For a unit, rep is its group's representative's unit
 * number (its own for the representative and for a unit that is alone), size the number of units in the group, dup = 1 iff rep is not
 * its own number.  A fragment that is not a pair unit gets -1, 0, 0, 0.  A read that is not a read unit gets -1, 0, d, o, with d and o
 * the dup and overflow of its fragment's pair row when it is a mate of a pair unit, and both 0 otherwise: the read rows' dup column
 * alone filters a read list for a pileup.
 * UNCLIPPED ENDS (wfa_hip_placer_duplicates_ex, WFA_HIP_DUP_UNCLIPPED).  On core coordinates a PCR copy whose first base carries a
 * substitution, or that starts with a small insertion, begins a base later and misses its group.  Under this flag the rule is the
 * same except for the coordinates in keys and buckets, which are the unclipped ones of "placement" (CLIPS): a pair unit's key is
 * (j, us_F, ue_R, first) with b = us_F; a read unit's key is (j, reverse, p5) with p5 = us forward and ue - 1 reverse, b = p5.
 * Group, place and pair — eligibility, same locus, properness and `insert` — keep the core intervals.  Under scope score the clips
 * are 0 and the flag changes nothing.
 * REPRESENTATIVE BY BASE QUALITY (WFA_HIP_DUP_BY_QUALITY).  As short-read pipelines do: qsum(r) is the sum of q over all stored
 * bases of read r in a quality set with q >= min_quality (0 .. WFA_HIP_MAX_QUALITY; 15 is customary), in 64 bits, saturated to
 * INT32_MAX.  A read unit's score is qsum(r), a pair unit's qsum(m1) + qsum(m2), saturated the same way; ties still go to the
 * smallest unit number.  The qualities are those of the whole read, not of a pattern window.
 * WHAT IT DOES NOT DO.  Without the flags: no unclipped coordinates and the representative by alignment score.  With or without:
 * no matching of a lone read against an end of a pair unit; no optical duplicates, no UMIs, no library or read-group split; no
 * hashed plane; clips wider than WFA_HIP_CLIP_MAX saturate.  NOT MEASURED HERE: how many planted copies either rule marks, and what
 * the flags cost; DESIGN.md section 6.4 holds what tools/probes/dup_ends_index.py gave, or says that it was not run.
 *
 * wfa_hip_placer_duplicates runs group, place and pair on the device exactly as wfa_hip_placer_rescue does, downloads none of their
 * outputs, and marks the duplicates there (csrc/wfa_dup.hpp, k_dup.hip: every unit is one 32-byte record with a 64-bit bucket number,
 * counted into a plane that is direct-addressed by the text set's base offsets; a scan and a scatter bring the records into bucket
 * order; a thread per record walks its bucket for the group's size and the maximum of (score, ~unit number), both order-free: two
 * calls give identical bytes).  read_rows receives nreads x WFA_HIP_DUP_COLS int32, pair_rows nfrag x WFA_HIP_DUP_COLS.  nfrag == 0
 * with both mate arrays NULL is the single-end form: every read is a candidate read unit, pair_rows may be NULL.  It may be called
 * before, after or between the placer's other runs and adds; wfa_hip_placer_kernel_ms then covers the new kernels too.
 * DEVICE MEMORY, allocated by the first call and kept on the placer (nothing of it without one): 4 BYTES PER BASE OF THE TEXT SET for
 * the plane plus the scan's chunk sums, 64 bytes per read for the unit records and their bucket-ordered copy, 1 byte per read.  The
 * plane's cost grows with the text set, not with the reads; a hashed plane is not built.
 * WFA_HIP_EINVAL, nothing launched, nothing written (wfa_hip_last_error names the first offending position and its values): what
 * wfa_hip_placer_run_pairs refuses (pair_rows aside); a NULL set or a set of another aligner; a hit whose j is not below the number of
 * texts; NULL read_rows with nreads > 0; NULL pair_rows with nfrag > 0.  A failed allocation: WFA_HIP_EDEVICE with the byte count.
 *
 * wfa_hip_placer_duplicates_ex takes the same arguments and flags, quals, min_quality.  flags == 0 with quals == NULL is
 * wfa_hip_placer_duplicates byte for byte, with its allocations and launches.  WFA_HIP_DUP_UNCLIPPED: the key kernels read the clip
 * word of the records they load anyway; nothing more is allocated or launched.  WFA_HIP_DUP_BY_QUALITY: `quals` is a quality set of
 * this aligner over at least nreads reads, read r of the placer being entry r; one more kernel in front of the key kernels (a wave
 * per read, 16-byte loads of the quality bytes inside the read, byte loads at its unaligned ends, no byte outside the read is
 * loaded; a wave reduction; no LDS, no atomics) writes qsum, 4 BYTES PER READ kept on the placer from the first such call; the key
 * kernels take the score from it.  Two calls give identical bytes.  WFA_HIP_EINVAL, nothing launched, in addition: an unknown flag
 * bit; the quality flag without quals or quals without the flag; min_quality outside 0 .. WFA_HIP_MAX_QUALITY under the flag; a
 * quality set of another aligner or over fewer than nreads reads.
 */
#define WFA_HIP_DUP_UNCLIPPED 1
#define WFA_HIP_DUP_BY_QUALITY 2
int  wfa_hip_placer_duplicates_ex(wfa_hip_placer_t* placer, const wfa_hip_seqset_t* texts, int32_t min_score, int32_t full_gap,
                                  int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag,
                                  const int32_t* mate1 /* nullable */, const int32_t* mate2 /* nullable */,
                                  int32_t* read_rows /* nreads x 4 */, int32_t* pair_rows /* nfrag x 4, nullable when nfrag == 0 */,
                                  int flags, const wfa_hip_qualset_t* quals /* NULL without WFA_HIP_DUP_BY_QUALITY */,
                                  int32_t min_quality);
#define WFA_HIP_DUP_COLS 4          /* rep, size, dup, overflow */
#define WFA_HIP_DUP_MAX_BUCKET 4096
int  wfa_hip_placer_duplicates(wfa_hip_placer_t* placer, const wfa_hip_seqset_t* texts, int32_t min_score, int32_t full_gap,
                               int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag,
                               const int32_t* mate1 /* nullable */, const int32_t* mate2 /* nullable */,
                               int32_t* read_rows /* nreads x 4 */, int32_t* pair_rows /* nfrag x 4, nullable when nfrag == 0 */);

/* Host only, needs no GPU: the rule above in plain C++ over the arrays wfa_hip_pair_host takes and text_len[ntexts]: what
 * wfa_hip_placer_add_hits + wfa_hip_placer_duplicates give.  Returns WFA_HIP_OK, or WFA_HIP_EINVAL (nothing written; msg as for
 * wfa_hip_place_host) for whatever wfa_hip_pair_host refuses (pair_rows aside); a negative ntexts or text_len; a hit whose
 * j >= ntexts; a missing pointer (text_len with ntexts > 0, read_rows with nreads > 0, pair_rows with nfrag > 0). */
int wfa_hip_duplicates_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse, const int32_t* score,
                            const int32_t* status, const int32_t* text_start, const int32_t* text_end, int32_t min_score,
                            int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag,
                            const int32_t* mate1 /* nullable */, const int32_t* mate2 /* nullable */, int64_t ntexts,
                            const int32_t* text_len, int32_t* read_rows /* nreads x 4 */, int32_t* pair_rows /* nfrag x 4 */,
                            char* msg, size_t msg_cap);
/* wfa_hip_duplicates_host plus lead and trail per hit (either nullable: 0; negative: refused; above WFA_HIP_CLIP_MAX: saturated),
 * flags, and qsum[nreads], the summed base quality of every read (required, and not negative, under WFA_HIP_DUP_BY_QUALITY; NULL
 * without it): what wfa_hip_placer_add_hits_clips + wfa_hip_placer_duplicates_ex give over a quality set with those sums.
 * wfa_hip_duplicates_host is this with NULL, NULL, 0, NULL. */
int wfa_hip_duplicates_host_ex(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                               const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end,
                               int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired,
                               int64_t nfrag, const int32_t* mate1 /* nullable */, const int32_t* mate2 /* nullable */, int64_t ntexts,
                               const int32_t* text_len, int32_t* read_rows /* nreads x 4 */, int32_t* pair_rows /* nfrag x 4 */,
                               const int32_t* lead /* nullable */, const int32_t* trail /* nullable */, int flags,
                               const int32_t* qsum /* nreads, NULL without the quality flag */, char* msg, size_t msg_cap);
/* Host only: qsum of one read, the sum of quals[k] >= min_quality over its len bytes, 64-bit, saturated to INT32_MAX.  WFA_HIP_EINVAL
 * for a NULL output, a negative len, NULL quals with len > 0 or min_quality outside 0 .. WFA_HIP_MAX_QUALITY. */
int wfa_hip_qsum_host(const uint8_t* quals, int64_t len, int32_t min_quality, int32_t* out);

/* ---- seed finder: an exact-match k-mer index over a text set, candidate windows for every read ------------ */

/*
 * The first stage of read mapping on resident sets: from `texts` (references) an index of their k-mers, built on the device; from
 * `patterns` (reads) the best candidate windows of every read on both strands, in the shape wfa_hip_batch_create_windows and
 * wfa_hip_pileup_add take (i = the read, j, t_start = text_start, t_len = text_len, reverse).
 *
 * Valid k-mers.  The k-mer at position p of a sequence is valid when p + k <= len and none of its k letters is outside ACGT (the
 * letters wfa_hip_seqset_create flags; a set is upper-cased by nothing in this ABI: lower case is outside ACGT).  Matching is exact, on
 * the 2-bit codes; the aligner's wildcard plays no part.
 * Index (k in 8 .. 15, stride >= 1, max_occ >= 1).  Position (j, t) is indexed when t % stride == 0 and the k-mer at t of texts[j] is
 * valid.  occ(x) is the number of indexed positions of k-mer x over the whole set; a k-mer with occ(x) > max_occ yields no hits (the
 * repeat mask).
 * Hits of read i (length L).  R_0 is the read, R_1 its reverse complement.  Every valid k-mer of R_s at position r, for every indexed
 * position (j, t) of the same k-mer, is one hit (s, j, d = t - r).  H is the number of hits over both strands; H > max_hits: the read
 * gets overflow = 1 and no seeds.  A read shorter than k has no hits.
 * Clusters.  The read's hits sorted by (s, j, d); a cluster is a maximal run of consecutive hits of one (s, j) whose neighbouring d
 * differ by at most `gap`, with hits = its size c, d_lo and d_hi.  (A definition on the sorted multiset: no bucket or thread order
 * enters.)  The clusters with c >= min_hits, ranked by c descending, then s, j, d_lo ascending; the first n are the read's seeds.
 * Window of a cluster.  text_start = max(0, d_lo - pad), text_end = min(len(texts[j]), d_hi + L + pad), text_len = text_end -
 * text_start (always positive).
 * Result.  Five M x n int32 row-major arrays j, reverse, text_start, text_len, hits, rows padded with j = -1 and zeros elsewhere (as
 * wfa_hip_cross_topk pads), and overflow, M bytes.
 *
 * wfa_hip_seed_index_create builds the index in HBM (csrc/wfa_seed.hpp, k_seed.hip: a direct-addressed counting sort): A TABLE OF
 * 4^k * 4 BYTES (k = 13: 256 MiB; k = 15: 4 GiB) PLUS 8 BYTES PER INDEXED POSITION; a failed allocation: NULL, WFA_HIP_EDEVICE, the
 * message names the byte count.  The index copies what it needs of the set (lengths; the query reads no text base) and stays valid
 * after the set is destroyed.  WFA_HIP_EINVAL (NULL, wfa_hip_last_error names the parameter and its value; nothing is launched): k,
 * stride or max_occ out of range, a set of another aligner, an empty set (no sequence), a set of 2^31 bases or more.
 * wfa_hip_seed_index_query: synchronous, writes the host arrays above for the M sequences of `patterns` (n in 1 ..
 * WFA_HIP_SEED_MAX_N, min_hits >= 1, gap >= 0, pad >= 0, max_hits in 1 .. WFA_HIP_SEED_MAX_HITS).  One kernel, a workgroup per read;
 * the reads' words are read in place, 20 n + 1 bytes per read come back.  WFA_HIP_EINVAL, nothing launched: a parameter out of range
 * (named, with its value), a set of another aligner, a missing array with M > 0.  M = 0 is fine.
 * wfa_hip_seed_index_stats (any pointer may be NULL): the indexed positions, the k-mers over max_occ, the bytes of table and
 * records, and the HIP-event milliseconds of the last build and of the last query's kernel (0 before the first query).
 */
#define WFA_HIP_SEED_MAX_N    16
#define WFA_HIP_SEED_MAX_HITS 4096
typedef struct wfa_hip_seed_index wfa_hip_seed_index_t;
wfa_hip_seed_index_t* wfa_hip_seed_index_create(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* texts, int k, int stride, int max_occ);
void wfa_hip_seed_index_destroy(wfa_hip_seed_index_t* index);
int wfa_hip_seed_index_query(wfa_hip_seed_index_t* index, const wfa_hip_seqset_t* patterns, int n, int min_hits, int gap, int pad,
                             int max_hits, int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits,
                             uint8_t* overflow);
int wfa_hip_seed_index_stats(const wfa_hip_seed_index_t* index, int64_t* positions, int64_t* masked_kmers, int64_t* table_bytes,
                             float* build_ms, float* query_ms);

/* Host only, needs no GPU: the row wfa_hip_seed_index_query writes for ONE read, by the definitions above, from the ASCII read and the
 * ASCII text set (text q = texts[t_off[q] .. + t_len[q])): j, reverse, text_start, text_len, hits receive n values each, *overflow one
 * byte.  Returns WFA_HIP_OK, or WFA_HIP_EINVAL for a parameter out of range (msg, when not NULL, receives up to msg_cap bytes naming
 * the parameter and its value, exactly as the device entries' wfa_hip_last_error), a negative length or a missing array. */
int wfa_hip_seeds_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                       const int32_t* t_len, int k, int stride, int max_occ, int n, int min_hits, int gap, int pad, int max_hits,
                       int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits, uint8_t* overflow,
                       char* msg, size_t msg_cap);

/* ---- chains: co-linear chaining of a read's anchors on the seed index, candidate windows for long reads --- */

/*
 * A second query on the same index, for reads whose hits neither fit the seed query's max_hits nor stay within `gap` of one diagonal:
 * the read's anchors are chained along the read, and the best chains become windows.  Integers only, and a definition on a sorted
 * multiset: no bucket order or thread order enters.  The index semantics (valid k-mers, stride, max_occ, R_0 the read and R_1 its
 * reverse complement) are exactly those of the seed finder above.
 *
 * Anchors of read i (length L).  Every valid k-mer of R_s at position r, for every indexed position (j, t) of the same k-mer with
 * occ <= max_occ, is one anchor (s, r, j, t) with diagonal d = t - r.  N is the number of anchors over both strands; N > max_anchors:
 * the read gets overflow = 1 and a padded row.
 * Order.  The anchors sorted by (s, r, j, t): the order in which a scan along the read meets them, made canonical inside a bucket.
 * Chaining.  In that order; an anchor starts with f = k, cnt = 1, d_lo = d_hi = d, r_first = r.  The candidate predecessors of anchor a
 * are the up to `lookback` anchors immediately before a in the order.  Candidate b is eligible when it has the same s and j as a,
 * dr = r_a - r_b > 0 and dt = t_a - t_b > 0, dr <= max_dist and dt <= max_dist, and g = |dt - dr| <= band.  Its value is
 * f(b) + min(dr, dt, k) - cost(g), with cost(0) = 0 and cost(g) = ((g * k) >> 6) + (floor(log2 g) >> 1) for g >= 1.  Anchor a adopts
 * the eligible candidate of largest value, on a tie the nearest one (the largest index), but only when that value is strictly greater
 * than k; it then takes f = that value, cnt = cnt(b) + 1, d_lo = min(d_lo(b), d), d_hi = max(d_hi(b), d), r_first = r_first(b).
 * Selection.  n rounds.  Of the anchors with cnt >= min_hits and f >= min_score that are not yet covered, the one of largest f, on a tie
 * the smallest index in the order, is taken; its window is text_start = max(0, d_lo - pad), text_end = min(len(texts[j]), d_hi + L +
 * pad) (the shape of a seed cluster's window); every anchor of the same (s, j) with text_start <= t and t + k <= text_end becomes
 * covered (the chosen anchor always does).  The rounds stop when no anchor qualifies.
 * Result.  Eight M x n int32 row-major arrays: j, reverse (= s), text_start, text_len, hits (= cnt), score (= f), and pattern_start,
 * pattern_len: the chain's span [r_first, r_a + k) of R_s in the coordinates of the stored read, as wfa_hip_batch_create_windows takes
 * them (s = 0: pattern_start = r_first; s = 1: pattern_start = L - (r_a + k)).  Rows padded with j = -1 and zeros elsewhere, and
 * overflow, M bytes.
 * Ranges (outside: WFA_HIP_EINVAL, the parameter named with its value, nothing launched): n in 1 .. WFA_HIP_SEED_MAX_N, min_hits >= 1,
 * min_score >= 0, lookback in 1 .. WFA_HIP_CHAIN_MAX_LOOKBACK, max_dist in 1 .. 2^20, band in 0 .. 2^16, pad >= 0, max_anchors in 1 ..
 * WFA_HIP_CHAIN_MAX_ANCHORS.  Within them every value above fits 32 bits.
 *
 * wfa_hip_seed_index_chain: synchronous, writes the host arrays above for the M sequences of `patterns`; also refused: a set of another
 * aligner, a missing array with M > 0.  M = 0 is fine.  One kernel, a workgroup per read (csrc/wfa_chain.hpp, k_chain.hip); the anchors
 * and their chain state live in a workspace in HBM of 32 BYTES x max_anchors PER RESIDENT WORKGROUP, its own allocation, kept on the
 * index and grown on demand (freed with the index); a failed allocation: WFA_HIP_EDEVICE, the message names the byte count.
 * wfa_hip_seed_index_chain_stats (either pointer may be NULL): the HIP-event milliseconds of the last chain kernel (0 before the first)
 * and the bytes of the workspace now held.
 */
#define WFA_HIP_CHAIN_MAX_LOOKBACK 64
#define WFA_HIP_CHAIN_MAX_ANCHORS  65536
int wfa_hip_seed_index_chain(wfa_hip_seed_index_t* index, const wfa_hip_seqset_t* patterns, int n, int min_hits, int min_score, int lookback,
                             int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse, int32_t* text_start,
                             int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start, int32_t* pattern_len,
                             uint8_t* overflow);
int wfa_hip_seed_index_chain_stats(const wfa_hip_seed_index_t* index, float* kernel_ms, int64_t* workspace_bytes);

/* Host only, needs no GPU: the row wfa_hip_seed_index_chain writes for ONE read, by the definitions above, from the ASCII read and the
 * ASCII text set (as wfa_hip_seeds_host takes them): the eight arrays receive n values each, *overflow one byte.  Returns WFA_HIP_OK,
 * or WFA_HIP_EINVAL with the device entry's message for a parameter out of range, a negative length or a missing array. */
int wfa_hip_chains_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                        const int32_t* t_len, int k, int stride, int max_occ, int n, int min_hits, int min_score, int lookback,
                        int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse, int32_t* text_start,
                        int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start, int32_t* pattern_len,
                        uint8_t* overflow, char* msg, size_t msg_cap);

/* ---- minimizers: (w,k) sampling of the seed index, for seeds and chains alike ----------------------------- */

/*
 * A second way of thinning the index, beside `stride`: the text and the read are sampled by the same content-defined rule, so the read
 * looks up only its own minimizers, the index holds about 2 / (w + 1) of the valid positions, and any exact match of at least
 * w + k - 1 bases shares a sampled position on both sides.  Valid k-mers, the 2-bit codes, occ, max_occ, R_0 and R_1 are those of the
 * seed finder above.
 *
 * Key of a position.  For a sequence of length len, key(p) = +inf when p < 0 or p + k > len, or when the k-mer at p is not valid.
 * Otherwise key(p) = mix32(min(code, rc(code))): code the 2-bit code of the k-mer at p (base p + i in bits 2 i .. 2 i + 1), rc(code) the
 * code of its reverse complement, and, on uint32_t,
 *     mix32(h):  h ^= h >> 16;  h *= 0x85ebca6b;  h ^= h >> 13;  h *= 0xc2b2ae35;  h ^= h >> 16.
 * mix32 is a bijection: two positions tie only when their canonical k-mers are equal.
 * Selection.  p is a minimizer iff key(p) is finite and the maximal run of positions around p whose keys are >= key(p) (+inf counts as
 * >=) is at least w long.  In counts: l = the number of consecutive positions p - 1, p - 2, ... with key >= key(p), r likewise for
 * p + 1, p + 2, ..., each capped at w - 1; p is selected iff l + r + 1 >= w.  So every position that is a minimum of some window of w
 * consecutive k-mer starts is selected, and every tie with it; windows that hang over a sequence end or over a letter outside ACGT
 * count too (a short sequence still has minimizers); w = 1 selects every valid k-mer; and the rule is its own mirror image: the
 * minimizers of the reverse complement are the mirrored positions len - k - p.
 * Index (k in 8 .. 15, w in 1 .. WFA_HIP_MINIMIZER_MAX_W, max_occ >= 1).  Position (j, t) is indexed iff t is a minimizer of texts[j];
 * it goes into the bucket of its forward code.  occ and the repeat mask are as above, counted over the indexed positions.
 * Hits and anchors of a read.  As in the two sections above, but only from the read positions r of R_s that are minimizers of R_s.
 * Everything behind that (sorting, clusters, chaining, selection, windows, overflow) is unchanged, for the seeds and for the chains.
 *
 * wfa_hip_seed_index_create_minimizer: as wfa_hip_seed_index_create, with w in place of stride (w out of range: NULL, WFA_HIP_EINVAL, w
 * named with its value, nothing launched); the records take 8 BYTES PER INDEXED POSITION, allocated after the counting pass.  The
 * index remembers w: wfa_hip_seed_index_query and wfa_hip_seed_index_chain apply the selection to the reads of such an index, and do
 * exactly what they do for an index of wfa_hip_seed_index_create otherwise.
 * wfa_hip_seed_index_params (any pointer may be NULL): k, and stride with w = 0 for a stride index, stride = 1 with w for a minimizer
 * index.
 */
#define WFA_HIP_MINIMIZER_MAX_W 32
wfa_hip_seed_index_t* wfa_hip_seed_index_create_minimizer(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* texts, int k, int w,
                                                          int max_occ);
int wfa_hip_seed_index_params(const wfa_hip_seed_index_t* index, int* k, int* stride, int* w);

/* Host only, needs no GPU.  wfa_hip_minimizers_host: selected[p] = 1 for the minimizers of ONE ASCII sequence, 0 elsewhere (len bytes).
 * wfa_hip_seeds_host_minimizer / wfa_hip_chains_host_minimizer: the rows of wfa_hip_seeds_host / wfa_hip_chains_host for a minimizer
 * index, w in place of stride (one body each; only the predicate on text and read positions differs).  WFA_HIP_EINVAL as there, w named
 * with its value. */
int wfa_hip_minimizers_host(const uint8_t* seq, int64_t len, int k, int w, uint8_t* selected /* len bytes */, char* msg, size_t msg_cap);
int wfa_hip_seeds_host_minimizer(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                                 const int32_t* t_len, int k, int w, int max_occ, int n, int min_hits, int gap, int pad, int max_hits,
                                 int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits, uint8_t* overflow,
                                 char* msg, size_t msg_cap);
int wfa_hip_chains_host_minimizer(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                                  const int32_t* t_len, int k, int w, int max_occ, int n, int min_hits, int min_score, int lookback,
                                  int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse, int32_t* text_start,
                                  int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start, int32_t* pattern_len,
                                  uint8_t* overflow, char* msg, size_t msg_cap);

#ifdef __cplusplus
}
#endif
#endif /* WFA_HIP_H_ */
