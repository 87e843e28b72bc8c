// host_core.hpp — what the resident-set APIs (api_*.hip) need from the aligner and batch core (wfa_hip.hip), and nothing else: the two
// handles, the knobs, the error plumbing, the block pool and the batch-building steps.  Everything here is internal to libwfa_hip.so
// (hidden visibility: none of it enters the dynamic symbol table); the definitions are in wfa_hip.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <sched.h>
#include <string>
#include <map>
#include <unordered_map>
#include <vector>
#include <algorithm>
#include <thread>
#include <memory>
#include <atomic>

#include "wfa_hip.h"
#include "wfa_common.hpp"
#include "wfa_band.hpp"   // wfa::BandArgs, wfa::SlimMailbox

namespace wfa { struct WfaPieceDesc; }   // wfa_pack.hpp, which also defines kernels: the core alone includes it, and it alone creates and deletes batches

#pragma GCC visibility push(hidden)

extern thread_local std::string g_error;   // what wfa_hip_global_error() returns: one object for every unit (defined in wfa_hip.hip)

// Development knobs, read from the environment ONCE per aligner in wfa_hip_create: the hot entry points
// never call getenv.
#define WFA_COUNTER_WORDS 256  // counters of a batch (wfa_hip_batch::d_counters)
#define WFA_KNOBS(F)                                                                                              \
  F(ARENA_KB) F(BAND_DEBUG) F(BAND_SLIM) F(BAND_LDS_MAX) F(BAND_NO_WIN) F(BAND_SPLIT_MIN) F(NO_TINY_INLINE) F(BILEVEL) F(BILEVEL_WIDE_LEVELS) F(BILEVEL_PER_CU) F(BILEVEL_I32) F(BILEVEL_QCAP) F(BILEVEL_LEVELS) F(BILEVEL_LDS) F(BILEVEL_NO_1024) F(BILEVEL_HUGE_MIN) F(BILEVEL_LDS_W) F(BILEVEL_NO_SEQL) F(LANE_DYN) F(LANE_DYN_WAVES) F(BAND_LEFTOVER_WAVES_PER_CU) F(BAND_NCH) F(BAND_NO_LDS) F(BAND_NO_SPLIT) F(BAND_PB) F(PIPE_TAIL) F(LEN16) F(MAILBOX) F(MAILBOX_IDLE_US) F(TILE32)     \
  F(BAND_RECORDS) F(BAND_SPLIT_ROUNDS) F(BAND_WAVES_PER_CU) F(NO_BAND) F(NO_FAST) F(NO_SEGFULL) F(SEGFULL_PAIRS)     \
  F(SEGFULL_STAGES) F(STAGE_TIMING) F(LANE_HEUR32) F(THREADS) F(TINY_BATCH) F(WAVES_PER_CU) F(FAST_WAVES_PER_CU) F(TIMING)          \
  F(LANE_FULL) F(LANE_FULL_SPLIT) F(LANE_HEUR) F(SEG_HEUR) F(LANE_LDS_PAD_KB) F(LANE_MIN_PAIRS) F(PIPE_CHUNK) F(PIPE_THREADS) F(PACK_THREADS) F(NO_TINY_BAND) F(NO_TINY_POLL) F(UP_STREAMS) F(NO_DUAL) F(NO_WIDE) F(WIDE_ADAPT) F(WIDE_GROWS) F(WIDE_LDS_KB) F(WIDE_THREADS) F(TILE) F(TILE_T) F(TILE_WT) F(TILE_THREADS) F(TILE_PER_CU) F(NO_PIPE) F(HOST_PACK) F(GENERAL_PB) F(LANE_WAVES_PER_CU) F(LANE_REFILL_MIN) F(LANE_WINFIN) F(LANE_DEBUG) F(NO_TINY) F(PILOT_PCT) F(WIDE_ADAPT_LDS) F(LANE_NARROW_WAVES) F(LANE_NARROW_NRP) F(PILOT_NARROW_PCT) F(CROSS_BAND) F(CROSS_TOPK_CHUNK) F(REDUCE_TIMING) F(POISON)
enum WfaKnob {
#define WFA_KNOB_ENUM(n) K_##n,
  WFA_KNOBS(WFA_KNOB_ENUM)
#undef WFA_KNOB_ENUM
  K_COUNT
};
struct WfaKnobs {
  int value[K_COUNT];
  bool set[K_COUNT];
  std::string fast_stages;  // WFA_HIP_FAST_STAGES (digits)
  void load() {
    static const char* const names[K_COUNT] = {
#define WFA_KNOB_NAME(n) "WFA_HIP_" #n,
        WFA_KNOBS(WFA_KNOB_NAME)
#undef WFA_KNOB_NAME
    };
    for (int i = 0; i < K_COUNT; ++i) {
      const char* v = getenv(names[i]);
      set[i] = v && *v;
      value[i] = set[i] ? atoi(v) : 0;
    }
    const char* fs = getenv("WFA_HIP_FAST_STAGES");
    fast_stages = (fs && *fs) ? fs : "";
  }
};

struct wfa_hip_aligner {
  int numa_state = 0;     // 0 not looked up, 1 the device's node and its CPUs are known (`numa_cpus`), 2 no binding ever (no NUMA information, one node, too few CPUs, WFA_HIP_NUMA=0)
  int numa_node = -1;     // NUMA node of the device's PCIe slot
  cpu_set_t numa_cpus;    // that node's CPUs, as far as this process may run on them
  int numa_mode = 0;      // WFA_HIP_NUMA: 0 never bind, 1 always bind the spawned upload workers to the device's node, 2 only when the caller's input lives there
  cpu_set_t proc_cpus;    // the process's affinity mask when the aligner was created (before anything here bound a thread)
  bool proc_cpus_valid = false;
  int last_src_node = -1, last_bound = 0;   // the last pipelined upload: node of the caller's pages (-1 unknown), workers bound or not
  int host_share = 1;     // aligners / processes feeding GPUs from this host (thread plan of the upload pipeline)
  std::string rtc_note;   // why the run-time kernels were switched off (wfa_hip_batch_run), empty otherwise
  int device = 0;
  wfa_hip_config_t cfg;
  WfaDevConfig dcfg;
  int ncomp = 3;
  WfaDevConfig gcfg;      // what the general kernel runs (= dcfg unless dcfg.lin)
  int gncomp = 3;
  WfaKnobs knobs;
  hipStream_t stream = nullptr;
  std::vector<uint8_t> pair_blob;   // wfa_hip_align_pair: the two sequences of the call, back to back
  // lifetime: batches keep a pointer to their aligner; wfa_hip_destroy with batches still alive only marks the handle,
  // the last batch to go frees it
  int live_batches = 0;
  bool destroy_pending = false;
  // the workspace below is shared by every run of this aligner: a run enqueued on another stream than the previous
  // one first waits for ws_event (recorded after each run), so runs are stream-ordered whatever streams callers pass
  hipEvent_t ws_event = nullptr;
  hipStream_t ws_last_stream = nullptr;
  // the walks of a split stage's launch run on this stream, under the alignment kernel of the next launch (which writes
  // the other half of the workspace); created on first use
  hipStream_t side_stream = nullptr;
  // round 6: what ONE launch of a split stage hands on is aligned by the stages behind it on this stream, beside the split stage's
  // next launch (batch_run_once: "pipelined tail"); created on first use
  hipStream_t tail_stream = nullptr;
  hipEvent_t tail_fork[2] = {nullptr, nullptr}, tail_join = nullptr;
  hipEvent_t band_event[4] = {nullptr, nullptr, nullptr, nullptr}, walk_event[4] = {nullptr, nullptr, nullptr, nullptr};   // [0..1] the band stages' walks, [2..3] the lane-full stage's expands
  // second upload stream of the host-packed upload (every other slot's DMAs: two copy engines)
  hipStream_t up_stream = nullptr;
  hipEvent_t up_fork = nullptr, up_join = nullptr;
  bool ws_event_recorded = false;
  // pinned staging ring of the pipelined upload (batches of >= 256 k pairs): host threads copy pieces of the caller's
  // pageable arrays into the slots, each slot goes to the device by DMA as soon as it is full
  std::vector<uint8_t*> pin_slot;
  std::vector<hipEvent_t> pin_ev;
  std::vector<char> pin_ev_recorded;   // the slot's event was recorded: its DMA must be over before the slot is refilled
  // single calls of a pywfa-style loop (a handful of pairs): one pinned, device-visible staging block + its device copy,
  // allocated once; the call is then host writes -> copy kernel -> alignment kernel -> one stream sync -> host reads
  uint8_t* tiny_h = nullptr;
  uint8_t* tiny_hd = nullptr;
  uint8_t* tiny_d = nullptr;
  // the resident one-pair kernel (round 6; wfa_slim.hpp: wfa_slim_kernel_mailbox): its mailbox in pinned host memory, the stream its
  // instances run on, the arguments the running instance was started with (another configuration / workspace: it is told to leave first)
  wfa::SlimMailbox* mb_h = nullptr;
  wfa::SlimMailbox* mb_d = nullptr;
  hipStream_t mb_stream = nullptr;
  wfa::BandArgs mb_args;
  bool mb_args_valid = false;
  uint32_t mb_seq = 0;
  int mb_failures = 0;
  size_t pin_slot_bytes = 0;
  int cu_count = 256;
  size_t total_mem = 0;
  std::string err;
  // persistent workspace for the general kernel (grown on demand)
  int32_t* ws = nullptr;
  size_t ws_bytes = 0;
  // device blocks of finished batches kept for the next one (a batch takes ~20 arrays; for the small batches of
  // a pywfa-style loop of single alignments hipMalloc / hipFree are most of the call)
  std::multimap<size_t, void*> pool_free;
  std::unordered_map<void*, size_t> pool_size;
  size_t pool_cached = 0;
};

static inline int knob(const wfa_hip_aligner* al, WfaKnob k, int dflt) {
  return al->knobs.set[k] ? al->knobs.value[k] : dflt;
}

// WFA_HIP_POISON=1..255 (a development knob for the tests; synchronises): device memory that is handed out without its contents being
// defined — a block of the pool (fresh or recycled, over its whole size class), a direct allocation, the aligner's workspace at the start
// of a run — is filled with that byte first, so that a kernel reading a byte nothing wrote sees 0x7f7f.. or 0xffff.. and not the zero page
// of a fresh allocation or the previous batch's data.  The fill goes to `stream` and the call waits for that stream alone (never the
// device: the resident one-pair kernel may be running on its own stream).  A batch run has told that kernel to leave before its fill
// (mailbox_release); the single-call path (tiny_band) has NOT: the instance is idle between calls, its history is written per pair
// before its walk reads it, and it leaves by itself after its idle time.  A workspace that has just grown is filled twice on that path
// (ensure_ws, then wait_for_workspace): harmless.  Off (unset or 0): one array read.
static inline hipError_t poison_fill(const wfa_hip_aligner* al, void* p, size_t bytes, hipStream_t stream) {
  const int v = al->knobs.value[K_POISON];
  if (v < 1 || v > 255 || !p || bytes == 0) return hipSuccess;
  const hipError_t e = hipMemsetAsync(p, v, bytes, stream);
  return e != hipSuccess ? e : hipStreamSynchronize(stream);
}

struct wfa_hip_batch {
  wfa_hip_aligner* al = nullptr;
  // configuration in force when the batch was created: the layout of the batch (op regions, 8-bit work list, checked
  // free ends) follows it, so run / sync / results use this snapshot, never the aligner's current configuration
  wfa_hip_config_t cfg;
  WfaDevConfig dcfg;
  WfaDevConfig gcfg;       // the general kernel's configuration (= dcfg unless dcfg.lin: the original one-component distance)
  int gncomp = 3;
  int wild = -1;           // the wildcard letter of the 8-bit pairs when dcfg.wildcard was cleared for the 2-bit ones (round 5, below)
  int ncomp = 3;
  int64_t n = 0;
  // host copies needed later
  std::vector<int32_t> h_plen, h_tlen;
  std::vector<int64_t> h_coff;
  std::unique_ptr<WfaPairMeta[]> h_meta;  // kept until the batch dies: its upload may still be in flight when batch_build returns
  std::vector<wfa::WfaPieceDesc> h_pieces;   // host-packed upload with 16-bit lengths: the pieces' first pair / first word (uploaded; kept like h_meta)
  uint32_t* d_len16 = nullptr;               // ... the {plen, tlen} halves as uploaded, and the piece table on the device
  wfa::WfaPieceDesc* d_pieces = nullptr;
  int max_width = 0;       // max(plen+tlen)+3
  int max_len = 0;         // max(plen, tlen)
  int64_t packed_bytes = 0;  // sum of ceil(len/4) over all sequences (algorithmic 2-bit bytes)
  int64_t ops_bytes = 0;     // sum(plen+tlen)
  // device
  uint8_t* d_bytes = nullptr;
  int64_t* d_pboff = nullptr;
  int64_t* d_tboff = nullptr;
  WfaPairMeta* d_meta = nullptr;
  uint32_t* d_words = nullptr;
  uint8_t* d_flags = nullptr;
  int32_t* d_score = nullptr;
  int32_t* d_status = nullptr;
  uint8_t* d_ops = nullptr;
  int64_t* d_cigar_off = nullptr;
  int64_t* d_cigar_begin = nullptr;
  int32_t* d_cigar_len = nullptr;
  uint32_t* d_list_packed = nullptr;  // worklists (nullptr = identity over all pairs)
  uint32_t* d_list_bytes = nullptr;
  uint32_t n_packed = 0, n_bytes = 0;
  uint32_t* d_fb_list2[2] = {nullptr, nullptr};  // leftover lists handed from one kernel stage to the next (ping-pong)
  const uint32_t* leftover_count = nullptr;       // device count of the pairs that reached the general kernel
  uint32_t* d_ovf_list[2] = {nullptr, nullptr};  // pairs whose arena overflowed
  uint32_t* d_counters = nullptr;  // [0] fallback count, [1] overflow count A, [2] overflow count B, [4..5] the pilots, [8..15] lane-full list / debug, [16..] one hand-over count per stage of a run
  std::vector<hipEvent_t> ev;   // 2 events per run since the last sync (kernel timing)
  size_t ev_used = 0;
  int runs_pending = 0;
  double ms_sum = 0.0; int ms_runs = 0;
  bool ran = false, synced = true;
  float last_ms = 0.f;
  int64_t last_kernel_pairs = 0;
  int64_t last_fallback = 0;
  hipStream_t last_stream = nullptr;
  bool uploads_pending = false;
  // recorded on the aligner's stream after the last upload / memset / pack kernel of batch_build: a run on another stream
  // waits for it (the host-packed upload returns with its DMAs still in flight)
  hipEvent_t upload_event = nullptr;
  int stage_pick = 0;  // first register-kernel stage chosen by the pilot of the first run (0 = not yet): 16, 32 or 64 lanes
  int narrow_pick = 0; // stage_pick 16, score only: the 8-diagonal lane stage in front of the 16-diagonal one (1) or not (2), 0 undecided
  int narrow_nrp = 0;  // ... narrow_pick 1: its width in packed registers, 4, 5 or 6 (8, 10 or 12 diagonals: wfa_lane.hpp NRP), chosen by the pilot's cost model
  int narrow_permille = -1;   // ... and the share of its pilot's sample it handed on (-1: no pilot), which sizes the slices of the stage behind it
  int segh_pick = 0;   // the same for the general form of the 32-lane segments (wfa_seg_kernel<.., HEUR>)
  int band_pick = 0;   // exact reads of 300 - 1 200 bases: the 256-diagonal register window first (1) or not (2: its pilot handed on most pairs), 0 undecided
  int laneh_pick = 0;  // general score-only form of the lane kernel first (wf-adaptive / free ends / step limit): 1 yes, 2 no (its pilot), 0 undecided
  int64_t arena_ints = 0;  // FULL: arena size used by the last launch (the part that grows 8x when a pair overflows it)
  int64_t arena_fixed = 0; // FULL, piggy-back history of the general kernel: the score-only ring in front of the growing part
  // device-side result surface (RLE)
  int32_t* d_plen = nullptr; int32_t* d_tlen = nullptr; int32_t* d_run_count = nullptr; int32_t* d_locs = nullptr;
  int64_t* d_run_off = nullptr; int64_t rle_total = -1;
  // SAM fields (api_sam.hip): the rows of wfa_hip_batch_sam_counts and the two scans of their length columns stay here for
  // wfa_hip_batch_sam_strings; they hold for the run and the op strings they were made from (run_serial; a left alignment drops them)
  int64_t run_serial = 0;      // counts the runs of the batch
  int32_t* d_sam_rows = nullptr; uint64_t* d_sam_off = nullptr;   // n x 8; two arrays of n + 1
  int64_t sam_serial = -1;     // the run the rows belong to, -1: none
  int sam_flags = 0;
  int64_t sam_bytes[2] = {0, 0};   // the CIGAR and MD bytes of all pairs
  float sam_ms[2] = {0.f, 0.f};    // HIP-event times of the two passes
};

#define HIP_TRY(al, expr)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      char buf_[512];                                                                          \
      snprintf(buf_, sizeof(buf_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      if (al) (al)->err = buf_;                                                                \
      g_error = buf_;                                                                          \
      return WFA_HIP_EDEVICE;                                                                  \
    }                                                                                          \
  } while (0)

// ---- refusals: one message buffer (HIP_TRY's 512 bytes), one place per error channel -------------------------------------------------
#define WFA_FORMAT_ERR(buf, fmt) char buf[512]; do { va_list ap_; va_start(ap_, fmt); vsnprintf(buf, sizeof(buf), fmt, ap_); va_end(ap_); } while (0)
// an int entry refuses its arguments: al->err alone
__attribute__((format(printf, 2, 3))) static inline int fail_inval(wfa_hip_aligner* al, const char* fmt, ...) {
  WFA_FORMAT_ERR(buf, fmt);
  al->err = buf;
  return WFA_HIP_EINVAL;
}
// a creator refuses: g_error, and al->err where there is an aligner; converts to the null handle of any type
__attribute__((format(printf, 2, 3))) static inline decltype(nullptr) fail_create(wfa_hip_aligner* al, const char* fmt, ...) {
  WFA_FORMAT_ERR(buf, fmt);
  if (al) al->err = buf;
  g_error = buf;
  return nullptr;
}
// one of the checks shared with the *_host entries (host_place.cpp and its kin: their last two parameters are (msg, cap)), its refusal in al->err
template <class Check, class... A> static int check_inval(wfa_hip_aligner* al, Check check, A... args) {
  char buf[512];
  if (check(args..., buf, sizeof(buf)) == WFA_HIP_OK) return WFA_HIP_OK;
  al->err = buf;
  return WFA_HIP_EINVAL;
}
// a failed allocation of *p: HIP's error cleared, the pointer nulled, the message (bytes and what they were for) in al->err
__attribute__((format(printf, 3, 4))) static inline int fail_alloc(wfa_hip_aligner* al, void** p, const char* fmt, ...) {
  (void)hipGetLastError();
  *p = nullptr;
  WFA_FORMAT_ERR(buf, fmt);
  al->err = buf;
  return WFA_HIP_EDEVICE;
}
// "a finished batch of this aligner", as the entries that reduce a batch's results ask for it; `what`: the entry's prefix
static inline int batch_of(wfa_hip_aligner* al, const wfa_hip_batch* b, const char* what, bool need_full) {
  if (!b) return fail_inval(al, "%s: null batch", what);
  if (b->al != al) return fail_inval(al, "%s: batch of another aligner", what);
  if (need_full && b->cfg.scope != WFA_SCOPE_FULL) return fail_inval(al, "%s needs scope=full", what);
  if (!b->ran) return fail_inval(al, "%s needs a finished run of the batch", what);
  return WFA_HIP_OK;
}

// ---- wfa_hip.hip: the aligner's pool, lifetime and configuration ------------------------------------------------------------------
hipError_t pool_alloc(wfa_hip_aligner* al, void** p, size_t bytes);
void pool_release(wfa_hip_aligner* al, void* p);
void aligner_free(wfa_hip_aligner* al);
wfa_hip_batch* batch_new(wfa_hip_aligner* al);
void batch_free(wfa_hip_batch* b);
void mailbox_release(wfa_hip_aligner* al);
int64_t free_budget(wfa_hip_aligner* al);
void derive_dev_config(const wfa_hip_config_t& c, WfaDevConfig* d, int* ncomp, WfaDevConfig* gd = nullptr, int* gncomp = nullptr);
bool wildcard_in_acgt(int wc);

// ---- wfa_hip.hip: the steps every batch builder shares ------------------------------------------------------------------------------
int run_pilots(wfa_hip_aligner* al, wfa_hip_batch* b);
int batch_alloc_common(wfa_hip_aligner* al, wfa_hip_batch* b, uint64_t total_words, int zero_tail);
void batch_adopt_config(wfa_hip_aligner* al, wfa_hip_batch* b);
int upload_work_lists(wfa_hip_aligner* al, wfa_hip_batch* b, const std::vector<uint32_t>& lp, const std::vector<uint32_t>& lb, bool async);
int finish_batch_build(wfa_hip_aligner* al, wfa_hip_batch* b);

// parts 0 .. nparts - 1 of a pass over a batch on at most `team` host threads, the caller's among them (the parts are claimed from a counter)
template <class Fn> static void run_parts(int nparts, int team, Fn&& fn) {
  if (nparts == 1) { fn(0); return; }
  std::atomic<int> nextp(0);
  auto loop = [&]() { for (int t = nextp.fetch_add(1); t < nparts; t = nextp.fetch_add(1)) fn(t); };
  std::vector<std::thread> th;
  for (int t = 1; t < std::min(team, nparts); ++t) th.emplace_back(loop);
  loop();
  for (auto& x : th) x.join();
}

// why a part of a batch was refused (PART_OVER_LIGHT is no refusal: scan_lengths leaves the host-packed form on it)
enum PartError { PART_OK = 0, PART_NEGATIVE = 1, PART_TOO_LONG = 2, PART_ENDS_FREE = 3, PART_OVER_LIGHT = 4 };
const char* part_error_message(int err);
// wavefront_align.c:86-102: the reference exit(1)s here
static inline bool free_ends_exceed(const wfa_hip_config_t& c, int pl, int tl) {
  return c.span == WFA_SPAN_ENDSFREE && (c.pattern_begin_free > pl || c.pattern_end_free > pl || c.text_begin_free > tl || c.text_end_free > tl);
}

// WFA_HIP_REDUCE_TIMING=1 (a development knob): the summary, pileup, calls, sites and placement kernels are bracketed by two events and their
// HIP-event time goes to stderr, one line per call (tools/probes/pileup_index.py and pileup_calls.py read it).
struct ReduceTimer {
  wfa_hip_aligner* al; const char* what; int64_t n;
  hipEvent_t ev[2] = {nullptr, nullptr};
  const char* unit;
  ReduceTimer(wfa_hip_aligner* al_, const char* what_, int64_t n_, const char* unit_ = "pairs") : al(al_), what(what_), n(n_), unit(unit_) {
    if (knob(al, K_REDUCE_TIMING, 0) && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) (void)hipEventRecord(ev[0], al->stream);
  }
  void stop() { if (ev[1]) (void)hipEventRecord(ev[1], al->stream); }
  ~ReduceTimer() {   // (after the caller's stream synchronisation)
    float ms = 0.f;
    if (ev[1] && hipEventSynchronize(ev[1]) == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
      fprintf(stderr, "[wfa_hip] %s kernel %.4f ms (%lld %s)\n", what, ms, (long long)n, unit);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};

// The end of a launch whose results (or whose caller's arrays) the stream still holds: the timer stopped, the stream synchronised, then
// the two outcomes in this order: a failed launch's message, else the synchronisation's error.
static inline int launch_end(wfa_hip_aligner* al, ReduceTimer* timer, int launch_rc, const char* failed) {
  if (timer) timer->stop();
  const hipError_t e = hipStreamSynchronize(al->stream);
  if (launch_rc != 0) { al->err = failed; return WFA_HIP_EDEVICE; }
  HIP_TRY(al, e);
  return WFA_HIP_OK;
}

#pragma GCC visibility pop
