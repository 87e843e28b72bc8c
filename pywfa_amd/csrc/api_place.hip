// api_place.hip — the placer of libwfa_hip.so (the C ABI declared in include/wfa_hip.h).
#include "host_sets.hpp"
#include "wfa_place.hpp"
#include "wfa_dup.hpp"

// ------------------------------------------------------------------------------------------------
// placement: one row per read from the hits of any number of batches (include/wfa_hip.h; csrc/wfa_place.hpp, k_place.hip)
// ------------------------------------------------------------------------------------------------
static_assert(WFA_PLACE_COLS == WFA_HIP_PLACE_COLS, "columns of the kernels and of the ABI");

namespace wfa {   // host_place.cpp: the checks shared with wfa_hip_place_host
int place_check_hits(int64_t nreads, int64_t base, int64_t n, const int32_t* i, const int32_t* j, const int32_t* text_start,
                     const int32_t* text_end, char* msg, size_t cap);
int place_check_run(int32_t full_gap, char* msg, size_t cap);
// host_pair.cpp: the check shared with wfa_hip_pair_host
int pair_check(int64_t nreads, int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag, const int32_t* mate1,
               const int32_t* mate2, char* msg, size_t cap);
// host_rescue.cpp: the check shared with wfa_hip_rescue_host
int rescue_check(int32_t pad, int32_t min_len, int32_t anchor_mapq, int64_t cap, const int64_t* count, const int32_t* rows, char* msg,
                 size_t msg_cap);
// host_dup.cpp: the check shared with wfa_hip_duplicates_host
int dup_check(int64_t nreads, int64_t nfrag, const int32_t* read_rows, const int32_t* pair_rows, char* msg, size_t cap);
int dup_check_flags(int flags, bool have_quals, int32_t min_quality, char* msg, size_t cap);
int dup_check_clips(int64_t base, int64_t n, const int32_t* lead, const int32_t* trail, char* msg, size_t cap);
}
static_assert(WFA_PLACE_CLIP_MAX == WFA_HIP_CLIP_MAX, "clips: the kernels and the ABI");
static_assert(WFA_DUP_UNCLIPPED == WFA_HIP_DUP_UNCLIPPED && WFA_DUP_BY_QUALITY == WFA_HIP_DUP_BY_QUALITY, "duplicates: the flags of the kernels and of the ABI");
static_assert(WFA_RESCUE_COLS == WFA_HIP_RESCUE_COLS, "rescue: the kernels and the ABI");
static_assert(WFA_DUP_COLS == WFA_HIP_DUP_COLS && WFA_DUP_MAX_BUCKET == WFA_HIP_DUP_MAX_BUCKET, "duplicates: the kernels and the ABI");
static_assert(sizeof(wfa::DupUnit) == 32, "duplicates: a unit record is two 16-byte words");
static_assert(WFA_PAIR_COLS == WFA_HIP_PAIR_COLS && WFA_PAIR_MAX_PAIRINGS == WFA_HIP_PAIR_MAX_PAIRINGS, "pairing: the kernels and the ABI");

struct wfa_hip_placer {
  wfa_hip_aligner* al = nullptr;
  int64_t nreads = 0;
  int64_t nhits = 0, cap = 0;          // records in use, and allocated
  wfa::PlaceHit* d_hits = nullptr;     // the records, in hit-number order
  uint32_t* d_count = nullptr;         // [nreads + 1] (wfa_place.hpp: PlaceArgs::count)
  uint32_t* d_bsum = nullptr;
  uint32_t* d_order = nullptr;         // [order_cap] the grouped hit numbers
  int64_t order_cap = 0;
  int64_t grouped = -1;                // the number of hits d_count / d_order were made for (-1: none)
  // (hit number, j) of every hit whose j exceeds that of all hits before it: the last one is the greatest text index among the hits,
  // the first one with j >= n the first hit that a set of n texts does not hold (rescue checks it against its text set)
  std::vector<std::pair<int64_t, int32_t>> j_rise;
  // duplicates (wfa_dup.hpp), nothing of it before the first wfa_hip_placer_duplicates: the plane over the bases of a text set with
  // its chunk sums (grown when a larger set comes), the unit records and their bucket-ordered copy, the owner bytes
  uint32_t* d_dup_plane = nullptr;
  uint32_t* d_dup_bsum = nullptr;
  int64_t dup_bases = -1;              // the plane holds dup_bases + 1 counters (-1: none)
  wfa::DupUnit* d_dup_rec = nullptr;
  wfa::DupUnit* d_dup_sorted = nullptr;
  uint8_t* d_dup_owned = nullptr;
  int32_t* d_dup_qsum = nullptr;       // [nreads], from the first call under WFA_HIP_DUP_BY_QUALITY on
  hipEvent_t ev[2] = {nullptr, nullptr};
  float last_ms = 0.f;
};

extern "C" void wfa_hip_placer_destroy(wfa_hip_placer_t* p) {
  if (!p) return;
  wfa_hip_aligner* al = p->al;
  (void)hipSetDevice(al->device);
  (void)hipStreamSynchronize(al->stream);
  pool_release(al, p->d_hits); pool_release(al, p->d_count); pool_release(al, p->d_bsum); pool_release(al, p->d_order);
  if (p->d_dup_plane) pool_release(al, p->d_dup_plane);
  if (p->d_dup_bsum) pool_release(al, p->d_dup_bsum);
  if (p->d_dup_rec) pool_release(al, p->d_dup_rec);
  if (p->d_dup_sorted) pool_release(al, p->d_dup_sorted);
  if (p->d_dup_owned) pool_release(al, p->d_dup_owned);
  if (p->d_dup_qsum) pool_release(al, p->d_dup_qsum);
  for (hipEvent_t e : p->ev) if (e) (void)hipEventDestroy(e);
  destroy_end(p);
}

// a pool block of `count` values of T, or WFA_HIP_EDEVICE with the byte count and what they are for in the message
template <class T> static int placer_block(wfa_hip_aligner* al, T** out, size_t count, const char* what) {
  if (pool_alloc(al, (void**)out, count * sizeof(T)) == hipSuccess) return WFA_HIP_OK;
  return fail_alloc(al, (void**)out, "placement: the allocation of %zu bytes failed (%s)", count * sizeof(T), what);
}

static int placer_build(wfa_hip_aligner* al, wfa_hip_placer* p) {
  const size_t chunks = (size_t)((p->nreads + 1 + WFA_PLACE_SCAN_CHUNK - 1) / WFA_PLACE_SCAN_CHUNK);
  if (placer_block(al, &p->d_count, (size_t)(p->nreads + 1), "4 bytes per read") || placer_block(al, &p->d_bsum, chunks, "the scan's chunk sums")) return WFA_HIP_EDEVICE;
  if (hipEventCreate(&p->ev[0]) != hipSuccess || hipEventCreate(&p->ev[1]) != hipSuccess) { al->err = "placement: hipEventCreate failed"; return WFA_HIP_EDEVICE; }
  return WFA_HIP_OK;
}

extern "C" wfa_hip_placer_t* wfa_hip_placer_create(wfa_hip_aligner_t* al, int64_t nreads) {
  if (!al) return fail_create(al, "null aligner");
  if (nreads < 0 || nreads >= (int64_t)INT32_MAX) return fail_create(al, "placement: nreads = %lld is out of range (0 .. 2^31 - 2)", (long long)nreads);
  if (!create_begin(al)) return nullptr;
  wfa_hip_placer* p = create_adopt(al, new wfa_hip_placer());
  p->nreads = nreads;
  return create_done(al, p, placer_build(al, p), wfa_hip_placer_destroy);
}

extern "C" int64_t wfa_hip_placer_count(const wfa_hip_placer_t* p) { return p ? p->nhits : 0; }

extern "C" int wfa_hip_placer_clear(wfa_hip_placer_t* p) {
  if (!p) return WFA_HIP_EINVAL;
  p->nhits = 0; p->grouped = -1; p->j_rise.clear();
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_placer_kernel_ms(const wfa_hip_placer_t* p, float* ms) {
  if (!p || !ms) return WFA_HIP_EINVAL;
  *ms = p->last_ms;
  return WFA_HIP_OK;
}

// room for `more` records behind the ones in use: doubling, the records copied on the aligner's stream
static int placer_reserve(wfa_hip_placer* p, int64_t more) {
  wfa_hip_aligner* al = p->al;
  if (p->nhits + more <= p->cap) return WFA_HIP_OK;
  const int64_t want = std::max<int64_t>(p->nhits + more, std::max<int64_t>(2 * p->cap, 1024));
  wfa::PlaceHit* d_new = nullptr;
  if (placer_block(al, &d_new, (size_t)want, "32 bytes per hit")) return WFA_HIP_EDEVICE;
  if (p->nhits > 0) {
    const hipError_t e = hipMemcpyAsync(d_new, p->d_hits, (size_t)p->nhits * sizeof(wfa::PlaceHit), hipMemcpyDeviceToDevice, al->stream);
    const hipError_t e2 = hipStreamSynchronize(al->stream);
    if (e != hipSuccess || e2 != hipSuccess) { pool_release(al, d_new); HIP_TRY(al, e); HIP_TRY(al, e2); }
  }
  pool_release(al, p->d_hits);
  p->d_hits = d_new; p->cap = want;
  return WFA_HIP_OK;
}

// the rises of j among the n hits about to be appended (the caller's host array)
static void placer_note_texts(wfa_hip_placer* p, int64_t n, const int32_t* j) {
  int32_t top = p->j_rise.empty() ? -1 : p->j_rise.back().second;
  for (int64_t q = 0; q < n; ++q)
    if (j[q] > top) { top = j[q]; p->j_rise.emplace_back(p->nhits + q, top); }
}

extern "C" int wfa_hip_placer_add(wfa_hip_placer_t* p, wfa_hip_batch_t* b, const int32_t* i, const int32_t* j, const int32_t* t_start,
                                  const uint8_t* reverse) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  int rc = batch_of(al, b, "placement", false);
  if (rc != WFA_HIP_OK) return rc;
  const int64_t n = b->n;
  if (check_inval(al, wfa::place_check_hits, p->nreads, p->nhits, n, i, j, t_start, nullptr)) return WFA_HIP_EINVAL;
  rc = wfa_hip_batch_sync(b);
  if (rc != WFA_HIP_OK) return rc;
  if (n == 0) return WFA_HIP_OK;
  HIP_TRY(al, hipSetDevice(al->device));
  rc = placer_reserve(p, n);
  if (rc != WFA_HIP_OK) return rc;
  StreamScratch sc{al};   // (waits for the stream before the blocks go back)
  int32_t *d_i = nullptr, *d_j = nullptr, *d_ts = nullptr;
  uint8_t* d_rev = nullptr;
  if (sc.upload(&d_i, i, (size_t)n) || sc.upload(&d_j, j, (size_t)n) || sc.upload_opt(&d_ts, t_start, (size_t)n) || sc.upload_opt(&d_rev, reverse, (size_t)n))
    return WFA_HIP_EDEVICE;
  const bool full = b->cfg.scope == WFA_SCOPE_FULL;
  wfa::PlaceRecordArgs a;
  memset(&a, 0, sizeof(a));
  a.score = b->d_score; a.status = b->d_status; a.meta = b->d_meta;
  if (full) { a.ops = b->d_ops; a.cigar_begin = b->d_cigar_begin; a.cigar_len = b->d_cigar_len; }
  a.npairs = n; a.i = d_i; a.j = d_j; a.t_start = d_ts; a.reverse = d_rev; a.out = p->d_hits + p->nhits;
  {
    ReduceTimer timer(al, "place record", n);
    rc = launch_end(al, &timer, wfa::launch_place_record(a, full, al->cu_count, al->stream), "placement: record kernel launch failed");   // (the caller's arrays are read by the copies above)
    if (rc != WFA_HIP_OK) return rc;
  }
  placer_note_texts(p, n, j);
  p->nhits += n; p->grouped = -1;
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_placer_add_hits_clips(wfa_hip_placer_t* p, int64_t n, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                                             const int32_t* score, const int32_t* status, const int32_t* text_start,
                                             const int32_t* text_end, const int32_t* lead, const int32_t* trail) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  if (n > 0 && (!score || !status || !text_start || !text_end)) return fail_inval(al, "placement: a missing array");
  if (check_inval(al, wfa::place_check_hits, p->nreads, p->nhits, n, i, j, text_start, text_end)) return WFA_HIP_EINVAL;
  if (check_inval(al, wfa::dup_check_clips, p->nhits, n, lead, trail)) return WFA_HIP_EINVAL;
  if (n == 0) return WFA_HIP_OK;
  HIP_TRY(al, hipSetDevice(al->device));
  const int rc = placer_reserve(p, n);
  if (rc != WFA_HIP_OK) return rc;
  std::vector<wfa::PlaceHit> rec((size_t)n);
  for (int64_t q = 0; q < n; ++q) {
    wfa::PlaceHit& h = rec[(size_t)q];
    h.i = i[q]; h.j = j[q]; h.reverse = (reverse && reverse[q]) ? 1 : 0; h.status = status[q];
    h.score = score[q]; h.ts = text_start[q]; h.te = text_end[q];
    h.clips = wfa::place_clip_word(lead ? lead[q] : 0, trail ? trail[q] : 0);
  }
  HIP_TRY(al, hipMemcpyAsync(p->d_hits + p->nhits, rec.data(), (size_t)n * sizeof(wfa::PlaceHit), hipMemcpyHostToDevice, al->stream));
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  placer_note_texts(p, n, j);
  p->nhits += n; p->grouped = -1;
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_placer_add_hits(wfa_hip_placer_t* p, int64_t n, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                                       const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end) {
  return wfa_hip_placer_add_hits_clips(p, n, i, j, reverse, score, status, text_start, text_end, nullptr, nullptr);
}

// the clip words of all records, downloaded and split
extern "C" int wfa_hip_placer_read_clips(wfa_hip_placer_t* p, int32_t* lead, int32_t* trail) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  if (p->nhits > 0 && (!lead || !trail)) return fail_inval(al, "clips: a missing array (%s)", !lead ? "lead" : "trail");
  if (p->nhits == 0) return WFA_HIP_OK;
  HIP_TRY(al, hipSetDevice(al->device));
  std::vector<wfa::PlaceHit> rec((size_t)p->nhits);
  HIP_TRY(al, hipMemcpyAsync(rec.data(), p->d_hits, (size_t)p->nhits * sizeof(wfa::PlaceHit), hipMemcpyDeviceToHost, al->stream));
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  for (int64_t q = 0; q < p->nhits; ++q) {
    lead[q] = wfa::place_clip_lead(rec[(size_t)q].clips);
    trail[q] = wfa::place_clip_trail(rec[(size_t)q].clips);
  }
  return WFA_HIP_OK;
}

// ---- what the three runs (run, run_pairs, rescue) share, in the order they use it -------------------------------------------------------
// d_order holds a hit number per record
static int placer_ensure_order(wfa_hip_placer* p) {
  wfa_hip_aligner* al = p->al;
  if (p->nhits <= p->order_cap) return WFA_HIP_OK;
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  pool_release(al, p->d_order); p->d_order = nullptr; p->order_cap = 0;
  if (placer_block(al, &p->d_order, (size_t)p->cap, "4 bytes per hit")) return WFA_HIP_EDEVICE;
  p->order_cap = p->cap;
  return WFA_HIP_OK;
}

// the placement kernels' arguments; the rows, and the flags when `want_flags`, in the run's scratch
static int placer_args(wfa_hip_placer* p, StreamScratch& sc, wfa::PlaceArgs& s, int32_t min_score, int32_t full_gap, bool want_flags) {
  memset(&s, 0, sizeof(s));
  s.hits = p->d_hits; s.nhits = p->nhits; s.nreads = p->nreads; s.count = p->d_count; s.bsum = p->d_bsum; s.order = p->d_order;
  s.min_score = min_score; s.full_gap = full_gap;
  if (sc.alloc(&s.rows, (size_t)p->nreads * WFA_PLACE_COLS)) return WFA_HIP_EDEVICE;
  if (want_flags && sc.alloc(&s.flags, (size_t)p->nhits)) return WFA_HIP_EDEVICE;
  return WFA_HIP_OK;
}

// ev[0] recorded, then group (when the hits changed since the last one) and place enqueued.  `*launch_rc`: nonzero when a launch failed
// (the later ones are then left out; placer_launched handles it)
static int placer_enqueue_place(wfa_hip_placer* p, const wfa::PlaceArgs& s, int* launch_rc) {
  wfa_hip_aligner* al = p->al;
  *launch_rc = 0;
  HIP_TRY(al, hipEventRecord(p->ev[0], al->stream));
  if (p->grouped != p->nhits) {
    p->grouped = -1;
    HIP_TRY(al, hipMemsetAsync(p->d_count, 0, (size_t)(p->nreads + 1) * sizeof(uint32_t), al->stream));
    *launch_rc = wfa::launch_place_group(s, al->stream);
  }
  if (*launch_rc == 0) *launch_rc = wfa::launch_place(s, al->cu_count, al->stream);
  return WFA_HIP_OK;
}

// behind the run's last launch: ev[1] recorded and the timer stopped either way; a failed launch leaves the hits ungrouped
static int placer_launched(wfa_hip_placer* p, ReduceTimer& timer, int launch_rc, const char* failed) {
  wfa_hip_aligner* al = p->al;
  HIP_TRY(al, hipEventRecord(p->ev[1], al->stream));
  timer.stop();
  if (launch_rc != 0) { (void)hipStreamSynchronize(al->stream); p->grouped = -1; al->err = failed; return WFA_HIP_EDEVICE; }
  p->grouped = p->nhits;
  return WFA_HIP_OK;
}

// the run's downloads are enqueued: the stream synchronised, the kernels' time read
static int placer_finish(wfa_hip_placer* p) {
  HIP_TRY(p->al, hipStreamSynchronize(p->al->stream));
  HIP_TRY(p->al, hipEventElapsedTime(&p->last_ms, p->ev[0], p->ev[1]));
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_placer_run(wfa_hip_placer_t* p, int32_t min_score, int32_t full_gap, int32_t* rows, uint8_t* flags) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  if (check_inval(al, wfa::place_check_run, full_gap)) return WFA_HIP_EINVAL;
  if (p->nreads > 0 && !rows) return fail_inval(al, "placement: null rows");
  if (p->nreads == 0) return WFA_HIP_OK;
  HIP_TRY(al, hipSetDevice(al->device));
  int rc = placer_ensure_order(p);
  if (rc != WFA_HIP_OK) return rc;
  StreamScratch sc{al};
  wfa::PlaceArgs a;
  if (placer_args(p, sc, a, min_score, full_gap, flags != nullptr)) return WFA_HIP_EDEVICE;
  ReduceTimer timer(al, "place", p->nhits, "hits");
  int lrc = 0;
  if ((rc = placer_enqueue_place(p, a, &lrc)) != WFA_HIP_OK || (rc = placer_launched(p, timer, lrc, "placement: kernel launch failed")) != WFA_HIP_OK) return rc;
  if (sc.download(rows, a.rows, (size_t)p->nreads * WFA_PLACE_COLS)) return WFA_HIP_EDEVICE;
  if (flags && p->nhits > 0 && sc.download(flags, a.flags, (size_t)p->nhits)) return WFA_HIP_EDEVICE;
  return placer_finish(p);
}

// What wfa_hip_placer_run_pairs and wfa_hip_placer_rescue share, after their checks: the blocks of one pair run in `sc`, the mates
// uploaded, then group, place (placer_enqueue_place) and the pair kernel enqueued; the single-end rows and flags stay on the device for
// the join.  The caller goes on with placer_launched, as wfa_hip_placer_run does.
static int placer_enqueue_pairs(wfa_hip_placer* p, StreamScratch& sc, wfa::PairArgs& a, int32_t min_score, int32_t full_gap,
                                int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag, const int32_t* mate1,
                                const int32_t* mate2, bool want_pair_flags, int* launch_rc) {
  wfa_hip_aligner* al = p->al;
  *launch_rc = 0;
  const int rc = placer_ensure_order(p);
  if (rc != WFA_HIP_OK) return rc;
  memset(&a, 0, sizeof(a));
  wfa::PlaceArgs& s = a.place;
  if (placer_args(p, sc, s, min_score, full_gap, true)) return WFA_HIP_EDEVICE;
  a.min_insert = min_insert; a.max_insert = max_insert; a.unpaired = unpaired; a.nfrag = nfrag;
  if (want_pair_flags && sc.alloc(&a.pair_flags, (size_t)p->nhits)) return WFA_HIP_EDEVICE;
  if (nfrag > 0 && sc.alloc(&a.pair_rows, (size_t)nfrag * WFA_PAIR_COLS)) return WFA_HIP_EDEVICE;
  if (mate1 && nfrag > 0) {
    int32_t *d_m1 = nullptr, *d_m2 = nullptr;
    if (sc.upload(&d_m1, mate1, (size_t)nfrag) || sc.upload(&d_m2, mate2, (size_t)nfrag)) return WFA_HIP_EDEVICE;
    a.mate1 = d_m1; a.mate2 = d_m2;
  }
  int lrc = 0;
  { const int erc = placer_enqueue_place(p, s, &lrc); if (erc != WFA_HIP_OK) return erc; }
  // reads in no fragment, and fragments that are not proper, keep their single-end flags
  if (lrc == 0 && a.pair_flags && p->nhits > 0)
    HIP_TRY(al, hipMemcpyAsync(a.pair_flags, s.flags, (size_t)p->nhits, hipMemcpyDeviceToDevice, al->stream));
  if (lrc == 0) lrc = wfa::launch_pair(a, al->cu_count, al->stream);
  *launch_rc = lrc;
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_placer_run_pairs(wfa_hip_placer_t* p, int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert,
                                        int32_t unpaired, int64_t nfrag, const int32_t* mate1, const int32_t* mate2, int32_t* rows,
                                        uint8_t* flags, int32_t* pair_rows, uint8_t* pair_flags) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  if (check_inval(al, wfa::place_check_run, full_gap)) return WFA_HIP_EINVAL;
  if (check_inval(al, wfa::pair_check, p->nreads, min_insert, max_insert, unpaired, nfrag, mate1, mate2)) return WFA_HIP_EINVAL;
  if (nfrag > 0 && !pair_rows) return fail_inval(al, "pairing: null pair_rows");
  if (p->nreads == 0) return WFA_HIP_OK;   // (no read: no fragment, no hit)
  HIP_TRY(al, hipSetDevice(al->device));
  StreamScratch sc{al};
  wfa::PairArgs a;
  ReduceTimer timer(al, "place pairs", p->nhits, "hits");
  int lrc = 0, rc;
  if ((rc = placer_enqueue_pairs(p, sc, a, min_score, full_gap, min_insert, max_insert, unpaired, nfrag, mate1, mate2, pair_flags != nullptr, &lrc)) != WFA_HIP_OK ||
      (rc = placer_launched(p, timer, lrc, "pairing: kernel launch failed")) != WFA_HIP_OK)
    return rc;
  const wfa::PlaceArgs& s = a.place;
  if (rows && sc.download(rows, s.rows, (size_t)p->nreads * WFA_PLACE_COLS)) return WFA_HIP_EDEVICE;
  if (flags && p->nhits > 0 && sc.download(flags, s.flags, (size_t)p->nhits)) return WFA_HIP_EDEVICE;
  if (nfrag > 0 && sc.download(pair_rows, a.pair_rows, (size_t)nfrag * WFA_PAIR_COLS)) return WFA_HIP_EDEVICE;
  if (pair_flags && p->nhits > 0 && sc.download(pair_flags, a.pair_flags, (size_t)p->nhits)) return WFA_HIP_EDEVICE;
  return placer_finish(p);
}

// group, place and pair as wfa_hip_placer_run_pairs enqueues them, none of their outputs downloaded; then decide, scan and emit
// (k_rescue.hip).  4 bytes (the count) and 32 per returned window come back.
extern "C" int wfa_hip_placer_rescue(wfa_hip_placer_t* p, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts, int32_t min_score,
                                     int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag,
                                     const int32_t* mate1, const int32_t* mate2, int32_t pad, int32_t min_len, int32_t anchor_mapq,
                                     int64_t cap, int64_t* count, int32_t* rows) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  if (check_inval(al, wfa::place_check_run, full_gap)) return WFA_HIP_EINVAL;
  if (check_inval(al, wfa::pair_check, p->nreads, min_insert, max_insert, unpaired, nfrag, mate1, mate2)) return WFA_HIP_EINVAL;
  if (check_inval(al, wfa::rescue_check, pad, min_len, anchor_mapq, cap, count, rows)) return WFA_HIP_EINVAL;
  if (!patterns || !texts) return fail_inval(al, "rescue: a missing sequence set");
  if (patterns->al != al || texts->al != al) return fail_inval(al, "rescue: sequence set of another aligner");
  if (patterns->n < p->nreads)
    return fail_inval(al, "rescue: the pattern set has %lld sequences, the placer %lld reads", (long long)patterns->n, (long long)p->nreads);
  if (!p->j_rise.empty() && (int64_t)p->j_rise.back().second >= texts->n) {
    size_t k = 0;   // (the rises ascend in j: the first one outside the set is the first such hit of the list)
    while ((int64_t)p->j_rise[k].second < texts->n) ++k;
    return fail_inval(al, "rescue: text index out of range at position %lld of the hit list: j = %d over %lld texts",
                      (long long)p->j_rise[k].first, (int)p->j_rise[k].second, (long long)texts->n);
  }
  if (p->nreads == 0 || nfrag == 0) { *count = 0; return WFA_HIP_OK; }   // (no fragment: no window)
  HIP_TRY(al, hipSetDevice(al->device));
  StreamScratch sc{al};
  wfa::RescueArgs r;
  memset(&r, 0, sizeof(r));
  const int64_t nslots = 2 * nfrag, out_cap = std::min<int64_t>(cap, nslots);
  r.read_len = patterns->d_len; r.npatterns = patterns->n; r.text_len = texts->d_len; r.ntexts = texts->n;
  r.pad = pad; r.min_len = min_len; r.anchor_mapq = anchor_mapq; r.cap = out_cap;
  if (sc.alloc(&r.slot, (size_t)nslots + 1)) return WFA_HIP_EDEVICE;
  if (sc.alloc(&r.bsum, (size_t)((nslots + 1 + WFA_PLACE_SCAN_CHUNK - 1) / WFA_PLACE_SCAN_CHUNK))) return WFA_HIP_EDEVICE;
  if (out_cap > 0 && sc.alloc(&r.out, (size_t)out_cap * WFA_RESCUE_COLS)) return WFA_HIP_EDEVICE;
  ReduceTimer timer(al, "rescue", p->nhits, "hits");
  int pair_rc = 0, lrc = 0, rc;
  if ((rc = placer_enqueue_pairs(p, sc, r.pair, min_score, full_gap, min_insert, max_insert, unpaired, nfrag, mate1, mate2, false, &pair_rc)) != WFA_HIP_OK) return rc;
  if (pair_rc == 0) lrc = wfa::launch_rescue(r, al->cu_count, al->stream);
  if ((rc = placer_launched(p, timer, pair_rc, "pairing: kernel launch failed")) != WFA_HIP_OK) return rc;
  if (lrc != 0) { (void)hipStreamSynchronize(al->stream); al->err = "rescue: kernel launch failed"; return WFA_HIP_EDEVICE; }
  uint32_t n = 0;
  if (sc.download(&n, r.slot + nslots, 1) || (rc = placer_finish(p)) != WFA_HIP_OK) return WFA_HIP_EDEVICE;
  const int64_t take = std::min<int64_t>((int64_t)n, out_cap);
  if (take > 0) {
    if (sc.download(rows, r.out, (size_t)take * WFA_RESCUE_COLS)) return WFA_HIP_EDEVICE;
    HIP_TRY(al, hipStreamSynchronize(al->stream));
  }
  *count = (int64_t)n;
  return WFA_HIP_OK;
}

// ---- duplicates (include/wfa_hip.h, "duplicates"; wfa_dup.hpp, k_dup.hip) ---------------------------------------------------------------
// the blocks the placer keeps for it: the per-read ones once, the plane again when a text set has more bases than any before
static int placer_ensure_dup(wfa_hip_placer* p, int64_t nbases) {
  wfa_hip_aligner* al = p->al;
  const size_t nreads = (size_t)p->nreads;
  if (!p->d_dup_rec && placer_block(al, &p->d_dup_rec, nreads, "32 bytes per read, the unit records")) return WFA_HIP_EDEVICE;
  if (!p->d_dup_sorted && placer_block(al, &p->d_dup_sorted, nreads, "32 bytes per read, the units in bucket order")) return WFA_HIP_EDEVICE;
  if (!p->d_dup_owned && placer_block(al, &p->d_dup_owned, nreads, "1 byte per read")) return WFA_HIP_EDEVICE;
  if (nbases <= p->dup_bases) return WFA_HIP_OK;
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  if (p->d_dup_plane) pool_release(al, p->d_dup_plane);
  if (p->d_dup_bsum) pool_release(al, p->d_dup_bsum);
  p->d_dup_plane = nullptr; p->d_dup_bsum = nullptr; p->dup_bases = -1;
  const size_t counters = (size_t)nbases + 1, chunks = (counters + WFA_PLACE_SCAN_CHUNK - 1) / WFA_PLACE_SCAN_CHUNK;
  if (placer_block(al, &p->d_dup_plane, counters, "4 bytes per text base, the bucket plane") ||
      placer_block(al, &p->d_dup_bsum, chunks, "the plane scan's chunk sums"))
    return WFA_HIP_EDEVICE;
  p->dup_bases = nbases;
  return WFA_HIP_OK;
}

// group, place and pair as wfa_hip_placer_run_pairs enqueues them, none of their outputs downloaded; then key, scan, scatter and resolve
// (k_dup.hip).  16 bytes per read and per fragment come back.
// Under WFA_HIP_DUP_BY_QUALITY the qsum kernel runs in front of the key kernels; under WFA_HIP_DUP_UNCLIPPED the key kernels take the
// clip words of the records they load.  flags == 0: the launches and allocations of wfa_hip_placer_duplicates before there were flags.
extern "C" int wfa_hip_placer_duplicates_ex(wfa_hip_placer_t* p, const wfa_hip_seqset_t* texts, int32_t min_score, int32_t full_gap,
                                            int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag, const int32_t* mate1,
                                            const int32_t* mate2, int32_t* read_rows, int32_t* pair_rows, int flags,
                                            const wfa_hip_qualset_t* quals, int32_t min_quality) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  if (check_inval(al, wfa::dup_check_flags, flags, quals != nullptr, min_quality)) return WFA_HIP_EINVAL;
  if (quals && quals->al != al) return fail_inval(al, "duplicates: quality set of another aligner");
  if (quals && quals->n < p->nreads)
    return fail_inval(al, "duplicates: the quality set has %lld reads, the placer %lld", (long long)quals->n, (long long)p->nreads);
  if (check_inval(al, wfa::place_check_run, full_gap)) return WFA_HIP_EINVAL;
  if (check_inval(al, wfa::pair_check, p->nreads, min_insert, max_insert, unpaired, nfrag, mate1, mate2)) return WFA_HIP_EINVAL;
  if (!texts) return fail_inval(al, "duplicates: a missing sequence set");
  if (texts->al != al) return fail_inval(al, "duplicates: sequence set of another aligner");
  if (!p->j_rise.empty() && (int64_t)p->j_rise.back().second >= texts->n) {
    size_t k = 0;   // (the rises ascend in j: the first one outside the set is the first such hit of the list)
    while ((int64_t)p->j_rise[k].second < texts->n) ++k;
    return fail_inval(al, "duplicates: text index out of range at position %lld of the hit list: j = %d over %lld texts",
                      (long long)p->j_rise[k].first, (int)p->j_rise[k].second, (long long)texts->n);
  }
  if (check_inval(al, wfa::dup_check, p->nreads, nfrag, read_rows, pair_rows)) return WFA_HIP_EINVAL;
  if (p->nreads == 0) return WFA_HIP_OK;   // (no read: no fragment, no unit)
  HIP_TRY(al, hipSetDevice(al->device));
  int rc = placer_ensure_dup(p, texts->nbytes);
  if (rc != WFA_HIP_OK) return rc;
  StreamScratch sc{al};
  wfa::DupArgs d;
  memset(&d, 0, sizeof(d));
  d.boff = texts->d_boff; d.text_len = texts->d_len; d.ntexts = texts->n; d.nbases = texts->nbytes;
  d.plane = p->d_dup_plane; d.bsum = p->d_dup_bsum; d.rec = p->d_dup_rec; d.sorted = p->d_dup_sorted; d.owned = p->d_dup_owned;
  if (sc.alloc(&d.read_rows, (size_t)p->nreads * WFA_DUP_COLS)) return WFA_HIP_EDEVICE;
  if (nfrag > 0 && sc.alloc(&d.frag_rows, (size_t)nfrag * WFA_DUP_COLS)) return WFA_HIP_EDEVICE;
  d.flags = flags;
  if (flags & WFA_DUP_BY_QUALITY) {
    if (!p->d_dup_qsum && placer_block(al, &p->d_dup_qsum, (size_t)p->nreads, "4 bytes per read, the summed base qualities")) return WFA_HIP_EDEVICE;
    d.qsum = p->d_dup_qsum;
  }
  ReduceTimer timer(al, "duplicates", p->nhits, "hits");
  int pair_rc = 0, lrc = 0;
  if ((rc = placer_enqueue_pairs(p, sc, d.pair, min_score, full_gap, min_insert, max_insert, unpaired, nfrag, mate1, mate2, false, &pair_rc)) != WFA_HIP_OK) return rc;
  if (pair_rc == 0) {
    HIP_TRY(al, hipMemsetAsync(d.plane, 0, ((size_t)d.nbases + 1) * sizeof(uint32_t), al->stream));
    HIP_TRY(al, hipMemsetAsync(d.owned, 0, (size_t)p->nreads, al->stream));
    if (flags & WFA_DUP_BY_QUALITY) {
      wfa::DupQsumArgs q;
      q.quals = quals->d_quals; q.off = quals->d_off; q.len = quals->d_len; q.nreads = p->nreads; q.min_quality = min_quality;
      q.qsum = p->d_dup_qsum;
      lrc = wfa::launch_dup_qsum(q, al->cu_count, al->stream);
    }
    if (lrc == 0) lrc = wfa::launch_dup(d, al->cu_count, al->stream);
  }
  if ((rc = placer_launched(p, timer, pair_rc, "pairing: kernel launch failed")) != WFA_HIP_OK) return rc;
  if (lrc != 0) { (void)hipStreamSynchronize(al->stream); al->err = "duplicates: kernel launch failed"; return WFA_HIP_EDEVICE; }
  if (sc.download(read_rows, d.read_rows, (size_t)p->nreads * WFA_DUP_COLS)) return WFA_HIP_EDEVICE;
  if (nfrag > 0 && sc.download(pair_rows, d.frag_rows, (size_t)nfrag * WFA_DUP_COLS)) return WFA_HIP_EDEVICE;
  return placer_finish(p);
}

extern "C" int wfa_hip_placer_duplicates(wfa_hip_placer_t* p, const wfa_hip_seqset_t* texts, int32_t min_score, int32_t full_gap,
                                         int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag, const int32_t* mate1,
                                         const int32_t* mate2, int32_t* read_rows, int32_t* pair_rows) {
  return wfa_hip_placer_duplicates_ex(p, texts, min_score, full_gap, min_insert, max_insert, unpaired, nfrag, mate1, mate2, read_rows, pair_rows,
                                      0, nullptr, 0);
}
