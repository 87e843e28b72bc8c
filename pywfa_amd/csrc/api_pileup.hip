// api_pileup.hip — pileups and calls of libwfa_hip.so (the C ABI declared in include/wfa_hip.h).
#include "host_sets.hpp"
#include "wfa_deletions.hpp"
#include "wfa_insertions.hpp"
#include "wfa_leftalign.hpp"

// ------------------------------------------------------------------------------------------------
// left alignment of a batch's op strings (include/wfa_hip.h, "left alignment"; csrc/wfa_leftalign.hpp, k_leftalign.hip)
// ------------------------------------------------------------------------------------------------
extern "C" int wfa_hip_batch_left_align(wfa_hip_batch_t* b, int64_t* stats) {
  if (!b) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = b->al;
  int rc = batch_of(al, b, "left alignment", true);
  if (rc != WFA_HIP_OK) return rc;
  rc = wfa_hip_batch_sync(b);
  if (rc != WFA_HIP_OK) return rc;
  if (stats) stats[0] = stats[1] = 0;
  if (b->n == 0) return WFA_HIP_OK;
  HIP_TRY(al, hipSetDevice(al->device));
  b->rle_total = -1;   // the run-length encoding of the strings as they were
  b->sam_serial = -1;  // ... and their SAM fields
  StreamScratch sc{al};
  wfa::LeftAlignArgs a;
  memset(&a, 0, sizeof(a));
  a.ops = b->d_ops; a.cigar_begin = b->d_cigar_begin; a.cigar_len = b->d_cigar_len; a.status = b->d_status;
  a.meta = b->d_meta; a.words = b->d_words; a.bytes = b->d_bytes; a.pboff = b->d_pboff; a.tboff = b->d_tboff; a.flags = b->d_flags;
  a.npairs = b->n;
  if (sc.alloc(&a.stats, 2)) return WFA_HIP_EDEVICE;
  HIP_TRY(al, hipMemsetAsync(a.stats, 0, 2 * sizeof(unsigned long long), al->stream));
  unsigned long long got[2] = {0, 0};
  ReduceTimer timer(al, "left align", b->n);
  const int lrc = wfa::launch_left_align(a, al->cu_count, al->stream);
  timer.stop();
  if (lrc == 0 && sc.download(got, a.stats, 2)) return WFA_HIP_EDEVICE;
  rc = launch_end(al, nullptr, lrc, "left alignment kernel launch failed");
  if (rc == WFA_HIP_OK && stats) { stats[0] = (int64_t)got[0]; stats[1] = (int64_t)got[1]; }
  return rc;
}

// ------------------------------------------------------------------------------------------------
// pileup over a text set (include/wfa_hip.h; csrc/wfa_pileup.hpp, k_pileup.hip)
// ------------------------------------------------------------------------------------------------
static_assert(WFA_PILEUP_COLS == WFA_HIP_PILEUP_COLS, "columns of the kernels and of the ABI");

struct wfa_hip_pileup {
  wfa_hip_aligner* al = nullptr;
  int64_t nseq = 0, total = 0;         // sequences, and bases of all of them (the stride of a plane)
  std::vector<int32_t> h_len;
  std::vector<int64_t> h_off;          // first base of a sequence in a plane
  int32_t* d_table = nullptr;          // WFA_PILEUP_COLS planes of `total` counters (its own allocation: up to 32 bytes x every text base)
  int64_t* d_off = nullptr; int32_t* d_len = nullptr;
  // the insertion log (include/wfa_hip.h, "insertions"; csrc/wfa_insertions.hpp): its own allocations, grown by doubling
  bool track = false, added = false;   // added: an add since the create or the last clear
  wfa::InsRecord* d_rec = nullptr; uint8_t* d_ins = nullptr;
  int64_t nrec = 0, nins = 0, cap_rec = 0, cap_ins = 0;
  // strands (include/wfa_hip.h, "strands and genotypes"): the forward table, of the table's size and layout, while tracking is on
  bool strands = false;
  int32_t* d_fwd = nullptr;
  // base qualities (include/wfa_hip.h, "base qualities"): the quality table, of the table's size and layout, while tracking is on
  bool quals = false;
  int32_t* d_qtab = nullptr;
  // the deletion log and the starts plane (include/wfa_hip.h, "deletions"; csrc/wfa_deletions.hpp): the log grown by doubling, the
  // plane one counter per text base while tracking is on
  bool dels = false;
  wfa::DelRecord* d_del = nullptr;
  int32_t* d_starts = nullptr;
  int64_t ndel = 0, ndel_bases = 0, cap_del = 0;
};

static size_t pileup_plane_bytes(const wfa_hip_pileup* p) { return (size_t)std::max<int64_t>(p->total, 1) * sizeof(int32_t); }

static size_t pileup_table_bytes(const wfa_hip_pileup* p) { return (size_t)std::max<int64_t>(p->total, 1) * WFA_PILEUP_COLS * sizeof(int32_t); }

extern "C" void wfa_hip_pileup_destroy(wfa_hip_pileup_t* p) {
  if (!p) return;
  wfa_hip_aligner* al = p->al;
  (void)hipSetDevice(al->device);
  if (p->d_table) (void)hipFree(p->d_table);
  if (p->d_fwd) (void)hipFree(p->d_fwd);
  if (p->d_qtab) (void)hipFree(p->d_qtab);
  if (p->d_rec) (void)hipFree(p->d_rec);
  if (p->d_ins) (void)hipFree(p->d_ins);
  if (p->d_del) (void)hipFree(p->d_del);
  if (p->d_starts) (void)hipFree(p->d_starts);
  pool_release(al, p->d_off); pool_release(al, p->d_len);
  destroy_end(p);
}

static int pileup_build(wfa_hip_aligner* al, wfa_hip_pileup* p, const wfa_hip_seqset_t* T) {
  p->nseq = T->n;
  p->h_len = T->h_len;
  p->h_off.assign((size_t)T->n + 1, 0);
  for (int64_t k = 0; k < T->n; ++k) p->h_off[(size_t)k + 1] = p->h_off[(size_t)k] + T->h_len[(size_t)k];
  p->total = p->h_off[(size_t)T->n];
  const size_t bytes = (size_t)std::max<int64_t>(p->total, 1) * WFA_PILEUP_COLS * sizeof(int32_t);
  if (hipMalloc((void**)&p->d_table, bytes) != hipSuccess)
    return fail_alloc(al, (void**)&p->d_table, "pileup table: hipMalloc of %zu bytes failed (32 bytes per text base, %lld bases)", bytes, (long long)p->total);
  HIP_TRY(al, poison_fill(al, p->d_table, bytes, al->stream));
  const size_t nn = (size_t)std::max<int64_t>(T->n, 1);
  HIP_TRY(al, pool_alloc(al, (void**)&p->d_off, nn * sizeof(int64_t)));
  HIP_TRY(al, pool_alloc(al, (void**)&p->d_len, nn * sizeof(int32_t)));
  HIP_TRY(al, hipMemsetAsync(p->d_table, 0, bytes, al->stream));
  if (T->n > 0) {
    HIP_TRY(al, hipMemcpyAsync(p->d_off, p->h_off.data(), (size_t)T->n * sizeof(int64_t), hipMemcpyHostToDevice, al->stream));
    HIP_TRY(al, hipMemcpyAsync(p->d_len, p->h_len.data(), (size_t)T->n * sizeof(int32_t), hipMemcpyHostToDevice, al->stream));
  }
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  return WFA_HIP_OK;
}

extern "C" wfa_hip_pileup_t* wfa_hip_pileup_create(wfa_hip_aligner_t* al, const wfa_hip_seqset_t* texts) {
  if (!al) return fail_create(al, "null aligner");
  if (!texts || texts->al != al) return fail_create(al, "sequence set of another aligner");
  if (!create_begin(al)) return nullptr;
  wfa_hip_pileup* p = create_adopt(al, new wfa_hip_pileup());
  return create_done(al, p, pileup_build(al, p, texts), wfa_hip_pileup_destroy);
}

extern "C" int wfa_hip_pileup_clear(wfa_hip_pileup_t* p) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  HIP_TRY(al, hipSetDevice(al->device));
  HIP_TRY(al, hipMemsetAsync(p->d_table, 0, pileup_table_bytes(p), al->stream));
  if (p->d_fwd) HIP_TRY(al, hipMemsetAsync(p->d_fwd, 0, pileup_table_bytes(p), al->stream));
  if (p->d_qtab) HIP_TRY(al, hipMemsetAsync(p->d_qtab, 0, pileup_table_bytes(p), al->stream));
  if (p->d_starts) HIP_TRY(al, hipMemsetAsync(p->d_starts, 0, pileup_plane_bytes(p), al->stream));
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  p->nrec = p->nins = 0;   // (the log's blocks stay for the next adds)
  p->ndel = p->ndel_bases = 0;
  p->added = false;
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_pileup_track_insertions(wfa_hip_pileup_t* p, int on) {
  if (!p) return WFA_HIP_EINVAL;
  if (p->added) return fail_inval(p->al, "pileup: insertion tracking is chosen while the pileup is empty (fresh, or just cleared); this one has been added to");
  p->track = on != 0;
  return WFA_HIP_OK;
}

// a second table of the table's size and layout (`what`: "forward" or "quality"; `kind`: "strand" or "quality"), or with `plane` one
// plane of it (the deletion starts), kept or dropped, only while the pileup is empty; a failure leaves the pileup as it was
static int pileup_track_table(wfa_hip_pileup* p, int on, int32_t** table, bool* tracking, const char* what, const char* kind, bool plane = false) {
  wfa_hip_aligner* al = p->al;
  if (p->added) return fail_inval(al, "pileup: %s tracking is chosen while the pileup is empty (fresh, or just cleared); this one has been added to", kind);
  if ((on != 0) == *tracking) return WFA_HIP_OK;
  HIP_TRY(al, hipSetDevice(al->device));
  if (!on) {
    HIP_TRY(al, hipStreamSynchronize(al->stream));
    (void)hipFree(*table);
    *table = nullptr; *tracking = false;
    return WFA_HIP_OK;
  }
  const size_t bytes = plane ? pileup_plane_bytes(p) : pileup_table_bytes(p);
  int32_t* fresh = nullptr;
  if (hipMalloc((void**)&fresh, bytes) != hipSuccess)
    return fail_alloc(al, (void**)&fresh, "pileup %s %s: hipMalloc of %zu bytes failed (%d more bytes per text base, %lld bases)", what,
                      plane ? "plane" : "table", bytes, plane ? 4 : 32, (long long)p->total);
  hipError_t e = poison_fill(al, fresh, bytes, al->stream);
  if (e == hipSuccess) e = hipMemsetAsync(fresh, 0, bytes, al->stream);
  const hipError_t e2 = hipStreamSynchronize(al->stream);
  if (e != hipSuccess || e2 != hipSuccess) { (void)hipFree(fresh); HIP_TRY(al, e); HIP_TRY(al, e2); }
  *table = fresh; *tracking = true;
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_pileup_track_strands(wfa_hip_pileup_t* p, int on) {
  if (!p) return WFA_HIP_EINVAL;
  return pileup_track_table(p, on, &p->d_fwd, &p->strands, "forward", "strand");
}

extern "C" int wfa_hip_pileup_track_qualities(wfa_hip_pileup_t* p, int on) {
  if (!p) return WFA_HIP_EINVAL;
  return pileup_track_table(p, on, &p->d_qtab, &p->quals, "quality", "quality");
}

extern "C" int wfa_hip_pileup_track_deletions(wfa_hip_pileup_t* p, int on) {
  if (!p) return WFA_HIP_EINVAL;
  return pileup_track_table(p, on, &p->d_starts, &p->dels, "deletion starts", "deletion", true);
}

extern "C" int wfa_hip_pileup_deletion_stats(wfa_hip_pileup_t* p, int64_t* records, int64_t* bases) {
  if (!p) return WFA_HIP_EINVAL;
  if (!p->dels) return fail_inval(p->al, "pileup: this pileup was not made to track deletions");
  if (records) *records = p->ndel;
  if (bases) *bases = p->ndel_bases;
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_pileup_insertion_stats(wfa_hip_pileup_t* p, int64_t* records, int64_t* bases) {
  if (!p) return WFA_HIP_EINVAL;
  if (!p->track) return fail_inval(p->al, "pileup: this pileup was not made to track insertions");
  if (records) *records = p->nrec;
  if (bases) *bases = p->nins;
  return WFA_HIP_OK;
}

// room for `need` elements in a block of the log that holds `have` of them: a new block of twice the size (of the exact size when that
// fails), the old contents copied over.  A failure leaves the block as it was.
template <class T> static int pileup_log_grow(wfa_hip_aligner* al, T** block, int64_t* cap, int64_t have, int64_t need, const char* log,
                                              const char* what) {
  if (need <= *cap) return WFA_HIP_OK;
  T* fresh = nullptr;
  int64_t want = std::max<int64_t>({need, 2 * *cap, 1024});
  if (hipMalloc((void**)&fresh, (size_t)want * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    want = need;
    if (hipMalloc((void**)&fresh, (size_t)want * sizeof(T)) != hipSuccess)
      return fail_alloc(al, (void**)&fresh, "pileup %s log: hipMalloc of %zu bytes failed (%s, %lld of them)", log, (size_t)want * sizeof(T), what, (long long)want);
  }
  // (WFA_HIP_POISON: the fill first, the old contents over it — the grown tail stays filled until an add writes it)
  { const hipError_t e = poison_fill(al, fresh, (size_t)want * sizeof(T), al->stream); if (e != hipSuccess) { (void)hipFree(fresh); HIP_TRY(al, e); } }
  if (have > 0) {
    const hipError_t e = hipMemcpyAsync(fresh, *block, (size_t)have * sizeof(T), hipMemcpyDeviceToDevice, al->stream);
    const hipError_t e2 = hipStreamSynchronize(al->stream);
    if (e != hipSuccess || e2 != hipSuccess) { (void)hipFree(fresh); HIP_TRY(al, e); HIP_TRY(al, e2); }
  }
  if (*block) (void)hipFree(*block);
  *block = fresh; *cap = want;
  return WFA_HIP_OK;
}

// The count pass of a log of an add (csrc/wfa_insertions.hpp, wfa_deletions.hpp; g: InsLogArgs or DelLogArgs, zeroed): the scratch of
// the pass, the zeroed pair counts, launch() = count + the two scans, the 16-byte download of totals = {records, bases} of the batch.
// The caller grows its log by them before anything is written to it.
template <class LogArgs, class Launch>
static int pileup_log_count(wfa_hip_aligner* al, StreamScratch& sc, int64_t npairs, LogArgs* g, uint64_t* totals, const char* label, const char* failed,
                            Launch launch) {
  const size_t n = (size_t)npairs;
  memset(g, 0, sizeof(*g));
  if (sc.alloc(&g->pair_count, n) || sc.alloc(&g->rec_off, n + 1) || sc.alloc(&g->base_off, n + 1)) return WFA_HIP_EDEVICE;
  HIP_TRY(al, hipMemsetAsync(g->pair_count, 0, n * sizeof(*g->pair_count), al->stream));
  totals[0] = totals[1] = 0;
  ReduceTimer timer(al, label, npairs);
  const int lrc = launch();
  timer.stop();
  if (lrc != 0) { al->err = failed; return WFA_HIP_EDEVICE; }
  if (sc.download(&totals[0], g->rec_off + n, 1) || sc.download(&totals[1], g->base_off + n, 1)) return WFA_HIP_EDEVICE;
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  return WFA_HIP_OK;
}

// The insertion log's pass of an add with tracking on, before the table kernel in its tracking form: the count pass and the growth of
// the two blocks.  Nothing is added before the log has its room.
static int pileup_insertions_count(wfa_hip_pileup* p, StreamScratch& sc, const wfa::PileupArgs& a, wfa::InsLogArgs* g, uint64_t* totals) {
  wfa_hip_aligner* al = p->al;
  int rc = pileup_log_count(al, sc, a.npairs, g, totals, "pileup insertion count", "pileup insertion count kernel launch failed",
                            [&] { return wfa::launch_pileup_count(a, *g, al->cu_count, al->stream); });
  if (rc == WFA_HIP_OK) rc = pileup_log_grow(al, &p->d_rec, &p->cap_rec, p->nrec, p->nrec + (int64_t)totals[0], "insertion", "records of 24 bytes");
  if (rc == WFA_HIP_OK) rc = pileup_log_grow(al, &p->d_ins, &p->cap_ins, p->nins, p->nins + (int64_t)totals[1], "insertion", "inserted bases of 1 byte");
  if (rc != WFA_HIP_OK) return rc;
  g->records = p->d_rec; g->bases = p->d_ins;
  g->rec_base = p->nrec; g->base_base = p->nins; g->rec_cap = p->cap_rec; g->base_cap = p->cap_ins;
  return WFA_HIP_OK;
}

// The deletion log's pass of an add (csrc/wfa_deletions.hpp), before the table kernel of whatever form: the count pass and the growth.
// Nothing has been written when it fails.
static int pileup_deletions_count(wfa_hip_pileup* p, StreamScratch& sc, const wfa::PileupArgs& a, wfa::DelLogArgs* g, uint64_t* totals) {
  wfa_hip_aligner* al = p->al;
  int rc = pileup_log_count(al, sc, a.npairs, g, totals, "pileup deletion count", "pileup deletion count kernel launch failed",
                            [&] { return wfa::launch_del_count(a, *g, al->cu_count, al->stream); });
  if (rc == WFA_HIP_OK) rc = pileup_log_grow(al, &p->d_del, &p->cap_del, p->ndel, p->ndel + (int64_t)totals[0], "deletion", "records of 16 bytes");
  if (rc != WFA_HIP_OK) return rc;
  g->records = p->d_del; g->rec_base = p->ndel; g->rec_cap = p->cap_del; g->starts = p->d_starts;
  return WFA_HIP_OK;
}

// ... and behind the table kernel: the records at their scanned offsets, the starts plane
static int pileup_deletions_scatter(wfa_hip_pileup* p, const wfa::PileupArgs& a, const wfa::DelLogArgs& g, const uint64_t* totals) {
  wfa_hip_aligner* al = p->al;
  ReduceTimer timer(al, "pileup deletion scatter", a.npairs);
  const int rc = launch_end(al, &timer, wfa::launch_del_scatter(a, g, al->cu_count, al->stream), "pileup deletion scatter kernel launch failed");
  if (rc == WFA_HIP_OK) { p->ndel += (int64_t)totals[0]; p->ndel_bases += (int64_t)totals[1]; }
  return rc;
}

// what an add with qualities takes on top of the strands' (wfa_hip_pileup_add_quals)
struct PileupQualList {
  const wfa_hip_qualset_t* set; const int32_t* i; const int32_t* p_start;
  int32_t min_base_quality, quality_cap;
};

// the three adds: `stranded` is the entry (wfa_hip_pileup_add_strands), which must match the pileup's setting; `ql` that of
// wfa_hip_pileup_add_quals, which serves a pileup that tracks qualities with and without strands
static int pileup_add(wfa_hip_pileup_t* p, wfa_hip_batch_t* b, const int32_t* j, const int32_t* t_start, const uint8_t* keep, const uint8_t* reverse,
                      bool stranded, const PileupQualList* ql = nullptr) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  int rc = batch_of(al, b, "pileup", true);
  if (rc != WFA_HIP_OK) return rc;
  if (ql && !p->quals) return fail_inval(al, "pileup: this pileup was not made to track qualities (wfa_hip_pileup_track_qualities)");
  if (!ql && p->quals)
    return fail_inval(al, "pileup: this pileup tracks qualities; add to it with wfa_hip_pileup_add_quals, which takes the quality set and the pairs' reads");
  if (ql) {
    stranded = p->strands;
    if (!ql->set || ql->set->al != al) return fail_inval(al, "quality set of another aligner");
    if (ql->min_base_quality < 0 || ql->min_base_quality > WFA_HIP_MAX_QUALITY)
      return fail_inval(al, "pileup: min_base_quality = %d is out of range (0 .. %d)", (int)ql->min_base_quality, WFA_HIP_MAX_QUALITY);
    if (ql->quality_cap < 1 || ql->quality_cap > WFA_HIP_MAX_QUALITY)
      return fail_inval(al, "pileup: quality_cap = %d is out of range (1 .. %d)", (int)ql->quality_cap, WFA_HIP_MAX_QUALITY);
  }
  if (stranded && !p->strands) return fail_inval(al, "pileup: this pileup was not made to track strands (wfa_hip_pileup_track_strands); add to it with wfa_hip_pileup_add");
  if (!stranded && p->strands) return fail_inval(al, "pileup: this pileup tracks strands; add to it with wfa_hip_pileup_add_strands, which takes the pairs' strands");
  const int64_t n = b->n;
  if (n > 0 && !j) return fail_inval(al, "pileup: the text indices are missing");
  for (int64_t q = 0; q < n; ++q) {
    if (j[q] < 0 || j[q] >= p->nseq)
      return fail_inval(al, "pileup: text index out of range at position %lld of the pair list: j = %d over a set of %lld sequences",
                        (long long)q, (int)j[q], (long long)p->nseq);
    const int64_t ts = t_start ? t_start[q] : 0, tl = b->h_tlen[(size_t)q], have = p->h_len[(size_t)j[q]];
    if (ts < 0) return fail_inval(al, "pileup: negative text start at position %lld of the pair list: t_start = %lld", (long long)q, (long long)ts);
    if (ts + tl > have)
      return fail_inval(al, "pileup: text window out of range at position %lld of the pair list: [%lld, %lld + %lld) of sequence %d (%lld bases)",
                        (long long)q, (long long)ts, (long long)ts, (long long)tl, (int)j[q], (long long)have);
  }
  if (ql && n > 0 && !ql->i) return fail_inval(al, "pileup: the read indices are missing");
  for (int64_t q = 0; ql && q < n; ++q) {
    const int32_t r = ql->i[q];
    if (r < 0 || r >= ql->set->n)
      return fail_inval(al, "pileup: read index out of range at position %lld of the pair list: i = %d over a quality set of %lld reads",
                        (long long)q, (int)r, (long long)ql->set->n);
    const int64_t ps = ql->p_start ? ql->p_start[q] : 0, pl = b->h_plen[(size_t)q], have = ql->set->h_len[(size_t)r];
    if (ps < 0) return fail_inval(al, "pileup: negative pattern start at position %lld of the pair list: p_start = %lld", (long long)q, (long long)ps);
    if (ps + pl > have)
      return fail_inval(al, "pileup: pattern window out of range at position %lld of the pair list: [%lld, %lld + %lld) of read %d (%lld qualities)",
                        (long long)q, (long long)ps, (long long)ps, (long long)pl, (int)r, (long long)have);
  }
  rc = wfa_hip_batch_sync(b);
  if (rc != WFA_HIP_OK) return rc;
  if (n == 0) return WFA_HIP_OK;
  HIP_TRY(al, hipSetDevice(al->device));
  StreamScratch sc{al};   // (waits for the stream before the blocks go back)
  int32_t *d_j = nullptr, *d_ts = nullptr;
  uint8_t *d_keep = nullptr, *d_rev = nullptr;
  if (sc.upload(&d_j, j, (size_t)n) || sc.upload_opt(&d_ts, t_start, (size_t)n) || sc.upload_opt(&d_keep, keep, (size_t)n)) return WFA_HIP_EDEVICE;
  if (stranded && sc.upload_opt(&d_rev, reverse, (size_t)n)) return WFA_HIP_EDEVICE;
  wfa::PileupArgs a;
  memset(&a, 0, sizeof(a));
  a.ops = b->d_ops; a.cigar_begin = b->d_cigar_begin; a.cigar_len = b->d_cigar_len; a.status = b->d_status;
  a.meta = b->d_meta; a.words = b->d_words; a.bytes = b->d_bytes; a.pboff = b->d_pboff; a.flags = b->d_flags;
  a.npairs = n; a.j = d_j; a.t_start = d_ts; a.keep = d_keep;
  a.seq_off = p->d_off; a.seq_len = p->d_len; a.nseq = p->nseq; a.total = p->total; a.table = p->d_table;
  // the table kernel of the pileup's form (and the insertion log's count pass before it)
  const auto table_add = [&]() -> int {
    int32_t *d_i = nullptr, *d_ps = nullptr;
    if (ql) {
      if (!stranded && sc.upload_opt(&d_rev, reverse, (size_t)n)) return WFA_HIP_EDEVICE;
      if (sc.upload(&d_i, ql->i, (size_t)n) || sc.upload_opt(&d_ps, ql->p_start, (size_t)n)) return WFA_HIP_EDEVICE;
    }
    const wfa::PileupStrandArgs s{d_rev, p->d_fwd};
    const wfa::PileupQualArgs u = ql ? wfa::PileupQualArgs{ql->set->d_quals, ql->set->d_off, ql->set->d_len, ql->set->n, d_i, d_ps, d_rev,
                                                           ql->min_base_quality, ql->quality_cap, p->d_qtab}
                                     : wfa::PileupQualArgs{};
    wfa::InsLogArgs g;
    uint64_t totals[2] = {0, 0};
    if (p->track) {
      const int crc = pileup_insertions_count(p, sc, a, &g, totals);
      if (crc != WFA_HIP_OK) return crc;
    }
    ReduceTimer timer(al, p->track ? "pileup tracked" : ql ? "pileup qualities" : stranded ? "pileup stranded" : "pileup", n);
    p->added = true;
    const int arc = launch_end(al, &timer, wfa::launch_pileup(a, p->track ? &g : nullptr, stranded ? &s : nullptr, ql ? &u : nullptr, al->cu_count, al->stream),
                               "pileup kernel launch failed");   // (the caller's arrays are read by the copies above)
    if (arc == WFA_HIP_OK) { p->nrec += (int64_t)totals[0]; p->nins += (int64_t)totals[1]; }
    return arc;
  };
  if (!p->dels) return table_add();
  // the deletion log (csrc/wfa_deletions.hpp): its room first, so that a failed growth changes nothing; its records behind the table kernel
  wfa::DelLogArgs dg;
  uint64_t dtotals[2];
  rc = pileup_deletions_count(p, sc, a, &dg, dtotals);
  if (rc == WFA_HIP_OK) rc = table_add();
  if (rc == WFA_HIP_OK) rc = pileup_deletions_scatter(p, a, dg, dtotals);
  return rc;
}

extern "C" int wfa_hip_pileup_add(wfa_hip_pileup_t* p, wfa_hip_batch_t* b, const int32_t* j, const int32_t* t_start, const uint8_t* keep) {
  return pileup_add(p, b, j, t_start, keep, nullptr, false);
}

extern "C" int wfa_hip_pileup_add_strands(wfa_hip_pileup_t* p, wfa_hip_batch_t* b, const int32_t* j, const int32_t* t_start, const uint8_t* keep,
                                          const uint8_t* reverse) {
  return pileup_add(p, b, j, t_start, keep, reverse, true);
}

extern "C" int wfa_hip_pileup_add_quals(wfa_hip_pileup_t* p, wfa_hip_batch_t* b, const int32_t* j, const int32_t* t_start, const uint8_t* keep,
                                        const uint8_t* reverse, const wfa_hip_qualset_t* quals, const int32_t* i, const int32_t* p_start,
                                        int32_t min_base_quality, int32_t quality_cap) {
  const PileupQualList ql{quals, i, p_start, min_base_quality, quality_cap};
  return pileup_add(p, b, j, t_start, keep, reverse, false, &ql);
}

// rows [start, start + len) of sequence seq are rows of the pileup, or the refusal that names them
static int pileup_check_rows(const wfa_hip_pileup* p, int32_t seq, int64_t start, int64_t len) {
  if (seq >= 0 && seq < p->nseq && start >= 0 && len >= 0 && start + len <= p->h_len[(size_t)seq]) return WFA_HIP_OK;
  return fail_inval(p->al, "pileup: rows [%lld, %lld + %lld) of sequence %d are out of range (%lld sequences; sequence length %lld)", (long long)start,
                    (long long)start, (long long)len, (int)seq, (long long)p->nseq, (long long)((seq >= 0 && seq < p->nseq) ? p->h_len[(size_t)seq] : -1));
}

// the rows of one table (the total or the forward one) into `plane`, a stretch of len counters per column; the stream is not waited for
static int pileup_fetch_planes(const wfa_hip_pileup* p, const int32_t* table, int32_t seq, int64_t start, int64_t len, int32_t* plane) {
  for (int c = 0; c < WFA_PILEUP_COLS; ++c)
    HIP_TRY(p->al, hipMemcpyAsync(plane + (size_t)c * (size_t)len, table + (int64_t)c * p->total + p->h_off[(size_t)seq] + start,
                                  (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost, p->al->stream));
  return WFA_HIP_OK;
}

// the rows of one table, interleaved; `table` null: `missing` is the refusal
static int pileup_read_table(wfa_hip_pileup_t* p, const int32_t* table, const char* missing, int32_t seq, int64_t start, int64_t len, int32_t* counts) {
  wfa_hip_aligner* al = p->al;
  if (pileup_check_rows(p, seq, start, len) != WFA_HIP_OK) return WFA_HIP_EINVAL;
  if (!table) return fail_inval(al, "%s", missing);
  if (len == 0) return WFA_HIP_OK;
  if (!counts) return fail_inval(al, "pileup: null output");
  HIP_TRY(al, hipSetDevice(al->device));
  // the table is a plane per column: one copy per plane, interleaved into rows on the host
  std::vector<int32_t> plane((size_t)len * WFA_PILEUP_COLS);
  const int rc = pileup_fetch_planes(p, table, seq, start, len, plane.data());
  if (rc != WFA_HIP_OK) return rc;
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  for (int c = 0; c < WFA_PILEUP_COLS; ++c) {
    const int32_t* src = plane.data() + (size_t)c * (size_t)len;
    for (int64_t r = 0; r < len; ++r) counts[r * WFA_PILEUP_COLS + c] = src[r];
  }
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_pileup_read(wfa_hip_pileup_t* p, int32_t seq, int64_t start, int64_t len, int32_t* counts) {
  if (!p) return WFA_HIP_EINVAL;
  return pileup_read_table(p, p->d_table, "pileup: no table", seq, start, len, counts);
}

extern "C" int wfa_hip_pileup_read_quality(wfa_hip_pileup_t* p, int32_t seq, int64_t start, int64_t len, int32_t* qsums) {
  if (!p) return WFA_HIP_EINVAL;
  return pileup_read_table(p, p->quals ? p->d_qtab : nullptr, "pileup: this pileup was not made to track qualities", seq, start, len, qsums);
}

extern "C" int wfa_hip_pileup_read_strand(wfa_hip_pileup_t* p, int32_t seq, int64_t start, int64_t len, int strand, int32_t* counts) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  if (pileup_check_rows(p, seq, start, len) != WFA_HIP_OK) return WFA_HIP_EINVAL;
  if (strand != 0 && strand != 1) return fail_inval(al, "pileup: strand = %d is out of range (0 forward, 1 reverse)", strand);
  if (!p->strands) return fail_inval(al, "pileup: this pileup was not made to track strands");
  if (len == 0) return WFA_HIP_OK;
  if (!counts) return fail_inval(al, "pileup: null output");
  HIP_TRY(al, hipSetDevice(al->device));
  // forward: the forward table's rows; reverse: the table's rows minus those
  const size_t cells = (size_t)len * WFA_PILEUP_COLS;
  std::vector<int32_t> plane(cells * (strand ? 2 : 1));
  int rc = pileup_fetch_planes(p, p->d_fwd, seq, start, len, plane.data());
  if (rc == WFA_HIP_OK && strand) rc = pileup_fetch_planes(p, p->d_table, seq, start, len, plane.data() + cells);
  if (rc != WFA_HIP_OK) return rc;
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  for (int c = 0; c < WFA_PILEUP_COLS; ++c) {
    const int32_t* f = plane.data() + (size_t)c * (size_t)len;
    for (int64_t r = 0; r < len; ++r) counts[r * WFA_PILEUP_COLS + c] = strand ? f[cells + (size_t)r] - f[r] : f[r];
  }
  return WFA_HIP_OK;
}

// ---- calls and sites of a pileup against its reference set (include/wfa_hip.h; csrc/wfa_calls.hpp, k_calls.hip) ----------------------
static_assert(WFA_SITE_COLS == WFA_HIP_SITE_COLS, "columns of the kernels and of the ABI");

// the checks the two calls share: the set is the pileup's (same aligner, same lengths), the parameters, the range.  On success
// *g0 / *n are the run of global base indices (seq = -1, sites only: every base).
static int calls_check(wfa_hip_pileup* p, const wfa_hip_seqset_t* T, bool sites, int32_t seq, int64_t start, int64_t len, int32_t min_depth,
                       int32_t min_permille, int64_t cap, int64_t* g0, int64_t* n, int32_t permille_lo = 1) {
  wfa_hip_aligner* al = p->al;
  if (!T || T->al != al) return fail_inval(al, "sequence set of another aligner");
  if (T->n != p->nseq) return fail_inval(al, "pileup: the set holds %lld sequences, the pileup was made over %lld", (long long)T->n, (long long)p->nseq);
  for (int64_t k = 0; k < p->nseq; ++k)
    if (T->h_len[(size_t)k] != p->h_len[(size_t)k])
      return fail_inval(al, "pileup: sequence %lld of the set has %lld bases, the pileup was made over %lld", (long long)k,
                        (long long)T->h_len[(size_t)k], (long long)p->h_len[(size_t)k]);
  if (min_depth < 1) return fail_inval(al, "pileup: min_depth = %d is out of range (at least 1)", (int)min_depth);
  if (sites && (min_permille < permille_lo || min_permille > 1000))
    return fail_inval(al, "pileup: min_permille = %d is out of range (%d .. 1000)", (int)min_permille, (int)permille_lo);
  if (sites && cap < 0) return fail_inval(al, "pileup: cap = %lld is negative", (long long)cap);
  if (sites && seq == -1) {
    if (start != 0 || len != -1)
      return fail_inval(al, "pileup: seq = -1 (every sequence) goes with start = 0 and len = -1, got start = %lld, len = %lld", (long long)start, (long long)len);
    *g0 = 0; *n = p->total;
    return WFA_HIP_OK;
  }
  if (pileup_check_rows(p, seq, start, len) != WFA_HIP_OK) return WFA_HIP_EINVAL;
  *g0 = p->h_off[(size_t)seq] + start; *n = len;
  return WFA_HIP_OK;
}

// the end of a calls / sites launch: the timer stopped, the launch's outcome, `count` results back to the caller, the stream synchronised
template <class T> static int calls_launched(StreamScratch& sc, ReduceTimer& timer, int lrc, const char* failed, T* host, const T* dev, size_t count) {
  timer.stop();
  if (lrc != 0) { sc.al->err = failed; return WFA_HIP_EDEVICE; }
  if (sc.download(host, dev, count)) return WFA_HIP_EDEVICE;
  HIP_TRY(sc.al, hipStreamSynchronize(sc.al->stream));
  return WFA_HIP_OK;
}

static wfa::CallsArgs calls_args(const wfa_hip_pileup* p, const wfa_hip_seqset_t* T, int64_t g0, int64_t n, int32_t min_depth, int32_t min_permille) {
  wfa::CallsArgs a;
  memset(&a, 0, sizeof(a));
  a.table = p->d_table; a.total = p->total; a.ref = T->d_bytes; a.g0 = g0; a.n = n; a.min_depth = min_depth; a.min_permille = min_permille;
  a.seq_off = p->d_off; a.nseq = p->nseq;
  return a;
}

// a limit that is read per call from the environment; unset or empty: `preset`
static int64_t env_limit(const char* name, int64_t preset) {
  const char* env = getenv(name);
  return env && *env ? atoll(env) : preset;
}

// the chunks of a run and their two arrays.  Bases per chunk: a multiple of 64 in 64 .. 2^20
static int calls_chunks(StreamScratch& sc, wfa::CallsArgs* a) {
  const int64_t asked = env_limit("WFA_HIP_CALLS_CHUNK", 4096);
  a->chunk = std::min<int64_t>(1 << 20, std::max<int64_t>(64, (std::min<int64_t>(asked, 1 << 20) + 63) / 64 * 64));
  a->chunks = (a->n + a->chunk - 1) / a->chunk;
  if (sc.alloc(&a->chunk_count, (size_t)a->chunks) || sc.alloc(&a->chunk_off, (size_t)a->chunks + 1)) return WFA_HIP_EDEVICE;
  return WFA_HIP_OK;
}

// What the reports of ordered rows (sites, genotypes, insertions, deletions) do alike behind their own checks: the refusals of a null
// count and of null rows, then `also`, a report's own refusal that stands behind those two (nullptr: none); the device, the stream
// waited for, *count = 0.
static int report_begin(wfa_hip_aligner* al, int64_t cap, int64_t* count, const int32_t* rows, const char* also = nullptr) {
  if (!count) return fail_inval(al, "pileup: null count");
  if (cap > 0 && !rows) return fail_inval(al, "pileup: null rows with cap > 0");
  if (also) return fail_inval(al, "%s", also);
  HIP_TRY(al, hipSetDevice(al->device));
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  *count = 0;
  return WFA_HIP_OK;
}

// the count pass of a report over the chunks of c: launch() = count + scan under the timer `label`, *total = chunk_off[chunks] downloaded
template <class Launch>
static int report_total(StreamScratch& sc, const wfa::CallsArgs& c, const char* label, const char* failed, Launch launch, uint64_t* total) {
  ReduceTimer timer(sc.al, label, c.n, "bases");
  return calls_launched(sc, timer, launch(), failed, total, c.chunk_off + c.chunks, 1);
}

// the scratch of the select that the two logs' reports share (a: InsArgs or DelArgs, nsel set): the selected rows, their buckets over
// the log's nrec records, the rows; the fill counters zeroed
template <class Args> static int report_select_scratch(StreamScratch& sc, Args* a, int64_t nrec) {
  const size_t ns = (size_t)a->nsel;
  if (sc.alloc(&a->sel_g, ns) || sc.alloc(&a->bucket_size, ns) || sc.alloc(&a->bucket_off, ns + 1) || sc.alloc(&a->bucket_fill, ns) ||
      sc.alloc(&a->bucket, (size_t)nrec) || sc.alloc(&a->rows, ns * 8))   // (WFA_INSERTION_COLS, WFA_DELETION_COLS)
    return WFA_HIP_EDEVICE;
  HIP_TRY(sc.al, hipMemsetAsync(a->bucket_fill, 0, ns * sizeof(uint32_t), sc.al->stream));
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_pileup_calls(wfa_hip_pileup_t* p, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                    int32_t min_depth, uint8_t* out) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  int64_t g0 = 0, n = 0;
  const int rc = calls_check(p, texts, false, seq, start, len, min_depth, 1, 0, &g0, &n);
  if (rc != WFA_HIP_OK) return rc;
  if (n > 0 && !out) return fail_inval(al, "pileup: null output");
  HIP_TRY(al, hipSetDevice(al->device));
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  if (n == 0) return WFA_HIP_OK;
  StreamScratch sc{al};
  wfa::CallsArgs a = calls_args(p, texts, g0, n, min_depth, 1);
  if (sc.alloc(&a.out, (size_t)n)) return WFA_HIP_EDEVICE;
  ReduceTimer timer(al, "calls", n, "bases");
  return calls_launched(sc, timer, wfa::launch_calls(a, al->cu_count, al->stream), "calls kernel launch failed", out, a.out, (size_t)n);
}

extern "C" int wfa_hip_pileup_sites(wfa_hip_pileup_t* p, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                    int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  int64_t g0 = 0, n = 0;
  const int rc = calls_check(p, texts, true, seq, start, len, min_depth, min_permille, cap, &g0, &n);
  if (rc != WFA_HIP_OK) return rc;
  const int brc = report_begin(al, cap, count, rows);
  if (brc != WFA_HIP_OK) return brc;
  if (n == 0) return WFA_HIP_OK;
  StreamScratch sc{al};
  wfa::CallsArgs a = calls_args(p, texts, g0, n, min_depth, min_permille);
  if (calls_chunks(sc, &a)) return WFA_HIP_EDEVICE;
  uint64_t total = 0;
  const int crc = report_total(sc, a, "sites count", "sites count kernel launch failed", [&] { return wfa::launch_sites_count(a, al->stream); }, &total);
  if (crc != WFA_HIP_OK) return crc;
  *count = (int64_t)total;
  a.cap = std::min<int64_t>((int64_t)total, cap);
  if (a.cap == 0) return WFA_HIP_OK;
  if (sc.alloc(&a.rows, (size_t)a.cap * WFA_SITE_COLS)) return WFA_HIP_EDEVICE;
  ReduceTimer timer(al, "sites scatter", n, "bases");
  return calls_launched(sc, timer, wfa::launch_sites_scatter(a, al->stream), "sites scatter kernel launch failed", rows, a.rows, (size_t)a.cap * WFA_SITE_COLS);
}

// ---- genotyped sites (include/wfa_hip.h, "strands and genotypes"; csrc/wfa_calls.hpp, k_calls.hip) -----------------------------------
static_assert(WFA_GENOTYPE_COLS == WFA_HIP_GENOTYPE_COLS, "columns of the kernels and of the ABI");

// the two genotype calls: `quals` is the entry (wfa_hip_pileup_genotypes_quals), whose scatter pass takes the costs from the quality table
static int pileup_genotypes(wfa_hip_pileup_t* p, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len, int32_t min_depth,
                            int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap, int64_t* count, int32_t* rows, bool quals) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  int64_t g0 = 0, n = 0;
  const int rc = calls_check(p, texts, true, seq, start, len, min_depth, min_permille, cap, &g0, &n);
  if (rc != WFA_HIP_OK) return rc;
  if (quals && !p->quals) return fail_inval(al, "pileup: quality-weighted genotypes need a pileup made to track qualities (wfa_hip_pileup_track_qualities)");
  if (err_q < 1 || err_q > 60) return fail_inval(al, "pileup: err_q = %d is out of range (1 .. 60)", (int)err_q);
  if (min_alt_strand < 0) return fail_inval(al, "pileup: min_alt_strand = %d is negative", (int)min_alt_strand);
  if (min_alt_strand > 0 && !p->strands)
    return fail_inval(al, "pileup: min_alt_strand = %d needs a pileup made to track strands (wfa_hip_pileup_track_strands)", (int)min_alt_strand);
  const int brc = report_begin(al, cap, count, rows);
  if (brc != WFA_HIP_OK) return brc;
  if (n == 0) return WFA_HIP_OK;
  StreamScratch sc{al};
  wfa::GenoArgs a;
  memset(&a, 0, sizeof(a));
  a.c = calls_args(p, texts, g0, n, min_depth, min_permille);
  a.fwd = p->strands ? p->d_fwd : nullptr; a.err_q = err_q; a.min_alt_strand = min_alt_strand;
  if (calls_chunks(sc, &a.c)) return WFA_HIP_EDEVICE;
  uint64_t total = 0;
  const int crc = report_total(sc, a.c, "genotypes count", "genotypes count kernel launch failed", [&] { return wfa::launch_genotypes_count(a, al->stream); }, &total);
  if (crc != WFA_HIP_OK) return crc;
  *count = (int64_t)total;
  a.c.cap = std::min<int64_t>((int64_t)total, cap);
  if (a.c.cap == 0) return WFA_HIP_OK;
  if (sc.alloc(&a.c.rows, (size_t)a.c.cap * WFA_GENOTYPE_COLS)) return WFA_HIP_EDEVICE;
  ReduceTimer timer(al, "genotypes scatter", n, "bases");
  return calls_launched(sc, timer, wfa::launch_genotypes_scatter(a, quals, p->d_qtab, al->stream), "genotypes scatter kernel launch failed", rows, a.c.rows, (size_t)a.c.cap * WFA_GENOTYPE_COLS);
}

extern "C" int wfa_hip_pileup_genotypes(wfa_hip_pileup_t* p, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                        int32_t min_depth, int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap,
                                        int64_t* count, int32_t* rows) {
  return pileup_genotypes(p, texts, seq, start, len, min_depth, min_permille, err_q, min_alt_strand, cap, count, rows, false);
}

extern "C" int wfa_hip_pileup_genotypes_quals(wfa_hip_pileup_t* p, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                              int32_t min_depth, int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap,
                                              int64_t* count, int32_t* rows) {
  return pileup_genotypes(p, texts, seq, start, len, min_depth, min_permille, err_q, min_alt_strand, cap, count, rows, true);
}

// ---- what the reads insert: one allele per reported row (include/wfa_hip.h, "insertions"; csrc/wfa_insertions.hpp, k_insertions.hip) ------
static_assert(WFA_INSERTION_COLS == WFA_HIP_INSERTION_COLS, "columns of the kernels and of the ABI");

extern "C" int wfa_hip_pileup_insertions(wfa_hip_pileup_t* p, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                         int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows,
                                         int64_t bases_cap, int64_t* bases_count, uint8_t* bases) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  int64_t g0 = 0, n = 0;
  const int rc = calls_check(p, texts, true, seq, start, len, min_depth, min_permille, cap, &g0, &n, 0);
  if (rc != WFA_HIP_OK) return rc;
  if (!p->track) return fail_inval(al, "pileup: this pileup was not made to track insertions");
  if (bases_cap < 0) return fail_inval(al, "pileup: bases_cap = %lld is negative", (long long)bases_cap);
  if (!bases_count) return fail_inval(al, "pileup: null count");
  const int brc = report_begin(al, cap, count, rows, bases_cap > 0 && !bases ? "pileup: null bases with bases_cap > 0" : nullptr);
  if (brc != WFA_HIP_OK) return brc;
  *bases_count = 0;
  if (n == 0) return WFA_HIP_OK;
  StreamScratch sc{al};
  wfa::InsArgs a;
  memset(&a, 0, sizeof(a));
  a.c = calls_args(p, texts, g0, n, min_depth, min_permille);
  a.max_reads = (int32_t)std::min<int64_t>(INT32_MAX, std::max<int64_t>(1, env_limit("WFA_HIP_INS_MAX_READS", WFA_HIP_INS_MAX_READS)));   // records per row one wave reduces
  a.records = p->d_rec; a.bases = p->d_ins; a.nrec = p->nrec;
  if (calls_chunks(sc, &a.c)) return WFA_HIP_EDEVICE;
  uint64_t nsel = 0;
  const int crc = report_total(sc, a.c, "insertions count", "insertions count kernel launch failed", [&] { return wfa::launch_ins_select_count(a, al->stream); }, &nsel);
  if (crc != WFA_HIP_OK) return crc;
  if (nsel == 0) return WFA_HIP_OK;
  a.nsel = (int64_t)nsel;
  const size_t ns = (size_t)nsel;
  if (report_select_scratch(sc, &a, p->nrec) || sc.alloc(&a.best, ns) || sc.alloc(&a.allele_len, ns) || sc.alloc(&a.letter_off, ns + 1)) return WFA_HIP_EDEVICE;
  uint64_t nletters = 0;
  {
    ReduceTimer timer(al, "insertions reduce", (int64_t)nsel, "rows");
    int lrc = wfa::launch_ins_select(a, al->stream);
    if (lrc == 0) lrc = wfa::launch_ins_reduce(a, p->nins, al->cu_count, al->stream);
    const int rrc = calls_launched(sc, timer, lrc, "insertions reduce kernel launch failed", &nletters, a.letter_off + ns, 1);
    if (rrc != WFA_HIP_OK) return rrc;
  }
  const int64_t k = std::min<int64_t>((int64_t)nsel, cap);
  if (k > 0) {
    if (sc.download(rows, a.rows, (size_t)k * WFA_INSERTION_COLS)) return WFA_HIP_EDEVICE;
    HIP_TRY(al, hipStreamSynchronize(al->stream));
  }
  *count = (int64_t)nsel; *bases_count = (int64_t)nletters;
  // the letters of the rows that fit whole: a prefix of the byte array (a row's letters start where the rows before it end)
  int64_t end = 0, fit = 0;
  for (int64_t r = 0; r < k; ++r) {
    end += rows[r * WFA_INSERTION_COLS + 5];
    if (end <= bases_cap) fit = end;
  }
  if (fit == 0) return WFA_HIP_OK;
  if (sc.alloc(&a.letters, (size_t)fit)) return WFA_HIP_EDEVICE;
  ReduceTimer timer(al, "insertions letters", k, "rows");
  return calls_launched(sc, timer, wfa::launch_ins_letters(a, k, fit, al->cu_count, al->stream), "insertions letters kernel launch failed", bases, a.letters, (size_t)fit);
}

// ---- what the reads delete: one length per reported row (include/wfa_hip.h, "deletions"; csrc/wfa_deletions.hpp, k_deletions.hip) ---------
static_assert(WFA_DELETION_COLS == WFA_HIP_DELETION_COLS, "columns of the kernels and of the ABI");

extern "C" int wfa_hip_pileup_read_deletion_starts(wfa_hip_pileup_t* p, int32_t seq, int64_t start, int64_t len, int32_t* out) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  if (pileup_check_rows(p, seq, start, len) != WFA_HIP_OK) return WFA_HIP_EINVAL;
  if (!p->dels) return fail_inval(al, "pileup: this pileup was not made to track deletions");
  if (len == 0) return WFA_HIP_OK;
  if (!out) return fail_inval(al, "pileup: null output");
  HIP_TRY(al, hipSetDevice(al->device));
  HIP_TRY(al, hipMemcpyAsync(out, p->d_starts + p->h_off[(size_t)seq] + start, (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost, al->stream));
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_pileup_deletions(wfa_hip_pileup_t* p, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                        int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows) {
  if (!p) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = p->al;
  int64_t g0 = 0, n = 0;
  const int rc = calls_check(p, texts, true, seq, start, len, min_depth, min_permille, cap, &g0, &n, 0);
  if (rc != WFA_HIP_OK) return rc;
  if (!p->dels) return fail_inval(al, "pileup: this pileup was not made to track deletions");
  const int brc = report_begin(al, cap, count, rows);
  if (brc != WFA_HIP_OK) return brc;
  if (n == 0) return WFA_HIP_OK;
  StreamScratch sc{al};
  wfa::DelArgs a;
  memset(&a, 0, sizeof(a));
  a.c = calls_args(p, texts, g0, n, min_depth, min_permille);
  a.starts = p->d_starts;
  a.max_reads = (int32_t)std::min<int64_t>(INT32_MAX, std::max<int64_t>(1, env_limit("WFA_HIP_DEL_MAX_READS", WFA_HIP_DEL_MAX_READS)));   // records per row one wave reduces
  a.records = p->d_del; a.nrec = p->ndel;
  if (calls_chunks(sc, &a.c)) return WFA_HIP_EDEVICE;
  uint64_t nsel = 0;
  const int crc = report_total(sc, a.c, "deletions count", "deletions count kernel launch failed", [&] { return wfa::launch_del_select_count(a, al->stream); }, &nsel);
  if (crc != WFA_HIP_OK) return crc;
  *count = (int64_t)nsel;
  const int64_t k = std::min<int64_t>((int64_t)nsel, cap);
  if (k == 0) return WFA_HIP_OK;
  a.nsel = (int64_t)nsel;
  if (report_select_scratch(sc, &a, p->ndel)) return WFA_HIP_EDEVICE;
  ReduceTimer timer(al, "deletions reduce", (int64_t)nsel, "rows");
  int lrc = wfa::launch_del_select(a, al->stream);
  if (lrc == 0) lrc = wfa::launch_del_reduce(a, al->cu_count, al->stream);
  return calls_launched(sc, timer, lrc, "deletions reduce kernel launch failed", rows, a.rows, (size_t)k * WFA_DELETION_COLS);
}
