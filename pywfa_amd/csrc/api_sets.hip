// api_sets.hip — sequence sets and score matrices of libwfa_hip.so (the C ABI declared in include/wfa_hip.h).
#include "host_sets.hpp"
#include "wfa_cross.hpp"

namespace wfa { bool host_pack_seq(const uint8_t* s, int len, uint32_t* out, int form); }   // host_pack.cpp

// ------------------------------------------------------------------------------------------------
// score matrices (include/wfa_hip.h: sequence sets packed once, cross products in bands of rows, csrc/wfa_cross.hpp)
// ------------------------------------------------------------------------------------------------
static_assert(WFA_CROSS_MAX_K == WFA_HIP_CROSS_MAX_K, "top-k bound of the kernels and of the ABI");

struct wfa_hip_cross {
  wfa_hip_aligner* al = nullptr;
  int64_t m = 0, n = 0;
  int want = 0;
  int32_t* d_score = nullptr; int32_t* d_status = nullptr;           // dense: m x n
  int32_t* d_ci = nullptr; int32_t* d_cj = nullptr; int32_t* d_cs = nullptr;   // completed pairs
  int k = 0;
  uint64_t* d_topk = nullptr;                                          // top-k: m x k keys (wfa_cross.hpp), descending per row
  int64_t count = 0, cap = 0;
  double ms = 0.0;
  int64_t pairs = 0;
};

extern "C" void wfa_hip_seqset_destroy(wfa_hip_seqset_t* s) {
  if (!s) return;
  wfa_hip_aligner* al = s->al;
  (void)hipSetDevice(al->device);
  void* ptrs[] = {s->d_words, s->d_bytes, s->d_woff, s->d_len, s->d_boff, s->d_flag, s->d_mask};
  for (void* p : ptrs) pool_release(al, p);
  destroy_end(s);
}

// the runs of letters host_pack_seq flags (anything but upper-case ACGT) in one sequence
static void flagged_runs(const uint8_t* seq, int32_t len, std::vector<int32_t>& runs) {
  for (int32_t p = 0; p < len;) {
    const uint8_t ch = seq[p];
    if (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') { ++p; continue; }
    int32_t e = p + 1;
    while (e < len && !(seq[e] == 'A' || seq[e] == 'C' || seq[e] == 'G' || seq[e] == 'T')) ++e;
    runs.push_back(p); runs.push_back(e);
    p = e;
  }
}

static int seqset_build(wfa_hip_aligner* al, wfa_hip_seqset* s, int64_t n, const uint8_t* seqs, const int64_t* off, const int32_t* len) {
  s->n = n;
  s->h_len.assign(len, len + n);
  s->h_flag.assign((size_t)n, 0);
  s->h_runs.assign((size_t)n, std::vector<int32_t>());
  std::vector<uint32_t> woff((size_t)n);
  std::vector<int64_t> boff((size_t)n);
  uint64_t w = 0;
  int64_t bb = 0;
  for (int64_t k = 0; k < n; ++k) {
    if (len[k] < 0 || off[k] < 0) return fail_inval(al, "negative length or offset");
    if (len[k] > INT_MAX / 4 - 8) return fail_inval(al, "sequence too long");
    woff[(size_t)k] = (uint32_t)w; w += (uint64_t)((len[k] + 15) >> 4);
    boff[(size_t)k] = bb; bb += len[k];
    if (w > 0x7FFFFFF0ull) return fail_inval(al, "sequence set too large: more than 2^31 packed words");
  }
  s->nwords = w; s->nbytes = bb;
  std::vector<uint32_t> words((size_t)w + 4, 0u);
  std::vector<uint8_t> bytes((size_t)bb + 64, 0u);
  // packed and copied on host threads: m + n sequences, once
  const int nthr = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, std::thread::hardware_concurrency()), (bb >> 20) + 1));
  auto work = [&](int t) {
    for (int64_t k = n * t / nthr, hi = n * (t + 1) / nthr; k < hi; ++k) {
      s->h_flag[(size_t)k] = wfa::host_pack_seq(seqs + off[k], len[k], words.data() + woff[(size_t)k], -1) ? 1 : 0;
      if (s->h_flag[(size_t)k]) flagged_runs(seqs + off[k], len[k], s->h_runs[(size_t)k]);
      if (len[k] > 0) memcpy(bytes.data() + boff[(size_t)k], seqs + off[k], (size_t)len[k]);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nthr; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  const size_t nn = (size_t)std::max<int64_t>(n, 1);
  HIP_TRY(al, pool_alloc(al, (void**)&s->d_words, words.size() * sizeof(uint32_t)));
  HIP_TRY(al, pool_alloc(al, (void**)&s->d_bytes, bytes.size()));
  HIP_TRY(al, pool_alloc(al, (void**)&s->d_woff, nn * sizeof(uint32_t)));
  HIP_TRY(al, pool_alloc(al, (void**)&s->d_len, nn * sizeof(int32_t)));
  HIP_TRY(al, pool_alloc(al, (void**)&s->d_boff, nn * sizeof(int64_t)));
  HIP_TRY(al, pool_alloc(al, (void**)&s->d_flag, nn));
  HIP_TRY(al, hipMemcpy(s->d_words, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(al, hipMemcpy(s->d_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  if (n > 0) {
    HIP_TRY(al, hipMemcpy(s->d_woff, woff.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(al, hipMemcpy(s->d_len, len, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(al, hipMemcpy(s->d_boff, boff.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(al, hipMemcpy(s->d_flag, s->h_flag.data(), (size_t)n, hipMemcpyHostToDevice));
  }
  return WFA_HIP_OK;
}

extern "C" wfa_hip_seqset_t* wfa_hip_seqset_create(wfa_hip_aligner_t* al, int64_t n, const uint8_t* seqs, const int64_t* off, const int32_t* len) {
  if (!al) return fail_create(al, "null aligner");
  if (n < 0 || n > 0x7FFFFFF0ll || (n > 0 && (!seqs || !off || !len))) return fail_create(al, "invalid sequence set arguments");
  if (!create_begin(al)) return nullptr;
  mailbox_release(al);   // (the resident one-pair kernel: sets take the device)
  wfa_hip_seqset* s = create_adopt(al, new wfa_hip_seqset());
  s->wildcard = al->cfg.wildcard;
  return create_done(al, s, seqset_build(al, s, n, seqs, off, len), wfa_hip_seqset_destroy);
}

// ---- the base qualities of a set's sequences (include/wfa_hip.h, "base qualities") ---------------------------------------------------
extern "C" void wfa_hip_qualset_destroy(wfa_hip_qualset_t* s) {
  if (!s) return;
  wfa_hip_aligner* al = s->al;
  (void)hipSetDevice(al->device);
  void* ptrs[] = {s->d_quals, s->d_off, s->d_len};
  for (void* p : ptrs) pool_release(al, p);
  destroy_end(s);
}

// the bytes packed read after read (the caller's offsets need not be), uploaded once
static int qualset_build(wfa_hip_aligner* al, wfa_hip_qualset* s, const wfa_hip_seqset_t* reads, const uint8_t* quals, const int64_t* off) {
  s->n = reads->n;
  s->h_len = reads->h_len;
  std::vector<int64_t> boff((size_t)s->n);
  int64_t bb = 0;
  for (int64_t k = 0; k < s->n; ++k) { boff[(size_t)k] = bb; bb += s->h_len[(size_t)k]; }
  s->nbytes = bb;
  std::vector<uint8_t> bytes((size_t)bb + 64, 0u);
  for (int64_t k = 0; k < s->n; ++k)
    if (s->h_len[(size_t)k] > 0) memcpy(bytes.data() + boff[(size_t)k], quals + off[k], (size_t)s->h_len[(size_t)k]);
  const size_t nn = (size_t)std::max<int64_t>(s->n, 1);
  HIP_TRY(al, pool_alloc(al, (void**)&s->d_quals, bytes.size()));
  HIP_TRY(al, pool_alloc(al, (void**)&s->d_off, nn * sizeof(int64_t)));
  HIP_TRY(al, pool_alloc(al, (void**)&s->d_len, nn * sizeof(int32_t)));
  HIP_TRY(al, hipMemcpy(s->d_quals, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  if (s->n > 0) {
    HIP_TRY(al, hipMemcpy(s->d_off, boff.data(), (size_t)s->n * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(al, hipMemcpy(s->d_len, s->h_len.data(), (size_t)s->n * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  return WFA_HIP_OK;
}

extern "C" wfa_hip_qualset_t* wfa_hip_qualset_create(wfa_hip_aligner_t* al, const wfa_hip_seqset_t* reads, const uint8_t* quals, const int64_t* off,
                                                     const int32_t* len) {
  if (!al) return fail_create(al, "null aligner");
  if (!reads || reads->al != al) return fail_create(al, "sequence set of another aligner");
  const int64_t n = reads->n;
  if (n > 0 && (!quals || !off || !len)) return fail_create(al, "quality set: the qualities, their offsets or their lengths are missing");
  for (int64_t k = 0; k < n; ++k) {
    if (off[k] < 0) return fail_create(al, "quality set: negative offset at entry %lld: off = %lld", (long long)k, (long long)off[k]);
    if (len[k] != reads->h_len[(size_t)k])
      return fail_create(al, "quality set: entry %lld has %d qualities, read %lld of the set has %d bases", (long long)k, (int)len[k], (long long)k,
                         (int)reads->h_len[(size_t)k]);
    for (int32_t x = 0; x < len[k]; ++x)
      if (quals[off[k] + x] > WFA_HIP_MAX_QUALITY)
        return fail_create(al, "quality set: quality %d at position %d of entry %lld is out of range (raw phred, 0 .. %d)", (int)quals[off[k] + x],
                           (int)x, (long long)k, WFA_HIP_MAX_QUALITY);
  }
  if (!create_begin(al)) return nullptr;
  wfa_hip_qualset* s = create_adopt(al, new wfa_hip_qualset());
  return create_done(al, s, qualset_build(al, s, reads, quals, off), wfa_hip_qualset_destroy);
}

extern "C" int64_t wfa_hip_plan_cross_bands(int64_t m, int64_t n, int triangle, int64_t max_pairs, int64_t* row_begin, int64_t cap) {
  if (m < 0 || n < 0 || max_pairs < 1 || (triangle != 0 && triangle != 1)) return WFA_HIP_EINVAL;
  const int64_t rows = (n == 0) ? 0 : (triangle ? n : m);
  if (row_begin && cap >= 1) row_begin[0] = 0;
  int64_t nb = 0, r = 0;
  while (r < rows) {
    int64_t acc = 0, r1 = r;
    if (!triangle) r1 = std::min(rows, r + std::max<int64_t>(1, max_pairs / n));
    else
      while (r1 < rows) {
        const int64_t wr = n - r1;
        if (r1 > r && acc + wr > max_pairs) break;
        acc += wr; ++r1;
      }
    r = r1; ++nb;
    if (row_begin && nb < cap) row_begin[nb] = r;
  }
  return nb;
}

extern "C" void wfa_hip_cross_destroy(wfa_hip_cross_t* x) {
  if (!x) return;
  wfa_hip_aligner* al = x->al;
  (void)hipSetDevice(al->device);
  (void)hipStreamSynchronize(al->stream);
  void* ptrs[] = {x->d_score, x->d_status, x->d_ci, x->d_cj, x->d_cs, x->d_topk};
  for (void* p : ptrs) pool_release(al, p);
  destroy_end(x);
}

// every refusal of a cross run, in this order (T: the text set, the pattern set itself for all-vs-all)
static int cross_check(wfa_hip_aligner* al, const wfa_hip_seqset* P, const wfa_hip_seqset* T, int want, int top_k) {
  if (!P || P->al != al || T->al != al) return fail_inval(al, "sequence set of another aligner");
  if (want <= 0 || (want & ~(WFA_HIP_CROSS_DENSE | WFA_HIP_CROSS_COMPLETED | WFA_HIP_CROSS_TOPK)) != 0)
    return fail_inval(al, "want: a combination of WFA_HIP_CROSS_DENSE, WFA_HIP_CROSS_COMPLETED and WFA_HIP_CROSS_TOPK");
  if ((want & WFA_HIP_CROSS_TOPK) && (top_k < 1 || top_k > WFA_HIP_CROSS_MAX_K)) return fail_inval(al, "k: 1 .. WFA_HIP_CROSS_MAX_K (64)");
  if (P->wildcard != al->cfg.wildcard || T->wildcard != al->cfg.wildcard) return fail_inval(al, "sequence set packed under another wildcard: create it again");
  const wfa_hip_config_t& c = al->cfg;
  if (c.span == WFA_SPAN_ENDSFREE && P->n > 0 && T->n > 0) {   // (wavefront_align.c:86-102, as batch_build)
    const int32_t minp = *std::min_element(P->h_len.begin(), P->h_len.end()), mint = *std::min_element(T->h_len.begin(), T->h_len.end());
    if (c.pattern_begin_free > minp || c.pattern_end_free > minp || c.text_begin_free > mint || c.text_end_free > mint)
      return fail_inval(al, "Ends-free parameters must be not larger than the sequences");
  }
  return WFA_HIP_OK;
}

// What a cross run over non-empty sets fixes on the host before anything is allocated (plan_cross)
struct CrossPlan {
  wfa_hip_config_t c;              // the aligner's configuration, scope = score
  bool ava = false, mirror = false, all_bytes = false, any_bytes = false;
  int tri = 0;                     // 1: the bands are rows of the upper triangle (the mirror rule holds)
  int64_t n = 0, rows = 0;         // columns, and rows that are run
  std::vector<int64_t> col_flag, row_bytes;   // prefix sums: flagged columns, byte pairs of the rows
  std::vector<int32_t> suf_t;      // the longest text at or behind column j (a triangle row's columns)
  int slot_p = 0, slot_t = 0;      // words of the longest pattern / text of up to WFA_FAST_MAX_LEN bases (a pair's slot)
  int64_t band_max = 0, nbands = 0, cap = 0;   // pairs a band may hold, bands, pairs of the largest band
  std::vector<int64_t> rb;         // first row of every band, and `rows`
  uint32_t t_wshift = 0; int64_t t_bshift = 0;   // where the text set's words / bytes start in the view's tables
  uint64_t table_words = 0, slot_words = 0;      // words in front of the slots, words of a slot
  int64_t tri_before(int64_t i) const { return i * n - (i * (i - 1)) / 2; }   // pairs of the triangle rows above row i
};

// the plan of a run: the mirror rule, the 2-bit / byte split of every row, the bands (one free_budget read sizes them: no other device call)
static void plan_cross(wfa_hip_aligner* al, const wfa_hip_seqset* P, const wfa_hip_seqset* T, bool ava, CrossPlan* p) {
  wfa_hip_config_t& c = p->c;
  c = al->cfg;
  c.scope = WFA_SCOPE_SCORE;
  const int64_t m = P->n, n = T->n;
  p->ava = ava; p->n = n;
  // the mirror rule: the score of (P[j], P[i]) is that of (P[i], P[j]) when nothing tells the pattern from the text — no heuristic (their
  // cut-offs look at offsets, not at the alignment's symmetry) and the same free ends on both sides
  p->mirror = ava && c.heuristic == WFA_HEUR_NONE &&
              (c.span == WFA_SPAN_END2END || (c.pattern_begin_free == c.text_begin_free && c.pattern_end_free == c.text_end_free));
  const int tri = p->tri = p->mirror ? 1 : 0;
  const int64_t rows = p->rows = tri ? n : m;
  const bool all_bytes = p->all_bytes = c.wildcard >= 0 && wildcard_in_acgt(c.wildcard);
  // the 2-bit / byte split of every row, from the sets' flags (host prefix sums: no band reads anything back for it)
  std::vector<int64_t>& col_flag = p->col_flag; std::vector<int64_t>& row_bytes = p->row_bytes;
  col_flag.assign((size_t)n + 1, 0); row_bytes.assign((size_t)rows + 1, 0);
  for (int64_t j = 0; j < n; ++j) col_flag[(size_t)j + 1] = col_flag[(size_t)j] + ((all_bytes || T->h_flag[(size_t)j]) ? 1 : 0);
  for (int64_t i = 0; i < rows; ++i) {
    const bool pf = all_bytes || P->h_flag[(size_t)i];
    const int64_t cnt = tri ? (pf ? n - i : col_flag[(size_t)n] - col_flag[(size_t)i]) : (pf ? n : col_flag[(size_t)n]);
    row_bytes[(size_t)i + 1] = row_bytes[(size_t)i] + cnt;
  }
  p->any_bytes = row_bytes[(size_t)rows] > 0;
  p->suf_t.assign((size_t)n + 1, 0);
  for (int64_t j = n - 1; j >= 0; --j) p->suf_t[(size_t)j] = std::max(p->suf_t[(size_t)j + 1], T->h_len[(size_t)j]);
  // band size: the knob, else what the lengths and the free memory allow (about 100 B of band arrays per pair; the workspace of the
  // general kernel is sized from the reads, not from the band)
  int slot_p = 0, slot_t = 0;
  for (int32_t l : P->h_len) if (l <= WFA_FAST_MAX_LEN) slot_p = std::max(slot_p, (l + 15) >> 4);
  for (int32_t l : T->h_len) if (l <= WFA_FAST_MAX_LEN) slot_t = std::max(slot_t, (l + 15) >> 4);
  int64_t band_max = knob(al, K_CROSS_BAND, 0);
  if (band_max <= 0) band_max = std::max<int64_t>(65536, std::min<int64_t>((int64_t)1 << 23, free_budget(al) / 4 / (112 + 4 * (slot_p + slot_t))));
  band_max = std::min<int64_t>(band_max, (int64_t)1 << 30);
  band_max = std::max<int64_t>(1, std::min<int64_t>(band_max, (int64_t)((0xFFFFFFF0ull - P->nwords - T->nwords - 64) / (uint64_t)std::max(1, slot_p + slot_t))));
  p->slot_p = slot_p; p->slot_t = slot_t; p->band_max = band_max;
  p->nbands = wfa_hip_plan_cross_bands(m, n, tri, band_max, nullptr, 0);
  p->rb.resize((size_t)p->nbands + 1);
  wfa_hip_plan_cross_bands(m, n, tri, band_max, p->rb.data(), p->nbands + 1);
  for (int64_t k = 0; k < p->nbands; ++k)
    p->cap = std::max(p->cap, tri ? p->tri_before(p->rb[(size_t)k + 1]) - p->tri_before(p->rb[(size_t)k]) : (p->rb[(size_t)k + 1] - p->rb[(size_t)k]) * n);
  p->t_wshift = ava ? 0u : (uint32_t)P->nwords;
  p->t_bshift = ava ? 0 : P->nbytes;
  p->table_words = P->nwords + (ava ? 0 : T->nwords) + 64;
  p->slot_words = (uint64_t)slot_p + slot_t;
}

struct ViewGuard {   // (the result and list pointers of the last band are the matrix's or the scratch's: not the view's to release)
  wfa_hip_batch* b = nullptr;
  ~ViewGuard() { if (b) { b->d_score = b->d_status = nullptr; b->d_list_packed = b->d_list_bytes = nullptr; batch_free(b); } }
};

// One cross run over non-empty sets: what its steps share.  The scratch pointers are null where the run does not need their group
struct CrossRun {
  wfa_hip_aligner* al; const wfa_hip_seqset *P, *T; wfa_hip_cross* x;
  bool dense, completed, topk;
  CrossPlan plan;
  StreamScratch sc;                 // (declared in front of the view: released after it)
  ViewGuard view;                  // the batch view: one for every band, so that the pilots' picks of the first large band hold for the later ones
  uint32_t *list_packed = nullptr, *list_bytes = nullptr;        // byte pairs: a band's two work lists ...
  int64_t *d_row_bytes = nullptr, *d_col_flag = nullptr;         // ... and the plan's two prefix tables
  int32_t *band_score = nullptr, *band_status = nullptr;         // a band's own results
  int32_t *st_i[2] = {nullptr, nullptr}, *st_j[2] = {nullptr, nullptr}, *st_s[2] = {nullptr, nullptr};   // completed pairs: two staging lists
  uint32_t *blk = nullptr, *d_cnt = nullptr;
  int64_t chunk = 0;               // top-k: cells of a row chunk, and the chunk lists
  uint64_t* part = nullptr;
  CrossRun(wfa_hip_aligner* al_, const wfa_hip_seqset* P_, const wfa_hip_seqset* T_, wfa_hip_cross* x_)
      : al(al_), P(P_), T(T_), x(x_), dense((x_->want & WFA_HIP_CROSS_DENSE) != 0), completed((x_->want & WFA_HIP_CROSS_COMPLETED) != 0),
        topk((x_->want & WFA_HIP_CROSS_TOPK) != 0), sc{al_} {}
  // chunks of a band row that starts at row r0b (0: the row is reduced whole)
  int64_t band_chunks(int64_t r0b) const { const int64_t len = plan.tri ? plan.n - r0b : plan.n; return len > chunk ? (len + chunk - 1) / chunk : (int64_t)0; }
};

// the batch view of a run: its configuration, the word and byte tables (copied from the sets) and what every band's pairs need
static int cross_view_alloc(CrossRun& run) {
  wfa_hip_aligner* al = run.al;
  const wfa_hip_seqset *P = run.P, *T = run.T;
  const CrossPlan& p = run.plan;
  const bool ava = p.ava;
  wfa_hip_batch* b = run.view.b = batch_new(al);
  b->cfg = p.c;
  derive_dev_config(p.c, &b->dcfg, &b->ncomp, &b->gcfg, &b->gncomp);
  if (!al->dcfg.rtc) { b->dcfg.rtc = 0; b->gcfg.rtc = 0; }   // (the run-time path failed earlier on this aligner)
  if (p.c.wildcard >= 0 && !p.all_bytes) { b->wild = p.c.wildcard; b->dcfg.wildcard = -1; b->gcfg.wildcard = -1; }   // (as batch_build)
  HIP_TRY(al, pool_alloc(al, (void**)&b->d_bytes, (size_t)(P->nbytes + (ava ? 0 : T->nbytes) + 64)));
  if (copy_sets(al, b->d_bytes, P->d_bytes, (size_t)P->nbytes, T->d_bytes, (size_t)T->nbytes, ava, 64)) return WFA_HIP_EDEVICE;
  // One word table per run: the pattern set's words, the text set's (cross mode), 64 zero words, then a slot per pair of a band for the
  // pairs of up to WFA_FAST_MAX_LEN bases: the register stages (wfa_lane.hpp, wfa_seg.hpp) fetch a pair's pattern and text words in ONE
  // load, the text's words right behind the pattern's, so the generator copies both sequences of such a pair into its slot.  Longer pairs
  // point into the sets' words (every other stage reads pattern and text through their own offsets).
  if (p.table_words + (uint64_t)p.cap * p.slot_words > 0xFFFFFFF0ull) return fail_inval(al, "sequence sets too large: more than 2^32 words of a band");
  HIP_TRY(al, pool_alloc(al, (void**)&b->d_words, (size_t)(p.table_words + (uint64_t)p.cap * p.slot_words) * sizeof(uint32_t)));
  if (copy_sets(al, b->d_words, P->d_words, (size_t)P->nwords, T->d_words, (size_t)T->nwords, ava, 0)) return WFA_HIP_EDEVICE;
  HIP_TRY(al, hipMemsetAsync(b->d_words + p.table_words - 64, 0, 64 * sizeof(uint32_t), al->stream));
  const size_t ncap = (size_t)p.cap;
  HIP_TRY(al, pool_alloc(al, (void**)&b->d_meta, ncap * sizeof(WfaPairMeta)));
  HIP_TRY(al, pool_alloc(al, (void**)&b->d_flags, ncap));
  HIP_TRY(al, pool_alloc(al, (void**)&b->d_fb_list2[0], ncap * sizeof(uint32_t)));
  HIP_TRY(al, pool_alloc(al, (void**)&b->d_fb_list2[1], ncap * sizeof(uint32_t)));
  HIP_TRY(al, pool_alloc(al, (void**)&b->d_counters, WFA_COUNTER_WORDS * sizeof(uint32_t)));
  HIP_TRY(al, hipMemsetAsync(b->d_counters, 0, WFA_COUNTER_WORDS * sizeof(uint32_t), al->stream));
  if (p.any_bytes) {
    HIP_TRY(al, pool_alloc(al, (void**)&b->d_pboff, ncap * sizeof(int64_t)));
    HIP_TRY(al, pool_alloc(al, (void**)&b->d_tboff, ncap * sizeof(int64_t)));
  }
  return WFA_HIP_OK;
}

// the run's optional blocks besides the view's, by group: byte pairs, a band's own results, completed pairs, top-k (its chunk is sized here)
static int cross_scratch_alloc(CrossRun& run) {
  wfa_hip_aligner* al = run.al;
  const CrossPlan& p = run.plan;
  StreamScratch& sc = run.sc;
  const size_t ncap = (size_t)p.cap;
  if (p.any_bytes) {
    if (sc.alloc(&run.list_packed, ncap) || sc.alloc(&run.list_bytes, ncap) || sc.alloc(&run.d_row_bytes, p.row_bytes.size()) || sc.alloc(&run.d_col_flag, p.col_flag.size()))
      return WFA_HIP_EDEVICE;
    HIP_TRY(al, hipMemcpy(run.d_row_bytes, p.row_bytes.data(), p.row_bytes.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(al, hipMemcpy(run.d_col_flag, p.col_flag.data(), p.col_flag.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  // a band's own score / status: always, except rectangular bands of a dense run (those ARE the matrix's rows r0 .. r1)
  if (p.tri || !run.dense) {
    if (sc.alloc(&run.band_score, ncap) || sc.alloc(&run.band_status, ncap)) return WFA_HIP_EDEVICE;
  }
  // completed pairs: each band compacts into one of two staging lists; the band before is appended to the handle's list once its
  // count is known (read while the next band runs)
  if (run.completed) {
    for (int h = 0; h < 2; ++h)
      if (sc.alloc(&run.st_i[h], ncap) || sc.alloc(&run.st_j[h], ncap) || sc.alloc(&run.st_s[h], ncap)) return WFA_HIP_EDEVICE;
    if (sc.alloc(&run.blk, (ncap + WFA_CROSS_CHUNK - 1) / WFA_CROSS_CHUNK) || sc.alloc(&run.d_cnt, 2)) return WFA_HIP_EDEVICE;
    HIP_TRY(al, hipHostMalloc((void**)&sc.h_cnt, 2 * sizeof(uint32_t), hipHostMallocDefault));
    for (int h = 0; h < 2; ++h) HIP_TRY(al, hipEventCreateWithFlags(&sc.ev[h], hipEventDisableTiming));
  }
  // top-k: the running lists (m x k keys, "empty") and the row pass's chunk lists.  A band row longer than one chunk is split into
  // chunks of `chunk` cells, each reduced by a wave of its own (a band of a wide rectangle holds few rows); the chunk grows until the
  // largest band's chunk lists fit a share of the memory that is free now, behind every block above
  if (run.topk) {
    wfa_hip_cross* x = run.x;
    HIP_TRY(al, pool_alloc(al, (void**)&x->d_topk, (size_t)x->m * (size_t)x->k * sizeof(uint64_t)));
    HIP_TRY(al, hipMemsetAsync(x->d_topk, 0, (size_t)x->m * (size_t)x->k * sizeof(uint64_t), al->stream));
    run.chunk = std::max<int64_t>(64, ((int64_t)knob(al, K_CROSS_TOPK_CHUNK, 4096) + 63) / 64 * 64);
    int64_t part_keys = 0;
    for (;;) {
      part_keys = 0;
      for (int64_t kb = 0; kb < p.nbands; ++kb)
        part_keys = std::max(part_keys, (p.rb[(size_t)kb + 1] - p.rb[(size_t)kb]) * run.band_chunks(p.rb[(size_t)kb]) * x->k);
      if (part_keys * (int64_t)sizeof(uint64_t) <= std::max<int64_t>(free_budget(al) / 8, (int64_t)64 << 20) || run.chunk >= ((int64_t)1 << 30)) break;
      run.chunk *= 2;
    }
    if (part_keys > 0 && sc.alloc(&run.part, (size_t)part_keys)) return WFA_HIP_EDEVICE;
  }
  return WFA_HIP_OK;
}

// append band k's completed pairs to the handle's list, once its count has arrived (the list grows by doubling)
static int cross_drain(CrossRun& run, int64_t k) {
  wfa_hip_aligner* al = run.al;
  wfa_hip_cross* x = run.x;
  const int h = (int)(k & 1);
  HIP_TRY(al, hipEventSynchronize(run.sc.ev[h]));
  const int64_t cnt = run.sc.h_cnt[h];
  if (cnt == 0) return WFA_HIP_OK;
  if (x->count + cnt > x->cap) {
    const int64_t ncap2 = std::max<int64_t>(x->count + cnt, std::max<int64_t>(2 * x->cap, 4096));
    int32_t* nb[3] = {nullptr, nullptr, nullptr};
    int32_t** old[3] = {&x->d_ci, &x->d_cj, &x->d_cs};
    for (int a = 0; a < 3; ++a) {
      HIP_TRY(al, pool_alloc(al, (void**)&nb[a], (size_t)ncap2 * sizeof(int32_t)));
      if (x->count) HIP_TRY(al, hipMemcpyAsync(nb[a], *old[a], (size_t)x->count * sizeof(int32_t), hipMemcpyDeviceToDevice, al->stream));
      pool_release(al, *old[a]);   // (back to the pool; anything that takes it again is ordered behind this copy on the stream)
      *old[a] = nb[a];
    }
    x->cap = ncap2;
  }
  HIP_TRY(al, hipMemcpyAsync(x->d_ci + x->count, run.st_i[h], (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToDevice, al->stream));
  HIP_TRY(al, hipMemcpyAsync(x->d_cj + x->count, run.st_j[h], (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToDevice, al->stream));
  HIP_TRY(al, hipMemcpyAsync(x->d_cs + x->count, run.st_s[h], (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToDevice, al->stream));
  x->count += cnt;
  return WFA_HIP_OK;
}

// one band of a run: its number, rows [r0, r1), the triangle pairs above r0, its pairs and how many of them are byte pairs
struct CrossBand { int64_t k, r0, r1, tri0, np, nbytes; };

// band k of the plan; the view's per-band fields (sizes, work lists, where the results go) are pointed at it
static CrossBand cross_band_view(CrossRun& run, int64_t k) {
  const CrossPlan& p = run.plan;
  wfa_hip_batch* b = run.view.b;
  const int tri = p.tri;
  const int64_t n = p.n;
  const int64_t r0 = p.rb[(size_t)k], r1 = p.rb[(size_t)k + 1];
  const int64_t tri0 = tri ? p.tri_before(r0) : 0;
  const int64_t np = tri ? p.tri_before(r1) - tri0 : (r1 - r0) * n;
  const int64_t nbytes = p.row_bytes[(size_t)r1] - p.row_bytes[(size_t)r0];
  int maxp = 0, maxw = 0;
  for (int64_t i = r0; i < r1; ++i) {
    const int32_t pl = run.P->h_len[(size_t)i], tl = p.suf_t[tri ? (size_t)i : 0];
    maxp = std::max(maxp, pl); maxw = std::max(maxw, pl + tl);
  }
  b->n = np;
  b->n_bytes = (uint32_t)nbytes; b->n_packed = (uint32_t)(np - nbytes);
  b->max_len = std::max(maxp, p.suf_t[tri ? (size_t)r0 : 0]);
  b->max_width = maxw + 3;
  b->d_list_packed = (nbytes > 0 && np > nbytes) ? run.list_packed : nullptr;
  b->d_list_bytes = nbytes > 0 ? run.list_bytes : nullptr;
  b->d_score = run.band_score ? run.band_score : run.x->d_score + r0 * n;
  b->d_status = run.band_status ? run.band_status : run.x->d_status + r0 * n;
  return CrossBand{k, r0, r1, tri0, np, nbytes};
}

// the generator: the band's metadata, slots and work lists, written on the device
static int cross_band_generate(CrossRun& run, const CrossBand& bd) {
  wfa_hip_aligner* al = run.al;
  const wfa_hip_seqset *P = run.P, *T = run.T;
  const CrossPlan& p = run.plan;
  wfa_hip_batch* b = run.view.b;
  wfa::CrossGenArgs ga;
  memset(&ga, 0, sizeof(ga));
  ga.p_woff = P->d_woff; ga.p_len = P->d_len; ga.p_boff = P->d_boff; ga.p_flag = P->d_flag;
  ga.t_woff = T->d_woff; ga.t_len = T->d_len; ga.t_boff = T->d_boff; ga.t_flag = T->d_flag;
  ga.t_wshift = p.t_wshift; ga.t_bshift = p.t_bshift;
  ga.words = b->d_words; ga.slot_base = (uint32_t)p.table_words; ga.slot_words = (uint32_t)p.slot_words;
  ga.row_bytes = run.d_row_bytes; ga.col_flag = run.d_col_flag;
  ga.n = p.n; ga.r0 = bd.r0; ga.tri0 = bd.tri0; ga.npairs = bd.np; ga.tri = p.tri; ga.all_bytes = p.all_bytes ? 1 : 0; ga.lists = bd.nbytes > 0 ? 1 : 0;
  ga.meta = b->d_meta; ga.pboff = b->d_pboff; ga.tboff = b->d_tboff; ga.flags = b->d_flags;
  ga.list_packed = run.list_packed; ga.list_bytes = run.list_bytes;
  if (wfa::launch_cross_gen(ga, al->stream) != 0) { al->err = "cross band generator launch failed"; return WFA_HIP_EDEVICE; }
  return WFA_HIP_OK;
}

// what the run keeps of a finished band: the dense scatter (triangle bands), the compaction of its completed pairs into the band's
// staging list (its count travels while band k - 1 is drained), its rows' top-k
static int cross_band_reduce(CrossRun& run, const CrossBand& bd) {
  wfa_hip_aligner* al = run.al;
  const CrossPlan& p = run.plan;
  wfa_hip_cross* x = run.x;
  wfa_hip_batch* b = run.view.b;
  wfa::CrossResArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.score = b->d_score; ra.status = b->d_status;
  ra.n = p.n; ra.r0 = bd.r0; ra.tri0 = bd.tri0; ra.npairs = bd.np; ra.tri = p.tri; ra.upper = p.ava ? 1 : 0; ra.mirror = p.mirror ? 1 : 0;
  ra.dense_score = x->d_score; ra.dense_status = x->d_status;
  if (run.dense && p.tri && wfa::launch_cross_scatter(ra, al->stream) != 0) { al->err = "cross scatter launch failed"; return WFA_HIP_EDEVICE; }
  if (run.completed) {
    const int h = (int)(bd.k & 1);
    ra.blk_count = run.blk; ra.band_count = run.d_cnt + h; ra.out_i = run.st_i[h]; ra.out_j = run.st_j[h]; ra.out_score = run.st_s[h];
    if (wfa::launch_cross_compact(ra, al->stream) != 0) { al->err = "cross compaction launch failed"; return WFA_HIP_EDEVICE; }
    HIP_TRY(al, hipMemcpyAsync(run.sc.h_cnt + h, run.d_cnt + h, sizeof(uint32_t), hipMemcpyDeviceToHost, al->stream));
    HIP_TRY(al, hipEventRecord(run.sc.ev[h], al->stream));
    if (bd.k > 0) { const int rc = cross_drain(run, bd.k - 1); if (rc != WFA_HIP_OK) return rc; }
  }
  if (run.topk) {
    wfa::CrossTopkArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.score = b->d_score; ta.status = b->d_status;
    ta.n = p.n; ta.r0 = bd.r0; ta.r1 = bd.r1; ta.tri0 = bd.tri0; ta.tri = p.tri; ta.ava = p.ava ? 1 : 0;
    ta.k = x->k; ta.chunk = run.chunk; ta.nch = run.band_chunks(bd.r0); ta.part = run.part; ta.run = x->d_topk;
    if (wfa::launch_cross_topk(ta, al->stream) != 0) { al->err = "cross top-k launch failed"; return WFA_HIP_EDEVICE; }
  }
  return WFA_HIP_OK;
}

// band k from end to end: view, generator, pilots, the batch run, what the run keeps of it
static int cross_band(CrossRun& run, int64_t k) {
  const CrossBand bd = cross_band_view(run, k);
  { const int rc = cross_band_generate(run, bd); if (rc != WFA_HIP_OK) return rc; }
  // the pilots: no-ops once the first band of >= 64 k pairs has picked (the picks live in the view)
  { const int prc = run_pilots(run.al, run.view.b); if (prc != WFA_HIP_OK) return prc; }
  { const int rc = wfa_hip_batch_run(run.view.b, nullptr); if (rc != WFA_HIP_OK) return rc; }
  { const int rc = cross_band_reduce(run, bd); if (rc != WFA_HIP_OK) return rc; }
  run.x->pairs += bd.np;
  return WFA_HIP_OK;
}

// a whole run into the handle x: check, the dense matrix, plan, the view and the scratch, band by band, the last drain
static int cross_run_impl(wfa_hip_aligner* al, const wfa_hip_seqset* P, const wfa_hip_seqset* T, int want, int top_k, wfa_hip_cross* x) {
  const bool ava = (T == nullptr);
  if (ava) T = P;
  { const int rc = cross_check(al, P, T, want, top_k); if (rc != WFA_HIP_OK) return rc; }
  const int64_t m = P->n, n = T->n;
  x->m = m; x->n = n; x->want = want;
  if (want & WFA_HIP_CROSS_TOPK) x->k = top_k;
  if ((want & WFA_HIP_CROSS_DENSE) && m * n > 0) {
    HIP_TRY(al, pool_alloc(al, (void**)&x->d_score, (size_t)(m * n) * sizeof(int32_t)));
    HIP_TRY(al, pool_alloc(al, (void**)&x->d_status, (size_t)(m * n) * sizeof(int32_t)));
  }
  if (m == 0 || n == 0) return WFA_HIP_OK;   // (top-k: all padding, written by wfa_hip_cross_topk)
  CrossRun run(al, P, T, x);
  plan_cross(al, P, T, ava, &run.plan);
  { const int rc = cross_view_alloc(run); if (rc != WFA_HIP_OK) return rc; }
  { const int rc = cross_scratch_alloc(run); if (rc != WFA_HIP_OK) return rc; }
  for (int64_t k = 0; k < run.plan.nbands; ++k) { const int rc = cross_band(run, k); if (rc != WFA_HIP_OK) return rc; }
  if (run.completed && run.plan.nbands > 0) { const int rc = cross_drain(run, run.plan.nbands - 1); if (rc != WFA_HIP_OK) return rc; }
  { const int rc = wfa_hip_batch_sync(run.view.b); if (rc != WFA_HIP_OK) return rc; }
  x->ms = run.view.b->ms_sum;
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  return WFA_HIP_OK;
}

extern "C" wfa_hip_cross_t* wfa_hip_cross_run_k(wfa_hip_aligner_t* al, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts, int want, int k) {
  if (!create_begin(al)) return nullptr;
  mailbox_release(al);
  wfa_hip_cross* x = create_adopt(al, new wfa_hip_cross());
  return create_done(al, x, cross_run_impl(al, patterns, texts, want, k, x), wfa_hip_cross_destroy);
}

extern "C" wfa_hip_cross_t* wfa_hip_cross_run(wfa_hip_aligner_t* al, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts, int want) {
  if (al && (want & WFA_HIP_CROSS_TOPK)) return fail_create(al, "want: WFA_HIP_CROSS_DENSE and / or WFA_HIP_CROSS_COMPLETED (top-k: wfa_hip_cross_run_k)");
  return wfa_hip_cross_run_k(al, patterns, texts, want, 0);
}

extern "C" int wfa_hip_cross_topk(wfa_hip_cross_t* x, int32_t* j, int32_t* score) {
  if (!x) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = x->al;
  if (!(x->want & WFA_HIP_CROSS_TOPK)) return fail_inval(al, "the run was made without WFA_HIP_CROSS_TOPK");
  const size_t cells = (size_t)x->m * (size_t)x->k;
  if (cells == 0) return WFA_HIP_OK;
  if (!j || !score) return fail_inval(al, "j/score outputs are required");
  std::vector<uint64_t> keys(cells, 0ull);   // (no device list: no columns, every row is padding)
  if (x->d_topk) {
    HIP_TRY(al, hipSetDevice(al->device));
    HIP_TRY(al, hipMemcpy(keys.data(), x->d_topk, cells * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  for (size_t c = 0; c < cells; ++c) {   // key 0 decodes to j = -1, score = INT32_MIN
    j[c] = (int32_t)~(uint32_t)keys[c];
    score[c] = (int32_t)((uint32_t)(keys[c] >> 32) ^ 0x80000000u);
  }
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_cross_dense(wfa_hip_cross_t* x, int32_t* score, int32_t* status) {
  if (!x) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = x->al;
  if (!(x->want & WFA_HIP_CROSS_DENSE)) return fail_inval(al, "the run was made without WFA_HIP_CROSS_DENSE");
  const size_t cells = (size_t)(x->m * x->n);
  if (cells == 0) return WFA_HIP_OK;
  if (!score || !status) return fail_inval(al, "score/status outputs are required");
  HIP_TRY(al, hipSetDevice(al->device));
  HIP_TRY(al, hipMemcpy(score, x->d_score, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(al, hipMemcpy(status, x->d_status, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_cross_completed(wfa_hip_cross_t* x, int64_t* count, int32_t* i, int32_t* j, int32_t* score) {
  if (!x || !count) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = x->al;
  if (!(x->want & WFA_HIP_CROSS_COMPLETED)) return fail_inval(al, "the run was made without WFA_HIP_CROSS_COMPLETED");
  *count = x->count;
  if (x->count == 0) return WFA_HIP_OK;
  HIP_TRY(al, hipSetDevice(al->device));
  const size_t bytes = (size_t)x->count * sizeof(int32_t);
  if (i) HIP_TRY(al, hipMemcpy(i, x->d_ci, bytes, hipMemcpyDeviceToHost));
  if (j) HIP_TRY(al, hipMemcpy(j, x->d_cj, bytes, hipMemcpyDeviceToHost));
  if (score) HIP_TRY(al, hipMemcpy(score, x->d_cs, bytes, hipMemcpyDeviceToHost));
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_cross_kernel_ms(wfa_hip_cross_t* x, float* ms, int64_t* pairs) {
  if (!x) return WFA_HIP_EINVAL;
  if (ms) *ms = (float)x->ms;
  if (pairs) *pairs = x->pairs;
  return WFA_HIP_OK;
}
