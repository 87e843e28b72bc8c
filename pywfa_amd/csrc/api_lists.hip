// api_lists.hip — list-built batches of libwfa_hip.so (the C ABI declared in include/wfa_hip.h).
#include "host_sets.hpp"
#include "wfa_cross.hpp"

// ------------------------------------------------------------------------------------------------
// list-built batches (include/wfa_hip.h; csrc/wfa_cross.hpp): indexed batches, a list of (i, j) index pairs over resident sequence
// sets (k_pairs.hip), and windowed batches, windows of resident sequences, either strand, by index (k_windows.hip)
// ------------------------------------------------------------------------------------------------
namespace {   // (the descriptors' members: internal, so that none of them is exported)

// What a descriptor (IndexedPairs, WindowPairs below) tells batch_build_list about the pair at one list position
struct ListPair {
  int pl = 0, tl = 0;       // the lengths of what is aligned
  int gen_words = 0;        // the words one lane group of the generator covers for it
  bool slot = true;         // it has a word slot (otherwise it points into the sets' words, copied in front of the slots)
  bool bytes = false;       // it is aligned on its bytes
  bool opt = false;         // the descriptor recorded an option for it
  int64_t byte_slot = 0;    // a byte pair's byte slot, where the descriptor has byte slots
};

// ... and what batch_build_list tells the descriptor, once the list is laid out and the batch's common blocks are allocated
struct ListPlan {
  bool all_bytes, lists, any_long, any_opt;
  uint64_t table_words;     // words in front of the slots
  int64_t slot_bytes;
  int log2g;                // lanes per pair of the generator: the largest gen_words, rounded up to a power of two (at most a whole wave)
  const std::vector<uint32_t>& chunk_base;
  const std::vector<int64_t>& chunk_bbase;
};

// does [start, start + len) of sequence k of the set touch a run of flagged letters?
static inline bool window_flagged(const wfa_hip_seqset* S, size_t k, int32_t start, int32_t len) {
  if (!S->h_flag[k] || len <= 0) return false;
  const std::vector<int32_t>& r = S->h_runs[k];
  size_t lo = 0, hi = r.size() / 2;   // the first run that ends behind `start`
  while (lo < hi) { const size_t mid = (lo + hi) / 2; if (r[2 * mid + 1] > start) hi = mid; else lo = mid + 1; }
  return lo < r.size() / 2 && r[2 * lo] < start + len;
}

// Index pairs: whole sequences.  A pair of up to WFA_FAST_MAX_LEN bases gets a word slot, a longer one points into the sets' words; a
// pair is a byte pair when one of its sequences is flagged.  The batch owns all it reads afterwards: the slots, and copies (device to
// device) of the sets' words when a listed pair is too long for a slot, of their bytes when a listed pair is aligned on its bytes —
// so it outlives the sets.
struct IndexedPairs {
  const wfa_hip_seqset *P, *T;
  bool same;
  const int32_t *i, *j;
  static constexpr bool byte_slots = false;
  static constexpr const char* too_large = "indexed batch too large: more than 2^32 words of sets and slots (split the list)";

  __attribute__((always_inline)) void get(int64_t q, bool all_bytes, ListPair* p) const {
    const size_t a = (size_t)i[q], bq = (size_t)j[q];
    p->pl = P->h_len[a]; p->tl = T->h_len[bq];
    p->slot = p->pl <= WFA_FAST_MAX_LEN && p->tl <= WFA_FAST_MAX_LEN;
    p->gen_words = p->slot ? ((p->pl + 15) >> 4) + ((p->tl + 15) >> 4) : 0;   // (the longest slot)
    p->bytes = all_bytes || P->h_flag[a] || T->h_flag[bq];
  }
  __attribute__((always_inline)) int check(int64_t q, bool all_bytes, ListPair* p) const { get(q, all_bytes, p); return 0; }   // (indices in range: nothing else to refuse)
  int refuse(wfa_hip_aligner* al, int, int64_t) const { return fail_inval(al, "%s", ""); }
  // the sets' words and 64 zero words, only when a listed pair points into them
  uint64_t table_words(bool any_long) const { return any_long ? P->nwords + (same ? 0 : T->nwords) + 64 : 0; }
  // byte pairs: the sets' bytes, the text set's behind the pattern set's
  int byte_store(wfa_hip_aligner* al, wfa_hip_batch* b, const ListPlan&) const {
    HIP_TRY(al, pool_alloc(al, (void**)&b->d_bytes, (size_t)(P->nbytes + (same ? 0 : T->nbytes) + 64)));
    return copy_sets(al, b->d_bytes, P->d_bytes, (size_t)P->nbytes, T->d_bytes, (size_t)T->nbytes, same, 64);
  }
  int generate(wfa_hip_aligner* al, wfa_hip_batch* b, StreamScratch& sc, const ListPlan& plan) const {
    const int64_t n = b->n;
    if (plan.any_long) {
      if (copy_sets(al, b->d_words, P->d_words, (size_t)P->nwords, T->d_words, (size_t)T->nwords, same, 0)) return WFA_HIP_EDEVICE;
      HIP_TRY(al, hipMemsetAsync(b->d_words + (plan.table_words - 64), 0, 64 * sizeof(uint32_t), al->stream));
    }
    int32_t *d_i = nullptr, *d_j = nullptr;
    uint32_t* d_chunk = nullptr;
    if (sc.upload(&d_i, i, (size_t)n) || sc.upload(&d_j, j, (size_t)n) || sc.upload(&d_chunk, plan.chunk_base.data(), plan.chunk_base.size())) return WFA_HIP_EDEVICE;
    wfa::PairsGenArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.p_words = P->d_words; ga.p_woff = P->d_woff; ga.p_len = P->d_len; ga.p_boff = P->d_boff; ga.p_flag = P->d_flag;
    ga.t_words = T->d_words; ga.t_woff = T->d_woff; ga.t_len = T->d_len; ga.t_boff = T->d_boff; ga.t_flag = T->d_flag;
    ga.i = d_i; ga.j = d_j; ga.chunk_base = d_chunk;
    ga.words = b->d_words; ga.t_wshift = same ? 0u : (uint32_t)P->nwords; ga.t_bshift = same ? 0 : P->nbytes; ga.npairs = n;
    ga.log2g = plan.log2g;
    ga.all_bytes = plan.all_bytes ? 1 : 0; ga.lists = plan.lists ? 1 : 0;
    ga.meta = b->d_meta; ga.pboff = b->d_pboff; ga.tboff = b->d_tboff; ga.flags = b->d_flags;
    if (wfa::launch_pairs_gen(ga, al->cu_count, al->stream) != 0) { al->err = "indexed batch generator launch failed"; return WFA_HIP_EDEVICE; }
    return WFA_HIP_OK;
  }
};

// Windows: every pair has a word slot, a byte pair a byte slot, and whether a pair is a byte pair is looked up per window in the sets'
// runs of flagged letters.  One byte of options per pair (strand, byte pair) goes to the device when the list has a reversed or a byte
// pair; the batch owns its slots and nothing of the sets.
struct WindowPairs {
  const wfa_hip_seqset *P, *T;
  const int32_t *i, *j, *p_start, *p_len, *t_start, *t_len;
  const uint8_t* reverse;
  std::vector<uint8_t> opt;   // per pair: written by check, read by get
  static constexpr bool byte_slots = true;
  static constexpr const char* too_large = "windowed batch too large: more than 2^32 words of slots (split the list)";

  struct Win { int64_t ps, pl, ts, tl; };
  Win window(int64_t q, int64_t pseq, int64_t tseq) const {
    Win w;
    w.ps = p_start ? p_start[q] : 0; w.ts = t_start ? t_start[q] : 0;
    w.pl = p_len ? p_len[q] : pseq - w.ps; w.tl = t_len ? t_len[q] : tseq - w.ts;
    return w;
  }
  static void fill(ListPair* p, int pl, int tl, bool byt) {
    p->pl = pl; p->tl = tl; p->bytes = byt;
    p->gen_words = std::max((pl + 15) >> 4, (tl + 15) >> 4);   // (the longest window)
    p->byte_slot = byt ? (((int64_t)pl + 3) & ~(int64_t)3) + (((int64_t)tl + 3) & ~(int64_t)3) : 0;
  }
  __attribute__((always_inline)) int check(int64_t q, bool all_bytes, ListPair* p) {
    const size_t a = (size_t)i[q], bq = (size_t)j[q];
    const int64_t pseq = P->h_len[a], tseq = T->h_len[bq];
    const Win w = window(q, pseq, tseq);
    if (w.ps < 0 || w.ts < 0 || (p_len && w.pl < 0) || (t_len && w.tl < 0)) return 2;
    if (w.ps + w.pl > pseq || w.ts + w.tl > tseq || w.pl < 0 || w.tl < 0) return 4;
    const int pl = (int)w.pl, tl = (int)w.tl;
    const bool rev = reverse && reverse[q] != 0;
    const bool byt = all_bytes || window_flagged(P, a, (int32_t)w.ps, pl) || window_flagged(T, bq, (int32_t)w.ts, tl);
    opt[(size_t)q] = (uint8_t)((rev ? WFA_WIN_REVERSE : 0) | (byt ? WFA_WIN_BYTES : 0));
    fill(p, pl, tl, byt);
    p->opt = rev || byt;
    return 0;
  }
  __attribute__((always_inline)) void get(int64_t q, bool, ListPair* p) const {
    const Win w = window(q, P->h_len[(size_t)i[q]], T->h_len[(size_t)j[q]]);
    fill(p, (int)w.pl, (int)w.tl, (opt[(size_t)q] & WFA_WIN_BYTES) != 0);
  }
  int refuse(wfa_hip_aligner* al, int err, int64_t q) const {
    const int64_t pseq = P->h_len[(size_t)i[q]], tseq = T->h_len[(size_t)j[q]];
    const Win w = window(q, pseq, tseq);
    return fail_inval(al, "%s at position %lld of the pair list: pattern window [%lld, %lld + %lld) of sequence %d (%lld bases), "
                      "text window [%lld, %lld + %lld) of sequence %d (%lld bases)", err == 2 ? "negative start or length" : "window out of range",
                      (long long)q, (long long)w.ps, (long long)w.ps, (long long)w.pl, (int)i[q], (long long)pseq,
                      (long long)w.ts, (long long)w.ts, (long long)w.tl, (int)j[q], (long long)tseq);
  }
  uint64_t table_words(bool) const { return 0; }
  // byte pairs: their byte slots and 64 zero bytes
  int byte_store(wfa_hip_aligner* al, wfa_hip_batch* b, const ListPlan& plan) const {
    HIP_TRY(al, pool_alloc(al, (void**)&b->d_bytes, (size_t)plan.slot_bytes + 64));
    HIP_TRY(al, hipMemsetAsync(b->d_bytes + plan.slot_bytes, 0, 64, al->stream));
    return WFA_HIP_OK;
  }
  int generate(wfa_hip_aligner* al, wfa_hip_batch* b, StreamScratch& sc, const ListPlan& plan) const {
    const int64_t n = b->n;
    int32_t* d_arr[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint8_t* d_opt = nullptr;
    uint32_t* d_chunk = nullptr;
    int64_t* d_bchunk = nullptr;
    if (plan.lists && sc.upload(&d_bchunk, plan.chunk_bbase.data(), plan.chunk_bbase.size())) return WFA_HIP_EDEVICE;
    const int32_t* h_arr[6] = {i, j, p_start, p_len, t_start, t_len};
    for (int k = 0; k < 6; ++k)
      if (sc.upload_opt(&d_arr[k], h_arr[k], (size_t)n)) return WFA_HIP_EDEVICE;
    if (plan.any_opt && sc.upload(&d_opt, opt.data(), (size_t)n)) return WFA_HIP_EDEVICE;
    if (sc.upload(&d_chunk, plan.chunk_base.data(), plan.chunk_base.size())) return WFA_HIP_EDEVICE;
    wfa::WindowsGenArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.p_words = P->d_words; ga.p_woff = P->d_woff; ga.p_len = P->d_len; ga.p_boff = P->d_boff; ga.p_bytes = P->d_bytes;
    ga.t_words = T->d_words; ga.t_woff = T->d_woff; ga.t_len = T->d_len; ga.t_boff = T->d_boff; ga.t_bytes = T->d_bytes;
    ga.i = d_arr[0]; ga.j = d_arr[1]; ga.p_start = d_arr[2]; ga.p_wlen = d_arr[3]; ga.t_start = d_arr[4]; ga.t_wlen = d_arr[5];
    ga.opt = d_opt; ga.chunk_base = d_chunk; ga.chunk_bbase = d_bchunk;
    ga.words = b->d_words; ga.bytes = b->d_bytes; ga.npairs = n;
    ga.log2g = plan.log2g;
    ga.all_bytes = plan.all_bytes ? 1 : 0; ga.lists = plan.lists ? 1 : 0;
    ga.meta = b->d_meta; ga.pboff = b->d_pboff; ga.tboff = b->d_tboff; ga.flags = b->d_flags;
    if (wfa::launch_windows_gen(ga, al->cu_count, al->stream) != 0) { al->err = "windowed batch generator launch failed"; return WFA_HIP_EDEVICE; }
    return WFA_HIP_OK;
  }
};

}  // namespace

// What batch_build does for an explicit batch, from the sets' host tables instead of the caller's arrays: one pass over the list checks
// and sums (on threads for long lists; the parts start on chunk boundaries of the generator), a second writes what the host keeps (the
// op-region prefix, the lengths, the work lists) and the generator's chunk bases.  The generator then writes the metadata and the slots
// on the device.  How a listed pair is described, what stands in front of the slots, where a byte pair's bytes are and the generator
// itself are the descriptor's (IndexedPairs, WindowPairs); its per-pair calls inline into the two passes.
template <class Desc>
static int batch_build_list(wfa_hip_aligner* al, wfa_hip_batch* b, int64_t n, Desc& D) {
  batch_adopt_config(al, b);
  const wfa_hip_config_t& c = b->cfg;
  const bool all_bytes = c.wildcard >= 0 && b->wild < 0;   // (a wildcard among ACGT: every pair on its bytes)
  b->al = al;
  b->n = n;
  const bool full = (c.scope == WFA_SCOPE_FULL);
  const int64_t np_set = D.P->n, nt_set = D.T->n;
  const int nthr = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, std::thread::hardware_concurrency()), n / 65536));
  auto part_lo = [&](int t) -> int64_t { return t >= nthr ? n : (n * t / nthr) & ~(int64_t)(WFA_PAIRS_CHUNK - 1); };
  struct Part {
    uint64_t words = 0; int64_t packed = 0, ops = 0, nbytes = 0, slot_bytes = 0, bad = -1;
    int max_width = 0, max_len = 0, max_gen = 0, err = 0; bool any_long = false, any_opt = false;
  };
  std::vector<Part> parts((size_t)nthr);
  auto pass1 = [&](int t) {
    Part& pt = parts[(size_t)t];
    for (int64_t q = part_lo(t), hi = part_lo(t + 1); q < hi; ++q) {
      const int64_t a = D.i[q], bq = D.j[q];
      if (a < 0 || a >= np_set || bq < 0 || bq >= nt_set) { pt.err = 1; pt.bad = q; return; }
      ListPair p;
      if (const int bad = D.check(q, all_bytes, &p)) { pt.err = bad; pt.bad = q; return; }
      const int pl = p.pl, tl = p.tl;
      // wavefront_align.c:86-102, per listed pair as batch_build: against what is aligned (the sequences, or the windows)
      if (free_ends_exceed(c, pl, tl)) { pt.err = PART_ENDS_FREE; pt.bad = q; return; }
      if (p.slot) pt.words += (uint64_t)(((pl + 15) >> 4) + ((tl + 15) >> 4));
      else pt.any_long = true;
      pt.max_gen = std::max(pt.max_gen, p.gen_words);
      pt.max_width = std::max(pt.max_width, pl + tl + 3);
      pt.max_len = std::max(pt.max_len, std::max(pl, tl));
      pt.packed += (int64_t)((pl + 3) >> 2) + ((tl + 3) >> 2);
      pt.ops += (int64_t)pl + tl;
      if (p.bytes) { pt.nbytes += 1; pt.slot_bytes += p.byte_slot; }
      pt.any_opt |= p.opt;
    }
  };
  run_parts(nthr, nthr, pass1);   // (a thread per part)
  uint64_t slot_words = 0;
  int64_t nbytes = 0, slot_bytes = 0;
  int max_gen = 0;
  bool any_long = false, any_opt = false;
  std::vector<uint64_t> wbase((size_t)nthr);
  std::vector<int64_t> obase((size_t)nthr), bbase((size_t)nthr), sbase((size_t)nthr);
  for (int t = 0; t < nthr; ++t) {
    const Part& pt = parts[(size_t)t];
    if (pt.err == 1)
      return fail_inval(al, "index out of range at position %lld of the pair list: (%d, %d) over sets of %lld and %lld sequences",
                        (long long)pt.bad, (int)D.i[pt.bad], (int)D.j[pt.bad], (long long)np_set, (long long)nt_set);
    if (pt.err == PART_ENDS_FREE) return fail_inval(al, "%s", part_error_message(pt.err));
    if (pt.err) return D.refuse(al, pt.err, pt.bad);
    wbase[(size_t)t] = slot_words; obase[(size_t)t] = b->ops_bytes; bbase[(size_t)t] = nbytes; sbase[(size_t)t] = slot_bytes;
    slot_words += pt.words; nbytes += pt.nbytes; slot_bytes += pt.slot_bytes;
    max_gen = std::max(max_gen, pt.max_gen); any_long |= pt.any_long; any_opt |= pt.any_opt;
    b->max_width = std::max(b->max_width, pt.max_width); b->max_len = std::max(b->max_len, pt.max_len);
    b->packed_bytes += pt.packed; b->ops_bytes += pt.ops;
  }
  // the word table: what the descriptor puts in front, the slots, 64 zero words
  const uint64_t table_words = D.table_words(any_long);
  if (table_words + slot_words + 64 > 0xFFFFFFF0ull) return fail_inval(al, "%s", Desc::too_large);
  const bool lists = nbytes > 0;
  const int64_t chunks = (n + WFA_PAIRS_CHUNK - 1) / WFA_PAIRS_CHUNK;
  std::vector<uint32_t> chunk_base((size_t)std::max<int64_t>(chunks, 1), (uint32_t)table_words);
  std::vector<int64_t> chunk_bbase(lists && Desc::byte_slots ? (size_t)std::max<int64_t>(chunks, 1) : 0, 0);
  std::vector<uint32_t> lp(lists ? (size_t)(n - nbytes) : 0), lb(lists ? (size_t)nbytes : 0);
  if (full) {   // needed later to lay out the op-string regions
    b->h_plen.resize((size_t)n); b->h_tlen.resize((size_t)n);
    b->h_coff.assign((size_t)n + 1, 0);
  }
  auto pass2 = [&](int t) {
    uint64_t w = table_words + wbase[(size_t)t];
    int64_t o = obase[(size_t)t], nb = bbase[(size_t)t], sb = sbase[(size_t)t];
    const int64_t lo = part_lo(t), hi = part_lo(t + 1);
    int64_t npk = lo - nb;   // 2-bit pairs before this part
    for (int64_t q = lo; q < hi; ++q) {
      ListPair p;
      D.get(q, all_bytes, &p);
      const int pl = p.pl, tl = p.tl;
      if ((q & (WFA_PAIRS_CHUNK - 1)) == 0) {
        chunk_base[(size_t)(q / WFA_PAIRS_CHUNK)] = (uint32_t)w;
        if (!chunk_bbase.empty()) chunk_bbase[(size_t)(q / WFA_PAIRS_CHUNK)] = sb;
      }
      if (p.slot) w += (uint64_t)(((pl + 15) >> 4) + ((tl + 15) >> 4));
      if (full) { b->h_plen[(size_t)q] = pl; b->h_tlen[(size_t)q] = tl; o += (int64_t)pl + tl; b->h_coff[(size_t)q + 1] = o; }
      if (lists) {
        if (p.bytes) { lb[(size_t)nb++] = (uint32_t)q; sb += p.byte_slot; }
        else lp[(size_t)npk++] = (uint32_t)q;
      }
    }
  };
  run_parts(nthr, nthr, pass2);
  StreamScratch sc{al};   // (declared behind the host tables above: it waits for the stream before they go)
  const size_t nn = (size_t)std::max<int64_t>(n, 1);
  { const int arc = batch_alloc_common(al, b, table_words + slot_words + 64, 64); if (arc != WFA_HIP_OK) return arc; }
  b->n_bytes = (uint32_t)nbytes;
  b->n_packed = (uint32_t)(n - nbytes);
  if (n > 0) {
    ListPlan plan{all_bytes, lists, any_long, any_opt, table_words, slot_bytes, 2, chunk_base, chunk_bbase};
    while (plan.log2g < 6 && (1 << plan.log2g) < max_gen) ++plan.log2g;
    if (lists) {   // (byte pairs: where their bytes are, the descriptor's; the two work lists, ascending)
      { const int src = D.byte_store(al, b, plan); if (src != WFA_HIP_OK) return src; }
      HIP_TRY(al, pool_alloc(al, (void**)&b->d_pboff, nn * sizeof(int64_t)));
      HIP_TRY(al, pool_alloc(al, (void**)&b->d_tboff, nn * sizeof(int64_t)));
      { const int lrc = upload_work_lists(al, b, lp, lb, true); if (lrc != WFA_HIP_OK) return lrc; }
    }
    { const int grc = D.generate(al, b, sc, plan); if (grc != WFA_HIP_OK) return grc; }
  }
  { const int frc = finish_batch_build(al, b); if (frc != WFA_HIP_OK) return frc; }
  // the caller's arrays, the host tables above and the sets are read by what is enqueued: over before this returns
  HIP_TRY(al, hipStreamSynchronize(al->stream));
  return WFA_HIP_OK;
}

// What both creators check before the build, in this order; the new batch, counted among the aligner's live ones, or nullptr with the
// reason in al->err and g_error.  *texts == nullptr: one set against itself.
static wfa_hip_batch* list_batch_new(wfa_hip_aligner* al, const wfa_hip_seqset* patterns, const wfa_hip_seqset** texts,
                                     int64_t npairs, const int32_t* i, const int32_t* j) {
  if (!al) return fail_create(al, "null aligner");
  if (!*texts) *texts = patterns;
  if (!patterns || patterns->al != al || (*texts)->al != al) return fail_create(al, "sequence set of another aligner");
  if (patterns->wildcard != al->cfg.wildcard || (*texts)->wildcard != al->cfg.wildcard)
    return fail_create(al, "sequence set packed under another wildcard: create it again");
  if (npairs < 0 || npairs > 0x7FFFFFF0ll || (npairs > 0 && (!i || !j))) return fail_create(al, "invalid pair list arguments");
  if (!create_begin(al)) return nullptr;
  mailbox_release(al);   // (the resident one-pair kernel: batches take the device)
  return batch_new(al);   // (the core's own adopt step)
}

extern "C" wfa_hip_batch_t* wfa_hip_batch_create_indexed(wfa_hip_aligner_t* al, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts,
                                                         int64_t npairs, const int32_t* i, const int32_t* j) {
  const bool same = (texts == nullptr);
  wfa_hip_batch* b = list_batch_new(al, patterns, &texts, npairs, i, j);
  if (!b) return nullptr;
  IndexedPairs D{patterns, texts, same, i, j};
  return create_done(al, b, batch_build_list(al, b, npairs, D), batch_free);
}

extern "C" int wfa_hip_window_2bit(const uint32_t* words, int64_t start, int32_t len, int reverse, uint32_t* out) {
  if (start < 0 || len < 0 || (len > 0 && (!words || !out))) return WFA_HIP_EINVAL;
  if (len == 0) return WFA_HIP_OK;
  const int64_t w_lo = start >> 4, w_hi = (start + len - 1) >> 4;   // the source words that hold a base of the window: nothing else is read
  const uint32_t n = (uint32_t)(len + 15) >> 4;
  for (uint32_t w = 0; w < n; ++w) {
    const int64_t first = wfa::wfa_window_first(start, len, w, reverse != 0), si = first >> 4;
    const uint32_t lo = (si >= w_lo && si <= w_hi) ? words[si] : 0u, hi = (si + 1 >= w_lo && si + 1 <= w_hi) ? words[si + 1] : 0u;
    out[w] = wfa::wfa_window_word(lo, hi, first, len, w, reverse != 0);
  }
  return WFA_HIP_OK;
}

extern "C" wfa_hip_batch_t* wfa_hip_batch_create_windows(wfa_hip_aligner_t* al, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts,
                                                         int64_t npairs, const int32_t* i, const int32_t* j,
                                                         const int32_t* p_start, const int32_t* p_len, const int32_t* t_start, const int32_t* t_len,
                                                         const uint8_t* reverse) {
  wfa_hip_batch* b = list_batch_new(al, patterns, &texts, npairs, i, j);
  if (!b) return nullptr;
  WindowPairs D{patterns, texts, i, j, p_start, p_len, t_start, t_len, reverse, std::vector<uint8_t>((size_t)npairs, 0)};
  return create_done(al, b, batch_build_list(al, b, npairs, D), batch_free);
}
