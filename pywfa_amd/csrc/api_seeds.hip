// api_seeds.hip — the seed index and chains of libwfa_hip.so (the C ABI declared in include/wfa_hip.h).
#include "host_sets.hpp"
#include "wfa_chain.hpp"

// ------------------------------------------------------------------------------------------------
// seed finder: a k-mer index over a text set, candidate windows per read (include/wfa_hip.h; csrc/wfa_seed.hpp, k_seed.hip)
// ------------------------------------------------------------------------------------------------
static_assert(WFA_SEED_MAX_N == WFA_HIP_SEED_MAX_N && WFA_SEED_MAX_HITS == WFA_HIP_SEED_MAX_HITS, "bounds of the kernels and of the ABI");
static_assert(WFA_SEED_MAX_W == WFA_HIP_MINIMIZER_MAX_W, "bounds of the minimizer kernels and of the ABI");
static_assert(WFA_CHAIN_MAX_LOOKBACK == WFA_HIP_CHAIN_MAX_LOOKBACK && WFA_CHAIN_MAX_ANCHORS == WFA_HIP_CHAIN_MAX_ANCHORS, "bounds of the chain kernel and of the ABI");

namespace wfa {   // host_seed.cpp: the parameter checks shared with wfa_hip_seeds_host
int seed_check_index(int k, int stride, int max_occ, char* msg, size_t cap);
int seed_check_minimizer(int k, int w, int max_occ, char* msg, size_t cap);
int seed_check_query(int n, int min_hits, int gap, int pad, int max_hits, char* msg, size_t cap);
// host_chain.cpp: the check shared with wfa_hip_chains_host
int seed_check_chain(int n, int min_hits, int min_score, int lookback, int max_dist, int band, int pad, int max_anchors, char* msg, size_t cap);
}

struct wfa_hip_seed_index {
  wfa_hip_aligner* al = nullptr;
  int k = 0, stride = 0, max_occ = 0;
  int w = 0;                          // 0: a stride index; 1 .. 32: a minimizer index (stride = 1)
  int64_t nseq = 0;
  uint32_t* d_table = nullptr;        // 4^k + 1 bucket starts (its own allocation: 4^k * 4 bytes)
  wfa::SeedRec* d_recs = nullptr;     // {j, t} per indexed position, in bucket order (its own allocation)
  int32_t* d_len = nullptr;           // the texts' lengths
  int64_t positions = 0, masked = 0, table_bytes = 0;
  float build_ms = 0.f, query_ms = 0.f;
  int32_t* d_chain_ws = nullptr;      // the chaining workspace: a slab per workgroup of the last launch (its own allocation, grown on demand)
  size_t chain_ws_bytes = 0;
  float chain_ms = 0.f;
};

// The letters outside ACGT of a set as the seed kernels read them: bit b of mask[w] = base 16 (w - woff) + b of the word's sequence,
// from the runs the set keeps on the host; uploaded on the first call, nullptr when no sequence of the set is flagged.
static int seqset_mask(wfa_hip_aligner* al, const wfa_hip_seqset* S, const uint16_t** out) {
  *out = S->d_mask;
  if (S->d_mask || std::find(S->h_flag.begin(), S->h_flag.end(), (uint8_t)1) == S->h_flag.end()) return WFA_HIP_OK;
  std::vector<uint16_t> mask((size_t)S->nwords + 4, 0);
  uint64_t w = 0;
  for (int64_t q = 0; q < S->n; ++q) {
    const std::vector<int32_t>& r = S->h_runs[(size_t)q];
    for (size_t x = 0; x + 1 < r.size(); x += 2)
      for (int32_t p = r[x]; p < r[x + 1]; ++p) mask[(size_t)w + ((size_t)p >> 4)] |= (uint16_t)(1u << (p & 15));
    w += (uint64_t)((S->h_len[(size_t)q] + 15) >> 4);
  }
  uint16_t* d = nullptr;
  HIP_TRY(al, pool_alloc(al, (void**)&d, mask.size() * sizeof(uint16_t)));
  const hipError_t e = hipMemcpy(d, mask.data(), mask.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) { pool_release(al, d); HIP_TRY(al, e); }
  S->d_mask = d;
  *out = d;
  return WFA_HIP_OK;
}

static wfa::SeedSetView seed_view(const wfa_hip_seqset* S, const uint16_t* mask) {
  wfa::SeedSetView v;
  v.words = S->d_words; v.mask = mask; v.woff = S->d_woff; v.len = S->d_len; v.nseq = S->n; v.nwords = S->nwords;
  return v;
}

extern "C" void wfa_hip_seed_index_destroy(wfa_hip_seed_index_t* x) {
  if (!x) return;
  wfa_hip_aligner* al = x->al;
  (void)hipSetDevice(al->device);
  if (x->d_table) (void)hipFree(x->d_table);
  if (x->d_recs) (void)hipFree(x->d_recs);
  if (x->d_chain_ws) (void)hipFree(x->d_chain_ws);
  pool_release(al, x->d_len);
  destroy_end(x);
}

static int seed_index_build(wfa_hip_aligner* al, wfa_hip_seed_index* x, const wfa_hip_seqset* T) {
  x->nseq = T->n;
  uint64_t cap = 0;   // the positions the stride takes of sequences without a flagged letter: at least the indexed ones
  for (int32_t len : T->h_len)
    if (len >= x->k) cap += (uint64_t)((len - x->k) / x->stride + 1);
  const uint64_t buckets = 1ull << (2 * x->k);
  const size_t table_bytes = (size_t)(buckets + 1) * sizeof(uint32_t), rec_bytes = (size_t)std::max<uint64_t>(cap, 1) * sizeof(wfa::SeedRec);
  if (hipMalloc((void**)&x->d_table, table_bytes) != hipSuccess)
    return fail_alloc(al, (void**)&x->d_table, "seed index table: hipMalloc of %zu bytes failed (4 bytes per k-mer of k = %d: 4^k buckets)", table_bytes, x->k);
  const auto alloc_recs = [&](size_t bytes, uint64_t positions) {
    if (hipMalloc((void**)&x->d_recs, bytes) == hipSuccess) { HIP_TRY(al, poison_fill(al, x->d_recs, bytes, al->stream)); return WFA_HIP_OK; }
    return fail_alloc(al, (void**)&x->d_recs, "seed index records: hipMalloc of %zu bytes failed (8 bytes per indexed position, %llu positions)", bytes,
                      (unsigned long long)positions);
  };
  HIP_TRY(al, poison_fill(al, x->d_table, table_bytes, al->stream));
  if (x->w == 0 && alloc_recs(rec_bytes, cap)) return WFA_HIP_EDEVICE;   // (a minimizer index: after the counting pass, by its total)
  x->table_bytes = (int64_t)(table_bytes + rec_bytes);
  const uint16_t* mask = nullptr;
  if (seqset_mask(al, T, &mask) != WFA_HIP_OK) return WFA_HIP_EDEVICE;
  StreamScratch sc{al};
  uint32_t *d_bsum = nullptr, *d_masked = nullptr;
  if (sc.alloc(&d_bsum, (size_t)((buckets + 1 + WFA_SEED_SCAN_CHUNK - 1) / WFA_SEED_SCAN_CHUNK)) || sc.alloc(&d_masked, 1)) return WFA_HIP_EDEVICE;
  HIP_TRY(al, pool_alloc(al, (void**)&x->d_len, (size_t)T->n * sizeof(int32_t)));
  HIP_TRY(al, hipMemcpyAsync(x->d_len, T->d_len, (size_t)T->n * sizeof(int32_t), hipMemcpyDeviceToDevice, al->stream));
  HIP_TRY(al, hipEventCreate(&sc.ev[0]));
  HIP_TRY(al, hipEventCreate(&sc.ev[1]));
  wfa::SeedBuildArgs a;
  memset(&a, 0, sizeof(a));
  a.t = seed_view(T, mask);
  a.k = x->k; a.stride = x->stride; a.w = x->w; a.max_occ = (uint32_t)x->max_occ;
  a.table = x->d_table; a.recs = x->d_recs; a.bsum = d_bsum; a.masked = d_masked;
  HIP_TRY(al, hipEventRecord(sc.ev[0], al->stream));
  HIP_TRY(al, hipMemsetAsync(x->d_table, 0, table_bytes, al->stream));
  HIP_TRY(al, hipMemsetAsync(d_masked, 0, sizeof(uint32_t), al->stream));
  int lrc = wfa::launch_seed_count(a, al->stream) | wfa::launch_seed_scan(a, al->stream);
  uint32_t total = 0, masked = 0;
  if (x->w >= 1 && lrc == 0) {
    // the records by the count: the scan has left the total behind the last bucket
    if (sc.download(&total, x->d_table + buckets, 1)) return WFA_HIP_EDEVICE;
    HIP_TRY(al, hipStreamSynchronize(al->stream));
    cap = total;
    const size_t bytes = (size_t)std::max<uint64_t>(cap, 1) * sizeof(wfa::SeedRec);
    if (alloc_recs(bytes, cap)) return WFA_HIP_EDEVICE;
    x->table_bytes = (int64_t)(table_bytes + bytes);
    a.recs = x->d_recs;
  }
  lrc |= wfa::launch_seed_fill(a, (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull), al->stream);
  HIP_TRY(al, hipEventRecord(sc.ev[1], al->stream));
  if (sc.download(&total, x->d_table + buckets, 1) || sc.download(&masked, d_masked, 1)) return WFA_HIP_EDEVICE;
  { const int erc = launch_end(al, nullptr, lrc, "seed index kernel launch failed"); if (erc != WFA_HIP_OK) return erc; }
  HIP_TRY(al, hipEventElapsedTime(&x->build_ms, sc.ev[0], sc.ev[1]));
  x->positions = total; x->masked = masked;
  return WFA_HIP_OK;
}

// the one body of both creates; minimizer: w is the window and stride plays no part, otherwise w = 0
static wfa_hip_seed_index_t* seed_index_create(wfa_hip_aligner_t* al, const wfa_hip_seqset_t* texts, int k, int stride, int w, int max_occ, bool minimizer) {
  if (!al) return fail_create(al, "null aligner");
  if (!texts || texts->al != al) return fail_create(al, "seed index: sequence set of another aligner");
  const int crc = minimizer ? check_inval(al, wfa::seed_check_minimizer, k, w, max_occ) : check_inval(al, wfa::seed_check_index, k, stride, max_occ);
  if (crc != WFA_HIP_OK) { g_error = al->err; return nullptr; }
  if (texts->n == 0) return fail_create(al, "seed index: texts = a set of 0 sequences is out of range (at least 1)");
  if (texts->nbytes >= (1ll << 31))
    return fail_create(al, "seed index: texts = a set of %lld bases is out of range (below 2^31: split the set)", (long long)texts->nbytes);
  if (!create_begin(al)) return nullptr;
  mailbox_release(al);   // (the resident one-pair kernel: the build takes the device)
  wfa_hip_seed_index* x = create_adopt(al, new wfa_hip_seed_index());
  x->k = k; x->stride = stride; x->w = w; x->max_occ = max_occ;
  return create_done(al, x, seed_index_build(al, x, texts), wfa_hip_seed_index_destroy);
}

extern "C" wfa_hip_seed_index_t* wfa_hip_seed_index_create(wfa_hip_aligner_t* al, const wfa_hip_seqset_t* texts, int k, int stride, int max_occ) {
  return seed_index_create(al, texts, k, stride, 0, max_occ, false);
}

extern "C" wfa_hip_seed_index_t* wfa_hip_seed_index_create_minimizer(wfa_hip_aligner_t* al, const wfa_hip_seqset_t* texts, int k, int w, int max_occ) {
  return seed_index_create(al, texts, k, 1, w, max_occ, true);
}

extern "C" int wfa_hip_seed_index_params(const wfa_hip_seed_index_t* x, int* k, int* stride, int* w) {
  if (!x) return WFA_HIP_EINVAL;
  if (k) *k = x->k;
  if (stride) *stride = x->stride;
  if (w) *w = x->w;
  return WFA_HIP_OK;
}

// What a query and a chain run share: the reads' mask, then a block of `ncols` int32 columns of P->n x n cells and a byte per read in the
// scratch, two events round the launch, and the columns back to the caller's arrays.  Only the argument struct and the launch differ.
namespace {   // (internal: none of its members is exported)
struct SeedRows {
  wfa_hip_seed_index* x; const wfa_hip_seqset* P; int n;
  StreamScratch sc;
  const uint16_t* mask = nullptr;
  size_t cells = 0;
  int32_t* d_rows = nullptr;
  uint8_t* d_over = nullptr;
  int begin() {
    wfa_hip_aligner* al = sc.al;
    HIP_TRY(al, hipSetDevice(al->device));
    mailbox_release(al);
    return seqset_mask(al, P, &mask) != WFA_HIP_OK ? WFA_HIP_EDEVICE : WFA_HIP_OK;
  }
  // the blocks and the events; *a zeroed, then what SeedQueryArgs and ChainArgs have in common (the first five columns among it)
  template <class Args> int rows(int ncols, Args* a) {
    wfa_hip_aligner* al = sc.al;
    cells = (size_t)P->n * (size_t)n;
    if (sc.alloc(&d_rows, (size_t)ncols * cells) || sc.alloc(&d_over, (size_t)P->n)) return WFA_HIP_EDEVICE;
    HIP_TRY(al, hipEventCreate(&sc.ev[0]));
    HIP_TRY(al, hipEventCreate(&sc.ev[1]));
    memset(a, 0, sizeof(*a));
    a->p = seed_view(P, mask);
    a->table = x->d_table; a->recs = x->d_recs; a->t_len = x->d_len; a->t_nseq = x->nseq;
    a->k = x->k; a->w = x->w; a->max_occ = (uint32_t)x->max_occ;
    a->n = n;
    a->j = d_rows; a->reverse = d_rows + cells; a->text_start = d_rows + 2 * cells; a->text_len = d_rows + 3 * cells; a->hits = d_rows + 4 * cells;
    a->overflow = d_over;
    return WFA_HIP_OK;
  }
  // behind the launch: the second event, the downloads, the stream synchronised, the launch's outcome, the kernel's time
  int finish(int lrc, int ncols, int32_t* const* host, uint8_t* overflow, float* ms, const char* failed) {
    wfa_hip_aligner* al = sc.al;
    HIP_TRY(al, hipEventRecord(sc.ev[1], al->stream));
    if (sc.download_columns(host, ncols, d_rows, cells) || sc.download(overflow, d_over, (size_t)P->n)) return WFA_HIP_EDEVICE;
    const int rc = launch_end(al, nullptr, lrc, failed);
    if (rc != WFA_HIP_OK) return rc;
    HIP_TRY(al, hipEventElapsedTime(ms, sc.ev[0], sc.ev[1]));
    return WFA_HIP_OK;
  }
};
}  // namespace

extern "C" int wfa_hip_seed_index_query(wfa_hip_seed_index_t* x, const wfa_hip_seqset_t* P, int n, int min_hits, int gap, int pad, int max_hits,
                                        int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits, uint8_t* overflow) {
  if (!x) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = x->al;
  if (!P || P->al != al) return fail_inval(al, "seed query: sequence set of another aligner");
  if (check_inval(al, wfa::seed_check_query, n, min_hits, gap, pad, max_hits)) return WFA_HIP_EINVAL;
  if (P->n == 0) return WFA_HIP_OK;
  if (!j || !reverse || !text_start || !text_len || !hits || !overflow) return fail_inval(al, "seed query: a result array is missing");
  SeedRows r{x, P, n, StreamScratch{al}};
  wfa::SeedQueryArgs a;
  if (r.begin() || r.rows(5, &a)) return WFA_HIP_EDEVICE;
  a.min_hits = min_hits; a.max_hits = max_hits; a.gap = (uint32_t)gap; a.pad = pad;
  HIP_TRY(al, hipEventRecord(r.sc.ev[0], al->stream));
  const int lrc = wfa::launch_seed_query(a, P->n, al->cu_count, al->stream);
  int32_t* host[5] = {j, reverse, text_start, text_len, hits};
  return r.finish(lrc, 5, host, overflow, &x->query_ms, "seed query kernel launch failed");
}

extern "C" int wfa_hip_seed_index_stats(const wfa_hip_seed_index_t* x, int64_t* positions, int64_t* masked_kmers, int64_t* table_bytes,
                                        float* build_ms, float* query_ms) {
  if (!x) return WFA_HIP_EINVAL;
  if (positions) *positions = x->positions;
  if (masked_kmers) *masked_kmers = x->masked;
  if (table_bytes) *table_bytes = x->table_bytes;
  if (build_ms) *build_ms = x->build_ms;
  if (query_ms) *query_ms = x->query_ms;
  return WFA_HIP_OK;
}

// chains: the anchors of every read chained along the read, the best chains as windows (include/wfa_hip.h "chains"; csrc/wfa_chain.hpp)
extern "C" int wfa_hip_seed_index_chain(wfa_hip_seed_index_t* x, const wfa_hip_seqset_t* P, int n, int min_hits, int min_score, int lookback,
                                        int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse, int32_t* text_start,
                                        int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start, int32_t* pattern_len,
                                        uint8_t* overflow) {
  if (!x) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = x->al;
  if (!P || P->al != al) return fail_inval(al, "seed chain: sequence set of another aligner");
  if (check_inval(al, wfa::seed_check_chain, n, min_hits, min_score, lookback, max_dist, band, pad, max_anchors)) return WFA_HIP_EINVAL;
  const int64_t m = P->n;
  if (m == 0) return WFA_HIP_OK;
  if (!j || !reverse || !text_start || !text_len || !hits || !score || !pattern_start || !pattern_len || !overflow)
    return fail_inval(al, "seed chain: a result array is missing");
  SeedRows r{x, P, n, StreamScratch{al}};
  if (r.begin()) return WFA_HIP_EDEVICE;
  // the workspace: a slab of WFA_CHAIN_PLANES x max_anchors int32 per workgroup of this launch
  const unsigned grid = wfa::chain_grid(m, al->cu_count);
  const size_t ws_bytes = (size_t)grid * WFA_CHAIN_PLANES * (size_t)max_anchors * sizeof(int32_t);
  if (ws_bytes > x->chain_ws_bytes) {
    HIP_TRY(al, hipStreamSynchronize(al->stream));
    if (x->d_chain_ws) (void)hipFree(x->d_chain_ws);
    x->d_chain_ws = nullptr;
    x->chain_ws_bytes = 0;
    if (hipMalloc((void**)&x->d_chain_ws, ws_bytes) != hipSuccess)
      return fail_alloc(al, (void**)&x->d_chain_ws, "seed chain workspace: hipMalloc of %zu bytes failed (32 bytes x max_anchors = %d per workgroup, %u workgroups)",
                        ws_bytes, max_anchors, grid);
    x->chain_ws_bytes = ws_bytes;
    HIP_TRY(al, poison_fill(al, x->d_chain_ws, ws_bytes, al->stream));
  }
  wfa::ChainArgs a;
  if (r.rows(8, &a)) return WFA_HIP_EDEVICE;
  a.min_hits = min_hits; a.min_score = min_score; a.lookback = lookback; a.max_dist = max_dist; a.band = band; a.pad = pad;
  a.max_anchors = (uint32_t)max_anchors;
  a.slab = x->d_chain_ws;
  a.score = r.d_rows + 5 * r.cells; a.pattern_start = r.d_rows + 6 * r.cells; a.pattern_len = r.d_rows + 7 * r.cells;
  HIP_TRY(al, hipEventRecord(r.sc.ev[0], al->stream));
  const int lrc = wfa::launch_chain(a, m, grid, al->stream);
  int32_t* host[8] = {j, reverse, text_start, text_len, hits, score, pattern_start, pattern_len};
  return r.finish(lrc, 8, host, overflow, &x->chain_ms, "seed chain kernel launch failed");
}

extern "C" int wfa_hip_seed_index_chain_stats(const wfa_hip_seed_index_t* x, float* kernel_ms, int64_t* workspace_bytes) {
  if (!x) return WFA_HIP_EINVAL;
  if (kernel_ms) *kernel_ms = x->chain_ms;
  if (workspace_bytes) *workspace_bytes = (int64_t)x->chain_ws_bytes;
  return WFA_HIP_OK;
}
