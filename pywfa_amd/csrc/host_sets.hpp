// host_sets.hpp — the resident sequence set as the units built on it see it (api_*.hip; the core, wfa_hip.hip, knows nothing of sets),
// and what every resident handle's create, destroy, uploads and downloads share.
#pragma once
#include "host_core.hpp"

#pragma GCC visibility push(hidden)

struct wfa_hip_seqset {
  wfa_hip_aligner* al = nullptr;
  int64_t n = 0;
  int wildcard = -1;               // the aligner's wildcard when the set was packed
  std::vector<int32_t> h_len;
  std::vector<uint8_t> h_flag;     // 1: a letter outside ACGT (its pairs are aligned on their bytes)
  std::vector<std::vector<int32_t>> h_runs;   // flagged sequences only: the runs of such letters as (start, end) pairs, ascending (windowed batches)
  uint64_t nwords = 0;             // words of the table, without the 4 zero words behind it
  int64_t nbytes = 0;              // bytes of the ASCII blob
  uint32_t* d_words = nullptr;     // one word-aligned run per sequence (wfa_hip_pack_2bit's layout)
  uint8_t* d_bytes = nullptr;      // the sequences' bytes, back to back (a byte pair needs both of its sequences' bytes)
  uint32_t* d_woff = nullptr; int32_t* d_len = nullptr; int64_t* d_boff = nullptr; uint8_t* d_flag = nullptr;
  mutable uint16_t* d_mask = nullptr;   // the seed finder's view of h_runs: one bit per base, 16 per word (seqset_mask: built on first use)
};

// the base qualities of a set's sequences (include/wfa_hip.h, "base qualities"): a byte per base, raw phred, read after read
struct wfa_hip_qualset {
  wfa_hip_aligner* al = nullptr;
  int64_t n = 0;
  int64_t nbytes = 0;
  std::vector<int32_t> h_len;      // the lengths of the reads it was made over
  uint8_t* d_quals = nullptr; int64_t* d_off = nullptr; int32_t* d_len = nullptr;
};

// ---- a resident handle's life: create_begin, the creator's own checks and `new`, create_adopt, its build, create_done; its destroy
// releases what it owns and ends in destroy_end.  Handles count as the aligner's live batches: the last one to go frees an aligner
// whose destroy is pending.
static inline bool create_begin(wfa_hip_aligner* al) {
  if (!al) return fail_create(al, "null aligner"), false;
  if (hipSetDevice(al->device) != hipSuccess) return fail_create(al, "hipSetDevice failed"), false;
  return true;
}
template <class H> static H* create_adopt(wfa_hip_aligner* al, H* h) {
  h->al = al;
  al->live_batches += 1;
  return h;
}
// the build's outcome: the handle, or nullptr with the reason in g_error too and the handle destroyed
template <class H> static H* create_done(wfa_hip_aligner* al, H* h, int rc, void (*destroy)(H*)) {
  if (rc == WFA_HIP_OK) return h;
  g_error = al->err;
  destroy(h);
  return nullptr;
}
template <class H> static void destroy_end(H* h) {
  wfa_hip_aligner* al = h->al;
  delete h;
  if (--al->live_batches == 0 && al->destroy_pending) aligner_free(al);
}

// The device blocks an entry needs until it returns, with the copies between them and the caller's arrays on the aligner's stream.  The
// destructor waits for the stream before the blocks go back to the pool: an early return behind an enqueued copy leaves no DMA in flight.
struct StreamScratch {
  wfa_hip_aligner* al;
  std::vector<void*> blocks;
  uint32_t* h_cnt = nullptr;          // pinned: the completed pairs of a cross run's last two bands
  hipEvent_t ev[2] = {nullptr, nullptr};
  template <class T> int alloc(T** p, size_t count) {
    HIP_TRY(al, pool_alloc(al, (void**)p, std::max<size_t>(count, 1) * sizeof(T)));
    blocks.push_back(*p);
    return WFA_HIP_OK;
  }
  template <class T> int upload(T** d, const T* host, size_t count) {
    if (alloc(d, count)) return WFA_HIP_EDEVICE;
    HIP_TRY(al, hipMemcpyAsync(*d, host, count * sizeof(T), hipMemcpyHostToDevice, al->stream));
    return WFA_HIP_OK;
  }
  // an optional array: *d stays null without it
  template <class T> int upload_opt(T** d, const T* host, size_t count) { return host ? upload(d, host, count) : WFA_HIP_OK; }
  template <class T> int download(T* host, const T* dev, size_t count) {
    HIP_TRY(al, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, al->stream));
    return WFA_HIP_OK;
  }
  // column c of a block of `ncols` columns of `cells` values each, to host[c]
  template <class T> int download_columns(T* const* host, int ncols, const T* dev, size_t cells) {
    for (int c = 0; c < ncols; ++c)
      if (download(host[c], dev + (size_t)c * cells, cells)) return WFA_HIP_EDEVICE;
    return WFA_HIP_OK;
  }
  ~StreamScratch() {
    (void)hipStreamSynchronize(al->stream);
    for (void* p : blocks) pool_release(al, p);
    if (h_cnt) (void)hipHostFree(h_cnt);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};

// The words (tail 0) or bytes (tail 64: the zero bytes behind a set's blob) of two sets into one table of a batch, device to device: the
// pattern set's, and behind them the text set's unless it is the same set.
template <class T> static int copy_sets(wfa_hip_aligner* al, T* dst, const T* p, size_t np, const T* t, size_t nt, bool same, size_t tail) {
  HIP_TRY(al, hipMemcpyAsync(dst, p, (np + (same ? tail : 0)) * sizeof(T), hipMemcpyDeviceToDevice, al->stream));
  if (!same) HIP_TRY(al, hipMemcpyAsync(dst + np, t, (nt + tail) * sizeof(T), hipMemcpyDeviceToDevice, al->stream));
  return WFA_HIP_OK;
}

#pragma GCC visibility pop
