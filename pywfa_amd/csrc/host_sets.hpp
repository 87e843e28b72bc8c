// host_sets.hpp — the resident sequence set as the units built on it see it (api_*.hip; the core, wfa_hip.hip, knows nothing of sets).
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

static void aligner_release_ref(wfa_hip_aligner* al) {
  if (--al->live_batches == 0 && al->destroy_pending) aligner_free(al);
}

// the device blocks of one cross run besides the batch view's (released when the run returns)
struct CrossScratch {
  wfa_hip_aligner* al;
  std::vector<void*> blocks;
  uint32_t* h_cnt = nullptr;          // pinned: the completed pairs of the last two bands
  hipEvent_t ev[2] = {nullptr, nullptr};
  template <class T> int alloc(T** p, size_t count) {
    HIP_TRY(al, pool_alloc(al, (void**)p, std::max<size_t>(count, 1) * sizeof(T)));
    blocks.push_back(*p);
    return WFA_HIP_OK;
  }
  ~CrossScratch() {
    (void)hipStreamSynchronize(al->stream);
    for (void* p : blocks) pool_release(al, p);
    if (h_cnt) (void)hipHostFree(h_cnt);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};

#pragma GCC visibility pop
