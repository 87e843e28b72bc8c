// api_sam.hip — the SAM fields of a batch's pairs (the C ABI declared in include/wfa_hip.h, "SAM fields"; csrc/wfa_sam.hpp, k_sam.hip).
#include "host_sets.hpp"
#include "wfa_sam.hpp"

static_assert(WFA_SAM_COLS == WFA_HIP_SAM_COLS, "columns of the kernels and of the ABI");

// what both passes read of the batch
static wfa::SamArgs sam_args(const wfa_hip_batch* b) {
  wfa::SamArgs a;
  memset(&a, 0, sizeof(a));
  a.ops = b->d_ops; a.cigar_begin = b->d_cigar_begin; a.cigar_len = b->d_cigar_len; a.status = b->d_status;
  a.meta = b->d_meta; a.words = b->d_words; a.bytes = b->d_bytes; a.tboff = b->d_tboff; a.flags = b->d_flags;
  a.npairs = b->n;
  a.sam_flags = b->sam_flags;
  a.rows = b->d_sam_rows;
  a.cigar_off = b->d_sam_off; a.md_off = b->d_sam_off + (b->n + 1);
  return a;
}

// the HIP-event time between two recorded events of the scratch, after the stream's synchronisation
static float sam_elapsed(const StreamScratch& sc) {
  float ms = 0.f;
  return sc.ev[0] && sc.ev[1] && hipEventElapsedTime(&ms, sc.ev[0], sc.ev[1]) == hipSuccess ? ms : 0.f;
}

extern "C" int wfa_hip_batch_sam_counts(wfa_hip_batch_t* b, int flags, int32_t* rows, int64_t* cigar_bytes, int64_t* md_bytes) {
  if (!b) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = b->al;
  int rc = batch_of(al, b, "SAM fields", true);
  if (rc != WFA_HIP_OK) return rc;
  if (flags & ~(WFA_HIP_SAM_EQX | WFA_HIP_SAM_CORE)) return fail_inval(al, "SAM fields: unknown flag bits in %d", flags);
  const int64_t n = b->n;
  if ((n > 0 && !rows) || !cigar_bytes || !md_bytes) return fail_inval(al, "SAM fields: null output");
  rc = wfa_hip_batch_sync(b);
  if (rc != WFA_HIP_OK) return rc;
  b->sam_serial = -1;
  b->sam_flags = flags;
  b->sam_bytes[0] = b->sam_bytes[1] = 0;
  b->sam_ms[0] = b->sam_ms[1] = 0.f;
  if (n > 0) {
    HIP_TRY(al, hipSetDevice(al->device));
    const size_t nn = (size_t)n;
    if (!b->d_sam_rows) HIP_TRY(al, pool_alloc(al, (void**)&b->d_sam_rows, nn * WFA_SAM_COLS * sizeof(int32_t)));
    if (!b->d_sam_off) HIP_TRY(al, pool_alloc(al, (void**)&b->d_sam_off, 2 * (nn + 1) * sizeof(uint64_t)));
    StreamScratch sc{al};
    HIP_TRY(al, hipEventCreate(&sc.ev[0]));
    HIP_TRY(al, hipEventCreate(&sc.ev[1]));
    const wfa::SamArgs a = sam_args(b);
    uint64_t totals[2] = {0, 0};
    ReduceTimer timer(al, "SAM counts", n);
    HIP_TRY(al, hipEventRecord(sc.ev[0], al->stream));
    const int lrc = wfa::launch_sam_counts(a, b->d_sam_off, b->d_sam_off + (nn + 1), al->cu_count, al->stream);
    HIP_TRY(al, hipEventRecord(sc.ev[1], al->stream));
    timer.stop();
    if (lrc == 0 && (sc.download(rows, a.rows, nn * WFA_SAM_COLS) || sc.download(&totals[0], a.cigar_off + nn, 1) ||
                     sc.download(&totals[1], a.md_off + nn, 1)))
      return WFA_HIP_EDEVICE;
    rc = launch_end(al, nullptr, lrc, "SAM fields: kernel launch failed");
    if (rc != WFA_HIP_OK) return rc;
    b->sam_ms[0] = sam_elapsed(sc);
    b->sam_bytes[0] = (int64_t)totals[0]; b->sam_bytes[1] = (int64_t)totals[1];
  }
  b->sam_serial = b->run_serial;
  *cigar_bytes = b->sam_bytes[0]; *md_bytes = b->sam_bytes[1];
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_batch_sam_strings(wfa_hip_batch_t* b, uint8_t* cigar, uint8_t* md) {
  if (!b) return WFA_HIP_EINVAL;
  wfa_hip_aligner* al = b->al;
  int rc = batch_of(al, b, "SAM fields", true);
  if (rc != WFA_HIP_OK) return rc;
  if (b->sam_serial < 0 || b->sam_serial != b->run_serial) return fail_inval(al, "SAM fields: call wfa_hip_batch_sam_counts first");
  if ((b->sam_bytes[0] > 0 && !cigar) || (b->sam_bytes[1] > 0 && !md)) return fail_inval(al, "SAM fields: null output");
  if (b->n == 0 || (b->sam_bytes[0] == 0 && b->sam_bytes[1] == 0)) return WFA_HIP_OK;
  HIP_TRY(al, hipSetDevice(al->device));
  StreamScratch sc{al};
  HIP_TRY(al, hipEventCreate(&sc.ev[0]));
  HIP_TRY(al, hipEventCreate(&sc.ev[1]));
  wfa::SamArgs a = sam_args(b);
  if (sc.alloc(&a.cigar, (size_t)b->sam_bytes[0]) || sc.alloc(&a.md, (size_t)b->sam_bytes[1])) return WFA_HIP_EDEVICE;
  ReduceTimer timer(al, "SAM strings", b->n);
  HIP_TRY(al, hipEventRecord(sc.ev[0], al->stream));
  const int lrc = wfa::launch_sam_strings(a, al->cu_count, al->stream);
  HIP_TRY(al, hipEventRecord(sc.ev[1], al->stream));
  timer.stop();
  if (lrc == 0 && ((b->sam_bytes[0] > 0 && sc.download(cigar, a.cigar, (size_t)b->sam_bytes[0])) ||
                   (b->sam_bytes[1] > 0 && sc.download(md, a.md, (size_t)b->sam_bytes[1]))))
    return WFA_HIP_EDEVICE;
  rc = launch_end(al, nullptr, lrc, "SAM fields: kernel launch failed");
  if (rc == WFA_HIP_OK) b->sam_ms[1] = sam_elapsed(sc);
  return rc;
}

extern "C" int wfa_hip_batch_sam_kernel_ms(wfa_hip_batch_t* b, float* ms) {
  if (!b || !ms) return WFA_HIP_EINVAL;
  *ms = b->sam_ms[0] + b->sam_ms[1];
  return WFA_HIP_OK;
}
