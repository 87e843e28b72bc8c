# wfa_hip.pxd — the Cython declarations of include/wfa_hip.h a pywfa maintainer adds in place of pywfa/WFA_wrap.pxd
# (INTEGRATION.md §2).  tests/test_cython_shim.py compiles this file and wfa_shim.pyx against the header and libwfa_hip.so.
from libc.stdint cimport int32_t, int64_t, uint8_t

cdef extern from "wfa_hip.h" nogil:
    ctypedef struct wfa_hip_config_t:
        int32_t distance, match, mismatch, gap_opening, gap_extension, gap_opening2, gap_extension2
        int32_t scope, span, pattern_begin_free, pattern_end_free, text_begin_free, text_end_free
        int32_t heuristic, min_wavefront_length, max_distance_threshold, steps_between_cutoffs, xdrop
        int32_t memory_mode, max_steps, wildcard, reserved
    ctypedef struct wfa_hip_aligner_t
    int wfa_hip_abi_version()
    int wfa_hip_device_count()
    int wfa_hip_config_default(wfa_hip_config_t* cfg)
    int wfa_hip_config_validate(const wfa_hip_config_t* cfg, char* err, size_t errlen)
    wfa_hip_aligner_t* wfa_hip_create(const wfa_hip_config_t* cfg, int device)
    void wfa_hip_destroy(wfa_hip_aligner_t* aligner)
    int wfa_hip_set_config(wfa_hip_aligner_t* aligner, const wfa_hip_config_t* cfg)
    const char* wfa_hip_last_error(const wfa_hip_aligner_t* aligner)
    const char* wfa_hip_global_error()
    int wfa_hip_align_batch(wfa_hip_aligner_t* aligner, int64_t n, const uint8_t* seqs,
                            const int64_t* p_off, const int32_t* p_len,
                            const int64_t* t_off, const int32_t* t_len,
                            int32_t* score, int32_t* status, uint8_t* cigar_ops,
                            const int64_t* cigar_off, int64_t* cigar_begin, int32_t* cigar_len)
    int64_t wfa_hip_cigar_sprint_pretty(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen,
                            const uint8_t* text, int32_t tlen, char* out, int64_t cap)
    # the seed finder over resident sequence sets (include/wfa_hip.h: "seed finder")
    ctypedef struct wfa_hip_seqset_t
    ctypedef struct wfa_hip_seed_index_t
    wfa_hip_seqset_t* wfa_hip_seqset_create(wfa_hip_aligner_t* aligner, int64_t n, const uint8_t* seqs, const int64_t* off, const int32_t* len)
    void wfa_hip_seqset_destroy(wfa_hip_seqset_t* set)
    wfa_hip_seed_index_t* wfa_hip_seed_index_create(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* texts, int k, int stride, int max_occ)
    void wfa_hip_seed_index_destroy(wfa_hip_seed_index_t* index)
    int wfa_hip_seed_index_query(wfa_hip_seed_index_t* index, const wfa_hip_seqset_t* patterns, int n, int min_hits, int gap, int pad,
                            int max_hits, int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits,
                            uint8_t* overflow)
    int wfa_hip_seed_index_stats(const wfa_hip_seed_index_t* index, int64_t* positions, int64_t* masked_kmers, int64_t* table_bytes,
                            float* build_ms, float* query_ms)
    int wfa_hip_seeds_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                            const int32_t* t_len, int k, int stride, int max_occ, int n, int min_hits, int gap, int pad, int max_hits,
                            int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits, uint8_t* overflow,
                            char* msg, size_t msg_cap)
    int wfa_hip_seed_index_chain(wfa_hip_seed_index_t* index, const wfa_hip_seqset_t* patterns, int n, int min_hits, int min_score,
                            int lookback, int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse,
                            int32_t* text_start, int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start,
                            int32_t* pattern_len, uint8_t* overflow)
    int wfa_hip_seed_index_chain_stats(const wfa_hip_seed_index_t* index, float* kernel_ms, int64_t* workspace_bytes)
    int wfa_hip_chains_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                            const int32_t* t_len, int k, int stride, int max_occ, int n, int min_hits, int min_score, int lookback,
                            int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse, int32_t* text_start,
                            int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start, int32_t* pattern_len,
                            uint8_t* overflow, char* msg, size_t msg_cap)
    # minimizers (include/wfa_hip.h: "minimizers")
    wfa_hip_seed_index_t* wfa_hip_seed_index_create_minimizer(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* texts, int k, int w,
                            int max_occ)
    int wfa_hip_seed_index_params(const wfa_hip_seed_index_t* index, int* k, int* stride, int* w)
    int wfa_hip_minimizers_host(const uint8_t* seq, int64_t len, int k, int w, uint8_t* selected, char* msg, size_t msg_cap)
    int wfa_hip_seeds_host_minimizer(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                            const int32_t* t_len, int k, int w, int max_occ, int n, int min_hits, int gap, int pad, int max_hits,
                            int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits, uint8_t* overflow,
                            char* msg, size_t msg_cap)
    int wfa_hip_chains_host_minimizer(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                            const int32_t* t_len, int k, int w, int max_occ, int n, int min_hits, int min_score, int lookback,
                            int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse, int32_t* text_start,
                            int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start, int32_t* pattern_len,
                            uint8_t* overflow, char* msg, size_t msg_cap)
    # calls and sites of a pileup (include/wfa_hip.h: "calls and sites")
    ctypedef struct wfa_hip_pileup_t
    int wfa_hip_pileup_calls(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                            int32_t min_depth, uint8_t* out)
    int wfa_hip_pileup_sites(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                            int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows)
    int wfa_hip_calls_host(const int32_t* counts, const uint8_t* ref, int64_t len, int32_t min_depth, uint8_t* out)
    int wfa_hip_sites_host(const int32_t* counts, const uint8_t* ref, int64_t len, int32_t seq, int64_t start, int32_t min_depth,
                            int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows)
    # what the reads insert: the log of a tracking pileup and its alleles (include/wfa_hip.h: "insertions")
    int wfa_hip_pileup_track_insertions(wfa_hip_pileup_t* pileup, int on)
    int wfa_hip_pileup_insertion_stats(wfa_hip_pileup_t* pileup, int64_t* records, int64_t* bases)
    int wfa_hip_pileup_insertions(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                  int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows,
                                  int64_t bases_cap, int64_t* bases_count, uint8_t* bases)
    int wfa_hip_ops_insertions(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, int32_t tlen, int64_t cap,
                               int64_t* count, int32_t* recs, int64_t cols_cap, int64_t* cols_count, uint8_t* cols)
    int wfa_hip_insertions_host(const int32_t* counts, int64_t len, int32_t seq, int64_t start, int32_t min_depth, int32_t min_permille,
                                int64_t nrec, const int64_t* rec_row, const int32_t* rec_n, const int64_t* rec_off, const uint8_t* cols,
                                int64_t ncols, int64_t cap, int64_t* count, int32_t* rows, int64_t bases_cap, int64_t* bases_count,
                                uint8_t* bases)
    # what the reads delete: the log of a tracking pileup, its starts plane and its rows (include/wfa_hip.h: "deletions")
    int wfa_hip_pileup_track_deletions(wfa_hip_pileup_t* pileup, int on)
    int wfa_hip_pileup_deletion_stats(wfa_hip_pileup_t* pileup, int64_t* records, int64_t* bases)
    int wfa_hip_pileup_read_deletion_starts(wfa_hip_pileup_t* pileup, int32_t seq, int64_t start, int64_t len, int32_t* out)
    int wfa_hip_pileup_deletions(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                 int32_t min_depth, int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows)
    int wfa_hip_ops_deletions(const uint8_t* ops, int64_t ops_len, int32_t plen, int32_t tlen, int64_t cap, int64_t* count,
                              int32_t* recs)
    int wfa_hip_deletions_host(const int32_t* counts, const int32_t* starts, int64_t len, int32_t seq, int64_t start,
                               int32_t min_depth, int32_t min_permille, int64_t nrec, const int64_t* rec_row, const int32_t* rec_n,
                               int64_t cap, int64_t* count, int32_t* rows)
    # placement: one row per read from the hits of any number of batches (include/wfa_hip.h: "placement")
    ctypedef struct wfa_hip_batch_t
    ctypedef struct wfa_hip_placer_t
    wfa_hip_placer_t* wfa_hip_placer_create(wfa_hip_aligner_t* aligner, int64_t nreads)
    int wfa_hip_placer_add(wfa_hip_placer_t* placer, wfa_hip_batch_t* batch, const int32_t* i, const int32_t* j, const int32_t* t_start,
                            const uint8_t* reverse)
    int wfa_hip_placer_add_hits(wfa_hip_placer_t* placer, int64_t n, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                            const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end)
    int wfa_hip_placer_run(wfa_hip_placer_t* placer, int32_t min_score, int32_t full_gap, int32_t* rows, uint8_t* flags)
    int64_t wfa_hip_placer_count(const wfa_hip_placer_t* placer)
    int wfa_hip_placer_clear(wfa_hip_placer_t* placer)
    int wfa_hip_placer_kernel_ms(const wfa_hip_placer_t* placer, float* ms)
    void wfa_hip_placer_destroy(wfa_hip_placer_t* placer)
    int wfa_hip_place_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse, const int32_t* score,
                            const int32_t* status, const int32_t* text_start, const int32_t* text_end, int32_t min_score,
                            int32_t full_gap, int32_t* rows, uint8_t* flags, char* msg, size_t msg_cap)
    # per-strand counts and genotyped sites of a pileup (include/wfa_hip.h: "strands and genotypes")
    int wfa_hip_pileup_track_strands(wfa_hip_pileup_t* pileup, int on)
    int wfa_hip_pileup_add_strands(wfa_hip_pileup_t* pileup, wfa_hip_batch_t* batch, const int32_t* j, const int32_t* t_start,
                                   const uint8_t* keep, const uint8_t* reverse)
    int wfa_hip_pileup_read_strand(wfa_hip_pileup_t* pileup, int32_t seq, int64_t start, int64_t len, int strand, int32_t* counts)
    int wfa_hip_pileup_genotypes(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                 int32_t min_depth, int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap,
                                 int64_t* count, int32_t* rows)
    int wfa_hip_genotypes_host(const int32_t* counts, const int32_t* counts_fwd, const uint8_t* ref, int64_t len, int32_t seq,
                               int64_t start, int32_t min_depth, int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap,
                               int64_t* count, int32_t* rows)
    # base qualities of a pileup (include/wfa_hip.h: "base qualities")
    ctypedef struct wfa_hip_qualset_t
    wfa_hip_qualset_t* wfa_hip_qualset_create(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* reads, const uint8_t* quals,
                                              const int64_t* off, const int32_t* len)
    void wfa_hip_qualset_destroy(wfa_hip_qualset_t* quals)
    int wfa_hip_pileup_track_qualities(wfa_hip_pileup_t* pileup, int on)
    int wfa_hip_pileup_add_quals(wfa_hip_pileup_t* pileup, wfa_hip_batch_t* batch, const int32_t* j, const int32_t* t_start,
                                 const uint8_t* keep, const uint8_t* reverse, const wfa_hip_qualset_t* quals, const int32_t* i,
                                 const int32_t* p_start, int32_t min_base_quality, int32_t quality_cap)
    int wfa_hip_pileup_read_quality(wfa_hip_pileup_t* pileup, int32_t seq, int64_t start, int64_t len, int32_t* qsums)
    int wfa_hip_pileup_genotypes_quals(wfa_hip_pileup_t* pileup, const wfa_hip_seqset_t* texts, int32_t seq, int64_t start, int64_t len,
                                       int32_t min_depth, int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap,
                                       int64_t* count, int32_t* rows)
    int wfa_hip_ops_pileup_quals(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, int32_t tlen,
                                 const uint8_t* quals, int32_t min_base_quality, int32_t quality_cap, int32_t* rows, int32_t* qrows)
    int wfa_hip_genotypes_quals_host(const int32_t* counts, const int32_t* qsums, const int32_t* counts_fwd, const uint8_t* ref,
                                     int64_t len, int32_t seq, int64_t start, int32_t min_depth, int32_t min_permille, int32_t err_q,
                                     int32_t min_alt_strand, int64_t cap, int64_t* count, int32_t* rows)
    # pairing: one row per fragment of two reads (include/wfa_hip.h: "pairing")
    int wfa_hip_placer_run_pairs(wfa_hip_placer_t* placer, int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert,
                            int32_t unpaired, int64_t nfrag, const int32_t* mate1, const int32_t* mate2, int32_t* rows, uint8_t* flags,
                            int32_t* pair_rows, uint8_t* pair_flags)
    int wfa_hip_pair_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse, const int32_t* score,
                            const int32_t* status, const int32_t* text_start, const int32_t* text_end, int32_t min_score,
                            int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag,
                            const int32_t* mate1, const int32_t* mate2, int32_t* rows, uint8_t* flags, int32_t* pair_rows,
                            uint8_t* pair_flags, char* msg, size_t msg_cap)
    # rescue: the window of a lost mate from its anchored partner (include/wfa_hip.h: "rescue")
    int wfa_hip_placer_rescue(wfa_hip_placer_t* placer, const wfa_hip_seqset_t* patterns, const wfa_hip_seqset_t* texts, int32_t min_score,
                            int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag,
                            const int32_t* mate1, const int32_t* mate2, int32_t pad, int32_t min_len, int32_t anchor_mapq, int64_t cap,
                            int64_t* count, int32_t* rows)
    int wfa_hip_rescue_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse, const int32_t* score,
                            const int32_t* status, const int32_t* text_start, const int32_t* text_end, int32_t min_score,
                            int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag,
                            const int32_t* mate1, const int32_t* mate2, const int32_t* read_len, int64_t ntexts, const int32_t* text_len,
                            int32_t pad, int32_t min_len, int32_t anchor_mapq, int64_t cap, int64_t* count, int32_t* rows, char* msg,
                            size_t msg_cap)
    # duplicates: one representative per group of fragments / reads with the same ends (include/wfa_hip.h: "duplicates")
    int wfa_hip_placer_duplicates(wfa_hip_placer_t* placer, const wfa_hip_seqset_t* texts, int32_t min_score, int32_t full_gap,
                            int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag, const int32_t* mate1,
                            const int32_t* mate2, int32_t* read_rows, int32_t* pair_rows)
    int wfa_hip_duplicates_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                            const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end,
                            int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired,
                            int64_t nfrag, const int32_t* mate1, const int32_t* mate2, int64_t ntexts, const int32_t* text_len,
                            int32_t* read_rows, int32_t* pair_rows, char* msg, size_t msg_cap)
    # clips of every hit, duplicates on unclipped ends, the representative by summed base quality (include/wfa_hip.h: "placement" CLIPS,
    # "duplicates")
    int wfa_hip_placer_add_hits_clips(wfa_hip_placer_t* placer, int64_t n, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                            const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end,
                            const int32_t* lead, const int32_t* trail)
    int wfa_hip_placer_read_clips(wfa_hip_placer_t* placer, int32_t* lead, int32_t* trail)
    int wfa_hip_ops_clips(const uint8_t* ops, int64_t ops_len, int32_t plen, int32_t tlen, int32_t* lead, int32_t* trail)
    int wfa_hip_placer_duplicates_ex(wfa_hip_placer_t* placer, const wfa_hip_seqset_t* texts, int32_t min_score, int32_t full_gap,
                            int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag, const int32_t* mate1,
                            const int32_t* mate2, int32_t* read_rows, int32_t* pair_rows, int flags, const wfa_hip_qualset_t* quals,
                            int32_t min_quality)
    int wfa_hip_duplicates_host_ex(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                            const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end,
                            int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired,
                            int64_t nfrag, const int32_t* mate1, const int32_t* mate2, int64_t ntexts, const int32_t* text_len,
                            int32_t* read_rows, int32_t* pair_rows, const int32_t* lead, const int32_t* trail, int flags,
                            const int32_t* qsum, char* msg, size_t msg_cap)
    int wfa_hip_qsum_host(const uint8_t* quals, int64_t len, int32_t min_quality, int32_t* out)
