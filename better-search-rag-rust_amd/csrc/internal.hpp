// internal.hpp -- host-side state shared by the C-ABI translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>

#include <atomic>

#include <string>
#include <vector>

#include "bsr.h"
#include "kernels.hpp"

namespace bsr {

int set_error(int code, const char* fmt, ...);
void clear_error();

#define BSR_HIP(call)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return ::bsr::set_error(BSR_E_HIP, "%s failed: %s (%s:%d)", #call,              \
                                    hipGetErrorString(e_), __FILE__, __LINE__);             \
    } while (0)

#define BSR_TRY(call)               \
    do {                            \
        int r_ = (call);            \
        if (r_ != BSR_OK) return r_; \
    } while (0)

// Bumped by every device / pinned (re)allocation: a captured search graph is valid only
// for the generation it was captured in.
extern std::atomic<uint64_t> g_alloc_gen;

// Growable device allocation (never shrinks).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need);
    // At least `need` bytes with the first `keep` bytes kept and zeros behind them: a new
    // allocation takes the buffer's place once the copy is done (the stream is then idle).
    int grow(size_t need, size_t keep, hipStream_t s);
    void release();
    template <class T> T* as() const { return static_cast<T*>(p); }
    ~DevBuf() { release(); }
};

bool is_device_ptr(const void* p);
void* coherent_host_alias(const void* p);  // device address of coherent pinned host memory, or nullptr
hipError_t stream_wait(hipStream_t s);  // poll until the stream's work is done
// Poll a host flag a publishing kernel raises (checking the stream now and then): hipSuccess,
// the stream's error, or hipErrorUnknown when the stream finished without raising it.
hipError_t flag_wait(const uint32_t* flag, hipStream_t s);
int select_device(int device);

static inline uint64_t round_up(uint64_t x, uint64_t m) { return (x + m - 1) / m * m; }
// Rows of the fop_s sample operand of an n-row shard: every kSampleStride-th row, padded to whole
// scale groups (at least one).
static inline uint64_t sample_rows_pad(uint64_t n) {
    const uint64_t n_s = (n + kSampleStride - 1) / kSampleStride;
    return round_up(n_s ? n_s : 1, kSampleScaleRows);
}

struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    bool armed = false;
    ~Events();
    int create();
};

}  // namespace bsr

struct bsr_index {
    bsr_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t dim = 0, ld = 0;
    uint64_t n = 0, n_pad = 0, global_offset = 0;
    bool loaded = false;
    bool approx_ok = false;
    uint32_t row_flags = 0;
    uint32_t op_row_bytes = 0;          // bytes of one filter operand row
    float row_ebound = 0.0f;            // int8: max_row ||a/|a| - s q||_2 (certification)

    bsr::DevBuf rows;   // f32 [n_pad][ld], zero padded: the reference's values
    bsr::DevBuf na;     // f32 [n_pad]: exact magnitudes (src/metrics.rs:154)
    bsr::DevBuf fop;    // filter operand rows: int8 [n_pad][ld]
    bsr::DevBuf fop_s;  // every kSampleStride-th row as the sample pass's operand, contiguous
    bsr::DevBuf ascale_s; // int8: f32 [n_s_pad / kSampleScaleRows] sample operand scales
    // The sample of the batch in flight (set by its sample pass, read by its emit pass): sample
    // tiles of fop scored once (GemmArgs::s_tiles; 0: the fop_s sample), the row length of S and
    // its valid values per query.
    uint32_t smp_tiles = 0, smp_ld = 0, smp_vals = 0;
    bsr::DevBuf ascale; // int8: f32 [n_pad/32] block scales
    bsr::DevBuf flags;  // u32 [2]: row flags, int8 row error bound (f32 bits)

    // per-search scratch
    bsr::DevBuf q_in, qf32, nb, qop, qscale, ebound, qflags, tau, S, cand, cnt, cand_rows, ncand,
        tau_excl, keys, fail, fail2, part, qids, qids_id, tmp;

    // Packed per-search result, double-buffered: [status words | counts | distances |
    // indices].  One D2H copy per search reads it all back (into pinned memory); the
    // finalize kernel of search i zeroes the status words of the buffer search i+1 uses.
    bsr::DevBuf res[2];
    uint8_t* h_res = nullptr;  // pinned, fine-grained (hipHostMallocCoherent) mirror of one result buffer
    uint8_t* h_res_dev = nullptr;   // its device-side address (the publishing kernel writes it)
    size_t h_res_bytes = 0;
    uint32_t* h_flag = nullptr;     // fine-grained host word raised by the publishing kernel
    uint32_t* h_flag_dev = nullptr;
    bsr::DevBuf pub_ticket;         // device word: workgroups finished in the publishing kernel
    uint32_t cur = 0;          // result buffer of the last search
    bool next_status_clean = false;  // status words of res[cur ^ 1] are known to be zero
    size_t res_off_cnt = 0, res_off_dist = 0, res_off_idx = 0, res_off_x = 0, res_bytes = 0;
    uint32_t* d_status = nullptr;
    uint32_t* d_cnt = nullptr;
    float* d_dist = nullptr;
    uint64_t* d_idx = nullptr;
    float* d_x = nullptr;      // global-threshold search: per-query exclusion bounds

    std::vector<uint32_t> h_qflags, h_fail;

    bsr_search_stats stats{};
    bsr_profile prof{};
    bsr::Events ev_emit, ev_sample, ev_select, ev_rescore, ev_scan, ev_total;
    int prof_level = 2;  // bsr_index_set_profile

    // Filtered batches replay a captured hipGraph of query prep -> filter -> select -> rescore
    // (-> D2H) instead of ~9 launches.  One graph per result buffer; captured on the second search
    // of a shape (the first sizes every buffer), dropped when the shape or any allocation changes.
    // Only untimed searches are captured (a timed search launches directly, its events recorded
    // on the stream).
    // The shape of a graphable search: what a capture bakes in.
    struct SearchKey {
        uint32_t nq = 0, k = 0;
        const float* qsrc = nullptr;  // the queries on the device (the caller's, or q_in)
        uint64_t n = 0, gen = 0;      // shard rows; g_alloc_gen
        uint64_t dead_gen = 0;        // tombstone generation (a capture bakes the live count and the bitset)
        bool top = false;            // the self-thresholded single-query path (round 6)
        // the switches read per search (A/B runs change them in process):
        uint32_t top_layout = 2;      // the TOP row layout (BSR_TOP_LAYOUT, lab)
        bool skinny_glds = true;      // BSR_SKINNY_GLDS
        bool sample_tiles = true;     // BSR_SAMPLE_TILES
        bool operator==(const SearchKey& o) const {
            return nq == o.nq && k == o.k && qsrc == o.qsrc && n == o.n && gen == o.gen &&
                   dead_gen == o.dead_gen && top == o.top &&
                   top_layout == o.top_layout && skinny_glds == o.skinny_glds && sample_tiles == o.sample_tiles;
        }
    };
    struct SearchGraph {
        hipGraphExec_t exec = nullptr;
        SearchKey key;
    };
    bool capturing = false;    // a search is being captured into a graph
    SearchGraph graphs[2];
    SearchKey warm;  // the last direct search of a graphable shape
    uint64_t graph_replays = 0;
    ~bsr_index();

    // Run the local search; results stay in d_idx / d_dist / d_cnt (device, [nq][k]) and in
    // the pinned host mirror h_res at the same offsets.  after_launch (optional) runs once the
    // search's GPU work is enqueued, before the host waits for it (the parallel search issues
    // its shape-agreement collective there); its non-OK status is returned after the wait.
    // force_threshold: the search's own rerun of a batch the self-thresholded path left uncertified.
    int search_device(const float* queries, uint32_t nq, uint32_t k, int (*after_launch)(void*) = nullptr,
                      void* ctx = nullptr, bool force_threshold = false);
    int prepare_result(uint32_t nq, uint32_t k);

    // The local search restricted to the rows an allow mask names (bsr_local_top_k_masked,
    // DESIGN.md §10): launched directly, never captured, no publish flag; results where
    // search_device leaves them.  allow: host or device words, ceil(n / 64) of them.
    int search_device_masked(const float* queries, uint32_t nq, uint32_t k, const uint64_t* allow,
                             uint64_t allow_words, uint32_t mode);
    bsr::DevBuf mask_dev;   // a host mask's device copy
    bsr::DevBuf mask_blk;   // u32 [mask_blocks(n) + 1]: block offsets, the allowed-row count
    bsr::DevBuf mask_list;  // u32 [A]: the allowed rows, ascending
    bsr::DevBuf mask_aux;   // u32 [qpad + 1]: emitted counts before the cut; the rescore's item count

    // The same with one allow mask per group of queries (bsr_local_top_k_masked_groups, DESIGN.md
    // §12): allow [n_masks][allow_words], query_mask [nq], each host or device.
    int search_device_masked_groups(const float* queries, uint32_t nq, uint32_t k, const uint64_t* allow,
                                    uint64_t allow_words, uint32_t n_masks, const uint32_t* query_mask,
                                    uint32_t mode);
    bsr::DevBuf grp_qmask;  // u32 [nq]: a host query_mask's device copy
    bsr::DevBuf grp_blk;    // u32 [n_masks][mask_blocks(n) + 1]: every mask's block offsets
    bsr::DevBuf grp_out;    // u32 [n_masks + 1]: A_g; the query_mask entries that name no mask
    bsr::DevBuf grp_ksq;    // u32 [qpad]: per-query threshold depth (0: the query's group takes the list)
    bsr::DevBuf grp_aq;     // u32 [nq]: A of the query's mask (the result count's bound)
    bsr::DevBuf grp_lists;  // MaskListDesc: the lists of every chunk
    bsr::DevBuf grp_scan;   // ScanGroupDesc: the query groups of every grouped scan launch
    std::vector<uint32_t> h_grp_qmask, h_grp_out, h_grp_ksq, h_grp_aq;
    std::vector<int32_t> h_grp_ids;
    std::vector<bsr::MaskListDesc> h_grp_lists;
    std::vector<bsr::ScanGroupDesc> h_grp_scan;

    // Tombstones (bsr_index_delete): the bitset of deleted rows, allocated by the
    // first delete (ceil(n_pad / 64) words, zero beyond the deleted rows), and what is derived from it.
    // Every mask kernel takes the bitset next to the allow mask and removes its rows as it reads.
    bsr::DevBuf dead;
    uint64_t n_dead = 0;     // deleted rows
    uint64_t dead_gen = 0;   // bumped by every delete that changes a row, and by a load that clears any
    bsr::DevBuf dead_ids;    // a delete's host ids on the device
    bsr::DevBuf dead_cnt;    // u32 [2]: ids out of range, rows newly deleted
    bsr::DevBuf live_blk;    // the live rows' block offsets (launch_mask_list_count); during a delete, the bitset's own
    bsr::DevBuf live_list;   // u32 [live]: the live rows, ascending -- the exact fallback's row list
    bool live_list_ok = false;  // built since the last delete / append / load
    uint64_t live_rows() const { return n - n_dead; }
    const uint64_t* dead_bits() const { return n_dead ? dead.as<uint64_t>() : nullptr; }
    int delete_rows(const uint64_t* ids, uint64_t n_ids, uint64_t* out_deleted);
    int deleted_mask(uint64_t* out_words, uint64_t words) const;
    void clear_tombstones();        // load: every row live again
    int tombstones_after_append();  // the bitset grown to the new rows, the operand zeroed again
    int ensure_live_list();         // live_list, built from the bitset (no allow mask) when it is not there

    // In-place update (bsr_index_update): rows replaced by global id, the derived
    // state of their blocks rebuilt from lists.  A captured search graph bakes in nothing an update
    // changes (rows, na, fop, the scales and ea_max are read through the same pointers; approx_ok is
    // read per search, before the graph is looked up), so SearchKey has no update generation.
    int update_rows(const uint64_t* ids, const void* new_rows, uint64_t n_ids);
    bsr::DevBuf upd_ids;    // an update's host ids on the device
    bsr::DevBuf upd_bits;   // u64: touched rows [n_pad / 64] | touched blocks | touched sample groups
    bsr::DevBuf upd_cnt;    // u64 [kUpdCounts]
    bsr::DevBuf upd_blk;    // u32: block prefixes of the blocks' and of the groups' bitset (launch_mask_list_count)
    bsr::DevBuf upd_list;   // u32: the touched blocks, then the touched sample groups, each ascending

    // Compaction (bsr_index_compact): the deleted rows dropped, the live rows packed
    // in place in ascending order (chunks through the bounded staging buffer), the derived state
    // rebuilt by index_finish_load, the tombstones cleared and the global offset replaced.
    int compact_rows(uint64_t new_global_offset, uint32_t flags, uint64_t* out_old_ids, uint64_t out_capacity,
                     uint64_t* out_count);
    bsr::DevBuf cmp_stage;  // f32 [chunk rows][ld]: BSR_COMPACT_STAGE_BYTES (read per call), kept
    bsr::DevBuf cmp_first;  // u32: the first row that moves

    // Range search (bsr_local_range_search): every live row within radius[q] of
    // query q, `capacity` result slots per query.  Launched directly, never captured; its result
    // rows go to buffers of its own (the packed result of begin_batch carries only its status
    // words), and from there to the caller's arrays, host or device.
    int range_search_device(const float* queries, uint32_t nq, const float* radius, uint32_t capacity,
                            uint64_t* out_idx, float* out_dist, uint32_t* out_count);
    bsr::DevBuf rng_radius;  // f32 [nq]: a host radius array's device copy
    bsr::DevBuf rng_keys;    // u64 [nq][range_cap(capacity)]: the in-range distance keys, any order
    bsr::DevBuf rng_cnt;     // u32 [nq]: their exact counts
    bsr::DevBuf rng_idx, rng_dist, rng_out_cnt;  // the result rows [nq][capacity], the counts [nq]

    // Scoring caller-chosen rows (bsr_local_score_ids / bsr_local_rerank_ids): the
    // distance of every id of ids [nq][m] (k = 0: into out_dist [nq][m] and out_found, nullable), or
    // the k best distinct present ids of every list (k > 0: out_idx / out_dist [nq][k], out_count).
    // Launched directly, never captured; everything goes to buffers of its own first and to the
    // caller's arrays, host or device, only once the status words are read.
    int score_ids_device(const float* queries, uint32_t nq, const uint64_t* ids, uint32_t m, uint32_t k,
                         uint64_t* out_idx, float* out_dist, uint32_t* out_cnt);
    bsr::DevBuf scr_ids;    // u64 [nq][m]: a host id array's device copy
    bsr::DevBuf scr_dist;   // f32 [nq][m]: the aligned distances
    bsr::DevBuf scr_keys;   // u64 [nq][m]: the rerank's distance keys, any order
    bsr::DevBuf scr_cnt;    // u32 [nq]: the present slots (score) or the keys (rerank) of a query
    bsr::DevBuf scr_idx, scr_odist, scr_ocnt;  // the rerank's result rows [nq][k], the counts [nq]

    // Masked range search (bsr_local_range_search_masked): the range search with an
    // allow mask per query group -- the grouped masked search's mask buffers (grp_*), the range
    // search's result buffers (rng_*), and the row lists in segments.
    int range_search_device_masked(const float* queries, uint32_t nq, const float* radius, uint32_t capacity,
                                   const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                   const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx, float* out_dist,
                                   uint32_t* out_count);
    bsr::DevBuf rng_route;  // u32 [nq]: 1 = the query's group takes the list scan by design
    bsr::DevBuf rng_segs;   // MaskSegDesc: the list segments of every chunk
    std::vector<uint32_t> h_rng_route;
    std::vector<bsr::MaskSegDesc> h_rng_segs;

    // MMR search (bsr_local_top_k_mmr): the candidate search with k = fetch_k (plain,
    // masked or grouped, by the mask arguments) run to completion, then the selection kernel over the
    // lists it left in d_idx / d_dist / d_cnt -- launched directly, never captured -- into the
    // caller's arrays, host or device (out_rank nullable).  The candidate search keeps its graphs.
    int mmr_search_device(const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k, float lambda,
                          const uint64_t* allow, uint64_t allow_words, uint32_t n_masks, const uint32_t* query_mask,
                          uint32_t mode, uint64_t* out_idx, float* out_dist, uint32_t* out_rank, uint32_t* out_count);
    bsr::DevBuf mmr_idx, mmr_dist, mmr_rank, mmr_cnt;  // the picks [nq][k], their counts [nq]

    // Collapsed search (bsr_local_top_k_collapsed): the group check, the candidate
    // search with k = fetch_k run to completion, the walk over its lists, and for the queries the
    // walk could not certify the group scan in rounds -- table memset, scan, selection, merge, finish.
    // All launched directly, never captured; the candidate search keeps its graphs.  Every buffer
    // but the table is sized before the candidate search; the table at the first scan, and kept.
    int collapsed_search_device(const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k,
                                const uint32_t* row_group, uint32_t n_groups, const uint64_t* allow,
                                uint64_t allow_words, uint32_t n_masks, const uint32_t* query_mask, uint32_t mode,
                                uint64_t* out_idx, float* out_dist, uint32_t* out_group, uint32_t* out_count);
    // Capped search (bsr_local_top_k_capped): the same sequence with the capped walk
    // and scan, min(per_group, k) table entries per (query, group), and the same buffers -- the two
    // are group_search_device (per_group = 0: the collapsed search).
    int capped_search_device(const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k, uint32_t per_group,
                             const uint32_t* row_group, uint32_t n_groups, const uint64_t* allow, uint64_t allow_words,
                             uint32_t n_masks, const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx,
                             float* out_dist, uint32_t* out_group, uint32_t* out_count);
    int group_search_device(const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k, uint32_t per_group,
                            const uint32_t* row_group, uint32_t n_groups, const uint64_t* allow, uint64_t allow_words,
                            uint32_t n_masks, const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx,
                            float* out_dist, uint32_t* out_group, uint32_t* out_count);
    bsr::DevBuf col_grp;    // u32 [n]: a host row_group's device copy
    bsr::DevBuf col_flag;   // u32 [2]: the group check's flag; the fail list's count
    bsr::DevBuf col_fail;   // u32 [nq]: the queries the walk could not certify
    bsr::DevBuf col_qids;   // i32 [rounds][kScanQF]: their ids by scan round, each round padded
    bsr::DevBuf col_keys;   // u64 [nq][k]: the merged keys of the scanned queries
    bsr::DevBuf col_best;   // u64 [queries of a round][n_groups][entries per group]: the scan's tables
    bsr::DevBuf col_idx, col_dist, col_group, col_cnt;  // the result rows [nq][k], the counts [nq]

    // Parallel search with a global emission threshold (P > 1), in two halves
    // around the all-gather of every rank's ks best sample keys:
    //   phase A: query prep, the sample pass, tau0 and the keys (smax [qpad][gt_ks]);
    //   phase B: the global threshold from the gathered keys g[P][qpad][gt_ks], the emit pass
    //            and the exact rescore of EVERY emitted row, its top-k written as the result
    //            rows with the per-query exclusion bound d_x (no local certification).
    // Both enqueue only (no host wait); gtau_prepare sizes every buffer of phase A first.
    // gtau_eligible: the filter path with a sample pass.
    bool gtau_eligible(uint32_t nq, uint32_t k) const;
    int gtau_prepare(const float* queries, uint32_t nq, uint32_t k);  // buffers only (before the header)
    int gtau_phase_a(const float* queries, int part);  // launches only: part 0 query prep, 1 sample + tau0
    int gtau_phase_b(const uint64_t* g_smax, uint32_t P, uint32_t* merge_words = nullptr);
    bsr::DevBuf smax;
    uint32_t gt_nq = 0, gt_k = 0, gt_qpad = 0, gt_ks = 0;
};
