// kernels.hpp -- host-side launchers for the gfx950 kernels (k_prep.hip, k_filter.hip,
// k_exact.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bsr {

// Layout constants shared by the host orchestration and the kernels.
constexpr uint32_t kLdAlign = 64;      // f32 row leading dimension multiple (elements)
constexpr uint32_t kRowPad = 256;      // rows are padded to a multiple of this (zero rows)
constexpr uint32_t kScanQF = 8;        // queries per exact-scan launch (max)
constexpr uint32_t kSampleStride = 32; // candidate-threshold sample: every 32nd row
constexpr uint32_t kQuantBlock = 32;   // rows sharing one int8 scale (one 32-row MFMA block)
constexpr uint32_t kSampleScaleRows = 128; // int8 sample rows sharing one scale (one filter tile)
constexpr uint32_t kFilterTile = 256;  // MFMA filter tile: 256 corpus rows x 256 queries

// Row-state flags (index load).
constexpr uint32_t kRowNonFinite = 1u;  // a NaN/Inf element
constexpr uint32_t kRowNormOvf = 2u;    // sum of squares overflowed
constexpr uint32_t kRowNormRange = 4u;  // nonzero norm outside [1e-18, 1e18]: no MFMA stage

// Query flags.
constexpr uint32_t kQueryNonFinite = 1u;
constexpr uint32_t kQueryNoApprox = 2u;   // norm zero/tiny/huge: answered by the exact scan

// Search status words (device, one small D2H copy per search).
enum StatusWord : uint32_t { kStFail = 0, kStEmitted = 1, kStQueryFlags = 2, kStFail2 = 3, kStWords = 4 };

// ---- data movement / load-time preparation (k_prep.hip) -------------------------------
hipError_t launch_synth_uniform(float* out, uint64_t row0, uint64_t n_rows, uint32_t dim,
                                uint32_t ld, uint64_t seed, hipStream_t s);
hipError_t launch_copy_rows_f32(const float* src, uint64_t n, uint32_t dim, uint32_t ld,
                                float* dst, hipStream_t s);
hipError_t launch_widen_bf16_rows(const uint16_t* src, uint64_t n, uint32_t dim, uint32_t ld,
                                  float* dst, hipStream_t s);
hipError_t launch_row_norms(const float* rows, uint64_t n, uint32_t dim, uint32_t ld,
                            float* na, uint32_t* flags, hipStream_t s);
// int8 filter operand: per 32-row block scale s (127*s >= max |a_i|/|a| over the block),
// q_i = rint(a_i/(|a| s)); ea_max (u32 bits of a non-negative float, atomicMax) receives
// an upper bound of max_row || a/|a| - s q ||_2.
hipError_t launch_rows_to_i8(const float* rows, uint64_t n, uint64_t n_pad, uint32_t dim,
                             uint32_t ld, int8_t* out, float* scales, uint32_t* ea_max,
                             hipStream_t s);
// The sample pass's operand: rows 0, kSampleStride, 2 kSampleStride, ... of the corpus,
// contiguous, int8 with one scale per kSampleScaleRows of them (the sample pass only sets the
// emission threshold; no certification depends on its quantization).  out: [n_s_pad][ld],
// scales: [n_s_pad / kSampleScaleRows], n_s_pad = round_up(n_s, kSampleScaleRows).
hipError_t launch_rows_to_i8_sample(const float* rows, uint64_t n, uint32_t dim, uint32_t ld,
                                    int8_t* out, float* scales, hipStream_t s);
// Query preparation: exact |b| (src/metrics.rs:155), flags, padded f32 copy, the filter
// operand (int8 + scale) and the per-query certification bound ebound[q].
struct QueryPrepArgs {
    const float* q;        // caller's queries [nq][dim]
    uint32_t nq, qpad, dim, ld;
    const uint32_t* ea_max;  // row-side error bound (device word)
    float* qf32;           // [qpad][ld]
    float* nb;             // [qpad]
    void* qop;             // int8 [qpad][ld]
    float* qscale;         // [qpad]
    float* ebound;         // [qpad]
    uint32_t* qflags;      // [qpad]
    int32_t* qids;         // [qpad]: min(q, nq-1), the exact scan's query-id list
    uint32_t* status;      // kStQueryFlags word receives the OR of the flags
    bool with_op;          // build the filter operand (false: exact scan only)
};
hipError_t launch_query_prep(const QueryPrepArgs& a, hipStream_t s);
// The parallel search's header exchange without host copies: this rank's 8 words into the device
// send buffer; the P received headers into fine-grained pinned host memory, then host_flag = seq
// (system-scope release) -- the host polls the flag.
hipError_t launch_header_put(const int32_t w[8], int32_t* dst, hipStream_t s);
hipError_t launch_header_publish(const int32_t* src, uint32_t words, int32_t* host, uint32_t* host_flag, uint32_t seq,
                                 hipStream_t s);
// The loopback communicator's all-gather: recv[r] = script[r] (a recorded contribution of a real
// P-rank run) for r != rank, this rank's send otherwise (every slot when script is null).
hipError_t launch_gather_emulate(const void* send, const void* script, void* recv, uint64_t bytes, uint32_t P,
                                 uint32_t rank, hipStream_t s);

// Mask bitsets, one kernel family.  An allow mask: bit (i & 63) of word (i >> 6)
// allows local row i; bits at positions >= n are ignored; allow = nullptr allows every row < n.
// dead (nullable): the index's bitset of deleted rows -- every kernel forms allow[w] & ~dead[w] as
// it reads, no copy of a mask is made.  A mask's row list is built in two steps around the host's
// read of the count: blk [mask_blocks(n) + 1] receives the exclusive prefix sums of the per-block
// popcounts and, in its last word, the number of allowed live rows A (two launches); the scatter
// then writes the first n_list of the A ids in ascending order.
constexpr uint32_t kMaskBlockWords = 256;  // mask words per workgroup of the list build
static inline uint32_t mask_blocks(uint64_t n) {
    const uint64_t words = (n + 63) / 64, b = (words + kMaskBlockWords - 1) / kMaskBlockWords;
    return (uint32_t)(b < 1 ? 1 : b);
}
hipError_t launch_mask_list_count(const uint64_t* allow, const uint64_t* dead, uint64_t n, uint32_t* blk,
                                  hipStream_t s);
hipError_t launch_mask_list_scatter(const uint64_t* allow, const uint64_t* dead, uint64_t n, const uint32_t* blk,
                                    uint32_t n_list, uint32_t* list, hipStream_t s);

// The same for n_masks allow masks of `words` = ceil(n / 64) words each, allow[g * words ..] (the
// grouped masked search), and query_mask[q] < n_masks naming query q's.
// The counts, two launches: blk[g * (mask_blocks(n) + 1) ..] receives mask g's exclusive block
// prefixes; out[g] = A_g, the rows mask g allows, and -- query_mask given -- out[n_masks] = the
// entries of query_mask[0 .. nq) that name no mask (>= n_masks; no kernel indexes a mask with one).
hipError_t launch_mask_groups_count(const uint64_t* allow, uint64_t words, uint32_t n_masks, uint64_t n,
                                    const uint64_t* dead, const uint32_t* query_mask, uint32_t nq, uint32_t* blk,
                                    uint32_t* out, hipStream_t s);
// One list per entry of d[0 .. n_lists) (device): the first d[y].n_list ids of mask d[y].mask,
// ascending, at list + d[y].off.
struct MaskListDesc { uint64_t off; uint32_t mask, n_list; };
hipError_t launch_mask_groups_scatter(const uint64_t* allow, uint64_t words, uint64_t n, const uint64_t* dead,
                                      const uint32_t* blk, const MaskListDesc* d, uint32_t n_lists, uint32_t* list,
                                      hipStream_t s);
// The emitted lists cut by query q's mask, allow + query_mask[q] * words (query_mask = nullptr: mask
// 0 for every query), less the deleted rows: cand[q][0 .. cnt[q]) compacted in place to the keys of
// allowed live rows and cnt[q] rewritten (an overflowed list, cnt[q] > cap, is left overflowed);
// raw[q] = the emitted count; *items = nq.
hipError_t launch_mask_cut(uint64_t* cand, uint32_t* cnt, uint32_t cap, uint32_t nq, const uint64_t* allow,
                           uint64_t words, const uint32_t* query_mask, const uint64_t* dead, uint64_t n, uint32_t* raw,
                           uint32_t* items, hipStream_t s);
// A query group of the grouped list scan (launch_scan_list_groups): its list and its own queries.
struct ScanGroupDesc { uint64_t off; uint32_t n_list, nq; };

// Tombstones.  dead: the index's bitset of deleted rows, bit (i & 63) of word
// (i >> 6) set = local row i is deleted; no bit at a position >= n is ever set.
// *bad += the ids outside [lo, lo + n).
hipError_t launch_dead_check(const uint64_t* ids, uint64_t n_ids, uint64_t lo, uint64_t n, uint32_t* bad,
                             hipStream_t s);
// The bits of rows ids[i] - lo set (atomicOr); *newly += the rows whose bit was clear before.
hipError_t launch_dead_apply(const uint64_t* ids, uint64_t n_ids, uint64_t lo, uint64_t n, uint64_t* dead,
                             uint32_t* newly, hipStream_t s);
// Zeros over the fop row of every deleted row: it scores exactly 0 in every filter kernel.  The
// fop_s row of every kSampleStride-row block with a deleted row becomes the operand of the block's
// live row whose rank among the live rows is a multiple of kSampleStride, or zeros when it has
// none: the sample is the live rows thinned 1 in kSampleStride (rows: the f32 slab
// [n_pad][row_bytes]; scales_s: the sample operand's scales, kept; dead_blk
// [mask_blocks(n) + 1]: launch_mask_list_count of dead as the mask).  row_bytes = ld, a multiple of 64.
hipError_t launch_dead_zero_fop(const uint64_t* dead, uint64_t n, const uint32_t* dead_blk, uint32_t row_bytes,
                                uint8_t* fop, uint8_t* fop_s, const float* rows, uint32_t dim, const float* scales_s,
                                hipStream_t s);

// In-place update (bsr_index_update): n_ids incoming rows src [n_ids][dim] (f32, or
// bf16 bits) replace the slab rows ids[j] - lo.  Every kernel is driven by the ids or by a list
// built from them: none walks the shard's rows.
// The check writes only its own scratch: the bits of the named rows in `touched` (ceil(n / 64)
// words), of their 32-row blocks in `blocks` and of the fop_s sample groups (kSampleScaleRows
// sampled rows = 4,096 corpus rows) whose sampled row is named in `groups`, all zeroed by the
// caller, and the four counts of cnt (u64, zeroed by the caller).
enum UpdCount : uint32_t { kUpdBadId = 0, kUpdDupId = 1, kUpdNonFinite = 2, kUpdSampleRows = 3, kUpdCounts = 4 };
hipError_t launch_upd_check(const uint64_t* ids, uint64_t n_ids, uint64_t lo, uint64_t n, const void* src,
                            uint32_t dim, bool bf16, uint64_t* touched, uint64_t* blocks, uint64_t* groups,
                            uint64_t* cnt, hipStream_t s);
// rows[ids[j] - lo][0 .. ld) = src[j] widened exactly, zeros past dim (the ids checked: in range, distinct).
hipError_t launch_upd_scatter(const uint64_t* ids, uint64_t n_ids, uint64_t lo, const void* src, uint32_t dim,
                              uint32_t ld, bool bf16, float* rows, hipStream_t s);
// launch_row_norms over the rows ids[j] - lo alone: na[row], the flags OR-ed into flags[0].
hipError_t launch_upd_row_norms(const float* rows, const uint64_t* ids, uint64_t n_ids, uint64_t lo, uint32_t dim,
                                uint32_t ld, float* na, uint32_t* flags, hipStream_t s);
// launch_rows_to_i8 / launch_rows_to_i8_sample for the *count blocks / groups list[0 .. *count)
// (count on the device; cap >= *count workgroups are launched).  What a block or group receives is
// what the load's kernel writes for it: the same device function.
hipError_t launch_upd_rows_to_i8(const float* rows, uint64_t n, uint32_t dim, uint32_t ld, int8_t* out, float* scales,
                                 uint32_t* ea_max, const uint32_t* list, const uint32_t* count, uint32_t cap,
                                 hipStream_t s);
hipError_t launch_upd_rows_to_i8_sample(const float* rows, uint64_t n, uint32_t dim, uint32_t ld, int8_t* out,
                                        float* scales, const uint32_t* list, const uint32_t* count, uint32_t cap,
                                        hipStream_t s);

// Compaction (bsr_index_compact).  out[j][0 .. ld) = rows[list[j]][0 .. ld) for
// j < cnt: slab rows gathered, packed, into ANOTHER buffer (out must not overlap rows: list[j] >= j
// makes an in-slab gather a race; the host moves chunks through a staging buffer in stream order).
// ld % kLdAlign == 0; the grid is sized by the device.
hipError_t launch_compact_gather(const float* rows, const uint32_t* list, uint64_t cnt, uint32_t ld, float* out,
                                 hipStream_t s);
// out[j] = lo + list[j] for j < cnt (out nullable; list = nullptr: the identity), and *first =
// min(*first, the lowest j with list[j] != j) -- preset *first to ~0.
hipError_t launch_compact_ids(const uint32_t* list, uint64_t cnt, uint64_t lo, uint64_t* out, uint32_t* first,
                              hipStream_t s);

// ---- MFMA candidate filter (k_filter.hip) ---------------------------------------------
struct GemmArgs {
    const uint8_t* A;       // filter rows [n_pad][row_bytes]
    uint64_t a_stride;      // bytes between consecutive tile rows (row_bytes, or x sample stride)
    uint32_t n_rows;        // valid tile rows (n for emit, n_sample for the sample pass)
    uint32_t a_scale_rows;  // int8: tile rows per a_scale entry (kQuantBlock emit, kSampleScaleRows sample)
    const uint8_t* B;       // filter queries [qpad][row_bytes]
    uint32_t row_bytes;     // bytes of one operand row (multiple of 64)
    uint32_t n_rt, n_qt;    // row tiles, query tiles
    const float* a_scale;   // i8: [n_pad / 32] block scales
    const float* b_scale;   // i8: [qpad] query scales
    float* S;               // sample: scores [qpad][s_ld]
    uint32_t s_ld;
    uint32_t s_compact;     // sample: 1 = one maximum per 32 sampled rows, 0 = every score
    const float* tau;       // emit: per-query threshold
    uint64_t* cand;         // emit: [qpad][cap] score keys
    uint32_t* cnt;          // emit: [qpad] counters
    uint32_t cap;
    // emit, int8 query-stationary kernel: all but the last 1/kTailDiv of its 128-row tiles go
    // to the workgroups' row streams round-robin, the rest are claimed one at a time per query
    // tile from tail[qt] (zeroed by k_select_tau); tail = nullptr: every tile static
    uint32_t* tail;
    // skinny TOP: the search's status words (zeroed by the kernel: no k_select_tau runs) and
    // the batch's query count (padding queries keep no list)
    uint32_t* status;
    uint32_t n_q;
    uint32_t top_layout;  // the skinny TOP row layout: 2 = the product strided pairs (0: lab, k_filter.hip)
    // Sample tiles (int8 query-stationary kernel, compact sample; 0 = off): the sample is the
    // s_tiles 128-row tiles 32 L + kSampleTilePhase of A itself, scored once -- the sample pass
    // reads them with the emit scales (S[q][4 L + g] = the exact maximum emit score of the tile's
    // g-th 32-row block), the emit pass walks the other tiles, and launch_sample_fixup emits the
    // sample tiles' rows.  s_vals: the values of S per query that hold a valid row.
    uint32_t s_tiles, s_vals;
};
constexpr uint32_t kSampleTileEvery = 32;  // one 128-row tile in 32 is a sample tile ...
constexpr uint32_t kSampleTilePhase = 31;  // ... the last of each 32
// Sample tiles of a shard of n rows: floor(ceil(n / 128) / 32).
static inline uint32_t sample_tiles_for(uint64_t n) { return (uint32_t)(((n + 127) / 128) / kSampleTileEvery); }
// Dynamic tail of the emit filter: 1/kTailDiv of the row tiles; counters per (XCD pool, query
// tile) (<= kTailCounters query tiles) after the per-query counters, cnt[qpad + x * n_qt + qt].
constexpr uint32_t kTailDiv = 8;
constexpr uint32_t kTailCounters = 64;
// Row-stream gangs of the emit filter (GANG > 0): one 64-bit progress word per row stream (its
// n_qt <= 4 workgroups' static tile counts, 16 bits each) after the tail counters,
// cnt[qpad + 8 * kTailCounters ...], zeroed with them.
constexpr uint32_t kGangWords = 2 * 256;
// (static tiles per row stream: gangs from ~5.6M rows at 1000 queries.  Round 5, the filter
// builds in one process at the global threshold's rate: the gang build 2.4% slower than the
// small-shard build at 2.5M rows, 0.8% at 5M, 0-1% faster at 10M -- profiles/r05hm_hist_*,
// r05e_hist_10m.txt; the threshold was 256, ~2.5M rows)
constexpr uint32_t kGangMinTiles = 600;
// The 768-byte gang build's emission queue: records per wave (one record = the 32 integer values
// of one lane's query block on one tile; at most 64: the flush takes one record per lane).  32, 48
// and 64 timed in one process at 10M rows lie within the run's spread of each other
// (profiles/r10_emit_queue.txt); a wave queues ~125 records per launch at the bench's rate.
constexpr int kEmitQueueDepth = 48;
hipError_t launch_filter_sample(const GemmArgs& a, hipStream_t s);
hipError_t launch_filter_emit(const GemmArgs& a, hipStream_t s);
// The 768-byte gang build k_filter_qs16<true, 12, true> whatever the shard size (the kernel-level
// tests' entry; 768-byte rows only).  Below kGangMinTiles static tiles per row stream no workgroup
// runs in a gang, so the throttle is idle and the launch emits what launch_filter_emit emits.
hipError_t launch_filter_emit_gang(const GemmArgs& a, hipStream_t s);
// The sample tiles' share of the emission (a.s_tiles != 0; after the threshold is final, before
// the rescore): for every query q < a.n_q and sample value S[q][j] >= tau[q] (ties included),
// the 32 rows of that block are scored as the emit pass scores them and those reaching tau[q]
// are appended to the query's list (the emit pass's keys, counters and overflow behaviour).
// A query with tau = +inf (flagged, padding) emits nothing.
hipError_t launch_sample_fixup(const GemmArgs& a, hipStream_t s);
// int8 only, batches of <= 16 queries (query tile rows 0..15), HBM-bound: the same
// contract as the two launches above.
constexpr uint32_t kSkinnyMaxQ = 16;
hipError_t launch_filter_skinny_sample(const GemmArgs& a, hipStream_t s);
hipError_t launch_filter_skinny_emit(const GemmArgs& a, hipStream_t s);
// The self-thresholded single-query path (round 6; rows of <= 16 K slices): no sample pass and no
// tau0 -- each of the skinny2 grid's W = skinny_top_lists(n) workgroups writes its 4 best keys per
// query to cand[q][W][4] (ascending; every other row of the workgroup scores at most the 4th), and
// cnt[q] = 4 W for q < 16; the status words kStFail / kStEmitted / kStFail2 are zeroed.
hipError_t launch_filter_skinny_top(const GemmArgs& a, hipStream_t s);
uint32_t skinny_top_lists(uint32_t n_rows);
bool skinny_glds_on();  // the LDS-DMA skinny filter for 768-byte rows (BSR_SKINNY_GLDS=0: off; read per call)
// Shards of at least this many rows take the self-thresholded path for batches of <= 16 queries
// and k' <= 63 (every wave of the 512-workgroup grid then holds >= 64 units of 16 rows).
constexpr uint64_t kSkinnyTopMinRows = 2u << 20;

// tau[q] = the ks-th best sampled score (ks <= 128); also zeroes cnt[0..qpad) and the status
// words kStFail / kStEmitted / kStFail2 for the emit pass and rescores that follow.
// smax (optional): the query's ks best sample keys [qpad][ks] (kKeyNone where there are none),
// the input of the global threshold of a parallel search.
// ks_q (optional, [qpad], grouped masked search): query q's own depth ks_q[q] <= ks (ks then only
// picks the kernel's width); ks_q[q] = 0: tau[q] = +INFINITY, the query emits nothing.  No smax.
hipError_t launch_select_tau(const float* S, uint32_t s_ld, uint32_t n_s, uint32_t nq,
                             uint32_t qpad, const uint32_t* qflags, uint32_t ks, float* tau,
                             uint32_t* cnt, uint32_t* status, hipStream_t s, uint64_t* smax = nullptr,
                             const uint32_t* ks_q = nullptr);
// tau[q] = the ks-th best of the all-gathered sample keys g[P][qpad][ks] (parallel search,
// DESIGN.md §6); INFINITY for padding / no-filter queries.
hipError_t launch_global_tau(const uint64_t* g, uint32_t P, uint32_t qpad, uint32_t nq, uint32_t ks,
                             const uint32_t* qflags, float* tau, hipStream_t s);
// The k' = kp best emitted candidates (rows) and tau_excl = the (kp+1)-th score, for lists
// larger than kFusedSelectCap (smaller ones are selected inside the rescore).
hipError_t launch_select_cand(const uint64_t* cand, const uint32_t* cnt, uint32_t cap,
                              uint32_t nq, const float* tau, uint32_t kp, uint32_t* cand_rows,
                              uint32_t* ncand, float* tau_excl, hipStream_t s);

// ---- exact arithmetic (k_exact.hip) ---------------------------------------------------
// Exact rescoring of candidates + certification (one wave per query, or device-counted
// 8-wave workgroups for the second chance).
struct RescoreArgs {
    const float* rows;          // f32 [n_pad][ld]
    uint32_t ld, dim;
    const float* na;            // row magnitudes
    const float* qf32;          // queries [qpad][ld]
    const float* nb;            // query magnitudes
    uint32_t n_items;           // queries to process (the grid), or the bound on *n_items_dev
    const uint32_t* n_items_dev;  // non-null: the item count is read on the device (a status
                                  // word written by an earlier kernel of the same stream)
    const uint32_t* qlist;      // query id of item b (nullptr: b)
    // mode A, the k' selected candidates: cand_rows[q*kp + i], i < ncand[q]; tau_excl[q]
    const uint32_t* cand_rows;
    const uint32_t* ncand;
    uint32_t kp;
    const float* tau_excl;
    // mode B (cand_keys != nullptr), every emitted candidate: key_row(cand_keys[q*cap + i]),
    // i < cnt[q] <= cap (an overflowed list fails); certified against tau0[q]
    const uint64_t* cand_keys;
    const uint32_t* cnt;
    uint32_t cap;
    const float* tau0;
    // mode S (sel != 0, one-wave launch, cap <= 1024): the k' candidates selected in the
    // rescore kernel itself from cand_keys / cnt (radix select; tau_x = the (k'+1)-th score,
    // or tau0 when fewer were emitted) -- k_select_cand is not launched
    uint32_t sel;
    // mode S of the self-thresholded single-query path (top_w != 0; the tiny-batch kernel
    // k_rescore_kp only): cand_keys[q * cap ..] holds top_w ascending 4-lists (cap = 4 top_w <=
    // 64 kTopKeysPerLane, launch_filter_skinny_top); its wave 0 radix-selects the k' best of them.  The bound on the rows outside the lists -- the best score among the
    // lists' 4th keys -- goes to top_tau[q], and the keys above it are compacted to the front of
    // the query's list, their count to top_cnt[q]: the second chance's mode-B input (a query the
    // filter cannot serve: count 0, bound +inf).
    uint32_t top_w;
    const uint32_t* qflags;
    float* top_tau;
    uint32_t* top_cnt;
    uint32_t k;
    const float* ebound;        // per-query certification bound E_q
    uint64_t* out_keys;         // [nq][k]
    uint32_t* fail_cnt;         // uncertified queries: count (a status word) and list
    uint32_t* fail_list;
    // Fused finalize (the filter path: no k_finalize launch): the list of a query becomes its
    // (global index, distance) result rows here -- modes S / A for the certified queries, mode
    // B for every item it rescored (the uncertified ones are rewritten after the exact scan).
    uint64_t* res_idx;          // [nq][k] (nullptr: no fused finalize)
    float* res_dist;
    uint32_t* res_cnt;          // [nq]
    uint64_t offset, n_rows;    // global index of local row 0; the shard's live rows (count = min(k, n_rows))
    // Tombstones (k_rescore, k_rescore_kp): the index's bitset of deleted rows --
    // a candidate whose bit is set offers no key.  nullptr: no row of the index is deleted.
    // (Not with excl_out: k_rescore_flat does not read it, and launch_rescore refuses the pair.)
    const uint64_t* dead;
    // (optional) the host mirror of the same rows (fine-grained pinned memory): every result row
    // is written there too, by the wave that finalizes it, so the publish copies only the status
    // words (the standard path; the global-threshold path publishes its whole buffer)
    uint64_t* hres_idx;
    float* hres_dist;
    uint32_t* hres_cnt;
    // mode B: block 0 also zeroes the NEXT search's status words and sums the emitted counts
    // into cur_status[kStEmitted] (what k_finalize does on the other paths)
    uint32_t* next_status;
    const uint32_t* emit_cnt;
    uint32_t* cur_status;
    uint32_t n_queries;
    // Parallel search with a global threshold (mode B, one wave per query): no
    // local certification -- every query's list of its rescored emitted rows becomes its
    // result (count = min(k, rows rescored)) and excl_out[q] receives the distance below which
    // no row left out can lie (1 - tau0 - E_q - 2.5e-7 rounded down; -inf when nothing can be
    // certified, +inf when every row was a candidate); the root certifies the merged lists.
    float* excl_out;
    // (optional, block 0) the parallel search merge's two words, set before its launch:
    // merge_words[0] = 0 (uncertified count), merge_words[1] = ~0 (lowest query with a NaN)
    uint32_t* merge_words;
    // Publish (optional, the batch's last kernel): the workgroup that finishes last copies
    // pub_bytes of the packed result buffer pub_src to host memory pub_dst (fine-grained pinned)
    // and then sets *pub_flag = 1 with a system-scope release, so the host sees the result
    // without waiting for the stream's completion signal and without a D2H copy node.
    // (pub_bytes: a multiple of 16 -- the copy moves whole 16-byte units and drops a remainder.)
    const uint8_t* pub_src;
    uint8_t* pub_dst;
    size_t pub_bytes;
    uint32_t* pub_flag;
    uint32_t* pub_ticket;       // kTicketWords device words, 0 between launches
    uint32_t solo;              // (set by launch_rescore) a one-workgroup grid: its own last arrival
};
// The publishing kernels' arrival ticket: kTicketLeaves leaf counters and one root counter,
// each on a 64-byte line of its own (a workgroup adds to its leaf, blockIdx % kTicketLeaves; the
// last of a leaf adds to the root), all zero between launches.
constexpr uint32_t kTicketLeaves = 8, kTicketStride = 16, kTicketWords = (kTicketLeaves + 1) * kTicketStride;
// Workgroups of the device-counted rescore (failed certifications, usually a few queries).
constexpr uint32_t kRescoreAllGrid = 128;
// Candidate lists up to this many keys (k <= 10) are selected inside the rescore kernel.
constexpr uint32_t kFusedSelectCap = 1024;
// The candidate stage's sizes for a top-k: k' candidates per query, lists of cap keys, the
// threshold's depth ks in the sample.
static inline uint32_t kp_for(uint32_t k) { return 64u * ((3u * k + 34u + 63u) / 64u) - 1u; }
static inline uint32_t cap_for(uint32_t k) { return 16u * (kp_for(k) + 1u); }
static inline uint32_t ks_for(uint32_t k) { return (kp_for(k) + 1u) / 8u; }
hipError_t launch_rescore(const RescoreArgs& a, hipStream_t s);
// whether launch_rescore takes k_rescore_kp for a tiny batch's first pass (BSR_RESCORE_KP != 0)
bool rescore_kp_enabled();
// The self-thresholded path's lists per query are selected by one wave, this many keys per lane.
constexpr uint32_t kTopKeysPerLane = 32;
// Exact full scan for up to kScanQF queries (ids in qids, device).  part must hold
// grid * kScanQF * k keys.
hipError_t launch_scan_exact(const float* rows, uint32_t ld, uint32_t dim, uint64_t n,
                             const float* na, const float* qf32, const int32_t* qids,
                             uint32_t nqf, const float* nb, uint32_t k, uint32_t grid,
                             uint64_t* part, hipStream_t s);
hipError_t launch_merge_parts(const uint64_t* part, uint32_t grid, const int32_t* qids,
                              uint32_t nqf, uint32_t k, uint64_t* out_keys, hipStream_t s);
// Exact top-k over a row list (masked search): the n_list rows list[0 .. n_list) of the slab
// (local ids, each < n), gathered whole, for `groups` groups of queries in one launch -- group g
// takes the ids qids[g * kScanQF ..] and writes its partial lists to part + g * grid * kScanQF * k
// (launch_merge_parts' layout).  groups > 1 needs nqf == kScanQF; n_list >= 1.
hipError_t launch_scan_list(const float* rows, uint32_t ld, uint32_t dim, const uint32_t* list,
                            uint32_t n_list, const float* na, const float* qf32, const int32_t* qids,
                            uint32_t nqf, uint32_t groups, const float* nb, uint32_t k, uint32_t grid,
                            uint64_t* part, hipStream_t s);
// The root's merge of gathered [P][nq][k_in] lists (counts [P][nq]) into [nq][k] outputs on
// the device (compute_global_top_k); P <= 64, P * k_in <= kMergeMaxEntries, k <= 256.
// *first_nan must hold ~0 before the launch; afterwards the lowest query with a NaN distance.
constexpr uint32_t kMergeMaxEntries = 1024;
hipError_t launch_merge_lists(const uint64_t* idx, const float* dist, const uint32_t* cnt, uint32_t P, uint32_t nq,
                              uint32_t k_in, uint32_t k, uint64_t* out_idx, float* out_dist, uint32_t* out_count,
                              uint32_t* first_nan, hipStream_t s);
// The general form: strided lists (the all-gathered packed result buffers of a parallel search)
// and, with excl, the certification of a global-threshold search.
struct MergeArgs {
    const uint64_t* idx;        // list l of query q: idx + l * idx_stride + q * k_in
    const float* dist;          // dist + l * dist_stride + q * k_in
    const uint32_t* cnt;        // cnt[l * cnt_stride + q]
    uint64_t idx_stride, dist_stride, cnt_stride;
    uint32_t P, nq, k_in, k;
    uint64_t* out_idx;          // [nq][k]
    float* out_dist;
    uint32_t* out_count;        // [nq]
    uint32_t* first_nan;        // ~0 before the launch
    // certification (optional): list l's exclusion bounds excl[l * excl_stride + q]; a query
    // is certified iff its merged list holds need = min(k, corpus rows) entries and the k-th
    // distance is below every bound -- the others are appended to fail_list / *fail_cnt
    const float* excl;
    uint64_t excl_stride;
    uint32_t need;
    uint32_t* fail_cnt;
    uint32_t* fail_list;
    // (optional) each list's kStWords status words, st[l * st_stride + w] -> st_all[l][w]
    const uint32_t* st;
    uint64_t st_stride;
    uint32_t* st_all;
    // (optional) the host mirror of out_idx / out_dist / out_count: the merged rows are written
    // there too, by the wave that merges them (pub_bytes then covers the part before them)
    uint64_t* hout_idx;
    float* hout_dist;
    uint32_t* hout_count;
    // (optional) publish the merged result buffer to host memory, as RescoreArgs::pub_*
    const uint8_t* pub_src;
    uint8_t* pub_dst;
    size_t pub_bytes;
    uint32_t* pub_flag;
    uint32_t* pub_ticket;
    uint32_t force_hash;  // (lab, set by launch_merge from BSR_MERGE_HASH) no disjoint-lists shortcut
    // every list is one search's own top-k (no index twice within a list): lists whose index ranges
    // are pairwise disjoint then skip the first-occurrence filter
    uint32_t lists_unique;
};
hipError_t launch_merge(const MergeArgs& a, hipStream_t s);
// Keys -> (global index, distance) rows; also zeroes `status`, the status words of the
// result buffer the next search will use.
// status: the NEXT search's status words (zeroed); emit_cnt (optional): per-query emitted
// counts, summed into cur_status[kStEmitted].
// n_q (optional): query q's rows are counted against n_q[q] instead of n (grouped masked search).
hipError_t launch_finalize(const uint64_t* keys, uint32_t nq, uint32_t k, uint64_t n,
                           uint64_t offset, uint64_t* out_idx, float* out_dist,
                           uint32_t* out_count, uint32_t* status, const uint32_t* emit_cnt,
                           uint32_t* cur_status, hipStream_t s, const uint32_t* n_q = nullptr);
// The grouped masked search's list scan: launch_scan_list with a list per query
// group -- group y (blockIdx.y) scans the grp[y].n_list ids at list + grp[y].off for the qf
// queries qids[y * qf ..] (qf one of 1, 2, 4, 8; the first grp[y].nq are the group's own, the rest
// padding with ids of the same mask) and writes its partial lists to part + y * grid * qf * k.
// grid: scan_grid_for(the launch's longest list); a workgroup without a tile in its group's list
// writes empty partial lists.  launch_merge_parts_groups merges every group's lists in one launch
// into out_keys[id] for the group's own queries.
hipError_t launch_scan_list_groups(const float* rows, uint32_t ld, uint32_t dim, const uint32_t* list,
                                   const ScanGroupDesc* grp, uint32_t groups, uint32_t qf, const float* na,
                                   const float* qf32, const int32_t* qids, const float* nb, uint32_t k,
                                   uint32_t grid, uint64_t* part, hipStream_t s);
hipError_t launch_merge_parts_groups(const uint64_t* part, uint32_t grid, const int32_t* qids, uint32_t qf,
                                     const ScanGroupDesc* grp, uint32_t groups, uint32_t k, uint64_t* out_keys,
                                     hipStream_t s);
hipError_t launch_cosine_pair(const float* a, uint32_t la, const float* b, uint32_t lb,
                              float* out, hipStream_t s);

// ---- range search (bsr_local_range_search; k_exact.hip) -----------------------
// The emitted lists of a range search of `capacity` result slots per query: twice the capacity,
// at least 1024 and at most 8192 keys, a multiple of 64.  (8192 keys are 64 KB: a list fits the
// 160 KB LDS of a gfx950 CU next to the finish kernel's own 32 KB; the sort itself only ever holds
// capacity <= 4096 keys.)
constexpr uint32_t kRangeMaxResults = 4096;
static inline uint32_t range_cap(uint32_t capacity) {
    const uint32_t c = 2u * capacity < 1024u ? 1024u : 2u * capacity > 8192u ? 8192u : 2u * capacity;
    return (c + 63u) / 64u * 64u;
}
// OR-ed into the kStQueryFlags status word by launch_range_tau: a radius of the batch is NaN.
constexpr uint32_t kRangeNanRadius = 0x100u;
// The emission threshold from the radius, before the filter runs (it takes k_select_tau's place):
// tau[q] = the largest f32 t (to within a few ulps) with exclusion_bound(t, ebound[q], nb[q]) >
// radius[q], so every row the filter does not emit lies outside the radius.  A query that cannot
// filter -- kQueryNoApprox, ebound >= 1, or a threshold <= 0 -- gets tau = +inf and is appended to
// scan_list (status[kStFail] counts the list, status[kStFail2] these queries); radius < 0 and
// padding queries get +inf and no scan; a NaN radius gets +inf, no scan and kRangeNanRadius.
// Also zeroes what k_select_tau zeroes for the emit pass -- cnt[0 .. qpad), the tail counters and
// gang words behind them, the status words kStFail / kStEmitted / kStFail2 (before it counts into
// them) -- and the range counts rcnt[0 .. nq).  One workgroup.
hipError_t launch_range_tau(const float* radius, const float* ebound, const float* nb, const uint32_t* qflags,
                            uint32_t nq, uint32_t qpad, float* tau, uint32_t* cnt, uint32_t* rcnt,
                            uint32_t* scan_list, uint32_t* status, hipStream_t s);
// What the range kernels share: the exact operands, the radii, the per-query lists keys [nq][cap]
// of distance keys (in arbitrary order) and their counts rcnt [nq].
struct RangeArgs {
    const float* rows;          // f32 [n_pad][ld]
    uint32_t ld, dim;
    uint64_t n;                 // rows of the shard (the scan)
    const float* na;            // row magnitudes (read, never recomputed)
    const float* qf32;          // queries [qpad][ld]
    const float* nb;            // query magnitudes
    const float* radius;        // [nq]
    const uint64_t* dead;       // the bitset of deleted rows (nullable)
    uint64_t* keys;             // [nq][cap]
    uint32_t* rcnt;             // [nq]
    uint32_t cap;
    uint32_t nq;
    // the rescore: the emitted score keys cand [qpad][cap] and their counts cnt; a query with
    // cnt[q] > cap appends itself to scan_list / status[kStFail] and writes nothing
    const uint64_t* cand;
    const uint32_t* cnt;
    uint32_t* scan_list;
    uint32_t* status;           // also: status[kStEmitted] = the sum of cnt[0 .. nq)
    // the scan: the ids of the launch's nqf <= kScanQF queries (device; entries up to the template
    // width -- 1, 2, 4 or 8 -- must be valid ids, those past nqf count nothing)
    const int32_t* qids;
    uint32_t nqf;
    // the rescore behind a mask cut (optional): the emitted counts before the cut, summed into
    // status[kStEmitted] in cnt's place
    const uint32_t* emit_cnt;
};
// One workgroup per query over its emitted rows: the reference distance of every listed row; the
// live rows with d <= radius[q] become the query's list, their number rcnt[q].
hipError_t launch_range_rescore(const RangeArgs& a, hipStream_t s);
// The exact fallback, the exact scans' tile loop: every valid live row with d <=
// radius claims a slot of its query's list by an atomic add on rcnt[id] (zero before the launch)
// and stores its key when the slot is below cap; the count stays exact beyond that.
hipError_t launch_range_scan(const RangeArgs& a, uint32_t grid, hipStream_t s);
// One workgroup per query: a list of rcnt[q] <= capacity keys sorted ascending (distance, then
// row) into out_idx / out_dist [nq][capacity] as (offset + row, distance), (~0, +inf) behind them;
// a longer list: (~0, +inf) in every slot.  out_count[q] = rcnt[q] either way.
hipError_t launch_range_finish(const uint64_t* keys, const uint32_t* rcnt, uint32_t cap, uint32_t nq,
                               uint32_t capacity, uint64_t offset, uint64_t* out_idx, float* out_dist,
                               uint32_t* out_count, hipStream_t s);

// ---- scoring caller-chosen rows (bsr_local_score_ids / bsr_local_rerank_ids) -----
// The longest list the rerank sorts (a list is sorted in LDS, as a range result is).
constexpr uint32_t kScoreMaxIds = 4096;
static_assert(kScoreMaxIds == kRangeMaxResults, "k_score_finish sorts with the range finish's network");
// Per query q a list ids[q][0 .. m) of GLOBAL ids.  A slot is present when its id lies in [offset,
// offset + n) and its row has no tombstone; no address is formed from an id outside that interval.
struct ScoreArgs {
    const float* rows;          // f32 [n_pad][ld]
    uint32_t ld, dim;
    uint64_t n, offset;         // rows of the shard, the shard's global offset
    const float* na;            // row magnitudes (read, never recomputed)
    const float* qf32;          // queries [qpad][ld]
    const float* nb;            // query magnitudes
    const uint64_t* dead;       // the bitset of deleted rows (nullable)
    const uint64_t* ids;        // [nq][m]
    uint32_t m, nq;
    // the sinks, each nullable, at least one given:
    float* dist;                // [nq][m]: the reference distance of a present slot, +inf otherwise
    uint64_t* keys;             // [nq][m]: dist_key(d, row) of the present slots, in any order, in
    uint32_t* kcnt;             //   the first kcnt[q] slots (zero before the launch; with keys)
    uint32_t* found;            // [nq], nullable: += the present slots (zero before the launch)
    uint32_t q0;                // (set by the launcher: the first query of a launch)
};
// Grid (ceil(m / 256), queries) x 256 threads, a wave per 64 consecutive slots, lane = slot: every
// slot of dist is written, keys past kcnt[q] are untouched.
hipError_t launch_score_ids(const ScoreArgs& a, hipStream_t s);
// One workgroup per query: the kcnt[q] <= m <= kScoreMaxIds keys sorted ascending (distance, then
// row), a key equal to its predecessor dropped, the first k as (offset + row, distance) in out_idx /
// out_dist [nq][k] with (~0, +inf) behind them; out_count[q] = min(k, distinct keys).  1 <= k <= m.
hipError_t launch_score_finish(const uint64_t* keys, const uint32_t* kcnt, uint32_t m, uint32_t nq, uint32_t k,
                               uint64_t offset, uint64_t* out_idx, float* out_dist, uint32_t* out_count,
                               hipStream_t s);

// ---- masked range search (bsr_local_range_search_masked) ------------------------
// The routing behind launch_range_tau: a query with to_list[q] != 0 (device, [nq]) is answered by
// the list scan by design -- tau[q] = +inf, and q appended to scan_list (status[kStFail] and
// status[kStFail2] counting it) unless launch_range_tau listed it already or its radius is < 0 or
// NaN.  Afterwards every query is on scan_list at most once.  One workgroup.
hipError_t launch_range_route(const uint32_t* to_list, const float* radius, uint32_t nq, float* tau,
                              uint32_t* scan_list, uint32_t* status, hipStream_t s);
// The range over row lists: launch_scan_list_groups' gather with launch_range_scan's epilogue.
// Group y (blockIdx.y) walks the grp[y].n_list ids at list + grp[y].off (local row ids, each < n;
// the list holds allowed live rows only -- no mask and no tombstone is read) for the qf queries
// qids[y * qf ..] (qf one of 1, 2, 4, 8; the first grp[y].nq count, the rest are padding ids of the
// same mask): every listed row with d <= radius[id] claims a slot of keys[id] by an atomic add on
// rcnt[id] and stores its key when the slot is below cap; the count stays exact beyond that.  rcnt
// of every scanned query is zero before its first launch; a list split over several launches
// accumulates.  grid: scan_grid_for(the launch's longest list).
struct RangeListArgs {
    const float* rows;          // f32 [n_pad][ld]
    uint32_t ld, dim;
    const float* na;            // row magnitudes (read, never recomputed)
    const float* qf32;          // queries [qpad][ld]
    const float* nb;            // query magnitudes
    const float* radius;        // [nq]
    const uint32_t* list;       // the launch's row lists
    const ScanGroupDesc* grp;   // [groups]
    uint32_t groups, qf;
    const int32_t* qids;        // [groups][qf]
    uint64_t* keys;             // [nq][cap]
    uint32_t* rcnt;             // [nq]
    uint32_t cap;
};
hipError_t launch_range_scan_list_groups(const RangeListArgs& a, uint32_t grid, hipStream_t s);
// A segment of a mask's row list (a list split over chunks): the ids of rank first .. first + n_list
// - 1 among the allowed live rows of mask `mask`, ascending, at list + off.  blk: the block prefixes
// of launch_mask_groups_count.
struct MaskSegDesc { uint64_t off; uint32_t mask, first, n_list, pad_; };
hipError_t launch_mask_groups_scatter_seg(const uint64_t* allow, uint64_t words, uint64_t n, const uint64_t* dead,
                                          const uint32_t* blk, const MaskSegDesc* d, uint32_t n_segs, uint32_t* list,
                                          hipStream_t s);

// ---- MMR selection (bsr_local_top_k_mmr; k_exact.hip) ---------------------------
// One workgroup per query picks k of its candidates greedily.  The candidates are the first
// m = min(cand_cnt[q], fetch_k) slots of row q of cand_idx / cand_dist [nq][fetch_k] (global ids and
// query distances dq, as a search leaves them; the kernel takes the slots as they stand -- position
// = slot -- and an id outside [offset, offset + n) is no candidate).  D(i, j) is the reference's
// distance of the stored rows of positions i and j with the stored magnitudes na.  The first pick is
// the lowest candidate position; every later one the unpicked position with the largest
// (mu * mind_i) - (lambda * dq_i), mu = 1.0f - lambda, mind_i = the smallest D(i, p) over the
// picks p so far (fminf, from +inf), every operation a rounded f32 one; ties go to the lower
// position.  Row q of out_idx / out_dist / out_rank (nullable) [nq][k] holds the picks in selection
// order -- global id, dq, position -- then (~0, +inf, ~0u); out_count[q] = the number of picks,
// min(k, candidates).  fetch_k <= kMmrMaxFetch, 1 <= k <= fetch_k, lambda in [0, 1].
constexpr uint32_t kMmrMaxFetch = 256;
struct MmrArgs {
    const float* rows;          // f32 [n_pad][ld]
    uint32_t ld, dim;
    uint64_t n, offset;         // rows of the shard; the global id of row 0
    const float* na;            // row magnitudes (read, never recomputed)
    const uint64_t* cand_idx;   // [nq][fetch_k]
    const float* cand_dist;     // [nq][fetch_k]
    const uint32_t* cand_cnt;   // [nq]
    uint32_t nq, fetch_k, k;
    float lambda;
    uint64_t* out_idx;          // [nq][k]
    float* out_dist;            // [nq][k]
    uint32_t* out_rank;         // [nq][k], nullable
    uint32_t* out_count;        // [nq]
};
hipError_t launch_mmr_select(const MmrArgs& a, hipStream_t s);

// ---- collapsed search (bsr_local_top_k_collapsed; k_exact.hip) ------------------
// The group check: *flag |= 1 when an entry of row_group[0 .. n) is >= n_groups (zero before the
// launch; 4 n bytes read, no pass over the rows).
hipError_t launch_group_check(const uint32_t* row_group, uint64_t n, uint32_t n_groups, uint32_t* flag,
                              hipStream_t s);
// The walk: one wave per query over its candidate list -- the first m = min(cand_cnt[q], fetch_k)
// slots of row q of cand_idx / cand_dist [nq][fetch_k], in (distance asc, id asc) order as a search
// leaves them; an id outside [offset, offset + n) is no candidate and nothing is read through it.
// The first occurrence of every group, in list order, and the first k of those: row q of out_idx /
// out_dist / out_group (nullable) [nq][k] holds (global id, distance, group), then (~0, +inf, ~0u);
// out_count[q] = their number.  A query that found fewer than k groups in a full list (cand_cnt[q]
// >= fetch_k) is appended to fail[] (any order), *fail_cnt (zero before the launch) counts them.
// 1 <= k <= fetch_k <= kCollapseMaxFetch.
constexpr uint32_t kCollapseMaxFetch = 256;
struct CollapseWalkArgs {
    const uint64_t* cand_idx;   // [nq][fetch_k]
    const float* cand_dist;     // [nq][fetch_k]
    const uint32_t* cand_cnt;   // [nq]
    uint32_t nq, fetch_k, k;
    uint64_t n, offset;         // rows of the shard; the global id of row 0
    const uint32_t* row_group;  // [n], every entry < n_groups (launch_group_check)
    uint64_t* out_idx;          // [nq][k]
    float* out_dist;            // [nq][k]
    uint32_t* out_group;        // [nq][k], nullable
    uint32_t* out_count;        // [nq]
    uint32_t* fail;             // [nq]
    uint32_t* fail_cnt;         // one word
};
hipError_t launch_collapse_walk(const CollapseWalkArgs& a, hipStream_t s);
// The group scan, the same tile loop: every valid row that is live (dead, nullable) and
// allowed lowers best[j][row_group[row]] to dist_key(d, row) by an atomic min, j the query's slot
// in the launch (best: u64 [template width][n_groups], all-ones before the launch).  The allow bit
// of slot j's query id: word row / 64 of mask query_mask[id] (mask 0 without a query_mask) of allow
// [n_masks][allow_words]; allow == nullptr allows every row.  qids: as RangeArgs has them.
struct CollapseScanArgs {
    const float* rows;          // f32 [n_pad][ld]
    uint32_t ld, dim;
    uint64_t n;
    const float* na;            // row magnitudes
    const float* qf32;          // queries [qpad][ld]
    const float* nb;            // query magnitudes
    const uint64_t* dead;       // the bitset of deleted rows (nullable)
    const uint32_t* row_group;  // [n]
    uint32_t n_groups;
    const uint64_t* allow;      // [n_masks][allow_words] (nullable)
    uint64_t allow_words;
    const uint32_t* query_mask; // [nq] (nullable: mask 0)
    const int32_t* qids;
    uint32_t nqf;
    uint64_t* best;             // [1, 2, 4 or 8][n_groups]
};
hipError_t launch_collapse_scan(const CollapseScanArgs& a, uint32_t grid, hipStream_t s);
// The selection over the tables of a launch's nqf queries: workgroup (g, j) keeps the k smallest keys
// of its slice of best[j][0 .. n_groups) and writes them as partial list g of query slot j in
// launch_merge_parts' layout (part: grid * width * k keys, width = nqf rounded up to 1, 2, 4, 8).
// grid: collapse_select_grid(n_groups).  k <= 256.
uint32_t collapse_select_grid(uint32_t n_groups);
hipError_t launch_collapse_select(const uint64_t* best, uint32_t n_groups, uint32_t nqf, uint32_t k, uint32_t grid,
                                  uint64_t* part, hipStream_t s);
// The finish: the merged keys [.][k] of the queries qids[0 .. nqf) (ascending, kKeyNone behind them)
// into row qids[j] of the outputs as (offset + row, distance, row_group[row]), then (~0, +inf, ~0u);
// out_count = the number of keys.  k <= 256.
hipError_t launch_collapse_finish(const uint64_t* keys, const int32_t* qids, uint32_t nqf, uint32_t k, uint64_t offset,
                                  const uint32_t* row_group, uint64_t* out_idx, float* out_dist, uint32_t* out_group,
                                  uint32_t* out_count, hipStream_t s);

// ---- capped search (bsr_local_top_k_capped; k_exact.hip) ------------------------
// The walk, launch_collapse_walk's arguments and contract with "first occurrence of its group"
// replaced by "fewer than per_group earlier list positions hold its group": the kept rows in list
// order, the first k of them, the same tail and count.  A query that kept fewer than k rows in a
// full list is appended to fail[].  per_group = 1 writes what launch_collapse_walk writes.
constexpr uint32_t kCapMaxPerGroup = 16;  // BSR_CAP_MAX_PER_GROUP
struct CapWalkArgs {
    CollapseWalkArgs w;
    uint32_t per_group;  // >= 1 (a value >= k caps nothing)
};
hipError_t launch_cap_walk(const CapWalkArgs& a, hipStream_t s);
// The capped group scan, launch_collapse_scan's arguments and loop with m entries per (query
// slot, group): s.best is u64 [template width][n_groups][m], all-ones before the launch, and ends
// holding, for every (slot, group), the m smallest keys dist_key(d, row) of the group's live allowed
// rows in no particular order (kKeyNone where the group has fewer).  1 <= m <= kCapMaxPerGroup.
// Read as m * n_groups entries per slot the tables are launch_collapse_select's input.
struct CapScanArgs {
    CollapseScanArgs s;
    uint32_t m;
};
hipError_t launch_cap_scan(const CapScanArgs& a, uint32_t grid, hipStream_t s);

uint32_t scan_grid_for(uint64_t n);

}  // namespace bsr
