/*
 * bsr.h -- C ABI of the MI355X-native search engine for the better-search-rag-rust hot path:
 * block-distributed exact cosine-distance scan + global top-k reduction.
 *
 * One process per GPU (the reference's one process per MPI rank).  Every entry point
 * returns 0 (BSR_OK) or a negative bsr_status (BSR_PARTIAL, positive, only from the
 * parallel search's root: see there); bsr_last_error() gives a thread-local message.  No
 * C++ exception or panic crosses this boundary.  Plain pointers only: query, row and
 * output pointers may be host or device (hipMalloc) memory, detected per call.
 * Device inputs: bsr_index_load / bsr_index_append synchronize the device before reading
 * device rows (one-time calls).  The search entry points do not: the library's streams are
 * blocking streams, so their work waits for work issued before the call on the legacy
 * default (NULL) stream (e.g. PyTorch's default stream); queries produced on any other
 * stream must be complete (synchronized) first.
 *
 * Each entry point names the reference item it replaces (paths relative to the reference
 * repository nichmorgan/better-search-rag-rust):
 *   bsr_cosine_distance               src/metrics.rs:143-165 (cosine_distance)
 *   bsr_interval_by_rank              src/mpi_helpers/load_balance.rs:24-42 (interval_by_rank)
 *   bsr_index_*                       src/vectorstore/polars.rs:79-91,121-169,243-246
 *                                     (PolarsVectorstore::new/get_many/get/get_count: the
 *                                     rank's corpus slab, resident in HBM)
 *   bsr_local_top_k                   src/mpi_helpers/metrics.rs:16-53 (compute_local_top_k)
 *   bsr_gather_top_k                  src/mpi_helpers/metrics.rs:56-138 (gather_top_k_results)
 *   bsr_global_top_k                  src/mpi_helpers/metrics.rs:141-171 (compute_global_top_k)
 *   bsr_gather_global_top_k           src/mpi_helpers/metrics.rs:56-171 (a-4 + a-5: the
 *                                     exchange and root merge of a-6, :194-202)
 *   bsr_parallel_top_k_similarity_search
 *                                     src/mpi_helpers/metrics.rs:174-206
 *                                     (parallel_top_k_similarity_search)
 *   bsr_broadcast                     src/main.rs:123-125 (broadcast_into of the query)
 *   bsr_allgather_bytes               src/mpi_helpers/benchmark.rs:131-293 (timing gather)
 *
 * Results are bit-identical to the reference's: indices in (distance asc, index asc)
 * order, each distance the exact f32 the reference computes (sequential f32 sums, no FMA,
 * correctly rounded sqrt/div, identical-vector shortcut).  Deviations (documented in
 * DESIGN.md): non-finite inputs return BSR_E_NONFINITE where the reference panics; a query
 * whose length differs from the index dimension returns BSR_E_DIM where the reference
 * scores every row 1.0.
 */
#ifndef BSR_H
#define BSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    BSR_PARTIAL = 1,      /* parallel search root: result valid but its own block is missing */
    BSR_OK = 0,
    BSR_E_INVALID = -1,   /* bad argument / null pointer / k out of range */
    BSR_E_NONFINITE = -2, /* NaN or Inf in a query or row (the reference panics) */
    BSR_E_HIP = -3,       /* HIP runtime error (message in bsr_last_error) */
    BSR_E_NOMEM = -4,     /* device allocation failed */
    BSR_E_RCCL = -5,      /* RCCL error */
    BSR_E_DIM = -6,       /* query length != index dimension */
    BSR_E_STATE = -7,     /* call out of order (e.g. search before load) */
    BSR_E_NODEVICE = -8   /* no HIP device visible: the engine has no CPU fallback */
} bsr_status;

typedef enum { BSR_F32 = 0, BSR_BF16 = 1 } bsr_dtype;

typedef struct {
    uint32_t dim;    /* embedding length (768 in the reference, src/main.rs:117) */
    uint32_t dtype;  /* bsr_dtype of the stored rows */
    uint32_t max_k;  /* largest top_k a search may ask for (<= BSR_MAX_K) */
    uint32_t flags;  /* BSR_FLAG_* */
    int32_t device;  /* HIP device ordinal; -1 = current device */
} bsr_config;

#define BSR_MAX_K 256u
#define BSR_FLAG_EXACT_ONLY 1u /* never use the MFMA candidate stage (always full exact scan) */
#define BSR_FLAG_PROFILE 2u    /* record per-kernel HIP events (bsr_index_profile) */
/* The MFMA candidate filter's operand is int8 (v_mfma_i32_16x16x64_i8 for rows of up to 768
 * bytes, v_mfma_i32_32x32x32_i8 otherwise; per-32-row-block and per-query scales, certified
 * with a measured Cauchy-Schwarz bound).  Every returned list is exact; the filter only
 * decides how much exact work a query needs.  The bf16 filter operand of earlier rounds is
 * retired: bsr_index_create with this flag returns BSR_E_INVALID (a bf16 CORPUS, cfg.dtype =
 * BSR_BF16, is served on the int8 filter). */
#define BSR_FLAG_FILTER_BF16 4u

/* Mirrors RankInterval {start_index, end_index} (load_balance.rs:8-17). end < start means
 * an empty block, as in the reference's release build. */
typedef struct {
    uint64_t start_index;
    uint64_t end_index;
} bsr_rank_interval;

typedef struct bsr_index bsr_index; /* one rank's corpus shard, resident in HBM */
typedef struct bsr_comm bsr_comm;   /* the rank group: RCCL (one GPU each), a host transport or a loopback */

/* Per-search statistics of the last bsr_local_top_k on an index. */
typedef struct {
    uint32_t n_queries;
    uint32_t n_exact_direct;   /* queries answered by the full exact scan by design */
    uint32_t n_fallback;       /* queries whose MFMA candidate set failed certification */
    uint32_t n_candidates;     /* k' candidates rescored per query */
    uint64_t n_emitted;        /* candidates emitted by the MFMA filter (all queries) */
    uint32_t filter_op;        /* 0 = int8 filter (the only operand since round 4) */
    float row_ebound;          /* max over rows of ||a/|a| - s q||_2 (int8 quantisation) */
    uint32_t n_rescued;        /* queries certified by the second chance (all emitted rows) */
    uint32_t graph_replay;     /* 1: the search replayed a captured hipGraph (every filtered batch
                                  from the second search of its shape on, at profile level 0) */
    uint32_t search_path;      /* BSR_PATH_* bits: which branches the last search took */
} bsr_search_stats;

/* bsr_search_stats.search_path: which branches the last search took (bits 1-16: the parallel
 * search; 32, 64: a batch of <= 16 queries on the self-thresholded path; 128,
 * 256: bsr_local_top_k_masked -- both when the filter path sent some queries to the list scan) */
#define BSR_PATH_COLLECTIVE 1u   /* the collectives ran (size > 1, or BSR_FORCE_COLLECTIVES=1) */
#define BSR_PATH_GLOBAL_TAU 2u   /* the global-threshold search */
#define BSR_PATH_DIRECT_OUT 4u   /* root: merged rows written straight into coherent pinned outputs */
#define BSR_PATH_DEVICE_MERGE 8u /* root of the standard path: the device merge (k_merge_lists) */
#define BSR_PATH_FALLBACK 16u    /* global threshold: uncertified queries took the collective fallback */
#define BSR_PATH_SKINNY_TOP 32u  /* no sample pass: every filter wave's 4 best keys per query */
#define BSR_PATH_TOP_RERUN 64u   /* ... left a query uncertified: the batch ran again, thresholded */
#define BSR_PATH_MASK_LIST   128u /* masked search: exact top-k over the allowed-row list */
#define BSR_PATH_MASK_FILTER 256u /* masked search: int8 filter, emitted lists cut by the mask */
#define BSR_PATH_MASK_GROUPS 512u /* bsr_local_top_k_masked_groups ran (with MASK_LIST / MASK_FILTER bits) */
#define BSR_PATH_RANGE      1024u /* bsr_local_range_search ran */
#define BSR_PATH_RANGE_SCAN 2048u /* ... and a query of the batch was answered by the exact range scan */
#define BSR_PATH_MMR        4096u /* bsr_local_top_k_mmr ran (with the bits of the candidate search) */
#define BSR_PATH_COLLAPSE       8192u  /* bsr_local_top_k_collapsed ran (with the candidate search's bits) */
#define BSR_PATH_COLLAPSE_SCAN 16384u  /* ... and a query of the batch was answered by the group scan */
#define BSR_PATH_CAP       32768u  /* bsr_local_top_k_capped ran (with the candidate search's bits) */
#define BSR_PATH_CAP_SCAN  65536u  /* ... and a query of the batch was answered by the capped group scan */
#define BSR_PATH_SCORE   131072u   /* bsr_local_score_ids / bsr_local_rerank_ids ran */

/* Per-kernel timing (BSR_FLAG_PROFILE): cumulative device milliseconds and launch counts
 * since the last reset, measured with hipEvents on the index's stream. */
typedef struct {
    double gemm_emit_ms;  uint64_t gemm_emit_launches;  /* dominant kernel */
    double gemm_sample_ms; uint64_t gemm_sample_launches;
    double select_ms;     uint64_t select_launches;
    double rescore_ms;    uint64_t rescore_launches;
    double scan_ms;       uint64_t scan_launches;
    double search_ms;     uint64_t searches;             /* whole bsr_local_top_k */
} bsr_profile;

/* ---- errors / device -------------------------------------------------------------- */
const char* bsr_last_error(void);
const char* bsr_status_string(int status);
int bsr_device_count(int* out_count);
const char* bsr_version(void);

/* ---- a-1: src/metrics.rs:143-165, one pair, computed on the GPU ------------------ */
int bsr_cosine_distance(const float* a, uint32_t len_a, const float* b, uint32_t len_b,
                        float* out);

/* ---- a-3: src/mpi_helpers/load_balance.rs:24-42 ---------------------------------- */
int bsr_interval_by_rank(int32_t rank, int32_t size, uint64_t count, bsr_rank_interval* out);

/* ---- the rank's shard (read side of src/vectorstore/polars.rs) ------------------- */
int bsr_index_create(const bsr_config* cfg, bsr_index** out);
void bsr_index_destroy(bsr_index* ix);
/* Copy n_rows row-major rows (f32, or bf16 bits when cfg.dtype == BSR_BF16) into HBM and
 * precompute per-row state.  global_offset is the global index of local row 0
 * (interval_by_rank(rank,size,N).start_index).  Replaces any previous contents.  Device rows
 * may come from any stream: load and append synchronize the device before reading them. */
int bsr_index_load(bsr_index* ix, const void* rows, uint64_t n_rows, uint64_t global_offset);
/* Append rows after the current ones (PolarsVectorstore::append_many, polars.rs:101-119). */
int bsr_index_append(bsr_index* ix, const void* rows, uint64_t n_rows);
int bsr_index_count(const bsr_index* ix, uint64_t* out);                /* get_count */
int bsr_index_dim(const bsr_index* ix, uint32_t* out);                  /* row length */
int bsr_index_global_offset(const bsr_index* ix, uint64_t* out);
/* Copy `count` rows starting at local row `offset` into out (f32, host or device):
 * PolarsVectorstore::get_many(SliceArgs{offset,length}) / get (polars.rs:121-169). */
int bsr_index_get_many(const bsr_index* ix, uint64_t offset, uint64_t count, float* out);

/* ---- tombstones: deleted rows of a loaded shard, honoured by every search.
 * Row positions never move: bsr_index_count, bsr_index_get_many (a deleted row's stored values
 * included) and the global indices of live rows are unchanged.  Every search -- bsr_local_top_k,
 * bsr_local_top_k_masked (over allow & ~deleted), the parallel search -- returns the reference's
 * result over a store that holds only the live rows, each keeping its global index:
 * out_count[q] = min(k, live), entries past the count (~0, +inf); zero live rows is not an error.
 * bsr_index_load clears the tombstones; bsr_index_append keeps them, and the appended rows are
 * live.  There is no undelete; bsr_index_compact drops the deleted rows.  The plain search keeps its fast path (graph
 * replay from the second search of a shape after a delete); a parallel search takes the standard
 * path (BSR_PATH_GLOBAL_TAU clear) while any row of this rank's shard is deleted.
 *
 * Mark rows as deleted.  ids are GLOBAL indices as the searches return them (global_offset + local
 * row), host or device memory (device ids complete before the call, as queries), any order,
 * duplicates allowed, n_ids < 2^32.  All or nothing: an id outside [global_offset, global_offset
 * + n) -> BSR_E_INVALID and no row changes.  *out_deleted (optional) = rows that went live ->
 * deleted in this call.  Not loaded: BSR_E_STATE.  n_ids = 0: BSR_OK.  A one-time mutation like
 * load and append: it synchronizes with the index's stream. */
int bsr_index_delete(bsr_index* ix, const uint64_t* ids, uint64_t n_ids, uint64_t* out_deleted);
int bsr_index_live_count(const bsr_index* ix, uint64_t* out);          /* n - deleted rows */
/* bit (i & 63) of word (i >> 6) set = local row i is deleted; words must equal ceil(n / 64)
 * (BSR_E_INVALID otherwise); host or device out.  (~ of it is a valid allow mask.)  Not loaded:
 * BSR_E_STATE. */
int bsr_index_deleted_mask(const bsr_index* ix, uint64_t* out_words, uint64_t words);

/* ---- in-place update: rows of a loaded shard replaced, their ids kept.
 * Row j of rows ([n_ids][dim] row-major: f32, or bf16 bits when cfg.dtype == BSR_BF16) replaces the
 * stored row ids[j]; ids are GLOBAL indices as bsr_index_delete takes them.  ids and rows are,
 * independently, host or device memory; with a device input the call synchronizes the device
 * before reading (the load / append rule), and it synchronizes with the index's stream before
 * returning: a one-time mutation.
 * All or nothing, checked on the device before any stored byte changes: an id outside
 * [global_offset, global_offset + n), or the same id twice in one call (no "last wins") ->
 * BSR_E_INVALID; a NaN or Inf in any incoming value (a bf16 row: after widening) ->
 * BSR_E_NONFINITE; the index then answers every search exactly as before the call.  Not loaded:
 * BSR_E_STATE.  n_ids = 0: BSR_OK.  Null ids or rows with n_ids > 0, or n_ids >= 2^32:
 * BSR_E_INVALID.
 * After BSR_OK bsr_index_get_many returns the new values, bsr_index_count and the global offset
 * are unchanged, and every search -- plain, masked, grouped, parallel -- returns the reference's
 * result over the modified store: the magnitudes, the filter operand, its scales and the
 * certification bound of the touched 32-row blocks are rebuilt by the load's own kernels' code.
 * Zero rows are legal (distance 1.0).  Tombstones are untouched: an updated row that is deleted
 * stays deleted (its new values are stored and bsr_index_get_many shows them).
 * The norm flags are sticky: an updated row whose magnitude overflows or leaves [1e-18, 1e18]
 * sends every later search to the exact scan, as a load of that row would, and replacing that row
 * again does not bring the filter back (a load does).  bsr_search_stats.row_ebound only grows.
 * Cost: O(n_ids ld + touched 32-row blocks x 32 ld + n / 64), no pass over the shard's rows; while
 * the shard has tombstones, O(n / 64 + n_dead ld) more, as bsr_index_delete (the operand of every
 * deleted row is zeroed again).  A captured search graph bakes in nothing an update changes and
 * replays on; only an update that had to grow its own scratch buffers (the first of its size)
 * makes the searches re-capture, as any allocation does. */
int bsr_index_update(bsr_index* ix, const uint64_t* ids, const void* rows, uint64_t n_ids);

/* ---- compaction: the deleted rows of a loaded shard dropped, on the device.
 * After BSR_OK the index is what a fresh index of the same config is after bsr_index_load of the
 * live rows at new_global_offset: the live rows packed in ascending order of their old position,
 * their values what bsr_index_get_many returned before the call; bsr_index_count =
 * bsr_index_live_count = the old live count; bsr_index_deleted_mask all zero; every search -- plain,
 * masked, grouped, parallel (BSR_PATH_GLOBAL_TAU eligible again) -- and bsr_search_stats.row_ebound
 * bit-identical to that fresh index; the sticky norm flags and the growing row_ebound of
 * bsr_index_update reset, as a load resets them (the derived state is rebuilt by the load's kernels).
 * out_old_ids (optional; host or device memory, out_capacity entries): out_old_ids[j] = the global
 * index, before the call, of the row whose global index is now new_global_offset + j.  NULL:
 * out_capacity is ignored.  *out_count (optional) = the new row count.
 * All or nothing, checked before any stored byte changes: null index, unknown flag bits, a non-null
 * out_old_ids with out_capacity below the live count, new_global_offset + live overflowing 64
 * bits -> BSR_E_INVALID; not loaded -> BSR_E_STATE.  A HIP failure after the move has begun leaves
 * the index unloaded (as a failed bsr_index_append does): load it again.
 * new_global_offset is always applied -- a rank without tombstones whose lower neighbours shrank
 * still rebases (ranks compact with the exclusive prefix sum of all ranks' live counts as their
 * offsets).  No tombstones and the same offset: a no-op that writes the identity map, allocates
 * nothing and keeps the captured search graphs; any other compaction makes them stale (the next
 * search launches directly, the one after captures).  Zero live rows is legal: the index stays
 * loaded with 0 rows.  The move is in place, through a staging buffer of BSR_COMPACT_STAGE_BYTES
 * (environment, read per call; default 256 MB, at least 256 rows) that the index keeps.
 * Without BSR_COMPACT_SHRINK every allocation keeps its size and later appends reuse it; with it
 * the slab and the derived buffers are reallocated at the new size where that saves bytes (the old
 * and the new slab exist together during the call) and the staging buffer is released.
 * A one-time mutation like load, append, delete and update: it synchronizes with the index's
 * stream.  Cost: one pass over the rows from the first deleted row on, plus the load's rebuild. */
#define BSR_COMPACT_SHRINK 1u /* also give back the HBM the dropped rows held */
int bsr_index_compact(bsr_index* ix, uint64_t new_global_offset, uint32_t flags, uint64_t* out_old_ids,
                      uint64_t out_capacity, uint64_t* out_count);

/* ---- a-2: compute_local_top_k for n_queries queries (row-major [n_queries][dim] f32).
 * out_idx/out_dist are [n_queries][k]; row q holds out_count[q] = min(k, n_rows) entries
 * in (distance asc, global index asc) order.  Indices are global (offset added). ------ */
int bsr_local_top_k(bsr_index* ix, const float* queries, uint32_t n_queries, uint32_t k,
                    uint64_t* out_idx, float* out_dist, uint32_t* out_count);

/* ---- a-2 over an allow-list of rows: compute_local_top_k as if the store held only the allowed
 * rows, each keeping its global index.  allow is ONE bitset for the whole batch: bit (i & 63) of
 * word (i >> 6) is set when local row i may be returned; host or device memory, detected per
 * call (a device mask produced on a non-default stream must be complete before the call, as
 * queries).  allow_words must equal ceil(n / 64) for the index's current row count n
 * (BSR_E_INVALID otherwise); bits at positions >= n are ignored.  allow == NULL or an unknown
 * mode: BSR_E_INVALID (a search without a mask is bsr_local_top_k).  With A allowed rows,
 * out_count[q] = min(k, A) entries in (distance asc, global index asc) order with the
 * reference's exact f32 distances; entries past the count are (~0, +inf).  A = 0 is not an
 * error: every count is 0.  Every other status as bsr_local_top_k.
 * mode picks the path (bsr_search_stats.search_path reports it; results are identical):
 *   BSR_MASK_LIST    an exact top-k over the list of allowed rows: cost scales with A;
 *   BSR_MASK_FILTER  the int8 filter over the whole shard with its threshold lowered by n / A,
 *                    the emitted lists cut by the mask, every remaining row rescored exactly and
 *                    certified; uncertified queries take the list scan.  Possible when the
 *                    unmasked search would filter (k <= 200, a shard of more rows than one
 *                    query's candidate list) and A / n >= ks(k) / 128 (1/16 for k <= 10, 0.19
 *                    for k = 50, 0.375 for k = 100); the list scan otherwise;
 *   BSR_MASK_AUTO    the library's choice.
 * Never graph-replayed (graph_replay = 0); it leaves the unmasked search's graphs as they are. */
#define BSR_MASK_AUTO   0u
#define BSR_MASK_LIST   1u
#define BSR_MASK_FILTER 2u
int bsr_local_top_k_masked(bsr_index* ix, const float* queries, uint32_t n_queries, uint32_t k,
                           const uint64_t* allow, uint64_t allow_words, uint32_t mode,
                           uint64_t* out_idx, float* out_dist, uint32_t* out_count);

/* ---- a-2, one allow mask per group of queries: a batch that mixes tenants or
 * metadata filters in ONE call -- one filter pass over the shard and one batched list scan
 * instead of a bsr_local_top_k_masked call per distinct mask.
 * allow is [n_masks][allow_words] bitsets, each laid out as bsr_local_top_k_masked's
 * (allow_words must equal ceil(n / 64), bits at positions >= n are ignored); query_mask[q] <
 * n_masks names query q's mask.  allow and query_mask are, independently, host or device memory,
 * detected per call (device memory produced on a non-default stream must be complete before the
 * call, as queries).  A mask that no query names is legal.  Query q gets the reference's result
 * over a store that holds only the rows of its mask that are not deleted, each keeping its global
 * index: out_count[q] = min(k, A_g) entries in (distance asc, global index asc) order with the
 * exact f32 distances, (~0, +inf) past the count; A_g = 0 is not an error.  The result is
 * bit-identical to bsr_local_top_k_masked called once per mask with that mask's queries.
 * BSR_E_INVALID: n_masks == 0, a null allow or query_mask (with n_queries > 0), a wrong
 * allow_words, an unknown mode, a query_mask entry >= n_masks (checked on the device before any
 * mask is indexed with it).  Every other status as bsr_local_top_k_masked.
 * mode applies per mask group, with A_g and the number of queries that name the mask:
 *   BSR_MASK_LIST    every group takes the list scan;
 *   BSR_MASK_FILTER  a group takes the filter where bsr_local_top_k_masked could (above), the list
 *                    scan otherwise;
 *   BSR_MASK_AUTO    bsr_local_top_k_masked's rule per group.
 * search_path carries BSR_PATH_MASK_GROUPS with BSR_PATH_MASK_FILTER and / or BSR_PATH_MASK_LIST;
 * n_exact_direct counts the queries sent to the list scan by design, n_fallback the uncertified
 * ones.  The row lists of a batch are built in chunks of at most BSR_MASK_LIST_BUDGET bytes of
 * ids (environment, read per search; default 256 MB).  Never graph-replayed. */
int bsr_local_top_k_masked_groups(bsr_index* ix, const float* queries, uint32_t n_queries, uint32_t k,
                                  const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                  const uint32_t* query_mask, uint32_t mode,
                                  uint64_t* out_idx, float* out_dist, uint32_t* out_count);

/* ---- range search: every live row of the shard within a distance of each query, exact.
 * out_count[q] = the number of live rows whose reference distance to query q is <= radius[q]:
 * the exact f32 of src/metrics.rs:143-165 (identical-vector shortcut and zero-magnitude rule
 * included), compared as plain f32.  The count is always exact, even above `capacity`.
 *   out_count[q] <= capacity: row q of out_idx / out_dist ([n_queries][capacity]) holds exactly
 *     those rows as (global index, distance) in (distance asc, global index asc) order, and
 *     (~0, +inf) after them;
 *   out_count[q] >  capacity: every slot of row q is (~0, +inf) -- call again with more capacity
 *     or a smaller radius, as with snprintf.  Never a partial or unordered subset.
 * radius[q] < 0: count 0.  radius[q] >= 2 or +inf: every live row is in range.  A NaN radius:
 * BSR_E_INVALID for the call, the outputs untouched (device radii are checked on the device,
 * before any result is written).
 * BSR_E_INVALID before any device is touched: a null index; with n_queries > 0 a null radius,
 * queries or output; capacity 0 or above BSR_RANGE_MAX_RESULTS.  Not loaded: BSR_E_STATE.  A
 * non-finite query: BSR_E_NONFINITE, as bsr_local_top_k.  n_queries = 0: BSR_OK.  An empty shard:
 * every count 0.  Every other status as bsr_local_top_k.
 * queries, radius and the outputs are, independently, host or device pointers, detected per call.
 * Deleted rows (bsr_index_delete) are never counted or returned.
 * How: the int8 filter's certified bound gives the emission threshold from the
 * radius, so the emitted rows are a superset of the answer and are rescored exactly; a query
 * whose emitted list overflows, or that the filter cannot serve, takes an exact scan of the shard.
 * An index that cannot filter (BSR_FLAG_EXACT_ONLY, out-of-range row norms, or no more rows than
 * an emitted list holds) scans every query.  Never graph-replayed; the plain search's graphs are
 * left alone.  bsr_search_stats: search_path carries BSR_PATH_RANGE, and BSR_PATH_RANGE_SCAN
 * when any query was answered by the scan; n_emitted = the emitted keys of the batch;
 * n_exact_direct = the queries sent to the scan by design; n_fallback = the queries whose emitted
 * list overflowed.
 * Out of scope: a multi-rank range search (every rank calls this on its shard and the caller
 * concatenates: ranges need no merge); a CSR (compressed sparse row) output.  An allow mask
 * combined with a radius: bsr_local_range_search_masked, below. */
#define BSR_RANGE_MAX_RESULTS 4096u
int bsr_local_range_search(bsr_index* ix, const float* queries, uint32_t n_queries,
                           const float* radius,            /* [n_queries], host or device */
                           uint32_t capacity,              /* result slots per query, 1..BSR_RANGE_MAX_RESULTS */
                           uint64_t* out_idx, float* out_dist,   /* [n_queries][capacity] */
                           uint32_t* out_count);                 /* [n_queries] */

/* ---- masked range search: a radius and an allow mask in one call ("every chunk of tenant T
 * within distance r").  bsr_local_range_search's contract over bsr_local_top_k_masked_groups'
 * masks, word for word where they overlap:
 * allow is [n_masks][allow_words] bitsets (allow_words must equal ceil(n / 64), bits at positions
 * >= n are ignored); query_mask[q] < n_masks names query q's mask; query_mask == NULL is legal only
 * when n_masks == 1, and every query then uses mask 0.  A mask that no query names is legal.
 * out_count[q] = the number of rows that are in q's mask, not deleted, and whose reference
 * distance is <= radius[q] -- always exact, also above `capacity`.
 *   out_count[q] <= capacity: exactly those rows, (distance asc, global index asc), the
 *     reference's f32 bits, then (~0, +inf);
 *   out_count[q] >  capacity: every slot of row q is (~0, +inf).
 * radius[q] < 0: count 0.  radius[q] >= 2 or +inf: count = A_g, the live rows mask g allows.
 * A_g = 0 is not an error.
 * queries, radius, allow, query_mask and the three outputs are, independently, host or device
 * pointers, detected per call.  Never graph-replayed; the plain search's graphs are left alone.
 * The checks, in this order; the caller's arrays are untouched on every error:
 *   1. BSR_E_INVALID before any device is touched: a null index; capacity 0 or above
 *      BSR_RANGE_MAX_RESULTS; n_masks == 0; an unknown mode; with n_queries > 0 a null radius,
 *      queries, output or allow; a null query_mask with n_masks > 1;
 *   2. BSR_E_STATE: the index is not loaded;
 *   3. BSR_E_INVALID: allow_words != ceil(n / 64); a NaN in a host radius array;
 *   4. n_queries = 0: BSR_OK;
 *   5. BSR_E_INVALID, checked on the device: a query_mask entry >= n_masks (found before any mask
 *      is indexed with it);
 *   6. BSR_E_NONFINITE: a non-finite query; BSR_E_INVALID: a NaN in a device radius array -- both
 *      read from the batch's status words, before any result is written.
 * An empty shard: every count 0.
 * mode applies per mask group, with A_g and the number of queries that name the mask:
 *   BSR_MASK_FILTER  the group's queries go through the int8 filter with the threshold
 *                    bsr_local_range_search derives from the radius -- it does not depend on the
 *                    mask, so there is no lower bound on A_g / n -- their emitted lists are cut by
 *                    the mask and the survivors rescored exactly.  Possible whenever
 *                    bsr_local_range_search would filter; otherwise the list scan.  A query the
 *                    threshold cannot serve (a zero / tiny / huge query, a radius near 1 or above),
 *                    or whose emitted list overflowed, takes the list scan on its own;
 *   BSR_MASK_LIST    every query takes the list scan: an exact range over the list of its mask's
 *                    live rows, cost proportional to A_g;
 *   BSR_MASK_AUTO    per group: the list where bsr_local_top_k_masked's rule prefers it, or where
 *                    A_g / n < capacity / (2 L), L = min(8192, max(1024, 2 capacity)) the keys of
 *                    an emitted list -- 1/8 up to 512 slots: results
 *                    that about fill their capacity then overflow the emitted lists (the filter
 *                    emits from the whole shard) and would pay both paths.
 * The full-shard scan never runs here.  bsr_search_stats: search_path carries BSR_PATH_RANGE,
 * BSR_PATH_MASK_FILTER when the filter pass ran, BSR_PATH_MASK_LIST when any query was answered
 * by the list scan, BSR_PATH_MASK_GROUPS when a query_mask was given, never BSR_PATH_RANGE_SCAN;
 * n_exact_direct = the queries sent to the list scan by design (by mode, by AUTO, or because they
 * cannot filter), n_fallback = the queries whose emitted list overflowed, n_emitted = the emitted
 * keys before the cut.  The row lists are built in chunks of at most BSR_MASK_LIST_BUDGET bytes
 * of ids (a long list is split over chunks).
 * Out of scope: a multi-rank masked range search (every rank calls this on its shard and the
 * caller concatenates); a CSR output. */
int bsr_local_range_search_masked(bsr_index* ix, const float* queries, uint32_t n_queries,
                                  const float* radius, uint32_t capacity,
                                  const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                  const uint32_t* query_mask, uint32_t mode,
                                  uint64_t* out_idx, float* out_dist, uint32_t* out_count);

/* ---- MMR search: a diversified top-k (maximal marginal relevance) over the exact candidates.
 * For a query whose neighbourhood is a cluster of near-duplicates the exact top-k is k copies of
 * one passage; MMR fetches fetch_k candidates and picks k of them greedily, trading closeness to
 * the query against closeness to what is already picked.  The result is one bit pattern
 * (DESIGN.md §18).  For one query:
 *   1. the candidates are exactly what bsr_local_top_k returns for k = fetch_k (with allow masks:
 *      bsr_local_top_k_masked / bsr_local_top_k_masked_groups): m = min(fetch_k, allowed live rows)
 *      positions 0 .. m-1 in (distance asc, global index asc) order, each with its query distance
 *      dq_i, the reference's f32 bits;
 *   2. D(i, j) is the reference's cosine_distance of the stored rows of positions i and j (the
 *      sequential f32 dot in index order, the max |a - b| identical shortcut, the zero-magnitude
 *      rule, the stored magnitudes); symmetric bit for bit; on a bf16 index the stored rows are the
 *      widened f32 values;
 *   3. lam = lambda as f32, mu = 1.0f - lam (one f32 subtraction);
 *   4. the first pick is position 0, the nearest row;
 *   5. every later pick: for each unpicked i, mind_i = fminf(mind_i, D(i, last pick)) (from +inf),
 *      score_i = (mu * mind_i) - (lam * dq_i) -- two f32 multiplies and one f32 subtraction, each
 *      rounded on its own, no FMA -- and the largest score wins, ties to the smallest position;
 *   6. out_count[q] = min(k, m); row q holds the picks in selection order: out_idx the global
 *      index, out_dist dq of the pick, out_rank (nullable) its position in the candidate list;
 *      past the count (~0, +inf, ~0u).
 * lambda = 1 returns bsr_local_top_k(k) bit for bit; pick 0 is always the top-1; with k = fetch_k
 * the output is a permutation of the candidate list; exact duplicates of a picked row get mind = 0
 * and drop to the bottom.
 * allow == NULL: the plain search finds the candidates (n_masks must be 0, query_mask NULL), with
 * its captured graphs: graph_replay is 1 wherever bsr_local_top_k(n_queries, fetch_k) would replay.
 * allow != NULL: bsr_local_range_search_masked's contract for allow, allow_words, n_masks,
 * query_mask and mode (query_mask == NULL is legal only with n_masks == 1).
 * 1 <= k <= fetch_k <= cfg.max_k; lambda finite and within [0, 1].  queries, the masks and the
 * four outputs are, independently, host or device pointers, detected per call.
 * The checks, in this order; the caller's arrays are untouched on every error:
 *   1. BSR_E_INVALID before any device is touched: a null index; k or fetch_k out of range; a NaN
 *      or out-of-range lambda; an inconsistent mask argument set (allow NULL with n_masks != 0 or a
 *      query_mask; allow with n_masks == 0; a null query_mask with n_masks > 1); an unknown mode;
 *      with n_queries > 0 a null queries pointer or a null out_idx / out_dist / out_count;
 *   2. BSR_E_STATE: the index is not loaded;
 *   3. n_queries = 0: BSR_OK;
 *   4. everything else as the candidate search reports it: allow_words != ceil(n / 64), a
 *      query_mask entry >= n_masks, BSR_E_NONFINITE for a non-finite query, BSR_E_DIM.
 * bsr_search_stats: search_path carries the candidate search's bits plus BSR_PATH_MMR; the other
 * fields are the candidate search's.
 * Out of scope: multi-rank MMR (the pair distances need rows of other ranks: run the parallel
 * search for ids, then MMR on the rank that holds the rows); a per-query lambda; another diversity
 * measure; returning D. */
int bsr_local_top_k_mmr(bsr_index* ix, const float* queries, uint32_t n_queries,
                        uint32_t k, uint32_t fetch_k, float lambda,
                        const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                        const uint32_t* query_mask, uint32_t mode,
                        uint64_t* out_idx, float* out_dist, uint32_t* out_rank /* nullable */,
                        uint32_t* out_count);

/* ---- Collapsed search: the exact top-k of distinct groups, the best row of each (field
 * collapsing, DISTINCT ON).  The rows of a shard are often chunks of documents, and the exact top-k
 * of a query several chunks of one document; this call returns the k best documents, each with its
 * best chunk, exactly and in one call.
 * row_group[i] < n_groups is the group of local row i.  It is passed per call, like an allow mask,
 * and never stored on the index: load, append, delete, update and compact do not know it, and after
 * a compaction the caller remaps it through out_old_ids.  row_group_len must equal the index's row
 * count; row_group is host or device memory, detected per call (a host array is copied into a
 * buffer the index keeps).
 * For one query, over the rows that are live and allowed (masks exactly as bsr_local_top_k_mmr
 * takes them):
 *   1. the head of a group is its row that comes first in (reference distance asc, global index
 *      asc) order;
 *   2. the result is the heads of the k groups whose heads come first in that same order;
 *   3. out_count[q] = min(k, distinct groups among the allowed live rows);
 *   4. row q holds (global index, the reference's f32 distance bits, group id in out_group,
 *      nullable) in (distance asc, index asc) order, then (~0, +inf, ~0u).
 * row_group[i] = i with n_groups = n is bsr_local_top_k(k) bit for bit; all rows in one group
 * gives the top-1; the result is the same for every legal fetch_k.
 * fetch_k is the length of the exact candidate list (bsr_local_top_k / _masked / _masked_groups
 * with k = fetch_k) the call walks first: a query whose list shows k groups, or holds every allowed
 * live row, is answered from it.  Any other query takes an exact scan of the shard that keeps the
 * best row of every group in a table of 8 * n_groups bytes, in rounds of up to 8 queries and of at
 * most BSR_COLLAPSE_TABLE_BUDGET bytes of tables (read from the environment per call, 256 MB by
 * default; at least one query a round).  The scan reads the whole shard even under a sparse mask:
 * it is the fallback, so choose fetch_k to make it rare.  The tables are allocated at the first
 * scan that needs them and kept; like the first update of its size, that allocation makes the plain
 * search re-capture its graph once.
 * 1 <= k <= fetch_k <= cfg.max_k; n_groups >= 1.  queries, row_group, the masks and the four
 * outputs are, independently, host or device pointers.
 * The checks, in this order; the caller's arrays are untouched on every error:
 *   1. BSR_E_INVALID before any device is touched: a null index; k = 0, k > fetch_k or fetch_k >
 *      cfg.max_k; n_groups = 0; an inconsistent mask argument set (bsr_local_top_k_mmr's); an
 *      unknown mode; with n_queries > 0 a null queries pointer or a null out_idx / out_dist /
 *      out_count;
 *   2. BSR_E_STATE: the index is not loaded;
 *   3. BSR_E_INVALID: row_group_len != the index's rows, or a null row_group with rows;
 *   4. n_queries = 0: BSR_OK;
 *   5. BSR_E_INVALID, found on the device: a row_group entry >= n_groups;
 *   6. everything else as the candidate search reports it: allow_words != ceil(n / 64), a
 *      query_mask entry >= n_masks, BSR_E_NONFINITE for a non-finite query, BSR_E_DIM.
 * An empty shard gives every count 0.
 * bsr_search_stats: search_path carries the candidate search's bits plus BSR_PATH_COLLAPSE, and
 * BSR_PATH_COLLAPSE_SCAN when a query of the batch took the group scan; the other fields are the
 * candidate search's, and graph_replay is 1 wherever bsr_local_top_k(n_queries, fetch_k) would
 * replay.
 * More than one row per group ("at most m per document") is bsr_local_top_k_capped, below; a
 * multi-rank collapsed search is this call on every rank with out_group, bsr_allgather_bytes and
 * bsr_global_top_k_capped with per_group = 1.
 * Out of scope: group ids stored on the index; a parallel entry point that runs those collectives
 * itself; a list-driven scan for sparse masks; group sizes or counts in the output. */
int bsr_local_top_k_collapsed(bsr_index* ix, const float* queries, uint32_t n_queries,
                              uint32_t k, uint32_t fetch_k,
                              const uint32_t* row_group, uint64_t row_group_len, uint32_t n_groups,
                              const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                              const uint32_t* query_mask, uint32_t mode,
                              uint64_t* out_idx, float* out_dist, uint32_t* out_group /* nullable */,
                              uint32_t* out_count);

/* ---- Capped search: the exact top-k with at most per_group rows of any one group ("the k nearest
 * chunks, no more than m from one document"), between bsr_local_top_k (k rows, any groups) and
 * bsr_local_top_k_collapsed (one row of each of k groups), exactly and in one call.
 * row_group, row_group_len, n_groups, the masks, mode and fetch_k are taken exactly as
 * bsr_local_top_k_collapsed takes them.  For one query, over the rows that are live and allowed,
 * with m = per_group:
 *   1. order the rows by (reference distance asc, global index asc);
 *   2. a row is kept when fewer than m rows of its group come before it in that order;
 *   3. the result is the first k kept rows, in that order;
 *   4. out_count[q] = min(k, sum over the groups of min(m, the group's allowed live rows));
 *   5. row q holds (global index, the reference's f32 distance bits, group id in out_group,
 *      nullable), then (~0, +inf, ~0u).
 * per_group = 1 is bsr_local_top_k_collapsed byte for byte; per_group >= k is bsr_local_top_k(k)
 * bit for bit and never scans; all rows in one group gives the top-min(m, k); the result is the
 * same for every legal fetch_k.
 * The candidate list of length fetch_k is a prefix of the order, so every earlier row of a listed
 * row's group is listed too, and counting groups along the list decides "kept" exactly.  A query
 * whose list keeps k rows, or holds every allowed live row, is answered from it.  Any other query
 * takes an exact scan of the shard that keeps the min(m, k) best rows of every group in a table of
 * 8 * min(m, k) * n_groups bytes, in rounds of up to 8 queries and of at most
 * BSR_COLLAPSE_TABLE_BUDGET bytes of tables (the collapsed search's variable, read per call; at
 * least one query a round).  The tables are the collapsed search's buffer, allocated at the first
 * scan that needs them and kept; that allocation makes the plain search re-capture its graph once.
 * 1 <= k <= fetch_k <= cfg.max_k; 1 <= per_group <= BSR_CAP_MAX_PER_GROUP; n_groups >= 1.  queries,
 * row_group, the masks and the four outputs are, independently, host or device pointers.
 * The checks, in this order; the caller's arrays are untouched on every error:
 *   1. BSR_E_INVALID before any device is touched: a null index; k = 0, k > fetch_k or fetch_k >
 *      cfg.max_k; per_group = 0 or above BSR_CAP_MAX_PER_GROUP; n_groups = 0; min(per_group, k) *
 *      n_groups > 2^32 - 1 (a table's entries are counted in 32 bits); an inconsistent mask argument
 *      set (bsr_local_top_k_mmr's); an unknown mode; with n_queries > 0 a null queries pointer or a
 *      null out_idx / out_dist / out_count;
 *   2. to 6.: bsr_local_top_k_collapsed's, word for word.
 * bsr_search_stats: search_path carries the candidate search's bits plus BSR_PATH_CAP (never
 * BSR_PATH_COLLAPSE), and BSR_PATH_CAP_SCAN when a query of the batch took the scan; the other
 * fields are the candidate search's, and graph_replay is 1 wherever bsr_local_top_k(n_queries,
 * fetch_k) would replay.
 * A multi-rank capped search: this call on every rank with its own row_group (global group ids)
 * and out_group, bsr_allgather_bytes of the four outputs, bsr_global_top_k_capped.
 * Out of scope: "k groups with up to m rows each"; a per-query per_group; group ids stored on the
 * index; a list-driven scan for sparse masks; counts per group in the output. */
#define BSR_CAP_MAX_PER_GROUP 16u
int bsr_local_top_k_capped(bsr_index* ix, const float* queries, uint32_t n_queries,
                           uint32_t k, uint32_t fetch_k, uint32_t per_group,
                           const uint32_t* row_group, uint64_t row_group_len, uint32_t n_groups,
                           const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                           const uint32_t* query_mask, uint32_t mode,
                           uint64_t* out_idx, float* out_dist, uint32_t* out_group /* nullable */,
                           uint32_t* out_count);

/* ---- score given ids: the distances of rows the caller already has ("BM25 gave me these 300
 * chunk ids: how far is each from the query?", "re-check yesterday's answer", "rerank the list I
 * assembled from several searches").  a-1 (bsr_cosine_distance) batched against STORED rows:
 * ids[q][0 .. m) is query q's list of GLOBAL ids, as the searches return them.
 * A slot is PRESENT when its id lies in [global_offset, global_offset + n) and its row is not
 * deleted (bsr_index_delete).  Every other slot is ABSENT and never an error: the padding value ~0
 * (ragged lists are padded with it), an id of another rank's shard, a deleted row.  So the
 * multi-rank form needs no routing: every rank scores the same ids, and the element-wise fminf of
 * the ranks' out_dist is the answer over the whole store -- an id is present on at most one rank.
 * bsr_local_score_ids: out_dist[q][j] of a present slot is the reference's f32 distance of stored
 *   row ids[q][j] to query q (src/metrics.rs:143-165: the sequential f32 dot in index order with no
 *   FMA, the max|a-b| <= 1e-10 identical shortcut, a zero magnitude gives 1.0, the row's stored
 *   magnitude), bit for bit what bsr_local_top_k returns for that row; of an absent slot +inf.
 *   out_found[q] (nullable) = the present slots of row q.  An id may repeat: every slot gets its
 *   value and counts.  m has no limit but n_queries * m < 2^32.
 * bsr_local_rerank_ids: row q of out_idx / out_dist ([n_queries][k]) holds the DISTINCT present
 *   ids of list q in (distance asc, global index asc) order, the first out_count[q] = min(k, distinct
 *   present ids) of them, and (~0, +inf) behind them.  1 <= k <= m <= BSR_SCORE_MAX_IDS; k is not
 *   bounded by cfg.max_k (the call owns its buffers).
 * queries, ids and every output are, independently, host or device pointers, detected per call;
 * device inputs follow the stream rule of device queries.
 * The checks, in this order; the caller's arrays are untouched on every error:
 *   1. BSR_E_INVALID before any device is touched: a null index; m = 0; n_queries * m >= 2^32;
 *      rerank only: k = 0, k > m or m > BSR_SCORE_MAX_IDS; with n_queries > 0 a null queries, ids
 *      or mandatory output (out_found alone may be null);
 *   2. BSR_E_STATE: the index is not loaded;
 *   3. n_queries = 0: BSR_OK;
 *   4. BSR_E_NONFINITE: a non-finite query, read from the batch's status words before any of the
 *      caller's arrays, host or device, is written.
 * An empty shard: every slot absent, every count 0.  A bf16 index scores the widened stored values,
 * as every search does.  BSR_FLAG_EXACT_ONLY and the sticky norm flags do not matter: no filter
 * runs, and no filter operand of the queries is built.
 * How: one kernel, a wave per 64 consecutive slots of a list, lane = slot -- the range search's
 * rescore walk driven by the ids; no address is formed from an id that failed the interval check.
 * The rerank adds one workgroup per query that sorts the present slots' keys in LDS, as a range
 * result is sorted, and drops repeats.  Never graph-replayed; the plain search's graphs are left
 * alone (the first call of a size allocates, and that makes the plain search re-capture once, as
 * any allocation does).  bsr_search_stats: search_path = BSR_PATH_SCORE, n_queries,
 * n_candidates = m, every other field 0.  BSR_FLAG_PROFILE: the kernels in rescore_ms /
 * rescore_launches, the call in search_ms.
 * Out of scope: one id list shared by the whole batch (bsr_local_top_k_masked with BSR_MASK_LIST);
 * queries named by stored id; a collective that runs the fminf exchange itself; fused hybrid
 * scoring (the caller fuses the two scores). */
#define BSR_SCORE_MAX_IDS 4096u /* rerank only: the list is sorted in LDS, as a range result is */
int bsr_local_score_ids(bsr_index* ix, const float* queries, uint32_t n_queries,
                        const uint64_t* ids, uint32_t m,      /* [n_queries][m] GLOBAL ids */
                        float* out_dist,                      /* [n_queries][m], aligned with ids */
                        uint32_t* out_found /* [n_queries], nullable */);
int bsr_local_rerank_ids(bsr_index* ix, const float* queries, uint32_t n_queries,
                         const uint64_t* ids, uint32_t m, uint32_t k,
                         uint64_t* out_idx, float* out_dist,  /* [n_queries][k] */
                         uint32_t* out_count /* [n_queries] */);

/* ---- The merge of per-rank capped (or collapsed: per_group = 1) lists, on the host.  Layout and
 * null rules are bsr_global_top_k's, with group[(l*n_queries+q)*k_in ..] the group ids beside idx
 * and dist (global group ids: a group may span ranks) and out_group [n_queries][k] (nullable).
 * Per query: the lists concatenated, ordered by (distance asc, index asc), deduplicated by index; a
 * row is kept while fewer than per_group kept rows hold its group; the first k kept rows.  Entries
 * past out_count[q] are (~0, +inf, ~0u).  Over per-rank results of bsr_local_top_k_capped(k,
 * per_group) (k_in = k) this is the capped search over the whole store.
 * BSR_E_INVALID: a null array (group included, when there are entries), k = 0, per_group = 0 (there
 * is no upper cap here), any array in device memory (a device merge is out of scope).
 * BSR_E_NONFINITE: a NaN distance. */
int bsr_global_top_k_capped(const uint64_t* idx, const float* dist, const uint32_t* group, const uint32_t* count,
                            uint32_t n_lists, uint32_t n_queries, uint32_t k_in, uint32_t k, uint32_t per_group,
                            uint64_t* out_idx, float* out_dist, uint32_t* out_group /* nullable */,
                            uint32_t* out_count);

/* ---- a-5: compute_global_top_k over n_lists per-rank lists, for n_queries queries.
 * Input list l of query q: idx[(l*n_queries+q)*k_in ..] with count[l*n_queries+q]
 * entries.  Rank-order concatenation + stable sort by distance + dedupe, keep k.
 * Host arrays: merged on the host (threads over queries).  Every array in device memory
 * (n_lists <= 64, n_lists * k_in <= 1024, k <= 256): merged on the GPU, one wave per query
 * (the RCCL path's root merge).  Rows past out_count[q] are (~0, +inf). -------------- */
int bsr_global_top_k(const uint64_t* idx, const float* dist, const uint32_t* count,
                     uint32_t n_lists, uint32_t n_queries, uint32_t k_in, uint32_t k,
                     uint64_t* out_idx, float* out_dist, uint32_t* out_count);

/* ---- communicator (replaces the MPI world; RCCL over xGMI) ----------------------- */
#define BSR_UNIQUE_ID_BYTES 128
int bsr_comm_unique_id(uint8_t out_id[BSR_UNIQUE_ID_BYTES]); /* on rank 0; broadcast it */
int bsr_comm_init(const uint8_t id[BSR_UNIQUE_ID_BYTES], int32_t rank, int32_t size,
                  int32_t device, bsr_comm** out);
void bsr_comm_destroy(bsr_comm* comm);
int bsr_comm_rank(const bsr_comm* comm, int32_t* rank, int32_t* size);

/* Host transport for bsr_comm_init_host: an all-gather of `bytes` bytes from every rank
 * into recv (size * bytes, rank order), called collectively by every rank.  Returns 0 on
 * success.  Lets a caller run the exchange over its own transport (MPI, gloo, a test
 * harness) with the same gather + merge code as the RCCL path. */
typedef int (*bsr_host_allgather_fn)(const void* send, void* recv, uint64_t bytes, void* user);
int bsr_comm_init_host(int32_t rank, int32_t size, bsr_host_allgather_fn fn, void* user,
                       bsr_comm** out);

/* Loopback communicator (measurement and tests, not a transport): ONE process on one GPU acting
 * as rank `rank` of `size`.  Every all-gather is emulated by one device kernel enqueued exactly
 * where ncclAllGather would be (same stream, no host wait), so a parallel search runs the RCCL
 * path's enqueue-only control flow and its per-rank device timeline.  Without a script
 * (n_calls = 0) each all-gather gives every slot this rank's own contribution.  With one, the
 * all-gathers of each bsr_parallel_top_k_similarity_search replay, in order, the contributions
 * recorded in a real size-rank run of the same batch (call i: call_bytes[i] bytes per rank,
 * script holds its [size][call_bytes[i]] receive buffer, calls concatenated); this rank's slot
 * is always its live contribution, and a call that does not match the recording (another
 * size, past its end) replicates from then on in that search.  Broadcasts are no-ops. */
int bsr_comm_init_loopback(int32_t rank, int32_t size, int32_t device, uint32_t n_calls,
                           const uint64_t* call_bytes, const void* script, bsr_comm** out);
/* All-gathers replayed from the script and calls that missed it, since creation. */
int bsr_comm_loopback_stats(const bsr_comm* comm, uint64_t* replayed, uint64_t* missed);

/* ---- a-4: gather_top_k_results.  Every rank passes its [n_queries][k] local lists;
 * the root (rank 0) receives [size][n_queries][k] lists + counts in rank order
 * (host buffers, may be NULL on non-root ranks).  Collective: every rank calls it. ---- */
int bsr_gather_top_k(bsr_comm* comm, const uint64_t* local_idx, const float* local_dist,
                     const uint32_t* local_count, uint32_t n_queries, uint32_t k,
                     uint64_t* root_idx, float* root_dist, uint32_t* root_count);

/* ---- a-4 + a-5 composed (the exchange step of a-6): every rank passes its
 * [n_queries][k] local lists (host or device; all three NULL = an empty contribution, what
 * the reference sends after a local error, src/mpi_helpers/metrics.rs:185-191); the root
 * gets the global top-k (rank-order concatenation, stable sort by distance, dedupe by
 * index, :141-171) in out_*; other ranks get out_count[q] = 0.  Collective. ---------- */
int bsr_gather_global_top_k(bsr_comm* comm, const uint64_t* local_idx, const float* local_dist,
                            const uint32_t* local_count, uint32_t n_queries, uint32_t k,
                            uint64_t* out_idx, float* out_dist, uint32_t* out_count);

/* ---- a-6: parallel_top_k_similarity_search (src/mpi_helpers/metrics.rs:174-206) for a batch
 * of n_queries queries.  The root (rank 0) gets the global top-k in out_* (the reference's
 * Some(global_top_k)); other ranks get out_count[q] = 0 (its None).  comm may be NULL for a
 * single-rank run (the local lists are the result).  Collective: every rank calls it.
 *
 * With size > 1 every rank first all-gathers a 32-byte header {n_queries, k, local status,
 * magic, eligible for the global threshold, shard rows (2 words), 0}.  Ranks that disagree on
 * n_queries or k all return BSR_E_INVALID and no lists move.  Then one of two paths, the same
 * on every rank:
 *   - the global-threshold path (every rank eligible: n_queries > 16, k <= 200, a shard of
 *     more rows than one query's candidate list, size <= 64, size * k <= 1024; the library
 *     setting BSR_GLOBAL_TAU=0 turns it off): every rank all-gathers its best sample keys,
 *     emits against the threshold the whole corpus's sample selects, rescores every row it
 *     emitted exactly and all-gathers its packed result (lists, status words, per-query
 *     exclusion bounds).  EVERY rank merges the gathered lists on its GPU and certifies each
 *     merged list against every rank's bound; the uncertified queries (usually none) take the
 *     standard path below, collectively, and replace the root's rows;
 *   - the standard path: each rank's certified local top-k (bsr_local_top_k), the all-gather
 *     of the [n_queries][k] lists and the root's merge on its GPU (bsr_gather_global_top_k).
 * A rank whose local step fails (bad arguments, device mismatch, a failed search) still takes
 * part in every collective with an empty list (:185-191): a non-root rank then returns its
 * error; the root returns BSR_PARTIAL with the other ranks' global top-k in out_* (the
 * reference's root still returns Some(..), :199-202) and the message in bsr_last_error().
 * Over RCCL every step is enqueued on the device with one host wait at the end; over a host
 * transport each all-gather is a host round trip. ------------------------------------------ */
int bsr_parallel_top_k_similarity_search(bsr_comm* comm, bsr_index* ix, const float* queries,
                                         uint32_t n_queries, uint32_t k, uint64_t* out_idx,
                                         float* out_dist, uint32_t* out_count);

/* ---- pinned host buffers for results (round 5): coherent (fine-grained) pinned host memory.  Root
 * outputs of bsr_parallel_top_k_similarity_search in such memory are written by the GPU directly
 * on the global-threshold path (no staging copy after the search); any other host memory works
 * everywhere, through a copy. -------------------------------------------------------------- */
int bsr_host_alloc(uint64_t bytes, void** out);
void bsr_host_free(void* p);

/* ---- driver collectives: src/main.rs:123-125 (process_at_rank(ROOT).broadcast_into of the
 * query) and the timing gather of src/mpi_helpers/benchmark.rs:131-293.  Host or device
 * buffers; collective over the comm (RCCL or host transport). ------------------------ */
int bsr_broadcast(bsr_comm* comm, void* buf, uint64_t bytes, int32_t root);
int bsr_allgather_bytes(bsr_comm* comm, const void* send, void* recv, uint64_t bytes);

/* ---- diagnostics ------------------------------------------------------------------ */
int bsr_index_last_stats(const bsr_index* ix, bsr_search_stats* out);
int bsr_index_profile(bsr_index* ix, bsr_profile* out, int reset);
/* Which stages of a BSR_FLAG_PROFILE index record HIP events: 0 = none (the product path:
 * filtered batches replay a captured hipGraph), 1 = the filter / scan kernels only, 2 = every
 * stage (the default).  At levels 1 and 2 a search launches its kernels directly, with the
 * events recorded on the stream around them (how kernel durations are timed). */
int bsr_index_set_profile(bsr_index* ix, int level);

/* ---- synthetic data (bench / tests): U(-1,1) f32 from a counter-based hash of
 * (seed, global element index), written on the device: value(row, col) for rows
 * [row0, row0+n_rows).  Identical on every rank and GPU. --------------------------- */
int bsr_synth_uniform(float* dev_out, uint64_t row0, uint64_t n_rows, uint32_t dim,
                      uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* BSR_H */
