// index.cpp -- the rank's corpus shard in HBM and the local search pipeline
// (compute_local_top_k, src/mpi_helpers/metrics.rs:16-53, for a batch of queries).
//
// Pipeline for a batch, all on the index's stream:
//   1. query prep     exact |b| (src/metrics.rs:155), flags, the filter operand (int8 + scale)
//                     and the per-query certification bound E_q
//   2. sample filter  MFMA scores of every 32nd row -> tau0 (per query)
//   3. emit filter    MFMA scores of every row; rows with score >= tau0 -> candidates
//   4. select         top-(k'+1) candidates by approximate score
//   5. rescore        exact sequential-f32 distances of k' candidates, top-k, certify
//   6. one status readback; fallback: exact full scan of any uncertified / ineligible query
// k > 200, or an index with out-of-range norms, use the exact scan only.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <algorithm>

#include "internal.hpp"
#include "kernels.hpp"

namespace bsr {

constexpr uint32_t kMaxKForFilter = 200;

static thread_local std::string g_err;

int set_error(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
void clear_error() { g_err.clear(); }
const char* last_error_cstr() { return g_err.c_str(); }

std::atomic<uint64_t> g_alloc_gen{0};

int DevBuf::ensure(size_t need) {
    if (need <= bytes && p) return BSR_OK;
    release();
    ++g_alloc_gen;
    if (need == 0) need = 16;
    hipError_t e = hipMalloc(&p, need);
    if (e != hipSuccess) {
        p = nullptr;
        bytes = 0;
        (void)hipGetLastError();
        return set_error(BSR_E_NOMEM, "hipMalloc(%zu bytes) failed: %s", need, hipGetErrorString(e));
    }
    bytes = need;
    return BSR_OK;
}
void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}
int DevBuf::grow(size_t need, size_t keep, hipStream_t s) {
    if (p && bytes >= need) return BSR_OK;
    DevBuf grown;
    BSR_TRY(grown.ensure(need));
    BSR_HIP(hipMemsetAsync(grown.p, 0, need, s));
    if (p && keep) BSR_HIP(hipMemcpyAsync(grown.p, p, keep, hipMemcpyDeviceToDevice, s));
    BSR_HIP(hipStreamSynchronize(s));
    std::swap(p, grown.p);
    std::swap(bytes, grown.bytes);
    return BSR_OK;
}

// Completion of a search's work on its stream, polled (hipStreamQuery) rather than blocked on:
// a blocking synchronize wakes the host ~15 us after the GPU finishes (measured: the D2H copy
// ends, the next host call comes 15 us later), which is idle GPU time between batches.
hipError_t stream_wait(hipStream_t s) {
    for (;;) {
        const hipError_t r = hipStreamQuery(s);
        if (r != hipErrorNotReady) return r;
        __builtin_ia32_pause();
    }
}

// A published search (its last kernel raises *flag after copying the result to host memory):
// spin on the flag, and now and then ask the stream -- a stream that has finished (or failed)
// without raising it is an error, never an endless wait.
hipError_t flag_wait(const uint32_t* flag, hipStream_t s) {
    for (uint32_t i = 1;; ++i) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE)) return hipSuccess;
        if ((i & 4095) == 0) {
            const hipError_t r = hipStreamQuery(s);
            if (r == hipSuccess) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) ? hipSuccess : hipErrorUnknown;
            if (r != hipErrorNotReady) return r;
        }
        __builtin_ia32_pause();
    }
}

bool is_device_ptr(const void* p) {
    if (!p) return false;
    // no device visible (host-only entry points on a CPU machine): every pointer is host
    static const bool have_device = [] {
        int n = 0;
        const bool ok = hipGetDeviceCount(&n) == hipSuccess && n > 0;
        (void)hipGetLastError();
        return ok;
    }();
    if (!have_device) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// The device address of coherent (fine-grained) pinned host memory -- hipHostMalloc with
// hipHostMallocCoherent, e.g. bsr_host_alloc -- else nullptr (pageable memory, device memory,
// or non-coherent pinned memory, which the host could read stale from its caches).
void* coherent_host_alias(const void* p) {
    if (!p) return nullptr;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (attr.type != hipMemoryTypeHost || !(attr.allocationFlags & hipHostMallocCoherent) || !attr.devicePointer)
        return nullptr;
    return attr.devicePointer;
}

int select_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        return set_error(BSR_E_NODEVICE, "no HIP device visible (this engine has no CPU path)");
    }
    if (device >= 0) {
        if (device >= n) return set_error(BSR_E_INVALID, "device %d out of range (%d visible)", device, n);
        BSR_HIP(hipSetDevice(device));
    }
    return BSR_OK;
}

Events::~Events() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
}
int Events::create() {
    if (!a) BSR_HIP(hipEventCreate(&a));
    if (!b) BSR_HIP(hipEventCreate(&b));
    return BSR_OK;
}

}  // namespace bsr

using namespace bsr;

// ---------------------------------------------------------------------------------------
// profiling helpers
// ---------------------------------------------------------------------------------------
// Events exist when the index was created with BSR_FLAG_PROFILE; prof_level (bsr_index_set_profile)
// picks which stages record them: 1 = the emit filter / scan kernels only (the bench's timed
// steps: each recorded event is one more node in the search graph), 2 = every stage.
static inline bool profiling(const bsr_index* ix) { return (ix->cfg.flags & BSR_FLAG_PROFILE) != 0; }
static inline void ev_begin(bsr_index* ix, Events& e, int level = 2) {
    if (profiling(ix) && ix->prof_level >= level && e.a) { (void)hipEventRecord(e.a, ix->stream); e.armed = true; }
}
static inline void ev_end(bsr_index* ix, Events& e) {
    if (profiling(ix) && e.armed) (void)hipEventRecord(e.b, ix->stream);
}
// A filter / scan kernel launch timed at profile level >= 1: HIP events recorded on the stream
// around a direct launch (so the start event completes when the stream reaches the kernel).
// Two other forms were measured wrong on ROCm 7.2 (profiles/r04m_*): the events bound to the
// launch by hipExtLaunchKernel start at the kernel's submission -- behind the sample pass and
// tau selection still running, +0.2 ms on a 5.57 ms kernel -- and event-record nodes inside a
// replayed graph timed from the graph's start (6.12 ms).  Timed searches are therefore never
// graph-replayed (level 0 is the product path).
template <class F>
static inline hipError_t launch_timed(bsr_index* ix, Events& e, F&& launch, int level = 1) {
    const bool timed = !ix->capturing && profiling(ix) && ix->prof_level >= level && e.a;
    if (!timed) return launch();
    hipError_t r = hipEventRecord(e.a, ix->stream);
    if (r == hipSuccess) r = launch();
    if (r == hipSuccess) r = hipEventRecord(e.b, ix->stream);
    e.armed = r == hipSuccess;
    return r;
}
static inline void ev_collect(Events& e, double& ms, uint64_t& n, uint64_t launches) {
    if (!e.armed) return;
    float t = 0.0f;
    if (hipEventElapsedTime(&t, e.a, e.b) == hipSuccess) { ms += t; n += launches; }
    e.armed = false;
}

// ---------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------
// An input that may be host memory, on the device: a device pointer (dev) as it is, host memory
// copied into buf on the index's stream.
template <class T>
static int on_device(bsr_index* ix, DevBuf& buf, const T* src, size_t bytes, bool dev, const T** out) {
    *out = src;
    if (dev) return BSR_OK;
    BSR_TRY(buf.ensure(bytes));
    BSR_HIP(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ix->stream));
    *out = buf.as<T>();
    return BSR_OK;
}
// A byte budget from the environment (read per call): a decimal number, else the default.
static uint64_t env_bytes(const char* name, uint64_t dflt) {
    const char* v = getenv(name);
    if (v && v[0]) {
        char* end = nullptr;
        const unsigned long long x = strtoull(v, &end, 10);
        if (end != v) return x;
    }
    return dflt;
}
// The device's row flags and int8 row error bound, read back (one stream wait), and what follows
// from them: whether the filter may serve this index.
static int read_row_state(bsr_index* ix) {
    uint32_t f[2] = {0, 0};
    BSR_HIP(hipMemcpyAsync(f, ix->flags.p, sizeof f, hipMemcpyDeviceToHost, ix->stream));
    BSR_HIP(hipStreamSynchronize(ix->stream));
    ix->row_flags = f[0];
    memcpy(&ix->row_ebound, &f[1], sizeof(float));
    ix->approx_ok = !(f[0] & (kRowNormOvf | kRowNormRange)) && !(ix->cfg.flags & BSR_FLAG_EXACT_ONLY);
    return BSR_OK;
}

// ---------------------------------------------------------------------------------------
// load / append
// ---------------------------------------------------------------------------------------
static int index_prepare_rows(bsr_index* ix, const void* rows, uint64_t n_rows, uint64_t first_row) {
    // Copy rows [first_row, first_row+n_rows) of the padded slab from the caller's buffer.
    float* dst = ix->rows.as<float>() + first_row * ix->ld;
    const bool dev = is_device_ptr(rows);
    const size_t elem = ix->cfg.dtype == BSR_BF16 ? 2 : 4;
    const void* src = nullptr;
    // Device rows may still be in flight on ANY stream of the caller (a torch side stream, a
    // communication stream): the ABI has no stream argument, and a load runs once, outside
    // any timed region, so a full device synchronize costs nothing and removes the hazard.
    if (dev) BSR_HIP(hipDeviceSynchronize());
    BSR_TRY(on_device(ix, ix->tmp, rows, n_rows * (size_t)ix->dim * elem, dev, &src));
    if (ix->cfg.dtype == BSR_BF16)
        BSR_HIP(launch_widen_bf16_rows(static_cast<const uint16_t*>(src), n_rows, ix->dim, ix->ld, dst, ix->stream));
    else
        BSR_HIP(launch_copy_rows_f32(static_cast<const float*>(src), n_rows, ix->dim, ix->ld, dst, ix->stream));
    return BSR_OK;
}

// Per-row state: the reference's magnitudes, row flags and the filter operand.
static int index_finish_load(bsr_index* ix) {
    BSR_TRY(ix->na.ensure(ix->n_pad * sizeof(float)));
    BSR_TRY(ix->fop.ensure((size_t)ix->n_pad * ix->op_row_bytes));
    BSR_TRY(ix->flags.ensure(2 * sizeof(uint32_t)));
    BSR_HIP(hipMemsetAsync(ix->flags.p, 0, 2 * sizeof(uint32_t), ix->stream));
    BSR_HIP(hipMemsetAsync(ix->na.p, 0, ix->n_pad * sizeof(float), ix->stream));
    if (ix->n) BSR_HIP(launch_row_norms(ix->rows.as<float>(), ix->n, ix->dim, ix->ld, ix->na.as<float>(),
                                        ix->flags.as<uint32_t>(), ix->stream));
    BSR_TRY(ix->ascale.ensure(ix->n_pad / kQuantBlock * sizeof(float)));
    BSR_HIP(launch_rows_to_i8(ix->rows.as<float>(), ix->n, ix->n_pad, ix->dim, ix->ld, ix->fop.as<int8_t>(),
                              ix->ascale.as<float>(), ix->flags.as<uint32_t>() + 1, ix->stream));
    // The sample pass reads every kSampleStride-th row: those rows, contiguous (1/32 of the
    // operand bytes), so that it streams whole rows, quantized with one scale per filter tile
    // of sampled rows (its epilogue then takes integer maxima).
    const uint64_t n_s_pad = sample_rows_pad(ix->n);
    BSR_TRY(ix->fop_s.ensure((size_t)n_s_pad * ix->op_row_bytes));
    BSR_TRY(ix->ascale_s.ensure((size_t)(n_s_pad / kSampleScaleRows) * sizeof(float)));
    BSR_HIP(launch_rows_to_i8_sample(ix->rows.as<float>(), ix->n, ix->dim, ix->ld, ix->fop_s.as<int8_t>(),
                                     ix->ascale_s.as<float>(), ix->stream));
    BSR_TRY(read_row_state(ix));
    if (ix->row_flags & kRowNonFinite) {
        ix->loaded = false;
        ix->n = 0;
        return set_error(BSR_E_NONFINITE, "corpus contains NaN/Inf (the reference panics on NaN distances)");
    }
    ix->loaded = true;
    return BSR_OK;
}

int bsr_index_create_impl(const bsr_config* cfg, bsr_index** out) {
    if (!cfg || !out) return set_error(BSR_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->dim == 0) return set_error(BSR_E_INVALID, "dim must be >= 1");
    if (cfg->dtype != BSR_F32 && cfg->dtype != BSR_BF16) return set_error(BSR_E_INVALID, "unknown dtype");
    // The bf16 filter operand (rounds 1-3) is retired: the int8 operand runs at twice the MFMA
    // rate with an equally tight certification bound; a bf16 CORPUS (dtype)
    // is still served, on the int8 filter.
    if (cfg->flags & BSR_FLAG_FILTER_BF16)
        return set_error(BSR_E_INVALID, "BSR_FLAG_FILTER_BF16 is retired (the filter operand is int8)");
    if (cfg->max_k == 0 || cfg->max_k > BSR_MAX_K)
        return set_error(BSR_E_INVALID, "max_k must be in [1, %u]", BSR_MAX_K);
    BSR_TRY(select_device(cfg->device));
    bsr_index* ix = new (std::nothrow) bsr_index();
    if (!ix) return set_error(BSR_E_NOMEM, "host allocation failed");
    ix->cfg = *cfg;
    int dev = 0;
    (void)hipGetDevice(&dev);
    ix->device = dev;
    ix->dim = cfg->dim;
    ix->ld = (uint32_t)round_up(cfg->dim, kLdAlign);
    ix->op_row_bytes = ix->ld;  // int8 filter operand rows
    // A blocking stream: its work waits for work issued earlier on the legacy default (NULL)
    // stream -- PyTorch's default stream -- so device rows or queries a caller has just
    // produced there are complete before the library reads them (the ABI has no stream
    // argument).  Round 3's 50M test loaded shards whose bf16 conversion was still running on
    // torch's stream into a non-blocking stream: stale rows, wrong results.
    if (hipStreamCreateWithFlags(&ix->stream, hipStreamDefault) != hipSuccess) {
        delete ix;
        return set_error(BSR_E_HIP, "hipStreamCreate failed");
    }
    if (cfg->flags & BSR_FLAG_PROFILE) {
        for (Events* e : {&ix->ev_emit, &ix->ev_sample, &ix->ev_select, &ix->ev_rescore, &ix->ev_scan, &ix->ev_total}) {
            int r = e->create();
            if (r != BSR_OK) { delete ix; return r; }
        }
    }
    *out = ix;
    return BSR_OK;
}

bsr_index::~bsr_index() {
    for (SearchGraph& g : graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (h_res) (void)hipHostFree(h_res);
    if (h_flag) (void)hipHostFree(h_flag);
}

void bsr_index_destroy_impl(bsr_index* ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    (void)hipStreamSynchronize(ix->stream);
    (void)hipStreamDestroy(ix->stream);
    delete ix;
}

int bsr_index_load_impl(bsr_index* ix, const void* rows, uint64_t n_rows, uint64_t global_offset) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    if (n_rows && !rows) return set_error(BSR_E_INVALID, "null rows");
    if (n_rows >= (1ull << 31)) return set_error(BSR_E_INVALID, "shard too large (the reference slices with i32 offsets)");
    BSR_HIP(hipSetDevice(ix->device));
    ix->loaded = false;
    ix->clear_tombstones();  // (a load replaces the contents: every row live)
    ix->n = n_rows;
    ix->n_pad = round_up(n_rows ? n_rows : 1, kRowPad);
    ix->global_offset = global_offset;
    BSR_TRY(ix->rows.ensure(ix->n_pad * (size_t)ix->ld * sizeof(float)));
    BSR_HIP(hipMemsetAsync(ix->rows.p, 0, ix->n_pad * (size_t)ix->ld * sizeof(float), ix->stream));
    if (n_rows) BSR_TRY(index_prepare_rows(ix, rows, n_rows, 0));
    return index_finish_load(ix);
}

int bsr_index_append_impl(bsr_index* ix, const void* rows, uint64_t n_rows) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    if (!n_rows) return BSR_OK;
    if (!rows) return set_error(BSR_E_INVALID, "null rows");
    BSR_HIP(hipSetDevice(ix->device));
    const uint64_t old_n = ix->loaded ? ix->n : 0;
    const uint64_t new_n = old_n + n_rows;
    if (new_n >= (1ull << 31)) return set_error(BSR_E_INVALID, "shard too large");
    const uint64_t new_pad = round_up(new_n, kRowPad);
    const size_t row_bytes = (size_t)ix->ld * sizeof(float);
    BSR_TRY(ix->rows.grow(new_pad * row_bytes, old_n * row_bytes, ix->stream));
    ix->n = new_n;
    ix->n_pad = new_pad;
    // the tombstones are kept and the appended rows are live; the requantised operand of the
    // deleted rows is zeroed again
    int r = index_prepare_rows(ix, rows, n_rows, old_n);
    if (r == BSR_OK) r = index_finish_load(ix);
    if (r == BSR_OK) r = ix->tombstones_after_append();
    if (r != BSR_OK) {
        // n has grown past what the operand and the bitset cover: the index is empty until a load
        ix->loaded = false;
        ix->clear_tombstones();
    }
    return r;
}

int bsr_index_get_many_impl(const bsr_index* ix, uint64_t offset, uint64_t count, float* out) {
    if (!ix || (!out && count)) return set_error(BSR_E_INVALID, "null argument");
    if (!ix->loaded) return set_error(BSR_E_STATE, "index not loaded");
    if (offset > ix->n || count > ix->n - offset) return set_error(BSR_E_INVALID, "slice out of range");
    if (!count) return BSR_OK;
    BSR_HIP(hipSetDevice(ix->device));
    const hipMemcpyKind kind = is_device_ptr(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    BSR_HIP(hipMemcpy2DAsync(out, ix->dim * sizeof(float), ix->rows.as<float>() + offset * ix->ld,
                             ix->ld * sizeof(float), ix->dim * sizeof(float), count, kind, ix->stream));
    BSR_HIP(hipStreamSynchronize(ix->stream));
    return BSR_OK;
}

// ---------------------------------------------------------------------------------------
// tombstones (bsr_index_delete)
// ---------------------------------------------------------------------------------------
// The bitset sized for the padded shard: allocated zeroed, or grown with its contents kept (the
// stream is idle when the old allocation is freed).
static int dead_reserve(bsr_index* ix) {
    return ix->dead.grow(ix->n_pad / 64 * sizeof(uint64_t), ix->dead.bytes, ix->stream);
}

// A deleted row scores exactly 0 in the emit, fix-up and TOP kernels and in the sample tiles, and
// the fop_s sample becomes every 32nd LIVE row (by rank, from the bitset's prefix counts): it
// leaves tau0's order statistics and the candidate lists.  (Speed only: the exact kernels drop it
// whatever it scores.)  After every delete, and after an append -- index_finish_load requantises
// the shard.  Walks the whole bitset and rewrites every deleted row: O(n_dead ld), whatever the
// number of ids of the delete.
static int dead_zero_operand(bsr_index* ix) {
    BSR_TRY(ix->live_blk.ensure(((size_t)mask_blocks(ix->n) + 1) * sizeof(uint32_t)));
    // (the bitset itself as the mask: the deleted rows ahead of every block of words)
    BSR_HIP(launch_mask_list_count(ix->dead.as<uint64_t>(), nullptr, ix->n, ix->live_blk.as<uint32_t>(), ix->stream));
    BSR_HIP(launch_dead_zero_fop(ix->dead.as<uint64_t>(), ix->n, ix->live_blk.as<uint32_t>(), ix->op_row_bytes,
                                 ix->fop.as<uint8_t>(), ix->fop_s.as<uint8_t>(), ix->rows.as<float>(), ix->dim,
                                 ix->ascale_s.as<float>(), ix->stream));
    BSR_HIP(hipStreamSynchronize(ix->stream));
    return BSR_OK;
}

void bsr_index::clear_tombstones() {
    if (n_dead) ++dead_gen;
    n_dead = 0;
    live_list_ok = false;
    (void)hipStreamSynchronize(stream);
    dead.release();
}

int bsr_index::tombstones_after_append() {
    live_list_ok = false;
    if (!dead.p) return BSR_OK;
    BSR_TRY(dead_reserve(this));  // (the appended rows: live)
    if (n_dead) BSR_TRY(dead_zero_operand(this));
    return BSR_OK;
}

int bsr_index::delete_rows(const uint64_t* ids, uint64_t n_ids, uint64_t* out_deleted) {
    bsr_index* ix = this;
    if (out_deleted) *out_deleted = 0;
    if (!loaded) return set_error(BSR_E_STATE, "index not loaded");
    if (!n_ids) return BSR_OK;
    if (!ids) return set_error(BSR_E_INVALID, "null ids");
    if (n_ids >> 32) return set_error(BSR_E_INVALID, "n_ids=%llu: at most 2^32 - 1 ids per call", (unsigned long long)n_ids);
    BSR_HIP(hipSetDevice(device));
    const uint64_t* dids = nullptr;
    BSR_TRY(on_device(ix, dead_ids, ids, (size_t)n_ids * sizeof(uint64_t), is_device_ptr(ids), &dids));
    BSR_TRY(dead_cnt.ensure(2 * sizeof(uint32_t)));
    BSR_HIP(hipMemsetAsync(dead_cnt.p, 0, 2 * sizeof(uint32_t), stream));
    uint32_t* bad = dead_cnt.as<uint32_t>();
    uint32_t h[2] = {0, 0};
    // all or nothing: the ids are checked first, and nothing is applied when one is out of range
    BSR_HIP(launch_dead_check(dids, n_ids, global_offset, n, bad, stream));
    BSR_HIP(hipMemcpyAsync(h, bad, sizeof h, hipMemcpyDeviceToHost, stream));
    BSR_HIP(hipStreamSynchronize(stream));
    if (h[0])
        return set_error(BSR_E_INVALID, "%u of the ids lie outside [%llu, %llu): no row was deleted", h[0],
                         (unsigned long long)global_offset, (unsigned long long)(global_offset + n));
    BSR_TRY(dead_reserve(ix));
    BSR_HIP(launch_dead_apply(dids, n_ids, global_offset, n, dead.as<uint64_t>(), bad + 1, stream));
    BSR_HIP(hipMemcpyAsync(h, bad, sizeof h, hipMemcpyDeviceToHost, stream));
    BSR_HIP(hipStreamSynchronize(stream));
    if (out_deleted) *out_deleted = h[1];
    if (!h[1]) return BSR_OK;
    n_dead += h[1];
    ++dead_gen;
    live_list_ok = false;
    return dead_zero_operand(ix);
}

int bsr_index::deleted_mask(uint64_t* out_words, uint64_t words) const {
    if (!loaded) return set_error(BSR_E_STATE, "index not loaded");
    if (words != (n + 63) / 64)
        return set_error(BSR_E_INVALID, "words=%llu, the index holds %llu rows (%llu words)", (unsigned long long)words,
                         (unsigned long long)n, (unsigned long long)((n + 63) / 64));
    if (!words) return BSR_OK;
    if (!out_words) return set_error(BSR_E_INVALID, "null output");
    BSR_HIP(hipSetDevice(device));
    const size_t bytes = (size_t)words * sizeof(uint64_t);
    const bool dev = is_device_ptr(out_words);
    if (!n_dead) {
        if (dev) BSR_HIP(hipMemsetAsync(out_words, 0, bytes, stream));
        else memset(out_words, 0, bytes);
    } else {
        BSR_HIP(hipMemcpyAsync(out_words, dead.p, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
    }
    BSR_HIP(hipStreamSynchronize(stream));
    return BSR_OK;
}

// The exact fallback's row list with tombstones present: the live rows, ascending, built by the
// mask list kernels with no allow mask -- every row the bitset does not remove (the count is
// known: no host read) -- cached until the next delete, append or load.
int bsr_index::ensure_live_list() {
    if (live_list_ok) return BSR_OK;
    const uint64_t live = live_rows();
    if (!live) return BSR_OK;
    const uint32_t n_blk = mask_blocks(n);
    BSR_TRY(live_blk.ensure(((size_t)n_blk + 1) * sizeof(uint32_t)));
    BSR_TRY(live_list.ensure((size_t)live * sizeof(uint32_t)));
    BSR_HIP(launch_mask_list_count(nullptr, dead_bits(), n, live_blk.as<uint32_t>(), stream));
    BSR_HIP(launch_mask_list_scatter(nullptr, dead_bits(), n, live_blk.as<uint32_t>(), (uint32_t)live,
                                     live_list.as<uint32_t>(), stream));
    live_list_ok = true;
    return BSR_OK;
}

int bsr_index_delete_impl(bsr_index* ix, const uint64_t* ids, uint64_t n_ids, uint64_t* out_deleted) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    return ix->delete_rows(ids, n_ids, out_deleted);
}
int bsr_index_deleted_mask_impl(const bsr_index* ix, uint64_t* out_words, uint64_t words) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    return ix->deleted_mask(out_words, words);
}

// ---------------------------------------------------------------------------------------
// in-place update (bsr_index_update)
// ---------------------------------------------------------------------------------------
// Rows replaced by global id.  One check launch and one host read decide all or nothing before a
// stored byte changes; then the scatter, the norms of the named rows, and the operand of the
// touched 32-row blocks and sample groups rebuilt by the load's own device functions from
// ascending lists (the list kernels of the masked search over the check's bitsets; their counts
// stay on the device, the grids cover the lists' capacity).  No kernel walks the shard's rows:
// O(n_ids ld + touched blocks 32 ld + n / 64), plus dead_zero_operand's O(n / 64 + n_dead ld) when
// the shard has tombstones -- the requantised blocks would bring a deleted row's operand back.
int bsr_index::update_rows(const uint64_t* ids, const void* new_rows, uint64_t n_ids) {
    bsr_index* ix = this;
    if (!loaded) return set_error(BSR_E_STATE, "index not loaded");
    if (!n_ids) return BSR_OK;
    if (!ids || !new_rows) return set_error(BSR_E_INVALID, "null %s", ids ? "rows" : "ids");
    if (n_ids >> 32) return set_error(BSR_E_INVALID, "n_ids=%llu: at most 2^32 - 1 ids per call", (unsigned long long)n_ids);
    BSR_HIP(hipSetDevice(device));
    const bool bf16 = cfg.dtype == BSR_BF16;
    const bool ids_dev = is_device_ptr(ids), rows_dev = is_device_ptr(new_rows);
    // (device inputs may be in flight on any stream of the caller: the load / append rule)
    if (ids_dev || rows_dev) BSR_HIP(hipDeviceSynchronize());
    const uint64_t* dids = nullptr;
    const void* src = nullptr;
    BSR_TRY(on_device(ix, upd_ids, ids, (size_t)n_ids * sizeof(uint64_t), ids_dev, &dids));
    BSR_TRY(on_device(ix, tmp, new_rows, (size_t)n_ids * dim * (bf16 ? 2 : 4), rows_dev, &src));
    // every buffer is sized before the check, so that nothing can fail between the first stored
    // byte and the last
    const uint64_t nb = (n + kQuantBlock - 1) / kQuantBlock;                                  // 32-row blocks
    const uint64_t ng = sample_rows_pad(n) / kSampleScaleRows;                                // sample groups
    const uint64_t w_rows = n_pad / 64, w_blk = (nb + 63) / 64, w_grp = (ng + 63) / 64;
    const uint32_t cap_b = (uint32_t)std::min<uint64_t>(n_ids, nb), cap_g = (uint32_t)std::min<uint64_t>(n_ids, ng);
    const uint32_t mb_b = mask_blocks(nb), mb_g = mask_blocks(ng);
    BSR_TRY(upd_bits.ensure((size_t)(w_rows + w_blk + w_grp) * sizeof(uint64_t)));
    BSR_TRY(upd_cnt.ensure(kUpdCounts * sizeof(uint64_t)));
    BSR_TRY(upd_blk.ensure(((size_t)mb_b + 1 + mb_g + 1) * sizeof(uint32_t)));
    BSR_TRY(upd_list.ensure(((size_t)cap_b + cap_g) * sizeof(uint32_t)));
    uint64_t* touched = upd_bits.as<uint64_t>();
    uint64_t* blocks = touched + w_rows;
    uint64_t* groups = blocks + w_blk;
    uint32_t* blk_b = upd_blk.as<uint32_t>();
    uint32_t* blk_g = blk_b + mb_b + 1;
    uint32_t* list_b = upd_list.as<uint32_t>();
    uint32_t* list_g = list_b + cap_b;
    BSR_HIP(hipMemsetAsync(upd_bits.p, 0, (size_t)(w_rows + w_blk + w_grp) * sizeof(uint64_t), stream));
    BSR_HIP(hipMemsetAsync(upd_cnt.p, 0, kUpdCounts * sizeof(uint64_t), stream));
    BSR_HIP(launch_upd_check(dids, n_ids, global_offset, n, src, dim, bf16, touched, blocks, groups,
                             upd_cnt.as<uint64_t>(), stream));
    uint64_t h[kUpdCounts] = {0, 0, 0, 0};
    BSR_HIP(hipMemcpyAsync(h, upd_cnt.p, sizeof h, hipMemcpyDeviceToHost, stream));
    BSR_HIP(hipStreamSynchronize(stream));
    if (h[kUpdBadId])
        return set_error(BSR_E_INVALID, "%llu of the ids lie outside [%llu, %llu): no row was updated",
                         (unsigned long long)h[kUpdBadId], (unsigned long long)global_offset,
                         (unsigned long long)(global_offset + n));
    if (h[kUpdDupId])
        return set_error(BSR_E_INVALID, "%llu of the ids name a row a second time: no row was updated",
                         (unsigned long long)h[kUpdDupId]);
    if (h[kUpdNonFinite])
        return set_error(BSR_E_NONFINITE, "%llu NaN/Inf among the incoming values: no row was updated",
                         (unsigned long long)h[kUpdNonFinite]);

    float* slab = rows.as<float>();
    uint32_t* fl = flags.as<uint32_t>();
    BSR_HIP(launch_upd_scatter(dids, n_ids, global_offset, src, dim, ld, bf16, slab, stream));
    BSR_HIP(launch_upd_row_norms(slab, dids, n_ids, global_offset, dim, ld, na.as<float>(), fl, stream));
    BSR_HIP(launch_mask_list_count(blocks, nullptr, nb, blk_b, stream));
    BSR_HIP(launch_mask_list_scatter(blocks, nullptr, nb, blk_b, cap_b, list_b, stream));
    BSR_HIP(launch_upd_rows_to_i8(slab, n, dim, ld, fop.as<int8_t>(), ascale.as<float>(), fl + 1, list_b, blk_b + mb_b,
                                  cap_b, stream));
    if (h[kUpdSampleRows]) {  // (no row the fop_s sample reads: nothing of it changes)
        BSR_HIP(launch_mask_list_count(groups, nullptr, ng, blk_g, stream));
        BSR_HIP(launch_mask_list_scatter(groups, nullptr, ng, blk_g, cap_g, list_g, stream));
        BSR_HIP(launch_upd_rows_to_i8_sample(slab, n, dim, ld, fop_s.as<int8_t>(), ascale_s.as<float>(), list_g,
                                             blk_g + mb_g, cap_g, stream));
    }
    // tombstones stay as they are: the deleted rows' operand is zeroed again (as after an append)
    if (n_dead) BSR_TRY(dead_zero_operand(ix));
    // the flags are sticky (only a load clears them) and ea_max only grows (atomicMax)
    return read_row_state(ix);
}

int bsr_index_update_impl(bsr_index* ix, const uint64_t* ids, const void* rows, uint64_t n_ids) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    return ix->update_rows(ids, rows, n_ids);
}

// ---------------------------------------------------------------------------------------
// compaction (bsr_index_compact)
// ---------------------------------------------------------------------------------------
// The rows one chunk of the in-place move stages: BSR_COMPACT_STAGE_BYTES (read per call), 256 MB
// by default, at least kRowPad rows.
static uint64_t compact_stage_rows(const bsr_index* ix) {
    const uint64_t bytes = env_bytes("BSR_COMPACT_STAGE_BYTES", 256ull << 20);
    return std::max<uint64_t>(bytes / ((size_t)ix->ld * sizeof(float)), kRowPad);
}
static double host_ms() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

// The live rows L[0 .. live) (ascending; ensure_live_list) become rows 0 .. live - 1.  L[j] >= j, so
// rows[j] = rows[L[j]] in one parallel launch would overwrite sources not yet read (row 0 deleted
// alone: every destination is its neighbour's source).  The move therefore runs in chunks of
// destinations [j0, j1), each gathered into the staging buffer and copied back, in stream order:
// a source inside the chunk's destination range is a row j' <= L[j'] < j1 -- staged by this
// chunk or moved by an earlier one -- and everything behind j1 is still untouched.  Rows before the
// first deleted row stay where they are.  A shrink that saves bytes gathers straight into the new,
// smaller slab instead (two buffers: no hazard, no staging).  What the rows imply -- magnitudes,
// operand, scales, sample, error bound, flags -- is rebuilt by index_finish_load: the index is then
// what a load of the live rows leaves, by construction.
int bsr_index::compact_rows(uint64_t new_global_offset, uint32_t fl, uint64_t* out_old_ids, uint64_t out_capacity,
                            uint64_t* out_count) {
    bsr_index* ix = this;
    if (!loaded) return set_error(BSR_E_STATE, "index not loaded");
    if (fl & ~BSR_COMPACT_SHRINK) return set_error(BSR_E_INVALID, "unknown flag bits 0x%x", fl & ~BSR_COMPACT_SHRINK);
    const uint64_t live = live_rows();
    if (out_old_ids && out_capacity < live)
        return set_error(BSR_E_INVALID, "out_capacity=%llu, the index holds %llu live rows: nothing was moved",
                         (unsigned long long)out_capacity, (unsigned long long)live);
    if (new_global_offset > UINT64_MAX - live)
        return set_error(BSR_E_INVALID, "new_global_offset + %llu live rows overflows", (unsigned long long)live);
    BSR_HIP(hipSetDevice(device));
    const double t0 = host_ms();
    const size_t row_bytes = (size_t)ld * sizeof(float);
    const uint64_t old_pad = n_pad, old_off = global_offset;
    const uint64_t new_pad = round_up(std::max<uint64_t>(live, 1), kRowPad);
    const bool trim = (fl & BSR_COMPACT_SHRINK) && new_pad * row_bytes < rows.bytes;  // (a smaller slab saves bytes)
    const bool out_dev = out_old_ids && is_device_ptr(out_old_ids);

    if (!n_dead && !trim) {
        // nothing to drop: the identity map, and the offset -- baked into every captured graph
        // (launch_finalize's and the rescore's argument), so a change makes them stale
        if (out_old_ids && live) {
            if (out_dev) {
                BSR_HIP(launch_compact_ids(nullptr, live, old_off, out_old_ids, nullptr, stream));
                BSR_HIP(hipStreamSynchronize(stream));
            } else {
                for (uint64_t j = 0; j < live; ++j) out_old_ids[j] = old_off + j;
            }
        }
        if (new_global_offset != old_off) {
            global_offset = new_global_offset;
            ++dead_gen;
        }
        if (out_count) *out_count = live;
        return BSR_OK;
    }

    // The list, the id map and the first row that moves; then every buffer the move needs -- all
    // before a stored byte changes (a failure up to here leaves the index as it was).
    const uint32_t* list = nullptr;
    uint64_t* dids = out_dev ? out_old_ids : nullptr;
    uint32_t first32 = ~0u;
    if (live) {
        if (n_dead) {
            BSR_TRY(ensure_live_list());
            list = live_list.as<uint32_t>();
        }
        if (out_old_ids && !out_dev) {
            BSR_TRY(tmp.ensure((size_t)live * sizeof(uint64_t)));
            dids = tmp.as<uint64_t>();
        }
        BSR_TRY(cmp_first.ensure(sizeof(uint32_t)));
        BSR_HIP(hipMemsetAsync(cmp_first.p, 0xff, sizeof(uint32_t), stream));
        BSR_HIP(launch_compact_ids(list, live, old_off, dids, cmp_first.as<uint32_t>(), stream));
        BSR_HIP(hipMemcpyAsync(&first32, cmp_first.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        if (out_old_ids && !out_dev)
            BSR_HIP(hipMemcpyAsync(out_old_ids, tmp.p, (size_t)live * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    }
    BSR_HIP(hipStreamSynchronize(stream));
    const uint64_t first = std::min<uint64_t>(first32, live);  // rows [0, first) stay put
    uint64_t chunk = 0;
    DevBuf small;
    if (trim) {
        BSR_TRY(small.ensure(new_pad * row_bytes));
    } else if (first < live) {
        chunk = std::min<uint64_t>(compact_stage_rows(ix), live - first);
        BSR_TRY(cmp_stage.ensure(chunk * row_bytes));
    }
    const double t1 = host_ms();
    double t2 = t1;

    auto move_and_rebuild = [&]() -> int {
        float* slab = rows.as<float>();
        if (trim) {
            float* dst = small.as<float>();
            if (first) BSR_HIP(hipMemcpyAsync(dst, slab, first * row_bytes, hipMemcpyDeviceToDevice, stream));
            if (first < live) BSR_HIP(launch_compact_gather(slab, list + first, live - first, ld, dst + first * ld, stream));
            if (new_pad > live)
                BSR_HIP(hipMemsetAsync(dst + live * ld, 0, (new_pad - live) * row_bytes, stream));
            BSR_HIP(hipStreamSynchronize(stream));
            std::swap(rows.p, small.p);
            std::swap(rows.bytes, small.bytes);
            small.release();  // (the old slab, before the rebuild allocates)
        } else {
            float* stage = cmp_stage.as<float>();
            for (uint64_t j0 = first; j0 < live; j0 += chunk) {
                const uint64_t cnt = std::min<uint64_t>(chunk, live - j0);
                BSR_HIP(launch_compact_gather(slab, list + j0, cnt, ld, stage, stream));
                BSR_HIP(hipMemcpyAsync(slab + j0 * ld, stage, cnt * row_bytes, hipMemcpyDeviceToDevice, stream));
            }
            // zero padded, over everything the shard held: an append that does not regrow the slab
            // finds clean pad rows
            if (old_pad > live)
                BSR_HIP(hipMemsetAsync(slab + live * ld, 0, (old_pad - live) * row_bytes, stream));
            BSR_HIP(hipStreamSynchronize(stream));
        }
        t2 = host_ms();
        n = live;
        n_pad = new_pad;
        global_offset = new_global_offset;
        clear_tombstones();
        ++dead_gen;  // (the row count, the offset, the bitset: every captured graph is stale)
        if (fl & BSR_COMPACT_SHRINK) {
            // what index_finish_load sizes again, released where it is larger than that
            const uint64_t n_s_pad = sample_rows_pad(n);
            auto drop = [](DevBuf& b, size_t need) { if (b.bytes > std::max<size_t>(need, 16)) b.release(); };
            drop(na, n_pad * sizeof(float));
            drop(fop, (size_t)n_pad * op_row_bytes);
            drop(ascale, n_pad / kQuantBlock * sizeof(float));
            drop(fop_s, (size_t)n_s_pad * op_row_bytes);
            drop(ascale_s, (size_t)(n_s_pad / kSampleScaleRows) * sizeof(float));
            cmp_stage.release();
            live_list.release();
        }
        return index_finish_load(ix);
    };
    const int r = move_and_rebuild();
    if (r != BSR_OK) {
        // rows may be half moved and the derived state does not match them: empty until a load
        loaded = false;
        clear_tombstones();
        return r;
    }
    if (out_count) *out_count = live;
    const char* trace = getenv("BSR_COMPACT_TRACE");  // (tools/bench_compact.py: host clocks around the waits)
    if (trace && trace[0] && trace[0] != '0')
        fprintf(stderr, "bsr_index_compact: live=%llu first=%llu list_ms=%.3f move_ms=%.3f rebuild_ms=%.3f\n",
                (unsigned long long)live, (unsigned long long)first, t1 - t0, t2 - t1, host_ms() - t2);
    return BSR_OK;
}

int bsr_index_compact_impl(bsr_index* ix, uint64_t new_global_offset, uint32_t flags, uint64_t* out_old_ids,
                           uint64_t out_capacity, uint64_t* out_count) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    return ix->compact_rows(new_global_offset, flags, out_old_ids, out_capacity, out_count);
}

// ---------------------------------------------------------------------------------------
// search
// ---------------------------------------------------------------------------------------
// Exact full scan of n_ids queries whose ids are the device list `ids` (groups of kScanQF;
// an id list padded to a multiple of kScanQF with valid ids).
static int run_exact_scan(bsr_index* ix, const int32_t* ids, uint32_t n_ids, uint32_t k) {
    if (!n_ids) return BSR_OK;
    const uint32_t groups = (n_ids + kScanQF - 1) / kScanQF;
    const uint32_t grid = scan_grid_for(ix->n);
    BSR_TRY(ix->part.ensure((size_t)grid * kScanQF * k * sizeof(uint64_t)));
    ev_begin(ix, ix->ev_scan, 1);
    for (uint32_t g = 0; g < groups; ++g) {
        const uint32_t nqf = std::min(kScanQF, n_ids - g * kScanQF);
        const int32_t* qid = ids + (size_t)g * kScanQF;
        BSR_HIP(launch_scan_exact(ix->rows.as<float>(), ix->ld, ix->dim, ix->n, ix->na.as<float>(),
                                  ix->qf32.as<float>(), qid, nqf, ix->nb.as<float>(), k, grid,
                                  ix->part.as<uint64_t>(), ix->stream));
        BSR_HIP(launch_merge_parts(ix->part.as<uint64_t>(), grid, qid, nqf, k, ix->keys.as<uint64_t>(), ix->stream));
    }
    ev_end(ix, ix->ev_scan);
    return BSR_OK;
}

static int run_list_scan(bsr_index* ix, const int32_t* ids, uint32_t n_ids, uint32_t k, const uint32_t* list,
                         uint32_t n_list);
// The exact rounds of a search: the full scan, or -- an index with tombstones -- the list scan over
// its live rows (at least one: a shard without a live row takes the empty-shard branch).
static int run_exact_rounds(bsr_index* ix, const int32_t* ids, uint32_t n_ids, uint32_t k) {
    if (!ix->n_dead) return run_exact_scan(ix, ids, n_ids, k);
    BSR_TRY(ix->ensure_live_list());
    return run_list_scan(ix, ids, n_ids, k, ix->live_list.as<uint32_t>(), (uint32_t)ix->live_rows());
}

// The self-thresholded single-query path (round 6, DESIGN.md §5 tiny batches): batches of <= 16
// queries over shards of >= kSkinnyTopMinRows rows, k' <= 63, rows of <= 16 K slices, with the
// tiny-batch rescore kernel (BSR_SKINNY_TOP=0 turns it off, for A/B runs).  No sample pass and
// no tau0: the skinny filter keeps every wave's 4 best keys per query, the rescore selects the k'
// best of them.  Returns the lists' slots per query (0: the thresholded path).
static uint32_t top_slots(const bsr_index* ix, uint32_t nq, uint32_t k) {
    const char* v = getenv("BSR_SKINNY_TOP");
    if (v && v[0] == '0') return 0;
    if (nq > kSkinnyMaxQ || ix->n < kSkinnyTopMinRows || kp_for(k) > 63 || k > 64 || ix->op_row_bytes > 16 * 64 ||
        ix->ld % 64 != 0 || ix->ld > 1024 || !rescore_kp_enabled())
        return 0;
    const uint32_t slots = 4 * skinny_top_lists((uint32_t)ix->n);
    return slots <= 64u * kTopKeysPerLane ? slots : 0;  // (k_rescore_kp's wave 0 holds the lists)
}

// Buffers of the candidate stage for a batch (k' = kp_for(k) candidates, lists of cap keys).
// (top_slots whatever path the batch takes: the thresholded rerun of a self-thresholded batch finds
// the lists that batch sized.)
static int filter_buffers(bsr_index* ix, uint32_t nq, uint32_t qpad, uint32_t k, uint32_t cap_in = 0) {
    // k' candidates, (k'+1) % 64 == 0, about 3k: the k-th exact score must clear the (k'+1)-th
    // approximate one by E_q, and in a Gaussian-like tail that takes ~3x as many rows at
    // E_q/sigma ~ 0.26.  63 for k <= 10, 191 for k = 50, 383 for k = 100.
    const uint32_t kp = kp_for(k);
    const uint32_t cap = std::max(cap_in ? cap_in : cap_for(k), top_slots(ix, nq, k));
    ix->stats.n_candidates = kp;
    BSR_TRY(ix->tau.ensure((size_t)qpad * sizeof(float)));
    BSR_TRY(ix->cand.ensure((size_t)qpad * cap * sizeof(uint64_t)));
    BSR_TRY(ix->cnt.ensure(((size_t)qpad + 8 * kTailCounters + kGangWords) * sizeof(uint32_t)));  // + tail, gangs
    BSR_TRY(ix->cand_rows.ensure((size_t)nq * kp * sizeof(uint32_t)));
    BSR_TRY(ix->ncand.ensure((size_t)nq * sizeof(uint32_t)));
    BSR_TRY(ix->tau_excl.ensure((size_t)nq * sizeof(float)));
    BSR_TRY(ix->fail.ensure((size_t)nq * sizeof(uint32_t)));
    BSR_TRY(ix->fail2.ensure((size_t)nq * sizeof(uint32_t)));
    return BSR_OK;
}

static GemmArgs gemm_args(bsr_index* ix, uint32_t qpad) {
    GemmArgs g{};
    g.A = ix->fop.as<uint8_t>();
    g.B = ix->qop.as<uint8_t>();
    g.row_bytes = ix->op_row_bytes;
    g.n_qt = qpad / kFilterTile;
    g.a_scale = ix->ascale.as<float>();
    g.b_scale = ix->qscale.as<float>();
    return g;
}
// ... of a pass over every row of the shard that emits into the candidate lists (emit_pass, top_pass)
static GemmArgs emit_args(bsr_index* ix, uint32_t nq, uint32_t qpad) {
    GemmArgs g = gemm_args(ix, qpad);
    g.a_stride = ix->op_row_bytes;
    g.a_scale_rows = kQuantBlock;
    g.n_rows = (uint32_t)ix->n;
    g.n_rt = (uint32_t)((ix->n + kFilterTile - 1) / kFilterTile);
    g.cand = ix->cand.as<uint64_t>();
    g.cnt = ix->cnt.as<uint32_t>();
    g.n_q = nq;
    return g;
}

// The sample of a batch (n > cap): every 32nd row (fop_s) scored one by one or -- compact, large
// shards -- as maxima over 32 sampled rows; or, for the batched query-stationary filter in
// compact mode, whole tiles of fop scored once (tiles != 0, GemmArgs::s_tiles): one 128-row
// tile in 32, four values per tile, the same number of values per query as the compact sample.
struct SampleLayout {
    uint32_t n_s, n_rt_s;  // the fop_s sample: rows, 256-row tiles
    bool compact;
    uint32_t tiles;        // sample tiles of fop (0: the fop_s sample)
    uint32_t s_ld, n_vals; // S: row length, valid values per query
};
// BSR_SAMPLE_TILES=0 (read per search, an A/B switch): the fop_s sample for every batch.  No shard
// size limit: from 1M rows (no difference) to 10M (-2.4% per step) the sample tiles were never
// slower than the fop_s sample at 1000 queries.
static bool sample_tiles_on() {
    const char* v = getenv("BSR_SAMPLE_TILES");
    return !(v && v[0] == '0');
}
static SampleLayout sample_layout(const bsr_index* ix, uint32_t nq, uint32_t ks) {
    SampleLayout L{};
    const uint32_t BM = kFilterTile;
    L.n_s = (uint32_t)((ix->n + kSampleStride - 1) / kSampleStride);
    L.n_rt_s = (L.n_s + BM - 1) / BM;
    L.compact = L.n_s >= 32u * 8u * ks;
    const uint32_t nk = ix->op_row_bytes / 64;
    const bool qs16 = ix->op_row_bytes % 64 == 0 && nk % 2 == 0 && nk >= 2 && nk <= 12;
    if (L.compact && nq > kSkinnyMaxQ && qs16 && sample_tiles_on()) L.tiles = sample_tiles_for(ix->n);
    if (L.tiles) {
        // (the last sample tile may be the shard's partial last tile: its blocks with a valid row)
        const uint64_t last0 = ((uint64_t)(L.tiles - 1) * kSampleTileEvery + kSampleTilePhase) * 128;
        const uint64_t valid = std::min<uint64_t>(128, ix->n - last0);
        L.s_ld = 4 * L.tiles;
        L.n_vals = 4 * (L.tiles - 1) + (uint32_t)((valid + kQuantBlock - 1) / kQuantBlock);
    } else {
        L.s_ld = L.compact ? L.n_rt_s * (BM / 32) : L.n_rt_s * BM;
        L.n_vals = L.compact ? (L.n_s + 31) / 32 : L.n_s;
    }
    return L;
}

// Steps 2-3 of the candidate stage: the sample pass and tau0 (smax: also the ks best sample
// keys per query, the input of a parallel search's global threshold), then the emit pass.
// Batches of at most 16 queries use the skinny (HBM-bound, no LDS) filter kernels.
// ks / cap (0: ks_for(k) / cap_for(k)): the masked search's lowered threshold and longer lists.
// ks_q (optional, device [qpad]): the grouped masked search's per-query depths (ks_in their maximum).
static int sample_pass(bsr_index* ix, uint32_t nq, uint32_t qpad, uint32_t k, uint64_t* smax, uint32_t ks_in = 0,
                       uint32_t cap_in = 0, const uint32_t* ks_q = nullptr) {
    BSR_TRY(filter_buffers(ix, nq, qpad, k, cap_in));
    ix->smp_tiles = 0;
    const bool skinny = nq <= kSkinnyMaxQ;
    const uint32_t cap = cap_in ? cap_in : cap_for(k);
    // (k'+1)/8: about 8 x 32 = 256 rows reach tau0 for k <= 10.  Fewer (ks = (k'+1)/12, /16)
    // measured 1-2% less filter time and up to 1.3% of the queries falling back to the exact
    // scan (profiles/r02f_*): not worth it.
    const uint32_t ks = ks_in ? ks_in : ks_for(k);
    const uint64_t n = ix->n;
    GemmArgs g = gemm_args(ix, qpad);
    uint32_t* status = ix->d_status;
    if (n > cap) {
        // tau0 from every 32nd row: the ks-th best sampled score, or (large shards) the
        // ks-th best maximum over 32 sampled rows -- never above the former, so at least
        // ~ks*32 rows of the shard reach it.
        const SampleLayout L = sample_layout(ix, nq, ks);
        const uint32_t s_ld = L.s_ld, n_vals = L.n_vals;
        BSR_TRY(ix->S.ensure((size_t)qpad * s_ld * sizeof(float)));
        g.a_stride = ix->op_row_bytes;
        if (L.tiles) {
            // sample tiles of fop, the emit pass's scales (gemm_args): scored here and nowhere else
            g.a_scale_rows = kQuantBlock;
            g.n_rows = (uint32_t)n;
            g.n_rt = L.tiles;
            g.s_tiles = L.tiles;
            g.s_vals = n_vals;
            ix->smp_tiles = L.tiles;
            ix->smp_ld = s_ld;
            ix->smp_vals = n_vals;
        } else {
            g.A = ix->fop_s.as<uint8_t>();  // the sampled rows, contiguous
            g.a_scale = ix->ascale_s.as<float>();
            g.a_scale_rows = kSampleScaleRows;
            g.n_rows = L.n_s;
            g.n_rt = L.n_rt_s;
        }
        g.S = ix->S.as<float>();
        g.s_ld = s_ld;
        g.s_compact = L.compact ? 1u : 0u;
        BSR_HIP(launch_timed(ix, ix->ev_sample, [&] {
            return skinny ? launch_filter_skinny_sample(g, ix->stream) : launch_filter_sample(g, ix->stream);
        }, 2));
        BSR_HIP(launch_select_tau(ix->S.as<float>(), s_ld, n_vals, nq, qpad, ix->qflags.as<uint32_t>(), ks,
                                  ix->tau.as<float>(), ix->cnt.as<uint32_t>(), status, ix->stream, smax, ks_q));
    } else {
        BSR_HIP(launch_select_tau(nullptr, 0, 0, nq, qpad, ix->qflags.as<uint32_t>(), ks, ix->tau.as<float>(),
                                  ix->cnt.as<uint32_t>(), status, ix->stream, smax, ks_q));
    }
    return BSR_OK;
}

static int emit_pass(bsr_index* ix, uint32_t nq, uint32_t qpad, uint32_t k, uint32_t cap_in = 0) {
    const bool skinny = nq <= kSkinnyMaxQ;
    GemmArgs g = emit_args(ix, nq, qpad);
    g.tau = ix->tau.as<float>();
    g.cap = cap_in ? cap_in : cap_for(k);
    // the last 1/kTailDiv of the row tiles are balanced dynamically (k_filter_qs16)
    g.tail = g.n_qt <= kTailCounters ? ix->cnt.as<uint32_t>() + qpad : nullptr;
    // sample tiles (this batch's sample pass scored them): the emit filter skips them and the
    // fix-up emits their rows from S and the final threshold (one more kernel in the stream)
    g.s_tiles = skinny ? 0u : ix->smp_tiles;
    g.S = ix->S.as<float>();
    g.s_ld = ix->smp_ld;
    g.s_vals = ix->smp_vals;
    BSR_HIP(launch_timed(ix, ix->ev_emit, [&] {
        hipError_t r = skinny ? launch_filter_skinny_emit(g, ix->stream) : launch_filter_emit(g, ix->stream);
        if (r == hipSuccess && g.s_tiles) r = launch_sample_fixup(g, ix->stream);
        return r;
    }));
    return BSR_OK;
}

// the skinny TOP row layout: 2, the strided pairs (BSR_TOP_LAYOUT=0: contiguous units, lab A/B only)
static uint32_t top_layout_lab() {
    const char* lay = getenv("BSR_TOP_LAYOUT");
    return lay && lay[0] == '0' ? 0u : 2u;
}

// The self-thresholded filter pass: every wave's 4 best keys per query (launch_filter_skinny_top).
static int top_pass(bsr_index* ix, uint32_t nq, uint32_t qpad, uint32_t k, uint32_t top) {
    BSR_TRY(filter_buffers(ix, nq, qpad, k));
    GemmArgs g = emit_args(ix, nq, qpad);
    g.cap = top;
    g.status = ix->d_status;
    g.top_layout = top_layout_lab();
    BSR_HIP(launch_timed(ix, ix->ev_emit, [&] { return launch_filter_skinny_top(g, ix->stream); }));
    return BSR_OK;
}

// What every rescore launch of a batch takes from the index: the exact operands, one item per
// query, the k' / k of the batch, and the result rows of res[cur] (the rescore kernels write them
// themselves: no k_finalize launch) counted against the shard's live rows.
static RescoreArgs rescore_args(const bsr_index* ix, uint32_t nq, uint32_t k) {
    RescoreArgs r{};
    r.rows = ix->rows.as<float>();
    r.ld = ix->ld;
    r.dim = ix->dim;
    r.na = ix->na.as<float>();
    r.qf32 = ix->qf32.as<float>();
    r.nb = ix->nb.as<float>();
    r.n_items = nq;
    r.kp = kp_for(k);
    r.k = k;
    r.ebound = ix->ebound.as<float>();
    r.out_keys = ix->keys.as<uint64_t>();
    r.res_idx = ix->d_idx;
    r.res_dist = ix->d_dist;
    r.res_cnt = ix->d_cnt;
    r.offset = ix->global_offset;
    r.n_rows = ix->live_rows();
    r.dead = ix->dead_bits();  // (nullptr without a deleted row: the kernels as they always ran)
    return r;
}
// ... over the emitted lists of cap keys (mode B; with sel, the lists mode S selects from)
static void rescore_emitted(RescoreArgs& r, const bsr_index* ix, uint32_t cap) {
    r.cand_keys = ix->cand.as<uint64_t>();
    r.cnt = ix->cnt.as<uint32_t>();
    r.cap = cap;
    r.tau0 = ix->tau.as<float>();
}
// ... as the batch's last kernel: it zeroes the NEXT search's status words and sums the emitted
// counts (emit_cnt) into this search's
static void rescore_bookkeeping(RescoreArgs& r, const bsr_index* ix, uint32_t nq, const uint32_t* emit_cnt) {
    r.next_status = ix->res[ix->cur ^ 1u].as<uint32_t>();
    r.emit_cnt = emit_cnt;
    r.cur_status = ix->d_status;
    r.n_queries = nq;
}
// ... of a published search: the result rows also go straight to the host mirror, and the last
// kernel copies the status words there and raises the flag
static void rescore_mirror(RescoreArgs& r, const bsr_index* ix) {
    r.hres_idx = reinterpret_cast<uint64_t*>(ix->h_res_dev + ix->res_off_idx);
    r.hres_dist = reinterpret_cast<float*>(ix->h_res_dev + ix->res_off_dist);
    r.hres_cnt = reinterpret_cast<uint32_t*>(ix->h_res_dev + ix->res_off_cnt);
}
static void rescore_publish(RescoreArgs& r, const bsr_index* ix) {
    r.pub_src = ix->res[ix->cur].as<uint8_t>();
    r.pub_dst = ix->h_res_dev;
    r.pub_bytes = kStWords * sizeof(uint32_t);  // (the rows: written through by both passes)
    r.pub_flag = ix->h_flag_dev;
    r.pub_ticket = ix->pub_ticket.as<uint32_t>();
}

// Candidate stage (steps 2-5) for every query of the batch.  top: the slots per query of the
// self-thresholded path (top_slots), 0 on the thresholded path.
static int run_filter(bsr_index* ix, uint32_t nq, uint32_t qpad, uint32_t k, uint32_t top, bool publish) {
    if (top) {
        BSR_TRY(top_pass(ix, nq, qpad, k, top));
    } else {
        BSR_TRY(sample_pass(ix, nq, qpad, k, nullptr));
        BSR_TRY(emit_pass(ix, nq, qpad, k));
    }
    const uint32_t cap = top ? top : cap_for(k);
    uint32_t* status = ix->d_status;
    // lists of <= 1024 keys (k <= 10): the rescore kernel selects its own k' candidates (the
    // self-thresholded path: always, every wave of the tiny-batch kernel taking part)
    const bool fused_select = top || cap <= kFusedSelectCap;
    if (!fused_select) {
        ev_begin(ix, ix->ev_select);
        BSR_HIP(launch_select_cand(ix->cand.as<uint64_t>(), ix->cnt.as<uint32_t>(), cap, nq, ix->tau.as<float>(),
                                   kp_for(k), ix->cand_rows.as<uint32_t>(), ix->ncand.as<uint32_t>(),
                                   ix->tau_excl.as<float>(), ix->stream));
        ev_end(ix, ix->ev_select);
    }
    ev_begin(ix, ix->ev_rescore);
    // the first pass: the k' selected candidates (mode A), or selected here (mode S)
    RescoreArgs ra = rescore_args(ix, nq, k);
    ra.cand_rows = ix->cand_rows.as<uint32_t>();
    ra.ncand = ix->ncand.as<uint32_t>();
    ra.tau_excl = ix->tau_excl.as<float>();
    ra.fail_cnt = status + kStFail;
    ra.fail_list = ix->fail.as<uint32_t>();
    if (publish) rescore_mirror(ra, ix);
    if (fused_select) {
        ra.sel = 1;
        rescore_emitted(ra, ix, cap);
    }
    if (top) {
        ra.top_w = top / 4;  // (lists: one per workgroup of the skinny filter)
        ra.qflags = ix->qflags.as<uint32_t>();
        ra.top_tau = ix->tau.as<float>();  // (the second chance's tau0)
        ra.top_cnt = ix->cnt.as<uint32_t>();
    }
    BSR_HIP(launch_rescore(ra, ix->stream));
    // Second chance, in the same stream (and graph): a query that failed certification is
    // rescored over EVERY row it emitted (~4k'), certified against tau0 -- far less than a
    // scan.  The failed count is read on the device, so no host round trip; what fails here
    // too goes to fail2 (exact scan, host-driven).
    RescoreArgs rb = ra;
    rb.sel = 0;
    rb.top_w = 0;
    rb.n_items_dev = status + kStFail;
    rb.qlist = ix->fail.as<uint32_t>();
    rb.cand_rows = nullptr;
    rb.ncand = nullptr;
    rb.tau_excl = nullptr;
    rescore_emitted(rb, ix, cap);
    rb.fail_cnt = status + kStFail2;
    rb.fail_list = ix->fail2.as<uint32_t>();
    rescore_bookkeeping(rb, ix, nq, ix->cnt.as<uint32_t>());
    if (publish) rescore_publish(rb, ix);  // (the batch's last kernel)
    BSR_HIP(launch_rescore(rb, ix->stream));
    ev_end(ix, ix->ev_rescore);
    return BSR_OK;
}

// The packed result buffer of a batch (status words | counts | distances | indices | the
// global-threshold search's exclusion bounds), double-buffered; d_* point into res[cur].
int bsr_index::prepare_result(uint32_t nq, uint32_t k) {
    const size_t nqk = (size_t)std::max(nq, 1u) * k;
    res_off_cnt = 16;
    res_off_dist = round_up(res_off_cnt + (size_t)std::max(nq, 1u) * sizeof(uint32_t), 16);
    res_off_idx = round_up(res_off_dist + nqk * sizeof(float), 16);
    res_off_x = round_up(res_off_idx + nqk * sizeof(uint64_t), 16);
    res_bytes = round_up(res_off_x + (size_t)std::max(nq, 1u) * sizeof(float), 16);
    if (res[0].bytes < res_bytes || res[1].bytes < res_bytes) {
        for (DevBuf& r : res) {
            BSR_TRY(r.ensure(res_bytes));
            BSR_HIP(hipMemsetAsync(r.p, 0, r.bytes, stream));  // status words start at zero
        }
        next_status_clean = true;
    }
    if (h_res_bytes < res_bytes) {
        if (h_res) BSR_HIP(hipHostFree(h_res));
        h_res = nullptr;
        h_res_bytes = 0;
        // fine-grained: the rescore kernels write the result rows into it and the publishing
        // kernel the status words, and the host reads it while the stream may still be
        // finishing (the flag, not the completion signal, says the bytes are there)
        BSR_HIP(hipHostMalloc((void**)&h_res, res_bytes, hipHostMallocCoherent));
        BSR_HIP(hipHostGetDevicePointer((void**)&h_res_dev, h_res, 0));
        h_res_bytes = res_bytes;
        ++g_alloc_gen;
    }
    if (!h_flag) {
        BSR_HIP(hipHostMalloc((void**)&h_flag, 64, hipHostMallocCoherent));
        BSR_HIP(hipHostGetDevicePointer((void**)&h_flag_dev, h_flag, 0));
        *h_flag = 0;
        BSR_TRY(pub_ticket.ensure(kTicketWords * sizeof(uint32_t)));
        BSR_HIP(hipMemsetAsync(pub_ticket.p, 0, kTicketWords * sizeof(uint32_t), stream));
        ++g_alloc_gen;
    }
    cur ^= 1u;
    uint8_t* rb = res[cur].as<uint8_t>();
    d_status = reinterpret_cast<uint32_t*>(rb);
    d_cnt = reinterpret_cast<uint32_t*>(rb + res_off_cnt);
    d_dist = reinterpret_cast<float*>(rb + res_off_dist);
    d_idx = reinterpret_cast<uint64_t*>(rb + res_off_idx);
    d_x = reinterpret_cast<float*>(rb + res_off_x);
    if (!next_status_clean) BSR_HIP(hipMemsetAsync(d_status, 0, kStWords * sizeof(uint32_t), stream));
    next_status_clean = false;
    return BSR_OK;
}

// ---- the query stage (step 1), shared by the plain, masked and global-threshold searches ----
// Queries padded to the filter's 256-query tile; batches of <= 16 (the skinny kernels read query
// rows 0..15 only) to 16, so that the per-query kernels launch 16 workgroups, not 256.  (The
// global-threshold search, batches of more than 16 only, always takes the rounded value.)
static uint32_t qpad_for(uint32_t nq) {
    return nq <= kSkinnyMaxQ ? kSkinnyMaxQ : (uint32_t)round_up(nq, kFilterTile);
}
// Its scratch, and the batch's result keys.
static int query_buffers(bsr_index* ix, uint32_t nq, uint32_t qpad, uint32_t k) {
    BSR_TRY(ix->qf32.ensure((size_t)qpad * ix->ld * sizeof(float)));
    BSR_TRY(ix->nb.ensure((size_t)qpad * sizeof(float)));
    BSR_TRY(ix->qop.ensure((size_t)qpad * ix->op_row_bytes));
    BSR_TRY(ix->qscale.ensure((size_t)qpad * sizeof(float)));
    BSR_TRY(ix->ebound.ensure((size_t)qpad * sizeof(float)));
    BSR_TRY(ix->qflags.ensure((size_t)qpad * sizeof(uint32_t)));
    BSR_TRY(ix->qids_id.ensure((size_t)qpad * sizeof(int32_t)));
    BSR_TRY(ix->keys.ensure((size_t)nq * k * sizeof(uint64_t)));
    return BSR_OK;
}
// Its launch arguments over those buffers (qsrc: the queries on the device, stage_queries).
static QueryPrepArgs query_prep_args(const bsr_index* ix, const float* qsrc, uint32_t nq, uint32_t qpad, bool with_op) {
    QueryPrepArgs qa{};
    qa.q = qsrc;
    qa.nq = nq;
    qa.qpad = qpad;
    qa.dim = ix->dim;
    qa.ld = ix->ld;
    qa.ea_max = ix->flags.as<uint32_t>() + 1;
    qa.qf32 = ix->qf32.as<float>();
    qa.nb = ix->nb.as<float>();
    qa.qop = ix->qop.p;
    qa.qscale = ix->qscale.as<float>();
    qa.ebound = ix->ebound.as<float>();
    qa.qflags = ix->qflags.as<uint32_t>();
    qa.qids = ix->qids_id.as<int32_t>();
    qa.status = ix->d_status;
    qa.with_op = with_op;
    return qa;
}
// The queries on the device: device queries where they are, host queries copied into q_in (sized
// here unless it already is: gtau_prepare sizes it ahead of phase A, which allocates nothing).
static int stage_queries(bsr_index* ix, const float* queries, uint32_t nq, const float** qsrc) {
    return on_device(ix, ix->q_in, queries, (size_t)nq * ix->dim * sizeof(float), is_device_ptr(queries), qsrc);
}

// ---- after the status readback -----------------------------------------------------------
// A batch with a NaN/Inf query is an error that names the first such query.
static int check_queries(bsr_index* ix, uint32_t nq) {
    const uint32_t* st = reinterpret_cast<const uint32_t*>(ix->h_res);
    if (!(st[kStQueryFlags] & kQueryNonFinite)) return BSR_OK;
    ix->h_qflags.resize(nq);
    BSR_HIP(hipMemcpy(ix->h_qflags.data(), ix->qflags.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint32_t bad = 0;
    while (bad < nq && !(ix->h_qflags[bad] & kQueryNonFinite)) ++bad;
    return set_error(BSR_E_NONFINITE, "query %u contains NaN/Inf (the reference panics)", bad);
}
// The nfail queries of fail2 -- uncertified, or not served by the filter (zero/tiny/huge |b|) --
// and every query's flags, read into h_fail and h_qflags.
static int read_failed(bsr_index* ix, uint32_t nq, uint32_t nfail) {
    ix->h_fail.resize(nfail);
    ix->h_qflags.resize(nq);
    BSR_HIP(hipMemcpyAsync(ix->h_fail.data(), ix->fail2.p, (size_t)nfail * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           ix->stream));
    BSR_HIP(hipMemcpyAsync(ix->h_qflags.data(), ix->qflags.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           ix->stream));
    BSR_HIP(hipStreamSynchronize(ix->stream));
    return BSR_OK;
}
// The first n ids of h_fail as the exact scans take them: rounds of `per` <= kScanQF queries, every
// round padded to kScanQF ids with its first id.
static std::vector<int32_t> padded_scan_ids(const std::vector<uint32_t>& h_fail, uint32_t n, uint32_t per = kScanQF) {
    const uint32_t rounds = (n + per - 1) / per;
    std::vector<int32_t> padded((size_t)rounds * kScanQF);
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t nr = std::min(per, n - r * per);
        for (uint32_t i = 0; i < kScanQF; ++i)
            padded[(size_t)r * kScanQF + i] = (int32_t)h_fail[(size_t)r * per + (i < nr ? i : 0)];
    }
    return padded;
}
// ... as the exact scans' input: their ids in ascending order, counted into stats (direct: the filter
// cannot serve the query; fallback: it was left uncertified), in qids (device) in groups of kScanQF,
// the last group padded with its first id.  rerun (optional): set, with nothing counted or
// uploaded, when a query the filter serves is among them.
static int failed_queries(bsr_index* ix, uint32_t nq, uint32_t nfail, bool* rerun = nullptr) {
    BSR_TRY(read_failed(ix, nq, nfail));
    std::vector<uint32_t>& h_fail = ix->h_fail;
    if (rerun) {
        for (uint32_t q : h_fail) *rerun |= !(ix->h_qflags[q] & kQueryNoApprox);
        if (*rerun) return BSR_OK;
    }
    std::sort(h_fail.begin(), h_fail.end());
    for (uint32_t q : h_fail) {
        if (ix->h_qflags[q] & kQueryNoApprox) ++ix->stats.n_exact_direct;
        else ++ix->stats.n_fallback;
    }
    const std::vector<int32_t> padded = padded_scan_ids(h_fail, nfail);
    BSR_TRY(ix->qids.ensure(padded.size() * sizeof(int32_t)));
    BSR_HIP(hipMemcpyAsync(ix->qids.p, padded.data(), padded.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                           ix->stream));
    return BSR_OK;
}
// A later round (the exact scans of the failed queries) finalizes every query's keys again,
// counted against n_rows, and reads the result back.  poll: the masked search's form -- its total
// ends here and the host polls the stream; otherwise a blocking wait.
// rows_q (optional, device [nq]): per-query row counts instead of n_rows (the grouped masked search).
static int finalize_and_read(bsr_index* ix, uint32_t nq, uint32_t k, uint64_t n_rows, bool poll,
                             const uint32_t* rows_q = nullptr) {
    BSR_HIP(launch_finalize(ix->keys.as<uint64_t>(), nq, k, n_rows, ix->global_offset, ix->d_idx, ix->d_dist,
                            ix->d_cnt, ix->res[ix->cur ^ 1u].as<uint32_t>(), nullptr, ix->d_status, ix->stream,
                            rows_q));
    ix->next_status_clean = true;
    if (poll) ev_end(ix, ix->ev_total);
    BSR_HIP(hipMemcpyAsync(ix->h_res, ix->res[ix->cur].p, ix->res_bytes, hipMemcpyDeviceToHost, ix->stream));
    BSR_HIP(poll ? stream_wait(ix->stream) : hipStreamSynchronize(ix->stream));
    return BSR_OK;
}

// ---- the opening of a batch, shared by every search entry point ---------------------------------
// The checks every search makes first ...
static int check_batch(const bsr_index* ix, uint32_t k) {
    if (!ix->loaded) return set_error(BSR_E_STATE, "index not loaded");
    if (k == 0 || k > ix->cfg.max_k) return set_error(BSR_E_INVALID, "k=%u outside [1, max_k=%u]", k, ix->cfg.max_k);
    return BSR_OK;
}
// ... and, after the caller's own argument checks: the device, the batch's statistics (path: the
// search_path bits known from the start) and its result buffer.
static int begin_batch(bsr_index* ix, uint32_t nq, uint32_t k, uint32_t path = 0) {
    BSR_HIP(hipSetDevice(ix->device));
    ix->stats = bsr_search_stats{};
    ix->stats.n_queries = nq;
    ix->stats.filter_op = 0;  // int8
    ix->stats.row_ebound = ix->row_ebound;
    ix->stats.search_path = path;
    return ix->prepare_result(nq, k);
}

// force_threshold: the thresholded path whatever top_slots says, launched directly (the rerun of a
// batch the self-thresholded path left uncertified, below).
int bsr_index::search_device(const float* queries, uint32_t nq, uint32_t k, int (*after_launch)(void*), void* ctx,
                             bool force_threshold) {
    bsr_index* ix = this;
    BSR_TRY(check_batch(ix, k));
    BSR_TRY(begin_batch(ix, nq, k));
    if (nq == 0) return BSR_OK;
    if (!queries) return set_error(BSR_E_INVALID, "null queries");

    const uint32_t qpad = qpad_for(nq);
    BSR_TRY(query_buffers(ix, nq, qpad, k));
    ev_begin(ix, ev_total);
    const float* qsrc = nullptr;
    BSR_TRY(stage_queries(ix, queries, nq, &qsrc));
    // (the status words of res[cur] were zeroed by the previous search's finalize)
    // every batch is filtered (batches of <= 16 queries by the skinny kernels)
    // Tombstones: results are counted against the live rows; a shard whose live rows
    // would all fit one query's candidate list (live <= cap_for(k)) goes straight to the list scan
    // over them: that reads fewer rows than the filter would rescore, while the filter would still
    // stream the whole shard, and with live / 32 < 4 ks sampled live rows tau0 is no order
    // statistic worth the name (a shard of n <= cap rows has no sample pass for the same reason).
    const uint64_t live = live_rows();
    const bool use_filter = live > 0 && approx_ok && k <= kMaxKForFilter && (!n_dead || live > cap_for(k));
    const QueryPrepArgs qa = query_prep_args(ix, qsrc, nq, qpad, use_filter);
    const uint32_t top = use_filter && !force_threshold ? top_slots(ix, nq, k) : 0u;
    if (top) stats.search_path |= BSR_PATH_SKINNY_TOP;
    // The filtered path publishes its result: the rescore kernels write every result row into
    // the pinned host mirror as well, and the last kernel copies the status words there and
    // raises a host flag, which the host polls -- no D2H copy node, no wait for the stream's
    // completion signal.  Profile level 2 (every stage evented) keeps the D2H
    // copy and the stream wait.
    const bool publish = use_filter && (!profiling(ix) || prof_level <= 1);
    // prep -> local search -> finalize -> one D2H copy of the packed result (graph-capturable:
    // no allocation and no host synchronisation once the buffers are sized)
    auto enqueue_search = [&]() -> int {
        BSR_HIP(launch_query_prep(qa, stream));
        if (use_filter) {
            // (the rescore kernels write the result rows and the status bookkeeping)
            BSR_TRY(run_filter(ix, nq, qpad, k, top, publish));
        } else {
            if (live == 0) {
                // Empty shard (e.g. a rank whose interval_by_rank block is empty), or one whose
                // every row is deleted: no results.
                BSR_HIP(hipMemsetAsync(keys.p, 0xff, (size_t)nq * k * sizeof(uint64_t), stream));
            } else {
                stats.n_exact_direct = nq;
                BSR_TRY(run_exact_rounds(ix, qids_id.as<int32_t>(), nq, k));
            }
            BSR_HIP(launch_finalize(keys.as<uint64_t>(), nq, k, live, global_offset, d_idx, d_dist, d_cnt,
                                    res[cur ^ 1u].as<uint32_t>(), nullptr, d_status, stream));
        }
        ev_end(ix, ev_total);
        if (!publish) BSR_HIP(hipMemcpyAsync(h_res, res[cur].p, res_bytes, hipMemcpyDeviceToHost, stream));
        return BSR_OK;
    };
    if (publish) __atomic_store_n(h_flag, 0u, __ATOMIC_RELEASE);  // (before any launch of this search)

    // Every filtered batch is graph-capturable; a timed search (profile level >= 1) launches
    // directly, its events recorded on the stream (launch_timed), and so does a rerun.
    const bool graphable = use_filter && (!profiling(ix) || prof_level == 0) && !force_threshold;
    // (the key, after every buffer outside enqueue_search is sized; the switches are read per search)
    SearchKey key;
    key.nq = nq;
    key.k = k;
    key.qsrc = qsrc;
    key.n = n;
    key.gen = g_alloc_gen;
    key.dead_gen = dead_gen;  // (a delete since the capture: its live count and bitset pointer are stale)
    key.top = top != 0;
    key.top_layout = top ? top_layout_lab() : 2u;
    key.skinny_glds = skinny_glds_on();
    key.sample_tiles = sample_tiles_on();
    SearchGraph& gs = graphs[cur];
    if (graphable && gs.exec && gs.key == key) {
        BSR_HIP(hipGraphLaunch(gs.exec, stream));
        stats.n_candidates = kp_for(k);
        ++graph_replays;
        stats.graph_replay = 1;
    } else if (graphable && warm == key) {
        // capture (every buffer already sized by the direct search of this shape), then replay
        if (gs.exec) { (void)hipGraphExecDestroy(gs.exec); gs.exec = nullptr; }
        BSR_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        capturing = true;
        const int rc = enqueue_search();
        capturing = false;
        hipGraph_t graph = nullptr;
        const hipError_t ec = hipStreamEndCapture(stream, &graph);
        if (rc != BSR_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (ec != hipSuccess || g_alloc_gen != key.gen) {  // (an allocation inside the capture)
            if (graph) (void)hipGraphDestroy(graph);
            return set_error(BSR_E_HIP, "search graph capture failed: %s", hipGetErrorString(ec));
        }
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ei != hipSuccess) return set_error(BSR_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ei));
        gs = SearchGraph{exec, key};
        BSR_HIP(hipGraphLaunch(gs.exec, stream));
        ++graph_replays;
        stats.graph_replay = 1;
    } else {
        BSR_TRY(enqueue_search());
        if (graphable) {
            warm = key;
            warm.gen = g_alloc_gen;  // (the direct search sized the candidate stage's buffers)
        }
    }
    next_status_clean = true;
    int hook_st = BSR_OK;
    if (after_launch) hook_st = after_launch(ctx);
    if (publish) {
        const hipError_t r = flag_wait(h_flag, stream);
        if (r == hipErrorUnknown) return set_error(BSR_E_HIP, "the search's stream finished without publishing its result");
        BSR_HIP(r);
    } else {
        BSR_HIP(stream_wait(stream));
    }
    if (hook_st != BSR_OK) return hook_st;
    BSR_TRY(check_queries(ix, nq));
    if (!use_filter) return BSR_OK;
    const uint32_t* st = reinterpret_cast<const uint32_t*>(h_res);
    stats.n_emitted = st[kStEmitted];
    // st[kStFail] queries failed the first certification and were rescored over every
    // emitted row in the same launch sequence; st[kStFail2] of them failed again.
    const uint32_t nfail = st[kStFail2];
    stats.n_rescued = st[kStFail] - nfail;
    if (!nfail) return BSR_OK;
    bool rerun = false;
    BSR_TRY(failed_queries(ix, nq, nfail, top ? &rerun : nullptr));
    if (rerun) {
        // The self-thresholded path left a query it serves uncertified (more than a wave's 4
        // best of its rows lie near the top: a cluster of near-duplicates): the batch again
        // on the thresholded path, directly launched, whose own failures take the exact scan.
        const int r = search_device(queries, nq, k, nullptr, nullptr, true);
        stats.search_path |= BSR_PATH_SKINNY_TOP | BSR_PATH_TOP_RERUN;
        return r;
    }
    // Uncertified queries, and queries the filter cannot serve, take the exact full scan: the
    // reference's arithmetic on every row.  Later rounds finalize and read back again, directly.
    // (with tombstones: the list scan over the live rows)
    BSR_TRY(run_exact_rounds(ix, qids.as<int32_t>(), nfail, k));
    return finalize_and_read(ix, nq, k, live, false);
}

// ---------------------------------------------------------------------------------------
// Masked search (bsr_local_top_k_masked)
// ---------------------------------------------------------------------------------------
// Exact top-k over the allowed-row list for n_ids queries (device id list, padded to a multiple
// of kScanQF with valid ids): the full groups of kScanQF queries share launches (as many groups
// per launch as kListPartBytes of partial lists hold), the last partial group takes its own.
constexpr size_t kListPartBytes = 64u << 20;
static int run_list_scan(bsr_index* ix, const int32_t* ids, uint32_t n_ids, uint32_t k, const uint32_t* list,
                         uint32_t n_list) {
    if (!n_ids || !n_list) return BSR_OK;
    const uint32_t grid = scan_grid_for(n_list);
    const size_t group_bytes = (size_t)grid * kScanQF * k * sizeof(uint64_t);
    const uint32_t full = n_ids / kScanQF, rest = n_ids % kScanQF;
    const uint32_t per_launch = (uint32_t)std::min<size_t>(std::max<size_t>(kListPartBytes / group_bytes, 1), 65535);
    BSR_TRY(ix->part.ensure(group_bytes * std::max(1u, std::min(per_launch, full))));
    auto scan = [&](uint32_t g0, uint32_t groups, uint32_t nqf) -> int {
        BSR_HIP(launch_scan_list(ix->rows.as<float>(), ix->ld, ix->dim, list, n_list,
                                 ix->na.as<float>(), ix->qf32.as<float>(), ids + (size_t)g0 * kScanQF, nqf, groups,
                                 ix->nb.as<float>(), k, grid, ix->part.as<uint64_t>(), ix->stream));
        for (uint32_t g = 0; g < groups; ++g)
            BSR_HIP(launch_merge_parts(ix->part.as<uint64_t>() + (size_t)g * grid * kScanQF * k, grid,
                                       ids + (size_t)(g0 + g) * kScanQF, nqf, k, ix->keys.as<uint64_t>(), ix->stream));
        return BSR_OK;
    };
    ev_begin(ix, ix->ev_scan, 1);
    for (uint32_t g0 = 0; g0 < full; g0 += per_launch) BSR_TRY(scan(g0, std::min(per_launch, full - g0), kScanQF));
    if (rest) BSR_TRY(scan(full, 1, rest));
    ev_end(ix, ix->ev_scan);
    return BSR_OK;
}

// The masked filter path's lowered threshold: with a fraction rho = A / n of the
// rows allowed, the ks_m = ceil(ks_for(k) / rho)-th best sampled score lets as many ALLOWED rows
// through as the unmasked search's threshold lets rows through; 0 when launch_select_tau cannot
// select that deep (ks_m > 128, i.e. rho < ks_for(k) / 128).  n: the shard's LIVE rows -- deleted
// rows score 0 and are out of the sample's order statistics already, so the
// threshold is lowered by live / A only.
static uint32_t masked_ks(uint32_t k, uint64_t n, uint64_t A) {
    if (!A) return 0;
    const uint64_t ks_m = ((uint64_t)ks_for(k) * n + A - 1) / A;
    return ks_m <= 128 ? (uint32_t)ks_m : 0u;
}

// BSR_MASK_AUTO's choice where both paths are possible, a pure function of (n, A, nq, k): whether
// the list scan is expected to beat the filter path (the measured table).
// Measured (1M x 768 rows, k = 10, profiles/masked_bench.json): the list scan costs 0.52 ns per
// listed row for one query (HBM-bound) and 1.30 ns per row and group of kScanQF queries
// (VALU-bound), taken as linear in the queries per group between the two; the filter path costs
// one pass over the shard whatever A is.  One query: the list wins at A = n / 4 (0.24 vs 0.30
// ms), the filter at n / 2 (0.28 vs 0.37 ms), the lines cross near n / 3.  1000 queries: the
// filter wins wherever it is possible.  Hence: the list when groups x A x w <= n / 3, w = 1 for
// one query per group up to 2.6 for kScanQF.  k does not enter (the filter's range does that).
static bool auto_prefers_list(uint64_t n, uint64_t A, uint32_t nq, uint32_t k) {
    (void)k;
    const uint64_t groups = (nq + kScanQF - 1) / kScanQF;
    const uint64_t w100 = 100 + 23 * (uint64_t)(std::min(nq, kScanQF) - 1);
    return 3 * A * groups * w100 <= 100 * n;
}

// Which path a masked search takes.  BSR_MASK_FILTER: the filter path whenever it is possible
// at all; BSR_MASK_AUTO: where it is possible and auto_prefers_list says no.
static bool masked_filter_path(const bsr_index* ix, uint32_t mode, uint64_t A, uint32_t nq, uint32_t k) {
    const bool possible = ix->n > 0 && ix->approx_ok && k <= kMaxKForFilter && ix->n > cap_for(k) && A >= 1 &&
                          masked_ks(k, ix->live_rows(), A) != 0;
    if (!possible || mode == BSR_MASK_LIST) return false;
    return !(mode == BSR_MASK_AUTO && auto_prefers_list(ix->n, A, nq, k));
}

// The masked filter stage behind the cut, shared by the two masked searches: every remaining row of
// every query rescored exactly and certified against tau0 (mode B; raw_cnt / items: the cut's
// outputs, n_rows: what the fused finalize counts against), then read_bytes of the result read back
// (the status words lead it), the host polling the stream.  *nfail = the queries left to the list scan.
static int masked_filter_stage(bsr_index* ix, uint32_t nq, uint32_t k, const uint32_t* raw_cnt, const uint32_t* items,
                               uint32_t cap_m, uint64_t n_rows, size_t read_bytes, uint32_t* nfail) {
    ev_begin(ix, ix->ev_rescore);
    RescoreArgs rb = rescore_args(ix, nq, k);
    rb.n_items_dev = items;
    rb.qlist = reinterpret_cast<const uint32_t*>(ix->qids_id.as<int32_t>());  // (identity for q < nq)
    rescore_emitted(rb, ix, cap_m);
    rb.fail_cnt = ix->d_status + kStFail2;
    rb.fail_list = ix->fail2.as<uint32_t>();
    rb.n_rows = n_rows;
    rescore_bookkeeping(rb, ix, nq, raw_cnt);
    BSR_HIP(launch_rescore(rb, ix->stream));
    ev_end(ix, ix->ev_rescore);
    ix->next_status_clean = true;
    ev_end(ix, ix->ev_total);
    BSR_HIP(hipMemcpyAsync(ix->h_res, ix->res[ix->cur].p, read_bytes, hipMemcpyDeviceToHost, ix->stream));
    BSR_HIP(stream_wait(ix->stream));
    BSR_TRY(check_queries(ix, nq));
    const uint32_t* st = reinterpret_cast<const uint32_t*>(ix->h_res);
    ix->stats.n_emitted = st[kStEmitted];
    *nfail = st[kStFail2];
    return BSR_OK;
}

int bsr_index::search_device_masked(const float* queries, uint32_t nq, uint32_t k, const uint64_t* allow,
                                    uint64_t allow_words, uint32_t mode) {
    bsr_index* ix = this;
    BSR_TRY(check_batch(ix, k));
    if (!allow) return set_error(BSR_E_INVALID, "null allow mask (bsr_local_top_k searches without one)");
    if (mode != BSR_MASK_AUTO && mode != BSR_MASK_LIST && mode != BSR_MASK_FILTER)
        return set_error(BSR_E_INVALID, "unknown mask mode %u", mode);
    if (allow_words != (n + 63) / 64)
        return set_error(BSR_E_INVALID, "allow_words=%llu, the index holds %llu rows (%llu words)",
                         (unsigned long long)allow_words, (unsigned long long)n, (unsigned long long)((n + 63) / 64));
    BSR_TRY(begin_batch(ix, nq, k));
    if (nq == 0) return BSR_OK;
    if (!queries) return set_error(BSR_E_INVALID, "null queries");

    const uint32_t qpad = qpad_for(nq);
    BSR_TRY(query_buffers(ix, nq, qpad, k));
    BSR_TRY(mask_aux.ensure(((size_t)qpad + 1) * sizeof(uint32_t)));

    ev_begin(ix, ev_total);
    const float* qsrc = nullptr;
    BSR_TRY(stage_queries(ix, queries, nq, &qsrc));
    // The mask on the device, and the number of allowed rows A: the host needs it for the path,
    // the list's size and the result count min(k, A).
    // (tombstones: what drives A, the list, the cut and the counts is allow & ~dead, formed by every
    // mask kernel as it reads)
    const uint64_t* dmask = allow;
    uint32_t A = 0;
    if (n > 0) {
        BSR_TRY(on_device(ix, mask_dev, allow, (size_t)allow_words * sizeof(uint64_t), is_device_ptr(allow), &dmask));
        const uint32_t n_blk = mask_blocks(n);
        BSR_TRY(mask_blk.ensure(((size_t)n_blk + 1) * sizeof(uint32_t)));
        BSR_HIP(launch_mask_list_count(dmask, dead_bits(), n, mask_blk.as<uint32_t>(), stream));
        BSR_HIP(hipMemcpyAsync(&A, mask_blk.as<uint32_t>() + n_blk, sizeof A, hipMemcpyDeviceToHost, stream));
        BSR_HIP(hipStreamSynchronize(stream));
    }
    const bool use_filter = masked_filter_path(ix, mode, A, nq, k);
    const uint32_t ks_m = use_filter ? masked_ks(k, live_rows(), A) : 0u;
    const uint32_t cap_m = 128u * ks_m;  // (cap_for / ks_for's ratio)
    stats.search_path |= use_filter ? BSR_PATH_MASK_FILTER : BSR_PATH_MASK_LIST;
    BSR_HIP(launch_query_prep(query_prep_args(ix, qsrc, nq, qpad, use_filter), stream));

    // The list: the fallback of the filter path builds it only when a query needs it.
    bool have_list = false;
    auto build_list = [&]() -> int {
        if (have_list || !A) return BSR_OK;
        BSR_TRY(mask_list.ensure((size_t)A * sizeof(uint32_t)));
        BSR_HIP(launch_mask_list_scatter(dmask, dead_bits(), n, mask_blk.as<uint32_t>(), A, mask_list.as<uint32_t>(),
                                         stream));
        have_list = true;
        return BSR_OK;
    };
    if (!use_filter) {
        // the list path: every query by the exact scan of the allowed rows
        stats.n_exact_direct = nq;
        if (A) {
            BSR_TRY(build_list());
            BSR_TRY(run_list_scan(ix, qids_id.as<int32_t>(), nq, k, mask_list.as<uint32_t>(), A));
        } else {
            BSR_HIP(hipMemsetAsync(keys.p, 0xff, (size_t)nq * k * sizeof(uint64_t), stream));
        }
        BSR_TRY(finalize_and_read(ix, nq, k, A, true));
        return check_queries(ix, nq);
    }

    // The filter path: the threshold lowered by 1 / rho, the emitted lists cut by the mask, every
    // remaining row of every query rescored exactly and certified against tau0 (mode B).
    BSR_TRY(sample_pass(ix, nq, qpad, k, nullptr, ks_m, cap_m));
    BSR_TRY(emit_pass(ix, nq, qpad, k, cap_m));
    uint32_t* raw_cnt = mask_aux.as<uint32_t>();
    uint32_t* items = raw_cnt + qpad;
    BSR_HIP(launch_mask_cut(cand.as<uint64_t>(), cnt.as<uint32_t>(), cap_m, nq, dmask, allow_words, nullptr, dead_bits(),
                            n, raw_cnt, items, stream));
    uint32_t nfail = 0;  // (n_rows = A: the fused finalize's count is min(k, A))
    BSR_TRY(masked_filter_stage(ix, nq, k, raw_cnt, items, cap_m, A, res_bytes, &nfail));
    if (!nfail) return BSR_OK;
    // Uncertified queries (an overflowed list among them) and queries the filter cannot
    // serve take the list scan: the reference's arithmetic on every allowed row.
    BSR_TRY(failed_queries(ix, nq, nfail));
    stats.search_path |= BSR_PATH_MASK_LIST;
    BSR_TRY(build_list());
    BSR_TRY(run_list_scan(ix, qids.as<int32_t>(), nfail, k, mask_list.as<uint32_t>(), A));
    return finalize_and_read(ix, nq, k, A, true);
}

// ---------------------------------------------------------------------------------------
// Grouped masked search (bsr_local_top_k_masked_groups)
// ---------------------------------------------------------------------------------------
// The ids one chunk of row lists may hold: BSR_MASK_LIST_BUDGET bytes (read per search), 256 MB
// by default.  A dense mask per tenant over a large shard would otherwise want n_masks x n ids.
static uint64_t mask_list_budget_ids() {
    return std::max<uint64_t>(env_bytes("BSR_MASK_LIST_BUDGET", 256ull << 20) / sizeof(uint32_t), 1);
}

// What the two grouped list scans (top-k here, the range in §17) plan alike.
// The queries `listed` (ascending ids) whose mask allows a row, by mask and ascending within a mask
// (a counting sort): mask g's are order[start[g] .. start[g + 1]).
struct QueriesByMask { std::vector<uint32_t> start, order; };
static QueriesByMask queries_by_mask(const bsr_index* ix, uint32_t n_masks, const std::vector<uint32_t>& listed) {
    const std::vector<uint32_t>& qmask = ix->h_grp_qmask;
    const std::vector<uint32_t>& A = ix->h_grp_out;
    QueriesByMask by{std::vector<uint32_t>(n_masks + 1, 0), {}};
    for (uint32_t q : listed)
        if (A[qmask[q]]) ++by.start[qmask[q] + 1];
    for (uint32_t g = 0; g < n_masks; ++g) by.start[g + 1] += by.start[g];
    by.order.resize(by.start[n_masks]);
    std::vector<uint32_t> at(by.start.begin(), by.start.end() - 1);
    for (uint32_t q : listed)
        if (A[qmask[q]]) by.order[at[qmask[q]]++] = q;
    return by;
}

// A chunk's query groups, one width qf in {8, 4, 2, 1} after the other, appended to h_grp_scan and
// h_grp_ids: every list d[i] (.off, .n_list, .mask: a mask's row list or a segment of it) meets
// every group of its mask's queries -- full groups of kScanQF and one narrower group of the rest in
// the narrowest width that holds it (as launch_scan_list does), padded with the group's first id.
// Returned: the launches, per width one for as many groups as max_groups and, with partial lists
// of k keys (k = 0: none), kListPartBytes hold.
struct GroupLaunch { uint32_t qf, groups, grid; size_t scan0, ids0; };
template <class Desc>
static std::vector<GroupLaunch> plan_query_groups(bsr_index* ix, const Desc* d, size_t n_d, const QueriesByMask& by,
                                                  uint32_t max_groups, uint32_t k) {
    std::vector<ScanGroupDesc>& scans = ix->h_grp_scan;
    std::vector<int32_t>& ids = ix->h_grp_ids;
    std::vector<GroupLaunch> launches;
    for (uint32_t qf = kScanQF; qf >= 1; qf /= 2) {
        const size_t scan0 = scans.size(), ids0 = ids.size();
        uint32_t longest = 0;
        for (size_t l = 0; l < n_d; ++l) {
            const uint32_t q0 = by.start[d[l].mask], nqg = by.start[d[l].mask + 1] - q0, rest = nqg % kScanQF;
            auto group = [&](uint32_t first, uint32_t cnt) {
                scans.push_back(ScanGroupDesc{d[l].off, d[l].n_list, cnt});
                for (uint32_t j = 0; j < qf; ++j) ids.push_back((int32_t)by.order[first + (j < cnt ? j : 0)]);
                longest = std::max(longest, d[l].n_list);
            };
            if (qf == kScanQF)
                for (uint32_t f = 0; f + kScanQF <= nqg; f += kScanQF) group(q0 + f, kScanQF);
            if (rest && rest <= qf && rest > qf / 2) group(q0 + nqg - rest, rest);
        }
        const size_t n_groups = scans.size() - scan0;
        if (!n_groups) continue;
        const uint32_t grid = scan_grid_for(longest);
        size_t per = max_groups;
        if (k) per = std::min(std::max<size_t>(kListPartBytes / ((size_t)grid * qf * k * sizeof(uint64_t)), 1), per);
        for (size_t g0 = 0; g0 < n_groups; g0 += per)
            launches.push_back(GroupLaunch{qf, (uint32_t)std::min(per, n_groups - g0), grid, scan0 + g0, ids0 + g0 * qf});
    }
    return launches;
}

// The exact list scan of the queries `listed` (ascending ids), every one over the list of its own mask
// (DESIGN.md §12).  The masks that have such a query (and a row) are taken in ascending order into
// chunks whose lists fit the budget (a list longer than the budget is a chunk of its own); a
// chunk is one scatter launch, and per width qf in {8, 4, 2, 1} one grouped scan and one merge
// launch for as many query groups as kListPartBytes of partial lists hold.  A mask's queries form
// full groups of kScanQF and one narrower group of the rest, padded with the group's first id;
// no group holds queries of two masks.  The launch count depends on the chunks and the batch size,
// not on n_masks.  keys of queries whose mask allows no row are left as they are (kKeyNone).
static int run_list_scan_groups(bsr_index* ix, uint32_t k, const uint64_t* allow, uint64_t words, uint32_t n_masks,
                                const std::vector<uint32_t>& listed) {
    const std::vector<uint32_t>& A = ix->h_grp_out;
    const QueriesByMask by = queries_by_mask(ix, n_masks, listed);
    const std::vector<uint32_t>& start = by.start;
    if (by.order.empty()) return BSR_OK;

    struct Chunk { size_t list0; uint32_t n_lists; std::vector<GroupLaunch> launches; };
    std::vector<Chunk> chunks;
    std::vector<MaskListDesc>& lists = ix->h_grp_lists;
    std::vector<ScanGroupDesc>& scans = ix->h_grp_scan;
    std::vector<int32_t>& ids = ix->h_grp_ids;
    lists.clear();
    scans.clear();
    ids.clear();
    const uint64_t budget = mask_list_budget_ids();
    uint64_t list_ids = 0;
    size_t part_bytes = 0;
    for (uint32_t g = 0; g < n_masks;) {
        // the chunk's masks [g, g_end)
        Chunk c{lists.size(), 0, {}};
        uint64_t total = 0;
        uint32_t g_end = g;
        for (; g_end < n_masks; ++g_end) {
            if (start[g_end] == start[g_end + 1]) continue;
            if (c.n_lists && total + A[g_end] > budget) break;
            lists.push_back(MaskListDesc{total, g_end, A[g_end]});
            total += A[g_end];
            ++c.n_lists;
        }
        list_ids = std::max(list_ids, total);
        c.launches = plan_query_groups(ix, lists.data() + c.list0, c.n_lists, by, 65535, k);
        for (const GroupLaunch& l : c.launches)
            part_bytes = std::max(part_bytes, (size_t)l.grid * l.qf * k * sizeof(uint64_t) * l.groups);
        if (c.n_lists) chunks.push_back(std::move(c));
        g = g_end;
    }

    BSR_TRY(ix->mask_list.ensure((size_t)list_ids * sizeof(uint32_t)));
    BSR_TRY(ix->part.ensure(part_bytes));
    BSR_TRY(ix->grp_lists.ensure(lists.size() * sizeof(MaskListDesc)));
    BSR_TRY(ix->grp_scan.ensure(scans.size() * sizeof(ScanGroupDesc)));
    BSR_TRY(ix->qids.ensure(ids.size() * sizeof(int32_t)));
    BSR_HIP(hipMemcpyAsync(ix->grp_lists.p, lists.data(), lists.size() * sizeof(MaskListDesc), hipMemcpyHostToDevice,
                           ix->stream));
    BSR_HIP(hipMemcpyAsync(ix->grp_scan.p, scans.data(), scans.size() * sizeof(ScanGroupDesc), hipMemcpyHostToDevice,
                           ix->stream));
    BSR_HIP(hipMemcpyAsync(ix->qids.p, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice, ix->stream));
    ev_begin(ix, ix->ev_scan, 1);
    for (const Chunk& c : chunks) {
        // (the stream orders a chunk's scatter behind the scans of the chunk before it)
        BSR_HIP(launch_mask_groups_scatter(allow, words, ix->n, ix->dead_bits(), ix->grp_blk.as<uint32_t>(),
                                           ix->grp_lists.as<MaskListDesc>() + c.list0, c.n_lists,
                                           ix->mask_list.as<uint32_t>(), ix->stream));
        for (const GroupLaunch& l : c.launches) {
            const ScanGroupDesc* sg = ix->grp_scan.as<ScanGroupDesc>() + l.scan0;
            const int32_t* gid = ix->qids.as<int32_t>() + l.ids0;
            BSR_HIP(launch_scan_list_groups(ix->rows.as<float>(), ix->ld, ix->dim, ix->mask_list.as<uint32_t>(), sg,
                                            l.groups, l.qf, ix->na.as<float>(), ix->qf32.as<float>(), gid,
                                            ix->nb.as<float>(), k, l.grid, ix->part.as<uint64_t>(), ix->stream));
            BSR_HIP(launch_merge_parts_groups(ix->part.as<uint64_t>(), l.grid, gid, l.qf, sg, l.groups, k,
                                              ix->keys.as<uint64_t>(), ix->stream));
        }
    }
    ev_end(ix, ix->ev_scan);
    return BSR_OK;
}

int bsr_index::search_device_masked_groups(const float* queries, uint32_t nq, uint32_t k, const uint64_t* allow,
                                           uint64_t allow_words, uint32_t n_masks, const uint32_t* query_mask,
                                           uint32_t mode) {
    bsr_index* ix = this;
    BSR_TRY(check_batch(ix, k));
    if (n_masks == 0) return set_error(BSR_E_INVALID, "n_masks = 0 (bsr_local_top_k searches without a mask)");
    if (mode != BSR_MASK_AUTO && mode != BSR_MASK_LIST && mode != BSR_MASK_FILTER)
        return set_error(BSR_E_INVALID, "unknown mask mode %u", mode);
    if (allow_words != (n + 63) / 64)
        return set_error(BSR_E_INVALID, "allow_words=%llu, the index holds %llu rows (%llu words)",
                         (unsigned long long)allow_words, (unsigned long long)n, (unsigned long long)((n + 63) / 64));
    if (nq && !allow) return set_error(BSR_E_INVALID, "null allow masks");
    if (nq && !query_mask) return set_error(BSR_E_INVALID, "null query_mask");
    BSR_TRY(begin_batch(ix, nq, k, BSR_PATH_MASK_GROUPS));
    if (nq == 0) return BSR_OK;
    if (!queries) return set_error(BSR_E_INVALID, "null queries");

    const uint32_t qpad = qpad_for(nq);
    BSR_TRY(query_buffers(ix, nq, qpad, k));
    BSR_TRY(mask_aux.ensure(((size_t)qpad + 1) * sizeof(uint32_t)));

    ev_begin(ix, ev_total);
    const float* qsrc = nullptr;
    BSR_TRY(stage_queries(ix, queries, nq, &qsrc));
    // The masks and the mask ids on the device; the ids on the host too (it forms the query groups).
    const uint64_t* dallow = allow;
    if (allow_words)
        BSR_TRY(on_device(ix, mask_dev, allow, (size_t)n_masks * allow_words * sizeof(uint64_t), is_device_ptr(allow),
                          &dallow));
    const uint32_t* dqmask = query_mask;
    h_grp_qmask.resize(nq);
    if (is_device_ptr(query_mask)) {
        BSR_HIP(hipMemcpyAsync(h_grp_qmask.data(), query_mask, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               stream));
    } else {
        memcpy(h_grp_qmask.data(), query_mask, (size_t)nq * sizeof(uint32_t));
        BSR_TRY(grp_qmask.ensure((size_t)nq * sizeof(uint32_t)));
        BSR_HIP(hipMemcpyAsync(grp_qmask.p, h_grp_qmask.data(), (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice,
                               stream));
        dqmask = grp_qmask.as<uint32_t>();
    }
    // Every A_g (over allow_g & ~dead) and the check of query_mask: two launches, one copy of
    // n_masks + 1 words, the search's one stream wait before it picks the paths.
    const uint32_t n_blk = mask_blocks(n);
    BSR_TRY(grp_blk.ensure((size_t)n_masks * (n_blk + 1) * sizeof(uint32_t)));
    BSR_TRY(grp_out.ensure(((size_t)n_masks + 1) * sizeof(uint32_t)));
    h_grp_out.resize((size_t)n_masks + 1);
    BSR_HIP(launch_mask_groups_count(dallow, allow_words, n_masks, n, dead_bits(), dqmask, nq, grp_blk.as<uint32_t>(),
                                     grp_out.as<uint32_t>(), stream));
    BSR_HIP(hipMemcpyAsync(h_grp_out.data(), grp_out.p, ((size_t)n_masks + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           stream));
    BSR_HIP(hipStreamSynchronize(stream));
    if (h_grp_out[n_masks])
        return set_error(BSR_E_INVALID, "%u entries of query_mask name no mask (n_masks = %u)", h_grp_out[n_masks],
                         n_masks);

    // The path of every mask group, from its own A_g and query count.
    std::vector<uint32_t> nq_g(n_masks, 0), ks_g(n_masks, 0);
    for (uint32_t q = 0; q < nq; ++q) ++nq_g[h_grp_qmask[q]];
    uint32_t ks_max = 0, n_list_q = 0;
    uint64_t min_a = ~0ull;
    for (uint32_t g = 0; g < n_masks; ++g) {
        if (!nq_g[g] || !masked_filter_path(ix, mode, h_grp_out[g], nq_g[g], k)) continue;
        ks_g[g] = masked_ks(k, live_rows(), h_grp_out[g]);
        ks_max = std::max(ks_max, ks_g[g]);
        min_a = std::min<uint64_t>(min_a, h_grp_out[g]);
    }
    const bool any_filter = ks_max != 0;
    const uint32_t cap_m = 128u * ks_max;  // (one emission cap for the batch)
    std::vector<uint8_t> on_list(nq, 0);
    h_grp_ksq.assign(qpad, 0);
    h_grp_aq.resize(nq);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t g = h_grp_qmask[q];
        h_grp_aq[q] = h_grp_out[g];
        h_grp_ksq[q] = ks_g[g];
        on_list[q] = ks_g[g] == 0;
        n_list_q += on_list[q];
    }
    // (the fused finalize of the rescore counts min(k, n_rows): every filter group has more than k rows)
    if (any_filter && min_a < k) return set_error(BSR_E_STATE, "a filter group of %llu rows at k=%u", (unsigned long long)min_a, k);
    stats.search_path |= (any_filter ? BSR_PATH_MASK_FILTER : 0u) | (n_list_q ? BSR_PATH_MASK_LIST : 0u);
    stats.n_exact_direct = n_list_q;
    BSR_TRY(grp_aq.ensure((size_t)nq * sizeof(uint32_t)));
    BSR_HIP(hipMemcpyAsync(grp_aq.p, h_grp_aq.data(), (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    // (a query whose mask allows no row is never scanned: its keys stay empty)
    BSR_HIP(hipMemsetAsync(keys.p, 0xff, (size_t)nq * k * sizeof(uint64_t), stream));
    BSR_HIP(launch_query_prep(query_prep_args(ix, qsrc, nq, qpad, any_filter), stream));

    if (any_filter) {
        // The filter, once over the batch: every query's threshold at its own depth (a list-group
        // query's at +inf: it emits nothing), the lists cut by the query's own mask, every remaining
        // row rescored exactly and certified against tau[q] (mode B).
        BSR_TRY(grp_ksq.ensure((size_t)qpad * sizeof(uint32_t)));
        BSR_HIP(hipMemcpyAsync(grp_ksq.p, h_grp_ksq.data(), (size_t)qpad * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        BSR_TRY(sample_pass(ix, nq, qpad, k, nullptr, ks_max, cap_m, grp_ksq.as<uint32_t>()));
        BSR_TRY(emit_pass(ix, nq, qpad, k, cap_m));
        uint32_t* raw_cnt = mask_aux.as<uint32_t>();
        uint32_t* items = raw_cnt + qpad;
        BSR_HIP(launch_mask_cut(cand.as<uint64_t>(), cnt.as<uint32_t>(), cap_m, nq, dallow, allow_words, dqmask,
                                dead_bits(), n, raw_cnt, items, stream));
        // (n_rows = min_a >= k: the count of every filter-group query is k; with list-group queries
        // the rows are read after their scan: the status words alone here)
        uint32_t nfail = 0;
        BSR_TRY(masked_filter_stage(ix, nq, k, raw_cnt, items, cap_m, min_a,
                                    n_list_q ? kStWords * sizeof(uint32_t) : res_bytes, &nfail));
        if (!nfail && !n_list_q) return BSR_OK;
        if (nfail) {
            // Uncertified queries and queries the filter cannot serve join the list scan; the
            // list-group queries among them (empty lists: mode B fails them) are there already.
            BSR_TRY(read_failed(ix, nq, nfail));
            for (uint32_t q : h_fail) {
                if (q >= nq || on_list[q]) continue;
                on_list[q] = 1;
                if (h_qflags[q] & kQueryNoApprox) ++stats.n_exact_direct;
                else ++stats.n_fallback;
            }
            stats.search_path |= BSR_PATH_MASK_LIST;
        }
    }
    std::vector<uint32_t> listed;
    for (uint32_t q = 0; q < nq; ++q)
        if (on_list[q]) listed.push_back(q);
    BSR_TRY(run_list_scan_groups(ix, k, dallow, allow_words, n_masks, listed));
    BSR_TRY(finalize_and_read(ix, nq, k, 0, true, grp_aq.as<uint32_t>()));
    return check_queries(ix, nq);
}

// ---------------------------------------------------------------------------------------
// The parallel search's global emission threshold: phase A / phase B
// ---------------------------------------------------------------------------------------
bool bsr_index::gtau_eligible(uint32_t nq, uint32_t k) const {
    // the filter path with a sample pass (a shard of more rows than one query's candidate list)
    // (not while a row is deleted: its rescore and the merge's need = min(k, corpus rows) count
    // every row -- the header then takes every rank to the standard path)
    return loaded && nq > 0 && k >= 1 && k <= cfg.max_k && k <= kMaxKForFilter && approx_ok && n > cap_for(k) &&
           n_dead == 0;
}

// Phase A's buffers (the result buffer of this search, the query and filter scratch, the sample
// scores, the ks best keys): everything that can fail short of a device error, done before the
// parallel search posts its header -- which is then posted before phase A's kernels, so that
// its round trip overlaps them (round 5: posted after them it could finish behind the sample
// pass and hold the host's enqueue of phase B, +25 us per search in the loopback timeline).
int bsr_index::gtau_prepare(const float* queries, uint32_t nq, uint32_t k) {
    if (!gtau_eligible(nq, k)) return set_error(BSR_E_STATE, "global-threshold search not applicable");
    if (!queries) return set_error(BSR_E_INVALID, "null queries");
    BSR_TRY(begin_batch(this, nq, k));
    const uint32_t qpad = (uint32_t)round_up(nq, kFilterTile);
    const uint32_t ks = ks_for(k);
    BSR_TRY(query_buffers(this, nq, qpad, k));
    BSR_TRY(smax.ensure((size_t)qpad * ks * sizeof(uint64_t)));
    if (!is_device_ptr(queries)) BSR_TRY(q_in.ensure((size_t)nq * dim * sizeof(float)));
    BSR_TRY(filter_buffers(this, nq, qpad, k));
    BSR_TRY(S.ensure((size_t)qpad * sample_layout(this, nq, ks).s_ld * sizeof(float)));  // (sample_pass's size)
    gt_nq = nq;
    gt_k = k;
    gt_qpad = qpad;
    gt_ks = ks;
    return BSR_OK;
}

// Phase A's work, enqueued (after gtau_prepare sized every buffer: nothing is allocated here), in
// two parts so that the parallel search can post its header between them: the query prep (the
// GPU starts on it while the host issues the header's launches), then the sample pass and tau0.
int bsr_index::gtau_phase_a(const float* queries, int part) {
    bsr_index* ix = this;
    const uint32_t nq = gt_nq, k = gt_k, qpad = gt_qpad;
    if (part == 1) {
        BSR_TRY(sample_pass(ix, nq, qpad, k, smax.as<uint64_t>()));
        return BSR_OK;
    }
    const float* qsrc = nullptr;
    BSR_TRY(stage_queries(ix, queries, nq, &qsrc));  // (q_in: sized by gtau_prepare)
    ev_begin(ix, ev_total);
    BSR_HIP(launch_query_prep(query_prep_args(ix, qsrc, nq, qpad, true), stream));
    return BSR_OK;
}

int bsr_index::gtau_phase_b(const uint64_t* g_smax, uint32_t P, uint32_t* merge_words) {
    bsr_index* ix = this;
    const uint32_t nq = gt_nq, k = gt_k, qpad = gt_qpad;
    BSR_HIP(launch_global_tau(g_smax, P, qpad, nq, gt_ks, qflags.as<uint32_t>(), tau.as<float>(), stream));
    BSR_TRY(emit_pass(ix, nq, qpad, k));
    // every emitted row rescored exactly, one wave per query (mode B); the list is this rank's
    // contribution, its exclusion bound goes with it (the root certifies the merged lists)
    ev_begin(ix, ev_rescore);
    RescoreArgs ra = rescore_args(ix, nq, k);
    rescore_emitted(ra, ix, cap_for(k));
    ra.excl_out = d_x;
    rescore_bookkeeping(ra, ix, nq, cnt.as<uint32_t>());
    ra.merge_words = merge_words;  // (the merge's two words: no memset launches before it)
    BSR_HIP(launch_rescore(ra, stream));
    ev_end(ix, ev_rescore);
    ev_end(ix, ev_total);  // (the local part: phases A and B, the all-gather between them included)
    next_status_clean = true;
    return BSR_OK;
}

// Results of the last search to the caller's arrays: from the pinned host mirror for host
// arrays, device-to-device for device arrays.
static int copy_out(bsr_index* ix, uint32_t nq, uint32_t k, uint64_t* out_idx, float* out_dist, uint32_t* out_count) {
    const size_t nk = (size_t)nq * k;
    const bool dev = is_device_ptr(out_idx) || is_device_ptr(out_dist) || is_device_ptr(out_count);
    if (!dev) {
        if (out_idx) memcpy(out_idx, ix->h_res + ix->res_off_idx, nk * sizeof(uint64_t));
        if (out_dist) memcpy(out_dist, ix->h_res + ix->res_off_dist, nk * sizeof(float));
        if (out_count) memcpy(out_count, ix->h_res + ix->res_off_cnt, (size_t)nq * sizeof(uint32_t));
        return BSR_OK;
    }
    if (out_idx) BSR_HIP(hipMemcpyAsync(out_idx, ix->d_idx, nk * sizeof(uint64_t), hipMemcpyDefault, ix->stream));
    if (out_dist) BSR_HIP(hipMemcpyAsync(out_dist, ix->d_dist, nk * sizeof(float), hipMemcpyDefault, ix->stream));
    if (out_count) BSR_HIP(hipMemcpyAsync(out_count, ix->d_cnt, (size_t)nq * sizeof(uint32_t), hipMemcpyDefault, ix->stream));
    BSR_HIP(hipStreamSynchronize(ix->stream));
    return BSR_OK;
}

int bsr_copy_out_impl(bsr_index* ix, uint32_t nq, uint32_t k, uint64_t* out_idx, float* out_dist,
                      uint32_t* out_count) {
    return copy_out(ix, nq, k, out_idx, out_dist, out_count);
}

static void collect_profile(bsr_index* ix) {
    if (!profiling(ix)) return;
    bsr_profile& p = ix->prof;
    ev_collect(ix->ev_emit, p.gemm_emit_ms, p.gemm_emit_launches, 1);
    ev_collect(ix->ev_sample, p.gemm_sample_ms, p.gemm_sample_launches, 1);
    ev_collect(ix->ev_select, p.select_ms, p.select_launches, 1);
    ev_collect(ix->ev_rescore, p.rescore_ms, p.rescore_launches, 1);
    ev_collect(ix->ev_scan, p.scan_ms, p.scan_launches, 1);
    ev_collect(ix->ev_total, p.search_ms, p.searches, 1);
}

// A local top-k entry point around its search: the null checks, the search, the results to the
// caller's arrays, the profile.
template <class F>
static int top_k_call(bsr_index* ix, uint32_t nq, uint32_t k, uint64_t* out_idx, float* out_dist, uint32_t* out_count,
                      F&& search) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    if (nq && (!out_idx || !out_dist || !out_count)) return set_error(BSR_E_INVALID, "null output");
    BSR_TRY(search());
    BSR_TRY(copy_out(ix, nq, k, out_idx, out_dist, out_count));
    collect_profile(ix);
    return BSR_OK;
}

int bsr_local_top_k_impl(bsr_index* ix, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_idx,
                         float* out_dist, uint32_t* out_count) {
    return top_k_call(ix, nq, k, out_idx, out_dist, out_count, [&] { return ix->search_device(queries, nq, k); });
}

int bsr_local_top_k_masked_impl(bsr_index* ix, const float* queries, uint32_t nq, uint32_t k, const uint64_t* allow,
                                uint64_t allow_words, uint32_t mode, uint64_t* out_idx, float* out_dist,
                                uint32_t* out_count) {
    return top_k_call(ix, nq, k, out_idx, out_dist, out_count,
                      [&] { return ix->search_device_masked(queries, nq, k, allow, allow_words, mode); });
}

int bsr_local_top_k_masked_groups_impl(bsr_index* ix, const float* queries, uint32_t nq, uint32_t k,
                                       const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                       const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx, float* out_dist,
                                       uint32_t* out_count) {
    return top_k_call(ix, nq, k, out_idx, out_dist, out_count, [&] {
        return ix->search_device_masked_groups(queries, nq, k, allow, allow_words, n_masks, query_mask, mode);
    });
}

// ---------------------------------------------------------------------------------------
// Range search (bsr_local_range_search)
// ---------------------------------------------------------------------------------------
// The exact range scan of n_ids queries (device id list in groups of kScanQF, the last group padded
// with valid ids, as run_exact_scan's): every row of the shard, the deleted ones skipped by their bit.
static int run_range_scan(bsr_index* ix, RangeArgs ra, const int32_t* ids, uint32_t n_ids) {
    const uint32_t grid = scan_grid_for(ix->n);
    ev_begin(ix, ix->ev_scan, 1);
    for (uint32_t g = 0; g * kScanQF < n_ids; ++g) {
        ra.qids = ids + (size_t)g * kScanQF;
        ra.nqf = std::min(kScanQF, n_ids - g * kScanQF);
        BSR_HIP(launch_range_scan(ra, grid, ix->stream));
    }
    ev_end(ix, ix->ev_scan);
    return BSR_OK;
}

int bsr_index::range_search_device(const float* queries, uint32_t nq, const float* radius, uint32_t capacity,
                                   uint64_t* out_idx, float* out_dist, uint32_t* out_count) {
    bsr_index* ix = this;
    BSR_TRY(check_batch(ix, 1));
    // (host radii: a NaN is refused before any device work; device radii are checked by the
    // threshold kernel, and nothing is written to the caller's arrays before the status is read)
    const bool radius_dev = is_device_ptr(radius);
    if (!radius_dev)
        for (uint32_t q = 0; q < nq; ++q)
            if (radius[q] != radius[q]) return set_error(BSR_E_INVALID, "radius[%u] is NaN", q);
    BSR_TRY(begin_batch(ix, nq, 1, BSR_PATH_RANGE));
    if (nq == 0) return BSR_OK;

    const uint32_t cap = range_cap(capacity);
    const uint32_t qpad = qpad_for(nq);
    BSR_TRY(query_buffers(ix, nq, qpad, 1));
    BSR_TRY(filter_buffers(ix, nq, qpad, 1, cap));
    stats.n_candidates = 0;
    BSR_TRY(rng_keys.ensure((size_t)nq * cap * sizeof(uint64_t)));
    BSR_TRY(rng_cnt.ensure((size_t)nq * sizeof(uint32_t)));
    BSR_TRY(rng_idx.ensure((size_t)nq * capacity * sizeof(uint64_t)));
    BSR_TRY(rng_dist.ensure((size_t)nq * capacity * sizeof(float)));
    BSR_TRY(rng_out_cnt.ensure((size_t)nq * sizeof(uint32_t)));

    ev_begin(ix, ev_total);
    const float* qsrc = nullptr;
    BSR_TRY(stage_queries(ix, queries, nq, &qsrc));
    const float* rsrc = nullptr;
    BSR_TRY(on_device(ix, rng_radius, radius, (size_t)nq * sizeof(float), radius_dev, &rsrc));
    // An index that cannot filter scans every query: no int8 operand worth a threshold
    // (BSR_FLAG_EXACT_ONLY, sticky norm flags), or no more rows than one emitted list holds.
    const uint64_t live = live_rows();
    const bool use_filter = live > 0 && approx_ok && n > cap;
    BSR_HIP(launch_query_prep(query_prep_args(ix, qsrc, nq, qpad, use_filter), stream));
    // (the thresholds; in every mode: the zeroed counts and the device check of the radii)
    BSR_HIP(launch_range_tau(rsrc, ebound.as<float>(), nb.as<float>(), qflags.as<uint32_t>(), nq, qpad,
                             tau.as<float>(), cnt.as<uint32_t>(), rng_cnt.as<uint32_t>(), fail.as<uint32_t>(), d_status,
                             stream));
    RangeArgs ra{};
    ra.rows = rows.as<float>();
    ra.ld = ld;
    ra.dim = dim;
    ra.n = n;
    ra.na = na.as<float>();
    ra.qf32 = qf32.as<float>();
    ra.nb = nb.as<float>();
    ra.radius = rsrc;
    ra.dead = dead_bits();
    ra.keys = rng_keys.as<uint64_t>();
    ra.rcnt = rng_cnt.as<uint32_t>();
    ra.cap = cap;
    ra.nq = nq;
    ra.cand = cand.as<uint64_t>();
    ra.cnt = cnt.as<uint32_t>();
    ra.scan_list = fail.as<uint32_t>();
    ra.status = d_status;
    if (use_filter) {
        // the emit pass over every tile (no sample pass ran: no sample tiles to skip, no fix-up),
        // then the exact rescore of every emitted row against the radius
        smp_tiles = 0;
        BSR_TRY(emit_pass(ix, nq, qpad, 1, cap));
        ev_begin(ix, ev_rescore);
        BSR_HIP(launch_range_rescore(ra, stream));
        ev_end(ix, ev_rescore);
    } else if (live > 0) {
        stats.n_exact_direct = nq;
        stats.search_path |= BSR_PATH_RANGE_SCAN;
        BSR_TRY(run_range_scan(ix, ra, qids_id.as<int32_t>(), nq));
    }
    // The one status readback: the query flags (a non-finite query, a NaN radius) and the number
    // of queries left to the scan.
    BSR_HIP(hipMemcpyAsync(h_res, d_status, kStWords * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    BSR_HIP(stream_wait(stream));
    BSR_TRY(check_queries(ix, nq));
    const uint32_t* st = reinterpret_cast<const uint32_t*>(h_res);
    if (st[kStQueryFlags] & kRangeNanRadius) return set_error(BSR_E_INVALID, "a radius of the batch is NaN");
    if (use_filter) {
        stats.n_emitted = st[kStEmitted];
        const uint32_t nscan = st[kStFail], ndirect = st[kStFail2];
        stats.n_exact_direct = ndirect;
        stats.n_fallback = nscan - ndirect;
        if (nscan) {
            // queries the filter cannot serve, and queries whose emitted list overflowed
            stats.search_path |= BSR_PATH_RANGE_SCAN;
            h_fail.resize(nscan);
            BSR_HIP(hipMemcpy(h_fail.data(), fail.p, (size_t)nscan * sizeof(uint32_t), hipMemcpyDeviceToHost));
            std::sort(h_fail.begin(), h_fail.end());
            const std::vector<int32_t> padded = padded_scan_ids(h_fail, nscan);
            BSR_TRY(qids.ensure(padded.size() * sizeof(int32_t)));
            BSR_HIP(hipMemcpyAsync(qids.p, padded.data(), padded.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                   stream));
            BSR_HIP(hipStreamSynchronize(stream));  // (padded is read by the copy)
            BSR_TRY(run_range_scan(ix, ra, qids.as<int32_t>(), nscan));
        }
    }
    // The lists sorted into result rows: straight into the caller's arrays when all three are on
    // the device, else into the index's own and copied out.
    const bool out_dev = is_device_ptr(out_idx) && is_device_ptr(out_dist) && is_device_ptr(out_count);
    uint64_t* di = out_dev ? out_idx : rng_idx.as<uint64_t>();
    float* dd = out_dev ? out_dist : rng_dist.as<float>();
    uint32_t* dc = out_dev ? out_count : rng_out_cnt.as<uint32_t>();
    BSR_HIP(launch_range_finish(rng_keys.as<uint64_t>(), rng_cnt.as<uint32_t>(), cap, nq, capacity, global_offset, di,
                                dd, dc, stream));
    ev_end(ix, ev_total);
    if (!out_dev) {
        const size_t nk = (size_t)nq * capacity;
        BSR_HIP(hipMemcpyAsync(out_idx, di, nk * sizeof(uint64_t), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_dist, dd, nk * sizeof(float), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_count, dc, (size_t)nq * sizeof(uint32_t), hipMemcpyDefault, stream));
    }
    BSR_HIP(hipStreamSynchronize(stream));
    return BSR_OK;
}

int bsr_local_range_search_impl(bsr_index* ix, const float* queries, uint32_t nq, const float* radius,
                                uint32_t capacity, uint64_t* out_idx, float* out_dist, uint32_t* out_count) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    if (capacity == 0 || capacity > BSR_RANGE_MAX_RESULTS)
        return set_error(BSR_E_INVALID, "capacity=%u outside [1, %u]", capacity, BSR_RANGE_MAX_RESULTS);
    if (nq && !radius) return set_error(BSR_E_INVALID, "null radius");
    if (nq && !queries) return set_error(BSR_E_INVALID, "null queries");
    if (nq && (!out_idx || !out_dist || !out_count)) return set_error(BSR_E_INVALID, "null output");
    BSR_TRY(ix->range_search_device(queries, nq, radius, capacity, out_idx, out_dist, out_count));
    collect_profile(ix);
    return BSR_OK;
}

// ---------------------------------------------------------------------------------------
// Scoring caller-chosen rows (bsr_local_score_ids / bsr_local_rerank_ids)
// ---------------------------------------------------------------------------------------
int bsr_index::score_ids_device(const float* queries, uint32_t nq, const uint64_t* ids, uint32_t m, uint32_t k,
                                uint64_t* out_idx, float* out_dist, uint32_t* out_cnt) {
    bsr_index* ix = this;
    if (!loaded) return set_error(BSR_E_STATE, "index not loaded");
    BSR_TRY(begin_batch(ix, nq, 1, BSR_PATH_SCORE));
    stats.row_ebound = 0.0f;  // (no filter runs: every field but the three below stays 0)
    stats.n_candidates = m;
    if (nq == 0) return BSR_OK;

    const bool rerank = k > 0;
    const size_t nm = (size_t)nq * m;
    const uint32_t qpad = qpad_for(nq);
    BSR_TRY(query_buffers(ix, nq, qpad, 1));
    BSR_TRY(scr_cnt.ensure((size_t)nq * sizeof(uint32_t)));
    if (rerank) {
        BSR_TRY(scr_keys.ensure(nm * sizeof(uint64_t)));
        BSR_TRY(scr_idx.ensure((size_t)nq * k * sizeof(uint64_t)));
        BSR_TRY(scr_odist.ensure((size_t)nq * k * sizeof(float)));
        BSR_TRY(scr_ocnt.ensure((size_t)nq * sizeof(uint32_t)));
    } else {
        BSR_TRY(scr_dist.ensure(nm * sizeof(float)));
    }

    ev_begin(ix, ev_total);
    const float* qsrc = nullptr;
    BSR_TRY(stage_queries(ix, queries, nq, &qsrc));
    const uint64_t* isrc = nullptr;
    BSR_TRY(on_device(ix, scr_ids, ids, nm * sizeof(uint64_t), is_device_ptr(ids), &isrc));
    // (no filter operand: BSR_FLAG_EXACT_ONLY and the sticky norm flags do not matter here)
    BSR_HIP(launch_query_prep(query_prep_args(ix, qsrc, nq, qpad, false), stream));
    BSR_HIP(hipMemsetAsync(scr_cnt.p, 0, (size_t)nq * sizeof(uint32_t), stream));
    ScoreArgs sa{};
    sa.rows = rows.as<float>();
    sa.ld = ld;
    sa.dim = dim;
    sa.n = n;
    sa.offset = global_offset;
    sa.na = na.as<float>();
    sa.qf32 = qf32.as<float>();
    sa.nb = nb.as<float>();
    sa.dead = dead_bits();
    sa.ids = isrc;
    sa.m = m;
    sa.nq = nq;
    if (rerank) {
        sa.keys = scr_keys.as<uint64_t>();
        sa.kcnt = scr_cnt.as<uint32_t>();
    } else {
        sa.dist = scr_dist.as<float>();
        sa.found = scr_cnt.as<uint32_t>();
    }
    ev_begin(ix, ev_rescore);
    BSR_HIP(launch_score_ids(sa, stream));
    if (rerank)
        BSR_HIP(launch_score_finish(scr_keys.as<uint64_t>(), scr_cnt.as<uint32_t>(), m, nq, k, global_offset,
                                    scr_idx.as<uint64_t>(), scr_odist.as<float>(), scr_ocnt.as<uint32_t>(), stream));
    ev_end(ix, ev_rescore);
    // The one status readback (a non-finite query), before any of the caller's arrays is written.
    BSR_HIP(hipMemcpyAsync(h_res, d_status, kStWords * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    BSR_HIP(stream_wait(stream));
    BSR_TRY(check_queries(ix, nq));
    if (rerank) {
        const size_t nk = (size_t)nq * k;
        BSR_HIP(hipMemcpyAsync(out_idx, scr_idx.p, nk * sizeof(uint64_t), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_dist, scr_odist.p, nk * sizeof(float), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_cnt, scr_ocnt.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDefault, stream));
    } else {
        BSR_HIP(hipMemcpyAsync(out_dist, scr_dist.p, nm * sizeof(float), hipMemcpyDefault, stream));
        if (out_cnt) BSR_HIP(hipMemcpyAsync(out_cnt, scr_cnt.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDefault, stream));
    }
    ev_end(ix, ev_total);
    BSR_HIP(hipStreamSynchronize(stream));
    return BSR_OK;
}

// The first checks of both entry points, before any device is touched.
static int check_score_args(const bsr_index* ix, uint32_t nq, uint32_t m) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    if (m == 0) return set_error(BSR_E_INVALID, "m = 0 (an id list has at least one slot)");
    if ((uint64_t)nq * m > 0xffffffffull)
        return set_error(BSR_E_INVALID, "n_queries * m = %llu does not fit 32 bits", (unsigned long long)nq * m);
    return BSR_OK;
}

int bsr_local_score_ids_impl(bsr_index* ix, const float* queries, uint32_t nq, const uint64_t* ids, uint32_t m,
                             float* out_dist, uint32_t* out_found) {
    BSR_TRY(check_score_args(ix, nq, m));
    if (nq && !queries) return set_error(BSR_E_INVALID, "null queries");
    if (nq && !ids) return set_error(BSR_E_INVALID, "null ids");
    if (nq && !out_dist) return set_error(BSR_E_INVALID, "null output");
    BSR_TRY(ix->score_ids_device(queries, nq, ids, m, 0, nullptr, out_dist, out_found));
    collect_profile(ix);
    return BSR_OK;
}

int bsr_local_rerank_ids_impl(bsr_index* ix, const float* queries, uint32_t nq, const uint64_t* ids, uint32_t m,
                              uint32_t k, uint64_t* out_idx, float* out_dist, uint32_t* out_count) {
    BSR_TRY(check_score_args(ix, nq, m));
    if (m > BSR_SCORE_MAX_IDS) return set_error(BSR_E_INVALID, "m=%u above BSR_SCORE_MAX_IDS=%u", m, BSR_SCORE_MAX_IDS);
    if (k == 0 || k > m) return set_error(BSR_E_INVALID, "k=%u outside [1, m=%u]", k, m);
    if (nq && !queries) return set_error(BSR_E_INVALID, "null queries");
    if (nq && !ids) return set_error(BSR_E_INVALID, "null ids");
    if (nq && (!out_idx || !out_dist || !out_count)) return set_error(BSR_E_INVALID, "null output");
    BSR_TRY(ix->score_ids_device(queries, nq, ids, m, k, out_idx, out_dist, out_count));
    collect_profile(ix);
    return BSR_OK;
}

// ---------------------------------------------------------------------------------------
// Masked range search (bsr_local_range_search_masked)
// ---------------------------------------------------------------------------------------
// The exact range over row lists for the queries `listed` (ascending ids), every one over the list
// of its own mask (h_grp_qmask, A_g in h_grp_out): run_list_scan_groups' plan with the lists in
// segments, so that a chunk never holds more than the budget's ids and a list longer than that is
// split over chunks -- the counts accumulate through the atomic on rcnt, no merge is needed.  A
// chunk is one scatter launch and, per width qf in {8, 4, 2, 1}, one grouped range scan per 65535
// query groups.  Queries whose mask allows no row are not scanned: their count stays 0.
// BSR_MASK_AUTO for a range, where both paths are possible: a pure function of (n, A_g, nq_g,
// capacity).  Two terms (the measured table, profiles/range_masked_bench.json):
// - the masked top-k's cost rule, auto_prefers_list, unchanged -- a list-scan row against a filter
//   pass; the measured range points on its side of the second term agree with it;
// - the overflow term, the range's own: the filter emits from the whole shard, about 1 / rho rows
//   per allowed row in range, into lists of range_cap(capacity) keys.  A caller whose results about
//   fill their capacity overflows those lists once rho < capacity / range_cap(capacity), and an
//   overflowed query pays the filter pass AND the list scan.  Measured (1M x 768, capacity 256,
//   100 rows in range within the mask): at rho = 1/4 12% of 1000 queries overflow and the filter
//   still wins 4.4 to 28 ms; at 1/16 all do and it loses 7.7 to 6.9 ms, at 1/100 2.3 to 1.3 ms.
//   Hence: the list when rho < capacity / (2 range_cap(capacity)) -- 1/8 up to 512 slots.
// What the rule cannot see is the radius: a small radius under a sparse mask would filter well.
static bool range_auto_prefers_list(uint64_t n, uint64_t A, uint32_t nq, uint32_t capacity) {
    return auto_prefers_list(n, A, nq, 1) || 2 * A * range_cap(capacity) < n * (uint64_t)capacity;
}

static int run_range_list_scan(bsr_index* ix, RangeListArgs la, const uint64_t* allow, uint64_t words,
                               uint32_t n_masks, const std::vector<uint32_t>& listed) {
    const std::vector<uint32_t>& A = ix->h_grp_out;
    const QueriesByMask by = queries_by_mask(ix, n_masks, listed);
    const std::vector<uint32_t>& start = by.start;
    if (by.order.empty()) return BSR_OK;

    struct Chunk { size_t seg0; uint32_t n_segs; std::vector<GroupLaunch> launches; };
    std::vector<Chunk> chunks;
    std::vector<MaskSegDesc>& segs = ix->h_rng_segs;
    std::vector<ScanGroupDesc>& scans = ix->h_grp_scan;
    std::vector<int32_t>& ids = ix->h_grp_ids;
    segs.clear();
    scans.clear();
    ids.clear();
    const uint64_t budget = mask_list_budget_ids();
    uint64_t used = 0, list_ids = 0;
    Chunk cur{0, 0, {}};
    auto close = [&]() {
        if (!cur.n_segs) return;
        // (no partial lists: the counts accumulate on rcnt)
        cur.launches = plan_query_groups(ix, segs.data() + cur.seg0, cur.n_segs, by, 65535, 0);
        list_ids = std::max(list_ids, used);
        chunks.push_back(std::move(cur));
        cur = Chunk{segs.size(), 0, {}};
        used = 0;
    };
    for (uint32_t g = 0; g < n_masks; ++g) {
        if (start[g] == start[g + 1]) continue;
        for (uint32_t pos = 0; pos < A[g];) {
            if (used == budget) close();
            const uint32_t take = (uint32_t)std::min<uint64_t>(A[g] - pos, budget - used);
            segs.push_back(MaskSegDesc{used, g, pos, take, 0});
            ++cur.n_segs;
            used += take;
            pos += take;
        }
    }
    close();

    BSR_TRY(ix->mask_list.ensure((size_t)list_ids * sizeof(uint32_t)));
    BSR_TRY(ix->rng_segs.ensure(segs.size() * sizeof(MaskSegDesc)));
    BSR_TRY(ix->grp_scan.ensure(scans.size() * sizeof(ScanGroupDesc)));
    BSR_TRY(ix->qids.ensure(ids.size() * sizeof(int32_t)));
    BSR_HIP(hipMemcpyAsync(ix->rng_segs.p, segs.data(), segs.size() * sizeof(MaskSegDesc), hipMemcpyHostToDevice,
                           ix->stream));
    BSR_HIP(hipMemcpyAsync(ix->grp_scan.p, scans.data(), scans.size() * sizeof(ScanGroupDesc), hipMemcpyHostToDevice,
                           ix->stream));
    BSR_HIP(hipMemcpyAsync(ix->qids.p, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice, ix->stream));
    la.list = ix->mask_list.as<uint32_t>();
    ev_begin(ix, ix->ev_scan, 1);
    for (const Chunk& c : chunks) {
        // (the stream orders a chunk's scatter behind the scans of the chunk before it)
        BSR_HIP(launch_mask_groups_scatter_seg(allow, words, ix->n, ix->dead_bits(), ix->grp_blk.as<uint32_t>(),
                                               ix->rng_segs.as<MaskSegDesc>() + c.seg0, c.n_segs,
                                               ix->mask_list.as<uint32_t>(), ix->stream));
        for (const GroupLaunch& l : c.launches) {
            la.grp = ix->grp_scan.as<ScanGroupDesc>() + l.scan0;
            la.qids = ix->qids.as<int32_t>() + l.ids0;
            la.groups = l.groups;
            la.qf = l.qf;
            BSR_HIP(launch_range_scan_list_groups(la, l.grid, ix->stream));
        }
    }
    ev_end(ix, ix->ev_scan);
    return BSR_OK;
}

int bsr_index::range_search_device_masked(const float* queries, uint32_t nq, const float* radius, uint32_t capacity,
                                          const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                          const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx,
                                          float* out_dist, uint32_t* out_count) {
    bsr_index* ix = this;
    BSR_TRY(check_batch(ix, 1));
    if (allow_words != (n + 63) / 64)
        return set_error(BSR_E_INVALID, "allow_words=%llu, the index holds %llu rows (%llu words)",
                         (unsigned long long)allow_words, (unsigned long long)n, (unsigned long long)((n + 63) / 64));
    // (host radii: a NaN is refused before any device work, as bsr_local_range_search does)
    const bool radius_dev = is_device_ptr(radius);
    if (!radius_dev)
        for (uint32_t q = 0; q < nq; ++q)
            if (radius[q] != radius[q]) return set_error(BSR_E_INVALID, "radius[%u] is NaN", q);
    BSR_TRY(begin_batch(ix, nq, 1, BSR_PATH_RANGE | (query_mask ? BSR_PATH_MASK_GROUPS : 0u)));
    if (nq == 0) return BSR_OK;

    const uint32_t cap = range_cap(capacity);
    const uint32_t qpad = qpad_for(nq);
    BSR_TRY(query_buffers(ix, nq, qpad, 1));
    BSR_TRY(filter_buffers(ix, nq, qpad, 1, cap));
    stats.n_candidates = 0;
    BSR_TRY(mask_aux.ensure(((size_t)qpad + 1) * sizeof(uint32_t)));
    BSR_TRY(rng_keys.ensure((size_t)nq * cap * sizeof(uint64_t)));
    BSR_TRY(rng_cnt.ensure((size_t)nq * sizeof(uint32_t)));
    BSR_TRY(rng_idx.ensure((size_t)nq * capacity * sizeof(uint64_t)));
    BSR_TRY(rng_dist.ensure((size_t)nq * capacity * sizeof(float)));
    BSR_TRY(rng_out_cnt.ensure((size_t)nq * sizeof(uint32_t)));
    BSR_TRY(rng_route.ensure((size_t)nq * sizeof(uint32_t)));

    ev_begin(ix, ev_total);
    const float* qsrc = nullptr;
    BSR_TRY(stage_queries(ix, queries, nq, &qsrc));
    const float* rsrc = nullptr;
    BSR_TRY(on_device(ix, rng_radius, radius, (size_t)nq * sizeof(float), radius_dev, &rsrc));
    // The masks and the mask ids on the device; the ids on the host too (it forms the query groups).
    const uint64_t* dallow = allow;
    if (allow_words)
        BSR_TRY(on_device(ix, mask_dev, allow, (size_t)n_masks * allow_words * sizeof(uint64_t), is_device_ptr(allow),
                          &dallow));
    const uint32_t* dqmask = query_mask;  // (nullptr: mask 0 for every query, n_masks == 1)
    h_grp_qmask.assign(nq, 0);
    if (query_mask && is_device_ptr(query_mask)) {
        BSR_HIP(hipMemcpyAsync(h_grp_qmask.data(), query_mask, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               stream));
    } else if (query_mask) {
        memcpy(h_grp_qmask.data(), query_mask, (size_t)nq * sizeof(uint32_t));
        BSR_TRY(grp_qmask.ensure((size_t)nq * sizeof(uint32_t)));
        BSR_HIP(hipMemcpyAsync(grp_qmask.p, h_grp_qmask.data(), (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice,
                               stream));
        dqmask = grp_qmask.as<uint32_t>();
    }
    // 1. Every A_g (over allow_g & ~dead) and the check of query_mask: one readback.
    const uint32_t n_blk = mask_blocks(n);
    BSR_TRY(grp_blk.ensure((size_t)n_masks * (n_blk + 1) * sizeof(uint32_t)));
    BSR_TRY(grp_out.ensure(((size_t)n_masks + 1) * sizeof(uint32_t)));
    h_grp_out.assign((size_t)n_masks + 1, 0);
    BSR_HIP(launch_mask_groups_count(dallow, allow_words, n_masks, n, dead_bits(), dqmask, nq, grp_blk.as<uint32_t>(),
                                     grp_out.as<uint32_t>(), stream));
    BSR_HIP(hipMemcpyAsync(h_grp_out.data(), grp_out.p, ((size_t)n_masks + (dqmask ? 1 : 0)) * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, stream));
    BSR_HIP(hipStreamSynchronize(stream));
    if (dqmask && h_grp_out[n_masks])
        return set_error(BSR_E_INVALID, "%u entries of query_mask name no mask (n_masks = %u)", h_grp_out[n_masks],
                         n_masks);

    // 2. The route of every mask group.  The filter is possible where the unmasked range search
    // filters: the threshold comes from the radius alone, so the emitted rows are a superset of the
    // answer under any mask and no A_g is too small for it.  BSR_MASK_AUTO: the masked top-k's rule
    // (k does not enter it) and the range's overflow term, range_auto_prefers_list above.
    const uint64_t live = live_rows();
    const bool can_filter = live > 0 && approx_ok && n > cap;
    std::vector<uint32_t> nq_g(n_masks, 0);
    std::vector<uint8_t> list_g(n_masks, 1);
    for (uint32_t q = 0; q < nq; ++q) ++nq_g[h_grp_qmask[q]];
    bool any_filter = false, any_list = false;
    for (uint32_t g = 0; g < n_masks; ++g) {
        if (!nq_g[g]) continue;
        list_g[g] = !can_filter || mode == BSR_MASK_LIST ||
                    (mode == BSR_MASK_AUTO && range_auto_prefers_list(n, h_grp_out[g], nq_g[g], capacity));
        any_filter |= !list_g[g];
        any_list |= list_g[g] != 0;
    }
    h_rng_route.resize(nq);
    for (uint32_t q = 0; q < nq; ++q) h_rng_route[q] = list_g[h_grp_qmask[q]];
    if (any_list)
        BSR_HIP(hipMemcpyAsync(rng_route.p, h_rng_route.data(), (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice,
                               stream));

    // 3. The queries and the thresholds (in every mode: the zeroed counts, the device check of the
    // radii); 4. the list-by-design queries: tau = +inf, on the scan list once.
    BSR_HIP(launch_query_prep(query_prep_args(ix, qsrc, nq, qpad, any_filter), stream));
    BSR_HIP(launch_range_tau(rsrc, ebound.as<float>(), nb.as<float>(), qflags.as<uint32_t>(), nq, qpad,
                             tau.as<float>(), cnt.as<uint32_t>(), rng_cnt.as<uint32_t>(), fail.as<uint32_t>(), d_status,
                             stream));
    if (any_list)
        BSR_HIP(launch_range_route(rng_route.as<uint32_t>(), rsrc, nq, tau.as<float>(), fail.as<uint32_t>(), d_status,
                                   stream));
    if (any_filter) {
        // 5. the emit pass over every tile, the emitted lists cut by each query's mask (less the
        // tombstones; an overflowed list stays overflowed), the survivors rescored against the radius
        stats.search_path |= BSR_PATH_MASK_FILTER;
        smp_tiles = 0;
        BSR_TRY(emit_pass(ix, nq, qpad, 1, cap));
        uint32_t* raw_cnt = mask_aux.as<uint32_t>();
        BSR_HIP(launch_mask_cut(cand.as<uint64_t>(), cnt.as<uint32_t>(), cap, nq, dallow, allow_words, dqmask,
                                dead_bits(), n, raw_cnt, raw_cnt + qpad, stream));
        RangeArgs ra{};
        ra.rows = rows.as<float>();
        ra.ld = ld;
        ra.dim = dim;
        ra.n = n;
        ra.na = na.as<float>();
        ra.qf32 = qf32.as<float>();
        ra.nb = nb.as<float>();
        ra.radius = rsrc;
        ra.dead = dead_bits();
        ra.keys = rng_keys.as<uint64_t>();
        ra.rcnt = rng_cnt.as<uint32_t>();
        ra.cap = cap;
        ra.nq = nq;
        ra.cand = cand.as<uint64_t>();
        ra.cnt = cnt.as<uint32_t>();
        ra.scan_list = fail.as<uint32_t>();
        ra.status = d_status;
        ra.emit_cnt = raw_cnt;
        ev_begin(ix, ev_rescore);
        BSR_HIP(launch_range_rescore(ra, stream));
        ev_end(ix, ev_rescore);
    }
    // 6. The one status readback: the query flags (a non-finite query, a NaN radius) and the
    // number of queries on the scan list.
    BSR_HIP(hipMemcpyAsync(h_res, d_status, kStWords * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    BSR_HIP(stream_wait(stream));
    BSR_TRY(check_queries(ix, nq));
    const uint32_t* st = reinterpret_cast<const uint32_t*>(h_res);
    if (st[kStQueryFlags] & kRangeNanRadius) return set_error(BSR_E_INVALID, "a radius of the batch is NaN");
    const uint32_t nscan = st[kStFail], ndirect = st[kStFail2];
    stats.n_emitted = any_filter ? st[kStEmitted] : 0;
    stats.n_exact_direct = ndirect;
    stats.n_fallback = nscan - ndirect;
    if (nscan) {
        // 7. / 8. the row lists of the masks of the queries on the scan list, and the range over them
        stats.search_path |= BSR_PATH_MASK_LIST;
        h_fail.resize(nscan);
        BSR_HIP(hipMemcpy(h_fail.data(), fail.p, (size_t)nscan * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::sort(h_fail.begin(), h_fail.end());
        RangeListArgs la{};
        la.rows = rows.as<float>();
        la.ld = ld;
        la.dim = dim;
        la.na = na.as<float>();
        la.qf32 = qf32.as<float>();
        la.nb = nb.as<float>();
        la.radius = rsrc;
        la.keys = rng_keys.as<uint64_t>();
        la.rcnt = rng_cnt.as<uint32_t>();
        la.cap = cap;
        BSR_TRY(run_range_list_scan(ix, la, dallow, allow_words, n_masks, h_fail));
    }
    // The lists sorted into result rows: straight into the caller's arrays when all three are on
    // the device, else into the index's own and copied out.
    const bool out_dev = is_device_ptr(out_idx) && is_device_ptr(out_dist) && is_device_ptr(out_count);
    uint64_t* di = out_dev ? out_idx : rng_idx.as<uint64_t>();
    float* dd = out_dev ? out_dist : rng_dist.as<float>();
    uint32_t* dc = out_dev ? out_count : rng_out_cnt.as<uint32_t>();
    BSR_HIP(launch_range_finish(rng_keys.as<uint64_t>(), rng_cnt.as<uint32_t>(), cap, nq, capacity, global_offset, di,
                                dd, dc, stream));
    ev_end(ix, ev_total);
    if (!out_dev) {
        const size_t nk = (size_t)nq * capacity;
        BSR_HIP(hipMemcpyAsync(out_idx, di, nk * sizeof(uint64_t), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_dist, dd, nk * sizeof(float), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_count, dc, (size_t)nq * sizeof(uint32_t), hipMemcpyDefault, stream));
    }
    BSR_HIP(hipStreamSynchronize(stream));
    return BSR_OK;
}

int bsr_local_range_search_masked_impl(bsr_index* ix, const float* queries, uint32_t nq, const float* radius,
                                       uint32_t capacity, const uint64_t* allow, uint64_t allow_words,
                                       uint32_t n_masks, const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx,
                                       float* out_dist, uint32_t* out_count) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    if (capacity == 0 || capacity > BSR_RANGE_MAX_RESULTS)
        return set_error(BSR_E_INVALID, "capacity=%u outside [1, %u]", capacity, BSR_RANGE_MAX_RESULTS);
    if (n_masks == 0) return set_error(BSR_E_INVALID, "n_masks = 0 (bsr_local_range_search searches without a mask)");
    if (mode != BSR_MASK_AUTO && mode != BSR_MASK_LIST && mode != BSR_MASK_FILTER)
        return set_error(BSR_E_INVALID, "unknown mask mode %u", mode);
    if (nq && !radius) return set_error(BSR_E_INVALID, "null radius");
    if (nq && !queries) return set_error(BSR_E_INVALID, "null queries");
    if (nq && (!out_idx || !out_dist || !out_count)) return set_error(BSR_E_INVALID, "null output");
    if (nq && !allow) return set_error(BSR_E_INVALID, "null allow masks");
    if (!query_mask && n_masks > 1)
        return set_error(BSR_E_INVALID, "null query_mask with n_masks = %u (legal only with one mask)", n_masks);
    BSR_TRY(ix->range_search_device_masked(queries, nq, radius, capacity, allow, allow_words, n_masks, query_mask, mode,
                                           out_idx, out_dist, out_count));
    collect_profile(ix);
    return BSR_OK;
}

// ---------------------------------------------------------------------------------------
// MMR search (bsr_local_top_k_mmr)
// ---------------------------------------------------------------------------------------
int bsr_index::mmr_search_device(const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k, float lambda,
                                 const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                 const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx, float* out_dist,
                                 uint32_t* out_rank, uint32_t* out_count) {
    BSR_HIP(hipSetDevice(device));
    // The stage's own result rows first: an allocation after the candidate search would fall
    // between the capture of its graph and the replay (the key carries the allocation generation).
    const size_t nk = (size_t)nq * k;
    BSR_TRY(mmr_idx.ensure(nk * sizeof(uint64_t)));
    BSR_TRY(mmr_dist.ensure(nk * sizeof(float)));
    BSR_TRY(mmr_rank.ensure(nk * sizeof(uint32_t)));
    BSR_TRY(mmr_cnt.ensure((size_t)nq * sizeof(uint32_t)));
    // The candidates: the search itself with k = fetch_k, run to completion -- the exact rounds of
    // its uncertified queries and the thresholded rerun come after its host wait, so its lists are
    // final in d_idx / d_dist / d_cnt only once it returns.
    if (!allow) BSR_TRY(search_device(queries, nq, fetch_k));
    else if (n_masks == 1 && !query_mask) BSR_TRY(search_device_masked(queries, nq, fetch_k, allow, allow_words, mode));
    else BSR_TRY(search_device_masked_groups(queries, nq, fetch_k, allow, allow_words, n_masks, query_mask, mode));
    stats.search_path |= BSR_PATH_MMR;
    // The selection, launched directly (never captured; the packed result's status words are not
    // its business): straight into the caller's arrays when they are all on the device, else into
    // the index's own and copied out.
    const bool out_dev = is_device_ptr(out_idx) && is_device_ptr(out_dist) && is_device_ptr(out_count) &&
                         (!out_rank || is_device_ptr(out_rank));
    MmrArgs ma{};
    ma.rows = rows.as<float>();
    ma.ld = ld;
    ma.dim = dim;
    ma.n = n;
    ma.offset = global_offset;
    ma.na = na.as<float>();
    ma.cand_idx = d_idx;
    ma.cand_dist = d_dist;
    ma.cand_cnt = d_cnt;
    ma.nq = nq;
    ma.fetch_k = fetch_k;
    ma.k = k;
    ma.lambda = lambda;
    ma.out_idx = out_dev ? out_idx : mmr_idx.as<uint64_t>();
    ma.out_dist = out_dev ? out_dist : mmr_dist.as<float>();
    ma.out_rank = out_dev ? out_rank : mmr_rank.as<uint32_t>();
    ma.out_count = out_dev ? out_count : mmr_cnt.as<uint32_t>();
    BSR_HIP(launch_mmr_select(ma, stream));
    if (!out_dev) {
        BSR_HIP(hipMemcpyAsync(out_idx, ma.out_idx, nk * sizeof(uint64_t), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_dist, ma.out_dist, nk * sizeof(float), hipMemcpyDefault, stream));
        if (out_rank) BSR_HIP(hipMemcpyAsync(out_rank, ma.out_rank, nk * sizeof(uint32_t), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_count, ma.out_count, (size_t)nq * sizeof(uint32_t), hipMemcpyDefault, stream));
    }
    BSR_HIP(hipStreamSynchronize(stream));
    return BSR_OK;
}

int bsr_local_top_k_mmr_impl(bsr_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k,
                             float lambda, const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                             const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx, float* out_dist,
                             uint32_t* out_rank, uint32_t* out_count) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    if (k == 0 || k > fetch_k || fetch_k > ix->cfg.max_k)
        return set_error(BSR_E_INVALID, "k=%u, fetch_k=%u outside 1 <= k <= fetch_k <= max_k=%u", k, fetch_k,
                         ix->cfg.max_k);
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return set_error(BSR_E_INVALID, "lambda=%g outside [0, 1]", (double)lambda);
    if (!allow && (n_masks != 0 || query_mask))
        return set_error(BSR_E_INVALID, "n_masks = %u or a query_mask without allow masks", n_masks);
    if (allow && n_masks == 0) return set_error(BSR_E_INVALID, "n_masks = 0 with allow masks");
    if (allow && !query_mask && n_masks > 1)
        return set_error(BSR_E_INVALID, "null query_mask with n_masks = %u (legal only with one mask)", n_masks);
    if (mode != BSR_MASK_AUTO && mode != BSR_MASK_LIST && mode != BSR_MASK_FILTER)
        return set_error(BSR_E_INVALID, "unknown mask mode %u", mode);
    if (nq && !queries) return set_error(BSR_E_INVALID, "null queries");
    if (nq && (!out_idx || !out_dist || !out_count)) return set_error(BSR_E_INVALID, "null output");
    if (!ix->loaded) return set_error(BSR_E_STATE, "index not loaded");
    if (nq == 0) return BSR_OK;
    BSR_TRY(ix->mmr_search_device(queries, nq, k, fetch_k, lambda, allow, allow_words, n_masks, query_mask, mode,
                                  out_idx, out_dist, out_rank, out_count));
    collect_profile(ix);
    return BSR_OK;
}

// ---------------------------------------------------------------------------------------
// Collapsed search (bsr_local_top_k_collapsed) and capped search
// (bsr_local_top_k_capped): one host sequence.  per_group = 0 is the collapsed search
// with its own walk and scan kernels; per_group >= 1 the capped search, whose walk counts up to
// m_eff = min(per_group, k) rows of a group and whose tables hold m_eff entries per (query, group).
// ---------------------------------------------------------------------------------------
int bsr_index::collapsed_search_device(const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k,
                                       const uint32_t* row_group, uint32_t n_groups, const uint64_t* allow,
                                       uint64_t allow_words, uint32_t n_masks, const uint32_t* query_mask,
                                       uint32_t mode, uint64_t* out_idx, float* out_dist, uint32_t* out_group,
                                       uint32_t* out_count) {
    return group_search_device(queries, nq, k, fetch_k, 0, row_group, n_groups, allow, allow_words, n_masks,
                               query_mask, mode, out_idx, out_dist, out_group, out_count);
}

int bsr_index::capped_search_device(const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k,
                                    uint32_t per_group, const uint32_t* row_group, uint32_t n_groups,
                                    const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                    const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx, float* out_dist,
                                    uint32_t* out_group, uint32_t* out_count) {
    return group_search_device(queries, nq, k, fetch_k, per_group, row_group, n_groups, allow, allow_words, n_masks,
                               query_mask, mode, out_idx, out_dist, out_group, out_count);
}

static_assert(kCapMaxPerGroup == BSR_CAP_MAX_PER_GROUP, "the capped scan's limit is the ABI's");

int bsr_index::group_search_device(const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k,
                                   uint32_t per_group, const uint32_t* row_group, uint32_t n_groups,
                                   const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                   const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx, float* out_dist,
                                   uint32_t* out_group, uint32_t* out_count) {
    bsr_index* ix = this;
    const bool capped = per_group != 0;
    // (table entries per (query, group); m_eff * n_groups fits 32 bits, the entry point checked it)
    const uint32_t m_eff = capped ? std::min(per_group, k) : 1;
    const uint32_t n_entries = m_eff * n_groups;
    BSR_HIP(hipSetDevice(device));
    // Every buffer of the stage but the scan's tables first: an allocation after the candidate
    // search would fall between the capture of its graph and the replay (the key carries the
    // allocation generation), as mmr_search_device has it.
    const size_t nk = (size_t)nq * k;
    const uint32_t sel_grid = collapse_select_grid(n_entries);
    BSR_TRY(col_flag.ensure(2 * sizeof(uint32_t)));
    BSR_TRY(col_fail.ensure((size_t)nq * sizeof(uint32_t)));
    BSR_TRY(col_qids.ensure((size_t)nq * kScanQF * sizeof(int32_t)));
    BSR_TRY(col_keys.ensure(nk * sizeof(uint64_t)));
    BSR_TRY(col_idx.ensure(nk * sizeof(uint64_t)));
    BSR_TRY(col_dist.ensure(nk * sizeof(float)));
    BSR_TRY(col_group.ensure(nk * sizeof(uint32_t)));
    BSR_TRY(col_cnt.ensure((size_t)nq * sizeof(uint32_t)));
    BSR_TRY(part.ensure((size_t)sel_grid * kScanQF * k * sizeof(uint64_t)));
    // The groups on the device and their check, before anything indexes a table with one.
    uint32_t* const flag = col_flag.as<uint32_t>();  // [0]: a group id out of range; [1]: the fail list's count
    BSR_HIP(hipMemsetAsync(flag, 0, 2 * sizeof(uint32_t), stream));
    const uint32_t* dgrp = nullptr;
    if (n) {
        BSR_TRY(on_device(ix, col_grp, row_group, (size_t)n * sizeof(uint32_t), is_device_ptr(row_group), &dgrp));
        BSR_HIP(launch_group_check(dgrp, n, n_groups, flag, stream));
        uint32_t bad = 0;
        BSR_HIP(hipMemcpyAsync(&bad, flag, sizeof bad, hipMemcpyDeviceToHost, stream));
        BSR_HIP(hipStreamSynchronize(stream));
        if (bad) return set_error(BSR_E_INVALID, "a row_group entry is >= n_groups = %u", n_groups);
    }
    // The candidates: the search itself with k = fetch_k, run to completion (mmr_search_device).
    if (!allow) BSR_TRY(search_device(queries, nq, fetch_k));
    else if (n_masks == 1 && !query_mask) BSR_TRY(search_device_masked(queries, nq, fetch_k, allow, allow_words, mode));
    else BSR_TRY(search_device_masked_groups(queries, nq, fetch_k, allow, allow_words, n_masks, query_mask, mode));
    stats.search_path |= capped ? BSR_PATH_CAP : BSR_PATH_COLLAPSE;
    // The walk, straight into the caller's arrays when they are all on the device, else into the
    // index's own, copied out at the end.
    const bool out_dev = is_device_ptr(out_idx) && is_device_ptr(out_dist) && is_device_ptr(out_count) &&
                         (!out_group || is_device_ptr(out_group));
    CollapseWalkArgs wa{};
    wa.cand_idx = d_idx;
    wa.cand_dist = d_dist;
    wa.cand_cnt = d_cnt;
    wa.nq = nq;
    wa.fetch_k = fetch_k;
    wa.k = k;
    wa.n = n;
    wa.offset = global_offset;
    wa.row_group = dgrp;
    wa.out_idx = out_dev ? out_idx : col_idx.as<uint64_t>();
    wa.out_dist = out_dev ? out_dist : col_dist.as<float>();
    wa.out_group = out_dev ? out_group : col_group.as<uint32_t>();
    wa.out_count = out_dev ? out_count : col_cnt.as<uint32_t>();
    wa.fail = col_fail.as<uint32_t>();
    wa.fail_cnt = flag + 1;
    if (capped) BSR_HIP(launch_cap_walk(CapWalkArgs{wa, m_eff}, stream));
    else BSR_HIP(launch_collapse_walk(wa, stream));
    uint32_t nfail = 0;
    BSR_HIP(hipMemcpyAsync(&nfail, flag + 1, sizeof nfail, hipMemcpyDeviceToHost, stream));
    BSR_HIP(hipStreamSynchronize(stream));
    if (nfail) {
        // The queries whose full list held fewer than k groups (kept rows): the group scan, in rounds
        // of as many queries as the table budget holds.
        stats.search_path |= capped ? BSR_PATH_CAP_SCAN : BSR_PATH_COLLAPSE_SCAN;
        h_fail.resize(nfail);
        BSR_HIP(hipMemcpy(h_fail.data(), col_fail.p, (size_t)nfail * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::sort(h_fail.begin(), h_fail.end());
        const uint64_t table = 8ull * n_entries;
        const uint64_t budget = env_bytes("BSR_COLLAPSE_TABLE_BUDGET", 256ull << 20);
        const uint32_t per = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({kScanQF, budget / table, nfail}));
        const uint32_t rounds = (nfail + per - 1) / per;
        const std::vector<int32_t> padded = padded_scan_ids(h_fail, nfail, per);
        // (the one allocation behind the candidate search: the plain search re-captures once)
        BSR_TRY(col_best.ensure((size_t)per * table));
        BSR_HIP(hipMemcpyAsync(col_qids.p, padded.data(), padded.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                               stream));
        BSR_HIP(hipStreamSynchronize(stream));  // (padded is read by the copy)
        CollapseScanArgs sa{};
        sa.rows = rows.as<float>();
        sa.ld = ld;
        sa.dim = dim;
        sa.n = n;
        sa.na = na.as<float>();
        sa.qf32 = qf32.as<float>();
        sa.nb = nb.as<float>();
        sa.dead = dead_bits();
        sa.row_group = dgrp;
        sa.n_groups = n_groups;
        // (the masks where the candidate search read them: the caller's device arrays or its copies)
        sa.allow = !allow ? nullptr : is_device_ptr(allow) ? allow : mask_dev.as<uint64_t>();
        sa.allow_words = allow_words;
        sa.query_mask = !allow || !query_mask ? nullptr
                        : is_device_ptr(query_mask) ? query_mask : grp_qmask.as<uint32_t>();
        sa.best = col_best.as<uint64_t>();
        const uint32_t grid = scan_grid_for(n);
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t nr = std::min(per, nfail - r * per);
            const int32_t* qid = col_qids.as<int32_t>() + (size_t)r * kScanQF;
            sa.qids = qid;
            sa.nqf = nr;
            BSR_HIP(hipMemsetAsync(col_best.p, 0xff, (size_t)nr * table, stream));
            if (capped) BSR_HIP(launch_cap_scan(CapScanArgs{sa, m_eff}, grid, stream));
            else BSR_HIP(launch_collapse_scan(sa, grid, stream));
            BSR_HIP(launch_collapse_select(sa.best, n_entries, nr, k, sel_grid, part.as<uint64_t>(), stream));
            BSR_HIP(launch_merge_parts(part.as<uint64_t>(), sel_grid, qid, nr, k, col_keys.as<uint64_t>(), stream));
            BSR_HIP(launch_collapse_finish(col_keys.as<uint64_t>(), qid, nr, k, global_offset, dgrp, wa.out_idx,
                                           wa.out_dist, wa.out_group, wa.out_count, stream));
        }
    }
    if (!out_dev) {
        BSR_HIP(hipMemcpyAsync(out_idx, wa.out_idx, nk * sizeof(uint64_t), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_dist, wa.out_dist, nk * sizeof(float), hipMemcpyDefault, stream));
        if (out_group) BSR_HIP(hipMemcpyAsync(out_group, wa.out_group, nk * sizeof(uint32_t), hipMemcpyDefault, stream));
        BSR_HIP(hipMemcpyAsync(out_count, wa.out_count, (size_t)nq * sizeof(uint32_t), hipMemcpyDefault, stream));
    }
    BSR_HIP(hipStreamSynchronize(stream));
    return BSR_OK;
}

int bsr_local_top_k_collapsed_impl(bsr_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k,
                                   const uint32_t* row_group, uint64_t row_group_len, uint32_t n_groups,
                                   const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                   const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx, float* out_dist,
                                   uint32_t* out_group, uint32_t* out_count) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    if (k == 0 || k > fetch_k || fetch_k > ix->cfg.max_k)
        return set_error(BSR_E_INVALID, "k=%u, fetch_k=%u outside 1 <= k <= fetch_k <= max_k=%u", k, fetch_k,
                         ix->cfg.max_k);
    if (n_groups == 0) return set_error(BSR_E_INVALID, "n_groups = 0");
    if (!allow && (n_masks != 0 || query_mask))
        return set_error(BSR_E_INVALID, "n_masks = %u or a query_mask without allow masks", n_masks);
    if (allow && n_masks == 0) return set_error(BSR_E_INVALID, "n_masks = 0 with allow masks");
    if (allow && !query_mask && n_masks > 1)
        return set_error(BSR_E_INVALID, "null query_mask with n_masks = %u (legal only with one mask)", n_masks);
    if (mode != BSR_MASK_AUTO && mode != BSR_MASK_LIST && mode != BSR_MASK_FILTER)
        return set_error(BSR_E_INVALID, "unknown mask mode %u", mode);
    if (nq && !queries) return set_error(BSR_E_INVALID, "null queries");
    if (nq && (!out_idx || !out_dist || !out_count)) return set_error(BSR_E_INVALID, "null output");
    if (!ix->loaded) return set_error(BSR_E_STATE, "index not loaded");
    if (row_group_len != ix->n)
        return set_error(BSR_E_INVALID, "row_group_len=%llu, the index holds %llu rows", (unsigned long long)row_group_len,
                         (unsigned long long)ix->n);
    if (ix->n && !row_group) return set_error(BSR_E_INVALID, "null row_group");
    if (nq == 0) return BSR_OK;
    BSR_TRY(ix->collapsed_search_device(queries, nq, k, fetch_k, row_group, n_groups, allow, allow_words, n_masks,
                                        query_mask, mode, out_idx, out_dist, out_group, out_count));
    collect_profile(ix);
    return BSR_OK;
}

int bsr_local_top_k_capped_impl(bsr_index* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t fetch_k,
                                uint32_t per_group, const uint32_t* row_group, uint64_t row_group_len,
                                uint32_t n_groups, const uint64_t* allow, uint64_t allow_words, uint32_t n_masks,
                                const uint32_t* query_mask, uint32_t mode, uint64_t* out_idx, float* out_dist,
                                uint32_t* out_group, uint32_t* out_count) {
    if (!ix) return set_error(BSR_E_INVALID, "null index");
    if (k == 0 || k > fetch_k || fetch_k > ix->cfg.max_k)
        return set_error(BSR_E_INVALID, "k=%u, fetch_k=%u outside 1 <= k <= fetch_k <= max_k=%u", k, fetch_k,
                         ix->cfg.max_k);
    if (per_group == 0 || per_group > BSR_CAP_MAX_PER_GROUP)
        return set_error(BSR_E_INVALID, "per_group=%u outside 1 <= per_group <= %u", per_group, BSR_CAP_MAX_PER_GROUP);
    if (n_groups == 0) return set_error(BSR_E_INVALID, "n_groups = 0");
    // (the tables' entries per query go through the selection's 32-bit length)
    if ((uint64_t)std::min(per_group, k) * n_groups > 0xFFFFFFFFull)
        return set_error(BSR_E_INVALID, "min(per_group, k) * n_groups = %u * %u exceeds 2^32 - 1", std::min(per_group, k),
                         n_groups);
    if (!allow && (n_masks != 0 || query_mask))
        return set_error(BSR_E_INVALID, "n_masks = %u or a query_mask without allow masks", n_masks);
    if (allow && n_masks == 0) return set_error(BSR_E_INVALID, "n_masks = 0 with allow masks");
    if (allow && !query_mask && n_masks > 1)
        return set_error(BSR_E_INVALID, "null query_mask with n_masks = %u (legal only with one mask)", n_masks);
    if (mode != BSR_MASK_AUTO && mode != BSR_MASK_LIST && mode != BSR_MASK_FILTER)
        return set_error(BSR_E_INVALID, "unknown mask mode %u", mode);
    if (nq && !queries) return set_error(BSR_E_INVALID, "null queries");
    if (nq && (!out_idx || !out_dist || !out_count)) return set_error(BSR_E_INVALID, "null output");
    if (!ix->loaded) return set_error(BSR_E_STATE, "index not loaded");
    if (row_group_len != ix->n)
        return set_error(BSR_E_INVALID, "row_group_len=%llu, the index holds %llu rows", (unsigned long long)row_group_len,
                         (unsigned long long)ix->n);
    if (ix->n && !row_group) return set_error(BSR_E_INVALID, "null row_group");
    if (nq == 0) return BSR_OK;
    BSR_TRY(ix->capped_search_device(queries, nq, k, fetch_k, per_group, row_group, n_groups, allow, allow_words,
                                     n_masks, query_mask, mode, out_idx, out_dist, out_group, out_count));
    collect_profile(ix);
    return BSR_OK;
}

int bsr_index_collect_profile_impl(bsr_index* ix) {
    collect_profile(ix);
    return BSR_OK;
}
