// kcheck_cap.cpp -- test-only shim over the launchers of the capped search (csrc/k_exact.hip:
// launch_cap_walk, and launch_cap_scan + launch_collapse_select + launch_merge_parts +
// launch_collapse_finish as one round of the capped group scan), with launch_collapse_walk and
// launch_collapse_scan over the same structs for the per_group = 1 comparisons.
//
// Built to lib/libbsr_kcheck_cap.so and linked against libbsr.so; not part of the ABI.  The
// conventions are kcheck_collapse.cpp's: host pointers and plain scalars in, device buffers of
// exactly the sizes given (a null pointer or 0 bytes: a null device pointer), the null stream, a
// synchronise, the written buffers copied back, the hipError_t returned as an int.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kernels.hpp"

namespace {

struct Bufs {
    struct B { void* d; void* h; size_t bytes; };  // h: where to copy back (nullptr: an input)
    std::vector<B> v;
    hipError_t err = hipSuccess;

    void* put(const void* h, void* back, size_t bytes) {
        if (err != hipSuccess || !h || !bytes) return nullptr;
        void* d = nullptr;
        err = hipMalloc(&d, bytes);
        if (err != hipSuccess) return nullptr;
        v.push_back({d, back, bytes});
        err = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
        return d;
    }
    template <class T>
    const T* in(const T* h, size_t bytes) { return static_cast<const T*>(put(h, nullptr, bytes)); }
    template <class T>
    T* io(T* h, size_t bytes) { return static_cast<T*>(put(h, h, bytes)); }
    int finish(hipError_t launch) {
        if (err == hipSuccess) err = launch;
        if (err == hipSuccess) err = hipDeviceSynchronize();
        for (auto& b : v) {
            if (err == hipSuccess && b.h) err = hipMemcpy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost);
            (void)hipFree(b.d);
        }
        v.clear();
        return (int)err;
    }
};

}  // namespace

extern "C" {

uint32_t kc_cap_max_fetch(void) { return bsr::kCollapseMaxFetch; }
uint32_t kc_cap_scan_qf(void) { return bsr::kScanQF; }
uint32_t kc_cap_max_per_group(void) { return bsr::kCapMaxPerGroup; }
uint32_t kc_cap_select_grid(uint32_t n_entries) { return bsr::collapse_select_grid(n_entries); }
uint32_t kc_cap_scan_grid(uint64_t n) { return bsr::scan_grid_for(n); }

// CapWalkArgs, flat, with the byte size of every buffer (the outputs, fail and fail_cnt in/out).
// collapse != 0: launch_collapse_walk on the same arguments (per_group unused).
struct KcCapWalk {
    const uint64_t* cand_idx; uint64_t cand_idx_bytes;
    const float* cand_dist; uint64_t cand_dist_bytes;
    const uint32_t* cand_cnt; uint64_t cand_cnt_bytes;
    uint32_t nq, fetch_k, k, per_group;
    uint64_t n, offset;
    const uint32_t* row_group; uint64_t row_group_bytes;
    uint64_t* out_idx; uint64_t out_idx_bytes;
    float* out_dist; uint64_t out_dist_bytes;
    uint32_t* out_group; uint64_t out_group_bytes;
    uint32_t* out_count; uint64_t out_count_bytes;
    uint32_t* fail; uint64_t fail_bytes;
    uint32_t* fail_cnt; uint64_t fail_cnt_bytes;
};

int kc_cap_walk(const KcCapWalk* h, uint32_t collapse) {
    Bufs b;
    bsr::CapWalkArgs c{};
    bsr::CollapseWalkArgs& a = c.w;
    a.cand_idx = b.in(h->cand_idx, h->cand_idx_bytes);
    a.cand_dist = b.in(h->cand_dist, h->cand_dist_bytes);
    a.cand_cnt = b.in(h->cand_cnt, h->cand_cnt_bytes);
    a.nq = h->nq;
    a.fetch_k = h->fetch_k;
    a.k = h->k;
    c.per_group = h->per_group;
    a.n = h->n;
    a.offset = h->offset;
    a.row_group = b.in(h->row_group, h->row_group_bytes);
    a.out_idx = b.io(h->out_idx, h->out_idx_bytes);
    a.out_dist = b.io(h->out_dist, h->out_dist_bytes);
    a.out_group = b.io(h->out_group, h->out_group_bytes);
    a.out_count = b.io(h->out_count, h->out_count_bytes);
    a.fail = b.io(h->fail, h->fail_bytes);
    a.fail_cnt = b.io(h->fail_cnt, h->fail_cnt_bytes);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(collapse ? bsr::launch_collapse_walk(a, nullptr) : bsr::launch_cap_walk(c, nullptr));
}

// One round of the capped group scan as the host runs it: the tables (best, in/out: all-ones from
// the caller, [nqf][n_groups][m]), the scan, the selection over m * n_groups entries into part
// (in/out), launch_merge_parts into keys (in/out, [.][k] indexed by query id), the finish into the
// outputs (in/out, indexed by query id).  collapse != 0: launch_collapse_scan in the scan's place
// (m must be 1).
struct KcCapScan {
    const float* rows; uint64_t rows_bytes; uint32_t ld, dim; uint64_t n, offset;
    const float* na; uint64_t na_bytes;
    const float* qf32; uint64_t qf32_bytes;
    const float* nb; uint64_t nb_bytes;
    const uint64_t* dead; uint64_t dead_bytes;
    const uint32_t* row_group; uint64_t row_group_bytes;
    uint32_t n_groups, nqf;
    const uint64_t* allow; uint64_t allow_bytes; uint64_t allow_words;
    const uint32_t* query_mask; uint64_t query_mask_bytes;
    const int32_t* qids; uint64_t qids_bytes;
    uint32_t k, grid, sel_grid, m;
    uint64_t* best; uint64_t best_bytes;
    uint64_t* part; uint64_t part_bytes;
    uint64_t* keys; uint64_t keys_bytes;
    uint64_t* out_idx; uint64_t out_idx_bytes;
    float* out_dist; uint64_t out_dist_bytes;
    uint32_t* out_group; uint64_t out_group_bytes;
    uint32_t* out_count; uint64_t out_count_bytes;
};

void kc_cap_sizes(uint32_t* out) {
    out[0] = (uint32_t)sizeof(KcCapWalk);
    out[1] = (uint32_t)sizeof(KcCapScan);
}

int kc_cap_scan(const KcCapScan* h, uint32_t collapse) {
    Bufs b;
    bsr::CapScanArgs c{};
    bsr::CollapseScanArgs& a = c.s;
    a.rows = b.in(h->rows, h->rows_bytes);
    a.ld = h->ld;
    a.dim = h->dim;
    a.n = h->n;
    a.na = b.in(h->na, h->na_bytes);
    a.qf32 = b.in(h->qf32, h->qf32_bytes);
    a.nb = b.in(h->nb, h->nb_bytes);
    a.dead = b.in(h->dead, h->dead_bytes);
    a.row_group = b.in(h->row_group, h->row_group_bytes);
    a.n_groups = h->n_groups;
    a.allow = b.in(h->allow, h->allow_bytes);
    a.allow_words = h->allow_words;
    a.query_mask = b.in(h->query_mask, h->query_mask_bytes);
    a.qids = b.in(h->qids, h->qids_bytes);
    a.nqf = h->nqf;
    c.m = h->m;
    a.best = b.io(h->best, h->best_bytes);
    uint64_t* part = b.io(h->part, h->part_bytes);
    uint64_t* keys = b.io(h->keys, h->keys_bytes);
    uint64_t* oi = b.io(h->out_idx, h->out_idx_bytes);
    float* od = b.io(h->out_dist, h->out_dist_bytes);
    uint32_t* og = b.io(h->out_group, h->out_group_bytes);
    uint32_t* oc = b.io(h->out_count, h->out_count_bytes);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    // (the table of a slot is m * n_groups entries; the bytes given must hold nqf of them)
    const uint64_t n_entries = (uint64_t)h->m * h->n_groups;
    if ((collapse && h->m != 1) || n_entries > 0xFFFFFFFFull || h->best_bytes < (uint64_t)h->nqf * n_entries * 8)
        return b.finish(hipErrorInvalidValue);
    hipError_t e = collapse ? bsr::launch_collapse_scan(a, h->grid, nullptr) : bsr::launch_cap_scan(c, h->grid, nullptr);
    if (e == hipSuccess)
        e = bsr::launch_collapse_select(a.best, (uint32_t)n_entries, a.nqf, h->k, h->sel_grid, part, nullptr);
    if (e == hipSuccess) e = bsr::launch_merge_parts(part, h->sel_grid, a.qids, a.nqf, h->k, keys, nullptr);
    if (e == hipSuccess)
        e = bsr::launch_collapse_finish(keys, a.qids, a.nqf, h->k, h->offset, a.row_group, oi, od, og, oc, nullptr);
    return b.finish(e);
}

}  // extern "C"
