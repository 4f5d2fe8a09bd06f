// kcheck_exact.cpp -- test-only shim over the launchers of the exact stage (csrc/k_exact.hip, and
// launch_row_norms of k_prep.hip, whose output is that stage's input).
//
// Built to lib/libbsr_kcheck_exact.so and linked against libbsr.so; not part of the ABI.  The
// conventions are kcheck.cpp's: host pointers and plain scalars in, device buffers of exactly the
// sizes given (a null pointer or 0 bytes: a null device pointer), the null stream, a synchronise,
// the written buffers copied back (a written buffer is in/out, so a pattern-filled output shows
// which words the kernel wrote), the hipError_t returned as an int.  The buffers a kernel writes
// through to the host (the result mirror, the published copy and its flag) are fine-grained pinned
// allocations, as the product's are, copied in before and out after the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "kernels.hpp"

namespace {

struct Bufs {
    struct B { void* d; void* h; size_t bytes; bool pinned; };  // h: where to copy back (nullptr: an input)
    std::vector<B> v;
    hipError_t err = hipSuccess;

    void* put(const void* h, void* back, size_t bytes) {
        if (err != hipSuccess || !h || !bytes) return nullptr;
        void* d = nullptr;
        err = hipMalloc(&d, bytes);
        if (err != hipSuccess) return nullptr;
        v.push_back({d, back, bytes, false});
        err = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
        return d;
    }
    template <class T>
    const T* in(const T* h, size_t bytes) { return static_cast<const T*>(put(h, nullptr, bytes)); }
    template <class T>
    T* io(T* h, size_t bytes) { return static_cast<T*>(put(h, h, bytes)); }
    // a host-visible buffer the kernel writes: fine-grained pinned memory, preset to the caller's
    // bytes; returns its device address
    template <class T>
    T* host_io(T* h, size_t bytes) {
        if (err != hipSuccess || !h || !bytes) return nullptr;
        void* p = nullptr;
        err = hipHostMalloc(&p, bytes, hipHostMallocCoherent);
        if (err != hipSuccess) return nullptr;
        v.push_back({p, h, bytes, true});
        memcpy(p, h, bytes);
        void* d = nullptr;
        err = hipHostGetDevicePointer(&d, p, 0);
        return static_cast<T*>(d);
    }
    int finish(hipError_t launch) {
        if (err == hipSuccess) err = launch;
        if (err == hipSuccess) err = hipDeviceSynchronize();
        for (auto& b : v) {
            if (b.pinned) {
                if (err == hipSuccess && b.h) memcpy(b.h, b.d, b.bytes);
                (void)hipHostFree(b.d);
            } else {
                if (err == hipSuccess && b.h) err = hipMemcpy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost);
                (void)hipFree(b.d);
            }
        }
        v.clear();
        return (int)err;
    }
};

}  // namespace

extern "C" {

// The exact stage's constants and the candidate stage's sizes for a k.
struct KcExactConsts {
    uint32_t scan_qf, rescore_all_grid, ticket_words, top_keys_per_lane, merge_max_entries, fused_select_cap;
    uint32_t st_words, st_fail, st_emitted, st_query_flags, st_fail2;
    uint32_t row_non_finite, row_norm_ovf, row_norm_range, query_no_approx;
};
void kc_exact_consts(KcExactConsts* c) {
    *c = KcExactConsts{bsr::kScanQF, bsr::kRescoreAllGrid, bsr::kTicketWords, bsr::kTopKeysPerLane,
                       bsr::kMergeMaxEntries, bsr::kFusedSelectCap, (uint32_t)bsr::kStWords, (uint32_t)bsr::kStFail,
                       (uint32_t)bsr::kStEmitted, (uint32_t)bsr::kStQueryFlags, (uint32_t)bsr::kStFail2,
                       bsr::kRowNonFinite, bsr::kRowNormOvf, bsr::kRowNormRange, bsr::kQueryNoApprox};
}
uint32_t kc_kp_for(uint32_t k) { return bsr::kp_for(k); }
uint32_t kc_cap_for(uint32_t k) { return bsr::cap_for(k); }
uint32_t kc_ks_for(uint32_t k) { return bsr::ks_for(k); }
uint32_t kc_scan_grid_for(uint64_t n) { return bsr::scan_grid_for(n); }

// RescoreArgs, flat, with the byte size of every buffer.  n_items_dev: a host pointer to the one
// device word.  cand_keys is in/out (the self-thresholded selection rewrites the lists' fronts).
// pub_alias != 0: pub_src is the res_idx device buffer (what the kernel left there); else the
// caller's own pub_src bytes.
struct KcRescore {
    const float* rows; uint64_t rows_bytes; uint32_t ld, dim;
    const float* na; uint64_t na_bytes;
    const float* qf32; uint64_t qf32_bytes;
    const float* nb; uint64_t nb_bytes;
    uint32_t n_items, kp;
    const uint32_t* n_items_dev;
    const uint32_t* qlist; uint64_t qlist_bytes;
    const uint32_t* cand_rows; uint64_t cand_rows_bytes;
    const uint32_t* ncand; uint64_t ncand_bytes;
    const float* tau_excl; uint64_t tau_excl_bytes;
    uint64_t* cand_keys; uint64_t cand_keys_bytes;
    const uint32_t* cnt; uint64_t cnt_bytes;
    const float* tau0; uint64_t tau0_bytes;
    uint32_t cap, sel, top_w, k;
    const uint32_t* qflags; uint64_t qflags_bytes;
    float* top_tau; uint64_t top_tau_bytes;
    uint32_t* top_cnt; uint64_t top_cnt_bytes;
    const float* ebound; uint64_t ebound_bytes;
    uint64_t* out_keys; uint64_t out_keys_bytes;
    uint32_t* fail_cnt; uint64_t fail_cnt_bytes;
    uint32_t* fail_list; uint64_t fail_list_bytes;
    uint64_t* res_idx; uint64_t res_idx_bytes;
    float* res_dist; uint64_t res_dist_bytes;
    uint32_t* res_cnt; uint64_t res_cnt_bytes;
    uint64_t offset, n_rows;
    const uint64_t* dead; uint64_t dead_bytes;
    uint64_t* hres_idx; uint64_t hres_idx_bytes;
    float* hres_dist; uint64_t hres_dist_bytes;
    uint32_t* hres_cnt; uint64_t hres_cnt_bytes;
    uint32_t* next_status; uint64_t next_status_bytes;
    const uint32_t* emit_cnt; uint64_t emit_cnt_bytes;
    uint32_t* cur_status; uint64_t cur_status_bytes;
    uint32_t n_queries, pub_alias;
    float* excl_out; uint64_t excl_out_bytes;
    uint32_t* merge_words; uint64_t merge_words_bytes;
    const uint8_t* pub_src; uint64_t pub_src_bytes;
    uint8_t* pub_dst; uint64_t pub_bytes;
    uint32_t* pub_flag;
    uint32_t* pub_ticket;
};

int kc_rescore(const KcRescore* h) {
    Bufs b;
    bsr::RescoreArgs a{};
    a.rows = b.in(h->rows, h->rows_bytes);
    a.ld = h->ld;
    a.dim = h->dim;
    a.na = b.in(h->na, h->na_bytes);
    a.qf32 = b.in(h->qf32, h->qf32_bytes);
    a.nb = b.in(h->nb, h->nb_bytes);
    a.n_items = h->n_items;
    a.n_items_dev = b.in(h->n_items_dev, sizeof(uint32_t));
    a.qlist = b.in(h->qlist, h->qlist_bytes);
    a.cand_rows = b.in(h->cand_rows, h->cand_rows_bytes);
    a.ncand = b.in(h->ncand, h->ncand_bytes);
    a.kp = h->kp;
    a.tau_excl = b.in(h->tau_excl, h->tau_excl_bytes);
    a.cand_keys = b.io(h->cand_keys, h->cand_keys_bytes);
    a.cnt = b.in(h->cnt, h->cnt_bytes);
    a.cap = h->cap;
    a.tau0 = b.in(h->tau0, h->tau0_bytes);
    a.sel = h->sel;
    a.top_w = h->top_w;
    a.qflags = b.in(h->qflags, h->qflags_bytes);
    a.top_tau = b.io(h->top_tau, h->top_tau_bytes);
    a.top_cnt = b.io(h->top_cnt, h->top_cnt_bytes);
    a.k = h->k;
    a.ebound = b.in(h->ebound, h->ebound_bytes);
    a.out_keys = b.io(h->out_keys, h->out_keys_bytes);
    a.fail_cnt = b.io(h->fail_cnt, h->fail_cnt_bytes);
    a.fail_list = b.io(h->fail_list, h->fail_list_bytes);
    a.res_idx = b.io(h->res_idx, h->res_idx_bytes);
    a.res_dist = b.io(h->res_dist, h->res_dist_bytes);
    a.res_cnt = b.io(h->res_cnt, h->res_cnt_bytes);
    a.offset = h->offset;
    a.n_rows = h->n_rows;
    a.dead = b.in(h->dead, h->dead_bytes);
    a.hres_idx = b.host_io(h->hres_idx, h->hres_idx_bytes);
    a.hres_dist = b.host_io(h->hres_dist, h->hres_dist_bytes);
    a.hres_cnt = b.host_io(h->hres_cnt, h->hres_cnt_bytes);
    a.next_status = b.io(h->next_status, h->next_status_bytes);
    a.emit_cnt = b.in(h->emit_cnt, h->emit_cnt_bytes);
    a.cur_status = b.io(h->cur_status, h->cur_status_bytes);
    a.n_queries = h->n_queries;
    a.excl_out = b.io(h->excl_out, h->excl_out_bytes);
    a.merge_words = b.io(h->merge_words, h->merge_words_bytes);
    if (h->pub_flag) {
        if (h->pub_alias) {
            if (!a.res_idx || h->pub_bytes > h->res_idx_bytes) return (int)b.finish(hipErrorInvalidValue);
            a.pub_src = reinterpret_cast<const uint8_t*>(a.res_idx);
        } else {
            if (h->pub_bytes > h->pub_src_bytes) return (int)b.finish(hipErrorInvalidValue);
            a.pub_src = b.in(h->pub_src, h->pub_src_bytes);
        }
        a.pub_dst = b.host_io(h->pub_dst, h->pub_bytes);
        a.pub_bytes = h->pub_bytes;
        a.pub_flag = b.host_io(h->pub_flag, sizeof(uint32_t));
        a.pub_ticket = b.io(h->pub_ticket, bsr::kTicketWords * sizeof(uint32_t));
    }
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_rescore(a, nullptr);
    return b.finish(r);
}

// The scans: launch_scan_exact (n rows), launch_scan_list (list, n_list, groups) and
// launch_scan_list_groups (list, grp, groups, qf = nqf) take the same flat structure; part is the
// whole partial-list buffer.
struct KcScan {
    const float* rows; uint64_t rows_bytes; uint32_t ld, dim; uint64_t n;
    const float* na; uint64_t na_bytes;
    const float* qf32; uint64_t qf32_bytes;
    const int32_t* qids; uint64_t qids_bytes;
    const float* nb; uint64_t nb_bytes;
    const uint32_t* list; uint64_t list_bytes;
    const bsr::ScanGroupDesc* grp; uint64_t grp_bytes;
    uint32_t n_list, nqf, groups, k, grid;
    uint64_t* part; uint64_t part_bytes;
};
}  // extern "C"
static int scan(int kind, const KcScan* h) {
    Bufs b;
    const float* rows = b.in(h->rows, h->rows_bytes);
    const float* na = b.in(h->na, h->na_bytes);
    const float* qf32 = b.in(h->qf32, h->qf32_bytes);
    const int32_t* qids = b.in(h->qids, h->qids_bytes);
    const float* nb = b.in(h->nb, h->nb_bytes);
    const uint32_t* list = b.in(h->list, h->list_bytes);
    const bsr::ScanGroupDesc* grp = b.in(h->grp, h->grp_bytes);
    uint64_t* part = b.io(h->part, h->part_bytes);
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) {
        if (kind == 0)
            r = bsr::launch_scan_exact(rows, h->ld, h->dim, h->n, na, qf32, qids, h->nqf, nb, h->k, h->grid, part, nullptr);
        else if (kind == 1)
            r = bsr::launch_scan_list(rows, h->ld, h->dim, list, h->n_list, na, qf32, qids, h->nqf, h->groups, nb, h->k,
                                      h->grid, part, nullptr);
        else if (kind == 2)
            r = bsr::launch_scan_list_groups(rows, h->ld, h->dim, list, grp, h->groups, h->nqf, na, qf32, qids, nb, h->k,
                                             h->grid, part, nullptr);
        else
            r = hipErrorInvalidValue;
    }
    return b.finish(r);
}
extern "C" {
int kc_scan_exact(const KcScan* h) { return scan(0, h); }
int kc_scan_list(const KcScan* h) { return scan(1, h); }
int kc_scan_list_groups(const KcScan* h) { return scan(2, h); }

// part [grid][qf][k] (qf = nqf rounded up to 1, 2, 4, 8); qids [nqf]; out_keys the whole buffer.
int kc_merge_parts(const uint64_t* part, uint64_t part_bytes, uint32_t grid, const int32_t* qids, uint64_t qids_bytes,
                   uint32_t nqf, uint32_t k, uint64_t* out_keys, uint64_t out_bytes) {
    Bufs b;
    const uint64_t* d_part = b.in(part, part_bytes);
    const int32_t* d_q = b.in(qids, qids_bytes);
    uint64_t* d_out = b.io(out_keys, out_bytes);
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_merge_parts(d_part, grid, d_q, nqf, k, d_out, nullptr);
    return b.finish(r);
}
int kc_merge_parts_groups(const uint64_t* part, uint64_t part_bytes, uint32_t grid, const int32_t* qids,
                          uint64_t qids_bytes, uint32_t qf, const bsr::ScanGroupDesc* grp, uint32_t groups, uint32_t k,
                          uint64_t* out_keys, uint64_t out_bytes) {
    Bufs b;
    const uint64_t* d_part = b.in(part, part_bytes);
    const int32_t* d_q = b.in(qids, qids_bytes);
    const bsr::ScanGroupDesc* d_g = b.in(grp, groups * sizeof(bsr::ScanGroupDesc));
    uint64_t* d_out = b.io(out_keys, out_bytes);
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_merge_parts_groups(d_part, grid, d_q, qf, d_g, groups, k, d_out, nullptr);
    return b.finish(r);
}

// keys, out_idx, out_dist [nq][k]; out_count, n_q (nullable), emit_cnt (nullable) [nq]; status and
// cur_status kStWords words each.
int kc_finalize(const uint64_t* keys, uint32_t nq, uint32_t k, uint64_t n, uint64_t offset, uint64_t* out_idx,
                float* out_dist, uint32_t* out_count, uint32_t* status, const uint32_t* emit_cnt, uint32_t* cur_status,
                const uint32_t* n_q) {
    Bufs b;
    const size_t nqk = (size_t)nq * k;
    const uint64_t* d_keys = b.in(keys, nqk * sizeof(uint64_t));
    uint64_t* d_idx = b.io(out_idx, nqk * sizeof(uint64_t));
    float* d_dist = b.io(out_dist, nqk * sizeof(float));
    uint32_t* d_cnt = b.io(out_count, nq * sizeof(uint32_t));
    uint32_t* d_st = b.io(status, bsr::kStWords * sizeof(uint32_t));
    const uint32_t* d_emit = b.in(emit_cnt, nq * sizeof(uint32_t));
    uint32_t* d_cur = b.io(cur_status, bsr::kStWords * sizeof(uint32_t));
    const uint32_t* d_nq = b.in(n_q, nq * sizeof(uint32_t));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess)
        r = bsr::launch_finalize(d_keys, nq, k, n, offset, d_idx, d_dist, d_cnt, d_st, d_emit, d_cur, nullptr, d_nq);
    return b.finish(r);
}

// MergeArgs without the host mirror and the publish; every buffer with its byte size.
struct KcMerge {
    const uint64_t* idx; uint64_t idx_bytes;
    const float* dist; uint64_t dist_bytes;
    const uint32_t* cnt; uint64_t cnt_bytes;
    uint64_t idx_stride, dist_stride, cnt_stride;
    uint32_t P, nq, k_in, k;
    uint64_t* out_idx; uint64_t out_idx_bytes;
    float* out_dist; uint64_t out_dist_bytes;
    uint32_t* out_count; uint64_t out_count_bytes;
    uint32_t* first_nan;
    const float* excl; uint64_t excl_bytes; uint64_t excl_stride;
    uint32_t need, lists_unique;
    uint32_t* fail_cnt;
    uint32_t* fail_list; uint64_t fail_list_bytes;
    const uint32_t* st; uint64_t st_bytes; uint64_t st_stride;
    uint32_t* st_all; uint64_t st_all_bytes;
};
int kc_merge(const KcMerge* h) {
    Bufs b;
    bsr::MergeArgs a{};
    a.idx = b.in(h->idx, h->idx_bytes);
    a.dist = b.in(h->dist, h->dist_bytes);
    a.cnt = b.in(h->cnt, h->cnt_bytes);
    a.idx_stride = h->idx_stride;
    a.dist_stride = h->dist_stride;
    a.cnt_stride = h->cnt_stride;
    a.P = h->P;
    a.nq = h->nq;
    a.k_in = h->k_in;
    a.k = h->k;
    a.out_idx = b.io(h->out_idx, h->out_idx_bytes);
    a.out_dist = b.io(h->out_dist, h->out_dist_bytes);
    a.out_count = b.io(h->out_count, h->out_count_bytes);
    a.first_nan = b.io(h->first_nan, sizeof(uint32_t));
    a.excl = b.in(h->excl, h->excl_bytes);
    a.excl_stride = h->excl_stride;
    a.need = h->need;
    a.fail_cnt = b.io(h->fail_cnt, sizeof(uint32_t));
    a.fail_list = b.io(h->fail_list, h->fail_list_bytes);
    a.st = b.in(h->st, h->st_bytes);
    a.st_stride = h->st_stride;
    a.st_all = b.io(h->st_all, h->st_all_bytes);
    a.lists_unique = h->lists_unique;
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_merge(a, nullptr);
    return b.finish(r);
}

// The sizes of the flat structures, for the loader to compare with its own layout.
void kc_exact_sizes(uint32_t out[3]) {
    out[0] = (uint32_t)sizeof(KcRescore);
    out[1] = (uint32_t)sizeof(KcScan);
    out[2] = (uint32_t)sizeof(KcMerge);
}

// rows [n_pad][ld]; na [n_pad] (rows >= n are not written); flags one word (OR-ed into).
int kc_row_norms(const float* rows, uint64_t n, uint64_t n_pad, uint32_t dim, uint32_t ld, float* na, uint32_t* flags) {
    Bufs b;
    const float* d_rows = b.in(rows, n_pad * (size_t)ld * sizeof(float));
    float* d_na = b.io(na, n_pad * sizeof(float));
    uint32_t* d_f = b.io(flags, sizeof(uint32_t));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_row_norms(d_rows, n, dim, ld, d_na, d_f, nullptr);
    return b.finish(r);
}

}  // extern "C"
