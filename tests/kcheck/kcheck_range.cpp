// kcheck_range.cpp -- test-only shim over the launchers of the range search (csrc/k_exact.hip:
// launch_range_tau, launch_range_rescore, launch_range_scan, launch_range_finish).
//
// Built to lib/libbsr_kcheck_range.so and linked against libbsr.so; not part of the ABI.  The
// conventions are kcheck_exact.cpp's: host pointers and plain scalars in, device buffers of exactly
// the sizes given (a null pointer or 0 bytes: a null device pointer), the null stream, a
// synchronise, the written buffers copied back (a written buffer is in/out, so a pattern-filled
// output shows which words the kernel wrote), the hipError_t returned as an int.
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

struct KcRangeConsts {
    uint32_t scan_qf, max_results, nan_radius, tail_words;
    uint32_t st_words, st_fail, st_emitted, st_query_flags, st_fail2, query_no_approx;
};
void kc_range_consts(KcRangeConsts* c) {
    *c = KcRangeConsts{bsr::kScanQF, bsr::kRangeMaxResults, bsr::kRangeNanRadius,
                       8 * bsr::kTailCounters + bsr::kGangWords, (uint32_t)bsr::kStWords, (uint32_t)bsr::kStFail,
                       (uint32_t)bsr::kStEmitted, (uint32_t)bsr::kStQueryFlags, (uint32_t)bsr::kStFail2,
                       bsr::kQueryNoApprox};
}
uint32_t kc_range_cap(uint32_t capacity) { return bsr::range_cap(capacity); }

// launch_range_tau: radius / ebound / nb / qflags [nq]; tau [qpad], cnt [qpad + tail_words], rcnt
// [nq], scan_list [nq] and status [st_words] are in/out.
int kc_range_tau(const float* radius, const float* ebound, const float* nb, const uint32_t* qflags, uint32_t nq,
                 uint32_t qpad, float* tau, uint32_t* cnt, uint64_t cnt_words, uint32_t* rcnt, uint32_t* scan_list,
                 uint32_t* status) {
    Bufs b;
    const float* d_r = b.in(radius, (size_t)nq * 4);
    const float* d_e = b.in(ebound, (size_t)nq * 4);
    const float* d_nb = b.in(nb, (size_t)nq * 4);
    const uint32_t* d_f = b.in(qflags, (size_t)nq * 4);
    float* d_tau = b.io(tau, (size_t)qpad * 4);
    uint32_t* d_cnt = b.io(cnt, (size_t)cnt_words * 4);
    uint32_t* d_rcnt = b.io(rcnt, (size_t)nq * 4);
    uint32_t* d_list = b.io(scan_list, (size_t)nq * 4);
    uint32_t* d_st = b.io(status, (size_t)bsr::kStWords * 4);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(bsr::launch_range_tau(d_r, d_e, d_nb, d_f, nq, qpad, d_tau, d_cnt, d_rcnt, d_list, d_st, nullptr));
}

// RangeArgs, flat, with the byte size of every buffer (keys, rcnt, scan_list and status in/out).
struct KcRange {
    const float* rows; uint64_t rows_bytes; uint32_t ld, dim; uint64_t n;
    const float* na; uint64_t na_bytes;
    const float* qf32; uint64_t qf32_bytes;
    const float* nb; uint64_t nb_bytes;
    const float* radius; uint64_t radius_bytes;
    const uint64_t* dead; uint64_t dead_bytes;
    uint64_t* keys; uint64_t keys_bytes;
    uint32_t* rcnt; uint64_t rcnt_bytes;
    uint32_t cap, nq;
    const uint64_t* cand; uint64_t cand_bytes;
    const uint32_t* cnt; uint64_t cnt_bytes;
    uint32_t* scan_list; uint64_t scan_list_bytes;
    uint32_t* status; uint64_t status_bytes;
    const int32_t* qids; uint64_t qids_bytes;
    uint32_t nqf, grid;
};
uint32_t kc_range_sizeof(void) { return (uint32_t)sizeof(KcRange); }

static bsr::RangeArgs range_args(Bufs& b, const KcRange* h) {
    bsr::RangeArgs a{};
    a.rows = b.in(h->rows, h->rows_bytes);
    a.ld = h->ld;
    a.dim = h->dim;
    a.n = h->n;
    a.na = b.in(h->na, h->na_bytes);
    a.qf32 = b.in(h->qf32, h->qf32_bytes);
    a.nb = b.in(h->nb, h->nb_bytes);
    a.radius = b.in(h->radius, h->radius_bytes);
    a.dead = b.in(h->dead, h->dead_bytes);
    a.keys = b.io(h->keys, h->keys_bytes);
    a.rcnt = b.io(h->rcnt, h->rcnt_bytes);
    a.cap = h->cap;
    a.nq = h->nq;
    a.cand = b.in(h->cand, h->cand_bytes);
    a.cnt = b.in(h->cnt, h->cnt_bytes);
    a.scan_list = b.io(h->scan_list, h->scan_list_bytes);
    a.status = b.io(h->status, h->status_bytes);
    a.qids = b.in(h->qids, h->qids_bytes);
    a.nqf = h->nqf;
    return a;
}

int kc_range_rescore(const KcRange* h) {
    Bufs b;
    const bsr::RangeArgs a = range_args(b, h);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(bsr::launch_range_rescore(a, nullptr));
}

int kc_range_scan(const KcRange* h) {
    Bufs b;
    const bsr::RangeArgs a = range_args(b, h);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(bsr::launch_range_scan(a, h->grid, nullptr));
}

// launch_range_finish: keys [nq][cap], rcnt [nq] in; out_idx / out_dist [nq][capacity], out_count [nq] in/out.
int kc_range_finish(const uint64_t* keys, const uint32_t* rcnt, uint32_t cap, uint32_t nq, uint32_t capacity,
                    uint64_t offset, uint64_t* out_idx, float* out_dist, uint32_t* out_count) {
    Bufs b;
    const uint64_t* d_keys = b.in(keys, (size_t)nq * cap * 8);
    const uint32_t* d_rcnt = b.in(rcnt, (size_t)nq * 4);
    uint64_t* d_idx = b.io(out_idx, (size_t)nq * capacity * 8);
    float* d_dist = b.io(out_dist, (size_t)nq * capacity * 4);
    uint32_t* d_cnt = b.io(out_count, (size_t)nq * 4);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(bsr::launch_range_finish(d_keys, d_rcnt, cap, nq, capacity, offset, d_idx, d_dist, d_cnt, nullptr));
}

}  // extern "C"
