// kcheck_range_list.cpp -- test-only shim over the launchers of the masked range search
// (csrc/k_exact.hip: launch_range_scan_list_groups, launch_range_route; csrc/k_prep.hip:
// launch_mask_groups_scatter_seg).
//
// Built to lib/libbsr_kcheck_range_list.so and linked against libbsr.so; not part of the ABI.  The
// conventions are kcheck_range.cpp's: host pointers and plain scalars in, device buffers of exactly
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

// RangeListArgs, flat, with the byte size of every buffer (keys and rcnt in/out).
struct KcRangeList {
    const float* rows; uint64_t rows_bytes; uint32_t ld, dim;
    const float* na; uint64_t na_bytes;
    const float* qf32; uint64_t qf32_bytes;
    const float* nb; uint64_t nb_bytes;
    const float* radius; uint64_t radius_bytes;
    const uint32_t* list; uint64_t list_bytes;
    const bsr::ScanGroupDesc* grp; uint64_t grp_bytes;
    uint32_t groups, qf;
    const int32_t* qids; uint64_t qids_bytes;
    uint64_t* keys; uint64_t keys_bytes;
    uint32_t* rcnt; uint64_t rcnt_bytes;
    uint32_t cap, grid;
};
uint32_t kc_range_list_sizeof(void) { return (uint32_t)sizeof(KcRangeList); }
uint32_t kc_seg_desc_sizeof(void) { return (uint32_t)sizeof(bsr::MaskSegDesc); }

int kc_range_scan_list_groups(const KcRangeList* h) {
    Bufs b;
    bsr::RangeListArgs a{};
    a.rows = b.in(h->rows, h->rows_bytes);
    a.ld = h->ld;
    a.dim = h->dim;
    a.na = b.in(h->na, h->na_bytes);
    a.qf32 = b.in(h->qf32, h->qf32_bytes);
    a.nb = b.in(h->nb, h->nb_bytes);
    a.radius = b.in(h->radius, h->radius_bytes);
    a.list = b.in(h->list, h->list_bytes);
    a.grp = b.in(h->grp, h->grp_bytes);
    a.groups = h->groups;
    a.qf = h->qf;
    a.qids = b.in(h->qids, h->qids_bytes);
    a.keys = b.io(h->keys, h->keys_bytes);
    a.rcnt = b.io(h->rcnt, h->rcnt_bytes);
    a.cap = h->cap;
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(bsr::launch_range_scan_list_groups(a, h->grid, nullptr));
}

// launch_range_route: to_list / radius [nq] in; tau [nq], scan_list [list_words] and status
// [kStWords] in/out.
int kc_range_route(const uint32_t* to_list, const float* radius, uint32_t nq, float* tau, uint32_t* scan_list,
                   uint64_t list_words, uint32_t* status) {
    Bufs b;
    const uint32_t* d_t = b.in(to_list, (size_t)nq * 4);
    const float* d_r = b.in(radius, (size_t)nq * 4);
    float* d_tau = b.io(tau, (size_t)nq * 4);
    uint32_t* d_list = b.io(scan_list, (size_t)list_words * 4);
    uint32_t* d_st = b.io(status, (size_t)bsr::kStWords * 4);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(bsr::launch_range_route(d_t, d_r, nq, d_tau, d_list, d_st, nullptr));
}

// launch_mask_groups_count + launch_mask_groups_scatter_seg: allow [n_masks][words], dead [words]
// (nullable), segs [n_segs] in; list [list_words] in/out; a_out [n_masks] receives every A_g.
int kc_mask_scatter_seg(const uint64_t* allow, uint64_t words, uint32_t n_masks, uint64_t n, const uint64_t* dead,
                        const bsr::MaskSegDesc* segs, uint32_t n_segs, uint32_t* list, uint64_t list_words,
                        uint32_t* a_out) {
    Bufs b;
    const uint32_t n_blk = bsr::mask_blocks(n);
    std::vector<uint32_t> blk((size_t)n_masks * (n_blk + 1), 0);
    const uint64_t* d_allow = b.in(allow, (size_t)n_masks * words * 8);
    const uint64_t* d_dead = b.in(dead, (size_t)words * 8);
    const bsr::MaskSegDesc* d_segs = b.in(segs, (size_t)n_segs * sizeof(bsr::MaskSegDesc));
    uint32_t* d_blk = static_cast<uint32_t*>(b.put(blk.data(), nullptr, blk.size() * 4));
    uint32_t* d_list = b.io(list, (size_t)list_words * 4);
    uint32_t* d_out = b.io(a_out, (size_t)n_masks * 4);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    hipError_t e = bsr::launch_mask_groups_count(d_allow, words, n_masks, n, d_dead, nullptr, 0, d_blk, d_out, nullptr);
    if (e == hipSuccess) e = bsr::launch_mask_groups_scatter_seg(d_allow, words, n, d_dead, d_blk, d_segs, n_segs, d_list, nullptr);
    return b.finish(e);
}

}  // extern "C"
