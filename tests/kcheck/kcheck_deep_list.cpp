// kcheck_deep_list.cpp -- test-only shim over the deep exact scan over row lists (csrc/k_exact.hip:
// launch_deep_scan_list, with launch_deep_select behind it as the masked deep search runs them).
//
// Built to lib/libbsr_kcheck_deep_list.so and linked against libbsr.so; not part of the ABI.  The
// conventions are kcheck_deep.cpp's: host pointers and plain scalars in, device buffers of exactly
// the sizes given, the null stream, a synchronise, the written buffers copied back (pattern-filled
// by the caller, so they show which words the kernels wrote), the hipError_t returned as an int.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kernels.hpp"

extern "C" {

uint32_t kc_deep_scan_buf(void) { return bsr::kDeepScanBuf; }

// One query group -- qids [qf], the first nq_own its own -- over the n_segs segments seg_off / seg_len
// of list [list_words], a launch per segment with `grid` workgroups a group (0: scan_grid_for of the
// segment) and the selection into the carry behind each: carry [nq][k] in/out (kKeyNone: no key
// yet).  At the end the selection of every query's carry into out_idx / out_dist [nq][k] and
// out_count [nq].  rows [n_pad][ld], na [n_pad], qf32 [nq][ld], nb [nq].
int kc_deep_scan_list(const float* rows, uint64_t n_pad, uint32_t ld, uint32_t dim, const float* na, const float* qf32,
                      const float* nb, uint32_t nq, const uint32_t* list, uint64_t list_words, const uint64_t* seg_off,
                      const uint32_t* seg_len, uint32_t n_segs, const int32_t* qids, uint32_t qf, uint32_t nq_own,
                      uint32_t k, uint32_t grid, uint64_t offset, uint64_t* carry, uint64_t* out_idx, float* out_dist,
                      uint32_t* out_count) {
    struct B { void* d; void* h; size_t bytes; };
    std::vector<B> v;
    hipError_t err = hipSuccess;
    auto put = [&](const void* h, void* back, size_t bytes) -> void* {
        void* d = nullptr;
        if (err != hipSuccess || !h || !bytes) return d;
        err = hipMalloc(&d, bytes);
        if (err != hipSuccess) return nullptr;
        v.push_back({d, back, bytes});
        err = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
        return d;
    };
    std::vector<bsr::ScanGroupDesc> grp(n_segs);
    uint32_t grid_max = 1;
    for (uint32_t s = 0; s < n_segs; ++s) {
        grp[s] = bsr::ScanGroupDesc{seg_off[s], seg_len[s], nq_own};
        const uint32_t g = grid ? grid : bsr::scan_grid_for(seg_len[s]);
        grid_max = g > grid_max ? g : grid_max;
    }
    const size_t part_keys = (size_t)qf * (grid_max + 1) * k;
    std::vector<uint64_t> part(part_keys, 0x5A5A5A5A5A5A5A5Aull);  // (a slot not written shows in the result)
    bsr::DeepListArgs a{};
    a.rows = (const float*)put(rows, nullptr, (size_t)n_pad * ld * 4);
    a.ld = ld;
    a.dim = dim;
    a.na = (const float*)put(na, nullptr, (size_t)n_pad * 4);
    a.qf32 = (const float*)put(qf32, nullptr, (size_t)nq * ld * 4);
    a.nb = (const float*)put(nb, nullptr, (size_t)nq * 4);
    a.list = (const uint32_t*)put(list, nullptr, (size_t)list_words * 4);
    const bsr::ScanGroupDesc* d_grp = (const bsr::ScanGroupDesc*)put(grp.data(), nullptr, grp.size() * sizeof grp[0]);
    a.groups = 1;
    a.qf = qf;
    a.qids = (const int32_t*)put(qids, nullptr, (size_t)qf * 4);
    a.k = k;
    a.part = (uint64_t*)put(part.data(), nullptr, part_keys * 8);
    uint64_t* d_carry = (uint64_t*)put(carry, carry, (size_t)nq * k * 8);
    a.carry = d_carry;
    bsr::DeepSelectArgs se{};
    se.keys = a.part;
    se.n_items = qf;
    se.qids = a.qids;
    se.k = k;
    se.out_keys = d_carry;
    se.qf = qf;
    for (uint32_t s = 0; s < n_segs && err == hipSuccess; ++s) {
        const uint32_t g = grid ? grid : bsr::scan_grid_for(seg_len[s]);
        a.grp = se.grp = d_grp + s;
        se.stride = (uint64_t)(g + 1) * k;
        se.n_keys = (g + 1) * k;
        err = bsr::launch_deep_scan_list(a, g, nullptr);
        if (err == hipSuccess) err = bsr::launch_deep_select(se, nullptr);
    }
    bsr::DeepSelectArgs fe{};
    fe.keys = d_carry;
    fe.stride = k;
    fe.n_keys = k;
    fe.n_items = nq;
    fe.k = k;
    fe.offset = offset;
    fe.out_idx = (uint64_t*)put(out_idx, out_idx, (size_t)nq * k * 8);
    fe.out_dist = (float*)put(out_dist, out_dist, (size_t)nq * k * 4);
    fe.out_count = (uint32_t*)put(out_count, out_count, (size_t)nq * 4);
    if (err == hipSuccess) err = bsr::launch_deep_select(fe, nullptr);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    for (auto& b : v) {
        if (err == hipSuccess && b.h) err = hipMemcpy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost);
        (void)hipFree(b.d);
    }
    return (int)err;
}

}  // extern "C"
