// kcheck_deep_cap_list.cpp -- test-only shim over the deep capped list scan (csrc/k_exact.hip:
// launch_deep_cap_scan_list, with launch_deep_cap_select without a bound behind it and
// launch_deep_cap_finish at the end, as the masked deep capped search runs them).
//
// Built to lib/libbsr_kcheck_deep_cap_list.so and linked against libbsr.so; not part of the ABI.  The
// conventions are kcheck_deep_list.cpp's: host pointers and plain scalars in, device buffers of
// exactly the sizes given, the null stream, a synchronise, the written buffers copied back
// (pattern-filled by the caller, so they show which words the kernels wrote), the hipError_t
// returned as an int.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kernels.hpp"

extern "C" {

uint32_t kc_deep_cap_scan_qf(void) { return bsr::kDeepCapScanQF; }

// One query group -- qids [qf], the first nq_own its own -- over the n_segs segments seg_off / seg_len
// of list [list_words], a launch per segment with `grid` workgroups a group (0: scan_grid_for of the
// segment) and the capped merge into the carry behind each: carry [nq][k] in/out (kKeyNone: no key
// yet).  At the end every query's carry as rows: out_idx / out_dist / out_group [nq][k], out_count
// [nq].  rows [n_pad][ld], na [n_pad], row_group [n_pad], qf32 [nq][ld], nb [nq].
int kc_deep_cap_scan_list(const float* rows, uint64_t n_pad, uint32_t ld, uint32_t dim, const float* na,
                          const uint32_t* row_group, const float* qf32, const float* nb, uint32_t nq,
                          const uint32_t* list, uint64_t list_words, const uint64_t* seg_off, const uint32_t* seg_len,
                          uint32_t n_segs, const int32_t* qids, uint32_t qf, uint32_t nq_own, uint32_t k, uint32_t m,
                          uint32_t grid, uint64_t offset, uint64_t* carry, uint64_t* out_idx, float* out_dist,
                          uint32_t* out_group, uint32_t* out_count) {
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
    std::vector<int32_t> all(nq);
    for (uint32_t q = 0; q < nq; ++q) all[q] = (int32_t)q;
    bsr::DeepCapListArgs a{};
    a.l.rows = (const float*)put(rows, nullptr, (size_t)n_pad * ld * 4);
    a.l.ld = ld;
    a.l.dim = dim;
    a.l.na = (const float*)put(na, nullptr, (size_t)n_pad * 4);
    a.l.qf32 = (const float*)put(qf32, nullptr, (size_t)nq * ld * 4);
    a.l.nb = (const float*)put(nb, nullptr, (size_t)nq * 4);
    a.l.list = (const uint32_t*)put(list, nullptr, (size_t)list_words * 4);
    const bsr::ScanGroupDesc* d_grp = (const bsr::ScanGroupDesc*)put(grp.data(), nullptr, grp.size() * sizeof grp[0]);
    a.l.groups = 1;
    a.l.qf = qf;
    a.l.qids = (const int32_t*)put(qids, nullptr, (size_t)qf * 4);
    a.l.k = k;
    a.l.part = (uint64_t*)put(part.data(), nullptr, part_keys * 8);
    uint64_t* d_carry = (uint64_t*)put(carry, carry, (size_t)nq * k * 8);
    a.l.carry = d_carry;
    a.row_group = (const uint32_t*)put(row_group, nullptr, (size_t)n_pad * 4);
    a.per_group = m;
    bsr::DeepCapSelectArgs se{};
    se.keys = a.l.part;
    se.nq = qf;
    se.qids = a.l.qids;
    se.k = k;
    se.per_group = m;
    se.row_group = a.row_group;
    se.out_keys = d_carry;
    se.qf = qf;
    for (uint32_t s = 0; s < n_segs && err == hipSuccess; ++s) {
        const uint32_t g = grid ? grid : bsr::scan_grid_for(seg_len[s]);
        a.l.grp = se.grp = d_grp + s;
        se.cap = (g + 1) * k;
        err = bsr::launch_deep_cap_scan_list(a, g, nullptr);
        if (err == hipSuccess) err = bsr::launch_deep_cap_select(se, nullptr);
    }
    const int32_t* d_all = (const int32_t*)put(all.data(), nullptr, (size_t)nq * 4);
    uint64_t* d_idx = (uint64_t*)put(out_idx, out_idx, (size_t)nq * k * 8);
    float* d_dist = (float*)put(out_dist, out_dist, (size_t)nq * k * 4);
    uint32_t* d_group = (uint32_t*)put(out_group, out_group, (size_t)nq * k * 4);
    uint32_t* d_count = (uint32_t*)put(out_count, out_count, (size_t)nq * 4);
    if (err == hipSuccess)
        err = bsr::launch_deep_cap_finish(d_carry, d_all, nq, k, offset, a.row_group, d_idx, d_dist, d_group, d_count,
                                          nullptr);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    for (auto& b : v) {
        if (err == hipSuccess && b.h) err = hipMemcpy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost);
        (void)hipFree(b.d);
    }
    return (int)err;
}

}  // extern "C"
