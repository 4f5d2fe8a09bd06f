// kcheck_deep.cpp -- test-only shim over the deep search's selection (csrc/k_exact.hip:
// launch_deep_select).
//
// Built to lib/libbsr_kcheck_deep.so and linked against libbsr.so; not part of the ABI.  The
// conventions are kcheck_exact.cpp's: host pointers and plain scalars in, device buffers of exactly
// the sizes given, the null stream, a synchronise, the written buffers copied back (pattern-filled
// by the caller, so they show which words the kernel wrote), the hipError_t returned as an int.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kernels.hpp"

extern "C" {

uint32_t kc_deep_max_k(void) { return bsr::kDeepMaxK; }
uint32_t kc_deep_cap(uint32_t k) { return bsr::deep_cap(k); }

// keys [n_items][n_keys] with kcnt [n_items] (nullable) -> out_idx / out_dist [n_items][k],
// out_count [n_items].  tau (nullable, with ebound / nb / emit_cnt [n_items]): the certification;
// fail [n_items] and status [kStWords] are then written too.
int kc_deep_select(const uint64_t* keys, const uint32_t* kcnt, uint32_t n_keys, uint32_t n_items, uint32_t k,
                   uint64_t offset, const float* tau, const float* ebound, const float* nb, const uint32_t* emit_cnt,
                   uint32_t cap, uint64_t* out_idx, float* out_dist, uint32_t* out_count, uint32_t* fail,
                   uint32_t* status) {
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
    const size_t ni = n_items;
    bsr::DeepSelectArgs a{};
    a.keys = (const uint64_t*)put(keys, nullptr, ni * n_keys * 8);
    a.stride = n_keys;
    a.kcnt = (const uint32_t*)put(kcnt, nullptr, ni * 4);
    a.n_keys = n_keys;
    a.n_items = n_items;
    a.k = k;
    a.offset = offset;
    a.tau = (const float*)put(tau, nullptr, ni * 4);
    a.ebound = (const float*)put(ebound, nullptr, ni * 4);
    a.nb = (const float*)put(nb, nullptr, ni * 4);
    a.emit_cnt = (const uint32_t*)put(emit_cnt, nullptr, ni * 4);
    a.cap = cap;
    a.out_idx = (uint64_t*)put(out_idx, out_idx, ni * k * 8);
    a.out_dist = (float*)put(out_dist, out_dist, ni * k * 4);
    a.out_count = (uint32_t*)put(out_count, out_count, ni * 4);
    a.fail = (uint32_t*)put(fail, fail, ni * 4);
    a.status = (uint32_t*)put(status, status, bsr::kStWords * 4);
    if (err == hipSuccess) err = bsr::launch_deep_select(a, nullptr);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    for (auto& b : v) {
        if (err == hipSuccess && b.h) err = hipMemcpy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost);
        (void)hipFree(b.d);
    }
    return (int)err;
}

}  // extern "C"
