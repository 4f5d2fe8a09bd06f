// kcheck_mmr.cpp -- test-only shim over the launcher of the MMR selection (csrc/k_exact.hip:
// launch_mmr_select).
//
// Built to lib/libbsr_kcheck_mmr.so and linked against libbsr.so; not part of the ABI.  The
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

uint32_t kc_mmr_max_fetch(void) { return bsr::kMmrMaxFetch; }

// MmrArgs, flat, with the byte size of every buffer (out_idx, out_dist, out_rank and out_count in/out).
struct KcMmr {
    const float* rows; uint64_t rows_bytes; uint32_t ld, dim; uint64_t n, offset;
    const float* na; uint64_t na_bytes;
    const uint64_t* cand_idx; uint64_t cand_idx_bytes;
    const float* cand_dist; uint64_t cand_dist_bytes;
    const uint32_t* cand_cnt; uint64_t cand_cnt_bytes;
    uint32_t nq, fetch_k, k; float lambda;
    uint64_t* out_idx; uint64_t out_idx_bytes;
    float* out_dist; uint64_t out_dist_bytes;
    uint32_t* out_rank; uint64_t out_rank_bytes;
    uint32_t* out_count; uint64_t out_count_bytes;
};
uint32_t kc_mmr_sizeof(void) { return (uint32_t)sizeof(KcMmr); }

int kc_mmr_select(const KcMmr* h) {
    Bufs b;
    bsr::MmrArgs a{};
    a.rows = b.in(h->rows, h->rows_bytes);
    a.ld = h->ld;
    a.dim = h->dim;
    a.n = h->n;
    a.offset = h->offset;
    a.na = b.in(h->na, h->na_bytes);
    a.cand_idx = b.in(h->cand_idx, h->cand_idx_bytes);
    a.cand_dist = b.in(h->cand_dist, h->cand_dist_bytes);
    a.cand_cnt = b.in(h->cand_cnt, h->cand_cnt_bytes);
    a.nq = h->nq;
    a.fetch_k = h->fetch_k;
    a.k = h->k;
    a.lambda = h->lambda;
    a.out_idx = b.io(h->out_idx, h->out_idx_bytes);
    a.out_dist = b.io(h->out_dist, h->out_dist_bytes);
    a.out_rank = b.io(h->out_rank, h->out_rank_bytes);
    a.out_count = b.io(h->out_count, h->out_count_bytes);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(bsr::launch_mmr_select(a, nullptr));
}

}  // extern "C"
