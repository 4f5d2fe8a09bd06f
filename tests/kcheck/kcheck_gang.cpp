// kcheck_gang.cpp -- test-only shim over launch_filter_emit_gang (csrc/kernels.hpp): the 768-byte
// gang build of the emit filter, k_filter_qs16<true, 12, true>, at shard sizes where
// launch_filter_emit picks the small-shard build.
//
// Built to lib/libbsr_kcheck_gang.so and linked against libbsr.so; not part of the ABI
// (include/bsr.h).  The conventions are kcheck.cpp's: host pointers and byte sizes in, device
// buffers of exactly those sizes, one launch on the null stream, the written buffers (cand, cnt)
// copied back after a clean run, the hipError_t returned as an int.
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

// kcheck.cpp's KcGemm, field for field (the Python side passes the same structure to both shims).
struct KcGemm {
    const uint8_t* A; uint64_t a_bytes; uint64_t a_stride; uint32_t n_rows, a_scale_rows;
    const uint8_t* B; uint64_t b_bytes; uint32_t row_bytes, n_rt, n_qt;
    const float* a_scale; uint64_t a_scale_bytes;
    const float* b_scale; uint64_t b_scale_bytes;
    float* S; uint64_t s_bytes; uint32_t s_ld, s_compact;
    const float* tau; uint64_t tau_bytes;
    uint64_t* cand; uint64_t cand_bytes;
    uint32_t* cnt; uint64_t cnt_bytes; uint32_t cap; int32_t tail_off;
    uint32_t* status; uint64_t status_bytes;
    uint32_t n_q, top_layout, s_tiles, s_vals;
};

// The records per wave of the gang build's emission queue (a dense tile must overfill it).
int kc_gang_queue_depth() { return bsr::kEmitQueueDepth; }

int kc_gemm_gang(const KcGemm* h) {
    Bufs b;
    bsr::GemmArgs g{};
    g.A = b.in(h->A, h->a_bytes);
    g.a_stride = h->a_stride;
    g.n_rows = h->n_rows;
    g.a_scale_rows = h->a_scale_rows;
    g.B = b.in(h->B, h->b_bytes);
    g.row_bytes = h->row_bytes;
    g.n_rt = h->n_rt;
    g.n_qt = h->n_qt;
    g.a_scale = b.in(h->a_scale, h->a_scale_bytes);
    g.b_scale = b.in(h->b_scale, h->b_scale_bytes);
    g.s_ld = h->s_ld;
    g.tau = b.in(h->tau, h->tau_bytes);
    g.cand = b.io(h->cand, h->cand_bytes);
    g.cnt = b.io(h->cnt, h->cnt_bytes);
    g.cap = h->cap;
    g.tail = (g.cnt && h->tail_off >= 0) ? g.cnt + h->tail_off : nullptr;
    g.n_q = h->n_q;
    g.s_tiles = h->s_tiles;
    g.s_vals = h->s_vals;
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_filter_emit_gang(g, nullptr);
    return b.finish(r);
}

}  // extern "C"
