// kcheck_score.cpp -- test-only shim over the launchers of the id scoring (csrc/k_exact.hip:
// launch_score_ids, launch_score_finish).
//
// Built to lib/libbsr_kcheck_score.so and linked against libbsr.so; not part of the ABI.  The
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

uint32_t kc_score_max_ids(void) { return bsr::kScoreMaxIds; }

// ScoreArgs, flat, with the byte size of every buffer (dist, keys, kcnt and found in/out).
struct KcScore {
    const float* rows; uint64_t rows_bytes; uint32_t ld, dim; uint64_t n, offset;
    const float* na; uint64_t na_bytes;
    const float* qf32; uint64_t qf32_bytes;
    const float* nb; uint64_t nb_bytes;
    const uint64_t* dead; uint64_t dead_bytes;
    const uint64_t* ids; uint64_t ids_bytes;
    uint32_t m, nq;
    float* dist; uint64_t dist_bytes;
    uint64_t* keys; uint64_t keys_bytes;
    uint32_t* kcnt; uint64_t kcnt_bytes;
    uint32_t* found; uint64_t found_bytes;
};
uint32_t kc_score_sizeof(void) { return (uint32_t)sizeof(KcScore); }

int kc_score_ids(const KcScore* h) {
    Bufs b;
    bsr::ScoreArgs a{};
    a.rows = b.in(h->rows, h->rows_bytes);
    a.ld = h->ld;
    a.dim = h->dim;
    a.n = h->n;
    a.offset = h->offset;
    a.na = b.in(h->na, h->na_bytes);
    a.qf32 = b.in(h->qf32, h->qf32_bytes);
    a.nb = b.in(h->nb, h->nb_bytes);
    a.dead = b.in(h->dead, h->dead_bytes);
    a.ids = b.in(h->ids, h->ids_bytes);
    a.m = h->m;
    a.nq = h->nq;
    a.dist = b.io(h->dist, h->dist_bytes);
    a.keys = b.io(h->keys, h->keys_bytes);
    a.kcnt = b.io(h->kcnt, h->kcnt_bytes);
    a.found = b.io(h->found, h->found_bytes);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(bsr::launch_score_ids(a, nullptr));
}

// launch_score_finish: keys [nq][m], kcnt [nq] in; out_idx / out_dist [nq][k], out_count [nq] in/out.
int kc_score_finish(const uint64_t* keys, const uint32_t* kcnt, uint32_t m, uint32_t nq, uint32_t k, uint64_t offset,
                    uint64_t* out_idx, float* out_dist, uint32_t* out_count) {
    Bufs b;
    const uint64_t* d_keys = b.in(keys, (size_t)nq * m * 8);
    const uint32_t* d_kcnt = b.in(kcnt, (size_t)nq * 4);
    uint64_t* d_idx = b.io(out_idx, (size_t)nq * k * 8);
    float* d_dist = b.io(out_dist, (size_t)nq * k * 4);
    uint32_t* d_cnt = b.io(out_count, (size_t)nq * 4);
    if (b.err != hipSuccess) return b.finish(hipSuccess);
    return b.finish(bsr::launch_score_finish(d_keys, d_kcnt, m, nq, k, offset, d_idx, d_dist, d_cnt, nullptr));
}

}  // extern "C"
