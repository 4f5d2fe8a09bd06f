// kcheck.cpp -- test-only shim over the launchers of the int8 candidate stage (csrc/kernels.hpp).
//
// Built to lib/libbsr_kcheck.so and linked against libbsr.so; not part of the ABI (include/bsr.h).
// Every function takes host pointers and plain scalars, allocates device buffers of exactly the
// sizes given (the caller passes the sizes the product's call sites in index.cpp use), copies the
// inputs in, launches on the null stream, synchronises, copies the written buffers back and frees
// everything.  A written buffer is in/out: what the kernel leaves untouched comes back as it went in,
// so a test can fill an output with a pattern and see which words were written.  Each function
// returns the hipError_t as an int; nothing is launched after an error.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kernels.hpp"

namespace {

// The device copies of one call's host buffers.
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
    // device copy of an input (nullptr or 0 bytes: no buffer, a null device pointer)
    template <class T>
    const T* in(const T* h, size_t bytes) { return static_cast<const T*>(put(h, nullptr, bytes)); }
    // device copy of a buffer the kernel writes: copied in, and back after the launch
    template <class T>
    T* io(T* h, size_t bytes) { return static_cast<T*>(put(h, h, bytes)); }
    // after the launch: synchronise, copy the written buffers back (only after a clean run), free
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

// Layout constants, so that the Python side never restates a number the kernels own.
struct KcConsts {
    uint32_t ld_align, row_pad, quant_block, sample_stride, sample_scale_rows, filter_tile;
    uint32_t tail_counters, gang_words, gang_min_tiles, sample_tile_every, sample_tile_phase;
    uint32_t skinny_max_q, fused_select_cap, st_words, st_fail, st_emitted, st_query_flags, st_fail2;
    uint64_t skinny_top_min_rows;
};
void kc_consts(KcConsts* c) {
    *c = KcConsts{bsr::kLdAlign, bsr::kRowPad, bsr::kQuantBlock, bsr::kSampleStride, bsr::kSampleScaleRows,
                  bsr::kFilterTile, bsr::kTailCounters, bsr::kGangWords, bsr::kGangMinTiles,
                  bsr::kSampleTileEvery, bsr::kSampleTilePhase, bsr::kSkinnyMaxQ, bsr::kFusedSelectCap,
                  (uint32_t)bsr::kStWords, (uint32_t)bsr::kStFail, (uint32_t)bsr::kStEmitted,
                  (uint32_t)bsr::kStQueryFlags, (uint32_t)bsr::kStFail2, bsr::kSkinnyTopMinRows};
}
uint32_t kc_skinny_top_lists(uint32_t n_rows) { return bsr::skinny_top_lists(n_rows); }
uint32_t kc_sample_tiles_for(uint64_t n) { return bsr::sample_tiles_for(n); }
int kc_skinny_glds_on() { return bsr::skinny_glds_on() ? 1 : 0; }

// rows [n_pad][ld] f32 (index_finish_load: the zero-padded slab), out [n_pad][ld] int8,
// scales [n_pad / 32], ea_max one word (atomicMax: the caller zeroes it, as the load does).
int kc_rows_to_i8(const float* rows, uint64_t n, uint64_t n_pad, uint32_t dim, uint32_t ld, int8_t* out,
                  float* scales, uint32_t* ea_max) {
    Bufs b;
    const float* d_rows = b.in(rows, n_pad * (size_t)ld * sizeof(float));
    int8_t* d_out = b.io(out, n_pad * (size_t)ld);
    float* d_sc = b.io(scales, n_pad / bsr::kQuantBlock * sizeof(float));
    uint32_t* d_ea = b.io(ea_max, sizeof(uint32_t));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_rows_to_i8(d_rows, n, n_pad, dim, ld, d_out, d_sc, d_ea, nullptr);
    return b.finish(r);
}

// out [n_s_pad][ld] int8, scales [n_s_pad / 128]; n_s_pad = round_up(max(ceil(n / 32), 1), 128).
int kc_rows_to_i8_sample(const float* rows, uint64_t n, uint64_t n_pad, uint32_t dim, uint32_t ld, int8_t* out,
                         float* scales, uint64_t n_s_pad) {
    Bufs b;
    const float* d_rows = b.in(rows, n_pad * (size_t)ld * sizeof(float));
    int8_t* d_out = b.io(out, n_s_pad * (size_t)ld);
    float* d_sc = b.io(scales, n_s_pad / bsr::kSampleScaleRows * sizeof(float));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_rows_to_i8_sample(d_rows, n, dim, ld, d_out, d_sc, nullptr);
    return b.finish(r);
}

// search_device's buffers: q [nq][dim]; qf32 [qpad][ld]; nb, qscale, ebound, qflags, qids [qpad];
// qop [qpad][ld] int8; status kStWords words; ea_max one word.
int kc_query_prep(const float* q, uint32_t nq, uint32_t qpad, uint32_t dim, uint32_t ld, const uint32_t* ea_max,
                  float* qf32, float* nb, int8_t* qop, float* qscale, float* ebound, uint32_t* qflags,
                  int32_t* qids, uint32_t* status, int with_op) {
    Bufs b;
    bsr::QueryPrepArgs a{};
    a.q = b.in(q, (size_t)nq * dim * sizeof(float));
    a.nq = nq;
    a.qpad = qpad;
    a.dim = dim;
    a.ld = ld;
    a.ea_max = b.in(ea_max, sizeof(uint32_t));
    a.qf32 = b.io(qf32, (size_t)qpad * ld * sizeof(float));
    a.nb = b.io(nb, qpad * sizeof(float));
    a.qop = b.io(qop, (size_t)qpad * ld);
    a.qscale = b.io(qscale, qpad * sizeof(float));
    a.ebound = b.io(ebound, qpad * sizeof(float));
    a.qflags = b.io(qflags, qpad * sizeof(uint32_t));
    a.qids = b.io(qids, qpad * sizeof(int32_t));
    a.status = b.io(status, bsr::kStWords * sizeof(uint32_t));
    a.with_op = with_op != 0;
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_query_prep(a, nullptr);
    return b.finish(r);
}

// The filter launchers.  GemmArgs with host pointers and the buffers' byte sizes; `kind` picks the
// launcher.  cnt is the whole counter buffer (qpad + 8 kTailCounters + kGangWords words) and
// tail_off the word offset of GemmArgs::tail in it (emit_pass: qpad), or < 0 for tail = nullptr.
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
enum KcKind { kKcSample = 0, kKcEmit = 1, kKcSkinnySample = 2, kKcSkinnyEmit = 3, kKcSkinnyTop = 4, kKcFixup = 5 };

int kc_gemm(int kind, const KcGemm* h) {
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
    g.S = b.io(h->S, h->s_bytes);
    g.s_ld = h->s_ld;
    g.s_compact = h->s_compact;
    g.tau = b.in(h->tau, h->tau_bytes);
    g.cand = b.io(h->cand, h->cand_bytes);
    g.cnt = b.io(h->cnt, h->cnt_bytes);
    g.cap = h->cap;
    g.tail = (g.cnt && h->tail_off >= 0) ? g.cnt + h->tail_off : nullptr;
    g.status = b.io(h->status, h->status_bytes);
    g.n_q = h->n_q;
    g.top_layout = h->top_layout;
    g.s_tiles = h->s_tiles;
    g.s_vals = h->s_vals;
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) {
        switch (kind) {
            case kKcSample: r = bsr::launch_filter_sample(g, nullptr); break;
            case kKcEmit: r = bsr::launch_filter_emit(g, nullptr); break;
            case kKcSkinnySample: r = bsr::launch_filter_skinny_sample(g, nullptr); break;
            case kKcSkinnyEmit: r = bsr::launch_filter_skinny_emit(g, nullptr); break;
            case kKcSkinnyTop: r = bsr::launch_filter_skinny_top(g, nullptr); break;
            case kKcFixup: r = bsr::launch_sample_fixup(g, nullptr); break;
            default: r = hipErrorInvalidValue; break;
        }
    }
    return b.finish(r);
}

// S [qpad][s_ld] (nullptr with n_s = 0: sample_pass's call for small shards); qflags, tau [qpad];
// cnt [qpad + 8 kTailCounters + kGangWords]; status kStWords words; smax [qpad][ks] or nullptr.
int kc_select_tau(const float* S, uint32_t s_ld, uint32_t n_s, uint32_t nq, uint32_t qpad, const uint32_t* qflags,
                  uint32_t ks, float* tau, uint32_t* cnt, uint64_t cnt_words, uint32_t* status, uint64_t* smax) {
    Bufs b;
    const float* d_S = b.in(S, (size_t)qpad * s_ld * sizeof(float));
    const uint32_t* d_f = b.in(qflags, qpad * sizeof(uint32_t));
    float* d_tau = b.io(tau, qpad * sizeof(float));
    uint32_t* d_cnt = b.io(cnt, cnt_words * sizeof(uint32_t));
    uint32_t* d_st = b.io(status, bsr::kStWords * sizeof(uint32_t));
    uint64_t* d_smax = b.io(smax, (size_t)qpad * ks * sizeof(uint64_t));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess)
        r = bsr::launch_select_tau(d_S, s_ld, n_s, nq, qpad, d_f, ks, d_tau, d_cnt, d_st, nullptr, d_smax);
    return b.finish(r);
}

// g [P][qpad][ks] gathered sample keys; qflags, tau [qpad].
int kc_global_tau(const uint64_t* g, uint32_t P, uint32_t qpad, uint32_t nq, uint32_t ks, const uint32_t* qflags,
                  float* tau) {
    Bufs b;
    const uint64_t* d_g = b.in(g, (size_t)P * qpad * ks * sizeof(uint64_t));
    const uint32_t* d_f = b.in(qflags, qpad * sizeof(uint32_t));
    float* d_tau = b.io(tau, qpad * sizeof(float));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_global_tau(d_g, P, qpad, nq, ks, d_f, d_tau, nullptr);
    return b.finish(r);
}

// cand [nq_buf][cap], cnt / tau [nq_buf] (nq_buf >= nq: the padded batch); cand_rows [nq][kp];
// ncand, tau_excl [nq].
int kc_select_cand(const uint64_t* cand, const uint32_t* cnt, uint32_t cap, uint32_t nq, uint32_t nq_buf,
                   const float* tau, uint32_t kp, uint32_t* cand_rows, uint32_t* ncand, float* tau_excl) {
    Bufs b;
    const uint64_t* d_cand = b.in(cand, (size_t)nq_buf * cap * sizeof(uint64_t));
    const uint32_t* d_cnt = b.in(cnt, nq_buf * sizeof(uint32_t));
    const float* d_tau = b.in(tau, nq_buf * sizeof(float));
    uint32_t* d_rows = b.io(cand_rows, (size_t)nq * kp * sizeof(uint32_t));
    uint32_t* d_nc = b.io(ncand, nq * sizeof(uint32_t));
    float* d_tx = b.io(tau_excl, nq * sizeof(float));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess) r = bsr::launch_select_cand(d_cand, d_cnt, cap, nq, d_tau, kp, d_rows, d_nc, d_tx, nullptr);
    return b.finish(r);
}

// ---- the mask bitsets (one kernel family: lists, counts, the cut) --------------------------------
uint32_t kc_mask_block_words() { return bsr::kMaskBlockWords; }
uint32_t kc_mask_blocks(uint64_t n) { return bsr::mask_blocks(n); }

// allow [n_masks][words] (nullptr: every row), dead [words] (nullptr: none), words = ceil(n / 64);
// blk [n_masks][mask_blocks(n) + 1].  grouped = 0: launch_mask_list_count (n_masks = 1; query_mask
// and out are not used); else launch_mask_groups_count with query_mask [nq] (nullable) and
// out [n_masks + 1].
int kc_mask_count(const uint64_t* allow, uint64_t words, uint32_t n_masks, uint64_t n, const uint64_t* dead,
                  const uint32_t* query_mask, uint32_t nq, uint32_t* blk, uint32_t* out, int grouped) {
    Bufs b;
    const uint64_t* d_allow = b.in(allow, (size_t)n_masks * words * sizeof(uint64_t));
    const uint64_t* d_dead = b.in(dead, words * sizeof(uint64_t));
    const uint32_t* d_qm = b.in(query_mask, nq * sizeof(uint32_t));
    uint32_t* d_blk = b.io(blk, (size_t)n_masks * (bsr::mask_blocks(n) + 1) * sizeof(uint32_t));
    uint32_t* d_out = b.io(out, ((size_t)n_masks + 1) * sizeof(uint32_t));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess)
        r = grouped ? bsr::launch_mask_groups_count(d_allow, words, n_masks, n, d_dead, d_qm, nq, d_blk, d_out, nullptr)
                    : bsr::launch_mask_list_count(d_allow, d_dead, n, d_blk, nullptr);
    return b.finish(r);
}

// blk as kc_mask_count left it; list [list_words].  grouped = 0: launch_mask_list_scatter writes the
// first n_list ids at list[0 ..]; else launch_mask_groups_scatter with the n_lists descriptors d
// (MaskListDesc: u64 off, u32 mask, u32 n_list), uploaded here.
int kc_mask_scatter(const uint64_t* allow, uint64_t words, uint32_t n_masks, uint64_t n, const uint64_t* dead,
                    const uint32_t* blk, const void* d, uint32_t n_lists, uint32_t n_list, uint32_t* list,
                    uint64_t list_words, int grouped) {
    Bufs b;
    const uint64_t* d_allow = b.in(allow, (size_t)n_masks * words * sizeof(uint64_t));
    const uint64_t* d_dead = b.in(dead, words * sizeof(uint64_t));
    const uint32_t* d_blk = b.in(blk, (size_t)n_masks * (bsr::mask_blocks(n) + 1) * sizeof(uint32_t));
    const bsr::MaskListDesc* d_d = static_cast<const bsr::MaskListDesc*>(b.in(d, n_lists * sizeof(bsr::MaskListDesc)));
    uint32_t* d_list = b.io(list, list_words * sizeof(uint32_t));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess)
        r = grouped ? bsr::launch_mask_groups_scatter(d_allow, words, n, d_dead, d_blk, d_d, n_lists, d_list, nullptr)
                    : bsr::launch_mask_list_scatter(d_allow, d_dead, n, d_blk, n_list, d_list, nullptr);
    return b.finish(r);
}

// cand [nq_buf][cap], cnt / raw [nq_buf] (nq_buf >= nq), items one word; allow [n_masks][words];
// query_mask [nq] (nullptr: mask 0 for every query); dead [words] (nullable).
int kc_mask_cut(uint64_t* cand, uint32_t* cnt, uint32_t cap, uint32_t nq, uint32_t nq_buf, const uint64_t* allow,
                uint64_t words, uint32_t n_masks, const uint32_t* query_mask, const uint64_t* dead, uint64_t n,
                uint32_t* raw, uint32_t* items) {
    Bufs b;
    uint64_t* d_cand = b.io(cand, (size_t)nq_buf * cap * sizeof(uint64_t));
    uint32_t* d_cnt = b.io(cnt, nq_buf * sizeof(uint32_t));
    const uint64_t* d_allow = b.in(allow, (size_t)n_masks * words * sizeof(uint64_t));
    const uint32_t* d_qm = b.in(query_mask, nq * sizeof(uint32_t));
    const uint64_t* d_dead = b.in(dead, words * sizeof(uint64_t));
    uint32_t* d_raw = b.io(raw, nq_buf * sizeof(uint32_t));
    uint32_t* d_items = b.io(items, sizeof(uint32_t));
    hipError_t r = hipSuccess;
    if (b.err == hipSuccess)
        r = bsr::launch_mask_cut(d_cand, d_cnt, cap, nq, d_allow, words, d_qm, d_dead, n, d_raw, d_items, nullptr);
    return b.finish(r);
}

}  // extern "C"
