// exact_walk.hpp -- the device pieces of the exact stage that more than one kernel file uses
// (k_exact.hip, k_groups.hip): the chunked walk of 64 rows against one vector, the tombstone test
// and the insert into the m entries of a group.  Include it only from a file compiled with
// -ffp-contract=off (see bsr_device.hpp).
#pragma once

#include "bsr_device.hpp"

namespace bsr {

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// Loads of one 64-element chunk of 64 candidate rows (16 x 16 B per lane; each
// wave-instruction covers 4 rows x 256 B).
__device__ __forceinline__ void load_cand_chunk(f32x4_t (&pre)[16], const float* __restrict__ rows,
                                                uint32_t ld, const uint32_t (&lrow)[16], uint32_t ch,
                                                int lane) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
        pre[i] = *reinterpret_cast<const f32x4_t*>(rows + (uint64_t)lrow[i] * ld + ch * 64 + (lane & 15) * 4);
}

// One 64-element chunk of 64 rows held in LDS (stride 68 floats), walked in index order by
// the lane that owns the row: sequential dot (separate f32 mul and add) and max|a_i - b_i|.
template <int QF>
__device__ __forceinline__ void seq_chunk(const float* __restrict__ my, const float* const (&bq)[QF],
                                          uint32_t nvalid, float (&acc)[QF], float (&mx)[QF]) {
    if (nvalid == 64) {
#pragma unroll
        for (int i = 0; i < 64; i += 4) {
            const f32x4_t a = *reinterpret_cast<const f32x4_t*>(my + i);
#pragma unroll
            for (int j = 0; j < QF; ++j) {
                const float* bb = bq[j] + i;
                acc[j] = acc[j] + a.x * bb[0]; mx[j] = fmaxf(mx[j], fabsf(a.x - bb[0]));
                acc[j] = acc[j] + a.y * bb[1]; mx[j] = fmaxf(mx[j], fabsf(a.y - bb[1]));
                acc[j] = acc[j] + a.z * bb[2]; mx[j] = fmaxf(mx[j], fabsf(a.z - bb[2]));
                acc[j] = acc[j] + a.w * bb[3]; mx[j] = fmaxf(mx[j], fabsf(a.w - bb[3]));
            }
        }
    } else {
        for (uint32_t i = 0; i < nvalid; ++i) {
            const float a = my[i];
#pragma unroll
            for (int j = 0; j < QF; ++j) {
                const float bv = bq[j][i];
                acc[j] = acc[j] + a * bv;
                mx[j] = fmaxf(mx[j], fabsf(a - bv));
            }
        }
    }
}

// This wave's LDS stage for the candidate rows is private to it (W > 1 waves per workgroup
// each walk their own 64 candidates): ordering inside the wave is enough.
// The LDS executes one wave's operations in order, so only the compiler must not move LDS
// accesses across this point.  (A fence or __syncthreads would also wait for every global
// load in flight -- vmcnt(0) -- and serialise the two-chunk prefetch below.)
__device__ __forceinline__ void wave_sync() { asm volatile("" ::: "memory"); }

// A valid row without a tombstone (dead: the bitset of deleted rows, nullable; read for valid rows).
__device__ __forceinline__ bool row_live(const uint64_t* dead, uint64_t row, bool valid) {
    const uint32_t dw = valid && dead ? reinterpret_cast<const uint32_t*>(dead)[row >> 5] : 0u;
    return valid && !((dw >> (row & 31)) & 1u);
}

// One wave's exact walk of 64 rows against one vector (k_range_rescore, k_score_ids, k_groups_fill):
// lane l's row myrow (any row below n_pad) goes chunk by chunk through the wave's own LDS stage `lds`
// (64 x 68 floats; load_cand_chunk, two chunks in flight) and the lane walks it in index order
// (seq_chunk) against qv -- the vector's ld floats, in LDS or in global memory.  acc and mx: the
// sequential dot and max|a_i - b_i| that finish_distance takes.
__device__ __forceinline__ void wave_walk_rows(float* lds, const float* __restrict__ rows, uint32_t ld, uint32_t dim,
                                               uint32_t myrow, const float* qv, int lane, float (&acc)[1],
                                               float (&mx)[1]) {
    const uint32_t nch = ld / 64;
    uint32_t lrow[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) lrow[i] = (uint32_t)__shfl((int)myrow, (i * 64 + lane) >> 4, kWave);
    auto step = [&](f32x4_t (&pre)[16], uint32_t ch) {
        wave_sync();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int L16 = i * 64 + lane;
            *reinterpret_cast<f32x4_t*>(lds + (L16 >> 4) * 68 + (L16 & 15) * 4) = pre[i];
        }
        wave_sync();
        if (ch + 2 < nch) load_cand_chunk(pre, rows, ld, lrow, ch + 2, lane);
        const float* const bb[1] = {qv + ch * 64};
        const uint32_t nvalid = dim - ch * 64 < 64 ? dim - ch * 64 : 64;
        seq_chunk<1>(lds + lane * 68, bb, nvalid, acc, mx);
    };
    f32x4_t preA[16], preB[16];
    load_cand_chunk(preA, rows, ld, lrow, 0, lane);
    if (nch > 1) load_cand_chunk(preB, rows, ld, lrow, 1, lane);
    for (uint32_t ch = 0; ch < nch; ch += 2) {
        step(preA, ch);
        if (ch + 1 < nch) step(preB, ch + 1);
    }
}

// A key into the m entries of its (query slot, group): after every insert has ended the entries
// hold the m smallest keys inserted, in no order, whatever the interleaving.  Each atomic min either
// leaves the entry and carries v on, or puts v in and carries the old value on, so a key ends in an
// entry or is carried off the end; a carried value passed an entry only while it was above it, and
// entries only fall, so every dropped key is above every final entry.  The plain reads ahead only
// skip a key that is below no entry (a stale read is not lower than the entry: it costs atomics,
// never a key).
__device__ __forceinline__ void cap_insert(unsigned long long* e, uint32_t m, uint64_t key) {
    bool below = false;
    for (uint32_t s = 0; s < m; ++s) below |= key < e[s];
    if (!below) return;
    unsigned long long v = key;
    for (uint32_t s = 0; s < m; ++s) {
        const unsigned long long old = atomicMin(&e[s], v);
        if (old == kKeyNone) break;
        v = old > v ? old : v;
    }
}

}  // namespace bsr
