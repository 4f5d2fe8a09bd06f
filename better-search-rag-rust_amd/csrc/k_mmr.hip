// k_mmr.hip -- deep MMR selection (bsr_local_top_k_deep_mmr) on gfx950: k of a
// query's m <= 1024 exact candidates picked greedily, the pair distances computed lazily.
//
// Compiled like k_exact.hip (-ffp-contract=off, correctly rounded divide and sqrt): the pair
// distances are the reference's arithmetic (load_cand_chunk, seq_chunk, finish_distance, the stored
// magnitudes), the score the three rounded f32 operations of k_mmr_select.
#include <cstdlib>
#include "bsr_device.hpp"
#include "exact_walk.hpp"
#include "kernels.hpp"

#include <math.h>

namespace bsr {

namespace {

// wave_walk_rows against QF vectors at once: lane l's row goes chunk by chunk through the wave's LDS
// stage (two chunks in flight) and the lane walks it in index order against qv[0 .. QF), each with
// its own sequential dot and max |a_i - b_i|.
template <int QF>
__device__ __forceinline__ void mmr_walk(float* lds, const float* __restrict__ rows, uint32_t ld, uint32_t dim,
                                         uint32_t myrow, const float* const (&qv)[QF], int lane, float (&acc)[QF],
                                         float (&mx)[QF]) {
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
        const float* bb[QF];
#pragma unroll
        for (int j = 0; j < QF; ++j) bb[j] = qv[j] + ch * 64;
        const uint32_t nvalid = dim - ch * 64 < 64 ? dim - ch * 64 : 64;
        seq_chunk<QF>(lds + lane * 68, bb, nvalid, acc, mx);
    };
    f32x4_t preA[16], preB[16];
    load_cand_chunk(preA, rows, ld, lrow, 0, lane);
    if (nch > 1) load_cand_chunk(preB, rows, ld, lrow, 1, lane);
    for (uint32_t ch = 0; ch < nch; ch += 2) {
        step(preA, ch);
        if (ch + 1 < nch) step(preB, ch + 1);
    }
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {  // set bits of mask below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

}  // namespace

// One workgroup of four waves per query.  The state of candidate position c lives in LDS: its local
// row, dq, mind, upto -- the picks 0 .. upto-1 are folded into mind -- and its key, score_key(score,
// c) of the score formed from that mind: kKeyNone for a picked position or no candidate, the bare
// position (below every score's key) while upto = 0, so that "absorbed nothing" is never a computed
// score.  mind only falls, every operation of the score is monotone in it, so a key formed at upto
// < t is at most the key the candidate would have at upto = t (smaller keys are better scores).
// Pick t, in rounds:
//   1. bc = the smallest key of the current candidates (upto >= t); the stale candidates whose key
//      is below bc are the only ones that can still win.  None: bc is the pick -- every other
//      candidate's current key is at least its stale key, which is above bc.
//   2. Of those, the B with the smallest keys are selected (all, when they are at most B): a radix
//      select over the keys' score words, 8 bits a pass through a 256-bin LDS histogram, ties at the
//      threshold and the slot order by position.  B = 64 in the first round of a pick after the
//      second -- the head of the order is what usually decides -- and 256 in the others.
//   3. Wave w owns the selected candidates w*64 .. w*64 + 63, a lane one of them.  The picks the
//      selected candidates miss are [b0, t), b0 their smallest upto; they are staged J = 4 rows at a
//      time in LDS (longer rows than 1024 floats are read from global memory), and every lane that
//      misses a pick of the window walks its row once against the window's rows (mmr_walk) and folds
//      the distances to the picks it misses into mind.  A lane that misses none walks the row of a
//      lane that does (a cache hit) and drops the result; a wave of such lanes skips the walk.
//   4. The refreshed candidates get upto = t and their key, and the round starts over.
// Every round makes a stale candidate current, so a pick ends; pick 0 is the lowest position (every
// key is its position).  The distances folded in are counted per lane and added once per workgroup
// to *a.pairs.
__global__ __launch_bounds__(256) void k_mmr_deep_select(MmrDeepArgs a) {
    constexpr int W = 4, J = 4, STAGE = 64 * 68, QMAX = 1024;
    constexpr uint32_t M = kMmrDeepMaxFetch, PER = M / 256, NC = PER * W;
    __shared__ __attribute__((aligned(16))) float lds_all[W * STAGE + J * QMAX];
    __shared__ uint64_t c_key[M];
    __shared__ uint32_t c_row[M], c_upto[M];
    __shared__ float c_dq[M], c_mind[M];
    __shared__ uint32_t p_row[kMmrDeepMaxPicks];
    __shared__ float p_na[kMmrDeepMaxPicks];
    __shared__ uint32_t sel[256], hist[256];
    __shared__ uint64_t s_best[W];
    __shared__ uint32_t s_q[NC], s_lt[NC], s_eq[NC], s_umin[W];
    __shared__ uint32_t s_bin, s_below, s_bucket, s_pairs;
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    float* const lds = lds_all + w * STAGE;
    float* const ldp = lds_all + W * STAGE;
    const uint32_t q = blockIdx.x;
    const uint32_t ld = a.ld, dim = a.dim, k = a.k, fk = a.fetch_k;
    const uint32_t m = a.cand_cnt[q] < fk ? a.cand_cnt[q] : fk;
    const float lam = a.lambda, mu = 1.0f - lam;
    const bool qlds = ld <= (uint32_t)QMAX;
    const float* const rows = a.rows;
    uint64_t* const oi = a.out_idx + (uint64_t)q * k;
    float* const od = a.out_dist + (uint64_t)q * k;
    uint32_t* const orank = a.out_rank ? a.out_rank + (uint64_t)q * k : nullptr;

#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) {
        const uint32_t c = i * 256 + tid;
        const uint64_t gidx = c < m ? a.cand_idx[(uint64_t)q * fk + c] : ~0ull;
        // (an id outside the shard is no candidate: no row is read through it)
        const bool valid = c < m && gidx >= a.offset && gidx - a.offset < a.n;
        c_row[c] = valid ? (uint32_t)(gidx - a.offset) : 0u;
        c_dq[c] = valid ? a.cand_dist[(uint64_t)q * fk + c] : INFINITY;
        c_mind[c] = INFINITY;
        c_upto[c] = 0;
        c_key[c] = valid ? (uint64_t)c : kKeyNone;
    }
    if (tid == 0) s_pairs = 0;
    __syncthreads();

    uint32_t npairs = 0, t = 0;
    for (; t < k; ++t) {
        uint64_t bc;
        for (uint32_t round = 0;; ++round) {
            // 1. the best current key, and the stale candidates below it
            uint64_t wb = kKeyNone;
#pragma unroll
            for (uint32_t i = 0; i < PER; ++i) {
                const uint32_t c = i * 256 + tid;
                const uint64_t key = c_key[c];
                if (c_upto[c] >= t && key < wb) wb = key;
            }
#pragma unroll
            for (int j = 32; j > 0; j >>= 1) {
                const uint64_t y = shfl_xor64(wb, j);
                wb = y < wb ? y : wb;
            }
            if (lane == 0) s_best[w] = wb;
            __syncthreads();
            bc = s_best[0];
#pragma unroll
            for (int i = 1; i < W; ++i) bc = s_best[i] < bc ? s_best[i] : bc;
            bool ql[PER];
            uint32_t hi[PER];
#pragma unroll
            for (uint32_t i = 0; i < PER; ++i) {
                const uint32_t c = i * 256 + tid;
                const uint64_t key = c_key[c];
                ql[i] = key < bc && c_upto[c] < t;
                hi[i] = (uint32_t)(key >> 32);
                const uint64_t bl = __ballot(ql[i]);
                if (lane == 0) s_q[i * W + w] = (uint32_t)__popcll(bl);
            }
            __syncthreads();
            uint32_t total = 0;
#pragma unroll
            for (uint32_t j = 0; j < NC; ++j) total += s_q[j];
            if (total == 0) break;  // (uniform over the workgroup: bc is the pick, or nothing is left)

            // 2. the B smallest of their keys: the threshold's `fixed` high bits of the score word
            const uint32_t B = (round == 0 && t > 1) ? 64u : 256u;
            uint32_t fixed = 0, prefix = 0, below = 0, live = total;
            while (below + live > B && fixed < 32) {
                const uint32_t shift = 24u - fixed;
                hist[tid] = 0;
                __syncthreads();
#pragma unroll
                for (uint32_t i = 0; i < PER; ++i)
                    if (ql[i] && (fixed == 0 || (hi[i] >> (32u - fixed)) == prefix))
                        atomicAdd(&hist[(hi[i] >> shift) & 255u], 1u);
                __syncthreads();
                if (w == 0) {  // the bin that holds the key of rank `need` in the live bucket
                    const uint32_t need = B - below;
                    uint32_t h[4], sum = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) sum += h[b] = hist[lane * 4 + b];
                    uint32_t incl = sum;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t v = (uint32_t)__shfl_up((int)incl, d, kWave);
                        if (lane >= d) incl += v;
                    }
                    uint32_t run = incl - sum;
                    if (run < need && need <= incl) {  // (one lane: the scan is monotone)
                        bool done = false;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            if (!done && run + h[b] >= need) {
                                s_bin = (uint32_t)lane * 4 + b;
                                s_below = run;
                                s_bucket = h[b];
                                done = true;
                            }
                            if (!done) run += h[b];
                        }
                    }
                }
                __syncthreads();
                prefix = (prefix << 8) | s_bin;
                fixed += 8;
                below += s_below;
                live = s_bucket;
            }
            // the keys under the threshold's bucket, then the bucket's, each in position order
            uint64_t blt[PER], beq[PER];
#pragma unroll
            for (uint32_t i = 0; i < PER; ++i) {
                const uint32_t pf = fixed ? hi[i] >> (32u - fixed) : 0u;
                blt[i] = __ballot(ql[i] && pf < prefix);
                beq[i] = __ballot(ql[i] && pf == prefix);
                if (lane == 0) {
                    s_lt[i * W + w] = (uint32_t)__popcll(blt[i]);
                    s_eq[i * W + w] = (uint32_t)__popcll(beq[i]);
                }
            }
            __syncthreads();
            uint32_t run_lt = 0, run_eq = 0, base_lt[PER], base_eq[PER];
#pragma unroll
            for (uint32_t j = 0; j < NC; ++j) {
                if ((int)(j % W) == w) {
                    base_lt[j / W] = run_lt;
                    base_eq[j / W] = run_eq;
                }
                run_lt += s_lt[j];
                run_eq += s_eq[j];
            }
            const uint32_t nsel = run_lt + run_eq < B ? run_lt + run_eq : B;
#pragma unroll
            for (uint32_t i = 0; i < PER; ++i) {
                const bool lt = (blt[i] >> lane) & 1ull, eq = (beq[i] >> lane) & 1ull;
                const uint32_t slot = lt ? base_lt[i] + lanes_below(blt[i]) : run_lt + base_eq[i] + lanes_below(beq[i]);
                if ((lt || eq) && slot < B) sel[slot] = i * 256 + tid;
            }
            __syncthreads();

            // 3. bring the selected candidates up to date
            const uint32_t si = (uint32_t)w * 64 + lane;
            const bool act = si < nsel;
            const uint32_t c = act ? sel[si] : 0u;
            uint32_t u = act ? c_upto[c] : t;
            const uint32_t r = act ? c_row[c] : 0u;
            float mind = act ? c_mind[c] : 0.0f;
            const float mag_a = act ? a.na[r] : 0.0f;
            const uint32_t wu = wave_reduce_u32(u, [](uint32_t x, uint32_t y) { return x < y ? x : y; });
            if (lane == 0) s_umin[w] = wu;
            __syncthreads();
            uint32_t b0 = s_umin[0];
#pragma unroll
            for (int i = 1; i < W; ++i) b0 = s_umin[i] < b0 ? s_umin[i] : b0;
            for (uint32_t b = b0; b < t; b += J) {
                const uint32_t nj = t - b < (uint32_t)J ? t - b : (uint32_t)J;
                if (qlds)
                    for (uint32_t j = 0; j < nj; ++j) {
                        const float* const pg = rows + (uint64_t)p_row[b + j] * ld;
                        for (uint32_t cc = tid; cc < ld; cc += 64 * W) ldp[j * QMAX + cc] = pg[cc];
                    }
                __syncthreads();
                const bool need = act && u < b + nj;
                const uint64_t nm = __ballot(need);
                if (nm) {  // (a wave that misses no pick of the window skips the walk, not the barriers)
                    const uint32_t other = (uint32_t)__shfl((int)r, __builtin_ctzll(nm), kWave);
                    const uint32_t wr = need ? r : other;
                    auto vec = [&](uint32_t j) {  // (a window of fewer than J picks repeats its last)
                        const uint32_t jj = j < nj ? j : nj - 1;
                        return qlds ? (const float*)(ldp + jj * QMAX) : rows + (uint64_t)p_row[b + jj] * ld;
                    };
                    auto fold = [&](uint32_t j, float dot, float maxdiff) {
                        if (need && j < nj && b + j >= u) {
                            mind = fminf(mind, finish_distance(dot, maxdiff, mag_a, p_na[b + j]));
                            ++npairs;
                        }
                    };
                    if (nj == 1) {
                        float acc[1] = {-0.0f}, mx[1] = {0.0f};
                        const float* const qv[1] = {vec(0)};
                        mmr_walk<1>(lds, rows, ld, dim, wr, qv, lane, acc, mx);
                        fold(0, acc[0], mx[0]);
                    } else {
                        float acc[J] = {-0.0f, -0.0f, -0.0f, -0.0f}, mx[J] = {0.0f, 0.0f, 0.0f, 0.0f};
                        const float* const qv[J] = {vec(0), vec(1), vec(2), vec(3)};
                        mmr_walk<J>(lds, rows, ld, dim, wr, qv, lane, acc, mx);
#pragma unroll
                        for (int j = 0; j < J; ++j) fold(j, acc[j], mx[j]);
                    }
                    if (need) u = b + nj;
                }
                __syncthreads();  // (the next window restages the picked rows)
            }
            // 4. the refreshed state and key
            if (act) {
                c_mind[c] = mind;
                c_upto[c] = t;
                const float gain = mu * mind, cost = lam * c_dq[c];
                c_key[c] = score_key(gain - cost, c);
            }
            __syncthreads();
        }
        if (bc == kKeyNone) break;  // (uniform over the workgroup: no candidate is left)
        if (tid == 0) {
            const uint32_t pos = (uint32_t)bc, pr = c_row[pos];
            p_row[t] = pr;
            p_na[t] = a.na[pr];
            oi[t] = a.cand_idx[(uint64_t)q * fk + pos];
            od[t] = c_dq[pos];
            if (orank) orank[t] = pos;
            c_key[pos] = kKeyNone;
        }
        __syncthreads();
    }
    // (t picks were made: the count, the padding behind them, the distances this workgroup computed)
    if (tid == 0) a.out_count[q] = t;
    for (uint32_t i = t + tid; i < k; i += 64 * W) {
        oi[i] = ~0ull;
        od[i] = INFINITY;
        if (orank) orank[i] = ~0u;
    }
    if (a.pairs) {
        const uint32_t wp = wave_reduce_u32(npairs, [](uint32_t x, uint32_t y) { return x + y; });
        if (lane == 0) atomicAdd(&s_pairs, wp);
        __syncthreads();
        if (tid == 0) atomicAdd(a.pairs, (unsigned long long)s_pairs);
    }
}

hipError_t launch_mmr_deep_select(const MmrDeepArgs& a, hipStream_t s) {
    if (!a.nq || !a.k || a.k > a.fetch_k || a.k > kMmrDeepMaxPicks || a.fetch_k > kMmrDeepMaxFetch || a.ld == 0 ||
        a.ld % 64 != 0 || !(a.lambda >= 0.0f && a.lambda <= 1.0f))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mmr_deep_select, dim3(a.nq), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace bsr
