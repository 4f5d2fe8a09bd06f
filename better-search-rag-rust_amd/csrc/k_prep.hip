// k_prep.hip -- data movement and preparation kernels (gfx950): synthetic data, the padded
// f32 slab, the reference's exact magnitudes, and the MFMA filter operands (int8)
// of corpus rows and queries together with their certification error bounds.
//
// Compiled with -ffp-contract=off: the magnitudes reproduce src/metrics.rs:154-155 (a
// sequential f32 sum of squares in index order, then a correctly rounded sqrt).  The
// filter operands are approximations whose error is measured here, in double precision,
// and carried to the certification step.
#include "bsr_device.hpp"
#include "kernels.hpp"

#include <math.h>

#include <algorithm>

namespace bsr {

// ------------------------------------------------------------------------------------
// Synthetic data: value(row, col) = U[-1,1) from splitmix64(seed, row*dim + col), 24 bits.
// ------------------------------------------------------------------------------------
__global__ void k_synth_uniform(float* __restrict__ out, uint64_t row0, uint64_t n_rows,
                                uint32_t dim, uint32_t ld, uint64_t seed) {
    const uint64_t total = n_rows * (uint64_t)ld;
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < total;
         e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = e / ld;
        const uint32_t c = (uint32_t)(e - r * ld);
        float v = 0.0f;
        if (c < dim) {
            const uint64_t g = (row0 + r) * (uint64_t)dim + c;
            const uint64_t h = splitmix64(seed * 0xD1B54A32D192ED03ull + g);
            v = (float)(h >> 40) * (1.0f / 8388608.0f) - 1.0f;  // 24-bit grid on [-1, 1)
        }
        out[e] = v;
    }
}

// Dense copy into the padded [n][ld] layout (zeros in the pad columns).
__global__ void k_copy_rows_f32(const float* __restrict__ src, uint64_t n, uint32_t dim,
                                uint32_t ld, float* __restrict__ dst) {
    const uint64_t total = n * (uint64_t)ld;
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < total;
         e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = e / ld;
        const uint32_t c = (uint32_t)(e - r * ld);
        dst[e] = c < dim ? src[r * dim + c] : 0.0f;
    }
}

__global__ void k_widen_bf16_rows(const uint16_t* __restrict__ src, uint64_t n, uint32_t dim,
                                  uint32_t ld, float* __restrict__ dst) {
    const uint64_t total = n * (uint64_t)ld;
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < total;
         e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = e / ld;
        const uint32_t c = (uint32_t)(e - r * ld);
        dst[e] = c < dim ? bf16_to_f32(src[r * dim + c]) : 0.0f;
    }
}

// ------------------------------------------------------------------------------------
// Row magnitudes exactly as src/metrics.rs:154: sqrt of the sequential f32 sum of a_i*a_i.
// One lane per row (the per-row dependency chain is inherently serial), but the rows reach
// the lanes through LDS: each wave owns 64 consecutive rows and stages them 64 columns at a
// time with coalesced 16-byte loads (16 lanes per 256-byte row segment), then every lane
// walks its own row's staged segment in index order.  (Round 2's lane-per-row float4 loads
// touched 64 rows per wave-instruction and fetched 3.6x the slab.)  Requires ld % 64 == 0
// (rows zero-padded to ld, kLdAlign).
// ------------------------------------------------------------------------------------
// The body, shared with the update's k_upd_row_norms: the wave's 64 rows are slab rows row_of(0 ..
// 63) (row_of(i) < 0: no row), lane i's magnitude goes to na[row_of(i)].
template <class RowOf>
__device__ __forceinline__ void row_norms_wave(const float* __restrict__ rows, uint32_t dim, uint32_t ld,
                                               float* __restrict__ na, uint32_t* flags, float* t, RowOf row_of) {
    constexpr int kCols = 64, kPitch = kCols + 1;  // odd pitch: lane l reads bank (l + j) % 32
    const int lane = threadIdx.x & 63;
    float acc = -0.0f;
    bool bad = false;
    for (uint32_t c0 = 0; c0 < dim; c0 += kCols) {
        const uint32_t cw = dim - c0 < (uint32_t)kCols ? dim - c0 : (uint32_t)kCols;
        const uint32_t col = (lane & 15) * 4;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const uint32_t rr = i * 4 + (lane >> 4);
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const int64_t r = row_of(rr);
            if (r >= 0) v = *reinterpret_cast<const float4*>(rows + (uint64_t)r * ld + c0 + col);
            float* d = t + rr * kPitch + col;
            d[0] = v.x;
            d[1] = v.y;
            d[2] = v.z;
            d[3] = v.w;
        }
        __syncthreads();
        const float* a = t + lane * kPitch;
        for (uint32_t j = 0; j < cw; ++j) {
            const float x = a[j];
            bad |= !isfinite(x);
            acc = acc + x * x;
        }
        __syncthreads();
    }
    const int64_t r = row_of((uint32_t)lane);
    uint32_t f = 0;
    if (r >= 0) {
        const float m = __builtin_sqrtf(acc);
        na[r] = m;
        if (bad) f |= kRowNonFinite;
        if (!isfinite(m)) f |= kRowNormOvf;
        if (m != 0.0f && (m < 1e-18f || m > 1e18f)) f |= kRowNormRange;
    }
    const uint32_t any = __reduce_or_sync(~0ull, f);
    if (any && lane_id() == 0) atomicOr(flags, any);
}

__global__ __launch_bounds__(256) void k_row_norms(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                   uint32_t ld, float* __restrict__ na, uint32_t* flags) {
    __shared__ float tile[4][64 * 65];
    const int w = threadIdx.x >> 6;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + w) * 64;
    row_norms_wave(rows, dim, ld, na, flags, tile[w],
                   [&](uint32_t i) -> int64_t { return r0 + i < n ? (int64_t)(r0 + i) : -1; });
}

// ------------------------------------------------------------------------------------
// int8 filter operand.  One workgroup (4 waves) per block of 32 rows, the rows of one
// 32x32 MFMA accumulator block:
//   x = a / |a|                      (double; |a| = sqrt of the double sum of squares)
//   s = the smallest f32 >= max_block |x_i| / 127
//   q_i = rint(x_i / s) in [-127, 127]
//   e_row = || x - s q ||_2          (double), ea_max = max_row e_row rounded up to f32.
// By Cauchy-Schwarz |x.y - (s q).(t p)| <= e_row + e_q + e_row e_q for unit x, y, which is
// the row-side half of the certification bound.  Zero rows give q = 0 and e = 0 (the
// reference scores them 1.0 = cosine 0, which is exactly the filter's value).
// ------------------------------------------------------------------------------------
// (butterflies in the VALU: the partner's value by DPP / permlane moves, bsr_device.hpp)
__device__ __forceinline__ double xor_lane_f64(double v, int o) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = xor_lane32((uint32_t)u, o), hi = xor_lane32((uint32_t)(u >> 32), o);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += xor_lane_f64(v, o);
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, xor_lane_f64(v, o));
    return v;
}
// Smallest f32 >= x (x >= 0, finite).
__device__ __forceinline__ float f32_round_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}
__device__ __forceinline__ int8_t quant_i8(double x, double s) {
    double qd = rint(x / s);
    qd = fmin(127.0, fmax(-127.0, qd));
    return (int8_t)(int)qd;
}

// The workgroup's body for 32-row block blk, shared by the load (k_rows_to_i8: every block) and the
// update (k_upd_rows_to_i8: the touched blocks): what either writes for a block is the same bytes.
__device__ __forceinline__ void rows_to_i8_block(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                 uint32_t ld, int8_t* __restrict__ out,
                                                 float* __restrict__ scales, uint32_t* __restrict__ ea_max,
                                                 const uint64_t blk) {
    __shared__ double s_inv[kQuantBlock];
    __shared__ double s_wmax[4];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    constexpr int kRowsPerWave = kQuantBlock / 4;
    double wmax = 0.0;
    for (int i = 0; i < kRowsPerWave; ++i) {
        const int rl = w * kRowsPerWave + i;
        const uint64_t r = blk * kQuantBlock + rl;
        double ss = 0.0, mx = 0.0;
        if (r < n) {
            const float* a = rows + r * ld;
            for (uint32_t c = lane; c < dim; c += kWave) {
                const double x = a[c];
                ss += x * x;
                mx = fmax(mx, fabs(x));
            }
        }
        ss = wave_sum_f64(ss);
        mx = wave_max_f64(mx);
        const double inv = (ss > 0.0 && ss < 1e300) ? 1.0 / sqrt(ss) : 0.0;
        if (lane == 0) s_inv[rl] = inv;
        wmax = fmax(wmax, mx * inv);
    }
    if (lane == 0) s_wmax[w] = wmax;
    __syncthreads();
    const double bmax = fmax(fmax(s_wmax[0], s_wmax[1]), fmax(s_wmax[2], s_wmax[3]));
    const float sc = bmax > 0.0 ? f32_round_up(bmax / 127.0) : 1.0f;
    if (t == 0) scales[blk] = sc;
    const double s = sc;
    double ew = 0.0;
    for (int i = 0; i < kRowsPerWave; ++i) {
        const int rl = w * kRowsPerWave + i;
        const uint64_t r = blk * kQuantBlock + rl;
        const double inv = s_inv[rl];
        const float* a = rows + r * ld;
        double e2 = 0.0;
        for (uint32_t c0 = lane * 4; c0 < ld; c0 += 4 * kWave) {
            char4 v = make_char4(0, 0, 0, 0);
            int8_t qv[4] = {0, 0, 0, 0};
            if (r < n && inv > 0.0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t c = c0 + j;
                    if (c < dim) {
                        const double x = (double)a[c] * inv;
                        qv[j] = quant_i8(x, s);
                        const double d = x - s * (double)qv[j];
                        e2 += d * d;
                    }
                }
            }
            v.x = qv[0]; v.y = qv[1]; v.z = qv[2]; v.w = qv[3];
            *reinterpret_cast<char4*>(out + r * ld + c0) = v;
        }
        e2 = wave_sum_f64(e2);
        ew = fmax(ew, sqrt(e2));
    }
    if (lane == 0) atomicMax(ea_max, __float_as_uint(f32_round_up(ew * (1.0 + 1e-9) + 1e-12)));
}

__global__ __launch_bounds__(256) void k_rows_to_i8(const float* __restrict__ rows, uint64_t n,
                                                    uint32_t dim, uint32_t ld,
                                                    int8_t* __restrict__ out,
                                                    float* __restrict__ scales,
                                                    uint32_t* __restrict__ ea_max) {
    rows_to_i8_block(rows, n, dim, ld, out, scales, ea_max, blockIdx.x);
}

// The sample operand: kSampleScaleRows sampled rows (corpus rows kSampleStride apart) per
// workgroup, one scale for all of them; rows past the corpus are zero.
// (the body for group blk, shared by k_rows_to_i8_sample and the update's k_upd_rows_to_i8_sample)
__device__ __forceinline__ void rows_to_i8_sample_group(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                        uint32_t ld, int8_t* __restrict__ out,
                                                        float* __restrict__ scales, const uint64_t blk) {
    __shared__ double s_inv[kSampleScaleRows];
    __shared__ double s_wmax[4];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    constexpr int kRowsPerWave = kSampleScaleRows / 4;
    double wmax = 0.0;
    for (int i = 0; i < kRowsPerWave; ++i) {
        const int rl = w * kRowsPerWave + i;
        const uint64_t r = (blk * kSampleScaleRows + rl) * kSampleStride;  // corpus row
        double ss = 0.0, mx = 0.0;
        if (r < n) {
            const float* a = rows + r * ld;
            for (uint32_t c = lane; c < dim; c += kWave) {
                const double x = a[c];
                ss += x * x;
                mx = fmax(mx, fabs(x));
            }
        }
        ss = wave_sum_f64(ss);
        mx = wave_max_f64(mx);
        const double inv = (ss > 0.0 && ss < 1e300) ? 1.0 / sqrt(ss) : 0.0;
        if (lane == 0) s_inv[rl] = inv;
        wmax = fmax(wmax, mx * inv);
    }
    if (lane == 0) s_wmax[w] = wmax;
    __syncthreads();
    const double bmax = fmax(fmax(s_wmax[0], s_wmax[1]), fmax(s_wmax[2], s_wmax[3]));
    const float sc = bmax > 0.0 ? f32_round_up(bmax / 127.0) : 1.0f;
    if (t == 0) scales[blk] = sc;
    const double s = sc;
    for (int i = 0; i < kRowsPerWave; ++i) {
        const int rl = w * kRowsPerWave + i;
        const uint64_t rs = blk * kSampleScaleRows + rl;  // sample row
        const uint64_t r = rs * kSampleStride;
        const double inv = s_inv[rl];
        const float* a = rows + r * ld;
        for (uint32_t c0 = lane * 4; c0 < ld; c0 += 4 * kWave) {
            int8_t qv[4] = {0, 0, 0, 0};
            if (r < n && inv > 0.0) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < dim) qv[j] = quant_i8((double)a[c0 + j] * inv, s);
            }
            *reinterpret_cast<char4*>(out + rs * ld + c0) = make_char4(qv[0], qv[1], qv[2], qv[3]);
        }
    }
}

__global__ __launch_bounds__(256) void k_rows_to_i8_sample(const float* __restrict__ rows, uint64_t n,
                                                           uint32_t dim, uint32_t ld, int8_t* __restrict__ out,
                                                           float* __restrict__ scales) {
    rows_to_i8_sample_group(rows, n, dim, ld, out, scales, blockIdx.x);
}

// ------------------------------------------------------------------------------------
// Queries: one workgroup of two waves per (padded) query, the whole preparation in one kernel.
//   1. the caller's row -> LDS (coalesced) and the padded f32 copy qf32[q] (zeros past dim)
//   2. wave 0's lane 0 walks the row in index order: |b| exactly as src/metrics.rs:155 (sequential
//      f32 sum of squares from -0.0, correctly rounded sqrt), finiteness
//   3. flags, the identity query-id list of the exact scan (min(q, nq-1))
//   4. the int8 filter operand from the LDS copy: x = b/|b| (double), s = smallest f32 >=
//      max|x_i|/127, q_i = rint(x_i/s), eb = ||x - s q||_2, E_q = ea + eb + ea*eb + 1.5e-4 (ea:
//      the row side; 1.5e-4 covers the reference's own f32 rounding, <= 9.3e-5, and the two f32
//      roundings of the filter's score)
//      queries the filter cannot serve (pad, zero/tiny/huge |b|) get a zero operand and
//      E_q = inf.
// ------------------------------------------------------------------------------------
constexpr uint32_t kQueryLdsFloats = 8192;  // rows up to 8192 floats are staged in LDS

// Steps 2 and 4 (int8) overlap: while wave 0's lane 0 walks the exact |b| (the reference's
// dependent chain of f32 adds), wave 1 quantises the row to int8 (double precision) into
// registers; the result is kept only if |b| admits the filter (else zeros, E_q = inf).
__global__ __launch_bounds__(128) void k_query_prep(const float* __restrict__ q, uint32_t nq, uint32_t dim,
                                                    uint32_t ld, bool with_op,
                                                    const uint32_t* __restrict__ ea_max,
                                                    float* __restrict__ qf32, float* __restrict__ nb,
                                                    void* __restrict__ qop, float* __restrict__ qscale,
                                                    float* __restrict__ ebound, uint32_t* __restrict__ qflags,
                                                    int32_t* __restrict__ qids, uint32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) float row[kQueryLdsFloats];
    __shared__ uint32_t s_flags;
    __shared__ uint32_t s_bad;
    const uint32_t qi = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const bool real = qi < nq;
    const bool staged = ld <= kQueryLdsFloats;
    const float* src = q + (uint64_t)qi * dim;
    float* dst = qf32 + (uint64_t)qi * ld;
    if (t == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    // 8 loads per thread in flight, then their stores (rows up to 1024 floats: one round)
    constexpr int B = 8;
    for (uint32_t c0 = 0; c0 < ld; c0 += B * 128) {
        float v[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const uint32_t c = c0 + j * 128 + t;
            v[j] = (real && c < dim) ? src[c] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const uint32_t c = c0 + j * 128 + t;
            if (c < ld) {
                bad |= !isfinite(v[j]);
                dst[c] = v[j];
                if (staged) row[c] = v[j];
            }
        }
    }
    if (__ballot(bad) != 0 && lane == 0) s_bad = 1;
    __syncthreads();
    bad = s_bad != 0;
    auto val = [&](uint32_t c) -> float { return staged ? row[c] : dst[c]; };
    const bool i8 = with_op;
    // wave 1 (int8 operand): the quantisation, speculatively, into registers
    constexpr int QV = 4;  // char4 groups per lane held (rows up to 1024 int8); longer rows: second pass
    char4 qv[QV];
    double e2 = 0.0;
    float sc = 1.0f;
    if (w == 1 && i8) {
        double ss = 0.0, mx = 0.0;
        if (real && !bad) {
            for (uint32_t c = lane; c < dim; c += kWave) {
                const double x = val(c);
                ss += x * x;
                mx = fmax(mx, fabs(x));
            }
        }
        ss = wave_sum_f64(ss);
        mx = wave_max_f64(mx);
        const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
        sc = (mx > 0.0 && inv > 0.0) ? f32_round_up(mx * inv / 127.0) : 1.0f;
        const double sd = sc;
        for (uint32_t g = 0, c0 = lane * 4; c0 < ld; ++g, c0 += 4 * kWave) {
            int8_t qq[4] = {0, 0, 0, 0};
            if (inv > 0.0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t c = c0 + j;
                    if (c < dim) {
                        const double x = (double)val(c) * inv;
                        qq[j] = quant_i8(x, sd);
                        const double d = x - sd * (double)qq[j];
                        e2 += d * d;
                    }
                }
            }
            const char4 v4 = make_char4(qq[0], qq[1], qq[2], qq[3]);
            if (g < (uint32_t)QV) qv[g] = v4;
            else *reinterpret_cast<char4*>(static_cast<int8_t*>(qop) + (uint64_t)qi * ld + c0) = v4;
        }
        e2 = wave_sum_f64(e2);
    }
    if (t == 0) {
        // the reference's sequential sum, 16 elements per step from 4 ds_read_b128
        float acc = -0.0f;
        uint32_t i = 0;
        if (real && staged) {
            const float4* r4 = reinterpret_cast<const float4*>(row);
            for (; i + 16 <= dim; i += 16) {
                const float4 x0 = r4[i / 4], x1 = r4[i / 4 + 1], x2 = r4[i / 4 + 2], x3 = r4[i / 4 + 3];
                acc = acc + x0.x * x0.x; acc = acc + x0.y * x0.y; acc = acc + x0.z * x0.z; acc = acc + x0.w * x0.w;
                acc = acc + x1.x * x1.x; acc = acc + x1.y * x1.y; acc = acc + x1.z * x1.z; acc = acc + x1.w * x1.w;
                acc = acc + x2.x * x2.x; acc = acc + x2.y * x2.y; acc = acc + x2.z * x2.z; acc = acc + x2.w * x2.w;
                acc = acc + x3.x * x3.x; acc = acc + x3.y * x3.y; acc = acc + x3.z * x3.z; acc = acc + x3.w * x3.w;
            }
        }
        if (real)
            for (; i < dim; ++i) {
                const float x = staged ? row[i] : src[i];
                acc = acc + x * x;
            }
        const float m = __builtin_sqrtf(acc);
        const bool approx_ok = real && !bad && isfinite(m) && m >= 1e-18f && m <= 1e18f;
        const uint32_t f = real ? ((bad ? kQueryNonFinite : 0u) | (approx_ok ? 0u : kQueryNoApprox)) : kQueryNoApprox;
        nb[qi] = real ? m : 0.0f;
        qflags[qi] = f;
        qids[qi] = (int32_t)(real ? qi : (nq ? nq - 1 : 0));
        if (f & kQueryNonFinite) atomicOr(status + kStQueryFlags, kQueryNonFinite);
        s_flags = f;
    }
    __syncthreads();
    const bool ok = !(s_flags & kQueryNoApprox);
    if (!with_op || w != 1) return;
    // wave 1: keep the speculative operand (the filter serves this query) or zero it
    int8_t* o = static_cast<int8_t*>(qop) + (uint64_t)qi * ld;
    for (uint32_t g = 0, c0 = lane * 4; c0 < ld; ++g, c0 += 4 * kWave) {
        if (g < (uint32_t)QV) *reinterpret_cast<char4*>(o + c0) = ok ? qv[g] : make_char4(0, 0, 0, 0);
        else if (!ok) *reinterpret_cast<char4*>(o + c0) = make_char4(0, 0, 0, 0);
    }
    if (lane == 0) {
        qscale[qi] = ok ? sc : 0.0f;
        if (ok) {
            const double ea = (double)__uint_as_float(*ea_max);
            const double eb = sqrt(e2) * (1.0 + 1e-9) + 1e-12;
            ebound[qi] = f32_round_up(ea + eb + ea * eb + 1.5e-4);
        } else {
            ebound[qi] = INFINITY;
        }
    }
}

// ------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------
static inline uint32_t grid_for(uint64_t work, uint32_t block, uint32_t cap = 65536) {
    uint64_t g = (work + block - 1) / block;
    if (g < 1) g = 1;
    return (uint32_t)(g > cap ? cap : g);
}

// ------------------------------------------------------------------------------------
// The loopback communicator's all-gather (bsr_comm_init_loopback): slot r of
// recv [P][bytes] receives this rank's `send` (r == rank, or every slot when there is no
// script) or the recorded contribution script[r] of a real P-rank run -- one launch on the
// stream where ncclAllGather would sit, no host wait.  bytes % 4 == 0.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gather_emulate(const uint32_t* __restrict__ send,
                                                        const uint32_t* __restrict__ script,
                                                        uint32_t* __restrict__ recv, uint64_t words,
                                                        uint32_t P, uint32_t rank) {
    const uint64_t total = words * P;
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < total;
         e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(e / words);
        const uint64_t i = e - (uint64_t)r * words;
        recv[e] = (script && r != rank) ? script[e] : send[i];
    }
}

// ------------------------------------------------------------------------------------
// The parallel search's header exchange without host copies (round 5): k_header_put writes this
// rank's 8 words (kernel arguments) into the device send buffer; after the all-gather,
// k_header_publish copies the P received headers into fine-grained pinned host memory with
// system-scope stores, releases them at system scope and then stores the search's sequence
// number into the host flag the host polls.  (Small hipMemcpyAsync copies to and from pinned
// memory return only when they are done: the header's two copies held the host's enqueue of
// phase A / phase B for their round trip.)
// ------------------------------------------------------------------------------------
struct HeaderWords { int32_t w[8]; };
__global__ void k_header_put(HeaderWords h, int32_t* __restrict__ dst) {
    if (threadIdx.x < 8) dst[threadIdx.x] = h.w[threadIdx.x];
}
__global__ __launch_bounds__(256) void k_header_publish(const int32_t* __restrict__ src, uint32_t words,
                                                        int32_t* host, uint32_t* host_flag, uint32_t seq) {
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x)
        __hip_atomic_store(host + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------------
// Mask bitsets: an allow mask as a list of row ids, and the emitted lists cut
// by a mask.  Bit (i & 63) of word (i >> 6) allows local row i; bits at positions >= n are
// ignored.  One family serves the masked search (one mask), the grouped masked search (n_masks
// masks of `words` words each, gridDim.y or the query picking one), the live-row list (no allow
// mask: every row) and the update's block bitsets; the index's tombstones (dead, nullable) are
// taken out as the words are read -- no copy of a mask is ever made.  A list is built in three
// deterministic steps -- per-block popcounts (a block = kMaskBlockWords words), one workgroup's
// exclusive scan of them per mask, a scatter -- so the ids come out ascending: the list scan then
// walks the slab front to back.
// ------------------------------------------------------------------------------------
// The one reader of a bitset word: the rows of word w that are allowed (allow = nullptr: every
// row < n) and not deleted (dead = nullptr: none is).
__device__ __forceinline__ uint64_t mask_bits(const uint64_t* __restrict__ allow, const uint64_t* __restrict__ dead,
                                              uint64_t w, uint64_t n) {
    const uint64_t lo = w * 64;
    if (lo >= n) return 0;
    uint64_t x = allow ? allow[w] : ~0ull;
    if (n - lo < 64) x &= (1ull << (n - lo)) - 1ull;
    return dead && x ? x & ~dead[w] : x;
}
__device__ __forceinline__ const uint64_t* mask_of(const uint64_t* allow, uint64_t g, uint64_t words) {
    return allow ? allow + g * words : nullptr;
}

// The workgroup's 256 per-thread counts: this thread's exclusive prefix, *total = their sum.
__device__ __forceinline__ uint32_t block_exclusive_256(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)inc, d, kWave);
        if (lane >= d) inc += y;
    }
    __syncthreads();  // (s_wave may still be read from an earlier call)
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t c = s_wave[i];
        before += i < w ? c : 0u;
        all += c;
    }
    *total = all;
    return before + inc - v;
}

// blockIdx.y = the mask: blk[y * stride + blockIdx.x] = the block's allowed live rows.
__global__ __launch_bounds__(256) void k_mask_count(const uint64_t* __restrict__ allow, uint64_t words, uint64_t n,
                                                    const uint64_t* __restrict__ dead, uint32_t* __restrict__ blk,
                                                    uint32_t stride) {
    __shared__ uint32_t s_wave[4];
    const uint64_t w = (uint64_t)blockIdx.x * kMaskBlockWords + threadIdx.x;
    uint32_t total;
    (void)block_exclusive_256((uint32_t)__popcll(mask_bits(mask_of(allow, blockIdx.y, words), dead, w, n)), s_wave, &total);
    if (threadIdx.x == 0) blk[(uint64_t)blockIdx.y * stride + blockIdx.x] = total;
}

// blockIdx.x = the mask g < n_masks: its row of blk, blk[0 .. n_blk) -> their exclusive prefix sums,
// blk[n_blk] = A_g, the number of its allowed rows, also out[g] (out nullable).  With a query_mask
// the launch has one more workgroup, blockIdx.x = n_masks: it counts the entries of query_mask that
// name no mask into out[n_masks] (the host refuses the call before any kernel indexes a mask with one).
__global__ __launch_bounds__(256) void k_mask_scan(uint32_t* __restrict__ blk_all, uint32_t n_blk, uint32_t n_masks,
                                                   const uint32_t* __restrict__ query_mask, uint32_t nq,
                                                   uint32_t* __restrict__ out) {
    __shared__ uint32_t s_wave[4];
    uint32_t carry = 0;
    if (blockIdx.x == n_masks) {
        for (uint32_t base = 0; base < nq; base += 256) {
            const uint32_t q = base + threadIdx.x;
            uint32_t total;
            (void)block_exclusive_256(q < nq && query_mask[q] >= n_masks ? 1u : 0u, s_wave, &total);
            carry += total;
        }
        if (threadIdx.x == 0) out[n_masks] = carry;
        return;
    }
    uint32_t* blk = blk_all + (uint64_t)blockIdx.x * (n_blk + 1);
    for (uint32_t base = 0; base < n_blk; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blk ? blk[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_256(v, s_wave, &total);
        if (i < n_blk) blk[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        blk[n_blk] = carry;
        if (out) out[blockIdx.x] = carry;
    }
}

// blockIdx.y = the list: the first n_list ids of mask me.mask, ascending, at list + me.off, with
// me = d[y], or -- d = nullptr, a single list -- the descriptor passed by value.
__global__ __launch_bounds__(256) void k_mask_scatter(const uint64_t* __restrict__ allow, uint64_t words, uint64_t n,
                                                      const uint64_t* __restrict__ dead,
                                                      const uint32_t* __restrict__ blk, uint32_t stride,
                                                      const MaskListDesc* __restrict__ d, MaskListDesc one,
                                                      uint32_t* __restrict__ list) {
    __shared__ uint32_t s_wave[4];
    const MaskListDesc me = d ? d[blockIdx.y] : one;
    const uint64_t w = (uint64_t)blockIdx.x * kMaskBlockWords + threadIdx.x;
    uint64_t x = mask_bits(mask_of(allow, me.mask, words), dead, w, n);
    uint32_t total;
    uint32_t pos = blk[(uint64_t)me.mask * stride + blockIdx.x] + block_exclusive_256((uint32_t)__popcll(x), s_wave, &total);
    uint32_t* out = list + me.off;
    while (x) {
        const uint32_t b = (uint32_t)__builtin_ctzll(x);
        x &= x - 1;
        if (pos < me.n_list) out[pos] = (uint32_t)(w * 64 + b);
        ++pos;
    }
}

// blockIdx.y = the segment (the masked range search): the ids of rank me.first ..
// me.first + me.n_list - 1 of mask me.mask, ascending, at list + me.off -- k_mask_scatter with a
// lower bound, so that a list longer than the chunk budget is built piece by piece.
__global__ __launch_bounds__(256) void k_mask_scatter_seg(const uint64_t* __restrict__ allow, uint64_t words,
                                                          uint64_t n, const uint64_t* __restrict__ dead,
                                                          const uint32_t* __restrict__ blk, uint32_t stride,
                                                          const MaskSegDesc* __restrict__ d,
                                                          uint32_t* __restrict__ list) {
    __shared__ uint32_t s_wave[4];
    const MaskSegDesc me = d[blockIdx.y];
    const uint64_t w = (uint64_t)blockIdx.x * kMaskBlockWords + threadIdx.x;
    uint64_t x = mask_bits(mask_of(allow, me.mask, words), dead, w, n);
    uint32_t total;
    uint32_t pos = blk[(uint64_t)me.mask * stride + blockIdx.x] + block_exclusive_256((uint32_t)__popcll(x), s_wave, &total);
    uint32_t* out = list + me.off;
    while (x) {
        const uint32_t b = (uint32_t)__builtin_ctzll(x);
        x &= x - 1;
        if (pos >= me.first && pos - me.first < me.n_list) out[pos - me.first] = (uint32_t)(w * 64 + b);
        ++pos;
    }
}

// One wave per query: cand[q][0 .. cnt[q]) compacted in place to the keys whose row the query's
// mask (query_mask[q]; query_mask = nullptr: mask 0 for every query) allows and no tombstone
// removes, cnt[q] rewritten; raw[q] keeps the emitted count.  A chunk of 64 keys is read before
// anything is written at or below it, so the compaction needs no second buffer.  An overflowed
// list (cnt[q] > cap: rows were dropped) is left as it is -- it must stay overflowed.  *items = nq
// (the device-counted rescore that follows reads its item count there).
__global__ __launch_bounds__(256) void k_mask_cut(uint64_t* __restrict__ cand, uint32_t* __restrict__ cnt,
                                                  uint32_t cap, uint32_t nq, const uint64_t* __restrict__ allow,
                                                  uint64_t words, const uint32_t* __restrict__ query_mask,
                                                  const uint64_t* __restrict__ dead, uint64_t n,
                                                  uint32_t* __restrict__ raw, uint32_t* __restrict__ items) {
    const int lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) *items = nq;
    if (q >= nq) return;
    const uint32_t c = cnt[q];
    if (lane == 0) raw[q] = c;
    if (c > cap) return;
    const uint64_t* mine = mask_of(allow, query_mask ? query_mask[q] : 0u, words);
    uint64_t* keys = cand + (uint64_t)q * cap;
    uint32_t out = 0;
    for (uint32_t base = 0; base < c; base += kWave) {
        const uint32_t i = base + lane;
        const uint64_t key = i < c ? keys[i] : kKeyNone;
        const uint32_t row = key_row(key);
        const bool keep = key != kKeyNone && ((mask_bits(mine, dead, row >> 6, n) >> (row & 63)) & 1ull);
        const uint64_t m = __ballot(keep);
        if (keep) keys[out + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = key;
        out += (uint32_t)__popcll(m);
    }
    if (lane == 0) cnt[q] = out;
}

// ------------------------------------------------------------------------------------
// Tombstones: the index's bitset of deleted rows -- bit (i & 63) of word (i >> 6)
// set = local row i is deleted; bits at positions >= n are never set.  A delete is two launches
// around the host's read of the first one's count: the check counts the ids outside
// [lo, lo + n) (all or nothing: the host applies nothing when there is one), the apply sets the
// bits and counts the rows that went live -> deleted (a duplicate, or a row deleted before, finds
// its bit set in the word atomicOr returns: counted once).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dead_check(const uint64_t* __restrict__ ids, uint64_t n_ids, uint64_t lo,
                                                    uint64_t n, uint32_t* __restrict__ bad) {
    uint32_t mine = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_ids; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t id = ids[i];
        mine += (id < lo || id - lo >= n) ? 1u : 0u;
    }
    mine = wave_reduce_u32(mine, [](uint32_t x, uint32_t y) { return x + y; });
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(bad, mine);
}

__global__ __launch_bounds__(256) void k_dead_apply(const uint64_t* __restrict__ ids, uint64_t n_ids, uint64_t lo,
                                                    uint64_t n, uint64_t* __restrict__ dead,
                                                    uint32_t* __restrict__ newly) {
    uint32_t mine = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_ids; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t id = ids[i];
        if (id < lo || id - lo >= n) continue;  // (the check found none: never taken)
        const uint64_t r = id - lo, bit = 1ull << (r & 63);
        const unsigned long long old = atomicOr(reinterpret_cast<unsigned long long*>(dead + (r >> 6)),
                                                (unsigned long long)bit);
        mine += (old & bit) ? 0u : 1u;
    }
    mine = wave_reduce_u32(mine, [](uint32_t x, uint32_t y) { return x + y; });
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(newly, mine);
}

// The filter operand of every deleted row zeroed, driven by the bitset: one wave per word of 64
// rows, its lanes writing 16-byte zeros along each deleted row of fop (row_bytes = ld, a multiple
// of 64).  A deleted row then scores exactly 0 in every filter kernel.  The fop_s sample holds one
// row per kSampleStride-row block, as loaded the block's first.  Every block with a deleted row
// gets its fop_s row rewritten so that the sample is the live rows thinned 1 in kSampleStride: it
// becomes the operand of the block's live row whose rank among the shard's live rows is a multiple
// of kSampleStride (at most one: a block has <= kSampleStride live rows of consecutive ranks) --
// quantized as k_rows_to_i8_sample quantizes, with the scale its group of sample rows already
// has, clamped to +-127 (the sample only places the threshold; no certification depends on it) --
// or zeros when the block has no such row.  dead_blk: launch_mask_list_count's prefix sums over
// the bitset itself, i.e. the deleted rows ahead of every kMaskBlockWords words.
__global__ __launch_bounds__(256) void k_dead_zero_fop(const uint64_t* __restrict__ dead, uint64_t n,
                                                       const uint32_t* __restrict__ dead_blk, uint32_t row_bytes,
                                                       uint8_t* __restrict__ fop, uint8_t* __restrict__ fop_s,
                                                       const float* __restrict__ rows, uint32_t dim,
                                                       const float* __restrict__ scales_s) {
    static_assert(kSampleStride == 32, "two sample blocks per word of the bitset");
    const int lane = threadIdx.x & 63;
    const uint64_t words = (n + 63) / 64;
    const uint32_t units = row_bytes / 16, ld = row_bytes;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < words; w += (uint64_t)gridDim.x * 4) {
        const uint64_t x0 = mask_bits(dead, nullptr, w, n);  // (wave-uniform)
        if (!x0) continue;
        uint64_t x = x0;
        while (x) {
            const uint32_t b = (uint32_t)__builtin_ctzll(x);
            x &= x - 1;
            uint4* row = reinterpret_cast<uint4*>(fop + (w * 64 + b) * row_bytes);
            for (uint32_t u = lane; u < units; u += kWave) row[u] = z;
        }
        // the deleted rows ahead of this word: those ahead of its block of words, plus the words between
        const uint64_t w0 = w / kMaskBlockWords * kMaskBlockWords;
        uint32_t before = 0;
        for (uint64_t v = w0 + lane; v < w; v += kWave) before += (uint32_t)__popcll(dead[v]);
        before = dead_blk[w / kMaskBlockWords] + wave_reduce_u32(before, [](uint32_t p, uint32_t q) { return p + q; });
        const uint64_t in_n = n - w * 64 >= 64 ? ~0ull : (1ull << (n - w * 64)) - 1ull;  // rows of the shard
        for (uint32_t j = 0; j < 2; ++j) {
            const uint64_t b0 = w * 64 + 32 * j;  // the block's first row
            const uint32_t gone = (uint32_t)(x0 >> (32 * j));
            if (b0 >= n || !gone) continue;
            uint32_t live = ~gone & (uint32_t)(in_n >> (32 * j));
            const uint64_t rank0 = b0 - before - (j ? (uint32_t)__popc((uint32_t)x0) : 0u);  // live rows ahead of b0
            uint32_t t = (uint32_t)((kSampleStride - rank0 % kSampleStride) % kSampleStride);
            const uint64_t rs = b0 / kSampleStride;  // sample row
            if (t >= (uint32_t)__popc(live)) {
                uint4* srow = reinterpret_cast<uint4*>(fop_s + rs * row_bytes);
                for (uint32_t u = lane; u < units; u += kWave) srow[u] = z;
                continue;
            }
            for (; t; --t) live &= live - 1;  // (its t-th live row)
            const float* a = rows + (b0 + (uint32_t)__builtin_ctz(live)) * (uint64_t)ld;
            double ss = 0.0;
            for (uint32_t c = lane; c < dim; c += kWave) {
                const double v = a[c];
                ss += v * v;
            }
            ss = wave_sum_f64(ss);
            const double inv = (ss > 0.0 && ss < 1e300) ? 1.0 / sqrt(ss) : 0.0;
            const double s = scales_s[rs / kSampleScaleRows];
            for (uint32_t c0 = lane * 4; c0 < ld; c0 += 4 * kWave) {
                int8_t qv[4] = {0, 0, 0, 0};
                if (inv > 0.0) {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
                        if (c0 + jj < dim) qv[jj] = quant_i8((double)a[c0 + jj] * inv, s);
                }
                *reinterpret_cast<char4*>(fop_s + rs * row_bytes + c0) = make_char4(qv[0], qv[1], qv[2], qv[3]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// In-place update (bsr_index_update): rows of the loaded shard replaced by id.  The
// check touches no stored byte; the scatter, the norms of the listed rows and the requantisation
// of the touched blocks and sample groups (from lists, ascending) follow only when it counted
// nothing.  Work: O(n_ids ld + touched blocks 32 ld + n / 64), no pass over the shard's rows.
// ------------------------------------------------------------------------------------
// The check, one launch.  The ids: cnt[kUpdBadId] += those outside [lo, lo + n); the bit of every
// other in `touched` (atomicOr; zeroed by the caller), cnt[kUpdDupId] += those that find it set;
// the first id of a 32-row block -- it finds the block's half of the word clear -- sets the
// block's bit in `blocks`; a row the fop_s sample reads (local index a multiple of kSampleStride)
// sets its group's bit in `groups` and counts in cnt[kUpdSampleRows].  The values: cnt[kUpdNonFinite]
// += the NaN / Inf among the n_vals incoming values (bf16: after widening, i.e. the same exponent
// test on the upper half), read 16 bytes at a time when vec (the base is 16-byte aligned).
template <bool BF16>
__global__ __launch_bounds__(256) void k_upd_check(const uint64_t* __restrict__ ids, uint64_t n_ids, uint64_t lo,
                                                   uint64_t n, const void* __restrict__ src, uint64_t n_vals, bool vec,
                                                   uint64_t* __restrict__ touched, uint64_t* __restrict__ blocks,
                                                   uint64_t* __restrict__ groups, unsigned long long* __restrict__ cnt) {
    static_assert(kSampleStride == kQuantBlock && kQuantBlock == 32, "a block is half a word of the bitset");
    const uint64_t tid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, nthr = (uint64_t)gridDim.x * blockDim.x;
    auto plus = [](uint32_t x, uint32_t y) { return x + y; };
    auto orbit = [](uint64_t* words, uint64_t i) {
        return (uint64_t)atomicOr(reinterpret_cast<unsigned long long*>(words + (i >> 6)), 1ull << (i & 63));
    };
    uint32_t bad = 0, dup = 0, smp = 0, nonf = 0;
    for (uint64_t i = tid; i < n_ids; i += nthr) {
        const uint64_t id = ids[i];
        if (id < lo || id - lo >= n) { ++bad; continue; }
        const uint64_t r = id - lo;
        const uint64_t old = orbit(touched, r);
        if ((old >> (r & 63)) & 1ull) { ++dup; continue; }
        if (!(uint32_t)(old >> (r & 32))) (void)orbit(blocks, r / kQuantBlock);
        if (r % kSampleStride == 0) {
            ++smp;
            (void)orbit(groups, r / (kSampleStride * (uint64_t)kSampleScaleRows));
        }
    }
    constexpr uint32_t kPer16 = BF16 ? 8 : 4;
    auto word_bad = [](uint32_t w) -> uint32_t {
        if (BF16) return ((w & 0x7f80u) == 0x7f80u ? 1u : 0u) + ((w & 0x7f800000u) == 0x7f800000u ? 1u : 0u);
        return (w & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    };
    const uint64_t n16 = vec ? n_vals / kPer16 : 0;
    const uint4* s16 = static_cast<const uint4*>(src);
    for (uint64_t u = tid; u < n16; u += nthr) {
        const uint4 v = s16[u];
        nonf += word_bad(v.x) + word_bad(v.y) + word_bad(v.z) + word_bad(v.w);
    }
    for (uint64_t e = n16 * kPer16 + tid; e < n_vals; e += nthr) {
        if (BF16) nonf += (static_cast<const uint16_t*>(src)[e] & 0x7f80u) == 0x7f80u ? 1u : 0u;
        else nonf += (static_cast<const uint32_t*>(src)[e] & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    }
    bad = wave_reduce_u32(bad, plus);
    dup = wave_reduce_u32(dup, plus);
    smp = wave_reduce_u32(smp, plus);
    nonf = wave_reduce_u32(nonf, plus);
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(cnt + kUpdBadId, (unsigned long long)bad);
        if (dup) atomicAdd(cnt + kUpdDupId, (unsigned long long)dup);
        if (nonf) atomicAdd(cnt + kUpdNonFinite, (unsigned long long)nonf);
        if (smp) atomicAdd(cnt + kUpdSampleRows, (unsigned long long)smp);
    }
}

// The scatter: one wave per incoming row j -> slab row ids[j] - lo, 16-byte stores along the whole
// padded row (zeros past dim).  f32: 4 columns per lane and step; bf16: 8, widened exactly
// (bits << 16, as k_widen_bf16_rows).  vec: the incoming rows are 16-byte aligned (the base is,
// and dim is a multiple of the columns of one 16-byte load) and are read 16 bytes at a time.
// The check found every id in range and none twice: no two waves write one row.
template <bool BF16>
__global__ __launch_bounds__(256) void k_upd_scatter(const uint64_t* __restrict__ ids, uint64_t n_ids, uint64_t lo,
                                                     const void* __restrict__ src, uint32_t dim, uint32_t ld, bool vec,
                                                     float* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < n_ids; j += (uint64_t)gridDim.x * 4) {
        float* dst = rows + (ids[j] - lo) * ld;
        if (BF16) {
            const uint16_t* a = static_cast<const uint16_t*>(src) + j * dim;
            for (uint32_t c0 = lane * 8; c0 < ld; c0 += 8 * kWave) {
                uint16_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (vec && c0 < dim) {
                    const uint4 v = *reinterpret_cast<const uint4*>(a + c0);
                    h[0] = (uint16_t)v.x; h[1] = (uint16_t)(v.x >> 16); h[2] = (uint16_t)v.y; h[3] = (uint16_t)(v.y >> 16);
                    h[4] = (uint16_t)v.z; h[5] = (uint16_t)(v.z >> 16); h[6] = (uint16_t)v.w; h[7] = (uint16_t)(v.w >> 16);
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (c0 + i < dim) h[i] = a[c0 + i];
                }
                *reinterpret_cast<float4*>(dst + c0) =
                    make_float4(bf16_to_f32(h[0]), bf16_to_f32(h[1]), bf16_to_f32(h[2]), bf16_to_f32(h[3]));
                *reinterpret_cast<float4*>(dst + c0 + 4) =
                    make_float4(bf16_to_f32(h[4]), bf16_to_f32(h[5]), bf16_to_f32(h[6]), bf16_to_f32(h[7]));
            }
        } else {
            const float* a = static_cast<const float*>(src) + j * dim;
            for (uint32_t c0 = lane * 4; c0 < ld; c0 += 4 * kWave) {
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (vec && c0 < dim) {
                    v = *reinterpret_cast<const float4*>(a + c0);
                } else {
                    if (c0 < dim) v.x = a[c0];
                    if (c0 + 1 < dim) v.y = a[c0 + 1];
                    if (c0 + 2 < dim) v.z = a[c0 + 2];
                    if (c0 + 3 < dim) v.w = a[c0 + 3];
                }
                *reinterpret_cast<float4*>(dst + c0) = v;
            }
        }
    }
}

// k_row_norms over the listed rows: a wave owns 64 consecutive entries of ids and gathers their
// slab rows through LDS, 16 lanes per 256-byte row segment, as k_row_norms stages its own; the
// arithmetic and the flag rules are row_norms_wave's, the flags OR-ed into flags[0].
__global__ __launch_bounds__(256) void k_upd_row_norms(const float* __restrict__ rows, const uint64_t* __restrict__ ids,
                                                       uint64_t n_ids, uint64_t lo, uint32_t dim, uint32_t ld,
                                                       float* __restrict__ na, uint32_t* flags) {
    __shared__ float tile[4][64 * 65];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t j = ((uint64_t)blockIdx.x * 4 + w) * 64 + lane;
    const uint64_t mine = j < n_ids ? ids[j] - lo : ~0ull;  // (the lane's slab row; ~0: none)
    row_norms_wave(rows, dim, ld, na, flags, tile[w], [&](uint32_t i) -> int64_t { return (int64_t)shfl64(mine, (int)i); });
}

// k_rows_to_i8 / k_rows_to_i8_sample from a list: workgroup b < *count takes block / group list[b]
// (ascending: launch_mask_list_scatter over the check's bitsets); the grid covers the list's
// capacity and the workgroups past the device-side count leave at once.
__global__ __launch_bounds__(256) void k_upd_rows_to_i8(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                        uint32_t ld, int8_t* __restrict__ out,
                                                        float* __restrict__ scales, uint32_t* __restrict__ ea_max,
                                                        const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ count) {
    if (blockIdx.x >= *count) return;
    rows_to_i8_block(rows, n, dim, ld, out, scales, ea_max, list[blockIdx.x]);
}
__global__ __launch_bounds__(256) void k_upd_rows_to_i8_sample(const float* __restrict__ rows, uint64_t n,
                                                               uint32_t dim, uint32_t ld, int8_t* __restrict__ out,
                                                               float* __restrict__ scales,
                                                               const uint32_t* __restrict__ list,
                                                               const uint32_t* __restrict__ count) {
    if (blockIdx.x >= *count) return;
    rows_to_i8_sample_group(rows, n, dim, ld, out, scales, list[blockIdx.x]);
}

// ------------------------------------------------------------------------------------
// Compaction (bsr_index_compact): the live rows list[0 .. cnt) of the slab, ascending,
// packed.  k_compact_gather copies slab row list[j] to row j of ANOTHER buffer (the staging buffer
// of a chunk, or the smaller slab of a shrink): list[j] >= j, so a gather within the slab would
// overwrite rows other lanes have not read yet -- the host moves chunk by chunk through the
// staging buffer, in stream order.  LPR lanes per row (16 for rows of fewer than 64 16-byte units),
// the row index read once per row, 16-byte loads and stores, four in flight per lane; every offset
// is a 64-bit count of 16-byte units.  No LDS.
// ------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(256) void k_compact_gather(const uint4* __restrict__ rows,
                                                        const uint32_t* __restrict__ list, uint64_t cnt,
                                                        uint32_t units, uint4* __restrict__ out) {
    const uint32_t sub = threadIdx.x % LPR;
    const uint64_t step = (uint64_t)gridDim.x * (256 / LPR);
    for (uint64_t j = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / LPR; j < cnt; j += step) {
        const uint4* __restrict__ src = rows + (uint64_t)list[j] * units;
        uint4* __restrict__ dst = out + j * units;
        uint32_t u = sub;
        for (; u + 3 * LPR < units; u += 4 * LPR) {
            const uint4 v0 = src[u], v1 = src[u + LPR], v2 = src[u + 2 * LPR], v3 = src[u + 3 * LPR];
            dst[u] = v0;
            dst[u + LPR] = v1;
            dst[u + 2 * LPR] = v2;
            dst[u + 3 * LPR] = v3;
        }
        for (; u < units; u += LPR) dst[u] = src[u];
    }
}

// The id map: out[j] = lo + list[j], the global index before the compaction of the row that becomes
// local row j (out may be null; list = nullptr: the identity, no row moves), and *first = the
// lowest j with list[j] != j (atomicMin; preset to ~0 by the caller): the rows before it stay put.
__global__ __launch_bounds__(256) void k_compact_ids(const uint32_t* __restrict__ list, uint64_t cnt, uint64_t lo,
                                                     uint64_t* __restrict__ out, uint32_t* __restrict__ first) {
    uint32_t mine = ~0u;
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < cnt; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = list ? list[j] : j;
        if (out) out[j] = lo + r;
        if (r != j && mine == ~0u) mine = (uint32_t)j;
    }
    mine = wave_reduce_u32(mine, [](uint32_t x, uint32_t y) { return x < y ? x : y; });
    if ((threadIdx.x & 63) == 0 && mine != ~0u) atomicMin(first, mine);
}

// The gather's grid follows the device (workgroups per compute unit), not the row count.
static uint32_t compact_grid(uint64_t groups_needed) {
    static const uint32_t cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
            n = 256;
        (void)hipGetLastError();
        return (uint32_t)n;
    }();
    const uint64_t cap = (uint64_t)cus * 8;
    return (uint32_t)(groups_needed < 1 ? 1 : groups_needed > cap ? cap : groups_needed);
}
hipError_t launch_compact_gather(const float* rows, const uint32_t* list, uint64_t cnt, uint32_t ld, float* out,
                                 hipStream_t s) {
    if (ld % kLdAlign != 0 || !ld) return hipErrorInvalidValue;
    if (!cnt) return hipSuccess;
    const uint32_t units = ld / 4;  // 16-byte units per row (a multiple of 16)
    const uint4* src = reinterpret_cast<const uint4*>(rows);
    uint4* dst = reinterpret_cast<uint4*>(out);
    if (units < 64)
        hipLaunchKernelGGL(k_compact_gather<16>, dim3(compact_grid((cnt + 15) / 16)), dim3(256), 0, s, src, list, cnt,
                           units, dst);
    else
        hipLaunchKernelGGL(k_compact_gather<64>, dim3(compact_grid((cnt + 3) / 4)), dim3(256), 0, s, src, list, cnt,
                           units, dst);
    return hipGetLastError();
}
hipError_t launch_compact_ids(const uint32_t* list, uint64_t cnt, uint64_t lo, uint64_t* out, uint32_t* first,
                              hipStream_t s) {
    if (!cnt) return hipSuccess;
    hipLaunchKernelGGL(k_compact_ids, dim3(grid_for(cnt, 256, 2048)), dim3(256), 0, s, list, cnt, lo, out, first);
    return hipGetLastError();
}

hipError_t launch_upd_check(const uint64_t* ids, uint64_t n_ids, uint64_t lo, uint64_t n, const void* src,
                            uint32_t dim, bool bf16, uint64_t* touched, uint64_t* blocks, uint64_t* groups,
                            uint64_t* cnt, hipStream_t s) {
    const uint64_t n_vals = n_ids * dim;
    const bool vec = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
    const uint32_t grid = grid_for(std::max<uint64_t>(n_ids, n_vals / (bf16 ? 8 : 4)), 256, 2048);
    unsigned long long* c = reinterpret_cast<unsigned long long*>(cnt);
    if (bf16)
        hipLaunchKernelGGL(k_upd_check<true>, dim3(grid), dim3(256), 0, s, ids, n_ids, lo, n, src, n_vals, vec, touched,
                           blocks, groups, c);
    else
        hipLaunchKernelGGL(k_upd_check<false>, dim3(grid), dim3(256), 0, s, ids, n_ids, lo, n, src, n_vals, vec, touched,
                           blocks, groups, c);
    return hipGetLastError();
}
hipError_t launch_upd_scatter(const uint64_t* ids, uint64_t n_ids, uint64_t lo, const void* src, uint32_t dim,
                              uint32_t ld, bool bf16, float* rows, hipStream_t s) {
    if (ld % kLdAlign != 0 || dim > ld) return hipErrorInvalidValue;
    const bool vec = (reinterpret_cast<uintptr_t>(src) & 15u) == 0 && dim % (bf16 ? 8 : 4) == 0;
    const uint32_t grid = grid_for(n_ids, 4, 8192);
    if (bf16)
        hipLaunchKernelGGL(k_upd_scatter<true>, dim3(grid), dim3(256), 0, s, ids, n_ids, lo, src, dim, ld, vec, rows);
    else
        hipLaunchKernelGGL(k_upd_scatter<false>, dim3(grid), dim3(256), 0, s, ids, n_ids, lo, src, dim, ld, vec, rows);
    return hipGetLastError();
}
hipError_t launch_upd_row_norms(const float* rows, const uint64_t* ids, uint64_t n_ids, uint64_t lo, uint32_t dim,
                                uint32_t ld, float* na, uint32_t* flags, hipStream_t s) {
    hipLaunchKernelGGL(k_upd_row_norms, dim3((uint32_t)((n_ids + 255) / 256)), dim3(256), 0, s, rows, ids, n_ids, lo,
                       dim, ld, na, flags);
    return hipGetLastError();
}
hipError_t launch_upd_rows_to_i8(const float* rows, uint64_t n, uint32_t dim, uint32_t ld, int8_t* out, float* scales,
                                 uint32_t* ea_max, const uint32_t* list, const uint32_t* count, uint32_t cap,
                                 hipStream_t s) {
    if (cap)
        hipLaunchKernelGGL(k_upd_rows_to_i8, dim3(cap), dim3(256), 0, s, rows, n, dim, ld, out, scales, ea_max, list,
                           count);
    return hipGetLastError();
}
hipError_t launch_upd_rows_to_i8_sample(const float* rows, uint64_t n, uint32_t dim, uint32_t ld, int8_t* out,
                                        float* scales, const uint32_t* list, const uint32_t* count, uint32_t cap,
                                        hipStream_t s) {
    if (cap)
        hipLaunchKernelGGL(k_upd_rows_to_i8_sample, dim3(cap), dim3(256), 0, s, rows, n, dim, ld, out, scales, list,
                           count);
    return hipGetLastError();
}

hipError_t launch_dead_check(const uint64_t* ids, uint64_t n_ids, uint64_t lo, uint64_t n, uint32_t* bad,
                             hipStream_t s) {
    hipLaunchKernelGGL(k_dead_check, dim3(grid_for(n_ids, 256, 2048)), dim3(256), 0, s, ids, n_ids, lo, n, bad);
    return hipGetLastError();
}
hipError_t launch_dead_apply(const uint64_t* ids, uint64_t n_ids, uint64_t lo, uint64_t n, uint64_t* dead,
                             uint32_t* newly, hipStream_t s) {
    hipLaunchKernelGGL(k_dead_apply, dim3(grid_for(n_ids, 256, 2048)), dim3(256), 0, s, ids, n_ids, lo, n, dead, newly);
    return hipGetLastError();
}
hipError_t launch_dead_zero_fop(const uint64_t* dead, uint64_t n, const uint32_t* dead_blk, uint32_t row_bytes,
                                uint8_t* fop, uint8_t* fop_s, const float* rows, uint32_t dim, const float* scales_s,
                                hipStream_t s) {
    if (row_bytes % 64 != 0 || dim > row_bytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dead_zero_fop, dim3(grid_for((n + 63) / 64, 4, 4096)), dim3(256), 0, s, dead, n, dead_blk,
                       row_bytes, fop, fop_s, rows, dim, scales_s);
    return hipGetLastError();
}
// (a grid's y extent is at most 65535: more masks or lists than that take a launch per 65535)
constexpr uint32_t kGridYMax = 65535;
static hipError_t mask_count(const uint64_t* allow, uint64_t words, uint32_t n_masks, uint64_t n, const uint64_t* dead,
                             const uint32_t* query_mask, uint32_t nq, uint32_t* blk, uint32_t* out, hipStream_t s) {
    const uint32_t n_blk = mask_blocks(n), stride = n_blk + 1;
    for (uint32_t g0 = 0; g0 < n_masks; g0 += kGridYMax) {
        const uint32_t g = n_masks - g0 < kGridYMax ? n_masks - g0 : kGridYMax;
        hipLaunchKernelGGL(k_mask_count, dim3(n_blk, g), dim3(256), 0, s, allow ? allow + (uint64_t)g0 * words : nullptr,
                           words, n, dead, blk + (uint64_t)g0 * stride, stride);
    }
    hipLaunchKernelGGL(k_mask_scan, dim3(n_masks + (query_mask ? 1u : 0u)), dim3(256), 0, s, blk, n_blk, n_masks,
                       query_mask, nq, out);
    return hipGetLastError();
}
hipError_t launch_mask_groups_count(const uint64_t* allow, uint64_t words, uint32_t n_masks, uint64_t n,
                                    const uint64_t* dead, const uint32_t* query_mask, uint32_t nq, uint32_t* blk,
                                    uint32_t* out, hipStream_t s) {
    if (!n_masks || words != (n + 63) / 64) return hipErrorInvalidValue;
    return mask_count(allow, words, n_masks, n, dead, query_mask, nq, blk, out, s);
}
hipError_t launch_mask_groups_scatter(const uint64_t* allow, uint64_t words, uint64_t n, const uint64_t* dead,
                                      const uint32_t* blk, const MaskListDesc* d, uint32_t n_lists, uint32_t* list,
                                      hipStream_t s) {
    const uint32_t n_blk = mask_blocks(n);
    for (uint32_t l0 = 0; l0 < n_lists; l0 += kGridYMax) {
        const uint32_t l = n_lists - l0 < kGridYMax ? n_lists - l0 : kGridYMax;
        hipLaunchKernelGGL(k_mask_scatter, dim3(n_blk, l), dim3(256), 0, s, allow, words, n, dead, blk, n_blk + 1, d + l0,
                           MaskListDesc{}, list);
    }
    return hipGetLastError();
}
hipError_t launch_mask_groups_scatter_seg(const uint64_t* allow, uint64_t words, uint64_t n, const uint64_t* dead,
                                          const uint32_t* blk, const MaskSegDesc* d, uint32_t n_segs, uint32_t* list,
                                          hipStream_t s) {
    const uint32_t n_blk = mask_blocks(n);
    for (uint32_t l0 = 0; l0 < n_segs; l0 += kGridYMax) {
        const uint32_t l = n_segs - l0 < kGridYMax ? n_segs - l0 : kGridYMax;
        hipLaunchKernelGGL(k_mask_scatter_seg, dim3(n_blk, l), dim3(256), 0, s, allow, words, n, dead, blk, n_blk + 1,
                           d + l0, list);
    }
    return hipGetLastError();
}
// One mask, one list: the same kernels, the list's descriptor a launch argument (no upload).
hipError_t launch_mask_list_count(const uint64_t* allow, const uint64_t* dead, uint64_t n, uint32_t* blk,
                                  hipStream_t s) {
    return mask_count(allow, 0, 1, n, dead, nullptr, 0, blk, nullptr, s);
}
hipError_t launch_mask_list_scatter(const uint64_t* allow, const uint64_t* dead, uint64_t n, const uint32_t* blk,
                                    uint32_t n_list, uint32_t* list, hipStream_t s) {
    const uint32_t n_blk = mask_blocks(n);
    hipLaunchKernelGGL(k_mask_scatter, dim3(n_blk), dim3(256), 0, s, allow, (uint64_t)0, n, dead, blk, n_blk + 1,
                       static_cast<const MaskListDesc*>(nullptr), MaskListDesc{0, 0, n_list}, list);
    return hipGetLastError();
}
hipError_t launch_mask_cut(uint64_t* cand, uint32_t* cnt, uint32_t cap, uint32_t nq, const uint64_t* allow,
                           uint64_t words, const uint32_t* query_mask, const uint64_t* dead, uint64_t n, uint32_t* raw,
                           uint32_t* items, hipStream_t s) {
    hipLaunchKernelGGL(k_mask_cut, dim3((nq + 3) / 4), dim3(256), 0, s, cand, cnt, cap, nq, allow, words, query_mask,
                       dead, n, raw, items);
    return hipGetLastError();
}

hipError_t launch_synth_uniform(float* out, uint64_t row0, uint64_t n_rows, uint32_t dim,
                                uint32_t ld, uint64_t seed, hipStream_t s) {
    hipLaunchKernelGGL(k_synth_uniform, dim3(grid_for(n_rows * ld, 256)), dim3(256), 0, s, out, row0,
                       n_rows, dim, ld, seed);
    return hipGetLastError();
}
hipError_t launch_copy_rows_f32(const float* src, uint64_t n, uint32_t dim, uint32_t ld, float* dst,
                                hipStream_t s) {
    hipLaunchKernelGGL(k_copy_rows_f32, dim3(grid_for(n * ld, 256)), dim3(256), 0, s, src, n, dim, ld, dst);
    return hipGetLastError();
}
hipError_t launch_widen_bf16_rows(const uint16_t* src, uint64_t n, uint32_t dim, uint32_t ld,
                                  float* dst, hipStream_t s) {
    hipLaunchKernelGGL(k_widen_bf16_rows, dim3(grid_for(n * ld, 256)), dim3(256), 0, s, src, n, dim, ld, dst);
    return hipGetLastError();
}
hipError_t launch_row_norms(const float* rows, uint64_t n, uint32_t dim, uint32_t ld, float* na,
                            uint32_t* flags, hipStream_t s) {
    hipLaunchKernelGGL(k_row_norms, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, rows, n, dim, ld,
                       na, flags);
    return hipGetLastError();
}
hipError_t launch_rows_to_i8(const float* rows, uint64_t n, uint64_t n_pad, uint32_t dim, uint32_t ld,
                             int8_t* out, float* scales, uint32_t* ea_max, hipStream_t s) {
    const uint64_t blocks = n_pad / kQuantBlock;
    hipLaunchKernelGGL(k_rows_to_i8, dim3((uint32_t)blocks), dim3(256), 0, s, rows, n, dim, ld, out, scales,
                       ea_max);
    return hipGetLastError();
}
hipError_t launch_rows_to_i8_sample(const float* rows, uint64_t n, uint32_t dim, uint32_t ld, int8_t* out,
                                    float* scales, hipStream_t s) {
    const uint64_t n_s = (n + kSampleStride - 1) / kSampleStride;
    const uint64_t blocks = (n_s + kSampleScaleRows - 1) / kSampleScaleRows;
    if (blocks)
        hipLaunchKernelGGL(k_rows_to_i8_sample, dim3((uint32_t)blocks), dim3(256), 0, s, rows, n, dim, ld, out,
                           scales);
    return hipGetLastError();
}
hipError_t launch_query_prep(const QueryPrepArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_query_prep, dim3(a.qpad), dim3(128), 0, s, a.q, a.nq, a.dim, a.ld, a.with_op,
                       a.ea_max, a.qf32, a.nb, a.qop, a.qscale, a.ebound, a.qflags, a.qids, a.status);
    return hipGetLastError();
}

hipError_t launch_gather_emulate(const void* send, const void* script, void* recv, uint64_t bytes, uint32_t P,
                                 uint32_t rank, hipStream_t s) {
    if (bytes % 4) return hipErrorInvalidValue;
    const uint64_t words = bytes / 4, total = words * P;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(2048, std::max<uint64_t>(1, (total + 255) / 256));
    hipLaunchKernelGGL(k_gather_emulate, dim3(grid), dim3(256), 0, s, static_cast<const uint32_t*>(send),
                       static_cast<const uint32_t*>(script), static_cast<uint32_t*>(recv), words, P, rank);
    return hipGetLastError();
}

hipError_t launch_header_put(const int32_t w[8], int32_t* dst, hipStream_t s) {
    HeaderWords h;
    for (int i = 0; i < 8; ++i) h.w[i] = w[i];
    hipLaunchKernelGGL(k_header_put, dim3(1), dim3(64), 0, s, h, dst);
    return hipGetLastError();
}
hipError_t launch_header_publish(const int32_t* src, uint32_t words, int32_t* host, uint32_t* host_flag, uint32_t seq,
                                 hipStream_t s) {
    hipLaunchKernelGGL(k_header_publish, dim3(1), dim3(256), 0, s, src, words, host, host_flag, seq);
    return hipGetLastError();
}

}  // namespace bsr
