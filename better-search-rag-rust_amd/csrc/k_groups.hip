// k_groups.hip -- group search (bsr_local_top_groups) on gfx950: the inverted list
// of row_group, the fill that scores the rows of a query's result groups and keeps the m best of
// each, and the finish of the queries split over several workgroups; and the deep group search's
// plan, fill and finish (bsr_local_top_groups_deep) for up to 1024 groups a query.
//
// Compiled like k_exact.hip (-ffp-contract=off, correctly rounded divide and sqrt: the walk is the
// reference's arithmetic), and with the device feature packed-fp32-ops off (Makefile).
#include <cstdlib>
#include "bsr_device.hpp"
#include "exact_walk.hpp"
#include "kernels.hpp"

#include <math.h>

namespace bsr {

// ------------------------------------------------------------------------------------
// Group search (bsr_local_top_groups): the k best groups with up to m rows of each.
// The collapsed search names the groups; the inverted list of row_group gives their rows; the fill
// scores exactly those rows and keeps the m best of every group.
// ------------------------------------------------------------------------------------
// The histogram of row_group (every entry < n_groups: k_group_check ran).
__global__ __launch_bounds__(256) void k_groups_count(const uint32_t* __restrict__ row_group, uint64_t n,
                                                      uint32_t* __restrict__ gcnt) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        atomicAdd(gcnt + row_group[i], 1u);
}

// A wave takes 64 consecutive groups at a time: the prefix sum of their counts inside the wave, one
// atomic add of the wave's total on the cursor, gpos[g] = the group's first slot.  The ranges are
// disjoint and cover [0, n) whatever the order the waves arrive in.
__global__ __launch_bounds__(256) void k_groups_offsets(const uint32_t* __restrict__ gcnt, uint32_t n_groups,
                                                        uint32_t* __restrict__ cursor, uint32_t* __restrict__ gpos) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6, waves = (uint64_t)gridDim.x * 4;
    for (uint64_t base = wave * 64; base < n_groups; base += waves * 64) {  // (uniform over the wave)
        const uint64_t g = base + lane;
        const uint32_t c = g < n_groups ? gcnt[g] : 0u;
        uint32_t inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)inc, d, kWave);
            inc += lane >= d ? v : 0u;
        }
        const uint32_t total = (uint32_t)__shfl((int)inc, 63, kWave);
        uint32_t b0 = 0;
        if (lane == 0 && total) b0 = atomicAdd(cursor, total);
        b0 = (uint32_t)__shfl((int)b0, 0, kWave);
        if (g < n_groups) gpos[g] = b0 + inc - c;
    }
}

// Row i takes the next slot of its group: gpos[g] ends at the end of the group's range (a slot is
// below n: the ranges cover [0, n)).
__global__ __launch_bounds__(256) void k_groups_scatter(const uint32_t* __restrict__ row_group, uint64_t n,
                                                        uint32_t* __restrict__ gpos, uint32_t* __restrict__ glist) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        glist[atomicAdd(gpos + row_group[i], 1u)] = (uint32_t)i;
}

// The table rows [k][m] of one query (any order inside a group, kKeyNone where a group has fewer
// rows) -> its outputs: a wave per group, one entry per lane through wave_sort64.
template <class Args>
__device__ __forceinline__ void groups_emit(const Args& a, uint32_t q, const unsigned long long* tab, uint32_t cnt) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t k = a.k, m = a.m;
    for (uint32_t g = w; g < k; g += 4) {
        const uint64_t x = wave_sort64((uint32_t)lane < m ? (uint64_t)tab[g * m + lane] : kKeyNone);
        const bool has = x != kKeyNone;
        const uint32_t nrows = (uint32_t)__popcll(__ballot(has));
        const uint64_t slot = (uint64_t)q * k + g;
        if ((uint32_t)lane < m) {
            a.out_idx[slot * m + lane] = has ? a.offset + key_row(x) : ~0ull;
            a.out_dist[slot * m + lane] = has ? key_dist(x) : INFINITY;
        }
        if (lane == 0) {
            if (a.out_rows) a.out_rows[slot] = nrows;
            if (a.out_group) a.out_group[slot] = g < cnt ? a.head_group[slot] : ~0u;
        }
    }
    if (threadIdx.x == 0) a.out_count[q] = cnt;
}

// One workgroup of four waves per query (SPLIT: blockIdx.y's share of the items of a long query).
// LDS: the waves' row stages and the query (k_score_ids), the prefix sums of the result groups'
// rows, and -- not SPLIT -- the table [k][m] of TAB entries; SPLIT offers into the global table.
// Position p of the concatenated row lists belongs to the result group g with pre[g] <= p < pre[g+1]
// (a binary search per lane); an item is 64 consecutive positions, taken from the LDS counter, so
// ten groups of six rows are one item and a group of 100k rows is dealt over every wave.  A lane
// past the end, a deleted or a disallowed row walks row 0 and drops its result; every address is
// formed from a glist entry, below n by construction.
template <int TAB, bool SPLIT>
__global__ __launch_bounds__(256) void k_groups_fill(GroupsFillArgs a) {
    constexpr int W = 4, STAGE = 64 * 68, QMAX = 1024, KMAX = (int)kCollapseMaxFetch;
    __shared__ __attribute__((aligned(16))) float lds_all[W * STAGE + QMAX];
    __shared__ unsigned long long s_tab[TAB];
    __shared__ uint32_t s_first[KMAX], s_pre[KMAX + 1], s_next;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t t = threadIdx.x;
    float* const lds = lds_all + w * STAGE;
    float* const ldq = lds_all + W * STAGE;
    const uint32_t q = SPLIT ? a.split[blockIdx.x] : blockIdx.x;
    const uint32_t k = a.k, m = a.m;
    const uint32_t cnt = a.head_cnt[q] < k ? a.head_cnt[q] : k;
    uint32_t len = 0;
    if (t < cnt) {
        const uint32_t g = a.head_group[(uint64_t)q * k + t];
        len = a.gcnt[g];
        s_first[t] = a.gpos[g] - len;
    }
    if (t == 0) s_pre[0] = 0;
    s_pre[t + 1] = len;
    __syncthreads();
    for (uint32_t s = 1; s < 256; s <<= 1) {  // (inclusive scan of the lengths in s_pre[1 .. 256])
        const uint32_t v = t >= s ? s_pre[t + 1 - s] : 0u;
        __syncthreads();
        s_pre[t + 1] += v;
        __syncthreads();
    }
    const uint32_t total = s_pre[KMAX];  // (at most n < 2^32 rows: the groups are distinct)
    const uint32_t items = total / 64 + (total % 64 ? 1u : 0u);
    uint32_t lo = 0, hi = items;
    if (SPLIT) {
        const uint32_t per = (items + gridDim.y - 1) / gridDim.y;
        lo = blockIdx.y * per < items ? blockIdx.y * per : items;
        hi = items - lo < per ? items : lo + per;
    } else if (items > a.split_items) {  // (uniform over the workgroup) the split launches answer it
        if (t == 0) {
            a.split[atomicAdd(a.split_info, 1u)] = q;
            atomicMax(a.split_info + 1, items);
        }
        return;
    }
    if (t == 0) s_next = lo;
    if (!SPLIT)
        for (uint32_t i = t; i < k * m; i += 64 * W) s_tab[i] = kKeyNone;
    const uint32_t ld = a.ld;
    const float* const qrow = a.qf32 + (uint64_t)q * ld;
    const bool qlds = ld <= (uint32_t)QMAX;  // (longer rows read the query from global memory)
    if (qlds)
        for (uint32_t cc = t; cc < ld; cc += 64 * W) ldq[cc] = qrow[cc];
    __syncthreads();
    unsigned long long* const tab =
        SPLIT ? reinterpret_cast<unsigned long long*>(a.table) + (uint64_t)blockIdx.x * k * m : s_tab;
    const uint64_t mask = a.allow && a.query_mask ? a.query_mask[q] : 0u;
    const uint32_t* const aw =
        a.allow ? reinterpret_cast<const uint32_t*>(a.allow + mask * a.allow_words) : nullptr;
    const float mag_b = a.nb[q];
    for (;;) {
        uint32_t it = 0;
        if (lane == 0) it = atomicAdd(&s_next, 1u);
        it = (uint32_t)__builtin_amdgcn_readfirstlane((int)it);
        if (it >= hi) break;
        const uint64_t p = (uint64_t)it * 64 + lane;
        const bool inlist = p < total;
        uint32_t g0 = 0, g1 = cnt;  // (the slot lies in [g0, g1); cnt >= 1 wherever an item exists)
        while (g1 - g0 > 1) {
            const uint32_t mid = (g0 + g1) >> 1;
            if (s_pre[mid] <= p) g0 = mid;
            else g1 = mid;
        }
        const uint32_t r = inlist ? a.glist[s_first[g0] + (uint32_t)(p - s_pre[g0])] : 0u;
        bool live = row_live(a.dead, r, inlist);
        if (live && aw) live = (aw[r >> 5] >> (r & 31)) & 1u;
        if (!__ballot(live)) continue;  // (uniform over the wave)
        const uint32_t myrow = live ? r : 0u;
        float acc[1] = {-0.0f}, mx[1] = {0.0f};
        wave_walk_rows(lds, a.rows, ld, a.dim, myrow, qlds ? ldq : qrow, lane, acc, mx);
        const float d = finish_distance(acc[0], mx[0], a.na[myrow], mag_b);
        // (cap_insert's reads ahead are the cut: a key below no entry of its group costs no atomic)
        if (live) cap_insert(tab + (uint64_t)g0 * m, m, dist_key(d, myrow));
    }
    if (SPLIT) return;
    __syncthreads();
    groups_emit(a, q, s_tab, cnt);
}

// One workgroup per split query: its row of the global table through groups_emit.
__global__ __launch_bounds__(256) void k_groups_finish(GroupsFillArgs a) {
    const uint32_t q = a.split[blockIdx.x];
    const uint32_t cnt = a.head_cnt[q] < a.k ? a.head_cnt[q] : a.k;
    groups_emit(a, q, reinterpret_cast<const unsigned long long*>(a.table) + (uint64_t)blockIdx.x * a.k * a.m, cnt);
}

// ------------------------------------------------------------------------------------
// Deep group search (bsr_local_top_groups_deep): up to 1024 result groups a query.
// The plan scans every query's group lengths once and leaves the prefix sums in global memory; the
// host reads three words and sets the budget; the fill copies its query's plan and deals the items.
// ------------------------------------------------------------------------------------
// One workgroup per query, four result groups a thread: the lengths of the head groups, their sum
// scanned over the wave by shuffles, one pass over the four wave totals.  pre[q][i] is the first
// position of result group i in the concatenated row lists (pre[q][i] = the total for i >= cnt),
// first[q][i] its first slot in glist.  A head group has a live row, so no length is zero; the
// groups are distinct, so a total is at most n < 2^32.
__global__ __launch_bounds__(256) void k_groups_deep_plan(GroupsDeepArgs a) {
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6, q = blockIdx.x, k = a.k;
    const uint32_t cnt = a.head_cnt[q] < k ? a.head_cnt[q] : k;
    uint32_t len[4], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t i = 4 * t + j;
        len[j] = 0;
        if (i < cnt) {
            const uint32_t g = a.head_group[(uint64_t)q * k + i];
            len[j] = a.gcnt[g];
            a.first[(uint64_t)q * k + i] = a.gpos[g] - len[j];
        }
        sum += len[j];
    }
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, d, kWave);
        inc += lane >= (uint32_t)d ? v : 0u;
    }
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    uint32_t base = inc - sum, total = 0;
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) {
        base += v < w ? s_wave[v] : 0u;
        total += s_wave[v];
    }
    uint32_t* const pre = a.pre + (uint64_t)q * (k + 1);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t i = 4 * t + j;
        if (i < k) pre[i] = base;
        base += len[j];
    }
    if (t == 0) {
        const uint32_t items = total / 64 + (total % 64 ? 1u : 0u);
        pre[k] = total;
        a.items[q] = items;
        if (items) {
            atomicAdd(reinterpret_cast<unsigned long long*>(a.info), (unsigned long long)items);
            atomicMax(a.info + 2, items);
        }
    }
}

// One workgroup of four waves per query (SPLIT: blockIdx.y's share of the items of a long query).
// LDS: the waves' row stages and the query as k_groups_fill has them, the query's plan (pre, first)
// copied from global memory, and -- not SPLIT -- the table [k][m] of TAB entries; SPLIT offers into
// row q of the global table.  A query is short when it has at most `budget` items: the plain launch
// answers the short queries and leaves the long ones (its workgroup exits), the SPLIT launch the
// reverse; nothing is listed and nothing is read back between them.  The item loop is
// k_groups_fill's: 64 consecutive positions an item from the LDS counter, the group by a binary
// search over pre (at most 10 steps), the row from glist -- the only source of an address -- the
// walk, and cap_insert into the group's m entries.
template <int TAB, bool SPLIT>
__global__ __launch_bounds__(256) void k_groups_fill_deep(GroupsDeepArgs a) {
    constexpr int W = 4, STAGE = 64 * 68, QMAX = 1024, KMAX = (int)kDeepMaxK;
    __shared__ __attribute__((aligned(16))) float lds_all[W * STAGE + QMAX];
    __shared__ unsigned long long s_tab[TAB];
    __shared__ uint32_t s_first[KMAX], s_pre[KMAX + 1], s_next;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t t = threadIdx.x;
    float* const lds = lds_all + w * STAGE;
    float* const ldq = lds_all + W * STAGE;
    const uint32_t q = blockIdx.x;
    const uint32_t k = a.k, m = a.m;
    const uint32_t items = a.items[q];
    if (SPLIT ? items <= a.budget : items > a.budget) return;  // (uniform over the workgroup)
    uint32_t lo = 0, hi = items;
    if (SPLIT) {
        const uint32_t per = (items + gridDim.y - 1) / gridDim.y;
        lo = blockIdx.y * per < items ? blockIdx.y * per : items;
        hi = items - lo < per ? items : lo + per;
        if (lo >= hi) return;  // (an empty share)
    }
    const uint32_t cnt = a.head_cnt[q] < k ? a.head_cnt[q] : k;
    for (uint32_t i = t; i < cnt; i += 64 * W) s_first[i] = a.first[(uint64_t)q * k + i];
    for (uint32_t i = t; i <= cnt; i += 64 * W) s_pre[i] = a.pre[(uint64_t)q * (k + 1) + i];
    if (t == 0) s_next = lo;
    if (!SPLIT)
        for (uint32_t i = t; i < k * m; i += 64 * W) s_tab[i] = kKeyNone;
    const uint32_t ld = a.ld;
    const float* const qrow = a.qf32 + (uint64_t)q * ld;
    const bool qlds = ld <= (uint32_t)QMAX;  // (longer rows read the query from global memory)
    if (qlds)
        for (uint32_t cc = t; cc < ld; cc += 64 * W) ldq[cc] = qrow[cc];
    __syncthreads();
    const uint32_t total = s_pre[cnt];
    unsigned long long* const tab =
        SPLIT ? reinterpret_cast<unsigned long long*>(a.table) + (uint64_t)q * k * m : s_tab;
    const uint64_t mask = a.allow && a.query_mask ? a.query_mask[q] : 0u;
    const uint32_t* const aw =
        a.allow ? reinterpret_cast<const uint32_t*>(a.allow + mask * a.allow_words) : nullptr;
    const float mag_b = a.nb[q];
    for (;;) {
        uint32_t it = 0;
        if (lane == 0) it = atomicAdd(&s_next, 1u);
        it = (uint32_t)__builtin_amdgcn_readfirstlane((int)it);
        if (it >= hi) break;
        const uint64_t p = (uint64_t)it * 64 + lane;
        const bool inlist = p < total;
        uint32_t g0 = 0, g1 = cnt;  // (the slot lies in [g0, g1); cnt >= 1 wherever an item exists)
        while (g1 - g0 > 1) {
            const uint32_t mid = (g0 + g1) >> 1;
            if (s_pre[mid] <= p) g0 = mid;
            else g1 = mid;
        }
        const uint32_t r = inlist ? a.glist[s_first[g0] + (uint32_t)(p - s_pre[g0])] : 0u;
        bool live = row_live(a.dead, r, inlist);
        if (live && aw) live = (aw[r >> 5] >> (r & 31)) & 1u;
        if (!__ballot(live)) continue;  // (uniform over the wave)
        const uint32_t myrow = live ? r : 0u;
        float acc[1] = {-0.0f}, mx[1] = {0.0f};
        wave_walk_rows(lds, a.rows, ld, a.dim, myrow, qlds ? ldq : qrow, lane, acc, mx);
        const float d = finish_distance(acc[0], mx[0], a.na[myrow], mag_b);
        if (live) cap_insert(tab + (uint64_t)g0 * m, m, dist_key(d, myrow));
    }
    if (SPLIT) return;
    __syncthreads();
    groups_emit(a, q, s_tab, cnt);  // (a wave per group: 256 groups a wave at k = 1024)
}

// One workgroup per query, the short ones exiting: row q of the global table through groups_emit.
__global__ __launch_bounds__(256) void k_groups_deep_finish(GroupsDeepArgs a) {
    const uint32_t q = blockIdx.x;
    if (a.items[q] <= a.budget) return;
    const uint32_t cnt = a.head_cnt[q] < a.k ? a.head_cnt[q] : a.k;
    groups_emit(a, q, reinterpret_cast<const unsigned long long*>(a.table) + (uint64_t)q * a.k * a.m, cnt);
}

// ------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------
static inline uint32_t grid_for(uint64_t work, uint32_t block, uint32_t cap = 65536) {
    uint64_t g = (work + block - 1) / block;
    if (g < 1) g = 1;
    return (uint32_t)(g > cap ? cap : g);
}

hipError_t launch_groups_invert(const uint32_t* row_group, uint64_t n, uint32_t n_groups, uint32_t* gcnt,
                                uint32_t* gpos, uint32_t* cursor, uint32_t* glist, hipStream_t s) {
    if (!n) return hipSuccess;
    if (!n_groups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_groups_count, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, row_group, n, gcnt);
    hipLaunchKernelGGL(k_groups_offsets, dim3(grid_for(n_groups, 256, 4096)), dim3(256), 0, s, gcnt, n_groups, cursor,
                       gpos);
    hipLaunchKernelGGL(k_groups_scatter, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, row_group, n, gpos, glist);
    return hipGetLastError();
}

static bool groups_shape_ok(const GroupsFillArgs& a) {
    return a.k && a.k <= kCollapseMaxFetch && a.m && a.m <= kGroupsMaxRows && a.k * a.m <= kGroupsMaxSlots;
}

hipError_t launch_groups_fill(const GroupsFillArgs& a, hipStream_t s) {
    if (!a.nq) return hipSuccess;
    if (!groups_shape_ok(a) || !a.split_items) return hipErrorInvalidValue;
    // (a table of at most 512 entries leaves room for two workgroups on a CU)
    if (a.k * a.m <= 512) hipLaunchKernelGGL((k_groups_fill<512, false>), dim3(a.nq), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_groups_fill<(int)kGroupsMaxSlots, false>), dim3(a.nq), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_groups_fill_split(const GroupsFillArgs& a, uint32_t n_split, uint32_t parts, hipStream_t s) {
    if (!n_split) return hipSuccess;
    if (!groups_shape_ok(a) || !parts || parts > 65535u || !a.table) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_groups_fill<1, true>), dim3(n_split, parts), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_groups_finish(const GroupsFillArgs& a, uint32_t n_split, hipStream_t s) {
    if (!n_split) return hipSuccess;
    if (!groups_shape_ok(a) || !a.table) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_groups_finish, dim3(n_split), dim3(256), 0, s, a);
    return hipGetLastError();
}

static bool groups_deep_shape_ok(const GroupsDeepArgs& a) {
    return a.k && a.k <= kDeepMaxK && a.m && a.m <= kGroupsMaxRows && a.k * a.m <= kDeepGroupsMaxSlots && a.pre &&
           a.first && a.items && a.info;
}

// The budget B = max(split_items, the batch's items over four workgroups a compute unit): a large
// batch keeps every ordinary query on one workgroup and a single long query still covers the chip.
uint32_t groups_deep_budget(uint64_t total_items, uint32_t split_items) {
    static const uint32_t cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
            n = 256;
        (void)hipGetLastError();
        return (uint32_t)n;
    }();
    const uint64_t share = (total_items + 4ull * cus - 1) / (4ull * cus);
    const uint64_t b = share > split_items ? share : split_items;
    return (uint32_t)(b > 0xFFFFFFFFull ? 0xFFFFFFFFull : b);
}

hipError_t launch_groups_deep_plan(const GroupsDeepArgs& a, hipStream_t s) {
    if (!a.nq) return hipSuccess;
    if (!groups_deep_shape_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_groups_deep_plan, dim3(a.nq), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_groups_fill_deep(const GroupsDeepArgs& a, hipStream_t s) {
    if (!a.nq) return hipSuccess;
    if (!groups_deep_shape_ok(a) || !a.budget) return hipErrorInvalidValue;
    if (a.k * a.m <= 2048) hipLaunchKernelGGL((k_groups_fill_deep<2048, false>), dim3(a.nq), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_groups_fill_deep<(int)kDeepGroupsMaxSlots, false>), dim3(a.nq), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_groups_fill_deep_split(const GroupsDeepArgs& a, uint32_t parts, hipStream_t s) {
    if (!a.nq) return hipSuccess;
    if (!groups_deep_shape_ok(a) || !a.budget || !parts || parts > 1024u || !a.table) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_groups_fill_deep<1, true>), dim3(a.nq, parts), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_groups_deep_finish(const GroupsDeepArgs& a, hipStream_t s) {
    if (!a.nq) return hipSuccess;
    if (!groups_deep_shape_ok(a) || !a.budget || !a.table) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_groups_deep_finish, dim3(a.nq), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace bsr
