// Positions of given (query, item) pairs in the full-catalogue ranking, and their scores -- what the reference would get
// from the whole (U, N) matrix of test() (macr_mf/train.py:224-251) followed by a full sort (ranklist_by_sorted), for
// the pairs alone: the position of a held-out item wherever it stands, not only inside the first K.
//
// The score is the one arithmetic of the evaluator (common.hpp::exact_score = the k-ascending fmaf chain + score_epilogue,
// which is also what the fp32 MFMA tile accumulates), the order the one rule (make_key: score descending, id ascending),
// so a position is an integer and exact.
//
//   k_score_pairs   one lane per pair: the exact score, and for the counting pass the pair's key (the "threshold")
//   k_rank_cols     cuts every query's pair list into columns of <= kColPairs pairs.  A column is what a lane column of
//                   the MFMA tile serves: a wave costs as much as its longest column, and a query with 1 000 pairs would
//                   otherwise hold its 31 neighbours up.  A query without pairs gets no column and costs nothing.
//   k_rank_count    U.I^T on v_mfma_f32_32x32x2_f32 over ALL local items, one column per lane column and 16 items per lane
//                   (the tile of k_score_stream); instead of listing, a score is compared with the column's thresholds and
//                   per-lane counters are bumped; they are added into per-pair counters when the column block's tile range
//                   ends.  Integer adds: the order of arrival does not matter.  The hot compare is on the floats (one v_cmp
//                   per score and threshold); an exact tie is seen by a second compare and settled by id on a rare path.
//   k_rank_finish   one wave per query: the count over all items minus the query's masked items that rank before the pair
//                   (their exact keys: sum |mask_q| row gathers, not a mask test per score in the big kernel), -1 for a
//                   pair that is masked, outside the shard or NaN.
//
// The item-sharded form (macr_rank_shard_*, SHARD = true below): local row l of the table is global item item_lo +
// l * item_stride, pair and mask ids are global, and the keys come from outside -- complete, i.e. summed over the shards
// (k_rank_shard_keys: an owner's key, 0 from everybody else).  k_rank_count and k_rank_finish are the same kernels with the
// candidate's GLOBAL id in the tie path and the ownership test on every mask entry; a shard's counts are int64 and add up
// over the shards to the position (k_rank_shard_combine).
#include <algorithm>
#include <type_traits>

#include "common.hpp"

namespace macr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kColPairs = 16;                 // thresholds a lane column carries
constexpr int kRankTile = 32;                 // MFMA tile: 32 items x 32 columns
constexpr int kRankWaves = 8;
constexpr int kRankCols = 32 * kRankWaves;    // columns per block
constexpr int kRankThreads = 64 * kRankWaves;
constexpr uint64_t kNoKey = ~0ull;            // a pair that has no position: no real key has these bits (the high word is a NaN's)
constexpr uint64_t kNoOwner = 0ull;           // sharded keys: no shard owns the pair's item (no real key: its low word would name id -1)

struct RankCol { int32_t q, p0, n, pad; };    // query, first pair, pairs (1..kColPairs)

template <int D>
struct RankCfg {
    static constexpr int RS = D + 4;          // LDS row stride (floats): see k_score_stream
    static constexpr int NT = D / 2;          // MFMA steps per tile
    static constexpr int LD4 = (kRankTile * D / 4 + kRankThreads - 1) / kRankThreads;
    static constexpr size_t smem = (size_t)2 * kRankTile * RS * 4 + 2 * kRankTile * 4;
};

// the query of pair p: the last q with pair_ptr[q] <= p (queries without pairs are stepped over)
__device__ __forceinline__ int pair_query(const int32_t *__restrict__ pair_ptr, int U, long long p) {
    int lo = 0, hi = U;                       // first i in [1, U] with pair_ptr[i] > p, minus one
    while (lo + 1 < hi) { const int mid = (lo + hi) >> 1; if ((long long)pair_ptr[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}

// the local row of global item g in the shard (item_lo, item_stride, n_local); -1: another shard's, or no item at all
__device__ __forceinline__ int shard_local(int g, int item_lo, int item_stride, int n_local) {
    if (g < item_lo) return -1;
    const int off = g - item_lo, l = off / item_stride;
    return (l * item_stride == off && l < n_local) ? l : -1;
}

// one lane per pair: the key of a pair whose item this shard owns (exact score, GLOBAL id; kNoKey for a NaN), kNoOwner else
template <int D, int KIND>
__global__ __launch_bounds__(256) void k_rank_shard_keys(int U, int n_local, const float *__restrict__ users_tab,
                                                         const int32_t *__restrict__ user_ids, const float *__restrict__ items,
                                                         const float *__restrict__ sig_u, const float *__restrict__ sig_i,
                                                         float c_val, const float *__restrict__ c_dev, int item_lo, int item_stride,
                                                         const int32_t *__restrict__ pair_ptr, const int32_t *__restrict__ pair_item,
                                                         long long n_pairs, uint64_t *__restrict__ keys) {
    const float c = c_dev ? *c_dev : c_val;
    const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int g = pair_item[p], l = shard_local(g, item_lo, item_stride, n_local);
    uint64_t k = kNoOwner;
    if (l >= 0) {
        const float v = exact_score<D, KIND>(pair_query(pair_ptr, U, p), l, users_tab, user_ids, items, sig_u, sig_i, c);
        k = v == v ? make_key(v, g) : kNoKey;
    }
    keys[p] = k;
}

// the counting pass of a shard starts from zero counters and no columns (k_score_pairs does this for the unsharded call)
__global__ __launch_bounds__(256) void k_rank_shard_reset(long long n_pairs, uint32_t *__restrict__ counts, uint32_t *__restrict__ n_cols) {
    const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (p == 0) *n_cols = 0u;
    if (p < n_pairs) counts[p] = 0u;
}

__global__ __launch_bounds__(256) void k_rank_shard_combine(long long n_pairs, const uint64_t *__restrict__ keys,
                                                            const long long *__restrict__ summed, int32_t *__restrict__ out_pos) {
    const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const uint64_t k = keys[p];
    const long long s = summed[p];
    out_pos[p] = (k == kNoOwner || k == kNoKey || (s & MACR_RANK_SHARD_MASKED)) ? -1 : (int32_t)(s & 0x7fffffffLL);
}

template <int D, int KIND>
__global__ __launch_bounds__(256) void k_score_pairs(int U, int n_local, const float *__restrict__ users_tab,
                                                     const int32_t *__restrict__ user_ids, const float *__restrict__ items,
                                                     const float *__restrict__ sig_u, const float *__restrict__ sig_i, float c_val,
                                                     const float *__restrict__ c_dev, const int32_t *__restrict__ pair_ptr,
                                                     const int32_t *__restrict__ pair_item, long long n_pairs,
                                                     float *__restrict__ out_scores, uint64_t *__restrict__ keys,
                                                     uint32_t *__restrict__ counts, uint32_t *__restrict__ n_cols) {
    const float c = c_dev ? *c_dev : c_val;
    const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (p == 0 && n_cols) *n_cols = 0u;
    if (p >= n_pairs) return;
    const int q = pair_query(pair_ptr, U, p);
    const int it = pair_item[p];
    const bool in = it >= 0 && it < n_local;
    const float v = in ? exact_score<D, KIND>(q, it, users_tab, user_ids, items, sig_u, sig_i, c) : __builtin_nanf("");
    if (out_scores) out_scores[p] = v;
    if (keys) { keys[p] = v == v ? make_key(v, it) : kNoKey; counts[p] = 0u; }
}

__global__ __launch_bounds__(256) void k_rank_cols(int U, const int32_t *__restrict__ pair_ptr, RankCol *__restrict__ cols,
                                                   uint32_t *__restrict__ n_cols) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const int a = q < U ? pair_ptr[q] : 0, l = q < U ? pair_ptr[q + 1] - a : 0;
    const int nc = l > 0 ? (l + kColPairs - 1) / kColPairs : 0;
    int x = nc;                               // inclusive scan over the wave: one global add per wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, kWave); if (lane >= o) x += y; }
    const int total = __shfl(x, 63, kWave);
    uint32_t base = 0u;
    if (lane == 63 && total) base = atomicAdd(n_cols, (uint32_t)total);
    base = __shfl(base, 63, kWave);
    for (int k = 0; k < nc; ++k) {
        RankCol rc;
        rc.q = q; rc.p0 = a + kColPairs * k; rc.n = min(kColPairs, l - kColPairs * k); rc.pad = 0;
        cols[base + (x - nc) + k] = rc;
    }
}

template <int D, int KIND, bool SHARD>
__global__ __launch_bounds__(kRankThreads, 2) void k_rank_count(
    int U, int n_local, const float *__restrict__ users_tab, const int32_t *__restrict__ user_ids, const float *__restrict__ items,
    const float *__restrict__ sig_u, const float *__restrict__ sig_i, float c_val, const float *__restrict__ c_dev,
    const RankCol *__restrict__ cols, const uint32_t *__restrict__ n_cols_dev, const uint64_t *__restrict__ keys,
    uint32_t *__restrict__ counts, int item_lo, int item_stride) {
    using C = RankCfg<D>;
    constexpr int RS = C::RS, NT = C::NT;
    const float c = c_dev ? *c_dev : c_val;
    extern __shared__ __align__(16) unsigned char smem[];
    float *s_a = reinterpret_cast<float *>(smem);                       // [2][32][RS]: A operand as [item][h][t], k = 2t+h
    float *s_sig = s_a + 2 * kRankTile * RS;                            // [2][32]

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int uslot = wid * 32 + col;
    const int n_cols = (int)*n_cols_dev;
    const int n_cb = (n_cols + kRankCols - 1) / kRankCols;
    const int T = (n_local + kRankTile - 1) / kRankTile;

    // Work = (column block, tile) pairs in column-block-major order, cut into gridDim.x equal ranges (k_score_stream's
    // scheme): the number of columns is known on the device only, and every resident block gets the same number of tiles.
    const long long W = (long long)n_cb * T, G = gridDim.x, b = blockIdx.x;
    const long long w_end = W * (b + 1) / G;
    for (long long w = W * b / G; w < w_end;) {
        const int cb = (int)(w / T), i0 = (int)(w - (long long)cb * T);
        const int i1 = (int)min((long long)T, i0 + (w_end - w));
        w += i1 - i0;

        const int ci = cb * kRankCols + uslot;
        const bool c_ok = ci < n_cols;
        RankCol rc = {0, 0, 0, 0};
        if (c_ok) rc = cols[ci];
        float bfrag[NT];
        {
            const float *urow = users_tab + (size_t)(c_ok ? (user_ids ? user_ids[rc.q] : rc.q) : 0) * D;
#pragma unroll
            for (int t4 = 0; t4 < D / 4; ++t4) {       // k = 4*t4 .. 4*t4+3  ->  steps 2*t4 (k=+0,+1) and 2*t4+1 (k=+2,+3)
                const float4 v = c_ok ? ld4(urow + 4 * t4) : make_float4(0.f, 0.f, 0.f, 0.f);
                bfrag[2 * t4] = h ? v.y : v.x;
                bfrag[2 * t4 + 1] = h ? v.w : v.z;
            }
        }
        const float su = (score_uses_sig_u(KIND) && c_ok) ? sig_u[rc.q] : 1.0f;
        // thresholds: +inf where the column has none (nothing is above it; a +inf score ties with it and the tie path
        // finds no key there)
        float ts[kColPairs];
        uint32_t cnt[kColPairs];
#pragma unroll
        for (int j = 0; j < kColPairs; ++j) {
            const uint64_t k = j < rc.n ? keys[rc.p0 + j] : kNoKey;
            ts[j] = (k != kNoKey && !(SHARD && k == kNoOwner)) ? key_score(k) : INFINITY;
            cnt[j] = 0u;
        }
        int nmax = rc.n;                                                // wave-uniform: the longest column of the wave
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nmax = max(nmax, __shfl_xor(nmax, m, kWave));
        nmax = __builtin_amdgcn_readfirstlane(nmax);

        // staging: thread -> (item row, float4 column); k=4c..4c+3 lands as (h=0: t=2c,2c+1 <- x,z) (h=1: <- y,w)
        float4 stg[C::LD4];
        float sg = 0.f;
        auto load_tile = [&](int tile) {                                // rows past the end are clamped; their scores are poisoned
#pragma unroll
            for (int k = 0; k < C::LD4; ++k) {
                const int e = tid + kRankThreads * k, row = (e / (D / 4)) & (kRankTile - 1), c4 = e % (D / 4);
                const int it = min(tile * kRankTile + row, n_local - 1);
                stg[k] = ld4(items + (size_t)it * D + 4 * c4);
            }
            if (score_uses_sig_i(KIND)) sg = sig_i[min(tile * kRankTile + (tid & (kRankTile - 1)), n_local - 1)];
        };
        auto store_tile = [&](int buf) {
#pragma unroll
            for (int k = 0; k < C::LD4; ++k) {
                const int e = tid + kRankThreads * k, row = e / (D / 4), c4 = e % (D / 4);
                if (row < kRankTile) {
                    float *p = s_a + ((size_t)buf * kRankTile + row) * RS + 2 * c4;
                    *reinterpret_cast<float2 *>(p) = make_float2(stg[k].x, stg[k].z);
                    *reinterpret_cast<float2 *>(p + NT) = make_float2(stg[k].y, stg[k].w);
                }
            }
            if (score_uses_sig_i(KIND) && tid < kRankTile) s_sig[buf * kRankTile + tid] = sg;
        };

        int buf = 0;
        load_tile(i0);
        store_tile(0);
        __syncthreads();
        for (int t = i0; t < i1; ++t) {
            const bool has_next = t + 1 < i1;
            if (has_next) load_tile(t + 1);
            if (nmax > 0) {                                             // (a wave of padding columns only stages)
                const int valid = n_local - t * kRankTile;              // < 32 only in the last tile
                const float *ua = s_a + ((size_t)buf * kRankTile + col) * RS + h * NT;
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = ((r & 3) + 8 * (r >> 2) + 4 * h) < valid ? 0.f : __builtin_nanf("");
                float a4[4];
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) {
                    if ((tt & 3) == 0) *reinterpret_cast<float4 *>(a4) = *reinterpret_cast<const float4 *>(ua + tt);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tt & 3], bfrag[tt], acc, 0, 0, 0);
                }
                float v[16];
                if (score_uses_sig_i(KIND)) {
                    float sgi[16];
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *reinterpret_cast<float4 *>(sgi + 4 * g) = *reinterpret_cast<const float4 *>(s_sig + buf * kRankTile + 8 * g + 4 * h);
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = score_epilogue<KIND>(acc[r], c, sgi[r], su);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = acc[r];
                }
                const int id0 = t * kRankTile + 4 * h;
#pragma unroll
                for (int j = 0; j < kColPairs; ++j) {
                    if (j < nmax) {                                     // wave-uniform
                        uint64_t tie = 0ull;                            // OR of the equality masks: scalar unit
#pragma unroll
                        for (int r = 0; r < 16; ++r) {                  // (a NaN score, poisoned or computed, is above nothing)
                            cnt[j] += v[r] > ts[j] ? 1u : 0u;
                            tie |= __ballot(v[r] == ts[j]);
                        }
                        // Equal scores: the smaller id ranks first.  Every pair meets its own item once, so this runs in
                        // one tile per pair even without a single tie: the lanes that saw none have nothing to add.
                        if (tie) {
                            // (kNoKey: id 0, kNoOwner: id -1 -- nothing is before either)
                            int gj = j < rc.n ? key_id(keys[rc.p0 + j]) : -1;
                            if (SHARD) {
                                // the candidate's id is item_lo + item_stride * l: it is below gj for the local rows
                                // l < ceil((gj - item_lo) / item_stride), so the compare below stays one on local rows
                                const int num = gj - item_lo;                              // (>= -2^31: gj >= -1, item_lo >= 0)
                                gj = num <= 0 ? 0 : (num - 1) / item_stride + 1;
                            }
#pragma unroll
                            for (int r = 0; r < 16; ++r) cnt[j] += (v[r] == ts[j] && id0 + (r & 3) + 8 * (r >> 2) < gj) ? 1u : 0u;
                        }
                    }
                }
            }
            if (has_next) store_tile(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
#pragma unroll
        for (int j = 0; j < kColPairs; ++j) {
            const uint32_t s = cnt[j] + __shfl_xor(cnt[j], 32, kWave);
            if (h == 0 && j < rc.n && s) atomicAdd(&counts[rc.p0 + j], s);
        }
    }
}

// SHARD: out is long long[n_pairs], this shard's share of the position (+ MACR_RANK_SHARD_MASKED where it owns the pair's
// item and the query masks it); else int32[n_pairs], the position itself
template <int D, int KIND, bool SHARD>
__global__ __launch_bounds__(256) void k_rank_finish(int U, int n_local, const float *__restrict__ users_tab,
                                                     const int32_t *__restrict__ user_ids, const float *__restrict__ items,
                                                     const float *__restrict__ sig_u, const float *__restrict__ sig_i, float c_val,
                                                     const float *__restrict__ c_dev, const int32_t *__restrict__ mask_ptr,
                                                     const int32_t *__restrict__ mask_idx, const int32_t *__restrict__ pair_ptr,
                                                     const uint64_t *__restrict__ keys, const uint32_t *__restrict__ counts,
                                                     typename std::conditional<SHARD, long long, int32_t>::type *__restrict__ out,
                                                     int item_lo, int item_stride) {
    const float c = c_dev ? *c_dev : c_val;
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= U) return;
    const int a = pair_ptr[q], b = pair_ptr[q + 1];
    const int m0 = mask_ptr ? mask_ptr[q] : 0, m1 = mask_ptr ? mask_ptr[q + 1] : 0;
    for (int p0 = a; p0 < b; p0 += 64) {                  // 64 pairs at a time, one per lane
        const int p = p0 + lane;
        uint64_t kp = p < b ? keys[p] : kNoKey;
        if (SHARD && kp == kNoOwner) kp = kNoKey;         // (nothing is counted for it, and no mask entry equals it)
        uint32_t sub = 0u;
        bool masked = false;
        for (int e0 = m0; e0 < m1; e0 += 64) {            // 64 masked items at a time: a lane scores one, all lanes compare all
            const int e = e0 + lane;
            uint64_t km = 0ull;                           // 0: ranks before nothing (outside the shard, NaN, a repeated entry)
            if (e < m1) {
                const int it = mask_idx[e];               // (SHARD: a global id, scored at its local row, keyed by itself)
                const int l = SHARD ? shard_local(it, item_lo, item_stride, n_local) : it;
                if (l >= 0 && (SHARD || it < n_local) && !(e > m0 && mask_idx[e - 1] == it)) {
                    const float v = exact_score<D, KIND>(q, l, users_tab, user_ids, items, sig_u, sig_i, c);
                    if (v == v) km = make_key(v, it);
                }
            }
            const int ne = min(64, m1 - e0);
            for (int s = 0; s < ne; ++s) {
                const uint32_t lo = __shfl(static_cast<uint32_t>(km), s, kWave), hi = __shfl(static_cast<uint32_t>(km >> 32), s, kWave);
                const uint64_t k = (static_cast<uint64_t>(hi) << 32) | lo;
                sub += (kp != kNoKey && k > kp) ? 1u : 0u;
                masked |= k == kp;                        // the same (score, id): the pair's own item is masked
            }
        }
        if constexpr (SHARD) {
            if (p < b) out[p] = kp == kNoKey ? 0 : (long long)(counts[p] - sub) + (masked ? MACR_RANK_SHARD_MASKED : 0);
        } else {
            if (p < b) out[p] = (kp == kNoKey || masked) ? -1 : (int32_t)(counts[p] - sub);
        }
    }
}

}  // namespace macr

using namespace macr;

#define MACR_RANK_DISPATCH_K(Dv, kind, ...)                                                                           \
    switch (kind) {                                                                                                   \
        case MACR_SCORE_NORMAL:            { constexpr int D = Dv, KIND = MACR_SCORE_NORMAL; __VA_ARGS__; } break;            \
        case MACR_SCORE_RUBI_BOTH:         { constexpr int D = Dv, KIND = MACR_SCORE_RUBI_BOTH; __VA_ARGS__; } break;         \
        case MACR_SCORE_RUBI:              { constexpr int D = Dv, KIND = MACR_SCORE_RUBI; __VA_ARGS__; } break;              \
        case MACR_SCORE_DIRECT_MINUS:      { constexpr int D = Dv, KIND = MACR_SCORE_DIRECT_MINUS; __VA_ARGS__; } break;      \
        case MACR_SCORE_DIRECT_MINUS_BOTH: { constexpr int D = Dv, KIND = MACR_SCORE_DIRECT_MINUS_BOTH; __VA_ARGS__; } break; \
    }
#define MACR_RANK_DISPATCH_DK(d, kind, ...)                              \
    switch (d) {                                                         \
        case 32:  MACR_RANK_DISPATCH_K(32, kind, __VA_ARGS__); break;    \
        case 64:  MACR_RANK_DISPATCH_K(64, kind, __VA_ARGS__); break;    \
        case 128: MACR_RANK_DISPATCH_K(128, kind, __VA_ARGS__); break;   \
        case 256: MACR_RANK_DISPATCH_K(256, kind, __VA_ARGS__); break;   \
    }

static inline bool rank_kind_valid(int k) { return k >= MACR_SCORE_NORMAL && k <= MACR_SCORE_DIRECT_MINUS_BOTH; }
static inline bool rank_sizes_valid(int U, long long n_pairs, int n_local) {
    return U > 0 && n_local > 0 && n_pairs >= 0 && n_pairs <= 0x7fffffffLL;
}

// workspace: keys u64[n_pairs] | cols RankCol[max_cols] | counts u32[n_pairs] | n_cols u32  (with_keys = false: no keys part)
struct RankWs { uint64_t *keys; RankCol *cols; uint32_t *counts, *n_cols; size_t bytes; };
static RankWs carve_rank_ws(void *base, int U, long long n_pairs, bool with_keys = true) {
    // sum over queries of ceil(l / kColPairs) <= (queries with pairs) + n_pairs / kColPairs
    const size_t max_cols = (size_t)std::min<long long>(U, n_pairs) + (size_t)(n_pairs / kColPairs) + 1;
    RankWs w;
    char *p = static_cast<char *>(base);
    size_t off = 0;
    w.keys = with_keys ? reinterpret_cast<uint64_t *>(p + off) : nullptr;
    if (with_keys) off += align_up((size_t)n_pairs * 8, 16);
    w.cols = reinterpret_cast<RankCol *>(p + off);    off += max_cols * sizeof(RankCol);
    w.counts = reinterpret_cast<uint32_t *>(p + off); off += align_up((size_t)n_pairs * 4, 16);
    w.n_cols = reinterpret_cast<uint32_t *>(p + off); off += 16;
    w.bytes = off;
    return w;
}

extern "C" size_t macr_rank_positions_workspace_bytes(int U, long long n_pairs, int n_local, int d) {
    if (!rank_sizes_valid(U, n_pairs, n_local) || !dim_supported(d)) return 0;
    return carve_rank_ws(nullptr, U, n_pairs).bytes;
}

extern "C" int macr_score_pairs(int score_kind, int U, int n_local, int d, const float *users_tab, const int32_t *user_ids,
                                const float *items, const float *sig_u, const float *sig_i, float c, const float *c_dev,
                                const int32_t *pair_ptr, const int32_t *pair_item, long long n_pairs, float *out_scores,
                                void *stream) {
    hipStream_t st = as_stream(stream);
    MACR_REQUIRE(rank_kind_valid(score_kind), MACR_E_INVALID, "score_pairs: score_kind=%d", score_kind);
    MACR_REQUIRE(rank_sizes_valid(U, n_pairs, n_local), MACR_E_INVALID, "score_pairs: U=%d n_local=%d n_pairs=%lld", U, n_local, n_pairs);
    MACR_REQUIRE(dim_supported(d), MACR_E_UNSUPPORTED, "score_pairs: d=%d not in {32,64,128,256}", d);
    MACR_REQUIRE(users_tab && items && pair_ptr && (pair_item || n_pairs == 0), MACR_E_INVALID, "score_pairs: null pointer");
    MACR_REQUIRE((!score_uses_sig_i(score_kind) || sig_i) && (!score_uses_sig_u(score_kind) || sig_u), MACR_E_INVALID,
                 "score_pairs: score_kind %d needs sig_i%s", score_kind, score_uses_sig_u(score_kind) ? " and sig_u" : "");
    MACR_REQUIRE(out_scores || n_pairs == 0, MACR_E_INVALID, "score_pairs: out_scores is null");
    if (n_pairs == 0) return MACR_OK;
    const unsigned blocks = (unsigned)((n_pairs + 255) / 256);
    MACR_RANK_DISPATCH_DK(d, score_kind, (k_score_pairs<D, KIND><<<blocks, 256, 0, st>>>(
                                             U, n_local, users_tab, user_ids, items, sig_u, sig_i, c, c_dev, pair_ptr, pair_item,
                                             n_pairs, out_scores, nullptr, nullptr, nullptr)));
    MACR_CHECK_LAUNCH("score_pairs", st);
    return MACR_OK;
}

extern "C" int macr_rank_positions(int score_kind, int U, int n_local, int d, const float *users_tab, const int32_t *user_ids,
                                   const float *items, const float *sig_u, const float *sig_i, float c, const float *c_dev,
                                   const int32_t *mask_ptr, const int32_t *mask_idx, const int32_t *pair_ptr,
                                   const int32_t *pair_item, long long n_pairs, int32_t *out_pos, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    hipStream_t st = as_stream(stream);
    MACR_REQUIRE(rank_kind_valid(score_kind), MACR_E_INVALID, "rank_positions: score_kind=%d", score_kind);
    MACR_REQUIRE(rank_sizes_valid(U, n_pairs, n_local), MACR_E_INVALID, "rank_positions: U=%d n_local=%d n_pairs=%lld", U, n_local, n_pairs);
    MACR_REQUIRE(dim_supported(d), MACR_E_UNSUPPORTED, "rank_positions: d=%d not in {32,64,128,256}", d);
    MACR_REQUIRE(users_tab && items && pair_ptr && (pair_item || n_pairs == 0), MACR_E_INVALID, "rank_positions: null pointer");
    MACR_REQUIRE((!score_uses_sig_i(score_kind) || sig_i) && (!score_uses_sig_u(score_kind) || sig_u), MACR_E_INVALID,
                 "rank_positions: score_kind %d needs sig_i%s", score_kind, score_uses_sig_u(score_kind) ? " and sig_u" : "");
    MACR_REQUIRE(!mask_ptr == !mask_idx, MACR_E_INVALID, "rank_positions: mask_ptr and mask_idx go together");
    MACR_REQUIRE(out_pos || n_pairs == 0, MACR_E_INVALID, "rank_positions: out_pos is null");
    MACR_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, MACR_E_INVALID,
                 "rank_positions: workspace is null or not 16-byte aligned (macr_rank_positions_workspace_bytes)");
    const RankWs ws = carve_rank_ws(workspace, U, n_pairs);
    MACR_REQUIRE(workspace_bytes >= ws.bytes, MACR_E_WORKSPACE, "rank_positions: workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
    if (n_pairs == 0) return MACR_OK;
    const unsigned pblocks = (unsigned)((n_pairs + 255) / 256);
    const int T = (n_local + kRankTile - 1) / kRankTile;
    // blocks of 8 waves resident on 256 CUs; never more than the work has tiles (an upper bound: the columns are counted
    // on the device)
    const long long w_max = ((long long)(std::min<long long>(U, n_pairs) + n_pairs / kColPairs) / kRankCols + 1) * T;
    // (restated as geometry() of tests/rank_cases.py: its cases are placed by this arithmetic)
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(d <= 64 ? 512 : 256, w_max));
    MACR_RANK_DISPATCH_DK(d, score_kind, {
        auto count = k_rank_count<D, KIND, false>;
        const size_t smem = RankCfg<D>::smem;
        MACR_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void *>(count), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) == hipSuccess,
                     MACR_E_LAUNCH, "rank_positions: cannot reserve %zu B of LDS", smem);
        k_score_pairs<D, KIND><<<pblocks, 256, 0, st>>>(U, n_local, users_tab, user_ids, items, sig_u, sig_i, c, c_dev, pair_ptr,
                                                       pair_item, n_pairs, nullptr, ws.keys, ws.counts, ws.n_cols);
        MACR_CHECK_LAUNCH("rank_keys", st);
        k_rank_cols<<<(U + 255) / 256, 256, 0, st>>>(U, pair_ptr, ws.cols, ws.n_cols);
        MACR_CHECK_LAUNCH("rank_cols", st);
        count<<<grid, kRankThreads, smem, st>>>(U, n_local, users_tab, user_ids, items, sig_u, sig_i, c, c_dev, ws.cols, ws.n_cols,
                                                ws.keys, ws.counts, 0, 1);
        MACR_CHECK_LAUNCH("rank_count", st);
        k_rank_finish<D, KIND, false><<<(U + 3) / 4, 256, 0, st>>>(U, n_local, users_tab, user_ids, items, sig_u, sig_i, c, c_dev,
                                                                  mask_ptr, mask_idx, pair_ptr, ws.keys, ws.counts, out_pos, 0, 1);
        MACR_CHECK_LAUNCH("rank_finish", st);
    });
    return MACR_OK;
}

// ---------------------------------------------------------------------------------------------- item-sharded positions
// workspace of macr_rank_shard_counts: that of macr_rank_positions without the keys, which the caller holds
static RankWs carve_rank_shard_ws(void *base, int U, long long n_pairs) { return carve_rank_ws(base, U, n_pairs, false); }

static inline bool rank_shard_valid(int item_lo, int item_stride) { return item_lo >= 0 && item_stride >= 1; }

extern "C" size_t macr_rank_shard_workspace_bytes(int U, long long n_pairs, int n_local, int d) {
    if (!rank_sizes_valid(U, n_pairs, n_local) || !dim_supported(d)) return 0;
    return carve_rank_shard_ws(nullptr, U, n_pairs).bytes;
}

extern "C" int macr_rank_shard_keys(int score_kind, int U, int n_local, int d, const float *users_tab, const int32_t *user_ids,
                                    const float *items, const float *sig_u, const float *sig_i, float c, const float *c_dev,
                                    int item_lo, int item_stride, const int32_t *pair_ptr, const int32_t *pair_item,
                                    long long n_pairs, uint64_t *out_keys, void *stream) {
    hipStream_t st = as_stream(stream);
    MACR_REQUIRE(rank_kind_valid(score_kind), MACR_E_INVALID, "rank_shard_keys: score_kind=%d", score_kind);
    MACR_REQUIRE(rank_sizes_valid(U, n_pairs, n_local), MACR_E_INVALID, "rank_shard_keys: U=%d n_local=%d n_pairs=%lld", U, n_local, n_pairs);
    MACR_REQUIRE(rank_shard_valid(item_lo, item_stride), MACR_E_INVALID, "rank_shard_keys: item_lo=%d item_stride=%d", item_lo, item_stride);
    MACR_REQUIRE(dim_supported(d), MACR_E_UNSUPPORTED, "rank_shard_keys: d=%d not in {32,64,128,256}", d);
    MACR_REQUIRE(users_tab && items && pair_ptr && (pair_item || n_pairs == 0), MACR_E_INVALID, "rank_shard_keys: null pointer");
    MACR_REQUIRE((!score_uses_sig_i(score_kind) || sig_i) && (!score_uses_sig_u(score_kind) || sig_u), MACR_E_INVALID,
                 "rank_shard_keys: score_kind %d needs sig_i%s", score_kind, score_uses_sig_u(score_kind) ? " and sig_u" : "");
    MACR_REQUIRE(out_keys || n_pairs == 0, MACR_E_INVALID, "rank_shard_keys: out_keys is null");
    if (n_pairs == 0) return MACR_OK;
    const unsigned pblocks = (unsigned)((n_pairs + 255) / 256);
    MACR_RANK_DISPATCH_DK(d, score_kind, (k_rank_shard_keys<D, KIND><<<pblocks, 256, 0, st>>>(
                                             U, n_local, users_tab, user_ids, items, sig_u, sig_i, c, c_dev, item_lo, item_stride,
                                             pair_ptr, pair_item, n_pairs, out_keys)));
    MACR_CHECK_LAUNCH("rank_shard_keys", st);
    return MACR_OK;
}

extern "C" int macr_rank_shard_counts(int score_kind, int U, int n_local, int d, const float *users_tab, const int32_t *user_ids,
                                      const float *items, const float *sig_u, const float *sig_i, float c, const float *c_dev,
                                      int item_lo, int item_stride, const int32_t *mask_ptr, const int32_t *mask_idx,
                                      const int32_t *pair_ptr, const uint64_t *keys, long long n_pairs, long long *out_cnt,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    hipStream_t st = as_stream(stream);
    MACR_REQUIRE(rank_kind_valid(score_kind), MACR_E_INVALID, "rank_shard_counts: score_kind=%d", score_kind);
    MACR_REQUIRE(rank_sizes_valid(U, n_pairs, n_local), MACR_E_INVALID, "rank_shard_counts: U=%d n_local=%d n_pairs=%lld", U, n_local, n_pairs);
    MACR_REQUIRE(rank_shard_valid(item_lo, item_stride), MACR_E_INVALID, "rank_shard_counts: item_lo=%d item_stride=%d", item_lo, item_stride);
    MACR_REQUIRE(dim_supported(d), MACR_E_UNSUPPORTED, "rank_shard_counts: d=%d not in {32,64,128,256}", d);
    MACR_REQUIRE(users_tab && items && pair_ptr && (keys || n_pairs == 0), MACR_E_INVALID, "rank_shard_counts: null pointer");
    MACR_REQUIRE((!score_uses_sig_i(score_kind) || sig_i) && (!score_uses_sig_u(score_kind) || sig_u), MACR_E_INVALID,
                 "rank_shard_counts: score_kind %d needs sig_i%s", score_kind, score_uses_sig_u(score_kind) ? " and sig_u" : "");
    MACR_REQUIRE(!mask_ptr == !mask_idx, MACR_E_INVALID, "rank_shard_counts: mask_ptr and mask_idx go together");
    MACR_REQUIRE(out_cnt || n_pairs == 0, MACR_E_INVALID, "rank_shard_counts: out_cnt is null");
    MACR_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, MACR_E_INVALID,
                 "rank_shard_counts: workspace is null or not 16-byte aligned (macr_rank_shard_workspace_bytes)");
    const RankWs ws = carve_rank_shard_ws(workspace, U, n_pairs);
    MACR_REQUIRE(workspace_bytes >= ws.bytes, MACR_E_WORKSPACE, "rank_shard_counts: workspace %zu < %zu bytes", workspace_bytes, ws.bytes);
    if (n_pairs == 0) return MACR_OK;
    const unsigned pblocks = (unsigned)((n_pairs + 255) / 256);
    const int T = (n_local + kRankTile - 1) / kRankTile;
    const long long w_max = ((long long)(std::min<long long>(U, n_pairs) + n_pairs / kColPairs) / kRankCols + 1) * T;      // as macr_rank_positions
    // (restated as geometry() of tests/rank_cases.py: its cases are placed by this arithmetic)
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(d <= 64 ? 512 : 256, w_max));
    MACR_RANK_DISPATCH_DK(d, score_kind, {
        auto count = k_rank_count<D, KIND, true>;
        const size_t smem = RankCfg<D>::smem;
        MACR_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void *>(count), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) == hipSuccess,
                     MACR_E_LAUNCH, "rank_shard_counts: cannot reserve %zu B of LDS", smem);
        k_rank_shard_reset<<<pblocks, 256, 0, st>>>(n_pairs, ws.counts, ws.n_cols);
        MACR_CHECK_LAUNCH("rank_shard_reset", st);
        k_rank_cols<<<(U + 255) / 256, 256, 0, st>>>(U, pair_ptr, ws.cols, ws.n_cols);
        MACR_CHECK_LAUNCH("rank_shard_cols", st);
        count<<<grid, kRankThreads, smem, st>>>(U, n_local, users_tab, user_ids, items, sig_u, sig_i, c, c_dev, ws.cols, ws.n_cols,
                                                keys, ws.counts, item_lo, item_stride);
        MACR_CHECK_LAUNCH("rank_shard_count", st);
        k_rank_finish<D, KIND, true><<<(U + 3) / 4, 256, 0, st>>>(U, n_local, users_tab, user_ids, items, sig_u, sig_i, c, c_dev,
                                                                 mask_ptr, mask_idx, pair_ptr, keys, ws.counts, out_cnt, item_lo,
                                                                 item_stride);
        MACR_CHECK_LAUNCH("rank_shard_finish", st);
    });
    return MACR_OK;
}

extern "C" int macr_rank_shard_combine(long long n_pairs, const uint64_t *keys, const long long *summed_cnt, int32_t *out_pos,
                                       void *stream) {
    hipStream_t st = as_stream(stream);
    MACR_REQUIRE(n_pairs >= 0 && n_pairs <= 0x7fffffffLL, MACR_E_INVALID, "rank_shard_combine: n_pairs=%lld", n_pairs);
    MACR_REQUIRE((keys && summed_cnt && out_pos) || n_pairs == 0, MACR_E_INVALID, "rank_shard_combine: null pointer");
    if (n_pairs == 0) return MACR_OK;
    k_rank_shard_combine<<<(unsigned)((n_pairs + 255) / 256), 256, 0, st>>>(n_pairs, keys, summed_cnt, out_pos);
    MACR_CHECK_LAUNCH("rank_shard_combine", st);
    return MACR_OK;
}
