// Per-item counts of an evaluation's ranking -- the device half of the reference's item_acc_list
// (macr_mf/train.py:261-277, k = 5; macr_lightgcn/utility/batch_test.py:94-115, k = 20): for every item, how many users
// have it among their first k ranked ids (rec_cnt) and how many of those hold it in their ground truth (hit_cnt).
//
// Form: LDS bins before any global add.  Recommendation lists follow the catalogue's Zipf head -- at
// 10^7 users x k entries most entries name a few thousand items -- so one global atomic per entry would funnel into a
// few addresses.  A workgroup keeps an open-addressed table of kItemBins (id -> {rec, hit}) in LDS: an entry claims a
// slot with one LDS compare-and-swap (or finds its id there) and adds to the slot's 64-bit counter pair with ONE LDS
// atomic; equal ids of a wave and of the workgroup meet in the slot.  A slot is claimed by the first id that hashes to
// it, which for a skewed stream is a hot id with overwhelming probability; an entry that finds its kItemProbes slots
// taken by other ids goes to global memory directly (the cold tail, spread over many addresses).  At the end the
// workgroup adds each occupied slot to global memory once: a hot item costs one global atomic per workgroup instead of
// one per entry.  Those adds still meet at the hot items' addresses -- a chain of one add per workgroup, about 0.2 us a
// link by the first version's time (1 205 workgroups adding straight into the outputs: 252 us at the Gowalla shape) -- so the workgroups add
// into kItemReplicas copies of a packed {rec, hit} 64-bit counter per item in the workspace (copy = block % kItemReplicas:
// the chain is an eighth as long, and rec and hit travel in one add), and a last launch sums the copies into the outputs
// with plain stores and forms the group sums on the way.  Integer adds: the counts are exact and do not depend on the
// order of arrival.
#include "common.hpp"

namespace macr {

constexpr int kItemBinBits = 11, kItemBins = 1 << kItemBinBits;   // 2048 slots x (4 + 8) B = 24 KB of LDS
constexpr int kItemProbes = 4;
constexpr int kItemThreads = 1024;
constexpr int kItemMaxBlocks = 1024;      // beyond this a block takes several tiles of 1024 entries: more entries per flush
constexpr int kItemReplicas = 8;          // copies of the per-item counters the workgroups spread their adds over

__device__ __forceinline__ bool item_in_sorted(const int32_t *a, int n, int32_t x) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo < n && a[lo] == x;
}

__global__ __launch_bounds__(256) void k_item_zero(unsigned long long *__restrict__ packed, size_t n_words,
                                                   long long *__restrict__ group_out, int n_group_words) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    for (size_t i = t; i < n_words; i += (size_t)gridDim.x * blockDim.x) packed[i] = 0ull;
    if (group_out && t < (size_t)n_group_words) group_out[t] = 0;
}

// n_entries = U * k entries (u, p), p < k, entry e = u * k + p, read from rankings[u * K + p]: runs of k consecutive ids.
// packed: kItemReplicas x n_items counters, low word rec, high word hit (rec <= U < 2^31: no carry into hit)
__global__ __launch_bounds__(kItemThreads) void k_item_counts(long long n_entries, int K, int k, int n_items,
                                                              const int32_t *__restrict__ rankings,
                                                              const int32_t *__restrict__ gt_ptr, const int32_t *__restrict__ gt_idx,
                                                              unsigned long long *__restrict__ packed) {
    unsigned long long *mine = packed + (size_t)(blockIdx.x % kItemReplicas) * n_items;
    __shared__ int32_t keys[kItemBins];
    __shared__ unsigned long long cnts[kItemBins];       // low word: rec, high word: hit (rec < 2^32 per block: no carry)
    for (int s = threadIdx.x; s < kItemBins; s += kItemThreads) { keys[s] = -1; cnts[s] = 0ull; }
    __syncthreads();
    for (long long e0 = (long long)blockIdx.x * kItemThreads; e0 < n_entries; e0 += (long long)gridDim.x * kItemThreads) {
        if (e0 + threadIdx.x >= n_entries) continue;
        // the tile's first user once per wave (uniform 64-bit division), the lane's own by a 32-bit one
        const long long u0 = n_entries <= 0x7fffffffLL ? (long long)((unsigned)e0 / (unsigned)k) : e0 / k;
        const unsigned r = (unsigned)(e0 - u0 * k) + threadIdx.x;
        const long long u = u0 + r / (unsigned)k;
        const int p = (int)(r % (unsigned)k);
        const int32_t id = rankings[(size_t)u * K + p];
        if (id < 0 || id >= n_items) continue;            // -1 = unused slot; an id outside the catalogue is never counted
        const int a = gt_ptr[u], b = gt_ptr[u + 1];
        const bool hit = item_in_sorted(gt_idx + a, b - a, id);
        const unsigned long long inc = hit ? ((1ull << 32) | 1ull) : 1ull;
        const unsigned h = ((unsigned)id * 2654435761u) >> (32 - kItemBinBits);
        bool binned = false;
#pragma unroll
        for (int probe = 0; probe < kItemProbes && !binned; ++probe) {
            const int s = (h + probe) & (kItemBins - 1);
            int32_t owner = keys[s];
            if (owner == -1) owner = atomicCAS(&keys[s], -1, id);       // -1: this lane claimed the slot
            if (owner == -1 || owner == id) { atomicAdd(&cnts[s], inc); binned = true; }
        }
        if (!binned) atomicAdd(&mine[id], inc);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kItemBins; s += kItemThreads) {
        const int32_t id = keys[s];
        if (id < 0) continue;
        atomicAdd(&mine[id], cnts[s]);
    }
}

// rec_cnt[i], hit_cnt[i] = the sum of item i's copies (plain stores: the outputs need no zero-fill), and with group_of
// group_out[2 g] += rec, group_out[2 g + 1] += hit over the items of group g (LDS bins, one global add per block and sum)
__global__ __launch_bounds__(256) void k_item_finish(int n_items, const unsigned long long *__restrict__ packed,
                                                     const int32_t *__restrict__ group_of, int n_groups,
                                                     int32_t *__restrict__ rec_cnt, int32_t *__restrict__ hit_cnt,
                                                     unsigned long long *__restrict__ group_out) {
    __shared__ unsigned long long sums[128];
    if (threadIdx.x < 128) sums[threadIdx.x] = 0ull;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += gridDim.x * blockDim.x) {
        unsigned long long c = 0ull;
#pragma unroll
        for (int r = 0; r < kItemReplicas; ++r) c += packed[(size_t)r * n_items + i];
        const unsigned rec = (unsigned)c, hit = (unsigned)(c >> 32);
        rec_cnt[i] = (int32_t)rec;
        hit_cnt[i] = (int32_t)hit;
        if (!group_out || rec == 0) continue;             // (hit <= rec: nothing to add either)
        const int g = group_of[i];
        if (g < 0 || g >= n_groups) continue;             // an item outside every group is in no sum
        atomicAdd(&sums[2 * g], (unsigned long long)rec);
        if (hit) atomicAdd(&sums[2 * g + 1], (unsigned long long)hit);
    }
    __syncthreads();
    if (group_out && threadIdx.x < 2 * n_groups && sums[threadIdx.x]) atomicAdd(&group_out[threadIdx.x], sums[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Position-weighted exposure (macr_item_exposure): per item the sum of pos_weight[p] over the entries (u, p < k) that name
// it (exp_w) and over those of them whose user's ground truth holds it (hit_w).  The form of k_item_counts with 64-bit
// sums: a slot is {key, exp, hit} = 4 + 8 + 8 bytes, so the table of kExpBins slots takes 40 KB of LDS; an entry claims
// its slot with one LDS compare-and-swap and adds its weight to the slot's exp sum, and to its hit sum when it is a hit
// (most entries are not: the second LDS add is skipped for them, adding zero would change nothing).  An entry whose
// kItemProbes slots belong to other ids adds to global memory directly.  The workgroups add their occupied slots into
// kExpReplicas copies of an {exp, hit} pair of 64-bit counters per item (16 bytes, the two adds of a flush meet one
// cache line), and k_exposure_finish sums the copies into the outputs with plain stores.  Unlike k_item_counts a
// workgroup takes a CONTIGUOUS run of tiles (tiles_per_block): consecutive users' lists, whose ground-truth rows are
// neighbours too.  Unsigned 64-bit integer adds throughout: exact, and independent of the order of arrival.
constexpr int kExpBinBits = 11, kExpBins = MACR_ITEM_EXPOSURE_BINS;      // 2048 slots x (4 + 8 + 8) B = 40 KB of LDS
constexpr int kExpThreads = MACR_ITEM_EXPOSURE_TILE;                      // one tile = one entry per thread
constexpr int kExpMaxBlocks = MACR_ITEM_EXPOSURE_MAX_BLOCKS;
constexpr int kExpReplicas = MACR_ITEM_EXPOSURE_REPLICAS;
static_assert(kExpBins == 1 << kExpBinBits, "the hash keeps kExpBinBits bits");
static_assert(kExpThreads == 1024 && kExpBins % kExpThreads == 0, "the tile is the workgroup");

// acc: kExpReplicas x n_items x {exp, hit}
__global__ __launch_bounds__(kExpThreads) void k_item_exposure(long long n_entries, long long tiles_per_block, int K, int k, int n_items,
                                                               const int32_t *__restrict__ rankings,
                                                               const int32_t *__restrict__ gt_ptr, const int32_t *__restrict__ gt_idx,
                                                               const uint32_t *__restrict__ pos_weight,
                                                               unsigned long long *__restrict__ acc) {
    unsigned long long *mine = acc + (size_t)(blockIdx.x % kExpReplicas) * n_items * 2;
    __shared__ int32_t keys[kExpBins];
    __shared__ unsigned long long exps[kExpBins];
    __shared__ unsigned long long hits[kExpBins];
    for (int s = threadIdx.x; s < kExpBins; s += kExpThreads) { keys[s] = -1; exps[s] = 0ull; hits[s] = 0ull; }
    __syncthreads();
    const long long first = (long long)blockIdx.x * tiles_per_block * kExpThreads;
    for (long long t = 0; t < tiles_per_block; ++t) {
        const long long e0 = first + t * kExpThreads;
        if (e0 + threadIdx.x >= n_entries) break;         // (entries ascend with t: nothing further for this lane)
        // the tile's first user once per wave (uniform 64-bit division), the lane's own by a 32-bit one
        const long long u0 = n_entries <= 0x7fffffffLL ? (long long)((unsigned)e0 / (unsigned)k) : e0 / k;
        const unsigned r = (unsigned)(e0 - u0 * k) + threadIdx.x;
        const long long u = u0 + r / (unsigned)k;
        const int p = (int)(r % (unsigned)k);
        const int32_t id = rankings[(size_t)u * K + p];
        if (id < 0 || id >= n_items) continue;            // -1 = unused slot; an id outside the catalogue is never counted
        const int a = gt_ptr[u], b = gt_ptr[u + 1];
        const bool hit = item_in_sorted(gt_idx + a, b - a, id);
        const unsigned long long wgt = pos_weight[p];
        const unsigned h = ((unsigned)id * 2654435761u) >> (32 - kExpBinBits);
        bool binned = false;
#pragma unroll
        for (int probe = 0; probe < kItemProbes && !binned; ++probe) {
            const int s = (h + probe) & (kExpBins - 1);
            int32_t owner = keys[s];
            if (owner == -1) owner = atomicCAS(&keys[s], -1, id);       // -1: this lane claimed the slot
            if (owner == -1 || owner == id) {
                atomicAdd(&exps[s], wgt);
                if (hit) atomicAdd(&hits[s], wgt);
                binned = true;
            }
        }
        if (!binned) {
            atomicAdd(&mine[2 * (size_t)id], wgt);
            if (hit) atomicAdd(&mine[2 * (size_t)id + 1], wgt);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kExpBins; s += kExpThreads) {
        const int32_t id = keys[s];
        if (id < 0) continue;
        if (exps[s]) atomicAdd(&mine[2 * (size_t)id], exps[s]);
        if (hits[s]) atomicAdd(&mine[2 * (size_t)id + 1], hits[s]);
    }
}

// exp_w[i], hit_w[i] = the sum of item i's copies (plain stores: the outputs need no zero-fill), and with group_of
// group_out[2 g] += exp, group_out[2 g + 1] += hit over the items of group g (LDS bins, one global add per block and sum)
__global__ __launch_bounds__(256) void k_exposure_finish(int n_items, const ulonglong2 *__restrict__ acc,
                                                         const int32_t *__restrict__ group_of, int n_groups,
                                                         unsigned long long *__restrict__ exp_w, unsigned long long *__restrict__ hit_w,
                                                         unsigned long long *__restrict__ group_out) {
    __shared__ unsigned long long sums[128];
    if (threadIdx.x < 128) sums[threadIdx.x] = 0ull;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += gridDim.x * blockDim.x) {
        unsigned long long e = 0ull, h = 0ull;
#pragma unroll
        for (int r = 0; r < kExpReplicas; ++r) {
            const ulonglong2 c = acc[(size_t)r * n_items + i];
            e += c.x;
            h += c.y;
        }
        exp_w[i] = e;
        hit_w[i] = h;
        if (!group_out || e == 0) continue;               // (hit <= exp: nothing to add either)
        const int g = group_of[i];
        if (g < 0 || g >= n_groups) continue;             // an item outside every group is in no sum
        atomicAdd(&sums[2 * g], e);
        if (h) atomicAdd(&sums[2 * g + 1], h);
    }
    __syncthreads();
    if (group_out && threadIdx.x < 2 * n_groups && sums[threadIdx.x]) atomicAdd(&group_out[threadIdx.x], sums[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Two rankings of the same queries, list by list (macr_list_shift, MACR_SHIFT_REPORT): what the second ("here") replaced
// of the first ("base"), how high up, and what that did to the hits.  One wave per query, kShiftQueries queries per
// workgroup; both rows' first k slots sit in LDS (k <= MACR_MAX_TOPK = 128: one or two entries per lane).  An entry finds
// its id in the other row by k broadcast LDS reads; an id that is valid and absent there has entered (here) or left
// (base), and its output slot in ascending id order is the number of smaller entered (left) ids, counted by k more
// broadcast reads -- no sort.  The eight per-query integers are popcounts of 64-bit ballots and one wave sum, written by
// lane 0 as one 32-byte row.  Every output element of a query is stored exactly once: no atomics, nothing to zero.
constexpr int kShiftQueries = 4;
constexpr int kShiftAbsent = 0x7fffffff;             // in the entered / left scratch rows: not an entered / left id
static_assert(MACR_MAX_TOPK == 2 * kWave, "a lane holds at most two entries of a row");

__device__ __forceinline__ int shift_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__global__ __launch_bounds__(kShiftQueries * kWave) void k_list_shift(int U, int K_base, int K_here, int k, int n_items,
                                                                     const int32_t *__restrict__ rank_base,
                                                                     const int32_t *__restrict__ rank_here,
                                                                     const int32_t *__restrict__ gt_ptr, const int32_t *__restrict__ gt_idx,
                                                                     int32_t *__restrict__ per_user, int32_t *__restrict__ entered,
                                                                     int32_t *__restrict__ left) {
    __shared__ int32_t rows[kShiftQueries][4][MACR_MAX_TOPK];        // base, here, left ids, entered ids: 8 KB
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const long long u = (long long)blockIdx.x * kShiftQueries + wave;
    const bool live = u < U;                          // (a wave past the last query still meets the barriers)
    int32_t *sb = rows[wave][0], *sh = rows[wave][1], *sl = rows[wave][2], *se = rows[wave][3];
    int32_t idb[2], idh[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = lane + j * kWave;
        idb[j] = idh[j] = -1;
        if (live && p < k) {
            idb[j] = rank_base[(size_t)u * K_base + p];
            idh[j] = rank_here[(size_t)u * K_here + p];
            sb[p] = idb[j];
            sh[p] = idh[j];
        }
    }
    __syncthreads();
    const int a = live ? gt_ptr[u] : 0, n_gt = live ? gt_ptr[u + 1] - a : 0;
    int n_base = 0, n_here = 0, common = 0, first_diff = k, footrule = 0, hits_base = 0, hits_here = 0, hits_common = 0;
    bool is_left[2] = {false, false}, is_entered[2] = {false, false};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j * kWave >= k) break;                    // (uniform: k <= 64 has no second entry in any lane)
        const int p = lane + j * kWave;
        const bool mine = live && p < k;
        const bool vb = mine && idb[j] >= 0 && idb[j] < n_items, vh = mine && idh[j] >= 0 && idh[j] < n_items;
        int at_base = -1, at_here = -1;               // where the here id stands in base, the base id in here
        for (int q = 0; q < k; ++q) {                 // (rows without repeated ids: at most one slot matches)
            if (vh && sb[q] == idh[j]) at_base = q;
            if (vb && sh[q] == idb[j]) at_here = q;
        }
        const bool kept = at_base >= 0;
        const bool hit_b = vb && item_in_sorted(gt_idx + a, n_gt, idb[j]);
        const bool hit_h = vh && item_in_sorted(gt_idx + a, n_gt, idh[j]);
        is_left[j] = vb && at_here < 0;
        is_entered[j] = vh && !kept;
        if (mine) {
            sl[p] = is_left[j] ? idb[j] : kShiftAbsent;
            se[p] = is_entered[j] ? idh[j] : kShiftAbsent;
        }
        n_base += __popcll(__ballot(vb));
        n_here += __popcll(__ballot(vh));
        common += __popcll(__ballot(kept));
        hits_base += __popcll(__ballot(hit_b));
        hits_here += __popcll(__ballot(hit_h));
        hits_common += __popcll(__ballot(hit_h && kept));
        footrule += kept ? (at_base > p ? at_base - p : p - at_base) : 0;
        const unsigned long long differ = __ballot(mine && idb[j] != idh[j]);       // raw slots, -1 included
        if (differ && first_diff == k) first_diff = j * kWave + __ffsll((long long)differ) - 1;
    }
    footrule = shift_wave_sum(footrule);
    __syncthreads();
    int total_left = 0, total_entered = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        total_left += __popcll(__ballot(is_left[j]));
        total_entered += __popcll(__ballot(is_entered[j]));
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = lane + j * kWave;
        if (!live || p >= k) continue;
        // ascending slot = the smaller ids of the same list (an equal id further left counts too: a row that repeats an
        // id against the contract still fills every slot once)
        int below_l = 0, below_e = 0;
        for (int q = 0; q < k; ++q) {
            const int32_t xl = sl[q], xe = se[q];
            below_l += (xl < idb[j] || (xl == idb[j] && q < p)) ? 1 : 0;
            below_e += (xe < idh[j] || (xe == idh[j] && q < p)) ? 1 : 0;
        }
        if (is_left[j]) left[(size_t)u * k + below_l] = idb[j];
        if (is_entered[j]) entered[(size_t)u * k + below_e] = idh[j];
        if (p >= total_left) left[(size_t)u * k + p] = -1;
        if (p >= total_entered) entered[(size_t)u * k + p] = -1;
    }
    if (live && lane == 0) {
        int4 *out = reinterpret_cast<int4 *>(per_user + (size_t)u * 8);
        out[0] = make_int4(n_base, n_here, common, first_diff);
        out[1] = make_int4(footrule, hits_base, hits_here, hits_common);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Per row, a histogram of item groups and a weighted sum (macr_group_hist, MACR_CALIBRATION_REPORT): the popularity mix of
// a user's list (ranking form: the first k slots of a row of stride `stride`) or of a user's profile (CSR form: the mask
// CSR's row, any length).  One wave per row, kHistRows rows per workgroup.  The wave walks its row in chunks of 64 entries:
// one coalesced read of the ids, one gather from group_of (and from item_weight) per lane, one LDS add into the wave's own
// 64 group counters, and for a list with ground truth the binary search of k_metrics_mf and a second LDS add.  The weights
// accumulate per lane in 64 bits and meet in one wave sum; the valid entries are counted by ballots.  The counters leave
// through plain stores, lane g writing column g: every output element of a row is stored exactly once -- no global atomics,
// nothing to zero, integer adds only, so the bytes do not depend on the order the lanes arrive in.
constexpr int kHistRows = 4;
constexpr int kHistGroups = 64;                      // n_groups <= 64: one counter per lane

__global__ __launch_bounds__(kHistRows * kWave) void k_group_hist(int U, const int32_t *__restrict__ row_ptr,
                                                                 const int32_t *__restrict__ ids, int stride, int k,
                                                                 const int32_t *__restrict__ gt_ptr, const int32_t *__restrict__ gt_idx,
                                                                 int n_items, const int32_t *__restrict__ group_of, int n_groups,
                                                                 const int32_t *__restrict__ item_weight, int32_t *__restrict__ cnt,
                                                                 int32_t *__restrict__ hit, long long *__restrict__ wsum) {
    __shared__ int32_t bins[kHistRows][2][kHistGroups];              // per wave: group counts, group hits -- 2 KB
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const long long u = (long long)blockIdx.x * kHistRows + wave;
    const bool live = u < U;                          // (a wave past the last row still meets the barriers)
    bins[wave][0][lane] = 0;
    bins[wave][1][lane] = 0;
    __syncthreads();
    long long first = 0;
    int len = 0, a = 0, n_gt = 0;
    if (live) {
        if (row_ptr) { first = row_ptr[u]; len = row_ptr[u + 1] - row_ptr[u]; }
        else { first = u * stride; len = k; }
        if (hit) { a = gt_ptr[u]; n_gt = gt_ptr[u + 1] - a; }
    }
    long long w = 0;
    int n_valid = 0;
    for (int p0 = 0; p0 < len; p0 += kWave) {          // (len is uniform over the wave: every lane meets the ballot)
        const int p = p0 + lane;
        const int32_t id = p < len ? ids[(size_t)first + p] : -1;
        const bool valid = id >= 0 && id < n_items;   // -1 = unused slot; an id outside the catalogue is never counted
        if (valid) {
            const int g = group_of[id];
            if (item_weight) w += item_weight[id];
            if (g >= 0 && g < n_groups) {             // an item outside every group is in no column
                atomicAdd(&bins[wave][0][g], 1);
                if (hit && item_in_sorted(gt_idx + a, n_gt, id)) atomicAdd(&bins[wave][1][g], 1);
            }
        }
        n_valid += __popcll(__ballot(valid));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) w += __shfl_xor(w, o, kWave);
    __syncthreads();
    if (!live) return;
    if (lane < n_groups) {
        cnt[(size_t)u * n_groups + lane] = bins[wave][0][lane];
        if (hit) hit[(size_t)u * n_groups + lane] = bins[wave][1][lane];
    }
    if (wsum && lane == 0) {
        longlong2 out;
        out.x = w;
        out.y = n_valid;
        reinterpret_cast<longlong2 *>(wsum)[u] = out;
    }
}

}  // namespace macr

using namespace macr;

extern "C" int macr_list_shift(int U, int K_base, int K_here, int k, const int32_t *rank_base, const int32_t *rank_here,
                               const int32_t *gt_ptr, const int32_t *gt_idx, int n_items, int32_t *per_user, int32_t *entered,
                               int32_t *left, void *stream) {
    hipStream_t st = as_stream(stream);
    MACR_REQUIRE(U >= 1 && k >= 1, MACR_E_INVALID, "list_shift: U=%d k=%d", U, k);
    MACR_REQUIRE(k <= K_base && k <= K_here, MACR_E_INVALID, "list_shift: k=%d above a row stride (K_base=%d, K_here=%d)", k, K_base, K_here);
    MACR_REQUIRE(K_base <= MACR_MAX_TOPK && K_here <= MACR_MAX_TOPK, MACR_E_INVALID,
                 "list_shift: K_base=%d K_here=%d above MACR_MAX_TOPK=%d", K_base, K_here, MACR_MAX_TOPK);
    MACR_REQUIRE(n_items > 0, MACR_E_INVALID, "list_shift: n_items=%d", n_items);
    MACR_REQUIRE(rank_base && rank_here && gt_ptr && gt_idx && per_user && entered && left, MACR_E_INVALID, "list_shift: null pointer");
    MACR_REQUIRE((reinterpret_cast<uintptr_t>(per_user) & 15) == 0, MACR_E_INVALID, "list_shift: per_user is not 16-byte aligned");
    const unsigned blocks = (unsigned)(((long long)U + kShiftQueries - 1) / kShiftQueries);
    k_list_shift<<<blocks, kShiftQueries * kWave, 0, st>>>(U, K_base, K_here, k, n_items, rank_base, rank_here, gt_ptr, gt_idx,
                                                           per_user, entered, left);
    MACR_CHECK_LAUNCH("list_shift", st);
    return MACR_OK;
}

extern "C" int macr_group_hist(int U, const int32_t *row_ptr, const int32_t *ids, int stride, int k, const int32_t *gt_ptr,
                               const int32_t *gt_idx, int n_items, const int32_t *group_of, int n_groups, const int32_t *item_weight,
                               int32_t *cnt, int32_t *hit, long long *wsum, void *stream) {
    hipStream_t st = as_stream(stream);
    MACR_REQUIRE(U >= 1, MACR_E_INVALID, "group_hist: U=%d", U);
    MACR_REQUIRE(n_items > 0, MACR_E_INVALID, "group_hist: n_items=%d", n_items);
    MACR_REQUIRE(n_groups >= 1 && n_groups <= kHistGroups, MACR_E_INVALID, "group_hist: n_groups=%d outside [1,%d]", n_groups, kHistGroups);
    MACR_REQUIRE(ids, MACR_E_INVALID, "group_hist: ids is null");
    MACR_REQUIRE(group_of, MACR_E_INVALID, "group_hist: group_of is null");
    MACR_REQUIRE(cnt, MACR_E_INVALID, "group_hist: cnt is null");
    if (row_ptr) {
        MACR_REQUIRE(stride == 0 && k == 0, MACR_E_INVALID, "group_hist: row_ptr given (CSR form) with stride=%d k=%d, both must be 0", stride, k);
    } else {
        MACR_REQUIRE(k >= 1 && k <= stride, MACR_E_INVALID, "group_hist: k=%d outside [1, stride=%d] (ranking form)", k, stride);
    }
    MACR_REQUIRE((hit != nullptr) == (gt_ptr != nullptr) && (hit != nullptr) == (gt_idx != nullptr), MACR_E_INVALID,
                 "group_hist: hit, gt_ptr and gt_idx are all given or all null (hit=%d gt_ptr=%d gt_idx=%d)", hit != nullptr,
                 gt_ptr != nullptr, gt_idx != nullptr);
    MACR_REQUIRE((reinterpret_cast<uintptr_t>(wsum) & 15) == 0, MACR_E_INVALID, "group_hist: wsum is not 16-byte aligned");
    const unsigned blocks = (unsigned)(((long long)U + kHistRows - 1) / kHistRows);
    k_group_hist<<<blocks, kHistRows * kWave, 0, st>>>(U, row_ptr, ids, stride, k, gt_ptr, gt_idx, n_items, group_of, n_groups,
                                                       item_weight, cnt, hit, wsum);
    MACR_CHECK_LAUNCH("group_hist", st);
    return MACR_OK;
}

extern "C" size_t macr_item_counts_workspace_bytes(int U, int K, int n_items) {
    if (U <= 0 || K < 1 || n_items <= 0) return 0;
    return (size_t)kItemReplicas * (size_t)n_items * sizeof(unsigned long long);
}

extern "C" int macr_item_counts(int U, int K, int k, const int32_t *rankings, const int32_t *gt_ptr, const int32_t *gt_idx,
                                int n_items, const int32_t *group_of, int n_groups, int32_t *rec_cnt, int32_t *hit_cnt,
                                long long *group_out, void *workspace, size_t workspace_bytes, void *stream) {
    hipStream_t st = as_stream(stream);
    MACR_REQUIRE(U > 0 && K >= 1, MACR_E_INVALID, "item_counts: U=%d K=%d", U, K);
    MACR_REQUIRE(k >= 1 && k <= K, MACR_E_INVALID, "item_counts: k=%d outside [1, K=%d]", k, K);
    MACR_REQUIRE(n_items > 0, MACR_E_INVALID, "item_counts: n_items=%d", n_items);
    MACR_REQUIRE(rankings && gt_ptr && gt_idx && rec_cnt && hit_cnt, MACR_E_INVALID, "item_counts: null pointer");
    MACR_REQUIRE(!group_of || (n_groups >= 1 && n_groups <= 64), MACR_E_INVALID,
                 "item_counts: group_of given with n_groups=%d outside [1,64]", n_groups);
    MACR_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, MACR_E_INVALID,
                 "item_counts: workspace is null or not 8-byte aligned (macr_item_counts_workspace_bytes)");
    MACR_REQUIRE(workspace_bytes >= macr_item_counts_workspace_bytes(U, K, n_items), MACR_E_WORKSPACE,
                 "item_counts: workspace %zu < %zu bytes", workspace_bytes, macr_item_counts_workspace_bytes(U, K, n_items));
    const bool groups = group_of && group_out;
    unsigned long long *packed = static_cast<unsigned long long *>(workspace);
    const size_t n_words = (size_t)kItemReplicas * n_items;
    const size_t zb = (n_words + 256 * 8 - 1) / (256 * 8);
    k_item_zero<<<(unsigned)(zb < 2048 ? zb : 2048), 256, 0, st>>>(packed, n_words, groups ? group_out : nullptr, groups ? 2 * n_groups : 0);
    MACR_CHECK_LAUNCH("item_zero", st);
    const long long n_entries = (long long)U * k;
    const long long tiles = (n_entries + kItemThreads - 1) / kItemThreads;
    k_item_counts<<<(unsigned)(tiles < kItemMaxBlocks ? tiles : kItemMaxBlocks), kItemThreads, 0, st>>>(
        n_entries, K, k, n_items, rankings, gt_ptr, gt_idx, packed);
    MACR_CHECK_LAUNCH("item_counts", st);
    const int fb = (n_items + 255) / 256 < 1024 ? (n_items + 255) / 256 : 1024;
    k_item_finish<<<fb, 256, 0, st>>>(n_items, packed, groups ? group_of : nullptr, n_groups, rec_cnt, hit_cnt,
                                      groups ? reinterpret_cast<unsigned long long *>(group_out) : nullptr);
    MACR_CHECK_LAUNCH("item_finish", st);
    return MACR_OK;
}

extern "C" size_t macr_item_exposure_workspace_bytes(int U, int K, int n_items) {
    if (U <= 0 || K < 1 || n_items <= 0) return 0;
    return (size_t)kExpReplicas * (size_t)n_items * 2 * sizeof(unsigned long long);
}

extern "C" int macr_item_exposure(int U, int K, int k, const int32_t *rankings, const int32_t *gt_ptr, const int32_t *gt_idx,
                                  const uint32_t *pos_weight, int n_items, const int32_t *group_of, int n_groups,
                                  long long *exp_w, long long *hit_w, long long *group_out, void *workspace, size_t workspace_bytes,
                                  void *stream) {
    hipStream_t st = as_stream(stream);
    MACR_REQUIRE(U > 0 && K >= 1, MACR_E_INVALID, "item_exposure: U=%d K=%d", U, K);
    MACR_REQUIRE(k >= 1 && k <= K, MACR_E_INVALID, "item_exposure: k=%d outside [1, K=%d]", k, K);
    MACR_REQUIRE(n_items > 0, MACR_E_INVALID, "item_exposure: n_items=%d", n_items);
    MACR_REQUIRE(rankings && gt_ptr && gt_idx && pos_weight && exp_w && hit_w, MACR_E_INVALID, "item_exposure: null pointer");
    MACR_REQUIRE(!group_of || (n_groups >= 1 && n_groups <= 64), MACR_E_INVALID,
                 "item_exposure: group_of given with n_groups=%d outside [1,64]", n_groups);
    MACR_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, MACR_E_INVALID,
                 "item_exposure: workspace is null or not 16-byte aligned (macr_item_exposure_workspace_bytes)");
    MACR_REQUIRE(workspace_bytes >= macr_item_exposure_workspace_bytes(U, K, n_items), MACR_E_WORKSPACE,
                 "item_exposure: workspace %zu < %zu bytes", workspace_bytes, macr_item_exposure_workspace_bytes(U, K, n_items));
    const bool groups = group_of && group_out;
    unsigned long long *acc = static_cast<unsigned long long *>(workspace);
    const size_t n_words = (size_t)kExpReplicas * n_items * 2;
    const size_t zb = (n_words + 256 * 8 - 1) / (256 * 8);
    k_item_zero<<<(unsigned)(zb < 2048 ? zb : 2048), 256, 0, st>>>(acc, n_words, groups ? group_out : nullptr, groups ? 2 * n_groups : 0);
    MACR_CHECK_LAUNCH("exposure_zero", st);
    const long long n_entries = (long long)U * k;
    const long long tiles = (n_entries + kExpThreads - 1) / kExpThreads;
    const long long cap = tiles < kExpMaxBlocks ? tiles : kExpMaxBlocks;
    const long long tiles_per_block = (tiles + cap - 1) / cap;
    const long long blocks = (tiles + tiles_per_block - 1) / tiles_per_block;       // <= cap; every block has a tile
    k_item_exposure<<<(unsigned)blocks, kExpThreads, 0, st>>>(n_entries, tiles_per_block, K, k, n_items, rankings, gt_ptr, gt_idx,
                                                              pos_weight, acc);
    MACR_CHECK_LAUNCH("item_exposure", st);
    const int fb = (n_items + 255) / 256 < 1024 ? (n_items + 255) / 256 : 1024;
    k_exposure_finish<<<fb, 256, 0, st>>>(n_items, reinterpret_cast<const ulonglong2 *>(acc), groups ? group_of : nullptr, n_groups,
                                          reinterpret_cast<unsigned long long *>(exp_w), reinterpret_cast<unsigned long long *>(hit_w),
                                          groups ? reinterpret_cast<unsigned long long *>(group_out) : nullptr);
    MACR_CHECK_LAUNCH("exposure_finish", st);
    return MACR_OK;
}
