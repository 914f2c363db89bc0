// The reference's host sampler stream, bit for bit, in plain C++ (no HIP header: tools/ref_sampler_check.cpp builds this
// file alone with g++ under the address and undefined-behaviour sanitizers).
//
// Replaces the Python loops of macr_mf/load_data.py:543-566 (Data.sample of the MF CLI) and
// macr_lightgcn/utility/load_data.py:174-212 (Data.sample), :214-254 (Data.sample_test): the batches AND the generator
// states they leave are those of CPython's `random` (random.py of 3.8 - 3.12: sample, choice, _randbelow_with_getrandbits)
// and NumPy's legacy RandomState.randint(low, high, size=1) (masked rejection on 32-bit words).  Both generators are
// MT19937; a "word" below is one tempered output, twisting in place when the position reaches 624.
//
//   randbelow(n)  on the Python generator: k = bit_length(n); r = word >> (32 - k); redraw while r >= n.  n = 1 still
//                 consumes words (k = 1: the top bit must come up 0).
//   randint(n)    on the NumPy generator: rng = n - 1; rng == 0 returns 0 WITHOUT a word; else mask = rng smeared to
//                 all-ones below its top bit; v = word & mask; redraw while v > rng.
//   users         B <= n_users: random.sample(population, B) -- setsize = 21 (+ the smallest power of 4 >= 3B when
//                 B > 5); n_pop <= setsize: the pool form on a fresh copy of the population; else the set form.
//                 B > n_users: B times population[randbelow(n_pop)].
//   items         per user, in order: positive = list[draw(len)], negative = draw(n_items) redrawn while excluded.
//                 MF draws both with randbelow (an empty list gives item 0 and draws nothing); LightGCN with randint
//                 (an empty list is an error: the reference raises KeyError).
// All or nothing: the states are worked on in copies and stored back only when every batch has been drawn.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace macr {
namespace refstream {

constexpr int kStateWords = 624;
constexpr int kOk = 0, kInvalid = -1, kWorkspace = -3;      // = MACR_OK, MACR_E_INVALID, MACR_E_WORKSPACE
constexpr int kStreamMF = 0, kStreamLGCN = 1;               // = MACR_REFSTREAM_MF, MACR_REFSTREAM_LGCN

struct MT19937 {
    uint32_t key[kStateWords];
    int pos;

    void twist() {
        constexpr int N = kStateWords, M = 397;
        constexpr uint32_t A = 0x9908b0dfu, UP = 0x80000000u, LO = 0x7fffffffu;
        int k = 0;
        for (; k < N - M; ++k) {
            const uint32_t y = (key[k] & UP) | (key[k + 1] & LO);
            key[k] = key[k + M] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
        }
        for (; k < N - 1; ++k) {
            const uint32_t y = (key[k] & UP) | (key[k + 1] & LO);
            key[k] = key[k + (M - N)] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
        }
        const uint32_t y = (key[N - 1] & UP) | (key[0] & LO);
        key[N - 1] = key[M - 1] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
        pos = 0;
    }
    uint32_t word() {
        if (pos >= kStateWords) twist();
        uint32_t y = key[pos++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }
    // CPython random._randbelow_with_getrandbits(n), 1 <= n < 2^31
    uint32_t randbelow(uint32_t n) {
        const int shift = __builtin_clz(n);                 // 32 - bit_length(n)
        uint32_t r = word() >> shift;
        while (r >= n) r = word() >> shift;
        return r;
    }
    // NumPy legacy RandomState.randint(0, n, size=1)[0], 1 <= n < 2^31
    uint32_t randint(uint32_t n) {
        const uint32_t rng = n - 1u;
        if (rng == 0u) return 0u;
        uint32_t mask = rng;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        uint32_t v = word() & mask;
        while (v > rng) v = word() & mask;
        return v;
    }
};

struct Args {
    int kind;                        // kStreamMF | kStreamLGCN
    int n_batches, B;
    int n_users;                     // rows of both CSRs; B <= n_users selects random.sample, else random.choice
    const int32_t *pop; int n_pop;   // population, ids in [0, n_users)
    const int32_t *pos_ptr, *pos_idx;     // positives per user id, in LIST order (a draw is an index into the list)
    const int32_t *excl_ptr, *excl_idx;   // what a negative must avoid per user id: ascending, without duplicates
    int n_items;
    uint32_t *py_key; int *py_pos;   // random.getstate()[1][:624], [624]         in/out
    uint32_t *np_key; int *np_pos;   // np.random.get_state()[1], [2]              in/out
    int32_t *out;                    // [n_batches][3][B]: users | pos_items | neg_items
    void *workspace; size_t workspace_bytes;
};

inline size_t workspace_bytes(int n_pop) { return n_pop > 0 ? (size_t)n_pop * sizeof(int32_t) : 0; }

// random.sample's threshold between the pool form and the set form
inline int64_t sample_setsize(int B) {
    int64_t setsize = 21;
    if (B > 5) {
        int64_t p = 1;
        while (p < 3 * (int64_t)B) p *= 4;       // 4 ** ceil(log4(3B)): exact in integers, 3B is never a power of 4
        setsize += p;
    }
    return setsize;
}

inline bool excluded(const int32_t *list, int len, int32_t item) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < item) lo = mid + 1; else hi = mid;
    }
    return lo < len && list[lo] == item;
}

#define MACR_REF_FAIL(code, ...)                      \
    do {                                              \
        snprintf(err, err_len, __VA_ARGS__);          \
        return (code);                                \
    } while (0)

// -> kOk, or an error code with `err` naming the offending argument; on error neither the states nor (for the checks
// made before any draw: everything but LightGCN's empty list) `out` have been written.
inline int sample_batches(const Args &a, char *err, size_t err_len) {
    if (a.kind != kStreamMF && a.kind != kStreamLGCN) MACR_REF_FAIL(kInvalid, "ref_sample_batches: kind=%d", a.kind);
    if (a.B <= 0) MACR_REF_FAIL(kInvalid, "ref_sample_batches: B=%d", a.B);
    if (a.n_batches < 0) MACR_REF_FAIL(kInvalid, "ref_sample_batches: n_batches=%d", a.n_batches);
    if (a.n_users <= 0 || a.n_items <= 0 || a.n_pop <= 0)
        MACR_REF_FAIL(kInvalid, "ref_sample_batches: n_users=%d n_items=%d n_pop=%d", a.n_users, a.n_items, a.n_pop);
    if (!a.pop) MACR_REF_FAIL(kInvalid, "ref_sample_batches: null pointer pop");
    if (!a.pos_ptr || !a.pos_idx) MACR_REF_FAIL(kInvalid, "ref_sample_batches: null pointer pos_ptr / pos_idx");
    if (!a.excl_ptr || !a.excl_idx) MACR_REF_FAIL(kInvalid, "ref_sample_batches: null pointer excl_ptr / excl_idx");
    if (!a.py_key || !a.py_pos) MACR_REF_FAIL(kInvalid, "ref_sample_batches: null pointer py_key / py_pos");
    if (!a.np_key || !a.np_pos) MACR_REF_FAIL(kInvalid, "ref_sample_batches: null pointer np_key / np_pos");
    if (!a.out) MACR_REF_FAIL(kInvalid, "ref_sample_batches: null pointer out");
    if (*a.py_pos < 0 || *a.py_pos > kStateWords) MACR_REF_FAIL(kInvalid, "ref_sample_batches: py_pos=%d outside 0..624", *a.py_pos);
    if (*a.np_pos < 0 || *a.np_pos > kStateWords) MACR_REF_FAIL(kInvalid, "ref_sample_batches: np_pos=%d outside 0..624", *a.np_pos);
    const bool distinct = a.B <= a.n_users;
    if (distinct && a.B > a.n_pop)               // random.sample raises "Sample larger than population"
        MACR_REF_FAIL(kInvalid, "ref_sample_batches: B=%d > n_pop=%d with B <= n_users=%d", a.B, a.n_pop, a.n_users);
    if (!a.workspace || a.workspace_bytes < workspace_bytes(a.n_pop))
        MACR_REF_FAIL(kWorkspace, "ref_sample_batches: workspace_bytes=%zu, needs %zu", a.workspace ? a.workspace_bytes : (size_t)0,
                      workspace_bytes(a.n_pop));
    for (int k = 0; k < a.n_pop; ++k) {
        const int32_t u = a.pop[k];
        if (u < 0 || u >= a.n_users) MACR_REF_FAIL(kInvalid, "ref_sample_batches: pop[%d]=%d outside 0..n_users-1", k, u);
        if (a.pos_ptr[u] < 0 || a.pos_ptr[u + 1] < a.pos_ptr[u])
            MACR_REF_FAIL(kInvalid, "ref_sample_batches: pos_ptr not ascending at user %d", u);
        if (a.excl_ptr[u] < 0 || a.excl_ptr[u + 1] < a.excl_ptr[u])
            MACR_REF_FAIL(kInvalid, "ref_sample_batches: excl_ptr not ascending at user %d", u);
        // a list that covers the catalogue makes the reference's rejection loop spin for ever: refused before any draw
        // (ascending without duplicates: the entries inside [0, n_items) are the ones between two binary searches)
        const int32_t *xl = a.excl_idx + a.excl_ptr[u];
        const int xn = a.excl_ptr[u + 1] - a.excl_ptr[u];
        if (xn >= a.n_items) {
            int lo = 0, hi = xn;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (xl[mid] < 0) lo = mid + 1; else hi = mid; }
            const int first = lo;
            hi = xn;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (xl[mid] < a.n_items) lo = mid + 1; else hi = mid; }
            if (lo - first >= a.n_items)
                MACR_REF_FAIL(kInvalid, "ref_sample_batches: excl list of user %d covers all n_items=%d", u, a.n_items);
        }
    }

    MT19937 py, np;
    memcpy(py.key, a.py_key, sizeof(py.key)); py.pos = *a.py_pos;
    memcpy(np.key, a.np_key, sizeof(np.key)); np.pos = *a.np_pos;
    const bool pool_form = distinct && (int64_t)a.n_pop <= sample_setsize(a.B);
    int32_t *ws = static_cast<int32_t *>(a.workspace);       // pool form: the pool; set form: batch stamp per slot
    if (distinct && !pool_form) memset(ws, 0, (size_t)a.n_pop * sizeof(int32_t));
    const uint32_t n_pop = (uint32_t)a.n_pop, n_items = (uint32_t)a.n_items;
    const int B = a.B;
    int32_t stamp = 0;

    for (int b = 0; b < a.n_batches; ++b) {
        int32_t *users = a.out + (size_t)b * 3 * B, *pos = users + B, *neg = pos + B;
        if (pool_form) {
            memcpy(ws, a.pop, (size_t)n_pop * sizeof(int32_t));
            for (int i = 0; i < B; ++i) {
                const uint32_t j = py.randbelow(n_pop - (uint32_t)i);
                users[i] = ws[j];
                ws[j] = ws[n_pop - (uint32_t)i - 1u];
            }
        } else if (distinct) {
            if (++stamp == INT32_MAX) { memset(ws, 0, (size_t)n_pop * sizeof(int32_t)); stamp = 1; }
            for (int i = 0; i < B; ++i) {
                uint32_t j = py.randbelow(n_pop);
                while (ws[j] == stamp) j = py.randbelow(n_pop);
                ws[j] = stamp;
                users[i] = a.pop[j];
            }
        } else {
            for (int i = 0; i < B; ++i) users[i] = a.pop[py.randbelow(n_pop)];
        }
        for (int i = 0; i < B; ++i) {
            const int32_t u = users[i];
            const int32_t *pl = a.pos_idx + a.pos_ptr[u];
            const int pn = a.pos_ptr[u + 1] - a.pos_ptr[u];
            const int32_t *xl = a.excl_idx + a.excl_ptr[u];
            const int xn = a.excl_ptr[u + 1] - a.excl_ptr[u];
            if (a.kind == kStreamMF) {
                pos[i] = pn > 0 ? pl[py.randbelow((uint32_t)pn)] : 0;
                int32_t j = (int32_t)py.randbelow(n_items);
                while (excluded(xl, xn, j)) j = (int32_t)py.randbelow(n_items);
                neg[i] = j;
            } else {
                if (pn <= 0) MACR_REF_FAIL(kInvalid, "ref_sample_batches: pos list of user %d is empty (LightGCN stream)", u);
                pos[i] = pl[np.randint((uint32_t)pn)];
                int32_t j = (int32_t)np.randint(n_items);
                while (excluded(xl, xn, j)) j = (int32_t)np.randint(n_items);
                neg[i] = j;
            }
        }
    }
    memcpy(a.py_key, py.key, sizeof(py.key)); *a.py_pos = py.pos;
    memcpy(a.np_key, np.key, sizeof(np.key)); *a.np_pos = np.pos;
    return kOk;
}
#undef MACR_REF_FAIL

}  // namespace refstream
}  // namespace macr
