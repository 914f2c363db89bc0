// Stand-alone check of macr_amd/csrc/ref_sampler_core.hpp, meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ref_sampler_check.cpp -o check
//   ./check cases.bin
// Reads the cases tests/test_reference_sampler_cpu.py writes (every array in a heap block of exactly its size, so a read or
// write past an end is caught), draws them with the core and exits non-zero on the first difference from what the Python
// form of the samplers produced: batches, both generator states, or -- for a case that must be refused -- the status
// code and untouched states.
//
// File: int32 words, little endian.  "RSC1", n_cases, then per case
//   kind n_batches B n_users n_pop n_items pos_nnz excl_nnz py_pos np_pos expect_rc chunk
//   pop[n_pop] pos_ptr[n_users+1] pos_idx[pos_nnz] excl_ptr[n_users+1] excl_idx[excl_nnz] py_key[624] np_key[624]
//   and, when expect_rc == 0: out[n_batches*3*B] py_key'[624] py_pos' np_key'[624] np_pos'
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../macr_amd/csrc/ref_sampler_core.hpp"

namespace rs = macr::refstream;

static FILE *g_f;

static int32_t *read_words(size_t n) {
    int32_t *p = static_cast<int32_t *>(malloc(n ? n * sizeof(int32_t) : 1));
    if (!p || fread(p, sizeof(int32_t), n, g_f) != n) {
        fprintf(stderr, "ref_sampler_check: short read (%zu words)\n", n);
        exit(2);
    }
    return p;
}

int main(int argc, char **argv) {
    if (argc != 2 || !(g_f = fopen(argv[1], "rb"))) {
        fprintf(stderr, "usage: ref_sampler_check cases.bin\n");
        return 2;
    }
    int32_t *head = read_words(2);
    if (memcmp(head, "RSC1", 4) != 0) { fprintf(stderr, "ref_sampler_check: not a case file\n"); return 2; }
    const int n_cases = head[1];
    free(head);
    for (int c = 0; c < n_cases; ++c) {
        int32_t *h = read_words(12);
        const int kind = h[0], n_batches = h[1], B = h[2], n_users = h[3], n_pop = h[4], n_items = h[5], pos_nnz = h[6],
                  excl_nnz = h[7], py_pos0 = h[8], np_pos0 = h[9], expect_rc = h[10], chunk = h[11];
        free(h);
        int32_t *pop = read_words(n_pop), *pos_ptr = read_words(n_users + 1), *pos_idx = read_words(pos_nnz);
        int32_t *excl_ptr = read_words(n_users + 1), *excl_idx = read_words(excl_nnz);
        uint32_t *py_key = reinterpret_cast<uint32_t *>(read_words(rs::kStateWords));
        uint32_t *np_key = reinterpret_cast<uint32_t *>(read_words(rs::kStateWords));
        std::vector<uint32_t> py0(py_key, py_key + rs::kStateWords), np0(np_key, np_key + rs::kStateWords);
        int py_pos = py_pos0, np_pos = np_pos0;
        const size_t n_out = (size_t)(n_batches > 0 ? n_batches : 0) * 3 * (size_t)(B > 0 ? B : 0);
        int32_t *out = static_cast<int32_t *>(malloc(n_out ? n_out * sizeof(int32_t) : 1));
        const size_t ws_bytes = rs::workspace_bytes(n_pop);
        void *ws = malloc(ws_bytes ? ws_bytes : 1);
        char err[256] = "";
        int rc = rs::kOk;
        for (int lo = 0; lo == 0 || lo < n_batches; lo += chunk) {
            const int m = n_batches - lo < chunk ? n_batches - lo : chunk;
            rs::Args a = {kind, m, B, n_users, pop, n_pop, pos_ptr, pos_idx, excl_ptr, excl_idx, n_items, py_key, &py_pos,
                          np_key, &np_pos, out + (size_t)lo * 3 * (B > 0 ? B : 0), ws, ws_bytes};
            rc = rs::sample_batches(a, err, sizeof(err));
            if (rc != rs::kOk) break;
        }
        if (rc != expect_rc) {
            fprintf(stderr, "case %d: status %d (%s), expected %d\n", c, rc, err, expect_rc);
            return 1;
        }
        if (expect_rc == rs::kOk) {
            int32_t *want = read_words(n_out);
            uint32_t *py1 = reinterpret_cast<uint32_t *>(read_words(rs::kStateWords + 1));
            uint32_t *np1 = reinterpret_cast<uint32_t *>(read_words(rs::kStateWords + 1));
            for (size_t k = 0; k < n_out; ++k)
                if (out[k] != want[k]) {
                    fprintf(stderr, "case %d: batch %zu row %zu column %zu: %d, expected %d\n", c, k / (3 * (size_t)B),
                            k / B % 3, k % B, out[k], want[k]);
                    return 1;
                }
            if (memcmp(py_key, py1, sizeof(uint32_t) * rs::kStateWords) || py_pos != (int)py1[rs::kStateWords]) {
                fprintf(stderr, "case %d: the Python generator's state differs (position %d, expected %d)\n", c, py_pos,
                        (int)py1[rs::kStateWords]);
                return 1;
            }
            if (memcmp(np_key, np1, sizeof(uint32_t) * rs::kStateWords) || np_pos != (int)np1[rs::kStateWords]) {
                fprintf(stderr, "case %d: the NumPy generator's state differs (position %d, expected %d)\n", c, np_pos,
                        (int)np1[rs::kStateWords]);
                return 1;
            }
            free(want); free(py1); free(np1);
        } else if (memcmp(py_key, py0.data(), sizeof(uint32_t) * rs::kStateWords) || py_pos != py_pos0 ||
                   memcmp(np_key, np0.data(), sizeof(uint32_t) * rs::kStateWords) || np_pos != np_pos0) {
            fprintf(stderr, "case %d: refused with %d but a generator state changed\n", c, rc);
            return 1;
        }
        free(pop); free(pos_ptr); free(pos_idx); free(excl_ptr); free(excl_idx); free(py_key); free(np_key); free(out); free(ws);
    }
    if (fgetc(g_f) != EOF) { fprintf(stderr, "ref_sampler_check: trailing bytes\n"); return 2; }
    fclose(g_f);
    printf("ref_sampler_check: %d cases ok\n", n_cases);
    return 0;
}
