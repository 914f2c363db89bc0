/* Test-only entry points of the MI355X build: NOT part of the product library.
 *
 * libmacr_hip.so (include/macr_hip.h) exports none of these; they exist in macr_amd/csrc/libmacr_hip_test.so, the same
 * sources compiled with -DMACR_TEST_ENTRY_POINTS, which only tests/ load (macr_amd/_lib.py::test_lib).  They make internals
 * observable that no product call returns:
 *   - the raw products and scores of the bf16 / fp16 candidate filters with the error margin the filter grants them (the
 *     reference has no counterpart: it scores in fp32, macr_mf/model.py:199);
 *   - the staged gradient path of the training steps: the radix sort of the row references (refsort.hpp) and the four row
 *     reductions behind it, on caller-chosen keys and staging rows;
 *   - where the MF step's workspace holds the outputs of pair_fwd. */
#ifndef MACR_HIP_TEST_H
#define MACR_HIP_TEST_H
#include "macr_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* TEST-ONLY: the invariant the bf16 candidate filter rests on, made observable.  Writes, for U query rows and N item
 * rows (dev, fp32 [U][d] / [N][d]), the RAW product the bf16 kernels compute -- two-term bf16 splits, hi*hi + hi*lo +
 * lo*hi on v_mfma_f32_32x32x16_bf16 in the listing pass's instruction order -- to prod (dev) fp32[U][N], and to margin
 * (dev) fp32[U] the error margin the filter grants each query at this c (what it subtracts from her threshold).
 * tests/ assert |prod - fp32 fmaf chain| <= margin element-wise on adversarial operands for every d; no product code
 * calls this.  (The reference scores in fp32: macr_mf/model.py:199.) */
size_t macr_test_bf16_products_workspace_bytes(int d, int U, int N);
int macr_test_bf16_products(int d, int U, int N, const float *users, const float *items, float c,
                            float *prod, float *margin, void *workspace, size_t workspace_bytes, void *stream);

/* TEST-ONLY: the same for the listing pass macr_score_topk runs (k_score_stream_c: the epilogue in the operand copies --
 * item rows scaled by sig_i, the bias -c*sig_i as a three-term bf16 slab in the last MFMA, query rows scaled for
 * DIRECT_MINUS_BOTH).  Writes the SCORE that pass would list for every (query, item) pair of the given kind, scores (dev)
 * fp32[U][N], and the margin per query; tests/ assert |scores - fp32 score| <= margin element-wise.  sig_u / sig_i (dev)
 * fp32[U] / [N] as the kind needs them. */
size_t macr_test_bf16_scores_workspace_bytes(int d, int U, int N);
int macr_test_bf16_scores(int score_kind, int d, int U, int N, const float *users, const float *items,
                          const float *sig_u, const float *sig_i, float c, float *scores, float *margin,
                          void *workspace, size_t workspace_bytes, void *stream);

/* TEST-ONLY: the same for the fp16 filter (MACR_EVAL_FILTER_F16; k_score_stream_h: one fp16 number per operand, the bias
 * -c*sig_i (x sig_u for DIRECT_MINUS_BOTH) as six cross terms of two three-term fp16 splits in the slab).  Workspace:
 * macr_test_bf16_scores_workspace_bytes.  A query whose row leaves fp16's range gets margin = +inf. */
int macr_test_f16_scores(int score_kind, int d, int U, int N, const float *users, const float *items,
                         const float *sig_u, const float *sig_i, float c, float *scores, float *margin,
                         void *workspace, size_t workspace_bytes, void *stream);

/* TEST-ONLY: launch_radix_sort (refsort.hpp) on n caller-given (key, value) pairs, keys <= max_key (all dev, uint32[n]): the tile
 * sort_tile_for(n) picks (MACR_SORT_TILE in the environment included), a ghist of sort_hist_words(n) words, one pass per 8 bits of
 * max_key; the sorted pairs are copied out of whichever of the two buffers the sort ended in. */
size_t macr_test_radix_sort_workspace_bytes(int n);
int macr_test_radix_sort(int n, const uint32_t *keys, const uint32_t *vals, uint32_t max_key, uint32_t *keys_out,
                         uint32_t *vals_out, void *workspace, size_t workspace_bytes, void *stream);
/* TEST-ONLY, host only: the workspace rule of the sort -- words of tile counts + digit totals a sort of UP TO n pairs may need,
 * and the tile (keys per workgroup) a sort of exactly n pairs takes. */
size_t macr_test_sort_hist_words(int n);
int macr_test_sort_tile_for(int n);

/* TEST-ONLY: the staged gradient path behind the pair kernels, on a caller-filled staging buffer.  u, i, j (dev) int32[B]: the
 * batch; stage (dev) fp32[3B][d]: row role * B + t = the gradient of position t's user / positive / negative row.  The rows this
 * "rank" owns are (u_lo, u_stride, n_users_loc, i_lo, i_stride, n_items_loc), as in macr_shard_apply.
 *   (0, 1, n_users, 0, 1, n_items) and mode != INV: the single-GPU steps' sequence -- k_refs_init, the sort, then the reduction
 *     launch_ref_sort_reduce runs for that mode (every index must lie inside its table);
 *   anything else, and every INV call: the row-sharded step's sequence -- k_shard_keys, the sort, then the reduction block of
 *     shard_apply (foreign references sort behind the owned ones and are ignored).
 * mode: MACR_TEST_REDUCE  k_seg_reduce (atomics for runs cut into chunks: gU/gI rows must be ZERO on entry, as between steps);
 *       MACR_TEST_INDEX   k_seg_scan + k_seg_sum, stopping before the indexed Adam pass: tU/tI hold (len << 26) | position for rows
 *                         of <= 16 references, 1 for longer ones, whose sums are ADDED to gU/gI (zero on entry);
 *       MACR_TEST_DET     k_seg_reduce<., true> + k_seg_fold;   MACR_TEST_INV   k_seg_reduce_inv + k_seg_fold_inv (plain stores).
 * gU/gI (dev) fp32[n_*_loc][d], tU/tI (dev) int32[n_*_loc] (NULL for a table without rows here).  sk_out, sv_out (dev)
 * uint32[3B]: the sorted keys and values. */
#define MACR_TEST_REDUCE 0
#define MACR_TEST_INDEX 1
#define MACR_TEST_DET 2
#define MACR_TEST_INV 3
size_t macr_test_ref_reduce_workspace_bytes(int B, int d);
int macr_test_ref_reduce(int mode, int B, int d, int n_users_loc, int n_items_loc, int u_lo, int u_stride, int i_lo,
                         int i_stride, const int32_t *u, const int32_t *i, const int32_t *j, const float *stage,
                         float *gU, float *gI, int32_t *tU, int32_t *tI, uint32_t *sk_out, uint32_t *sv_out,
                         void *workspace, size_t workspace_bytes, void *stream);

/* TEST-ONLY, host only: where the MF training step keeps pair_fwd's outputs in its workspace.  fwd_offset_bytes: the distance
 * from the workspace's first byte to `fwd`, seven arrays of *Bp floats (p, n, a, b, sig_si, sig_sj, and sig_su or the BPR
 * cell's factor, whose sign bit is the column flag of the BCE kinds); entry t < B of array k is float k * *Bp + t.
 * deterministic != 0: the layout of a step that carries MACR_STEP_DETERMINISTIC. */
int macr_test_pair_ws_layout(int B, int d, int deterministic, size_t *fwd_offset_bytes, int *Bp);

#ifdef __cplusplus
}
#endif
#endif
