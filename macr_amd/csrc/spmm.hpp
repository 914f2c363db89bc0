// The interface of the LightGCN propagation (spmm_kernels.hip) as its callers see it: the plan's header, the row-sparse
// modes, the fused optimizer of the last backward layer and the launch sequence itself.
#pragma once
#include "common.hpp"

namespace macr {

struct PlanHeader {               // all int32, followed by the arrays below
    int32_t magic, n_items, n_split, n_slots, N, chunk, n_groups, reserved;
    // RECORDS of the short rows (round 5, spmm_records in spmm_kernels.hip): item[0 .. n_single) are the pieces and the rows of more than
    // kRecEntries neighbours -- one wave each in a dense layer -- and every shorter row also sits in a record, several to a
    // wave: n_rec[c] records of class c (8, 4, 2, 1 rows of at most 4, 8, 16, 32 neighbours) from int32 offset rec_off on
    int32_t n_single, rec_off, n_rec[4], pad[2];
};
constexpr int32_t kPlanMagic = 0x4d414356;   // "MACV" (layout 5)
// layout after the header (64 bytes, so the descriptors are 16-byte aligned):
//   item[n_items] = {row, beg, end, slot}   the n_slots pieces of the split rows first (slot >= 0, in slot order), then
//                                           the other rows (slot = -1), longest first
//   slot_group[n_slots]                     the group a piece belongs to (kGroup consecutive pieces of one row)
//   group_slot0[n_groups+1]                 group g owns slots group_slot0[g] .. group_slot0[g+1]-1
//   group_split[n_groups]                   the hub row (index k) of a group
//   split_group0[n_split+1]                 hub row k owns groups split_group0[k] .. split_group0[k+1]-1
//   split_row[n_split]                      its row

// SPARSE modes (a LightGCN training step only needs the propagated rows of its batch, and its gradient enters the
// backward propagation with <= 3B non-zero rows):
//   kSparseOut  only the rows the batch refers to (and every hub row) are computed (the LAST forward layer: nothing
//               else is read afterwards).  One wave per batch reference -- a row referred to twice is computed twice,
//               to the same values; the hub rows, which hold the repeats of a popularity-skewed batch, are left to
//               their pieces.  (Building a duplicate-free row list first costs more than it saves: the atomics that
//               detect a row's first reference queue on the hot items' cache lines, ~24 ns each: 45 us per batch.)
//   kSparseIn   X and S_in are row-sparse: only rows with rows[.] != 0 are read (the FIRST backward layer)
constexpr int kDense = 0, kSparseOut = 1, kSparseIn = 2;

struct SparseCtx {                // device pointers
    int32_t *cnt;                 // [N] how often the current batch refers to a row (0: not a row of the batch).  The last
                                  // forward layer COUNTS (one wave per reference), the first backward layer reads the
                                  // counts as flags, the fused epilogue of the last backward layer consumes and clears them
    const int32_t *u, *i, *j;     // the batch: rows u[b], n_users + i[b], n_users + j[b]
    int B, n_users;
    int chunk;                    // rows longer than this are hub rows (cut into pieces by the plan); INT_MAX without a plan
    int count;                    // kSparseOut: 1 = count the references into cnt (a training step), 0 = leave it alone
};

// The optimizer, fused into the epilogue of the LAST backward layer (a LightGCN training step; LightGCN.py:186/:201 are
// dense Adam over the ego table T): the wave that finishes row r holds its gradient (S_in[r] + A X[r]) * scale in
// registers and applies it on the spot -- together with the ego-row regulariser coef * cnt[r] * T[r] (LightGCN.py:525-528:
// one term per reference) and the row's share cnt[r] * |T[r]|^2 of emb_loss -- instead of writing G for a separate pass
// over the table (125 MB of traffic and two more launches per step).  It also clears cnt[r] and the row dE[r] of the
// gradient buffer the pair kernels accumulate into: both are zero again when the next step starts.
struct AdamFuse {
    float *T, *m, *v;             // ego table and its Adam slots, updated in place (NULL: no fusion)
    const StepScalars *scal;      // lr_t of this step (written by pair_bwd)
    float b1, b2, eps, coef;      // coef = decay / batch_size
    float *dE;                    // gradient buffer of the pair kernels (rows of the batch are zeroed)
    double *emb_acc;              // [2048] partial sums of cnt * |T row|^2 (emb_loss), slot = row % 2048 (fp64 atomics: the order
                                  // of arrival shows in the last bits).  NULL: the epilogues leave it alone (the deterministic step)
    float *sb;                    // NULL, or (LightGCN --loss bce2) a scalar per row: the row's gradient also gets sb[r] * bw, and
    const float *bw;              // sb[r] is zeroed -- the item branch on the EGO rows, which does not pass through the propagation
};

// n_layers of E <- mean of the layers of A E0 (spmm_kernels.hip describes work, sp / sparse_mode and fuse at the definition)
int launch_propagate(int N, int d, int n_layers, const int32_t *rowptr, const int32_t *col, const float *val,
                     const void *plan_dev, const void *plan_host_header, const float *E0, float *E, float *work,
                     hipStream_t st, const SparseCtx *sp, int sparse_mode, const AdamFuse *fuse);

}  // namespace macr
