// C ABI of the reference-stream host sampler (ref_sampler_core.hpp): `--sampler reference` of both CLIs.
// Host code only -- MT19937 consumed through variable-length rejection loops is one sequential chain; batches that need
// not be the reference's stream come from the device sampler (sample_kernels.hip).
#include "common.hpp"
#include "ref_sampler_core.hpp"

static_assert(MACR_REFSTREAM_MF == macr::refstream::kStreamMF && MACR_REFSTREAM_LGCN == macr::refstream::kStreamLGCN, "stream kinds");
static_assert(MACR_OK == macr::refstream::kOk && MACR_E_INVALID == macr::refstream::kInvalid &&
              MACR_E_WORKSPACE == macr::refstream::kWorkspace, "status codes");

extern "C" size_t macr_ref_sample_workspace_bytes(int n_pop) { return macr::refstream::workspace_bytes(n_pop); }

extern "C" int macr_ref_sample_batches(int kind, int n_batches, int B, int n_users, const int32_t *pop, int n_pop,
                                       const int32_t *pos_ptr, const int32_t *pos_idx, const int32_t *excl_ptr,
                                       const int32_t *excl_idx, int n_items, uint32_t *py_key, int *py_pos, uint32_t *np_key,
                                       int *np_pos, int32_t *out, void *workspace, size_t workspace_bytes) {
    macr::refstream::Args a = {kind, n_batches, B, n_users, pop, n_pop, pos_ptr, pos_idx, excl_ptr, excl_idx, n_items,
                               py_key, py_pos, np_key, np_pos, out, workspace, workspace_bytes};
    char err[256];
    const int rc = macr::refstream::sample_batches(a, err, sizeof(err));
    if (rc != MACR_OK) macr::set_error("%s", err);
    return rc;
}
