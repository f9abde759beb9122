// inst_mla_index.hip -- the kernels of flash_attention_mla_index_topk / _paged (mla_index.hip.h): the index-logits
// kernel in its two cache forms and the radix-select top-k, launched one after the other on the call's stream.  Built without packed
// fp32 arithmetic (the Makefile's flag).
#include "mla_index.hip.h"

namespace fa {

int mla_index_launch(bool paged, unsigned grid, unsigned rows, hipStream_t st, const MlaIndexParams& p) {
    // (what the kernels dereference unconditionally)
    if (!p.Q || !p.W || !p.K || !p.k_scale || !p.logits || !p.indices || (paged && !p.block_table)) return FA_ERR_NULL_POINTER;
    const Kernel k = paged ? kernel_of<mla_index_logits_kernel<true>>(0) : kernel_of<mla_index_logits_kernel<false>>(0);
    const int rc = (int)launch(k, grid, MlaIndexCfg::THREADS, 0, st, p);
    if (rc != FA_OK) return rc;
    return (int)launch(kernel_of<mla_index_topk_kernel<MlaIndexCfg::SEL_THREADS>>(0), rows, MlaIndexCfg::SEL_THREADS, 0, st, p);
}

}  // namespace fa
