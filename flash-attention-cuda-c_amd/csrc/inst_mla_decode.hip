// inst_mla_decode.hip -- the kernels of flash_attention_mla_decode / _paged (mla_decode.hip.h): the MLA split kernel
// in its two cache forms, and decode_combine_kernel at D = 512 (TPR = 128, two slots), which no other unit instantiates.  Built with the
// MFMAs in VGPR form (the Makefile's flag): launch bounds (256, 1), and the accumulators are rescaled by the VALU at every tile.
#include "mla_decode.hip.h"

namespace fa {

int mla_decode_launch(bool paged, unsigned grid, hipStream_t st, const DecodeParams& p) {
    if (paged && !p.block_table) return FA_ERR_NULL_POINTER;   // (what the paged kernel dereferences unconditionally)
    const Kernel k = paged ? kernel_of<mla_decode_kernel<true>>(MlaCfg::LDS_BYTES) : kernel_of<mla_decode_kernel<false>>(MlaCfg::LDS_BYTES);
    return (int)launch(k, grid, MlaCfg::THREADS, MlaCfg::LDS_BYTES, st, p);
}

int mla_combine_launch(unsigned rows, hipStream_t st, const DecodeParams& p) {
    return (int)launch(kernel_of<decode_combine_kernel<MlaCfg::DL>>(0), rows, 256, 0, st, p);
}

}  // namespace fa
