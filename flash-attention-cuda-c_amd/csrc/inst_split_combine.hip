// inst_split_combine.hip -- the combine kernels of the split-KV calls under more than one split (decode_bf16.hip.h: decode_combine_kernel),
// the four (VARLEN, SINK) forms at D = 64 / 128, behind one launcher (one translation unit of libflash_attention.so: see launchers.hip.h
// and split_forms.hip.h).  VARLEN: every ragged call, which skips the rows no sequence owns; SINK: every flash_attention_sink_* call,
// decode's and chunked prefill's; all four cache forms take the same combine.  No MFMA here: built without the VGPR-form flag.
#include "split_forms.hip.h"

namespace fa {

template <bool VARLEN, bool SINK>
static int combine_launch_of(int d, unsigned rows, hipStream_t st, const SplitArgs& a) {
    if ((VARLEN && !a.cu_q) || (SINK && !a.sinks)) return FA_ERR_NULL_POINTER;   // (what this form's kernel dereferences unconditionally)
    const Kernel k = d == 128 ? kernel_of<decode_combine_kernel<128, VARLEN, SINK>>(0) : kernel_of<decode_combine_kernel<64, VARLEN, SINK>>(0);
    return (int)launch(k, rows, 256, 0, st, split_params<typename SplitParamsOf<VARLEN, SINK>::type>(a));
}

int combine_launch(bool varlen, bool sink, int d, unsigned rows, hipStream_t st, const SplitArgs& a) {
    return varlen ? (sink ? combine_launch_of<true, true> : combine_launch_of<true, false>)(d, rows, st, a)
                  : (sink ? combine_launch_of<false, true> : combine_launch_of<false, false>)(d, rows, st, a);
}

}  // namespace fa
