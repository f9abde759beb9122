// split_unit.hip -- the source of every split-KV unit of libflash_attention.so: compiled once per row of SPLIT_FORMS (split_forms.hip.h)
// with -DFA_SPLIT_UNIT=<the row's name>, it holds that form's split_kv_kernel at D = 64 / 128 and its launcher, so that the forms compile
// in parallel, each under its own flags: the RT > 1 forms (extend_*, shared_*) with the MFMAs in VGPR form, which the Makefile announces
// with -DFA_SPLIT_MFMA_VGPR.  Not a unit by itself.
#include "split_forms.hip.h"

namespace fa {

constexpr SplitUnit UNIT = SplitUnit::FA_SPLIT_UNIT;
constexpr SplitKind KIND = SPLIT_FORMS[(int)UNIT];
#ifdef FA_SPLIT_MFMA_VGPR
static_assert(KIND.extend, "a decode unit (RT = 1) is built without the VGPR-form flag");
#else
static_assert(!KIND.extend, "a chunked-prefill unit (RT > 1) must be built with the VGPR-form flag: 4 ... 17 % at d = 128");
#endif

// EXTEND: chunked prefill, ExtendCfg::RT 16-row tiles per wave (decode: one); the LDS size is that of the cache's element size
template <SplitKind K>
static Kernel split_unit_kernel(int d) {
    constexpr int ES = K.kv8 ? 1 : 2;
    return d == 128 ? kernel_of<split_kv_kernel<128, K.extend ? ExtendCfg<128>::RT : 1, K.paged, K.kv8, K.window, K.varlen, K.sink, K.tree, K.shared>>(DecodeCfg<128, ES>::LDS_BYTES)
                    : kernel_of<split_kv_kernel<64, K.extend ? ExtendCfg<64>::RT : 1, K.paged, K.kv8, K.window, K.varlen, K.sink, K.tree, K.shared>>(DecodeCfg<64, ES>::LDS_BYTES);
}

// The pointers this form's kernel dereferences unconditionally (a TREE form takes sinks = NULL as -inf).  decode_run refuses such a call
// before it gets here; this makes a wrong selection a return code, not a fault
template <>
int split_unit_launch<UNIT>(int d, unsigned grid, hipStream_t st, const SplitArgs& a) {
    constexpr SplitKind K = KIND;
    if ((K.varlen && !a.cu_q) || (K.sink && !K.tree && !a.sinks) || (K.tree && !a.tree_mask)) return FA_ERR_NULL_POINTER;
    static_assert(DecodeCfg<128>::THREADS == 256);
    const Kernel k = split_unit_kernel<K>(d);
    return (int)launch(k, grid, 256, k.lds_bytes, st, split_params<typename SplitParamsOf<K.varlen, K.sink, K.tree, K.shared>::type>(a));
}

}  // namespace fa
