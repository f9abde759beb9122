# Build everything for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
PKG      := flash-attention-cuda-c_amd
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     := gfx950
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++20 -fPIC -fno-slp-vectorize
LIB      := $(PKG)/libflash_attention.so
# the library's translation units: the C ABI + one unit per group of kernel instantiations (they compile in parallel)
# The split-KV units are the rows of SPLIT_FORMS in csrc/split_forms.hip.h, which says what each one is and who launches it: one object per
# name, all from csrc/split_unit.hip (not an object itself) with -DFA_SPLIT_UNIT=<name>.  A name here without a row does not compile;
# a row without a name here does not link.
SPLIT_UNITS := decode_bf16 decode_fp8 decode_paged_bf16 decode_paged_fp8 \
               extend_bf16 extend_fp8 extend_paged_bf16 extend_paged_fp8 \
               extend_window_bf16 extend_window_fp8 extend_window_paged_bf16 extend_window_paged_fp8 \
               extend_varlen_bf16 extend_varlen_fp8 extend_varlen_paged_bf16 extend_varlen_paged_fp8 \
               extend_window_varlen_bf16 extend_window_varlen_fp8 extend_window_varlen_paged_bf16 extend_window_varlen_paged_fp8 \
               decode_sink_bf16 decode_sink_fp8 decode_sink_paged_bf16 decode_sink_paged_fp8 \
               extend_sink_bf16 extend_sink_fp8 extend_sink_paged_bf16 extend_sink_paged_fp8 \
               extend_sink_varlen_bf16 extend_sink_varlen_fp8 extend_sink_varlen_paged_bf16 extend_sink_varlen_paged_fp8 \
               decode_tree_bf16 decode_tree_fp8 decode_tree_paged_bf16 decode_tree_paged_fp8 \
               extend_tree_bf16 extend_tree_fp8 extend_tree_paged_bf16 extend_tree_paged_fp8 \
               shared_bf16 shared_fp8 shared_paged_bf16 shared_paged_fp8
SPLIT_SRC := $(PKG)/csrc/split_unit.hip
SPLIT_OBJ := $(SPLIT_UNITS:%=build/obj/inst_%.o)
KSRC     := $(filter-out $(SPLIT_SRC),$(wildcard $(PKG)/csrc/*.hip))
KOBJ     := $(patsubst $(PKG)/csrc/%.hip,build/obj/%.o,$(KSRC)) $(SPLIT_OBJ)
KHDR     := $(wildcard $(PKG)/csrc/*.h) $(PKG)/helpers.hpp include/flash_attention.h

# `all` = the product, its C++ harness and driver, the oracle, the microbenchmarks bench.py uses (about 1.5 min with -j4).
# `tune` = the kernel-variant A/B harness: ~70 kernel instantiations, 3 more minutes; not needed by tests or bench.
all: $(LIB) oracle $(PKG)/fa_main tests/fa_test tests/unit_kernels tests/micro/simd_mix tests/micro/valu_rates

tune: tests/fa_tune

lib: $(LIB)

# The d = 128 pair kernels run one 4-wave workgroup per CU (launch bounds 256, 1): hipcc would then place the MFMA accumulators in the
# accumulation registers and pay a v_accvgpr_read for every score the softmax touches (-6 ... -11 %, profiles/r04_tune_q_*); with the
# MFMAs in VGPR form the second half of the register file only takes what would otherwise spill
MFMA_VGPR := -mllvm -amdgpu-mfma-vgpr-form=1
build/obj/inst_bf16_pair_d128.o: HIPFLAGS += $(MFMA_VGPR)
# the backward kernel (bwd_bf16.hip.h) likewise: dV^T / dK^T of 64 keys take 256 registers; in the default form hipcc spills ~280 to scratch at D = 128
build/obj/inst_bwd_bf16.o: HIPFLAGS += $(MFMA_VGPR)
# the MLA decode kernel (mla_decode.hip.h) likewise: 128 accumulator registers of O^T that the VALU rescales at every key tile
build/obj/inst_mla_decode.o: HIPFLAGS += $(MFMA_VGPR)
tests/fa_tune tests/fa_tune_c128 tests/fa_tune_seam tests/fa_tune_tail: HIPFLAGS += $(MFMA_VGPR)
# the chunked-prefill units of the split-KV kernel (the extend_* names of SPLIT_UNITS, and the shared_* ones, which are built at the same RT; decode_bf16.hip.h with RT = 4 at d = 128: four 16-row
# tiles per wave, launch bounds 256, 1; the decode units, RT = 1, are built without the flag): 206 accumulation registers in the default
# form, 81 in VGPR form and faster on every measured shape; its d = 64 instantiations use none either way.  The define
# tells the unit which way it was built, and the unit refuses to compile if that is not its row's way.  $* is the unit's name
SPLIT_FLAGS = -DFA_SPLIT_UNIT=$* $(if $(filter extend_% shared_%,$*),$(MFMA_VGPR) -DFA_SPLIT_MFMA_VGPR)

$(SPLIT_OBJ): build/obj/inst_%.o: $(SPLIT_SRC) $(KHDR)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) $(SPLIT_FLAGS) -c -o $@ $<

build/obj/%.o: $(PKG)/csrc/%.hip $(KHDR)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(LIB): $(KOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared -o $@ $(KOBJ)

oracle: oracle/liboracle_attention.so

# driver: the counterpart of the reference's main.cpp (device properties + the BASELINE configs sharded over the GPUs;
# RCCL reduces elapsed time and an output checksum; naive CPU attention + sampled check in the same run)
$(PKG)/fa_main: $(PKG)/main.cpp $(LIB) include/flash_attention.h
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++20 -o $@ $(PKG)/main.cpp -L$(PKG) -lflash_attention -Wl,-rpath,'$$ORIGIN' \
	    -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib -lpthread

# test harness: the counterpart of the reference's tests/main.cu (launch + CPU check); links the oracle
oracle/liboracle_attention.so: oracle/cpu_attention.c oracle/cpu_attention.h
	$(MAKE) -s -C oracle

tests/fa_test: tests/main.cpp $(LIB) oracle/liboracle_attention.so
	$(HIPCC) -O2 -std=c++17 -o $@ tests/main.cpp -L$(PKG) -lflash_attention -Loracle -loracle_attention \
	    -Wl,-rpath,'$$ORIGIN/../$(PKG)' -Wl,-rpath,'$$ORIGIN/../oracle'

# unit tests of the MFMA fragment layouts and the LDS images (run by tests/conftest.py at session start, checked by tests/test_driver.py)
tests/unit_kernels: tests/unit_kernels.hip $(KHDR)
	$(HIPCC) $(HIPFLAGS) -o $@ tests/unit_kernels.hip

# kernel-variant A/B harness (tuning infrastructure)
tests/fa_tune: tests/fa_tune.hip $(KHDR) oracle/liboracle_attention.so
	$(HIPCC) $(HIPFLAGS) -o $@ tests/fa_tune.hip -Loracle -loracle_attention -Wl,-rpath,'$$ORIGIN/../oracle'

# the seam switches of KernelCfg, one at a time, interleaved (profiles/ARMS_seam.md)
tests/fa_tune_seam: tests/fa_tune_seam.hip $(KHDR)
	$(HIPCC) $(HIPFLAGS) -o $@ tests/fa_tune_seam.hip

# the switches of a wave's last tile (KernelCfg::TAIL, TAIL_HALF), interleaved (profiles/ARMS_tail.md)
tests/fa_tune_tail: tests/fa_tune_tail.hip $(KHDR)
	$(HIPCC) $(HIPFLAGS) -o $@ tests/fa_tune_tail.hip

# ... with the causal d = 128 variants only (a third of the compile time)
tests/fa_tune_c128: tests/fa_tune.hip $(KHDR) oracle/liboracle_attention.so
	$(HIPCC) $(HIPFLAGS) -DFA_TUNE_CAUSAL_D128 -o $@ tests/fa_tune.hip -Loracle -loracle_attention -Wl,-rpath,'$$ORIGIN/../oracle'

# microbenchmarks: instruction issue rates; how busy 2 waves keep one SIMD's MFMA pipe; power-limited ceilings
tests/micro/%: tests/micro/%.hip
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++20 -o $@ $<

# Host-side sanitizers (there is no GPU ASan on this pool): the oracle under gcc's ASan + UBSan, and the library's
# HOST code -- argument validation, the launch routing, plan, plan_ex, shard_range: everything callable without a GPU -- under clang's
# (FlashAttention.hip rebuilt with -fsanitize=address,undefined; the kernel translation units are linked as built).  Each test file
# runs in a process of its own with the matching runtime preloaded; tests/main.cpp (the C++ harness) is compiled and linked under the
# same flags as a build check (running it needs a GPU).
ASAN_DIR  := build/asan
CLANGXX   := /opt/rocm/lib/llvm/bin/clang++
CLANG_ASAN_RT := $(shell /opt/rocm/lib/llvm/bin/clang -print-file-name=libclang_rt.asan-x86_64.so)
GCC_ASAN_RT   := $(shell gcc -print-file-name=libasan.so)
SANFLAGS  := -fsanitize=address,undefined -fno-omit-frame-pointer -g
# asan-host: the library's host code under the sanitizers, and the LADDERS -- stand-alone programs (their own main, the same flags,
# nothing preloaded; tests/host_ladder.h is what they share), each built and run: the validation ladders and plans of the ragged entry
# points, of the six attention-sink entry points beside their _window twins, of the four rope_append ones beside their kv_append twins,
# of the two tree-masked ones beside their sink twins, of the speculative step's rope_append_pos and kv_accept ones beside their rope_append
# and kv_append twins, of the two shared-prefix decode ones and their plan beside flash_attention_decode_window / _paged_window, of the two MLA decode ones and
# their plan beside flash_attention_decode / _paged
LADDERS := host_ladder host_sink_ladder host_rope_ladder host_tree_ladder host_spec_ladder host_cascade_ladder host_mla_ladder
$(ASAN_DIR)/libflash_attention.so: $(LIB)
	@mkdir -p $(ASAN_DIR)
	$(HIPCC) $(HIPFLAGS) $(SANFLAGS) -fno-gpu-sanitize -shared-libsan -c -o $(ASAN_DIR)/FlashAttention.o $(PKG)/csrc/FlashAttention.hip
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared $(SANFLAGS) -shared-libsan -o $@ $(ASAN_DIR)/FlashAttention.o $(filter-out build/obj/FlashAttention.o,$(KOBJ))

ladder-%: tests/%.cpp tests/host_ladder.h $(ASAN_DIR)/libflash_attention.so
	$(CLANGXX) -O1 -std=c++17 $(SANFLAGS) -shared-libsan -o $(ASAN_DIR)/$* $< -L$(ASAN_DIR) -lflash_attention \
	    -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,$(dir $(CLANG_ASAN_RT))
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $(ASAN_DIR)/$*

asan-host: $(addprefix ladder-,$(LADDERS))

asan: asan-host oracle
	gcc -O1 -march=x86-64-v3 -fopenmp -fPIC -Wall -Wextra -std=c11 $(SANFLAGS) -shared -o $(ASAN_DIR)/liboracle_attention.so oracle/cpu_attention.c -lm
	$(HIPCC) -O1 -std=c++17 $(SANFLAGS) -shared-libsan -o $(ASAN_DIR)/fa_test tests/main.cpp -L$(ASAN_DIR) -lflash_attention -Loracle -loracle_attention \
	    -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,'$$ORIGIN/../../oracle'
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 LD_PRELOAD=$(GCC_ASAN_RT) \
	    ORACLE_LIB_PATH=$(CURDIR)/$(ASAN_DIR)/liboracle_attention.so python -m pytest tests/test_oracle.py -q -p no:cacheprovider
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 LD_PRELOAD=$(CLANG_ASAN_RT) \
	    FA_LIB_PATH=$(CURDIR)/$(ASAN_DIR)/libflash_attention.so python -m pytest tests/test_abi.py tests/test_backward_abi.py tests/test_shard.py -q -p no:cacheprovider -m "not gpu"
	@echo "asan: oracle (gcc ASan+UBSan) and library host code (clang ASan+UBSan) clean"

# Device assembly of every library unit, under the flags of its object.  Only the __hip_cuid_ lines differ between two compiles of one
# source, so they are dropped: a source-level change that is meant to be free can be proved so by comparing build/asm before and after.
KASM     := $(patsubst $(PKG)/csrc/%.hip,build/asm/%.s,$(KSRC)) $(SPLIT_UNITS:%=build/asm/inst_%.s)
build/asm/inst_bf16_pair_d128.s build/asm/inst_bwd_bf16.s build/asm/inst_mla_decode.s: HIPFLAGS += $(MFMA_VGPR)
define ASM_RECIPE
@mkdir -p build/asm
$(HIPCC) $(HIPFLAGS) $(1) -S --cuda-device-only -o $@.tmp $<
grep -v __hip_cuid_ $@.tmp > $@
@rm -f $@.tmp
endef

$(SPLIT_UNITS:%=build/asm/inst_%.s): build/asm/inst_%.s: $(SPLIT_SRC) $(KHDR)
	$(call ASM_RECIPE,$(SPLIT_FLAGS))

build/asm/%.s: $(PKG)/csrc/%.hip $(KHDR)
	$(call ASM_RECIPE)

asm: $(KASM)

clean:
	rm -f $(LIB) $(PKG)/fa_main tests/fa_test tests/fa_tune tests/fa_tune_seam tests/fa_tune_tail tests/unit_kernels tests/micro/simd_mix tests/micro/valu_rates tests/micro/atomic_latency oracle/liboracle_attention.so
	rm -rf build
.PHONY: all lib tune oracle clean asm asan asan-host
