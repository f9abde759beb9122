// slot_engine.hip.h -- what the two per-wave MFMA engines of the forward pass share: WaveCompute (32x32x16, computers.hip.h) and
// WaveCompute16 (16x16x32, computers16.hip.h) derive from SlotEngine<W, C> (CRTP, as the stages derive from StageAll).
//
// Shared, stated here once: the slot plan (which overall slot carries which score element, staging load and LDS write), the tile
// step around the two slot sequences, the running-max bookkeeping (first_max / decide / the rescale site), bringing Q into
// fragments, and the LSE store of the epilogue.  (The read-out loops of store_o_lds / store_o_lds32 stay with the engines: hipcc lays
// the guarded stores' blocks out differently as soon as those loops sit in a function of their own.)
//
// An engine supplies
//   geometry   GROUPS query-row groups of RG = 1 << LOG_RG rows per wave (GROUPS * RG = 32), FPG Q fragments per group;
//              SA, SB (slots of phase A / B), SPAN, NE, NPRE, NL, NW;
//   state      qf[GROUPS][FPG], m[GROUPS], mx_a / mx_b[GROUPS], kf[NPRE], need, t_mid, t_end;
//   hooks      max_over_row(x)          cross-lane maximum over the lanes that share a query row
//              begin_tile(st, wr, nxt)  per-tile resets and st.set_dst, in the engine's own order
//              end_sums()               closes the tile's row sums
//              rescale(g, alpha)        multiplies row group g's sums and O accumulators
//   and everything that knows an MFMA shape: slots_a, slots_b, exp_elem, mask, row_max, k_read (also max3_slot, v_frag, qk_all, p_frag).
// Stage and score types are deduced (St, Sc): W is incomplete where the base's member declarations are instantiated.
#pragma once

#include "loaders.hip.h"

namespace fa {

template <class W, class C>
struct SlotEngine {
    __device__ __forceinline__ W& self() { return *static_cast<W*>(this); }

    // ---- slot plan -----------------------------------------------------------------------------
    __host__ __device__ static constexpr int elem_slot(int E) { return E * W::SPAN / W::NE; }
    // overall slot (0 .. SA + SB - 1) that issues staging load / LDS-DMA piece n of the tile two ahead: the odd slots from 1 on.
    // (Later is worse -- the pieces then land after the end-of-step wait: phase A's second half -2.6 %, phase B -9 ... -13 %,
    //  profiles/r03_tune_c_dma_slots_*.log.)
    __host__ __device__ static constexpr int load_slot(int n) { return 1 + 2 * n; }
    // LDS write n of the tile two ahead sits in phase B slot SB/2 + n * wstep(): every wstep()-th slot of phase B's second half
    __host__ __device__ static constexpr int wstep() { return 2 * W::NW <= W::SB / 2 + 1 ? 2 : 1; }
    // F16W (32x32x16: the mixed-precision kernels, C::MIX, only; 16x16x32: those and the fp16-weights kernels, C::P_F16): the unit runs
    // with fp16 softmax weights -- P rounded to fp16, V staged as fp16 through registers (MixStage), P.V on v_mfma_f32_32x32x16_f16 /
    // v_mfma_f32_16x16x32_f16.  A property of the pass, handed down as a template argument (default: bf16 weights, as in the stages).
    template <int SLOT, bool F16W = false, int N = 0, class St>
    __device__ __forceinline__ void load_in_slot(St& st, int t_load) {
        if constexpr (N < W::NL) {
            if constexpr (load_slot(N) == SLOT) st.template load<N, F16W>(t_load);   // (MixStage: V by DMA or, fp16 units, through registers)
            load_in_slot<SLOT, F16W, N + 1>(st, t_load);
        }
    }
    template <int J, bool F16W = false, class St>
    __device__ __forceinline__ void write_in_slot(St& st, lds_ptr wr_slot) {
        constexpr int H = W::SB / 2, WSTEP = wstep();   // (the whole plan, loads included, is checked here: W is incomplete at class scope)
        static_assert(2 * W::NL <= W::SA && WSTEP * (W::NW - 1) < W::SB - H, "staging does not fit the slot plan");
        if constexpr (J >= H && (J - H) % WSTEP == 0 && (J - H) / WSTEP < W::NW) st.template write<(J - H) / WSTEP, F16W>(wr_slot);
    }
    template <int SLOT, bool F16W = false, int E = 0, class Sc>
    __device__ __forceinline__ void exp_slot(const Sc& cur, float c) {
        if constexpr (E < W::NE) {
            if constexpr (elem_slot(E) == SLOT) self().template exp_elem<E, F16W>(cur, c);
            exp_slot<SLOT, F16W, E + 1>(cur, c);
        }
    }

    // ---- Q ---------------------------------------------------------------------------------------
    // Q fragment (g, u) of row q = row0 + RG*g + (lane & (RG-1)): 16 bytes at byte (64/RG)*16*u + 16*(lane >> LOG_RG) of the row.
    // 32x32x16, bf16: d = 16u + 8h .. +7 (k-step u).  fp8: d = 32u + 16h .. +15 -- the contraction order is permuted the same way
    // for K (chunk 2u+h of the K image), so one 16-byte fragment feeds two MFMAs.
    // row_bytes < D*ESZ (C::PAD): fragments past the end of the row are zero and are never read from memory.
    __device__ __forceinline__ void load_q(const char* Qh, int64_t qS_bytes, int row0, int S, int lane, int row_bytes = C::D * C::ESZ) {
        W& w = self();
        constexpr int FSTRIDE = (64 / W::RG) * 16;
#pragma unroll
        for (int g = 0; g < W::GROUPS; ++g) {
            int row = row0 + W::RG * g + (lane & (W::RG - 1));
            row = row < S ? row : S - 1;
            const char* src = Qh + row * qS_bytes + (lane >> W::LOG_RG) * 16;
#pragma unroll
            for (int u = 0; u < W::FPG; ++u) {
                if constexpr (C::PAD) {
                    w.qf[g][u] = u32x4{0u, 0u, 0u, 0u};
                    if (u * FSTRIDE + (lane >> W::LOG_RG) * 16 < row_bytes) w.qf[g][u] = load_global_b128<C::Q_CACHE>(src + u * FSTRIDE);
                } else {
                    w.qf[g][u] = load_global_b128<C::Q_CACHE>(src + u * FSTRIDE);
                }
            }
        }
    }
    // Coalesced form (KernelCfg::COALESCED_Q).  load_q above has every lane read 16-byte pieces of its own row: one
    // instruction touches 32 rows x 2 pieces, 64 separate 16-byte requests.  Here instruction i fetches 64/QCH WHOLE
    // rows (QCH = 16-byte chunks per row; lane = (row, chunk)), and the fragments are formed by one trip through
    // this wave's private LDS region: chunk c of row q is parked at chunk c ^ (q & (QCH-1)), so the 16 rows of a
    // ds_read_b128 lane group land on different banks.  Same instruction count, a quarter of the memory requests.
    static constexpr int QCH = (C::D * C::ESZ) / 16, QRPI = 64 / QCH;   // 16-byte chunks per Q row; rows fetched per instruction
    __device__ __forceinline__ void load_q_rows(const char* Qh, int64_t qS_bytes, int row0, int S, int lane) {
        static_assert(32 / QRPI == W::GROUPS * W::FPG, "coalesced Q: as many loads as fragments");
#pragma unroll
        for (int i = 0; i < W::GROUPS * W::FPG; ++i) {
            int row = row0 + i * QRPI + lane / QCH;
            row = row < S ? row : S - 1;
            self().qf[i / W::FPG][i % W::FPG] = load_global_b128<C::Q_CACHE>(Qh + row * qS_bytes + (lane % QCH) * 16);
        }
    }
    // region: 32 rows x D*ESZ bytes private to this wave, not aliased by anything live (kernel_bf16.hip.h)
    __device__ __forceinline__ void q_rows_to_fragments(lds_ptr region, int lane) {
        W& w = self();
        constexpr int ROWB = C::D * C::ESZ;
#pragma unroll
        for (int i = 0; i < W::GROUPS * W::FPG; ++i) {
            const int q = i * QRPI + lane / QCH, c = lane % QCH;
            lds_write_b128(region, q * ROWB + (((c ^ q) & (QCH - 1)) << 4), w.qf[i / W::FPG][i % W::FPG]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // own writes only: LDS executes a wave's accesses in order
#pragma unroll
        for (int g = 0; g < W::GROUPS; ++g)
#pragma unroll
            for (int u = 0; u < W::FPG; ++u) {
                const int q = W::RG * g + (lane & (W::RG - 1)), c = (64 / W::RG) * u + (lane >> W::LOG_RG);
                w.qf[g][u] = __builtin_bit_cast(u32x4, lds_read_b128(region, q * ROWB + (((c ^ q) & (QCH - 1)) << 4)));
            }
    }
    // Make the Q fragments look "consumed" so hipcc waits for their loads HERE and not with a
    // pessimistic vmcnt inside the main loop (where it would also drain the tile prefetch).
    __device__ __forceinline__ void pin_q() {
#pragma unroll
        for (int g = 0; g < W::GROUPS; ++g)
#pragma unroll
            for (int u = 0; u < W::FPG; ++u) asm volatile("" : "+v"(self().qf[g][u]));
    }

    // ---- running row max -----------------------------------------------------------------------
    // Tile 0 of a pass: m = its row max (m = -inf before; O and l are still 0).
    template <class Sc>
    __device__ __forceinline__ void first_max(const Sc& n, float c) {
        W& w = self();
#pragma unroll
        for (int g = 0; g < W::GROUPS; ++g) w.m[g] = fmaxf(w.m[g], W::max_over_row(w.row_max(n, g)) * c);
    }
    // tracked pass: mx_a / mx_b hold this lane's maxima of S(t+1); need = some row of the wave has to move its reference max
    __device__ __forceinline__ void decide(float c) {
        W& w = self();
        bool any = false;
#pragma unroll
        for (int g = 0; g < W::GROUPS; ++g) {
            const float mx = W::max_over_row(fmaxf(w.mx_a[g], w.mx_b[g])) * c;
            any = any || (mx > w.m[g] + (float)C::THR);
            w.mx_a[g] = mx;   // keep the scaled row max for the rescale body
        }
        w.need = __any(any);
    }

    // ---- the tile step ---------------------------------------------------------------------------
    // One tile: cur = S(t) (consumed), nxt = S(t+1) (produced; on the wave's last tile it is computed from a tile the wave does not
    // need and ignored: one hot code path; under KernelCfg::TAIL the optimistic passes run that tile through tail_step instead).  TRACK = true: running row max with lazy rescale (always safe).  TRACK = false: the
    // optimistic pass -- m stays the row max of tile 0 and no max / decision / rescale is issued.
    template <bool TRACK, bool F16W = false, class St, class Sc>
    __device__ __forceinline__ void tile_step(St& st, int t_load, lds_ptr wr_slot, lds_ptr k_next, lds_ptr v_cur, int kbase, int vbase, float c,
                                              const Sc& cur, Sc& nxt, bool has_next, bool mask_next, int kv0_next, int q_row0, int S, int lane) {
        W& w = self();
        w.begin_tile(st, wr_slot, nxt);
#pragma unroll
        for (int i = 0; i < W::NPRE; ++i) w.kf[i] = w.k_read(k_next, kbase, i);
        if constexpr (C::PRIO_A) __builtin_amdgcn_s_setprio(1);
        __builtin_amdgcn_sched_barrier(0);
        w.template slots_a<0, F16W>(st, t_load, k_next, v_cur, kbase, vbase, c, cur, nxt);
        if constexpr (C::PRIO_A) {
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (C::STAMP) w.t_mid = cycle_stamp();
        w.template slots_b<TRACK, 0, F16W>(st, wr_slot, v_cur, vbase, c, cur, nxt);
        if constexpr (C::STAMP) w.t_end = cycle_stamp();
        w.end_sums();
        // ONE rescale site: the masked (diagonal / ragged) tile only recomputes the scalar decision and the row max.  (Two sites
        // that both multiply O made hipcc copy all 64 accumulator registers twice per tile on the common path.)
        if (has_next && mask_next) {
            w.mask(nxt, kv0_next, q_row0, S, lane);
            if constexpr (TRACK) {
#pragma unroll
                for (int g = 0; g < W::GROUPS; ++g) { w.mx_a[g] = w.row_max(nxt, g); w.mx_b[g] = w.mx_a[g]; }
                decide(c);
            }
        }
        if constexpr (TRACK) {
            if (has_next && w.need) {
#pragma unroll
                for (int g = 0; g < W::GROUPS; ++g) {
                    const float mn = fmaxf(w.m[g], w.mx_a[g]);
                    const float alpha = fast_exp2(w.m[g] - mn);
                    w.m[g] = mn;
                    w.rescale(g, alpha);
                }
            }
        }
    }

    // The wave's LAST tile in an optimistic pass (KernelCfg::TAIL; attention_pass: the kind-1 steps): phase B alone.  cur = S(t) is
    // consumed -- its exponentials, the packs, the P.V MFMAs with their V^T reads VPRE ahead -- and nothing is produced: no next
    // score buffer, no K fragment window, no K read, no QK^T, no mask, no decision.  The wave's pieces of tile t_load still go to
    // ring slot wr_slot (the waves below it in the unit read them), all requested in front of the first MFMA, the fp16 form's LDS
    // writes behind the last.  One-MFMA slots fenced like slots_b (the engine's slots_t).  Same weights, sums and products in the
    // same order as tile_step: the result keeps its bits.
    // half (wave-uniform): keys 0 .. 31 of the tile only -- for the wave whose rows start on a 64-row boundary the keys 32 .. 63 of its
    // diagonal tile are masked in every row: their weights are exp2(-inf) = +0, which neither a row sum nor (V finite) an accumulator
    // notices.  The two forms share the lead-in and the slots of k-step 0 and part behind them (tail_rest<HALF>).  (As two whole
    // bodies hipcc hoists what they have in common -- 32 v_fma, the staging offsets -- in front of the branch and spills it.)
    template <bool HALF, bool F16W, class Sc>
    __device__ __forceinline__ void tail_rest(lds_ptr v_cur, int vbase, float c, const Sc& cur) {
        constexpr int DB = W::DB, ST = (HALF ? 2 : 4) * DB;
        self().template slots_t<DB, ST, ST, F16W>(v_cur, vbase, c, cur);
    }
    template <bool F16W = false, class St, class Sc>
    __device__ __forceinline__ void tail_step(St& st, int t_load, lds_ptr wr_slot, lds_ptr v_cur, int vbase, float c, const Sc& cur, bool half) {
        W& w = self();
        constexpr int DB = W::DB;
        w.begin_tail(st, wr_slot);
        __builtin_amdgcn_sched_barrier(0);
        w.template tail_pre<0, F16W>(st, t_load, v_cur, vbase, c, cur);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (C::STAMP) w.t_mid = cycle_stamp();
        w.template slots_t<0, DB, 2 * DB, F16W>(v_cur, vbase, c, cur);   // (the V^T fragments of k-step 1 are read in either form)
        if (half) tail_rest<true, F16W>(v_cur, vbase, c, cur);
        else tail_rest<false, F16W>(v_cur, vbase, c, cur);
        st.template write_all<F16W>(wr_slot);
        if constexpr (C::STAMP) w.t_end = cycle_stamp();
        w.end_sums();
    }

    // ---- epilogue -------------------------------------------------------------------------------
    // ln sum_k exp(scale*s_k) = (m + log2 l) * ln 2   (m is the reference max in the scaled log2 domain)
    __device__ __forceinline__ void store_lse(float* lse_head, float l_tot, int g, int row0, int S, int lane) {
        const int qi = row0 + W::RG * g + (lane & (W::RG - 1));
        if (lse_head && lane < W::RG && qi < S) lse_head[qi] = (self().m[g] + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f;
    }
};

}  // namespace fa
