// tests/fa_tune_tail.hip -- the switches of a wave's last tile (KernelCfg::TAIL, TAIL_HALF: csrc/kernel_bf16.hip.h, SlotEngine::tail_step)
// on the library's default kernel of BASELINE cfg2 (bf16, d = 128, fp32 O, causal), timed against each other the way tests/fa_tune_seam.hip
// times its arms: INTERLEAVED rounds inside one process, a fresh seeded random order per round, random N(0,1) data.  Every arm's O is
// compared bit for bit with the library's kernel (arm 0); the count of differing elements must be 0.  The yardstick arm -- tail off --
// is listed twice, "(a)" and "(b)": ONE template instantiation launched under two labels; what the two measure apart is the
// launch-to-launch scatter of the run.  Tuning infrastructure, not product: `make tests/fa_tune_tail`.
//
// usage: fa_tune_tail [--rounds R] [--only i,j,...] [--shape B H S]
//   a STAMP arm prints its segment sums (cycles per workgroup-wave) and the per-unit cycles of the steps that waves 6 and 7 run alone;
//   run one STAMP arm per process (--only): they share the buffer
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../flash-attention-cuda-c_amd/csrc/kernel_bf16.hip.h"

#define HIP_CHECK(x)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "HIP error: %s (%s:%d)\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(2);                                                                          \
        }                                                                                     \
    } while (0)

using namespace fa;
constexpr int D = 128;

struct Arm {
    std::string name;
    void (*launch)(const Params&);
    bool stamp;
};

static int g_cus = 256;

template <class K>
static void launch_cfg(const Params& p) {
    static bool once = [] {
        HIP_CHECK(hipFuncSetAttribute((const void*)fwd_mfma_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, K::LDS_BYTES));
        return true;
    }();
    (void)once;
    Params q = p;
    q.hp = K::MIX ? std::min(p.nQ, 1024 / 256) : 0;
    q.jpx = std::min(q.cpx, g_cus / 8);   // persistent grid: one workgroup per CU, or one per unit when there are fewer units
    hipLaunchKernelGGL((fwd_mfma_kernel<K>), dim3(8 * q.jpx), dim3(64 * K::NWAVES), K::LDS_BYTES, nullptr, q);
}

template <Opt O>
using Mixed = KernelCfg<D, true, float, 2, O>;   // the causal default (MixCfg) with explicit switches

static std::vector<Arm> arms(bool) {
    std::vector<Arm> v;
    v.push_back({"library (MixCfg)", launch_cfg<MixCfg<D, float>>, false});
    v.push_back({"tail off (a)", launch_cfg<Mixed<Opt{.m16 = 0, .mix = true, .tail = 0}>>, false});
    v.push_back({"tail off (b)", launch_cfg<Mixed<Opt{.m16 = 0, .mix = true, .tail = 0}>>, false});
    v.push_back({"tail on, HALF off", launch_cfg<Mixed<Opt{.m16 = 0, .mix = true, .tail = 1, .tail_half = 0}>>, false});
    v.push_back({"tail on, HALF on", launch_cfg<Mixed<Opt{.m16 = 0, .mix = true, .tail = 1, .tail_half = 1}>>, false});
    v.push_back({"STAMP tail off", launch_cfg<Mixed<Opt{.stamp = true, .m16 = 0, .mix = true, .tail = 0}>>, true});
    v.push_back({"STAMP tail on, HALF on", launch_cfg<Mixed<Opt{.stamp = true, .m16 = 0, .mix = true, .tail = 1, .tail_half = 1}>>, true});
    return v;
}

int main(int argc, char** argv) {
    int B = 8, H = 16, S = 4096, rounds = 21;
    const int causal = 1;
    std::vector<int> only;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--rounds" && i + 1 < argc) rounds = atoi(argv[++i]);
        else if (a == "--shape" && i + 3 < argc) { B = atoi(argv[i + 1]); H = atoi(argv[i + 2]); S = atoi(argv[i + 3]); i += 3; }
        else if (a == "--only" && i + 1 < argc) {
            for (char* t = strtok(argv[++i], ","); t; t = strtok(nullptr, ",")) only.push_back(atoi(t));
        }
    }
    if (B < 1 || H < 1 || S < 64 || (int64_t)B * H * S * D >= (1ll << 31)) { fprintf(stderr, "shape out of range\n"); return 2; }
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus >= 8) g_cus = cus;

    const int BH = B * H;
    const size_t n = (size_t)BH * S * D;
    const size_t per = (size_t)std::min(BH, 8) * S * D;   // eight distinct heads per tensor, repeated
    std::vector<uint16_t> h(per);
    void* d[3];
    std::mt19937_64 gen(12345);
    std::normal_distribution<float> nd(0.f, 1.f);
    for (int t = 0; t < 3; ++t) {
        for (size_t i = 0; i < per; ++i) {   // bf16 by truncation: any N(0,1)-like data serves
            const float x = nd(gen);
            uint32_t u;
            memcpy(&u, &x, 4);
            h[i] = (uint16_t)(u >> 16);
        }
        HIP_CHECK(hipMalloc(&d[t], n * 2));
        for (size_t off = 0; off < n; off += per)
            HIP_CHECK(hipMemcpy((char*)d[t] + off * 2, h.data(), std::min(per, n - off) * 2, hipMemcpyHostToDevice));
    }
    void* dout;
    HIP_CHECK(hipMalloc(&dout, n * 4));
    Params p{};
    p.Q = d[0]; p.K = d[1]; p.V = d[2]; p.O = dout;
    p.qS = p.kS = p.vS = p.oS = D;
    p.qH = p.kH = p.vH = p.oH = (int64_t)S * D;
    p.qB = p.kB = p.vB = p.oB = (int64_t)H * S * D;
    p.B = B; p.H = H; p.S = S; p.Sk = S; p.d = D;
    p.nQ = (S + 255) / 256;
    p.units = BH * p.nQ;
    p.cpx = (p.units + 7) / 8;
    p.scale = 1.0f / std::sqrt((float)D);
    p.scale_log2 = p.scale * 1.4426950408889634f;
    const size_t dbg_words = (size_t)8 * p.cpx * 8 * 24;
    unsigned long long* ddbg;
    HIP_CHECK(hipMalloc(&ddbg, dbg_words * 8));
    HIP_CHECK(hipMemset(ddbg, 0, dbg_words * 8));
    p.dbg = ddbg;

    std::vector<Arm> all = arms(causal != 0), v;
    if (only.empty()) { for (auto& a : all) if (!a.stamp) v.push_back(a); }
    else for (int i : only) if (i >= 0 && i < (int)all.size()) v.push_back(all[i]);
    if (v.empty()) { fprintf(stderr, "no arm selected\n"); return 2; }
    printf("problem: B=%d H=%d S=%d d=%d causal=%d rounds=%d CUs=%d\n", B, H, S, D, causal, rounds, g_cus);

    // every arm's O against the first arm's, bit for bit
    std::vector<uint32_t> o0(n), o(n);
    int differ = 0;
    for (size_t vi = 0; vi < v.size(); ++vi) {
        HIP_CHECK(hipMemset(dout, 0xff, n * 4));
        v[vi].launch(p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy((vi ? o : o0).data(), dout, n * 4, hipMemcpyDeviceToHost));
        size_t bad = 0, nan = 0;
        for (size_t i = 0; i < n; ++i) {
            if (vi && o[i] != o0[i]) ++bad;
            if (((vi ? o : o0)[i] & 0x7f800000u) == 0x7f800000u) ++nan;
        }
        printf("  [%zu] %-40s elements that differ from [0]: %zu  non-finite: %zu\n", vi, v[vi].name.c_str(), bad, nan);
        differ += bad != 0 || nan != 0;
    }

    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
    const int reps = 5;
    std::vector<std::vector<float>> ms(v.size());
    for (auto& a : v) { a.launch(p); a.launch(p); }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemset(ddbg, 0, dbg_words * 8));
    std::vector<size_t> order(v.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    unsigned long long lcg = 0x9E3779B97F4A7C15ull;
    for (int r = 0; r < rounds; ++r) {
        for (size_t i = order.size(); i > 1; --i) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(order[i - 1], order[(lcg >> 33) % i]);
        }
        for (size_t vi : order) {
            HIP_CHECK(hipEventRecord(e0, nullptr));
            for (int i = 0; i < reps; ++i) v[vi].launch(p);
            HIP_CHECK(hipEventRecord(e1, nullptr));
            HIP_CHECK(hipEventSynchronize(e1));
            float t;
            HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
            ms[vi].push_back(t / reps);
        }
    }
    {   // segment sums of the STAMP arm (Params::dbg: 24 words per wave, kernel_bf16.hip.h: run_units), per workgroup-wave
        std::vector<unsigned long long> w(dbg_words);
        HIP_CHECK(hipMemcpy(w.data(), ddbg, dbg_words * 8, hipMemcpyDeviceToHost));
        double seg[24] = {0};
        for (size_t i = 0; i < dbg_words / 24; ++i)
            for (int k = 0; k < 24; ++k) seg[k] += (double)w[i * 24 + k];
        // waves 6 and 7 (rows 192 .. 255 of a unit): cycles inside the tile steps (phases A and B and what follows them up to the
        // staging wait) per unit -- their last two steps run with no other wave of the workgroup in a full step
        double w67 = 0, n67 = 0, units = 0;
        for (size_t i = 0; i < dbg_words / 24; ++i)
            if (w[i * 24 + 11] && (i % 8) >= 6) { w67 += (double)(w[i * 24 + 1] + w[i * 24 + 2] + w[i * 24 + 3]); n67 += (double)w[i * 24 + 6]; units += 1; }
        if (units > 0) printf("  STAMP, waves 6 and 7: %.0f cycles in %.0f tile steps per workgroup-wave (%.1f per step)\n", w67 / units, n67 / units, w67 / n67);
        if (seg[11] > 0) {
            const double nw = seg[11];
            printf("  STAMP, cycles per workgroup-wave (%.0f waves, the arm's last launch): lifetime %.0f | Q load + pin %.0f | stage tiles 0, 1 + barrier %.0f | "
                   "QK(0) + max %.0f | tile loop %.0f | finite check %.0f | epilogue %.0f | setup %.0f | next unit decode + prefetch issue %.0f\n",
                   nw, seg[0] / nw, seg[7] / nw, seg[8] / nw, seg[9] / nw, (seg[1] + seg[2] + seg[3] + seg[5]) / nw, seg[10] / nw, seg[4] / nw, seg[12] / nw, seg[13] / nw);
        }
    }
    const double flops = (causal ? 2.0 : 4.0) * BH * (double)S * S * D;
    for (size_t vi = 0; vi < v.size(); ++vi) {
        std::sort(ms[vi].begin(), ms[vi].end());
        const double med = ms[vi][ms[vi].size() / 2];
        printf("  [%zu] %-40s med %.4f ms  min %.4f ms  %.1f TFLOP/s  best %.1f\n", vi, v[vi].name.c_str(), med, ms[vi][0], flops / med / 1e9, flops / ms[vi][0] / 1e9);
    }
    return differ ? 1 : 0;
}
