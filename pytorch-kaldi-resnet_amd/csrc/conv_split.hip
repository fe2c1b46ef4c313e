// bf16-split instantiations of the implicit-GEMM convolution (see conv_kernel.h, ConvCfg<SPLIT>) (the matching weight
// packing is in pack.hip).  fp32 activations and weights go in, fp32 results come out; inside, every operand is the exact sum of three
// bf16 terms and the matrix cores multiply the 6 most significant cross terms (or all 9) with fp32 accumulation; split == 3
// is the fp16 two-term form (three products on v_mfma_f32_32x32x16_f16, power-of-two operand scales).
#include "conv_kernel.h"

// ---- compile-time flag variants (conv_kernel.h, FL), f16x3 mode.  One list serves the selection and the launchers: a flag word
// (with the SPK_FL_* pointer bits) and the register tiles it is instantiated for.
// V2 / V1: the two fused BatchNorm-backward data gradients of a 32-channel BasicBlock - conv2's (mask of the block output as sign
// bits, pair side output, statistics of bn1's backward with the mask recomputed) and conv1's (mask recomputed, masked shortcut
// add, statistics of the previous block's last BatchNorm by sign bits)
constexpr int FLV_BNBWD2 = SPK_IN_BNBWD | SPK_SIDE_PRESPLIT | SPK_EPI_STATS | SPK_EPI_BNBWD | SPK_FL_INMASK;
constexpr int FLV_BNBWD1 = SPK_IN_BNBWD | SPK_SIDE_PRESPLIT | SPK_EPI_ADD | SPK_EPI_STATS | SPK_EPI_BNBWD | SPK_FL_ADDMASK | SPK_FL_BNMASK;
// the forward launches of the training step: fused input BatchNorm + ReLU with statistics, plain input with statistics (the
// stride-2 and 1x1 convolutions of a downsample block: also (3, 2) and (1, 4))
constexpr int FLV_FWD_AFF = SPK_IN_AFFINE_RELU | SPK_EPI_STATS;
constexpr int FLV_FWD = SPK_EPI_STATS;
// the data gradients of a downsample block: a parity class of the stride-2 3x3 (pair input, nothing else), and the 1x1
// shortcut accumulated onto them (plain input, unmasked add)
constexpr int FLV_DGRAD_PAIR = SPK_IN_PRESPLIT;
constexpr int FLV_DGRAD_ADD = SPK_EPI_ADD;

static constexpr bool split_has_fl(int MT, int NT, int ck, int fl) {
    const bool t21 = MT == 2 && NT == 1, t12 = MT == 1 && NT == 2, t22 = MT == 2 && NT == 2, t32 = MT == 3 && NT == 2;
    if (ck == 32) return (t21 || (MT == 1 && NT == 1)) && (fl == FLV_BNBWD1 || fl == FLV_BNBWD2);
    switch (fl) {
        case FLV_BNBWD1: case FLV_BNBWD2: return t21;
        case FLV_FWD_AFF: return t21 || t12 || t22;
        case FLV_FWD: return t21 || t12 || t22 || t32 || (MT == 1 && NT == 4);
        case FLV_DGRAD_PAIR: case FLV_DGRAD_ADD: return t21 || t22 || t32;
    }
    return false;
}

int spk_split_variant_of(int MT, int NT, int split, int ck, int flags, int ptrs) {
#ifdef SPK_NO_FL_VARIANTS
    return -1;
#else
    if (!spk_fl_variants_enabled() || split != 3 || (flags & SPK_EPI_WMASK)) return -1;      // (the length-masked instance is no variant)
    int fl = flags;
    if (flags & SPK_IN_BNBWD) {
        if (ptrs & (SPK_PTR_IN_ACT | SPK_PTR_BN_ACT | SPK_PTR_SIDE_DZ)) return -1;
        fl |= ((ptrs & SPK_PTR_ADD_MASK) ? SPK_FL_ADDMASK : 0) | ((ptrs & SPK_PTR_BN_MASK) ? SPK_FL_BNMASK : 0) |
              ((ptrs & SPK_PTR_IN_MASK) ? SPK_FL_INMASK : 0);
    } else if (ptrs & (SPK_PTR_ADD_MASK | SPK_PTR_BN_MASK | SPK_PTR_BN_ACT)) {
        return -1;
    }
    return split_has_fl(MT, NT, ck, fl) ? fl : -1;
#endif
}

// the instance the selection names; a word it names without an instance here is an error, never the generic kernel
#define FL_CASE(V, CK)                                                                                                                \
    case V:                                                                                                                           \
        if constexpr (split_has_fl(MT, NT, CK, V)) {                                                                                  \
            hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, ((V) & SPK_IN_BNBWD) != 0, 3, V, CK>), dim3(a.nblocks), dim3(256), lds_bytes, st, a); \
            return true;                                                                                                              \
        }                                                                                                                             \
        break;

// whole-pixel form of the fused BatchNorm-backward data gradient at Cin = 32 (conv_kernel.h, CKP = 32): the register tiles of
// its two candidate tiles - (2, 1) for 16 x 16 pixels, (1, 1) for 128-pixel tiles - with the same compile-time flag variants as
// the 16-channel form below, and the generic FL = -1
template <int MT, int NT>
static bool launch_fl_ck32(int fl, const ConvArgs& a, size_t lds_bytes, hipStream_t st) {
#ifndef SPK_NO_FL_VARIANTS
    switch (fl) {
        FL_CASE(FLV_BNBWD2, 32)
        FL_CASE(FLV_BNBWD1, 32)
    }
#endif
    return false;
}

template <int MT, int NT>
static int launch_split_ck32(const ConvArgs& a, size_t lds_bytes, hipStream_t st) {
    const int fl = spk_split_variant_of(MT, NT, 3, 32, a.flags, conv_ptr_pattern(a));
    if (fl < 0)
        hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, true, 3, -1, 32>), dim3(a.nblocks), dim3(256), lds_bytes, st, a);
    else if (!launch_fl_ck32<MT, NT>(fl, a, lds_bytes, st)) {
        spk_set_error("spk_conv_mfma: no instance of flag variant 0x%x for MT=%d NT=%d (32-channel planes)", fl, MT, NT);
        return -1;
    }
    SPK_LAUNCH_CHECK("spk_conv_mfma(split, 32-channel planes)");
    return 0;
}

template <int MT, int NT>
static bool launch_fl(int fl, const ConvArgs& a, size_t lds_bytes, hipStream_t st) {
#ifndef SPK_NO_FL_VARIANTS
    switch (fl) {
        FL_CASE(FLV_BNBWD2, SPK_SPLIT_CK)
        FL_CASE(FLV_BNBWD1, SPK_SPLIT_CK)
        FL_CASE(FLV_FWD_AFF, SPK_SPLIT_CK)
        FL_CASE(FLV_FWD, SPK_SPLIT_CK)
        FL_CASE(FLV_DGRAD_PAIR, SPK_SPLIT_CK)
        FL_CASE(FLV_DGRAD_ADD, SPK_SPLIT_CK)
    }
#endif
    return false;
}
#undef FL_CASE

template <int MT, int NT, int SPLIT>
static int launch_split(const ConvArgs& a, size_t lds_bytes, hipStream_t st) {
    const int fl = spk_split_variant_of(MT, NT, SPLIT, SPK_SPLIT_CK, a.flags, conv_ptr_pattern(a));
    if (fl >= 0) {
        if (!launch_fl<MT, NT>(fl, a, lds_bytes, st)) {
            spk_set_error("spk_conv_mfma: no instance of flag variant 0x%x for MT=%d NT=%d", fl, MT, NT);
            return -1;
        }
    } else if (a.flags & SPK_IN_BNBWD) {
        hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, true, SPLIT>), dim3(a.nblocks), dim3(256), lds_bytes, st, a);
    } else if (a.flags & SPK_EPI_WMASK) {      // length-masked eval forward (conv_kernel.h, WM)
        hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, false, SPLIT, SPK_EPI_WMASK>), dim3(a.nblocks), dim3(256), lds_bytes, st, a);
    } else {
        hipLaunchKernelGGL((conv_mfma_kernel<MT, NT, false, SPLIT>), dim3(a.nblocks), dim3(256), lds_bytes, st, a);
    }
    SPK_LAUNCH_CHECK("spk_conv_mfma(split)");
    return 0;
}

int spk_launch_conv_split(const ConvArgs& a, size_t lds_bytes, int MT, int NT, int split, int ck, hipStream_t st) {
    if (ck == 32) {      // (the entry has checked: f16x3, Cin = 32, fused BatchNorm backward)
        if (MT == 2 && NT == 1) return launch_split_ck32<2, 1>(a, lds_bytes, st);
        if (MT == 1 && NT == 1) return launch_split_ck32<1, 1>(a, lds_bytes, st);
        spk_set_error("spk_conv_mfma: 32-channel planes are instantiated for MT=2 / MT=1 with NT=1, not MT=%d NT=%d", MT, NT);
        return -1;
    }
#define CASE(M, N)                                                      \
    if (MT == M && NT == N) {                                           \
        if (split == 3) return launch_split<M, N, 3>(a, lds_bytes, st); \
        if (split == 6) return launch_split<M, N, 6>(a, lds_bytes, st); \
        return launch_split<M, N, 9>(a, lds_bytes, st);                 \
    }
    CASE(1, 1) CASE(2, 1) CASE(3, 1) CASE(4, 1) CASE(1, 2) CASE(2, 2) CASE(3, 2) CASE(1, 4)
#undef CASE
    spk_set_error("spk_conv_mfma: unsupported split tile config MT=%d NT=%d", MT, NT);
    return -1;
}

#ifdef CONV_STAMPS
extern "C" int spk_debug_stamps(unsigned long long* out, int nblocks) {     // diagnostic builds only (never in the in-tree library)
    if (nblocks < 0) {        // reset
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_conv_stamps)) != hipSuccess) return -1;
        return (int)hipMemset(p, 0, sizeof(unsigned long long) * 16 * CONV_STAMP_BLOCKS);
    }
    if (nblocks > CONV_STAMP_BLOCKS) nblocks = CONV_STAMP_BLOCKS;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_conv_stamps), (size_t)nblocks * 16 * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif
