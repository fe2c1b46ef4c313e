// In-wave pipelined instantiations of the implicit-GEMM convolution (conv_kernel.h, PIPE): f16x3 operands, nine taps,
// the next chunk staged in the shadow of the current chunk's matrix instructions, two LDS tiles, one barrier per chunk.
#include "conv_kernel.h"

// ---- compile-time flag variants (conv_kernel.h, FL) of the training step: the 16x16x32 form on its (3, 2) register tile.
// Pair-input data gradients with the BatchNorm-backward statistics (mask recomputed from the raw tensor), with the masked shortcut
// add + the statistics by sign bits, with the masked add alone.  Its forward form sits at its 256-register bound: its variants
// spill 10 registers - generic instantiation unless SPK_FL_FWD_PIPE is defined (A/B builds).  The 32x32x16 form has none: the
// stride-2 forward of the last downsample block on (1, 4) measured 251.1 us as a variant against 251.4 us generic.  Anything
// else (eval-mode epilogues, activation tensors as masks): generic.
constexpr int FLP_DGRAD_BN = SPK_IN_PRESPLIT | SPK_EPI_STATS | SPK_EPI_BNBWD;
constexpr int FLP_DGRAD_ADD_BN = SPK_IN_PRESPLIT | SPK_EPI_ADD | SPK_EPI_STATS | SPK_EPI_BNBWD | SPK_FL_ADDMASK | SPK_FL_BNMASK;
constexpr int FLP_DGRAD_ADD = SPK_IN_PRESPLIT | SPK_EPI_ADD | SPK_FL_ADDMASK;
constexpr int FLP_FWD_AFF = SPK_IN_AFFINE_RELU | SPK_EPI_STATS;
constexpr int FLP_FWD = SPK_EPI_STATS;

static constexpr bool pipe_has_fl(int MT, int NT, bool m16, int fl) {
    if (!m16 || !(MT == 3 && NT == 2)) return false;
#ifdef SPK_FL_FWD_PIPE
    if (fl == FLP_FWD_AFF || fl == FLP_FWD) return true;
#endif
    return fl == FLP_DGRAD_BN || fl == FLP_DGRAD_ADD_BN || fl == FLP_DGRAD_ADD;
}

int spk_pipe_variant_of(int MT, int NT, int flags, int ptrs) {
#ifdef SPK_NO_FL_VARIANTS
    return -1;
#else
    if (!spk_fl_variants_enabled() || (flags & (SPK_EPI_WMASK | SPK_IN_BNBWD)) || (ptrs & SPK_PTR_BN_ACT)) return -1;
    const bool m16 = (flags & SPK_CONV_M16) != 0;
    const int fl = (flags & ~SPK_CONV_M16) | ((ptrs & SPK_PTR_ADD_MASK) ? SPK_FL_ADDMASK : 0) | ((ptrs & SPK_PTR_BN_MASK) ? SPK_FL_BNMASK : 0);
    return pipe_has_fl(MT, NT, m16, fl) ? fl : -1;
#endif
}

// the instance the selection names (false: it names a word without an instance here - an error, never the generic kernel)
template <int MT, int NT>
static bool launch_pipe_fl(int fl, const ConvArgs& b, size_t lds_bytes, hipStream_t st) {
#ifndef SPK_NO_FL_VARIANTS
#define FL_CASE(V)                                                                                                         \
    case V:                                                                                                                \
        if constexpr (pipe_has_fl(MT, NT, true, V)) {                                                                      \
            hipLaunchKernelGGL((conv_pipe_kernel<MT, NT, false, false, ((V) & SPK_IN_PRESPLIT) != 0, true, V>), dim3(b.nblocks), \
                               dim3(256), lds_bytes, st, b);                                                               \
            return true;                                                                                                   \
        }                                                                                                                  \
        break;
    switch (fl) {
        FL_CASE(FLP_FWD_AFF)
        FL_CASE(FLP_FWD)
        FL_CASE(FLP_DGRAD_BN)
        FL_CASE(FLP_DGRAD_ADD_BN)
        FL_CASE(FLP_DGRAD_ADD)
    }
#undef FL_CASE
#endif
    return false;
}

template <int MT, int NT>
static int launch_pipe(const ConvArgs& a, size_t lds_bytes, hipStream_t st) {
    const int fl = spk_pipe_variant_of(MT, NT, a.flags, conv_ptr_pattern(a));
    if (a.flags & SPK_IN_BNBWD) {
#ifndef SPK_EXPERIMENTAL
        spk_set_error("spk_conv_mfma: the pipelined fused-BatchNorm-backward kernel is an experimental form: build with SPK_EXPERIMENTAL=1");
        return -1;
#else
        // fused BatchNorm backward: the sign-bit form only (the form that recomputes the mask from the raw tensor has more
        // VALU work per item than a tap has MFMA shadow and measured slower than conv_mfma_kernel), register tiles <= 2 x 2
        if constexpr (MT * NT <= 4) {
            SPK_REQUIRE(a.in_mask, "spk_conv_mfma: the pipelined fused-BatchNorm-backward kernel takes the ReLU mask as sign bits");
            hipLaunchKernelGGL((conv_pipe_kernel<MT, NT, true, true>), dim3(a.nblocks), dim3(256), lds_bytes, st, a);
        } else {
            spk_set_error("spk_conv_mfma: no pipelined fused-BatchNorm-backward kernel for MT=%d NT=%d", MT, NT);
            return -1;
        }
#endif
    } else if (a.flags & SPK_CONV_M16) {         // 16x16x32 matrix instruction, taps paired (conv_kernel.h, M16)
        ConvArgs b = a;
        b.flags = a.flags & ~SPK_CONV_M16;
        if constexpr (MT == 3 && NT == 2) {
#define LP(PREV, VV) hipLaunchKernelGGL((conv_pipe_kernel<MT, NT, false, false, PREV, true, VV>), dim3(a.nblocks), dim3(256), lds_bytes, st, b)
            if (b.flags & SPK_EPI_WMASK) {     // length-masked eval forward (plain input)
                LP(false, SPK_EPI_WMASK);
            } else if (fl >= 0) {
                if (!launch_pipe_fl<MT, NT>(fl, b, lds_bytes, st)) {
                    spk_set_error("spk_conv_mfma: no instance of flag variant 0x%x of the 16x16x32 pipelined kernel", fl);
                    return -1;
                }
            } else if (a.flags & SPK_IN_PRESPLIT) {
                LP(true, -1);
            } else {
                LP(false, -1);
            }
#undef LP
        } else {
            spk_set_error("spk_conv_mfma: no 16x16x32 pipelined kernel for MT=%d NT=%d", MT, NT);
            return -1;
        }
    } else if (a.flags & SPK_EPI_WMASK) {        // length-masked eval forward (conv_kernel.h, WM)
        hipLaunchKernelGGL((conv_pipe_kernel<MT, NT, false, false, false, false, SPK_EPI_WMASK>), dim3(a.nblocks), dim3(256), lds_bytes, st, a);
    } else if (a.flags & SPK_IN_PRESPLIT) {      // f16 pair input: staging by plain copy
        hipLaunchKernelGGL((conv_pipe_kernel<MT, NT, false, false, true>), dim3(a.nblocks), dim3(256), lds_bytes, st, a);
    } else {
        hipLaunchKernelGGL((conv_pipe_kernel<MT, NT, false>), dim3(a.nblocks), dim3(256), lds_bytes, st, a);
    }
    SPK_LAUNCH_CHECK("spk_conv_mfma(pipe)");
    return 0;
}

int spk_launch_conv_pipe(const ConvArgs& a, size_t lds_bytes, int MT, int NT, hipStream_t st) {
#define CASE(M, N) if (MT == M && NT == N) return launch_pipe<M, N>(a, lds_bytes, st);
    CASE(2, 1) CASE(3, 1) CASE(1, 2) CASE(2, 2) CASE(3, 2) CASE(1, 4)
#undef CASE
    spk_set_error("spk_conv_mfma: unsupported pipelined tile config MT=%d NT=%d", MT, NT);
    return -1;
}

#ifdef CONV_STAMPS
extern "C" int spk_debug_stamps_pipe(unsigned long long* out, int nblocks) {     // diagnostic builds only (never in the in-tree library)
    if (nblocks < 0) {        // reset
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_conv_stamps)) != hipSuccess) return -1;
        return (int)hipMemset(p, 0, sizeof(unsigned long long) * 16 * CONV_STAMP_BLOCKS);
    }
    if (nblocks > CONV_STAMP_BLOCKS) nblocks = CONV_STAMP_BLOCKS;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_conv_stamps), (size_t)nblocks * 16 * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif
