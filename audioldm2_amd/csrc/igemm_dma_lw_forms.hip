// igemm_dma_lw_forms.hip — the loader-wave DMA-fed GEMM (igemm_dma_lw.h) with a compile-time epilogue form (igemm_epilogue.h,
// ALDM_EPI_FORM_*), in a translation unit of its own so that it compiles next to igemm_dma_lw.hip.  3-part bf16 images (the
// default "bf16x6" mode), the 64- and 128-row tiles with 64 columns and the 64-row tile with 128: their MMA waves hold at most two
// 32x32 slabs, so the optional operand of every slab fits the registers (32 VGPRs at most) on top of the K loop's.  The 128x128
// tile runs two waves per SIMD at 229 of its 256 registers before any prefetch: it stays on the generic epilogue, like the 128x64
// tile on the 2-deep ring (see igemm_dma_lw_form_ok) and the 2-part and fp16 instantiations.  Registers, scratch and occupancy of
// every instantiation, before and after: profiles/r10_epilogue_forms_registers.txt.
#include "igemm_dma_lw.h"

namespace aldm {

int igemm_dma_lw_env_bpc();   // igemm_dma_lw.hip: $ALDM_LW_BPC

bool igemm_dma_lw_form_ok(int BM, int BN, int nst, int parts) {
    if (parts != 3 || igemm_dma_lw_env_bpc() == 1) return false;   // (the one-block-per-CU A/B runs the generic kernels)
    if (BM == 64 && BN == 128) return nst == 2 || nst == 4;
    // (128x64 on the 2-deep ring is budgeted for two blocks per CU at 128 registers and already spills in its generic form: the
    //  prefetched quads of its residual / row-bias forms would add 12 bytes of scratch per lane — the whole tile stays generic)
    if (BM == 128 && BN == 64) return nst == 4;
    if (BM == 64 && BN == 64) return nst == 2 || nst == 3;
    return false;
}

template <int BM, int BN, int NST>
static int launch_forms(int form, dim3 grid, hipStream_t st, const IgemmK& p) {
    // blocks per CU as igemm_launch_dma_lw budgets them
    constexpr int BPC = (160 * 1024) / dma_lds_bytes(BM, BN, NST, 3) >= 2 ? 2 : 1;
    switch (form) {
        case ALDM_EPI_FORM_PLAIN:
            hipLaunchKernelGGL((igemm_dma_lw_kernel<BM, BN, NST, 2, 3, BPC, false, ALDM_EPI_FORM_PLAIN>), grid, dim3(512), 0, st, p);
            return 0;
        case ALDM_EPI_FORM_ROWBIAS:
            hipLaunchKernelGGL((igemm_dma_lw_kernel<BM, BN, NST, 2, 3, BPC, false, ALDM_EPI_FORM_ROWBIAS>), grid, dim3(512), 0, st, p);
            return 0;
        case ALDM_EPI_FORM_RES:
            hipLaunchKernelGGL((igemm_dma_lw_kernel<BM, BN, NST, 2, 3, BPC, false, ALDM_EPI_FORM_RES>), grid, dim3(512), 0, st, p);
            return 0;
    }
    return -1;
}

int igemm_launch_dma_lw_form(int BM, int BN, int nst, int form, dim3 grid, hipStream_t st, const IgemmK& p) {
    if (BM == 64 && BN == 64 && nst == 2) return launch_forms<64, 64, 2>(form, grid, st, p);
    if (BM == 64 && BN == 64 && nst == 3) return launch_forms<64, 64, 3>(form, grid, st, p);
    if (BM == 128 && BN == 64 && nst == 4) return launch_forms<128, 64, 4>(form, grid, st, p);
    if (BM == 64 && BN == 128 && nst == 2) return launch_forms<64, 128, 2>(form, grid, st, p);
    if (BM == 64 && BN == 128 && nst == 4) return launch_forms<64, 128, 4>(form, grid, st, p);
    return -1;
}

}  // namespace aldm
