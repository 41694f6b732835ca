// igemm_dma_forms.hip — the classic DMA-fed GEMM (igemm_dma.h) with a compile-time epilogue form (igemm_epilogue.h,
// ALDM_EPI_FORM_*), in a translation unit of its own so that it compiles next to igemm_dma.hip.  3-part bf16 images (the default
// "bf16x6" mode) on the tiles whose waves hold at most two 32x32 slabs (64x64, 64x128, 128x64: two blocks per CU at 256 registers
// per wave, the prefetched quads take 32 at most).  The 128x128 and 256x128 tiles (four slabs per wave) stay on the generic
// epilogue, like the 2-part and fp16 instantiations.
#include "igemm_dma.h"

namespace aldm {

bool igemm_dma_form_ok(int BM, int BN, int nst, int parts) {
    if (parts != 3) return false;
    if ((BM == 64 && BN == 128) || (BM == 128 && BN == 64)) return nst == 2 || nst == 4;
    if (BM == 64 && BN == 64) return nst == 2 || nst == 3;
    return false;
}

template <int BM, int BN, int NST>
static int launch_forms(int form, dim3 grid, hipStream_t st, const IgemmK& p) {
    switch (form) {
        case ALDM_EPI_FORM_PLAIN:
            hipLaunchKernelGGL((igemm_dma_kernel<BM, BN, NST, 2, 3, false, false, ALDM_EPI_FORM_PLAIN>), grid, dim3(256), 0, st, p);
            return 0;
        case ALDM_EPI_FORM_ROWBIAS:
            hipLaunchKernelGGL((igemm_dma_kernel<BM, BN, NST, 2, 3, false, false, ALDM_EPI_FORM_ROWBIAS>), grid, dim3(256), 0, st, p);
            return 0;
        case ALDM_EPI_FORM_RES:
            hipLaunchKernelGGL((igemm_dma_kernel<BM, BN, NST, 2, 3, false, false, ALDM_EPI_FORM_RES>), grid, dim3(256), 0, st, p);
            return 0;
    }
    return -1;
}

int igemm_launch_dma_form(int BM, int BN, int nst, int form, dim3 grid, hipStream_t st, const IgemmK& p) {
    if (BM == 64 && BN == 64 && nst == 2) return launch_forms<64, 64, 2>(form, grid, st, p);
    if (BM == 64 && BN == 64 && nst == 3) return launch_forms<64, 64, 3>(form, grid, st, p);
    if (BM == 128 && BN == 64 && nst == 2) return launch_forms<128, 64, 2>(form, grid, st, p);
    if (BM == 128 && BN == 64 && nst == 4) return launch_forms<128, 64, 4>(form, grid, st, p);
    if (BM == 64 && BN == 128 && nst == 2) return launch_forms<64, 128, 2>(form, grid, st, p);
    if (BM == 64 && BN == 128 && nst == 4) return launch_forms<64, 128, 4>(form, grid, st, p);
    return -1;
}

}  // namespace aldm
