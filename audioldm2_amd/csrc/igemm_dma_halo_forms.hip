// igemm_dma_halo_forms.hip — the halo-patch 3x3 convolution kernel (igemm_dma_halo.h) with a compile-time epilogue form
// (igemm_epilogue.h, ALDM_EPI_FORM_*), in a translation unit of its own.  The 128x128 tile on 3-part bf16 images with the patch
// of the UNet's levels (MAXCH = 10) and the two (ring, waves) pairs the tuned tables use: on 4 waves a wave owns four slabs and
// runs alone on its SIMD (512 registers: 128 for the prefetched quads), on 8 waves two slabs at 256 registers (64 for the quads).
// The 256x128 tile holds four slabs per wave at two waves per SIMD — 224 of 256 registers before any prefetch: generic epilogue.
#include "igemm_dma_halo.h"

namespace aldm {

bool igemm_dma_halo_form_ok(int BM, int BN, int nstb, int wm, int parts, int maxch) {
    if (parts != 3 || BM != 128 || BN != 128 || maxch != 10) return false;
    return (nstb == 4 && wm == 2) || (nstb == 2 && wm == 4);
}

template <int NSTB, int WM>
static int launch_forms(int form, dim3 grid, hipStream_t st, const IgemmK& p) {
    switch (form) {
        case ALDM_EPI_FORM_PLAIN:
            hipLaunchKernelGGL((igemm_dma_halo_kernel<128, 128, NSTB, WM, 3, 10, false, ALDM_EPI_FORM_PLAIN>), grid, dim3(128 * WM), 0, st, p);
            return 0;
        case ALDM_EPI_FORM_ROWBIAS:
            hipLaunchKernelGGL((igemm_dma_halo_kernel<128, 128, NSTB, WM, 3, 10, false, ALDM_EPI_FORM_ROWBIAS>), grid, dim3(128 * WM), 0, st, p);
            return 0;
        case ALDM_EPI_FORM_RES:
            hipLaunchKernelGGL((igemm_dma_halo_kernel<128, 128, NSTB, WM, 3, 10, false, ALDM_EPI_FORM_RES>), grid, dim3(128 * WM), 0, st, p);
            return 0;
    }
    return -1;
}

int igemm_launch_dma_halo_form(int BM, int BN, int nstb, int wm, int maxch, int form, dim3 grid, hipStream_t st, const IgemmK& p) {
    if (BM != 128 || BN != 128 || maxch != 10) return -1;
    if (nstb == 4 && wm == 2) return launch_forms<4, 2>(form, grid, st, p);
    if (nstb == 2 && wm == 4) return launch_forms<2, 4>(form, grid, st, p);
    return -1;
}

}  // namespace aldm
