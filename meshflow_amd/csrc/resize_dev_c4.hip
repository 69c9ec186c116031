// mf_crop_resize_dev_u8c4's kernels: resize_c4.hip's resize8c4_kernel with the rectangle read from device memory (resize_rect.h,
// resize_dev.hip).  `up`: oW >= W and oH >= H, an upscale whatever the rectangle; otherwise the down instantiation, valid at every scale.
#define MF_RESIZE_DEV 1
#define resize8c4_kernel resize_bgra_dev_kernel
#include "resize_c4.hip"

namespace mf {

int launch_resize8c4_dev(const uint8_t* frames, uint8_t* out, int n, int W, int H, const int32_t* d_bounds, int oW, int oH, bool up,
                         const ResizeTab* xtab, const ResizeTab* ytab, const TileOrder& order, hipStream_t st)
{
    const dim3 grid(order.per_xcd * 8u), block(64 * kWaves);
    if (up)
        hipLaunchKernelGGL((resize8c4_kernel<kUpRows, kUpSlots, kUpPitch, false>), grid, block, 0, st, frames, out, n, W, H, d_bounds, oW, oH, xtab,
                           ytab, order);
    else
        hipLaunchKernelGGL((resize8c4_kernel<kDownRows, 2 * kDownRows, kDownPitch, true>), grid, block, 0, st, frames, out, n, W, H, d_bounds, oW,
                           oH, xtab, ytab, order);
    return hip_fail(hipGetLastError(), "resize_bgra_dev_kernel launch");
}

}  // namespace mf
