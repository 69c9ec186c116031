// mf_crop_resize_dev_u8c1's same-size kernel: resize_c1.hip's resize8c1_kernel with the rectangle read from device memory (resize_rect.h,
// resize_dev.hip).  A translation unit of its own because resize_c1.hip keeps its own copies of resize_u8.h's helpers.
#define MF_RESIZE_DEV 1
#define resize8c1_kernel resize8c1_dev_kernel
#include "resize_c1.hip"

namespace mf {

int launch_resize8c1_dev(const uint8_t* frames, uint8_t* out, int n, int W, int H, const int32_t* d_bounds, const ResizeTab* xtab,
                         const ResizeTab* ytab, const TileOrder& order, hipStream_t st)
{
    hipLaunchKernelGGL(resize8c1_kernel, dim3(order.per_xcd * 8u), dim3(64 * kWaves), 0, st, frames, out, n, W, H, d_bounds, xtab, ytab, order);
    return hip_fail(hipGetLastError(), "resize8c1_dev_kernel launch");
}

}  // namespace mf
