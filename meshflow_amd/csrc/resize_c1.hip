// mf_crop_resize_u8c1's kernel launch (resize_c1_body.h) behind resize.hip's checks and tables.
#include "resize_c1_body.h"

namespace mf {

// launch_crop_resize's launch for single-channel frames (checks done and resize.hip's tables built there)
int launch_resize8c1(const uint8_t* frames, uint8_t* out, int n, int W, int H, int left, int top, int cw, const void* work,
                     const TileOrder& order, hipStream_t st)
{
    const ResizeTab* xtab = (const ResizeTab*)work;
    const ResizeTab* ytab = xtab + W;
    hipLaunchKernelGGL(resize8c1_kernel, dim3(order.per_xcd * 8u), dim3(64 * kWaves), 0, st, frames, out, n, W, H, left, top, cw, xtab, ytab,
                       order);
    return hip_fail(hipGetLastError(), "resize8c1_kernel launch");
}

}  // namespace mf
