// The chroma half of mf_crop_resize_dev_nv16: resize_uv422.hip's launch from a rectangle that stays on the device, the way resize_uv_dev.hip
// does it for NV12 -- resize_uv422_body.h compiled a second time under MF_RESIZE_DEV (resize_rect.h) and other names: the rectangle is loaded
// instead of passed, everything else is the same code.  A rectangle that cannot be used (empty, negative, outside the frame): both kernels
// return at once; the luma tables kernel in front of them has added 1 to *d_status.
#define MF_RESIZE_DEV 1
#define uv422_tables_kernel uv422_tables_rect_kernel
#define uv422_resize_kernel uv422_resize_rect_kernel
#include "resize_uv422_body.h"

namespace mf {

int launch_resize_uv422_dev(const uint8_t* uv, uint8_t* out_uv, int W, int H, const int32_t* d_bounds, int oW, int oH, const void* luma_ytab,
                            void* tabs, const TileOrder& order, hipStream_t st)
{
    ResizeTab* xtab = (ResizeTab*)tabs;
    hipLaunchKernelGGL(uv422_tables_kernel, dim3((oW / 2 + 255) / 256), dim3(256), 0, st, d_bounds, W, H, oW, xtab);
    if (const int rc = hip_fail(hipGetLastError(), "uv422_tables_rect_kernel launch")) return rc;
    hipLaunchKernelGGL(uv422_resize_kernel, dim3(order.per_xcd * 8u), dim3(64 * kWaves), 0, st, uv, out_uv, W, H, d_bounds, oW, oH, xtab,
                       (const ResizeTab*)luma_ytab, order);
    return hip_fail(hipGetLastError(), "uv422_resize_rect_kernel launch");
}

}  // namespace mf
