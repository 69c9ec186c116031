// The chroma half of mf_crop_resize_dev_nv12: resize_uv.hip's launch from a rectangle that stays on the device, the way resize_dev.hip does it
// for the pixel formats -- resize_uv_body.h compiled a second time under MF_RESIZE_DEV (resize_rect.h) and other names: the rectangle is loaded
// instead of passed, everything else is the same code.  A rectangle that cannot be used (empty, negative, outside the frame): both kernels
// return at once; the luma tables kernel in front of them has added 1 to *d_status.
#define MF_RESIZE_DEV 1
#define chroma_tables_kernel chroma_tables_rect_kernel
#define chroma_resize_kernel chroma_resize_rect_kernel
#include "resize_uv_body.h"

namespace mf {

int launch_resize_uv_dev(const uint8_t* uv, uint8_t* out_uv, int W, int H, const int32_t* d_bounds, int oW, int oH, void* tabs,
                         const TileOrder& order, hipStream_t st)
{
    ResizeTab* xtab = (ResizeTab*)tabs;
    ResizeTab* ytab = xtab + oW / 2;
    const int m = (oW > oH ? oW : oH) / 2;
    hipLaunchKernelGGL(chroma_tables_kernel, dim3((m + 255) / 256), dim3(256), 0, st, d_bounds, W, H, oW, oH, xtab, ytab);
    if (const int rc = hip_fail(hipGetLastError(), "chroma_tables_rect_kernel launch")) return rc;
    hipLaunchKernelGGL(chroma_resize_kernel, dim3(order.per_xcd * 8u), dim3(64 * kWaves), 0, st, uv, out_uv, W, H, d_bounds, oW, oH, xtab, ytab,
                       order);
    return hip_fail(hipGetLastError(), "chroma_resize_rect_kernel launch");
}

}  // namespace mf
