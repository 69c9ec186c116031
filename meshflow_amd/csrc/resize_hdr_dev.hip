// mf_crop_resize_dev_p010: resize_hdr.hip's launches from a rectangle that stays on the device, the way resize_uv_dev.hip does it for NV12's
// chroma -- resize_hdr_body.h compiled a second time under MF_RESIZE_DEV (resize_rect.h) and other names: the rectangle is loaded instead of
// passed, everything else is the same code.  A rectangle that cannot be used (empty, negative, outside the frame): all three kernels return at
// once; the luma tables kernel in front of them (resize_dev.hip's) has added 1 to *d_status.
#define MF_RESIZE_DEV 1
#define hdr_luma_resize_kernel hdr_luma_resize_rect_kernel
#define hdr_uv_tables_kernel hdr_uv_tables_rect_kernel
#define hdr_uv_resize_kernel hdr_uv_resize_rect_kernel
// ... and mf_crop_resize_dev_p210's two chroma kernels (resize_wide422_body.h, which includes resize_hdr_body.h), the same way
#define wide422_tables_kernel wide422_tables_rect_kernel
#define wide422_resize_kernel wide422_resize_rect_kernel
#include "resize_wide422_body.h"

namespace mf {

int launch_resize_hdr_dev(const uint16_t* y, const uint16_t* uv, uint16_t* out_y, uint16_t* out_uv, int W, int H, const int32_t* d_bounds, int oW,
                          int oH, void* work, int32_t* d_status, const TileOrder& luma, const TileOrder& chroma, hipStream_t st)
{
    if (const int rc = launch_resize16_tables_dev(d_bounds, W, H, oW, oH, work, d_status, st)) return rc;
    const Resize16Tab* lx = (const Resize16Tab*)work;
    hipLaunchKernelGGL(hdr_luma_resize_kernel, dim3(luma.per_xcd * 8u), dim3(64 * kWaves), 0, st, y, out_y, W, H, d_bounds, oW, oH, lx, lx + oW,
                       luma);
    if (const int rc = hip_fail(hipGetLastError(), "hdr_luma_resize_rect_kernel launch")) return rc;
    Resize16Tab* xtab = (Resize16Tab*)((char*)work + crop_resize_workspace_bytes(oW, oH));
    Resize16Tab* ytab = xtab + oW / 2;
    const int m = (oW > oH ? oW : oH) / 2;
    hipLaunchKernelGGL(hdr_uv_tables_kernel, dim3((m + 255) / 256), dim3(256), 0, st, d_bounds, W, H, oW, oH, xtab, ytab);
    if (const int rc = hip_fail(hipGetLastError(), "hdr_uv_tables_rect_kernel launch")) return rc;
    hipLaunchKernelGGL(hdr_uv_resize_kernel, dim3(chroma.per_xcd * 8u), dim3(64 * kWaves), 0, st, uv, out_uv, W, H, d_bounds, oW, oH, xtab, ytab,
                       chroma);
    return hip_fail(hipGetLastError(), "hdr_uv_resize_rect_kernel launch");
}

int launch_resize_p210_dev(const uint16_t* y, const uint16_t* uv, uint16_t* out_y, uint16_t* out_uv, int W, int H, const int32_t* d_bounds, int oW,
                           int oH, void* work, int32_t* d_status, const TileOrder& luma, const TileOrder& chroma, hipStream_t st)
{
    if (const int rc = launch_resize16_tables_dev(d_bounds, W, H, oW, oH, work, d_status, st)) return rc;
    const Resize16Tab* lx = (const Resize16Tab*)work;
    hipLaunchKernelGGL(hdr_luma_resize_kernel, dim3(luma.per_xcd * 8u), dim3(64 * kWaves), 0, st, y, out_y, W, H, d_bounds, oW, oH, lx, lx + oW,
                       luma);
    if (const int rc = hip_fail(hipGetLastError(), "hdr_luma_resize_rect_kernel launch")) return rc;
    Resize16Tab* xtab = (Resize16Tab*)((char*)work + crop_resize_workspace_bytes(oW, oH));
    hipLaunchKernelGGL(wide422_tables_kernel, dim3((oW / 2 + 255) / 256), dim3(256), 0, st, d_bounds, W, H, oW, xtab);
    if (const int rc = hip_fail(hipGetLastError(), "wide422_tables_rect_kernel launch")) return rc;
    hipLaunchKernelGGL(wide422_resize_kernel, dim3(chroma.per_xcd * 8u), dim3(64 * kWaves), 0, st, uv, out_uv, W, H, d_bounds, oW, oH, xtab,
                       lx + oW, chroma);
    return hip_fail(hipGetLastError(), "wide422_resize_rect_kernel launch");
}

}  // namespace mf
