// The host side of the chroma half of mf_crop_resize_nv16 (rectangle known to the host): resize_uv422_body.h's x tables in `tabs`, then its
// kernel on them and on the luma call's y table.  The checks of the call are capi.hip's (they come before the luma launch); the tile order and
// the workspace layout both NV16 calls share are defined here, next to the kernel's tile constants.
#include "resize_uv422_body.h"

namespace mf {

// luma tables (mf_crop_resize_workspace_bytes), then the chroma x table: oW/2 entries (the y axis is the luma table's)
size_t crop_resize_nv16_workspace_bytes(int oW, int oH)
{
    return crop_resize_workspace_bytes(oW, oH) + (size_t)(oW / 2) * sizeof(ResizeTab);
}

// tiles: 256 chroma samples of kWaves * kUv422Rows output rows, over all oH rows
bool resize_uv422_tile_order(int oW, int oH, int n, TileOrder& order)
{
    const int rows = kWaves * kUv422Rows;
    return make_tile_order((oW / 2 + 255) / 256, (oH + rows - 1) / rows, n, order);
}

int launch_resize_uv422(const uint8_t* uv, uint8_t* out_uv, int W, int H, int left, int top, int right, int bottom, int oW, int oH,
                        const void* luma_ytab, void* tabs, const TileOrder& order, hipStream_t st)
{
    ResizeTab* xtab = (ResizeTab*)tabs;
    hipLaunchKernelGGL(uv422_tables_kernel, dim3((oW / 2 + 255) / 256), dim3(256), 0, st, left, top, right, bottom, oW, xtab);
    if (const int rc = hip_fail(hipGetLastError(), "uv422_tables_kernel launch")) return rc;
    hipLaunchKernelGGL(uv422_resize_kernel, dim3(order.per_xcd * 8u), dim3(64 * kWaves), 0, st, uv, out_uv, W, H, left, top, right - left + 1,
                       oW, oH, xtab, (const ResizeTab*)luma_ytab, order);
    return hip_fail(hipGetLastError(), "uv422_resize_kernel launch");
}

}  // namespace mf
