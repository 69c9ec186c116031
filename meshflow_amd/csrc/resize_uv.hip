// The host side of the chroma half of mf_crop_resize_nv12 (rectangle known to the host): resize_uv_body.h's tables in `tabs`, then its kernel.
// The checks of the call are capi.hip's (they come before the luma launch); the tile order and the workspace layout both NV12 calls share are
// defined here, next to the kernel's tile constants.
#include "resize_uv_body.h"

namespace mf {

// luma tables (mf_crop_resize_workspace_bytes), then the chroma tables: oW/2 x-entries and oH/2 y-entries
size_t crop_resize_nv12_workspace_bytes(int oW, int oH)
{
    return crop_resize_workspace_bytes(oW, oH) + (size_t)(oW / 2 + oH / 2) * sizeof(ResizeTab);
}

// tiles: 256 chroma samples of kWaves * kUvRows output chroma rows
bool resize_uv_tile_order(int oW, int oH, int n, TileOrder& order)
{
    const int rows = kWaves * kUvRows;
    return make_tile_order((oW / 2 + 255) / 256, (oH / 2 + rows - 1) / rows, n, order);
}

int launch_resize_uv(const uint8_t* uv, uint8_t* out_uv, int W, int H, int left, int top, int right, int bottom, int oW, int oH, void* tabs,
                     const TileOrder& order, hipStream_t st)
{
    ResizeTab* xtab = (ResizeTab*)tabs;
    ResizeTab* ytab = xtab + oW / 2;
    const int m = (oW > oH ? oW : oH) / 2;
    hipLaunchKernelGGL(chroma_tables_kernel, dim3((m + 255) / 256), dim3(256), 0, st, left, top, right, bottom, oW, oH, xtab, ytab);
    if (const int rc = hip_fail(hipGetLastError(), "chroma_tables_kernel launch")) return rc;
    hipLaunchKernelGGL(chroma_resize_kernel, dim3(order.per_xcd * 8u), dim3(64 * kWaves), 0, st, uv, out_uv, W, H, left, top, right - left + 1,
                       oW, oH, xtab, ytab, order);
    return hip_fail(hipGetLastError(), "chroma_resize_kernel launch");
}

}  // namespace mf
