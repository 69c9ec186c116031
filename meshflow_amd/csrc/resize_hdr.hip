// The host side of mf_crop_resize_p010 (rectangle known to the host): resize16.hip's luma tables, resize_hdr_body.h's luma kernel, then its chroma
// tables in `tabs` and its chroma kernel.  The checks of the call are capi.hip's (they come before the first launch); the tile orders and the
// workspace layout both P010 calls share are defined here, next to the kernels' tile constants.
// mf_crop_resize_p210 (10-bit 4:2:2) lives here too: the same luma tables and luma kernel, then resize_wide422_body.h's x table and its chroma
// kernel on the luma call's own y table.
#include "resize_wide422_body.h"

namespace mf {

// luma tables (mf_crop_resize_workspace_bytes), then the chroma tables: oW/2 x-entries and oH/2 y-entries
size_t crop_resize_p010_workspace_bytes(int oW, int oH)
{
    return crop_resize_workspace_bytes(oW, oH) + (size_t)(oW / 2 + oH / 2) * sizeof(Resize16Tab);
}

// tiles: 256 samples of kWaves * kHdrRows output rows, of the luma plane and of the chroma plane
bool resize_hdr_tile_orders(int oW, int oH, int n, TileOrder& luma, TileOrder& chroma)
{
    const int rows = kWaves * kHdrRows;
    return make_tile_order((oW + 255) / 256, (oH + rows - 1) / rows, n, luma) &&
           make_tile_order((oW / 2 + 255) / 256, (oH / 2 + rows - 1) / rows, n, chroma);
}

int launch_resize_hdr(const uint16_t* y, const uint16_t* uv, uint16_t* out_y, uint16_t* out_uv, int W, int H, int left, int top, int right,
                      int bottom, int oW, int oH, void* work, const TileOrder& luma, const TileOrder& chroma, hipStream_t st)
{
    const int cw = right - left + 1, ch = bottom - top + 1;
    if (const int rc = launch_resize16_tables(cw, ch, oW, oH, work, st)) return rc;
    const Resize16Tab* lx = (const Resize16Tab*)work;
    hipLaunchKernelGGL(hdr_luma_resize_kernel, dim3(luma.per_xcd * 8u), dim3(64 * kWaves), 0, st, y, out_y, W, H, left, top, cw, oW, oH,
                       2 * oW == cw && 2 * oH == ch, lx, lx + oW, luma);
    if (const int rc = hip_fail(hipGetLastError(), "hdr_luma_resize_kernel launch")) return rc;
    Resize16Tab* xtab = (Resize16Tab*)((char*)work + crop_resize_workspace_bytes(oW, oH));
    Resize16Tab* ytab = xtab + oW / 2;
    const int m = (oW > oH ? oW : oH) / 2;
    hipLaunchKernelGGL(hdr_uv_tables_kernel, dim3((m + 255) / 256), dim3(256), 0, st, left, top, right, bottom, oW, oH, xtab, ytab);
    if (const int rc = hip_fail(hipGetLastError(), "hdr_uv_tables_kernel launch")) return rc;
    hipLaunchKernelGGL(hdr_uv_resize_kernel, dim3(chroma.per_xcd * 8u), dim3(64 * kWaves), 0, st, uv, out_uv, W, H, left, top, cw, oW, oH, xtab,
                       ytab, chroma);
    return hip_fail(hipGetLastError(), "hdr_uv_resize_kernel launch");
}

// luma tables (mf_crop_resize_workspace_bytes), then the chroma x table: oW/2 entries (the y axis is the luma table's)
size_t crop_resize_p210_workspace_bytes(int oW, int oH)
{
    return crop_resize_workspace_bytes(oW, oH) + (size_t)(oW / 2) * sizeof(Resize16Tab);
}

// tiles: 256 samples of kWaves * kHdrRows output rows, of the luma plane and of the chroma plane -- (oW / 2, oH): chroma has luma's rows
bool resize_p210_tile_orders(int oW, int oH, int n, TileOrder& luma, TileOrder& chroma)
{
    const int rows = kWaves * kHdrRows;
    return make_tile_order((oW + 255) / 256, (oH + rows - 1) / rows, n, luma) &&
           make_tile_order((oW / 2 + 255) / 256, (oH + rows - 1) / rows, n, chroma);
}

int launch_resize_p210(const uint16_t* y, const uint16_t* uv, uint16_t* out_y, uint16_t* out_uv, int W, int H, int left, int top, int right,
                       int bottom, int oW, int oH, void* work, const TileOrder& luma, const TileOrder& chroma, hipStream_t st)
{
    const int cw = right - left + 1, ch = bottom - top + 1;
    if (const int rc = launch_resize16_tables(cw, ch, oW, oH, work, st)) return rc;
    const Resize16Tab* lx = (const Resize16Tab*)work;
    hipLaunchKernelGGL(hdr_luma_resize_kernel, dim3(luma.per_xcd * 8u), dim3(64 * kWaves), 0, st, y, out_y, W, H, left, top, cw, oW, oH,
                       2 * oW == cw && 2 * oH == ch, lx, lx + oW, luma);
    if (const int rc = hip_fail(hipGetLastError(), "hdr_luma_resize_kernel launch")) return rc;
    Resize16Tab* xtab = (Resize16Tab*)((char*)work + crop_resize_workspace_bytes(oW, oH));
    hipLaunchKernelGGL(wide422_tables_kernel, dim3((oW / 2 + 255) / 256), dim3(256), 0, st, left, top, right, bottom, oW, xtab);
    if (const int rc = hip_fail(hipGetLastError(), "wide422_tables_kernel launch")) return rc;
    hipLaunchKernelGGL(wide422_resize_kernel, dim3(chroma.per_xcd * 8u), dim3(64 * kWaves), 0, st, uv, out_uv, W, H, left, top, cw, oW, oH, xtab,
                       lx + oW, chroma);                           // (the chroma area branch does not exist: the float path on the luma y table)
    return hip_fail(hipGetLastError(), "wide422_resize_kernel launch");
}

}  // namespace mf
