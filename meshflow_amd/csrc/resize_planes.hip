// The host side of mf_crop_resize_plane_f32 / mf_crop_resize_plane_nearest (rectangle known to the host): every check of the call
// (resize_checks.h), resize_planes_body.h's tables in `work`, then its kernel.
#include "resize_planes_body.h"
#include "resize_checks.h"

namespace mf {

int launch_crop_resize_plane(int elem_bytes, const void* planes, void* out, int n, int W, int H, int left, int top, int right, int bottom,
                             int oW, int oH, void* work, hipStream_t st)
{
    const char* const call = "mf_crop_resize_";
    const char* name = elem_bytes ? "plane_nearest" : "plane_f32";
    if (!resize_shape_ok(call, name, n, W, H) || !resize_out_size_ok(call, name, oW, oH) ||
        !resize_rect_ok(call, name, left, top, right, bottom, W, H))
        return MF_ERR_INVALID_ARG;
    TileOrder order;                                                // tiles: 256 output pixels of one row
    if (!resize_tiles_ok(call, name, oW, oH, 1, n, order)) return MF_ERR_INVALID_ARG;
    const int cw = right - left + 1, ch = bottom - top + 1;
    const double scale_x = 1.0 / ((double)oW / (double)cw), scale_y = 1.0 / ((double)oH / (double)ch);
    Resize16Tab* xtab = (Resize16Tab*)work;
    Resize16Tab* ytab = xtab + oW;
    const dim3 tab_grid(((oW > oH ? oW : oH) + 255) / 256), grid(order.per_xcd * 8u), block(256);
    hipLaunchKernelGGL(plane_resize_tables, tab_grid, block, 0, st, cw, ch, oW, oH, scale_x, scale_y, elem_bytes, xtab, ytab);
    if (const int rc = hip_fail(hipGetLastError(), "plane_resize_tables launch")) return rc;
    switch (elem_bytes) {
    case 0:
        hipLaunchKernelGGL(plane_resize_f32, grid, block, 0, st, (const float*)planes, (float*)out, W, H, left, top, cw, oW, oH,
                           plane_f32_path(cw, ch, oW, oH), xtab, ytab, order);
        break;
    case 1:
        hipLaunchKernelGGL(plane_resize_nearest<uint8_t>, grid, block, 0, st, (const uint8_t*)planes, (uint8_t*)out, W, H, left, top, cw, oW, oH,
                           xtab, ytab, order);
        break;
    case 2:
        hipLaunchKernelGGL(plane_resize_nearest<uint16_t>, grid, block, 0, st, (const uint16_t*)planes, (uint16_t*)out, W, H, left, top, cw, oW, oH,
                           xtab, ytab, order);
        break;
    case 4:
        hipLaunchKernelGGL(plane_resize_nearest<uint32_t>, grid, block, 0, st, (const uint32_t*)planes, (uint32_t*)out, W, H, left, top, cw, oW, oH,
                           xtab, ytab, order);
        break;
    default:
        hipLaunchKernelGGL(plane_resize_nearest<uint64_t>, grid, block, 0, st, (const uint64_t*)planes, (uint64_t*)out, W, H, left, top, cw, oW, oH,
                           xtab, ytab, order);
        break;
    }
    return hip_fail(hipGetLastError(), elem_bytes ? "plane_resize_nearest launch" : "plane_resize_f32 launch");
}

}  // namespace mf
