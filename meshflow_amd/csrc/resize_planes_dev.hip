// mf_crop_resize_dev_plane_f32 / mf_crop_resize_dev_plane_nearest: resize_planes.hip's call from a rectangle that stays on the device, the
// way resize_dev.hip does it for the pixel formats -- resize_planes_body.h compiled a second time under MF_RESIZE_DEV (resize_rect.h) and other
// names: the rectangle is loaded instead of passed, everything else is the same code.  A rectangle that cannot be used (empty, negative,
// outside the plane): every kernel returns at once and the tables kernel adds 1 to *d_status.
#define MF_RESIZE_DEV 1
#define plane_resize_tables plane_resize_tables_dev
#define plane_resize_f32 plane_resize_f32_dev
#define plane_resize_nearest plane_resize_nearest_dev
#include "resize_planes_body.h"
#include "resize_checks.h"

namespace mf {

int launch_crop_resize_plane_dev(int elem_bytes, const void* planes, void* out, int n, int W, int H, const int32_t* d_bounds, int oW, int oH,
                                 void* work, int32_t* d_status, hipStream_t st)
{
    const char* const call = "mf_crop_resize_dev_";
    const char* name = elem_bytes ? "plane_nearest" : "plane_f32";
    if (!resize_shape_ok(call, name, n, W, H) || !resize_out_size_ok(call, name, oW, oH)) return MF_ERR_INVALID_ARG;
    TileOrder order;                                                // tiles: 256 output pixels of one row
    if (!resize_tiles_ok(call, name, oW, oH, 1, n, order)) return MF_ERR_INVALID_ARG;
    Resize16Tab* xtab = (Resize16Tab*)work;
    Resize16Tab* ytab = xtab + oW;
    const dim3 tab_grid(((oW > oH ? oW : oH) + 255) / 256), grid(order.per_xcd * 8u), block(256);
    hipLaunchKernelGGL(plane_resize_tables, tab_grid, block, 0, st, d_bounds, W, H, oW, oH, d_status, elem_bytes, xtab, ytab);
    if (const int rc = hip_fail(hipGetLastError(), "plane_resize_tables_dev launch")) return rc;
    switch (elem_bytes) {
    case 0:
        hipLaunchKernelGGL(plane_resize_f32, grid, block, 0, st, (const float*)planes, (float*)out, W, H, d_bounds, oW, oH, xtab, ytab, order);
        break;
    case 1:
        hipLaunchKernelGGL(plane_resize_nearest<uint8_t>, grid, block, 0, st, (const uint8_t*)planes, (uint8_t*)out, W, H, d_bounds, oW, oH, xtab,
                           ytab, order);
        break;
    case 2:
        hipLaunchKernelGGL(plane_resize_nearest<uint16_t>, grid, block, 0, st, (const uint16_t*)planes, (uint16_t*)out, W, H, d_bounds, oW, oH,
                           xtab, ytab, order);
        break;
    case 4:
        hipLaunchKernelGGL(plane_resize_nearest<uint32_t>, grid, block, 0, st, (const uint32_t*)planes, (uint32_t*)out, W, H, d_bounds, oW, oH,
                           xtab, ytab, order);
        break;
    default:
        hipLaunchKernelGGL(plane_resize_nearest<uint64_t>, grid, block, 0, st, (const uint64_t*)planes, (uint64_t*)out, W, H, d_bounds, oW, oH,
                           xtab, ytab, order);
        break;
    }
    return hip_fail(hipGetLastError(), elem_bytes ? "plane_resize_nearest_dev launch" : "plane_resize_f32_dev launch");
}

}  // namespace mf
