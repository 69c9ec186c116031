// _crop_frames (mfs.py:1111-1157) from a rectangle that stays on the device: mf_crop_resize_dev_u8c3 / _u16c3 / _u8c1 / _u8c4.  The rectangle
// {left, top, right, bottom} is the 16 bytes a warp's clip-level reduction left in device memory; the host never reads it, so these calls
// never wait for the warp.  The kernels are the four kernel headers' (resize_body.h, resize16_body.h, resize_c1_body.h, resize_c4_body.h)
// compiled a second time, under MF_RESIZE_DEV (resize_rect.h) and other names: the rectangle is loaded instead of passed,
// everything else is the same code.
//
// What the host still decides, from (W, H, oW, oH) alone:
//   oW >= W and oH >= H (the same-size call included): the crop lies inside the frame, so this is an upscale whatever the rectangle -- the
//       same-size kernels (oW x oH == W x H) or the `up` instantiations, the code the host-rectangle call runs;
//   anything else: the `down` instantiations, valid at every scale (each wavefront falls back to direct taps where its span does not fit).
//       The host-rectangle call may pick `up` (a small crop scaled up to less than the frame) or `direct` (a reduction beyond the staged
//       span) there; the bytes are the same, the cost is measured in profiles/resident_crop.md.
// A rectangle that cannot be used (empty, negative, outside the frame): every kernel returns at once and the tables kernel adds 1 to *d_status.
#define MF_RESIZE_DEV 1
#define resize_tables_kernel resize_tables_dev_kernel
#define resize_kernel resize_dev_kernel
#define resize16_tables_kernel resize16_tables_dev_kernel
#define resize16_kernel resize16_dev_kernel
#define resize_to_kernel resize_to_dev_kernel
#define resize8c1_to_kernel resize8c1_to_dev_kernel
#define resize16_to_kernel resize16_to_dev_kernel
#define resize8c1_kernel resize8c1_dev_kernel
#define resize8c4_kernel resize_bgra_dev_kernel
#include "resize_body.h"
#include "resize16_body.h"
#include "resize_c1_body.h"
#include "resize_c4_body.h"
#include "resize_checks.h"

namespace mf {

// resize16_tables_dev_kernel's tables for (oW, oH) in `work` (an unusable rectangle adds 1 to *d_status): launch_crop_resize_dev's uint16 tables,
// and the luma tables of mf_crop_resize_dev_p010 (resize_hdr_dev.hip)
int launch_resize16_tables_dev(const int32_t* d_bounds, int W, int H, int oW, int oH, void* work, int32_t* d_status, hipStream_t st)
{
    Resize16Tab* xtab = (Resize16Tab*)work;
    Resize16Tab* ytab = xtab + oW;
    hipLaunchKernelGGL(resize16_tables_kernel, dim3(((oW > oH ? oW : oH) + 255) / 256), dim3(256), 0, st, d_bounds, W, H, oW, oH, d_status, xtab,
                       ytab);
    return hip_fail(hipGetLastError(), "resize16_tables_dev_kernel launch");
}

int launch_crop_resize_dev(Px px, const void* frames, void* out, int n, int W, int H, const int32_t* d_bounds, int oW, int oH, void* work,
                           int32_t* d_status, hipStream_t st)
{
    const char* const call = "mf_crop_resize_dev_";
    const char* name = px_name(px);
    if (!resize_shape_ok(call, name, n, W, H) || !resize_out_size_ok(call, name, oW, oH)) return MF_ERR_INVALID_ARG;
    const bool up = oW >= W && oH >= H, same = oW == W && oH == H;
    TileOrder order;
    if (!resize_tiles_ok(call, name, oW, oH, resize_to_tile_rows(px, up), n, order)) return MF_ERR_INVALID_ARG;
    if (px == Px::U8C3)
        if (const int rc = check_d16_zero_fill(st)) return rc;
    const dim3 tab_grid(((oW > oH ? oW : oH) + 255) / 256), grid(order.per_xcd * 8u), block(64 * kWaves);
    if (px == Px::U16C3) {
        Resize16Tab* xtab = (Resize16Tab*)work;
        Resize16Tab* ytab = xtab + oW;
        if (const int rc = launch_resize16_tables_dev(d_bounds, W, H, oW, oH, work, d_status, st)) return rc;
        if (same)
            hipLaunchKernelGGL(resize16_kernel, grid, dim3(256), 0, st, (const uint16_t*)frames, (uint16_t*)out, W, H, d_bounds, xtab, ytab, order);
        else
            hipLaunchKernelGGL(resize16_to_kernel, grid, dim3(256), 0, st, (const uint16_t*)frames, (uint16_t*)out, W, H, d_bounds, oW, oH, xtab,
                               ytab, order);
        return hip_fail(hipGetLastError(), "resize16_dev_kernel launch");
    }
    ResizeTab* xtab = (ResizeTab*)work;
    ResizeTab* ytab = xtab + oW;
    hipLaunchKernelGGL(resize_tables_kernel, tab_grid, dim3(256), 0, st, d_bounds, W, H, oW, oH, d_status, xtab, ytab);
    if (const int rc = hip_fail(hipGetLastError(), "resize_tables_dev_kernel launch")) return rc;
    const uint8_t* src = (const uint8_t*)frames;
    uint8_t* dst = (uint8_t*)out;
    if (px == Px::U8C4) {
        if (up)
            hipLaunchKernelGGL((resize8c4_kernel<kUpRows, kUpSlots, kUpPitch, false>), grid, block, 0, st, src, dst, n, W, H, d_bounds, oW, oH, xtab,
                               ytab, order);
        else
            hipLaunchKernelGGL((resize8c4_kernel<kDown4Rows, 2 * kDown4Rows, kDown4Pitch, true>), grid, block, 0, st, src, dst, n, W, H, d_bounds,
                               oW, oH, xtab, ytab, order);
        return hip_fail(hipGetLastError(), "resize_bgra_dev_kernel launch");
    }
    if (px == Px::U8C1) {
        if (same) {
            hipLaunchKernelGGL(resize8c1_kernel, grid, block, 0, st, src, dst, n, W, H, d_bounds, xtab, ytab, order);
            return hip_fail(hipGetLastError(), "resize8c1_dev_kernel launch");
        }
        if (up)
            hipLaunchKernelGGL((resize8c1_to_kernel<kRows, kSrcRows, kC1RowPitch, false>), grid, block, 0, st, src, dst, n, W, H, d_bounds, oW, oH,
                               xtab, ytab, order);
        else
            hipLaunchKernelGGL((resize8c1_to_kernel<kDown1Rows, 2 * kDown1Rows, kDown1Pitch, true>), grid, block, 0, st, src, dst, n, W, H, d_bounds,
                               oW, oH, xtab, ytab, order);
        return hip_fail(hipGetLastError(), "resize8c1_to_dev_kernel launch");
    }
    if (same)
        hipLaunchKernelGGL(resize_kernel, grid, block, 0, st, src, dst, n, W, H, d_bounds, xtab, ytab, order);
    else if (up)
        hipLaunchKernelGGL((resize_to_kernel<kRows, kSrcRows, kRowPitch, false>), grid, block, 0, st, src, dst, n, W, H, d_bounds, oW, oH, xtab,
                           ytab, order);
    else
        hipLaunchKernelGGL((resize_to_kernel<kDownRows, 2 * kDownRows, kDownPitch, true>), grid, block, 0, st, src, dst, n, W, H, d_bounds, oW, oH,
                           xtab, ytab, order);
    return hip_fail(hipGetLastError(), "resize_dev_kernel launch");
}

}  // namespace mf
