// _crop_frames (mfs.py:1111-1157) from a rectangle that stays on the device: mf_crop_resize_dev_u8c3 / _u16c3 / _u8c1 / _u8c4.  The rectangle
// {left, top, right, bottom} is the 16 bytes a warp's clip-level reduction left in device memory; the host never reads it, so these calls
// never wait for the warp.  The kernels are the bodies of resize.hip, resize16.hip and resize_to.hip (here) and of resize_c1.hip / resize_c4.hip
// (resize_dev_c1.hip, resize_dev_c4.hip) compiled a second time under MF_RESIZE_DEV (resize_rect.h): the rectangle is loaded instead of
// passed, everything else is the same code, and the code objects of those five files stay what they are (tools/isa_compare.py).
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
#include "resize.hip"
#include "resize16.hip"
#include "resize_to.hip"

namespace mf {

int launch_crop_resize_dev(Px px, const void* frames, void* out, int n, int W, int H, const int32_t* d_bounds, int oW, int oH, void* work,
                           int32_t* d_status, hipStream_t st)
{
    const char* name = px_name(px);
    if (n <= 0 || W < 1 || H < 1 || W > 32767 || H > 32767) {
        set_error("mf_crop_resize_dev_%s: unsupported shape n=%d W=%d H=%d", name, n, W, H);
        return MF_ERR_INVALID_ARG;
    }
    if (oW < 1 || oH < 1 || oW > 32767 || oH > 32767) {
        set_error("mf_crop_resize_dev_%s: unsupported output size %dx%d (1 .. 32,767 each)", name, oW, oH);
        return MF_ERR_INVALID_ARG;
    }
    const bool up = oW >= W && oH >= H, same = oW == W && oH == H;
    TileOrder order;
    const int tile_rows = resize_to_tile_rows(px, up);
    if (!make_tile_order((oW + 255) / 256, (oH + tile_rows - 1) / tile_rows, n, order)) {
        set_error("mf_crop_resize_dev_%s: too many tiles", name);
        return MF_ERR_INVALID_ARG;
    }
    if (px == Px::U8C3)
        if (const int rc = check_d16_zero_fill(st)) return rc;
    const dim3 tab_grid(((oW > oH ? oW : oH) + 255) / 256), grid(order.per_xcd * 8u), block(64 * kWaves);
    if (px == Px::U16C3) {
        Resize16Tab* xtab = (Resize16Tab*)work;
        Resize16Tab* ytab = xtab + oW;
        hipLaunchKernelGGL(resize16_tables_kernel, tab_grid, dim3(256), 0, st, d_bounds, W, H, oW, oH, d_status, xtab, ytab);
        if (const int rc = hip_fail(hipGetLastError(), "resize16_tables_dev_kernel launch")) return rc;
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
    if (px == Px::U8C4) return launch_resize8c4_dev(src, dst, n, W, H, d_bounds, oW, oH, up, xtab, ytab, order, st);
    if (px == Px::U8C1) {
        if (same)
            return launch_resize8c1_dev(src, dst, n, W, H, d_bounds, xtab, ytab, order, st);
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
