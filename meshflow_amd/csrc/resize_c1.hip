// The u8c1 kernel launches of mf_crop_resize_u8c1 / mf_crop_resize_to_u8c1 (resize_c1_body.h) behind resize.hip's checks and tables.
#include "resize_c1_body.h"

namespace mf {

int resize8c1_tile_rows(bool up) { return kWaves * (up ? kRows : kDown1Rows); }

// launch_crop_resize's launch for single-channel frames (checks done and resize.hip's tables built there)
int launch_resize8c1(const uint8_t* frames, uint8_t* out, int n, int W, int H, int left, int top, int cw, const void* work,
                     const TileOrder& order, hipStream_t st)
{
    const ResizeTab* xtab = (const ResizeTab*)work;
    const ResizeTab* ytab = xtab + W;
    hipLaunchKernelGGL(resize8c1_kernel, dim3(order.per_xcd * 8u), dim3(64 * kWaves), 0, st, frames, out, n, W, H, left, top, cw, xtab, ytab,
                       order);
    return hip_fail(hipGetLastError(), "resize8c1_kernel launch");
}

// launch_crop_resize_to's launch for single-channel frames (checks done and resize.hip's tables for (oW, oH) built there)
int launch_resize8c1_to(const uint8_t* frames, uint8_t* out, int n, int W, int H, int left, int top, int cw, int oW, int oH, bool up,
                        const void* work, const TileOrder& order, hipStream_t st)
{
    const ResizeTab* xtab = (const ResizeTab*)work;
    const ResizeTab* ytab = xtab + oW;
    const dim3 grid(order.per_xcd * 8u), block(64 * kWaves);
    if (up)
        hipLaunchKernelGGL((resize8c1_to_kernel<kRows, kSrcRows, kC1RowPitch, false>), grid, block, 0, st, frames, out, n, W, H, left, top,
                           cw, oW, oH, xtab, ytab, order);
    else if (resize_span_fits(cw, oW, 1, 3, kDown1Pitch))
        hipLaunchKernelGGL((resize8c1_to_kernel<kDown1Rows, 2 * kDown1Rows, kDown1Pitch, true>), grid, block, 0, st, frames, out, n, W, H,
                           left, top, cw, oW, oH, xtab, ytab, order);
    else
        hipLaunchKernelGGL((resize8c1_to_kernel<kDown1Rows, 1, 0, true>), grid, block, 0, st, frames, out, n, W, H, left, top, cw, oW, oH,
                           xtab, ytab, order);
    return hip_fail(hipGetLastError(), "resize8c1_to_kernel launch");
}

}  // namespace mf
