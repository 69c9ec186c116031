// The u8c4 kernel launches of mf_crop_resize_u8c4 / mf_crop_resize_to_u8c4 (resize_c4_body.h) behind resize.hip's checks and tables.
#include "resize_c4_body.h"

namespace mf {

int resize8c4_tile_rows(bool up) { return kWaves * (up ? kUpRows : kDown4Rows); }

// launch_crop_resize's / launch_crop_resize_to's launch for 4-channel frames (checks done and resize.hip's tables for (oW, oH) built there)
int launch_resize8c4(const uint8_t* frames, uint8_t* out, int n, int W, int H, int left, int top, int cw, int oW, int oH, bool up,
                     const void* work, const TileOrder& order, hipStream_t st)
{
    const ResizeTab* xtab = (const ResizeTab*)work;
    const ResizeTab* ytab = xtab + oW;
    const dim3 grid(order.per_xcd * 8u), block(64 * kWaves);
    if (up)
        hipLaunchKernelGGL((resize8c4_kernel<kUpRows, kUpSlots, kUpPitch, false>), grid, block, 0, st, frames, out, n, W, H, left, top, cw, oW, oH,
                           xtab, ytab, order);
    else if (resize_span_fits(cw, oW, 4, 0, kDown4Pitch))
        hipLaunchKernelGGL((resize8c4_kernel<kDown4Rows, 2 * kDown4Rows, kDown4Pitch, true>), grid, block, 0, st, frames, out, n, W, H, left, top,
                           cw, oW, oH, xtab, ytab, order);
    else
        hipLaunchKernelGGL((resize8c4_kernel<kDown4Rows, 1, 0, true>), grid, block, 0, st, frames, out, n, W, H, left, top, cw, oW, oH, xtab, ytab,
                           order);
    return hip_fail(hipGetLastError(), "resize8c4_kernel launch");
}

}  // namespace mf
