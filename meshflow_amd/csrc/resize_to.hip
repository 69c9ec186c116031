// The kernel launches of mf_crop_resize_to_u8c3 / _u8c1 / _u16c3 (resize_to_body.h) behind resize.hip's checks and tables, and the output rows
// per tile of every format's instantiations.
#include "resize_to_body.h"

#include <cmath>

namespace mf {

// Whether the widest span 256 output pixels of a cw -> oW row can take (3 (ceil(255 scale_x) + 3) bytes of `px_bytes`-byte pixels, with the
// kernels' slack of `slack` bytes) fits `pitch`: the launchers pick the instantiation by it (each wavefront still checks its own span).
static bool span_fits(int cw, int oW, int px_bytes, int slack, int pitch)
{
    const double widest = (double)px_bytes * (std::ceil(255.0 * ((double)cw / (double)oW)) + 3.0);
    return widest + slack <= (double)pitch;
}

int resize_to_tile_rows(Px px, bool up)
{
    if (px == Px::U16C3) return 1;
    if (px == Px::U8C4) return resize8c4_tile_rows(up);
    if (px == Px::U8C1) return kWaves * (up ? kRows : kDown1Rows);
    return kWaves * (up ? kRows : kDownRows);
}

// launch_crop_resize_to's launch for the 8-bit formats (checks done and resize.hip's tables for (oW, oH) built there)
int launch_resize8_to(Px px, const uint8_t* frames, uint8_t* out, int n, int W, int H, int left, int top, int cw, int oW, int oH, bool up,
                      const void* work, const TileOrder& order, hipStream_t st)
{
    const ResizeTab* xtab = (const ResizeTab*)work;
    const ResizeTab* ytab = xtab + oW;
    const dim3 grid(order.per_xcd * 8u), block(64 * kWaves);
    if (px == Px::U8C1) {
        if (up)
            hipLaunchKernelGGL((resize8c1_to_kernel<kRows, kSrcRows, kC1RowPitch, false>), grid, block, 0, st, frames, out, n, W, H, left, top,
                               cw, oW, oH, xtab, ytab, order);
        else if (span_fits(cw, oW, 1, 3, kDown1Pitch))
            hipLaunchKernelGGL((resize8c1_to_kernel<kDown1Rows, 2 * kDown1Rows, kDown1Pitch, true>), grid, block, 0, st, frames, out, n, W, H,
                               left, top, cw, oW, oH, xtab, ytab, order);
        else
            hipLaunchKernelGGL((resize8c1_to_kernel<kDown1Rows, 1, 0, true>), grid, block, 0, st, frames, out, n, W, H, left, top, cw, oW, oH,
                               xtab, ytab, order);
        return hip_fail(hipGetLastError(), "resize8c1_to_kernel launch");
    }
    if (up)
        hipLaunchKernelGGL((resize_to_kernel<kRows, kSrcRows, kRowPitch, false>), grid, block, 0, st, frames, out, n, W, H, left, top, cw, oW,
                           oH, xtab, ytab, order);
    else if (span_fits(cw, oW, 3, 15, kDownPitch))
        hipLaunchKernelGGL((resize_to_kernel<kDownRows, 2 * kDownRows, kDownPitch, true>), grid, block, 0, st, frames, out, n, W, H, left, top,
                           cw, oW, oH, xtab, ytab, order);
    else
        hipLaunchKernelGGL((resize_to_kernel<kDownRows, 1, 0, true>), grid, block, 0, st, frames, out, n, W, H, left, top, cw, oW, oH, xtab,
                           ytab, order);
    return hip_fail(hipGetLastError(), "resize_to_kernel launch");
}

// launch_resize16's launch to a chosen size (resize16.hip: checks done, resize16_tables_kernel's tables for (oW, oH) built)
int launch_resize16_to_kernel(const uint16_t* frames, uint16_t* out, int W, int H, int left, int top, int cw, int oW, int oH, bool area,
                              const Resize16Tab* xtab, const Resize16Tab* ytab, const TileOrder& order, hipStream_t st)
{
    hipLaunchKernelGGL(resize16_to_kernel, dim3(order.per_xcd * 8u), dim3(256), 0, st, frames, out, W, H, left, top, cw, oW, oH, area, xtab,
                       ytab, order);
    return hip_fail(hipGetLastError(), "resize16_to_kernel launch");
}

}  // namespace mf
