// The uint16 launches of mf_crop_resize_u16c3 / mf_crop_resize_to_u16c3 behind resize.hip's checks: resize16_body.h's tables kernel, then
// resize16_kernel or resize16_to_kernel.
#include "resize16_body.h"

namespace mf {

// The tables of the cw x ch crop scaled to oW x oH (oW x-entries, then oH y-entries) in `work`: launch_resize16's, and the luma tables of
// mf_crop_resize_p010 (resize_hdr.hip)
int launch_resize16_tables(int cw, int ch, int oW, int oH, void* work, hipStream_t st)
{
    const double scale_x = 1.0 / ((double)oW / (double)cw), scale_y = 1.0 / ((double)oH / (double)ch);
    Resize16Tab* xtab = (Resize16Tab*)work;
    Resize16Tab* ytab = xtab + oW;
    const int m = oW > oH ? oW : oH;
    hipLaunchKernelGGL(resize16_tables_kernel, dim3((m + 255) / 256), dim3(256), 0, st, cw, ch, oW, oH, scale_x, scale_y, xtab, ytab);
    return hip_fail(hipGetLastError(), "resize16_tables_kernel launch");
}

// launch_crop_resize's and launch_crop_resize_to's launches for uint16 frames (every check done there): the tables, then the same-size kernel
// (oW x oH == W x H) or the one to a chosen size
int launch_resize16(const uint16_t* frames, uint16_t* out, int W, int H, int left, int top, int cw, int ch, int oW, int oH,
                    const TileOrder& order, void* work, hipStream_t st)
{
    if (const int rc = launch_resize16_tables(cw, ch, oW, oH, work, st)) return rc;
    Resize16Tab* xtab = (Resize16Tab*)work;
    Resize16Tab* ytab = xtab + oW;
    if (oW != W || oH != H) {
        hipLaunchKernelGGL(resize16_to_kernel, dim3(order.per_xcd * 8u), dim3(256), 0, st, frames, out, W, H, left, top, cw, oW, oH,
                           2 * oW == cw && 2 * oH == ch, xtab, ytab, order);
        return hip_fail(hipGetLastError(), "resize16_to_kernel launch");
    }
    hipLaunchKernelGGL(resize16_kernel, dim3(order.per_xcd * 8u), dim3(256), 0, st, frames, out, W, H, left, top, cw, xtab, ytab, order);
    return hip_fail(hipGetLastError(), "resize16_kernel launch");
}

}  // namespace mf
