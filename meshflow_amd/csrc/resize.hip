// The host side of mf_crop_resize_* and mf_crop_resize_to_* (rectangle known to the host): every check of the call, the tables launch, which
// instantiation a call to a chosen size takes, and the u8c3 kernels' launches (resize_body.h).  The other formats' kernels are launched from
// their own units (resize16.hip, resize_c1.hip, resize_c4.hip).
#include "resize_body.h"
#include "resize_checks.h"

#include <cmath>

namespace mf {

size_t crop_resize_workspace_bytes(int W, int H) { return (size_t)(W + H) * sizeof(ResizeTab); }

// resize_tables_kernel's tables of a cw x ch crop scaled to oW x oH (oW x-entries, then oH y-entries) in `work`
static int launch_resize_tables_to(int cw, int ch, int oW, int oH, void* work, hipStream_t st)
{
    const double scale_x = 1.0 / ((double)oW / (double)cw), scale_y = 1.0 / ((double)oH / (double)ch);
    ResizeTab* xtab = (ResizeTab*)work;
    ResizeTab* ytab = xtab + oW;
    const int m = oW > oH ? oW : oH;
    hipLaunchKernelGGL(resize_tables_kernel, dim3((m + 255) / 256), dim3(256), 0, st, cw, ch, oW, oH, scale_x, scale_y, xtab, ytab);
    return hip_fail(hipGetLastError(), "resize_tables_kernel launch");
}

int launch_crop_resize(Px px, const void* frames, void* out, int n, int W, int H, int left, int top, int right, int bottom,
                       void* work, hipStream_t st)
{
    if (px == Px::U8C3)
        if (const int rc = check_d16_zero_fill(st)) return rc;
    const char* const call = "mf_crop_resize_";
    const char* name = px_name(px);
    if (!resize_shape_ok(call, name, n, W, H) || !resize_rect_ok(call, name, left, top, right, bottom, W, H)) return MF_ERR_INVALID_ARG;
    // tiles: 256 pixels of kWaves * kRows output rows (resize16_kernel: of one row; resize8c4_kernel's same-size instantiation: the same)
    TileOrder order;
    if (!resize_tiles_ok(call, name, W, H, px == Px::U16C3 ? 1 : kWaves * kRows, n, order)) return MF_ERR_INVALID_ARG;
    const int cw = right - left + 1, ch = bottom - top + 1;
    if (px == Px::U16C3) return launch_resize16((const uint16_t*)frames, (uint16_t*)out, W, H, left, top, cw, ch, W, H, order, work, st);
    if (const int rc = launch_resize_tables_to(cw, ch, W, H, work, st)) return rc;
    if (px == Px::U8C1) return launch_resize8c1((const uint8_t*)frames, (uint8_t*)out, n, W, H, left, top, cw, work, order, st);
    if (px == Px::U8C4) return launch_resize8c4((const uint8_t*)frames, (uint8_t*)out, n, W, H, left, top, cw, W, H, true, work, order, st);
    const ResizeTab* xtab = (const ResizeTab*)work;
    const ResizeTab* ytab = xtab + W;
    hipLaunchKernelGGL(resize_kernel, dim3(order.per_xcd * 8u), dim3(64 * kWaves), 0, st, (const uint8_t*)frames, (uint8_t*)out, n, W, H, left, top,
                       cw, xtab, ytab, order);
    return hip_fail(hipGetLastError(), "resize_kernel launch");
}

// Whether the widest span 256 output pixels of a cw -> oW row can take (3 (ceil(255 scale_x) + 3) bytes of `px_bytes`-byte pixels, with the
// kernels' slack of `slack` bytes) fits `pitch`: the launchers pick the instantiation by it (each wavefront still checks its own span).
bool resize_span_fits(int cw, int oW, int px_bytes, int slack, int pitch)
{
    const double widest = (double)px_bytes * (std::ceil(255.0 * ((double)cw / (double)oW)) + 3.0);
    return widest + slack <= (double)pitch;
}

// output rows per tile of the format's instantiations (`up`: oW >= cw and oH >= ch)
int resize_to_tile_rows(Px px, bool up)
{
    if (px == Px::U16C3) return 1;
    if (px == Px::U8C4) return resize8c4_tile_rows(up);
    if (px == Px::U8C1) return resize8c1_tile_rows(up);
    return kWaves * (up ? kRows : kDownRows);
}

// launch_crop_resize_to's u8c3 launch (checks done and the tables for (oW, oH) built)
static int launch_resize_to(const uint8_t* frames, uint8_t* out, int n, int W, int H, int left, int top, int cw, int oW, int oH, bool up,
                            const void* work, const TileOrder& order, hipStream_t st)
{
    const ResizeTab* xtab = (const ResizeTab*)work;
    const ResizeTab* ytab = xtab + oW;
    const dim3 grid(order.per_xcd * 8u), block(64 * kWaves);
    if (up)
        hipLaunchKernelGGL((resize_to_kernel<kRows, kSrcRows, kRowPitch, false>), grid, block, 0, st, frames, out, n, W, H, left, top, cw, oW,
                           oH, xtab, ytab, order);
    else if (resize_span_fits(cw, oW, 3, 15, kDownPitch))
        hipLaunchKernelGGL((resize_to_kernel<kDownRows, 2 * kDownRows, kDownPitch, true>), grid, block, 0, st, frames, out, n, W, H, left, top,
                           cw, oW, oH, xtab, ytab, order);
    else
        hipLaunchKernelGGL((resize_to_kernel<kDownRows, 1, 0, true>), grid, block, 0, st, frames, out, n, W, H, left, top, cw, oW, oH, xtab,
                           ytab, order);
    return hip_fail(hipGetLastError(), "resize_to_kernel launch");
}

int launch_crop_resize_to(Px px, const void* frames, void* out, int n, int W, int H, int left, int top, int right, int bottom, int oW, int oH,
                          void* work, hipStream_t st)
{
    const char* const call = "mf_crop_resize_to_";
    const char* name = px_name(px);
    if (!resize_shape_ok(call, name, n, W, H) || !resize_out_size_ok(call, name, oW, oH) ||
        !resize_rect_ok(call, name, left, top, right, bottom, W, H))
        return MF_ERR_INVALID_ARG;
    const int cw = right - left + 1, ch = bottom - top + 1;
    const bool up = oW >= cw && oH >= ch;
    // tiles: 256 output pixels of kWaves x (the instantiation's rows) output rows (u16c3: one row)
    TileOrder order;
    if (!resize_tiles_ok(call, name, oW, oH, resize_to_tile_rows(px, up), n, order)) return MF_ERR_INVALID_ARG;
    if (oW == W && oH == H)                                          // the same size: mf_crop_resize_*'s call, byte for byte
        return launch_crop_resize(px, frames, out, n, W, H, left, top, right, bottom, work, st);
    if (px == Px::U8C3)
        if (const int rc = check_d16_zero_fill(st)) return rc;
    if (px == Px::U16C3)
        return launch_resize16((const uint16_t*)frames, (uint16_t*)out, W, H, left, top, cw, ch, oW, oH, order, work, st);
    if (const int rc = launch_resize_tables_to(cw, ch, oW, oH, work, st)) return rc;
    if (px == Px::U8C4)
        return launch_resize8c4((const uint8_t*)frames, (uint8_t*)out, n, W, H, left, top, cw, oW, oH, up, work, order, st);
    if (px == Px::U8C1)
        return launch_resize8c1_to((const uint8_t*)frames, (uint8_t*)out, n, W, H, left, top, cw, oW, oH, up, work, order, st);
    return launch_resize_to((const uint8_t*)frames, (uint8_t*)out, n, W, H, left, top, cw, oW, oH, up, work, order, st);
}

}  // namespace mf
