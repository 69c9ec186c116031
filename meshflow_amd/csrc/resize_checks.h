// The refusals the three crop-resize calls share (resize.hip: mf_crop_resize_*, mf_crop_resize_to_*; resize_dev.hip: mf_crop_resize_dev_*), each
// written once.  `call` is the call's name up to the format ("mf_crop_resize_", "mf_crop_resize_to_", "mf_crop_resize_dev_"), `name` is
// px_name(px); a helper that refuses has set mf_last_error's text and returns false, and the caller returns MF_ERR_INVALID_ARG.
#pragma once
#include "mf_common.h"

namespace mf {

inline bool resize_shape_ok(const char* call, const char* name, int n, int W, int H)
{
    if (n > 0 && W >= 1 && H >= 1 && W <= 32767 && H <= 32767) return true;    // (any number of frames that make_tile_order can count: 2^31 tiles)
    set_error("%s%s: unsupported shape n=%d W=%d H=%d", call, name, n, W, H);
    return false;
}

inline bool resize_out_size_ok(const char* call, const char* name, int oW, int oH)
{
    if (oW >= 1 && oH >= 1 && oW <= 32767 && oH <= 32767) return true;
    set_error("%s%s: unsupported output size %dx%d (1 .. 32,767 each)", call, name, oW, oH);
    return false;
}

// (the device-rectangle call's twin of this check is rect_usable, resize_rect.h)
inline bool resize_rect_ok(const char* call, const char* name, int left, int top, int right, int bottom, int W, int H)
{
    if (left >= 0 && top >= 0 && right < W && bottom < H && right >= left && bottom >= top) return true;
    set_error("%s%s: empty or out-of-frame crop rectangle (%d, %d, %d, %d) for %dx%d (cv2.resize would "
              "fail on an empty source)", call, name, left, top, right, bottom, W, H);
    return false;
}

// The tile order of n frames of oW x oH output pixels in tiles of 256 pixels x tile_rows rows
inline bool resize_tiles_ok(const char* call, const char* name, int oW, int oH, int tile_rows, int n, TileOrder& order)
{
    if (make_tile_order((oW + 255) / 256, (oH + tile_rows - 1) / tile_rows, n, order)) return true;
    set_error("%s%s: too many tiles", call, name);
    return false;
}

}  // namespace mf
