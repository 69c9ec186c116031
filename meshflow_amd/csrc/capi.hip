// C ABI of libmeshflow_hip.so: argument checking, error reporting, device plumbing and the
// host-buffer convenience wrappers.  Declarations and reference citations: include/meshflow_hip.h.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "mf_common.h"
#include "resize_checks.h"
#include "track.h"

namespace mf {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char* what)
{
    if (e == hipSuccess) return MF_OK;
    set_error("%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    return MF_ERR_HIP;
}

// The checks of every device warp entry, then launch_warp.  has_bounds: an mf_warp_bounds_* entry -- the clip-level rectangle goes to the
// caller's d_bounds instead of the table's.
static int warp_entry(const char* name, Px px, const void* d_frames, void* d_out, const void* d_table, int n, int W, int H, int R, int C,
                      const void* border, int32_t* d_crop, bool has_bounds, int32_t* d_bounds, void* stream)
{
    if (!d_frames || !d_out || !d_table || !border || !d_crop || (has_bounds && !d_bounds)) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (d_frames == d_out) { set_error("%s: d_frames and d_out alias", name); return MF_ERR_INVALID_ARG; }
    if (n <= 0 || R <= 0 || C <= 0) { set_error("%s: bad sizes", name); return MF_ERR_INVALID_ARG; }
    TableView tv = table_view(const_cast<void*>(d_table), n, W, H, R, C);
    if (has_bounds) tv.bounds = d_bounds;
    return launch_warp(px, d_frames, d_out, tv, n, W, H, R, C, pack_border(px, border), d_crop, (hipStream_t)stream);
}

// The checks of the two coordinate-map entries, then launch_warp's Px::MAPS launches on the table's frames first .. first + count - 1.
static int warp_maps_entry(const char* name, const void* d_table, float* d_maps, int n, int W, int H, int R, int C, int first, int count,
                           int32_t* d_crop, bool has_bounds, int32_t* d_bounds, void* stream)
{
    if (!d_table || !d_crop || (has_bounds && !d_bounds) || (count > 0 && !d_maps)) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (n <= 0 || R <= 0 || C <= 0) { set_error("%s: bad sizes", name); return MF_ERR_INVALID_ARG; }
    if (first < 0 || count < 0 || first > n || count > n - first) {
        set_error("%s: frames first=%d count=%d are not inside the table's n=%d", name, first, count, n);
        return MF_ERR_INVALID_ARG;
    }
    if (((uintptr_t)d_maps & 7u) != 0) { set_error("%s: d_maps must be 8-byte aligned", name); return MF_ERR_INVALID_ARG; }
    if (count == 0) return MF_OK;
    TableView tv = table_view(const_cast<void*>(d_table), n, W, H, R, C);
    if (has_bounds) tv.bounds = d_bounds;
    return launch_warp(Px::MAPS, nullptr, d_maps, table_slice(tv, first, W, H, R, C), count, W, H, R, C, 0, d_crop + 4 * (size_t)first,
                       (hipStream_t)stream);
}

// A semi-planar YUV format -- a luma plane stack and an interleaved chroma one of half the width: NV12 and NV16 (uint8 samples), P010 and P210 (uint16)
struct FmtYuv {
    int bytes;              // of a sample: 1 or 2
    const char* noun;       // with its article, for the messages
    Px luma, chroma;        // launch_warp's formats of the two plane stacks
    bool half_rows;         // chroma has half the luma rows (4:2:0: H is even too); else as many (4:2:2: H of either parity)
};
constexpr FmtYuv kNv12 = { 1, "an NV12", Px::U8C1, Px::NV12_UV, true }, kP010 = { 2, "a P010", Px::U16C1, Px::P010_UV, true },
                 kNv16 = { 1, "an NV16", Px::U8C1, Px::NV16_UV, false }, kP210 = { 2, "a P210", Px::U16C1, Px::P210_UV, false };

// The plane stacks of a semi-planar call, n frames of W x H in and of oW x oH out: aligned to 2 bytes -- the chroma pair of an NV12 or NV16 clip,
// all four of a P010 or P210 clip -- and no two of them share a byte
static bool planes_yuv_ok(const char* name, const FmtYuv& f, const void* d_y, const void* d_uv, const void* d_out_y, const void* d_out_uv, int n, int W,
                          int H, int oW, int oH)
{
    const struct { uintptr_t at; size_t bytes; const char* what; } pl[4] = {
        { (uintptr_t)d_y, (size_t)n * px_frame_bytes(f.luma, W, H), "d_y" }, { (uintptr_t)d_uv, (size_t)n * px_frame_bytes(f.chroma, W, H), "d_uv" },
        { (uintptr_t)d_out_y, (size_t)n * px_frame_bytes(f.luma, oW, oH), "d_out_y" },
        { (uintptr_t)d_out_uv, (size_t)n * px_frame_bytes(f.chroma, oW, oH), "d_out_uv" } };
    if ((((f.bytes == 2 ? pl[0].at | pl[2].at : 0) | pl[1].at | pl[3].at) & 1u) != 0) {
        set_error("%s: %s must be 2-byte aligned", name, f.bytes == 2 ? "d_y, d_uv, d_out_y and d_out_uv" : "d_uv and d_out_uv");
        return false;
    }
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (pl[i].at < pl[j].at + pl[j].bytes && pl[j].at < pl[i].at + pl[i].bytes) {
                set_error("%s: %s and %s alias", name, pl[i].what, pl[j].what);
                return false;
            }
    return true;
}

// The checks of the eight NV12, NV16, P010 and P210 warp entries, then the warp of the luma planes (launch_warp's f.luma launches: the grey warp, unchanged,
// for NV12 and NV16) and the chroma launches behind it on the same stream.  border_yuv: three samples of f.bytes each.  has_bounds: the clip-level
// rectangle goes to the caller's d_bounds instead of the table's.
static int warp_yuv_entry(const char* name, const FmtYuv& f, const void* d_y, const void* d_uv, void* d_out_y, void* d_out_uv, const void* d_table,
                          int n, int W, int H, int R, int C, const void* border_yuv, int32_t* d_crop, bool has_bounds, int32_t* d_bounds,
                          void* stream)
{
    if (!d_y || !d_uv || !d_out_y || !d_out_uv || !d_table || !border_yuv || !d_crop || (has_bounds && !d_bounds)) {
        set_error("%s: null pointer", name);
        return MF_ERR_INVALID_ARG;
    }
    if (n <= 0) { set_error("%s: bad sizes", name); return MF_ERR_INVALID_ARG; }
    if (W < 2 || H < 2 || W > 32767 || H > 32767) { set_error("%s: W=%d H=%d outside 2 .. 32,767", name, W, H); return MF_ERR_INVALID_ARG; }
    if ((f.half_rows ? W | H : W) & 1) {
        if (f.half_rows) set_error("%s: %s frame has an even W and H, got W=%d H=%d", name, f.noun, W, H);
        else set_error("%s: %s frame has an even W, got W=%d", name, f.noun, W);
        return MF_ERR_INVALID_ARG;
    }
    if (R < 1 || C < 1 || R > 64 || C > 64) { set_error("%s: mesh R=%d C=%d outside 1 .. 64", name, R, C); return MF_ERR_INVALID_ARG; }
    if (!planes_yuv_ok(name, f, d_y, d_uv, d_out_y, d_out_uv, n, W, H, W, H)) return MF_ERR_INVALID_ARG;
    TableView tv = table_view(const_cast<void*>(d_table), n, W, H, R, C);
    if (has_bounds) tv.bounds = d_bounds;
    const void* const border_uv = (const char*)border_yuv + f.bytes;
    if (const int rc = launch_warp(f.luma, d_y, d_out_y, tv, n, W, H, R, C, pack_border(f.luma, border_yuv), d_crop, (hipStream_t)stream)) return rc;
    return launch_warp(f.chroma, d_uv, d_out_uv, tv, n, W, H, R, C, pack_border(f.chroma, border_uv), d_crop, (hipStream_t)stream);
}

// The element checks every plane entry shares: elem_bytes is 0 (the float32 calls) or 1, 2, 4, 8, and both pointers are aligned to the element
static bool plane_elem_ok(const char* name, int elem_bytes, const void* d_planes, const void* d_out)
{
    if (elem_bytes != 0 && elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) {
        set_error("%s: elem_bytes=%d (1, 2, 4 or 8)", name, elem_bytes);
        return false;
    }
    const uintptr_t mask = (uintptr_t)(elem_bytes ? elem_bytes : 4) - 1u;
    if ((((uintptr_t)d_planes | (uintptr_t)d_out) & mask) != 0) {
        set_error("%s: d_planes and d_out must be aligned to their %d-byte elements", name, (int)mask + 1);
        return false;
    }
    return true;
}

// The checks of the two plane warps, then launch_warp's Px::PLANE_* launches.  elem_bytes == 0: mf_warp_plane_f32 (fill: the float's bits).
// d_bounds may be null: the clip-level rectangle then goes to the table's own four words, as in mf_warp_u8c3.
static int warp_plane_entry(const char* name, int elem_bytes, const void* d_planes, void* d_out, const void* d_table, int n, int W, int H, int R,
                            int C, uint64_t fill, int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    if (!d_planes || !d_out || !d_table || !d_crop) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (d_planes == d_out) { set_error("%s: d_planes and d_out alias", name); return MF_ERR_INVALID_ARG; }
    if (n <= 0 || R <= 0 || C <= 0) { set_error("%s: bad sizes", name); return MF_ERR_INVALID_ARG; }
    if (!plane_elem_ok(name, elem_bytes, d_planes, d_out)) return MF_ERR_INVALID_ARG;
    const Px px = elem_bytes == 0 ? Px::PLANE_F32 : elem_bytes == 1 ? Px::PLANE_N1 : elem_bytes == 2 ? Px::PLANE_N2 :
                  elem_bytes == 4 ? Px::PLANE_N4 : Px::PLANE_N8;
    TableView tv = table_view(const_cast<void*>(d_table), n, W, H, R, C);
    if (d_bounds) tv.bounds = d_bounds;
    return launch_warp(px, d_planes, d_out, tv, n, W, H, R, C, fill, d_crop, (hipStream_t)stream);
}

// The checks the four plane crop-resize entries share ahead of their launchers' (elem_bytes == 0: the float32 calls)
static int crop_resize_plane_checks(const char* name, int elem_bytes, const void* d_planes, const void* d_out, const void* d_work, bool dev,
                                    const void* d_bounds, const void* d_status)
{
    if (!d_planes || !d_out || !d_work || (dev && (!d_bounds || !d_status))) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (d_planes == d_out) { set_error("%s: d_planes and d_out alias", name); return MF_ERR_INVALID_ARG; }
    if (!plane_elem_ok(name, elem_bytes, d_planes, d_out)) return MF_ERR_INVALID_ARG;
    return MF_OK;
}

static int crop_resize_entry(const char* name, Px px, const void* d_frames, void* d_out, int n, int W, int H, int left, int top, int right,
                             int bottom, void* d_work, void* stream)
{
    if (!d_frames || !d_out || !d_work) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (d_frames == d_out) { set_error("%s: d_frames and d_out alias", name); return MF_ERR_INVALID_ARG; }
    return launch_crop_resize(px, d_frames, d_out, n, W, H, left, top, right, bottom, d_work, (hipStream_t)stream);
}

static int crop_resize_to_entry(const char* name, Px px, const void* d_frames, void* d_out, int n, int W, int H, int left, int top,
                                int right, int bottom, int out_W, int out_H, void* d_work, void* stream)
{
    if (!d_frames || !d_out || !d_work) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (d_frames == d_out) { set_error("%s: d_frames and d_out alias", name); return MF_ERR_INVALID_ARG; }
    return launch_crop_resize_to(px, d_frames, d_out, n, W, H, left, top, right, bottom, out_W, out_H, d_work, (hipStream_t)stream);
}

static int crop_resize_dev_entry(const char* name, Px px, const void* d_frames, void* d_out, int n, int W, int H, const int32_t* d_bounds,
                                 int out_W, int out_H, void* d_work, int32_t* d_status, void* stream)
{
    if (!d_frames || !d_out || !d_bounds || !d_work || !d_status) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (d_frames == d_out) { set_error("%s: d_frames and d_out alias", name); return MF_ERR_INVALID_ARG; }
    return launch_crop_resize_dev(px, d_frames, d_out, n, W, H, d_bounds, out_W, out_H, d_work, d_status, (hipStream_t)stream);
}

// The checks of the eight NV12, NV16, P010 and P210 crop-resize entries -- all of them ahead of the first launch, under the call's own name `name` --,
// then the format's launches on one stream.  NV12 and NV16: the luma call as it is (launch_crop_resize_to / launch_crop_resize_dev on Px::U8C1)
// and the chroma launches behind it (NV16's on the luma call's own y table: chroma has luma's rows, so H and oH may be odd).  P010: the luma
// tables, the luma kernel, the chroma tables and the chroma kernel (resize_hdr.hip / resize_hdr_dev.hip); P210: the same luma launches, then the
// chroma x table and the chroma kernel on the luma y table (the same two units).
// dev: an mf_crop_resize_dev_* call (the rectangle in d_bounds, left .. bottom unused).
static int crop_resize_yuv_entry(const char* name, const FmtYuv& f, bool dev, const void* d_y, const void* d_uv, void* d_out_y, void* d_out_uv,
                                 int n, int W, int H, int left, int top, int right, int bottom, const int32_t* d_bounds, int oW, int oH,
                                 void* d_work, int32_t* d_status, void* stream)
{
    if (!d_y || !d_uv || !d_out_y || !d_out_uv || !d_work || (dev && (!d_bounds || !d_status))) {
        set_error("%s: null pointer", name);
        return MF_ERR_INVALID_ARG;
    }
    if (n <= 0) { set_error("%s: bad sizes n=%d", name, n); return MF_ERR_INVALID_ARG; }
    if (W < 2 || H < 2 || W > 32767 || H > 32767) { set_error("%s: W=%d H=%d outside 2 .. 32,767", name, W, H); return MF_ERR_INVALID_ARG; }
    if (oW < 2 || oH < 2 || oW > 32767 || oH > 32767) {
        set_error("%s: unsupported output size %dx%d (2 .. 32,767 each)", name, oW, oH);
        return MF_ERR_INVALID_ARG;
    }
    if ((f.half_rows ? W | H : W) & 1) {
        if (f.half_rows) set_error("%s: %s frame has an even W and H, got W=%d H=%d", name, f.noun, W, H);
        else set_error("%s: %s frame has an even W, got W=%d", name, f.noun, W);
        return MF_ERR_INVALID_ARG;
    }
    if ((f.half_rows ? oW | oH : oW) & 1) {
        if (f.half_rows) set_error("%s: %s output has an even size, got %dx%d", name, f.noun, oW, oH);
        else set_error("%s: %s output has an even width, got %dx%d", name, f.noun, oW, oH);
        return MF_ERR_INVALID_ARG;
    }
    if (!planes_yuv_ok(name, f, d_y, d_uv, d_out_y, d_out_uv, n, W, H, oW, oH)) return MF_ERR_INVALID_ARG;
    if (!dev && !resize_rect_ok(name, "", left, top, right, bottom, W, H)) return MF_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (f.bytes == 2) {
        const uint16_t* const y = (const uint16_t*)d_y, * const uv = (const uint16_t*)d_uv;
        uint16_t* const out_y = (uint16_t*)d_out_y, * const out_uv = (uint16_t*)d_out_uv;
        TileOrder luma, chroma;
        if (!(f.half_rows ? resize_hdr_tile_orders(oW, oH, n, luma, chroma) : resize_p210_tile_orders(oW, oH, n, luma, chroma))) {
            set_error("%s: too many tiles", name);
            return MF_ERR_INVALID_ARG;
        }
        if (!f.half_rows) {
            if (dev) return launch_resize_p210_dev(y, uv, out_y, out_uv, W, H, d_bounds, oW, oH, d_work, d_status, luma, chroma, st);
            return launch_resize_p210(y, uv, out_y, out_uv, W, H, left, top, right, bottom, oW, oH, d_work, luma, chroma, st);
        }
        if (dev) return launch_resize_hdr_dev(y, uv, out_y, out_uv, W, H, d_bounds, oW, oH, d_work, d_status, luma, chroma, st);
        return launch_resize_hdr(y, uv, out_y, out_uv, W, H, left, top, right, bottom, oW, oH, d_work, luma, chroma, st);
    }
    // the luma call's tiles at their smallest (the `down` instantiation's rows: the most tiles any of its paths counts), then chroma's
    TileOrder luma_order, order;
    if (!resize_tiles_ok(name, "", oW, oH, resize_to_tile_rows(Px::U8C1, false), n, luma_order)) return MF_ERR_INVALID_ARG;
    if (!(f.half_rows ? resize_uv_tile_order(oW, oH, n, order) : resize_uv422_tile_order(oW, oH, n, order))) {
        set_error("%s: too many tiles", name);
        return MF_ERR_INVALID_ARG;
    }
    void* const tabs = (char*)d_work + crop_resize_workspace_bytes(oW, oH);
    const void* const luma_ytab = (const ResizeTab*)d_work + oW;      // (the luma call's y table: NV16 chroma rows are luma's)
    if (dev) {
        if (const int rc = launch_crop_resize_dev(Px::U8C1, d_y, d_out_y, n, W, H, d_bounds, oW, oH, d_work, d_status, st)) return rc;
        if (!f.half_rows) return launch_resize_uv422_dev((const uint8_t*)d_uv, (uint8_t*)d_out_uv, W, H, d_bounds, oW, oH, luma_ytab, tabs, order, st);
        return launch_resize_uv_dev((const uint8_t*)d_uv, (uint8_t*)d_out_uv, W, H, d_bounds, oW, oH, tabs, order, st);
    }
    if (const int rc = launch_crop_resize_to(Px::U8C1, d_y, d_out_y, n, W, H, left, top, right, bottom, oW, oH, d_work, st)) return rc;
    if (!f.half_rows) {
        return launch_resize_uv422((const uint8_t*)d_uv, (uint8_t*)d_out_uv, W, H, left, top, right, bottom, oW, oH, luma_ytab, tabs, order, st);
    }
    return launch_resize_uv((const uint8_t*)d_uv, (uint8_t*)d_out_uv, W, H, left, top, right, bottom, oW, oH, tabs, order, st);
}

// Every check the tracker's calls share (include/meshflow_hip.h); the geometry on success.
static int track_checks(const char* name, int n, int W, int H, int sub_rows, int sub_cols, int max_per, track::Geom& g)
{
    if (W < 1 || H < 1 || W > 32767 || H > 32767) { set_error("%s: W and H must be in 1 .. 32,767 (got %d x %d)", name, W, H); return MF_ERR_INVALID_ARG; }
    if (sub_rows < 1 || sub_cols < 1 || sub_rows > H || sub_cols > W) {
        set_error("%s: sub_rows must be in 1 .. H and sub_cols in 1 .. W (got %d x %d for %d x %d)", name, sub_rows, sub_cols, W, H);
        return MF_ERR_INVALID_ARG;
    }
    g = track::make_geom(W, H, sub_rows, sub_cols);
    const int last_w = W - (g.ncols - 1) * g.sub_w, last_h = H - (g.nrows - 1) * g.sub_h;
    if (last_w < MF_TRACK_MIN_SUBFRAME || last_h < MF_TRACK_MIN_SUBFRAME) {
        set_error("%s: sub-frame below the minimum: the smallest is %d x %d, every sub-frame must be at least %d x %d", name, last_w, last_h,
                  MF_TRACK_MIN_SUBFRAME, MF_TRACK_MIN_SUBFRAME);
        return MF_ERR_INVALID_ARG;
    }
    if (max_per < 1 || max_per > MF_TRACK_MAX_PER_SUBFRAME) {
        set_error("%s: max_per_subframe must be in 1 .. %d (got %d)", name, MF_TRACK_MAX_PER_SUBFRAME, max_per);
        return MF_ERR_INVALID_ARG;
    }
    if (n < 1 || 2ll * n * g.ncols * g.nrows > 65535) {
        set_error("%s: n must be at least 1 with 2 * n * sub-frames <= 65,535 (got n = %d, %d sub-frames): too many for one call", name, n,
                  g.ncols * g.nrows);
        return MF_ERR_INVALID_ARG;
    }
    return MF_OK;
}

static bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace mf

using namespace mf;

extern "C" {

int mf_abi_version(void) { return MF_ABI_VERSION; }
const char* mf_last_error(void) { return g_err; }

int mf_device_count(int* count)
{
    if (!count) { set_error("mf_device_count: null"); return MF_ERR_INVALID_ARG; }
    *count = 0;
    MF_HIP_TRY(hipGetDeviceCount(count));
    return MF_OK;
}

int mf_set_device(int device)
{
    MF_HIP_TRY(hipSetDevice(device));
    return check_d16_zero_fill(nullptr);       // the one-time, synchronising device check of the byte-tap kernels: here, not in a launch
}

int mf_malloc(void** d_ptr, size_t bytes)
{
    if (!d_ptr) { set_error("mf_malloc: null"); return MF_ERR_INVALID_ARG; }
    MF_HIP_TRY(hipMalloc(d_ptr, bytes));
    return MF_OK;
}
int mf_free(void* d_ptr) { MF_HIP_TRY(hipFree(d_ptr)); return MF_OK; }
int mf_malloc_host(void** h_ptr, size_t bytes)
{
    if (!h_ptr) { set_error("mf_malloc_host: null"); return MF_ERR_INVALID_ARG; }
    MF_HIP_TRY(hipHostMalloc(h_ptr, bytes, hipHostMallocDefault));
    return MF_OK;
}
int mf_free_host(void* h_ptr) { MF_HIP_TRY(hipHostFree(h_ptr)); return MF_OK; }
int mf_memcpy_h2d(void* d, const void* h, size_t bytes, void* stream)
{
    MF_HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return MF_OK;
}
int mf_memcpy_d2h(void* h, const void* d, size_t bytes, void* stream)
{
    MF_HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return MF_OK;
}
int mf_stream_synchronize(void* stream) { MF_HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); return MF_OK; }

int mf_jacobi_f64(const double* d_b, double* d_x, const double* d_taps, const double* d_lam,
                  const double* d_inv_on, int F, int S, int omega, int iters, void* stream)
{
    if (!d_b || !d_x || !d_taps || !d_lam || !d_inv_on) { set_error("mf_jacobi_f64: null pointer"); return MF_ERR_INVALID_ARG; }
    if (d_b == d_x) { set_error("mf_jacobi_f64: d_b and d_x alias"); return MF_ERR_INVALID_ARG; }
    return launch_jacobi(d_b, d_x, d_taps, d_lam, d_inv_on, F, S, omega, iters, (hipStream_t)stream);
}

size_t mf_cell_table_bytes(int n, int W, int H, int R, int C)
{
    if (n <= 0 || R <= 0 || C <= 0 || W <= 0 || H <= 0) return 0;
    return table_bytes(n, W, H, R, C);
}

size_t mf_cell_table_bounds_offset(int n, int W, int H, int R, int C)
{
    if (n <= 0 || R <= 0 || C <= 0 || W <= 0 || H <= 0) return 0;
    alignas(16) static char origin[16];                    // (any address: only the offset of the section is wanted)
    const TableView tv = table_view(origin, n, W, H, R, C);
    return (size_t)((const char*)tv.bounds - origin);
}

int mf_cell_table_f64(const double* d_unstab, const double* d_stab, int n, int W, int H, int R, int C,
                      void* d_table, int32_t* d_crop, int32_t* d_status, void* stream)
{
    if (!d_unstab || !d_stab || !d_table || !d_crop || !d_status) { set_error("mf_cell_table_f64: null pointer"); return MF_ERR_INVALID_ARG; }
    if (n <= 0 || R <= 0 || C <= 0) { set_error("mf_cell_table_f64: bad sizes"); return MF_ERR_INVALID_ARG; }
    const TableView tv = table_view(d_table, n, W, H, R, C);
    return launch_cell_table(d_unstab, d_stab, n, W, H, R, C, tv, d_crop, d_status, (hipStream_t)stream);
}

int mf_warp_u8c3(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                 int R, int C, const uint8_t border_bgr[3], int32_t* d_crop, void* stream)
{
    return warp_entry("mf_warp_u8c3", Px::U8C3, d_frames, d_out, d_table, n, W, H, R, C, border_bgr, d_crop, false, nullptr, stream);
}

int mf_warp_u16c3(const uint16_t* d_frames, uint16_t* d_out, const void* d_table, int n, int W, int H,
                  int R, int C, const uint16_t border_bgr[3], int32_t* d_crop, void* stream)
{
    return warp_entry("mf_warp_u16c3", Px::U16C3, d_frames, d_out, d_table, n, W, H, R, C, border_bgr, d_crop, false, nullptr, stream);
}

int mf_warp_u8c1(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                 int R, int C, uint8_t border, int32_t* d_crop, void* stream)
{
    return warp_entry("mf_warp_u8c1", Px::U8C1, d_frames, d_out, d_table, n, W, H, R, C, &border, d_crop, false, nullptr, stream);
}

int mf_warp_u8c4(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                 int R, int C, const uint8_t border_bgra[4], int32_t* d_crop, void* stream)
{
    return warp_entry("mf_warp_u8c4", Px::U8C4, d_frames, d_out, d_table, n, W, H, R, C, border_bgra, d_crop, false, nullptr, stream);
}

int mf_crop_scan_f64(const void* d_table, int n, int W, int H, int R, int C, int32_t* d_crop, void* stream)
{
    if (!d_table || !d_crop) { set_error("mf_crop_scan_f64: null pointer"); return MF_ERR_INVALID_ARG; }
    if (n <= 0 || R <= 0 || C <= 0) { set_error("mf_crop_scan_f64: bad sizes"); return MF_ERR_INVALID_ARG; }
    const TableView tv = table_view(const_cast<void*>(d_table), n, W, H, R, C);
    return launch_crop_scan(tv, n, W, H, R, C, d_crop, (hipStream_t)stream);
}

int mf_warp_maps_f32(const void* d_table, float* d_maps, int n, int W, int H, int R, int C, int first, int count, int32_t* d_crop, void* stream)
{
    return warp_maps_entry("mf_warp_maps_f32", d_table, d_maps, n, W, H, R, C, first, count, d_crop, false, nullptr, stream);
}

int mf_warp_maps_bounds_f32(const void* d_table, float* d_maps, int n, int W, int H, int R, int C, int first, int count, int32_t* d_crop,
                            int32_t* d_bounds, void* stream)
{
    return warp_maps_entry("mf_warp_maps_bounds_f32", d_table, d_maps, n, W, H, R, C, first, count, d_crop, true, d_bounds, stream);
}

int mf_warp_plane_f32(const float* d_planes, float* d_out, const void* d_table, int n, int W, int H, int R, int C, float fill,
                      int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    uint32_t bits;
    memcpy(&bits, &fill, sizeof bits);
    return warp_plane_entry("mf_warp_plane_f32", 0, d_planes, d_out, d_table, n, W, H, R, C, bits, d_crop, d_bounds, stream);
}

int mf_warp_plane_nearest(const void* d_planes, void* d_out, const void* d_table, int n, int W, int H, int R, int C, int elem_bytes,
                          uint64_t fill_bits, int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    if (elem_bytes == 0) elem_bytes = -1;           // (0 is warp_plane_entry's word for the float32 call)
    return warp_plane_entry("mf_warp_plane_nearest", elem_bytes, d_planes, d_out, d_table, n, W, H, R, C, fill_bits, d_crop, d_bounds, stream);
}

int mf_warp_nv12(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, const void* d_table, int n, int W, int H,
                 int R, int C, const uint8_t border_yuv[3], int32_t* d_crop, void* stream)
{
    return warp_yuv_entry("mf_warp_nv12", kNv12, d_y, d_uv, d_out_y, d_out_uv, d_table, n, W, H, R, C, border_yuv, d_crop, false, nullptr, stream);
}

int mf_warp_bounds_nv12(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, const void* d_table, int n, int W, int H,
                        int R, int C, const uint8_t border_yuv[3], int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    return warp_yuv_entry("mf_warp_bounds_nv12", kNv12, d_y, d_uv, d_out_y, d_out_uv, d_table, n, W, H, R, C, border_yuv, d_crop, true, d_bounds,
                          stream);
}

int mf_warp_nv16(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, const void* d_table, int n, int W, int H,
                 int R, int C, const uint8_t border_yuv[3], int32_t* d_crop, void* stream)
{
    return warp_yuv_entry("mf_warp_nv16", kNv16, d_y, d_uv, d_out_y, d_out_uv, d_table, n, W, H, R, C, border_yuv, d_crop, false, nullptr, stream);
}

int mf_warp_bounds_nv16(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, const void* d_table, int n, int W, int H,
                        int R, int C, const uint8_t border_yuv[3], int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    return warp_yuv_entry("mf_warp_bounds_nv16", kNv16, d_y, d_uv, d_out_y, d_out_uv, d_table, n, W, H, R, C, border_yuv, d_crop, true, d_bounds,
                          stream);
}

int mf_warp_p210(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, const void* d_table, int n, int W, int H,
                 int R, int C, const uint16_t border_yuv[3], int32_t* d_crop, void* stream)
{
    return warp_yuv_entry("mf_warp_p210", kP210, d_y, d_uv, d_out_y, d_out_uv, d_table, n, W, H, R, C, border_yuv, d_crop, false, nullptr, stream);
}

int mf_warp_bounds_p210(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, const void* d_table, int n, int W, int H,
                        int R, int C, const uint16_t border_yuv[3], int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    return warp_yuv_entry("mf_warp_bounds_p210", kP210, d_y, d_uv, d_out_y, d_out_uv, d_table, n, W, H, R, C, border_yuv, d_crop, true, d_bounds,
                          stream);
}

int mf_warp_p010(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, const void* d_table, int n, int W, int H,
                 int R, int C, const uint16_t border_yuv[3], int32_t* d_crop, void* stream)
{
    return warp_yuv_entry("mf_warp_p010", kP010, d_y, d_uv, d_out_y, d_out_uv, d_table, n, W, H, R, C, border_yuv, d_crop, false, nullptr, stream);
}

int mf_warp_bounds_p010(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, const void* d_table, int n, int W, int H,
                        int R, int C, const uint16_t border_yuv[3], int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    return warp_yuv_entry("mf_warp_bounds_p010", kP010, d_y, d_uv, d_out_y, d_out_uv, d_table, n, W, H, R, C, border_yuv, d_crop, true, d_bounds,
                          stream);
}

// ---- the same three calls with the clip-level rectangle in the CALLER's d_bounds[4] instead of inside the table blob ----

int mf_cell_table_bounds_f64(const double* d_unstab, const double* d_stab, int n, int W, int H, int R, int C,
                             void* d_table, int32_t* d_crop, int32_t* d_status, int32_t* d_bounds, void* stream)
{
    if (!d_unstab || !d_stab || !d_table || !d_crop || !d_status || !d_bounds) { set_error("mf_cell_table_bounds_f64: null pointer"); return MF_ERR_INVALID_ARG; }
    if (n <= 0 || R <= 0 || C <= 0) { set_error("mf_cell_table_bounds_f64: bad sizes"); return MF_ERR_INVALID_ARG; }
    TableView tv = table_view(d_table, n, W, H, R, C);
    tv.bounds = d_bounds;
    return launch_cell_table(d_unstab, d_stab, n, W, H, R, C, tv, d_crop, d_status, (hipStream_t)stream);
}

int mf_warp_bounds_u8c3(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                        int R, int C, const uint8_t border_bgr[3], int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    return warp_entry("mf_warp_bounds_u8c3", Px::U8C3, d_frames, d_out, d_table, n, W, H, R, C, border_bgr, d_crop, true, d_bounds, stream);
}

int mf_warp_bounds_u16c3(const uint16_t* d_frames, uint16_t* d_out, const void* d_table, int n, int W, int H,
                         int R, int C, const uint16_t border_bgr[3], int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    return warp_entry("mf_warp_bounds_u16c3", Px::U16C3, d_frames, d_out, d_table, n, W, H, R, C, border_bgr, d_crop, true, d_bounds, stream);
}

int mf_warp_bounds_u8c1(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                        int R, int C, uint8_t border, int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    return warp_entry("mf_warp_bounds_u8c1", Px::U8C1, d_frames, d_out, d_table, n, W, H, R, C, &border, d_crop, true, d_bounds, stream);
}

int mf_warp_bounds_u8c4(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                        int R, int C, const uint8_t border_bgra[4], int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    return warp_entry("mf_warp_bounds_u8c4", Px::U8C4, d_frames, d_out, d_table, n, W, H, R, C, border_bgra, d_crop, true, d_bounds, stream);
}

int mf_crop_scan_bounds_f64(const void* d_table, int n, int W, int H, int R, int C, int32_t* d_crop, int32_t* d_bounds, void* stream)
{
    if (!d_table || !d_crop || !d_bounds) { set_error("mf_crop_scan_bounds_f64: null pointer"); return MF_ERR_INVALID_ARG; }
    if (n <= 0 || R <= 0 || C <= 0) { set_error("mf_crop_scan_bounds_f64: bad sizes"); return MF_ERR_INVALID_ARG; }
    TableView tv = table_view(const_cast<void*>(d_table), n, W, H, R, C);
    tv.bounds = d_bounds;
    return launch_crop_scan(tv, n, W, H, R, C, d_crop, (hipStream_t)stream);
}

int mf_crop_reduce(const int32_t* d_crop, int n, int W, int H, int32_t* d_bounds, void* stream)
{
    if (!d_crop || !d_bounds) { set_error("mf_crop_reduce: null pointer"); return MF_ERR_INVALID_ARG; }
    return launch_crop_reduce(d_crop, n, W, H, d_bounds, (hipStream_t)stream);
}

size_t mf_crop_resize_workspace_bytes(int W, int H)
{
    return (W > 0 && H > 0) ? crop_resize_workspace_bytes(W, H) : 0;
}

int mf_crop_resize_u8c3(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right,
                        int bottom, void* d_work, void* stream)
{
    return crop_resize_entry("mf_crop_resize_u8c3", Px::U8C3, d_frames, d_out, n, W, H, left, top, right, bottom, d_work, stream);
}

int mf_crop_resize_u16c3(const uint16_t* d_frames, uint16_t* d_out, int n, int W, int H, int left, int top, int right,
                         int bottom, void* d_work, void* stream)
{
    return crop_resize_entry("mf_crop_resize_u16c3", Px::U16C3, d_frames, d_out, n, W, H, left, top, right, bottom, d_work, stream);
}

int mf_crop_resize_u8c1(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right,
                        int bottom, void* d_work, void* stream)
{
    return crop_resize_entry("mf_crop_resize_u8c1", Px::U8C1, d_frames, d_out, n, W, H, left, top, right, bottom, d_work, stream);
}

int mf_crop_resize_u8c4(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right,
                        int bottom, void* d_work, void* stream)
{
    return crop_resize_entry("mf_crop_resize_u8c4", Px::U8C4, d_frames, d_out, n, W, H, left, top, right, bottom, d_work, stream);
}

int mf_crop_resize_to_u8c3(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right, int bottom,
                           int out_W, int out_H, void* d_work, void* stream)
{
    return crop_resize_to_entry("mf_crop_resize_to_u8c3", Px::U8C3, d_frames, d_out, n, W, H, left, top, right, bottom, out_W, out_H, d_work,
                                stream);
}

int mf_crop_resize_to_u16c3(const uint16_t* d_frames, uint16_t* d_out, int n, int W, int H, int left, int top, int right, int bottom,
                            int out_W, int out_H, void* d_work, void* stream)
{
    return crop_resize_to_entry("mf_crop_resize_to_u16c3", Px::U16C3, d_frames, d_out, n, W, H, left, top, right, bottom, out_W, out_H, d_work,
                                stream);
}

int mf_crop_resize_to_u8c1(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right, int bottom,
                           int out_W, int out_H, void* d_work, void* stream)
{
    return crop_resize_to_entry("mf_crop_resize_to_u8c1", Px::U8C1, d_frames, d_out, n, W, H, left, top, right, bottom, out_W, out_H, d_work,
                                stream);
}

int mf_crop_resize_to_u8c4(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right, int bottom,
                           int out_W, int out_H, void* d_work, void* stream)
{
    return crop_resize_to_entry("mf_crop_resize_to_u8c4", Px::U8C4, d_frames, d_out, n, W, H, left, top, right, bottom, out_W, out_H, d_work,
                                stream);
}

int mf_crop_resize_dev_u8c3(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                            void* d_work, int32_t* d_status, void* stream)
{
    return crop_resize_dev_entry("mf_crop_resize_dev_u8c3", Px::U8C3, d_frames, d_out, n, W, H, d_bounds, out_W, out_H, d_work, d_status, stream);
}

int mf_crop_resize_dev_u16c3(const uint16_t* d_frames, uint16_t* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                             void* d_work, int32_t* d_status, void* stream)
{
    return crop_resize_dev_entry("mf_crop_resize_dev_u16c3", Px::U16C3, d_frames, d_out, n, W, H, d_bounds, out_W, out_H, d_work, d_status, stream);
}

int mf_crop_resize_dev_u8c1(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                            void* d_work, int32_t* d_status, void* stream)
{
    return crop_resize_dev_entry("mf_crop_resize_dev_u8c1", Px::U8C1, d_frames, d_out, n, W, H, d_bounds, out_W, out_H, d_work, d_status, stream);
}

int mf_crop_resize_dev_u8c4(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                            void* d_work, int32_t* d_status, void* stream)
{
    return crop_resize_dev_entry("mf_crop_resize_dev_u8c4", Px::U8C4, d_frames, d_out, n, W, H, d_bounds, out_W, out_H, d_work, d_status, stream);
}

size_t mf_crop_resize_nv12_workspace_bytes(int out_W, int out_H)
{
    return (out_W > 0 && out_H > 0) ? crop_resize_nv12_workspace_bytes(out_W, out_H) : 0;
}

int mf_crop_resize_nv12(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, int n, int W, int H, int left, int top,
                        int right, int bottom, int out_W, int out_H, void* d_work, void* stream)
{
    return crop_resize_yuv_entry("mf_crop_resize_nv12", kNv12, false, d_y, d_uv, d_out_y, d_out_uv, n, W, H, left, top, right, bottom, nullptr, out_W,
                                 out_H, d_work, nullptr, stream);
}

int mf_crop_resize_dev_nv12(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, int n, int W, int H,
                            const int32_t* d_bounds, int out_W, int out_H, void* d_work, int32_t* d_status, void* stream)
{
    return crop_resize_yuv_entry("mf_crop_resize_dev_nv12", kNv12, true, d_y, d_uv, d_out_y, d_out_uv, n, W, H, 0, 0, 0, 0, d_bounds, out_W, out_H,
                                 d_work, d_status, stream);
}

size_t mf_crop_resize_nv16_workspace_bytes(int out_W, int out_H)
{
    return (out_W > 0 && out_H > 0) ? crop_resize_nv16_workspace_bytes(out_W, out_H) : 0;
}

int mf_crop_resize_nv16(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, int n, int W, int H, int left, int top,
                        int right, int bottom, int out_W, int out_H, void* d_work, void* stream)
{
    return crop_resize_yuv_entry("mf_crop_resize_nv16", kNv16, false, d_y, d_uv, d_out_y, d_out_uv, n, W, H, left, top, right, bottom, nullptr, out_W,
                                 out_H, d_work, nullptr, stream);
}

int mf_crop_resize_dev_nv16(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, int n, int W, int H,
                            const int32_t* d_bounds, int out_W, int out_H, void* d_work, int32_t* d_status, void* stream)
{
    return crop_resize_yuv_entry("mf_crop_resize_dev_nv16", kNv16, true, d_y, d_uv, d_out_y, d_out_uv, n, W, H, 0, 0, 0, 0, d_bounds, out_W, out_H,
                                 d_work, d_status, stream);
}

size_t mf_crop_resize_p210_workspace_bytes(int out_W, int out_H)
{
    return (out_W > 0 && out_H > 0) ? crop_resize_p210_workspace_bytes(out_W, out_H) : 0;
}

int mf_crop_resize_p210(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, int n, int W, int H, int left, int top,
                        int right, int bottom, int out_W, int out_H, void* d_work, void* stream)
{
    return crop_resize_yuv_entry("mf_crop_resize_p210", kP210, false, d_y, d_uv, d_out_y, d_out_uv, n, W, H, left, top, right, bottom, nullptr, out_W,
                                 out_H, d_work, nullptr, stream);
}

int mf_crop_resize_dev_p210(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, int n, int W, int H,
                            const int32_t* d_bounds, int out_W, int out_H, void* d_work, int32_t* d_status, void* stream)
{
    return crop_resize_yuv_entry("mf_crop_resize_dev_p210", kP210, true, d_y, d_uv, d_out_y, d_out_uv, n, W, H, 0, 0, 0, 0, d_bounds, out_W, out_H,
                                 d_work, d_status, stream);
}

size_t mf_crop_resize_p010_workspace_bytes(int out_W, int out_H)
{
    return (out_W > 0 && out_H > 0) ? crop_resize_p010_workspace_bytes(out_W, out_H) : 0;
}

int mf_crop_resize_p010(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, int n, int W, int H, int left, int top,
                        int right, int bottom, int out_W, int out_H, void* d_work, void* stream)
{
    return crop_resize_yuv_entry("mf_crop_resize_p010", kP010, false, d_y, d_uv, d_out_y, d_out_uv, n, W, H, left, top, right, bottom, nullptr, out_W,
                                 out_H, d_work, nullptr, stream);
}

int mf_crop_resize_dev_p010(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, int n, int W, int H,
                            const int32_t* d_bounds, int out_W, int out_H, void* d_work, int32_t* d_status, void* stream)
{
    return crop_resize_yuv_entry("mf_crop_resize_dev_p010", kP010, true, d_y, d_uv, d_out_y, d_out_uv, n, W, H, 0, 0, 0, 0, d_bounds, out_W, out_H,
                                 d_work, d_status, stream);
}

int mf_crop_resize_plane_f32(const float* d_planes, float* d_out, int n, int W, int H, int left, int top, int right, int bottom, int out_W,
                             int out_H, void* d_work, void* stream)
{
    if (const int rc = crop_resize_plane_checks("mf_crop_resize_plane_f32", 0, d_planes, d_out, d_work, false, nullptr, nullptr)) return rc;
    return launch_crop_resize_plane(0, d_planes, d_out, n, W, H, left, top, right, bottom, out_W, out_H, d_work, (hipStream_t)stream);
}

int mf_crop_resize_plane_nearest(const void* d_planes, void* d_out, int n, int W, int H, int left, int top, int right, int bottom, int out_W,
                                 int out_H, int elem_bytes, void* d_work, void* stream)
{
    if (elem_bytes == 0) elem_bytes = -1;
    if (const int rc = crop_resize_plane_checks("mf_crop_resize_plane_nearest", elem_bytes, d_planes, d_out, d_work, false, nullptr, nullptr)) return rc;
    return launch_crop_resize_plane(elem_bytes, d_planes, d_out, n, W, H, left, top, right, bottom, out_W, out_H, d_work, (hipStream_t)stream);
}

int mf_crop_resize_dev_plane_f32(const float* d_planes, float* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                                 void* d_work, int32_t* d_status, void* stream)
{
    if (const int rc = crop_resize_plane_checks("mf_crop_resize_dev_plane_f32", 0, d_planes, d_out, d_work, true, d_bounds, d_status)) return rc;
    return launch_crop_resize_plane_dev(0, d_planes, d_out, n, W, H, d_bounds, out_W, out_H, d_work, d_status, (hipStream_t)stream);
}

int mf_crop_resize_dev_plane_nearest(const void* d_planes, void* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                                     int elem_bytes, void* d_work, int32_t* d_status, void* stream)
{
    if (elem_bytes == 0) elem_bytes = -1;
    if (const int rc = crop_resize_plane_checks("mf_crop_resize_dev_plane_nearest", elem_bytes, d_planes, d_out, d_work, true, d_bounds, d_status))
        return rc;
    return launch_crop_resize_plane_dev(elem_bytes, d_planes, d_out, n, W, H, d_bounds, out_W, out_H, d_work, d_status, (hipStream_t)stream);
}

size_t mf_track_workspace_bytes(int n_pairs, int W, int H, int sub_rows, int sub_cols, int max_per_subframe)
{
    track::Geom g;
    if (track_checks("mf_track_workspace_bytes", n_pairs, W, H, sub_rows, sub_cols, max_per_subframe, g)) return 0;
    const size_t mask = align16(track_mask_bytes(g, n_pairs)), pyramid = track_pyramid_bytes(g, n_pairs);
    return mask > pyramid ? mask : pyramid;
}

int mf_fast_corners_u8(const uint8_t* d_grey, int n, int W, int H, int sub_rows, int sub_cols, int max_per_subframe, int threshold,
                       float* d_points, int32_t* d_counts, int32_t* d_status, void* d_work, void* stream)
{
    const char* name = "mf_fast_corners_u8";
    if (!d_grey || !d_points || !d_counts || !d_status || !d_work) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    track::Geom g;
    if (const int rc = track_checks(name, n, W, H, sub_rows, sub_cols, max_per_subframe, g)) return rc;
    if (threshold < 1 || threshold > 254) { set_error("%s: threshold must be in 1 .. 254 (got %d)", name, threshold); return MF_ERR_INVALID_ARG; }
    if (((uintptr_t)d_points & 7) || ((uintptr_t)d_counts & 3) || ((uintptr_t)d_status & 3)) {
        set_error("%s: d_points must be 8-byte aligned, d_counts and d_status 4-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    const size_t slots = (size_t)n * g.ncols * g.nrows, frames = (size_t)n * W * H;
    if (overlap(d_grey, frames, d_points, slots * max_per_subframe * 8) || overlap(d_grey, frames, d_counts, slots * 4) ||
        overlap(d_grey, frames, d_status, slots * 4) || overlap(d_grey, frames, d_work, track_mask_bytes(g, n))) {
        set_error("%s: the frames alias an output or the workspace", name);
        return MF_ERR_INVALID_ARG;
    }
    return launch_fast_corners(d_grey, n, g, max_per_subframe, threshold, d_points, d_counts, d_status, d_work, (hipStream_t)stream);
}

int mf_lk_track_u8(const uint8_t* d_early, const uint8_t* d_late, int n_pairs, int W, int H, int sub_rows, int sub_cols,
                   int max_per_subframe, const float* d_points, const int32_t* d_counts, float* d_moved, uint8_t* d_found, void* d_work,
                   void* stream)
{
    const char* name = "mf_lk_track_u8";
    if (!d_early || !d_late || !d_points || !d_counts || !d_moved || !d_found || !d_work) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    track::Geom g;
    if (const int rc = track_checks(name, n_pairs, W, H, sub_rows, sub_cols, max_per_subframe, g)) return rc;
    if (((uintptr_t)d_points & 7) || ((uintptr_t)d_moved & 7) || ((uintptr_t)d_counts & 3)) {
        set_error("%s: d_points and d_moved must be 8-byte aligned, d_counts 4-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    const size_t slots = (size_t)n_pairs * g.ncols * g.nrows, frames = (size_t)n_pairs * W * H;
    for (const uint8_t* stack : {d_early, d_late})
        if (overlap(stack, frames, d_moved, slots * max_per_subframe * 8) || overlap(stack, frames, d_found, slots * max_per_subframe) ||
            overlap(stack, frames, d_work, track_pyramid_bytes(g, n_pairs))) {
            set_error("%s: the frames alias an output or the workspace", name);
            return MF_ERR_INVALID_ARG;
        }
    if (const int rc = launch_pyramid(d_early, d_late, n_pairs, g, d_work, (hipStream_t)stream)) return rc;
    return launch_lk_levels(d_early, d_late, n_pairs, g, max_per_subframe, d_points, d_counts, d_moved, d_found, d_work, (hipStream_t)stream);
}

// The checks mf_ransac_inliers_f32 and its workspace size share: the sizes only.
static int ransac_size_checks(const char* name, int n_pairs, int S, int max_per)
{
    if (max_per < 1 || max_per > MF_TRACK_MAX_PER_SUBFRAME) {
        set_error("%s: max_per_subframe must be in 1 .. %d (got %d)", name, MF_TRACK_MAX_PER_SUBFRAME, max_per);
        return MF_ERR_INVALID_ARG;
    }
    if (n_pairs < 1 || S < 1 || 2ll * n_pairs * S > 65535) {
        set_error("%s: n_pairs and S must be at least 1 with 2 * n_pairs * S <= 65,535 (got n_pairs = %d, S = %d): too many for one call", name,
                  n_pairs, S);
        return MF_ERR_INVALID_ARG;
    }
    return MF_OK;
}

size_t mf_ransac_workspace_bytes(int n_pairs, int S, int max_per_subframe)
{
    if (ransac_size_checks("mf_ransac_workspace_bytes", n_pairs, S, max_per_subframe)) return 0;
    return ransac_workspace_bytes(n_pairs, S, max_per_subframe);
}

int mf_ransac_inliers_f32(const float* d_points, const float* d_moved, const int32_t* d_counts, const uint8_t* d_found, int n_pairs, int S,
                          int max_per_subframe, int min_features, double threshold, double confidence, int max_iters, uint32_t seed,
                          uint8_t* d_inlier, int32_t* d_info, void* d_work, void* stream)
{
    const char* name = "mf_ransac_inliers_f32";
    if (!d_points || !d_moved || !d_counts || !d_found || !d_inlier || !d_info || !d_work) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (const int rc = ransac_size_checks(name, n_pairs, S, max_per_subframe)) return rc;
    if (min_features < 1) { set_error("%s: min_features must be at least 1 (got %d)", name, min_features); return MF_ERR_INVALID_ARG; }
    if (!(threshold > 0.0) || !(threshold - threshold == 0.0)) { set_error("%s: threshold must be finite and > 0 (got %g)", name, threshold); return MF_ERR_INVALID_ARG; }
    if (!(confidence > 0.0 && confidence < 1.0)) { set_error("%s: confidence must be in (0, 1) (got %g)", name, confidence); return MF_ERR_INVALID_ARG; }
    if (max_iters < 1 || max_iters > MF_RANSAC_MAX_ITERS) {
        set_error("%s: max_iters must be in 1 .. %d (got %d)", name, MF_RANSAC_MAX_ITERS, max_iters);
        return MF_ERR_INVALID_ARG;
    }
    if (((uintptr_t)d_points & 7) || ((uintptr_t)d_moved & 7) || ((uintptr_t)d_counts & 3) || ((uintptr_t)d_info & 3) || ((uintptr_t)d_work & 15)) {
        set_error("%s: d_points and d_moved must be 8-byte aligned, d_counts and d_info 4-byte aligned, d_work 16-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    const size_t slots = (size_t)n_pairs * S, features = slots * max_per_subframe;
    const struct { const void* at; size_t bytes; } in[4] = {{d_points, features * 8}, {d_moved, features * 8}, {d_counts, slots * 4}, {d_found, features}},
                                                   out[3] = {{d_inlier, features}, {d_info, slots * 16},
                                                             {d_work, ransac_workspace_bytes(n_pairs, S, max_per_subframe)}};
    for (const auto& i : in)
        for (const auto& o : out)
            if (overlap(i.at, i.bytes, o.at, o.bytes)) { set_error("%s: an input aliases an output or the workspace", name); return MF_ERR_INVALID_ARG; }
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (overlap(out[a].at, out[a].bytes, out[b].at, out[b].bytes)) {
                set_error("%s: two of d_inlier, d_info and d_work alias", name);
                return MF_ERR_INVALID_ARG;
            }
    return launch_ransac(d_points, d_moved, d_counts, d_found, n_pairs, S, max_per_subframe, min_features, threshold, confidence, max_iters, seed,
                         d_inlier, d_info, d_work, (hipStream_t)stream);
}

int mf_track_gather_f64(const float* d_points, const float* d_moved, const uint8_t* d_inlier, const int32_t* d_info, int n_pairs, int W, int H,
                        int sub_rows, int sub_cols, int max_per_subframe, int min_features, double* d_early, double* d_late,
                        int32_t* d_offsets, int32_t* d_pair_status, void* stream)
{
    const char* name = "mf_track_gather_f64";
    if (!d_points || !d_moved || !d_inlier || !d_info || !d_early || !d_late || !d_offsets || !d_pair_status) {
        set_error("%s: null pointer", name);
        return MF_ERR_INVALID_ARG;
    }
    track::Geom g;
    if (const int rc = track_checks(name, n_pairs, W, H, sub_rows, sub_cols, max_per_subframe, g)) return rc;
    if (min_features < 1) { set_error("%s: min_features must be at least 1 (got %d)", name, min_features); return MF_ERR_INVALID_ARG; }
    if (((uintptr_t)d_points & 7) || ((uintptr_t)d_moved & 7) || ((uintptr_t)d_early & 7) || ((uintptr_t)d_late & 7) || ((uintptr_t)d_info & 3) ||
        ((uintptr_t)d_offsets & 3) || ((uintptr_t)d_pair_status & 3)) {
        set_error("%s: d_points, d_moved, d_early and d_late must be 8-byte aligned, d_info, d_offsets and d_pair_status 4-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    const size_t slots = (size_t)n_pairs * g.ncols * g.nrows, features = slots * max_per_subframe;
    const struct { const void* at; size_t bytes; } in[4] = {{d_points, features * 8}, {d_moved, features * 8}, {d_inlier, features}, {d_info, slots * 16}},
                                                   out[4] = {{d_early, features * 16}, {d_late, features * 16}, {d_offsets, ((size_t)n_pairs + 1) * 4},
                                                             {d_pair_status, (size_t)n_pairs * 4}};
    for (const auto& i : in)
        for (const auto& o : out)
            if (overlap(i.at, i.bytes, o.at, o.bytes)) { set_error("%s: an input aliases an output", name); return MF_ERR_INVALID_ARG; }
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (overlap(out[a].at, out[a].bytes, out[b].at, out[b].bytes)) { set_error("%s: two outputs alias", name); return MF_ERR_INVALID_ARG; }
    return launch_track_gather(d_points, d_moved, d_inlier, d_info, n_pairs, g, max_per_subframe, min_features, d_early, d_late, d_offsets,
                               d_pair_status, (hipStream_t)stream);
}

size_t mf_homography_fit_workspace_bytes(int n_pairs)
{
    if (n_pairs < 0 || n_pairs > hfit::MAX_PAIRS) return 0;
    return hfit_workspace_bytes(n_pairs);
}

int mf_homography_fit_f64(const double* d_early, const double* d_late, const int32_t* d_offsets, int n_pairs, int K_total, double* d_h,
                          int32_t* d_info, double* d_diag, void* d_work, void* stream)
{
    const char* name = "mf_homography_fit_f64";
    if (n_pairs < 0 || K_total < 0) { set_error("%s: n_pairs and K_total must not be negative (got %d, %d)", name, n_pairs, K_total); return MF_ERR_INVALID_ARG; }
    if (n_pairs > hfit::MAX_PAIRS) {
        set_error("%s: n_pairs must be at most %d, the tracker's own limit (got %d): too many for one call", name, hfit::MAX_PAIRS, n_pairs);
        return MF_ERR_INVALID_ARG;
    }
    if (!d_offsets || !d_h || !d_info || !d_diag || !d_work || (K_total > 0 && (!d_early || !d_late))) {
        set_error("%s: null pointer", name);
        return MF_ERR_INVALID_ARG;
    }
    if (((uintptr_t)d_early & 7) || ((uintptr_t)d_late & 7) || ((uintptr_t)d_h & 7) || ((uintptr_t)d_diag & 7) || ((uintptr_t)d_work & 7) ||
        ((uintptr_t)d_offsets & 3) || ((uintptr_t)d_info & 3)) {
        set_error("%s: d_early, d_late, d_h, d_diag and d_work must be 8-byte aligned, d_offsets and d_info 4-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    const size_t P = (size_t)n_pairs, features = (size_t)K_total;
    const struct { const void* at; size_t bytes; } in[3] = {{d_early, features * 16}, {d_late, features * 16}, {d_offsets, (P + 1) * 4}},
                                                   out[4] = {{d_h, P * 72}, {d_info, P * 16}, {d_diag, P * 64}, {d_work, hfit_workspace_bytes(n_pairs)}};
    for (const auto& i : in)
        for (const auto& o : out)
            if (overlap(i.at, i.bytes, o.at, o.bytes)) { set_error("%s: an input aliases an output or the workspace", name); return MF_ERR_INVALID_ARG; }
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (overlap(out[a].at, out[a].bytes, out[b].at, out[b].bytes)) {
                set_error("%s: two of d_h, d_info, d_diag and d_work alias", name);
                return MF_ERR_INVALID_ARG;
            }
    if (n_pairs == 0) return MF_OK;
    return launch_homography_fit(d_early, d_late, d_offsets, n_pairs, K_total, d_h, d_info, d_diag, d_work, (hipStream_t)stream);
}

size_t mf_vertex_motion_workspace_bytes(int total_features, int max_per_pair, int P, int R, int C)
{
    if (total_features < 0 || max_per_pair < 0 || P < 0 || R <= 0 || C <= 0) return 0;
    return vertex_motion_workspace_bytes(total_features, max_per_pair, P, R, C);
}

int mf_vertex_motion_f64(const double* d_early, const double* d_late, const int32_t* d_offsets, const double* d_hom,
                         int P, int total_features, int max_per_pair, int W, int H, int R, int C,
                         int ellipse_rows, int ellipse_cols, float* d_velocities, double* d_displacements,
                         void* d_work, int32_t* d_status, void* stream)
{
    if (!d_offsets || !d_displacements || !d_work || !d_status || (P > 0 && (!d_hom || !d_velocities)) ||
        (total_features > 0 && (!d_early || !d_late))) {
        set_error("mf_vertex_motion_f64: null pointer");
        return MF_ERR_INVALID_ARG;
    }
    return launch_vertex_motion(d_early, d_late, d_offsets, d_hom, P, total_features, max_per_pair, W, H, R, C,
                                ellipse_rows, ellipse_cols, d_velocities, d_displacements, d_work, d_status, (hipStream_t)stream);
}

// What mf_online_smooth_f64, mf_online_smooth_lag_f64 and mf_online_smooth_group_f64 refuse alike, under the caller's name: MF_OK where the
// launches may go ahead.  K rows of n frames on the state stacks of B streams; the single calls are K = B = 1 with `seen` on the host and
// no d_ids / d_seen (group false).
static int online_smooth_checks(const char* name, const float* d_vel, const double* d_lam_known, const double* d_taps, int n, int S, int omega,
                                int window, int iters, double beta, double lam_newest, int64_t seen, double* d_c_state, double* d_q_state,
                                double* d_lam_state, double* d_c_out, double* d_p_out, bool group = false, int K = 1, int B = 1,
                                const int32_t* d_ids = nullptr, const int64_t* d_seen = nullptr)
{
    if (n < 1 || S < 1) { set_error("%s: n and S must be at least 1 (got %d, %d)", name, n, S); return MF_ERR_INVALID_ARG; }
    if (K < 1 || B < 1 || K > B || K > MF_ONLINE_GROUP_MAX_ROWS) {
        set_error("%s: K rows of B streams need 1 <= K <= B and K <= %d (got K=%d, B=%d)", name, MF_ONLINE_GROUP_MAX_ROWS, K, B);
        return MF_ERR_INVALID_ARG;
    }
    if (window < 2 || window > MF_ONLINE_MAX_WINDOW) {
        set_error("%s: window must be in 2 .. %d (got %d)", name, MF_ONLINE_MAX_WINDOW, window);
        return MF_ERR_INVALID_ARG;
    }
    if (omega < 1 || omega > MF_ONLINE_MAX_OMEGA) { set_error("%s: omega must be in 1 .. %d (got %d)", name, MF_ONLINE_MAX_OMEGA, omega); return MF_ERR_INVALID_ARG; }
    if (iters < 1 || iters > MF_ONLINE_MAX_ITERS) { set_error("%s: iters must be in 1 .. %d (got %d)", name, MF_ONLINE_MAX_ITERS, iters); return MF_ERR_INVALID_ARG; }
    if (!(beta >= 0.0) || !(beta - beta == 0.0)) { set_error("%s: beta must be finite and >= 0 (got %g)", name, beta); return MF_ERR_INVALID_ARG; }
    if (!(lam_newest >= 0.0) || !(lam_newest - lam_newest == 0.0)) {
        set_error("%s: lam_newest must be finite and >= 0 (got %g)", name, lam_newest);
        return MF_ERR_INVALID_ARG;
    }
    if (seen < 0) { set_error("%s: seen must not be negative (got %lld)", name, (long long)seen); return MF_ERR_INVALID_ARG; }
    if (!d_vel || !d_lam_known || !d_taps || !d_c_state || !d_q_state || !d_lam_state || !d_c_out || !d_p_out || (group && (!d_ids || !d_seen))) {
        set_error("%s: null pointer", name);
        return MF_ERR_INVALID_ARG;
    }
    if (((uintptr_t)d_vel & 3) || ((uintptr_t)d_lam_known & 7) || ((uintptr_t)d_taps & 7) || ((uintptr_t)d_c_state & 7) || ((uintptr_t)d_q_state & 7) ||
        ((uintptr_t)d_lam_state & 7) || ((uintptr_t)d_c_out & 7) || ((uintptr_t)d_p_out & 7)) {
        set_error("%s: d_vel must be 4-byte aligned, every float64 array 8-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    if (((uintptr_t)d_ids & 3) || ((uintptr_t)d_seen & 7)) {
        set_error("%s: d_ids must be 4-byte aligned, d_seen 8-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    const size_t rows = (size_t)K * (size_t)n, series = (size_t)S, held = (size_t)B * ((size_t)window - 1);
    const struct { const void* at; size_t bytes; } in[5] = {{d_vel, rows * series * 4}, {d_lam_known, rows * 8}, {d_taps, (size_t)omega * 8},
                                                            {d_ids, group ? (size_t)K * 4 : 0}, {d_seen, group ? (size_t)K * 8 : 0}},
                                                   state[3] = {{d_c_state, held * series * 8}, {d_q_state, held * series * 8}, {d_lam_state, held * 8}},
                                                   out[2] = {{d_c_out, rows * series * 8}, {d_p_out, rows * series * 8}};
    for (const auto& o : out) {
        for (const auto& i : in)
            if (i.bytes && overlap(i.at, i.bytes, o.at, o.bytes)) { set_error("%s: an output aliases an input", name); return MF_ERR_INVALID_ARG; }
        for (const auto& q : state)
            if (overlap(q.at, q.bytes, o.at, o.bytes)) { set_error("%s: an output aliases the state", name); return MF_ERR_INVALID_ARG; }
    }
    if (overlap(out[0].at, out[0].bytes, out[1].at, out[1].bytes)) { set_error("%s: d_c_out and d_p_out alias", name); return MF_ERR_INVALID_ARG; }
    for (int a = 0; a < 3; ++a) {                           // (the state is updated in place while the inputs are still being read)
        for (const auto& i : in)
            if (i.bytes && overlap(i.at, i.bytes, state[a].at, state[a].bytes)) { set_error("%s: the state aliases an input", name); return MF_ERR_INVALID_ARG; }
        for (int b = a + 1; b < 3; ++b)
            if (overlap(state[a].at, state[a].bytes, state[b].at, state[b].bytes)) {
                set_error("%s: two of the state arrays alias", name);
                return MF_ERR_INVALID_ARG;
            }
    }
    return MF_OK;
}

int mf_online_smooth_f64(const float* d_vel, const double* d_lam_known, const double* d_taps, int n, int S, int omega, int window, int iters,
                         double beta, double lam_newest, int64_t seen, double* d_c_state, double* d_q_state, double* d_lam_state,
                         double* d_c_out, double* d_p_out, void* stream)
{
    const int rc = online_smooth_checks("mf_online_smooth_f64", d_vel, d_lam_known, d_taps, n, S, omega, window, iters, beta, lam_newest, seen,
                                        d_c_state, d_q_state, d_lam_state, d_c_out, d_p_out);
    if (rc != MF_OK) return rc;
    return launch_online_smooth(d_vel, d_lam_known, d_taps, n, S, omega, window, iters, beta, lam_newest, (long long)seen, d_c_state, d_q_state,
                                d_lam_state, d_c_out, d_p_out, (hipStream_t)stream);
}

int mf_online_smooth_lag_f64(const float* d_vel, const double* d_lam_known, const double* d_taps, int n, int S, int omega, int window, int lag,
                             int iters, double beta, double lam_newest, int64_t seen, double* d_c_state, double* d_q_state,
                             double* d_lam_state, double* d_c_out, double* d_p_out, void* stream)
{
    const char* name = "mf_online_smooth_lag_f64";
    const int rc = online_smooth_checks(name, d_vel, d_lam_known, d_taps, n, S, omega, window, iters, beta, lam_newest, seen, d_c_state, d_q_state,
                                        d_lam_state, d_c_out, d_p_out);
    if (rc != MF_OK) return rc;
    if (lag < 0 || lag > window - 1) {
        set_error("%s: lag must be in 0 .. window - 1 = %d (got %d)", name, window - 1, lag);
        return MF_ERR_INVALID_ARG;
    }
    return launch_online_smooth_lag(d_vel, d_lam_known, d_taps, n, S, omega, window, lag, iters, beta, lam_newest, (long long)seen, d_c_state,
                                    d_q_state, d_lam_state, d_c_out, d_p_out, (hipStream_t)stream);
}

int mf_online_smooth_group_f64(const float* d_vel, const double* d_lam_known, const double* d_taps, const int32_t* d_ids, const int64_t* d_seen,
                               int K, int B, int n, int S, int omega, int window, int iters, double beta, double lam_newest, double* d_c_state,
                               double* d_q_state, double* d_lam_state, double* d_c_out, double* d_p_out, void* stream)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "d_seen is read as long long on the device");
    const int rc = online_smooth_checks("mf_online_smooth_group_f64", d_vel, d_lam_known, d_taps, n, S, omega, window, iters, beta, lam_newest, 0,
                                        d_c_state, d_q_state, d_lam_state, d_c_out, d_p_out, true, K, B, d_ids, d_seen);
    if (rc != MF_OK) return rc;
    return launch_online_smooth_group(d_vel, d_lam_known, d_taps, d_ids, reinterpret_cast<const long long*>(d_seen), K, B, n, S, omega, window,
                                      iters, beta, lam_newest, d_c_state, d_q_state, d_lam_state, d_c_out, d_p_out, (hipStream_t)stream);
}

int mf_online_smooth_group_lag_f64(const float* d_vel, const double* d_lam_known, const double* d_taps, const int32_t* d_ids, const int64_t* d_seen,
                                   int K, int B, int n, int S, int omega, int window, int lag, int iters, double beta, double lam_newest,
                                   double* d_c_state, double* d_q_state, double* d_lam_state, double* d_c_out, double* d_p_out, void* stream)
{
    const char* name = "mf_online_smooth_group_lag_f64";
    const int rc = online_smooth_checks(name, d_vel, d_lam_known, d_taps, n, S, omega, window, iters, beta, lam_newest, 0, d_c_state, d_q_state,
                                        d_lam_state, d_c_out, d_p_out, true, K, B, d_ids, d_seen);
    if (rc != MF_OK) return rc;
    if (lag < 0 || lag > window - 1) {
        set_error("%s: lag must be in 0 .. window - 1 = %d (got %d)", name, window - 1, lag);
        return MF_ERR_INVALID_ARG;
    }
    return launch_online_smooth_group_lag(d_vel, d_lam_known, d_taps, d_ids, reinterpret_cast<const long long*>(d_seen), K, B, n, S, omega, window,
                                          lag, iters, beta, lam_newest, d_c_state, d_q_state, d_lam_state, d_c_out, d_p_out, (hipStream_t)stream);
}

int mf_frame_signature_u8(const uint8_t* d_luma, int n, int W, int H, int32_t* d_sig, void* stream)
{
    const char* name = "mf_frame_signature_u8";
    if (!d_luma || !d_sig) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: n must be at least 1 (got %d)", name, n); return MF_ERR_INVALID_ARG; }
    if (W < 1 || W > MF_CUT_MAX_DIM || H < 1 || H > MF_CUT_MAX_DIM) {
        set_error("%s: W and H must be in 1 .. %d (got %d x %d)", name, MF_CUT_MAX_DIM, W, H);
        return MF_ERR_INVALID_ARG;
    }
    if ((uintptr_t)d_sig & 3) { set_error("%s: d_sig must be 4-byte aligned", name); return MF_ERR_INVALID_ARG; }
    if (overlap(d_luma, (size_t)n * (size_t)W * (size_t)H, d_sig, (size_t)n * MF_CUT_COUNTERS * 4)) {
        set_error("%s: d_sig overlaps the frames", name);
        return MF_ERR_INVALID_ARG;
    }
    return launch_frame_signature(d_luma, n, W, H, d_sig, (hipStream_t)stream);
}

int mf_cut_distance_i32(const int32_t* d_sig_prev, const int32_t* d_sig, int n, int32_t* d_dist, void* stream)
{
    const char* name = "mf_cut_distance_i32";
    if (!d_sig || !d_dist) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: n must be at least 1 (got %d)", name, n); return MF_ERR_INVALID_ARG; }
    if (((uintptr_t)d_sig_prev & 3) || ((uintptr_t)d_sig & 3) || ((uintptr_t)d_dist & 3)) {
        set_error("%s: d_sig_prev, d_sig and d_dist must be 4-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    if (overlap(d_sig, (size_t)n * MF_CUT_COUNTERS * 4, d_dist, (size_t)n * 4) ||
        (d_sig_prev && overlap(d_sig_prev, MF_CUT_COUNTERS * 4, d_dist, (size_t)n * 4))) {
        set_error("%s: d_dist overlaps a signature", name);
        return MF_ERR_INVALID_ARG;
    }
    return launch_cut_distance(d_sig_prev, d_sig, n, d_dist, (hipStream_t)stream);
}

int mf_cut_distance_pairs_i32(const int32_t* d_prev, const int32_t* d_sig, int n, int32_t* d_dist, void* stream)
{
    const char* name = "mf_cut_distance_pairs_i32";
    if (!d_prev || !d_sig || !d_dist) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: n must be at least 1 (got %d)", name, n); return MF_ERR_INVALID_ARG; }
    if (((uintptr_t)d_prev & 3) || ((uintptr_t)d_sig & 3) || ((uintptr_t)d_dist & 3)) {
        set_error("%s: d_prev, d_sig and d_dist must be 4-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    if (overlap(d_sig, (size_t)n * MF_CUT_COUNTERS * 4, d_dist, (size_t)n * 4) || overlap(d_prev, (size_t)n * MF_CUT_COUNTERS * 4, d_dist, (size_t)n * 4)) {
        set_error("%s: d_dist overlaps a signature", name);
        return MF_ERR_INVALID_ARG;
    }
    return launch_cut_distance_pairs(d_prev, d_sig, n, d_dist, (hipStream_t)stream);
}

// What mf_path_limit_f64 and mf_path_limit_group_f64 refuse alike, under the caller's name; carried: the int32 words d_k_prev holds where it is
// given (1, or a word per row of a group, where it must be given).
static int path_limit_checks(const char* name, const double* d_unstab, const double* d_stab, int n, int W, int H, int R, int C, int left, int top,
                             int right, int bottom, double guard, int steps, int rise, const int32_t* d_k_prev, size_t carried, int32_t* d_k_raw,
                             int32_t* d_k, double* d_out)
{
    if (n < 1) { set_error("%s: n must be at least 1 (got %d)", name, n); return MF_ERR_INVALID_ARG; }
    if (R < 1 || C < 1 || (long long)R + (long long)C > MF_PATH_LIMIT_MAX_BOUNDARY / 2) {
        set_error("%s: mesh R=%d C=%d: each at least 1 with 2 (R + C) <= %d boundary vertices", name, R, C, MF_PATH_LIMIT_MAX_BOUNDARY);
        return MF_ERR_INVALID_ARG;
    }
    if (W < 2 || H < 2) { set_error("%s: W and H must be at least 2 (got %d x %d)", name, W, H); return MF_ERR_INVALID_ARG; }
    if (!(0 <= left && left <= right && right <= W - 1 && 0 <= top && top <= bottom && bottom <= H - 1)) {
        set_error("%s: rectangle (%d, %d, %d, %d) is not inside a %d x %d frame", name, left, top, right, bottom, W, H);
        return MF_ERR_INVALID_ARG;
    }
    if (steps < 1 || steps > MF_PATH_LIMIT_MAX_STEPS) {
        set_error("%s: steps must be in 1 .. %d (got %d)", name, MF_PATH_LIMIT_MAX_STEPS, steps);
        return MF_ERR_INVALID_ARG;
    }
    if (rise < 1 || rise > steps) { set_error("%s: rise must be in 1 .. steps = %d (got %d)", name, steps, rise); return MF_ERR_INVALID_ARG; }
    if (!(guard >= 0.0) || !(guard - guard == 0.0)) { set_error("%s: guard must be finite and >= 0 (got %g)", name, guard); return MF_ERR_INVALID_ARG; }
    if (!d_unstab || !d_stab || !d_k_raw || !d_k || !d_out) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (((uintptr_t)d_unstab & 7) || ((uintptr_t)d_stab & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_k_prev & 3) || ((uintptr_t)d_k_raw & 3) ||
        ((uintptr_t)d_k & 3)) {
        set_error("%s: every float64 array must be 8-byte aligned, every int32 array 4-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    const size_t path = (size_t)n * (size_t)(R + 1) * (size_t)(C + 1) * 2 * sizeof(double), words = (size_t)n * sizeof(int32_t);
    const struct { const void* at; size_t bytes; } in[3] = {{d_unstab, path}, {d_stab, path}, {d_k_prev, d_k_prev ? carried * sizeof(int32_t) : 0}},
                                                   out[3] = {{d_k_raw, words}, {d_k, words}, {d_out, path}};
    for (int a = 0; a < 3; ++a) {
        for (const auto& i : in)
            if (i.bytes && overlap(i.at, i.bytes, out[a].at, out[a].bytes)) { set_error("%s: an output aliases an input", name); return MF_ERR_INVALID_ARG; }
        for (int b = a + 1; b < 3; ++b)
            if (overlap(out[a].at, out[a].bytes, out[b].at, out[b].bytes)) { set_error("%s: two of the outputs alias", name); return MF_ERR_INVALID_ARG; }
    }
    return MF_OK;
}

int mf_path_limit_f64(const double* d_unstab, const double* d_stab, int n, int W, int H, int R, int C, int left, int top, int right, int bottom,
                      double guard, int steps, int rise, const int32_t* d_k_prev, int32_t* d_k_raw, int32_t* d_k, double* d_out, void* stream)
{
    const int rc = path_limit_checks("mf_path_limit_f64", d_unstab, d_stab, n, W, H, R, C, left, top, right, bottom, guard, steps, rise, d_k_prev, 1,
                                     d_k_raw, d_k, d_out);
    if (rc != MF_OK) return rc;
    return launch_path_limit(d_unstab, d_stab, n, W, H, R, C, left, top, right, bottom, guard, steps, rise, d_k_prev, d_k_raw, d_k, d_out,
                             (hipStream_t)stream);
}

int mf_path_limit_group_f64(const double* d_unstab, const double* d_stab, int K, int W, int H, int R, int C, int left, int top, int right, int bottom,
                            double guard, int steps, int rise, const int32_t* d_k_prev, int32_t* d_k_raw, int32_t* d_k, double* d_out, void* stream)
{
    const char* name = "mf_path_limit_group_f64";
    const int rc = path_limit_checks(name, d_unstab, d_stab, K, W, H, R, C, left, top, right, bottom, guard, steps, rise, d_k_prev,
                                     K > 0 ? (size_t)K : 0, d_k_raw, d_k, d_out);
    if (rc != MF_OK) return rc;
    if (!d_k_prev) { set_error("%s: null pointer (d_k_prev holds a word per row; a negative word says that nothing is carried)", name); return MF_ERR_INVALID_ARG; }
    return launch_path_limit_group(d_unstab, d_stab, K, W, H, R, C, left, top, right, bottom, guard, steps, rise, d_k_prev, d_k_raw, d_k, d_out,
                                   (hipStream_t)stream);
}

int mf_stability_score_f64(const double* d_stab, int F, int S, double* d_series, double* d_score, void* stream)
{
    if (!d_stab || !d_series || !d_score) { set_error("mf_stability_score_f64: null pointer"); return MF_ERR_INVALID_ARG; }
    return launch_stability_score(d_stab, F, S, d_series, d_score, (hipStream_t)stream);
}

static int run_selftest(int (*launch)(unsigned long long, unsigned long long, unsigned long long*, hipStream_t),
                        uint64_t n, uint64_t seed, uint64_t* mismatches)
{
    void* d = nullptr;
    MF_HIP_TRY(hipMalloc(&d, sizeof(uint64_t)));
    hipError_t e = hipMemset(d, 0, sizeof(uint64_t));
    int rc = e == hipSuccess ? launch(n, seed, (unsigned long long*)d, nullptr) : hip_fail(e, "hipMemset");
    if (rc == MF_OK) rc = hip_fail(hipMemcpy(mismatches, d, sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

int mf_selftest_sqrt(uint64_t n, uint64_t seed, uint64_t* mismatches)
{
    if (!mismatches) { set_error("mf_selftest_sqrt: null"); return MF_ERR_INVALID_ARG; }
    return run_selftest(launch_selftest_sqrt, n, seed, mismatches);
}

int mf_selftest_recip(uint64_t n, uint64_t seed, uint64_t* mismatches)
{
    if (!mismatches) { set_error("mf_selftest_recip: null"); return MF_ERR_INVALID_ARG; }
    return run_selftest(launch_selftest_recip, n, seed, mismatches);
}

int mf_selftest_fast64(uint64_t n, uint64_t seed, uint64_t* counters)
{
    if (!counters) { set_error("mf_selftest_fast64: null"); return MF_ERR_INVALID_ARG; }
    void* d = nullptr;
    MF_HIP_TRY(hipMalloc(&d, 3 * sizeof(uint64_t)));
    hipError_t e = hipMemset(d, 0, 3 * sizeof(uint64_t));
    int rc = e == hipSuccess ? launch_selftest_fast64(n, seed, (unsigned long long*)d, nullptr) : hip_fail(e, "hipMemset");
    if (rc == MF_OK) rc = hip_fail(hipMemcpy(counters, d, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

int mf_selftest_fast64_margin(uint64_t n, uint64_t seed, double* max_ulps)
{
    if (!max_ulps) { set_error("mf_selftest_fast64_margin: null"); return MF_ERR_INVALID_ARG; }
    void* d = nullptr;
    MF_HIP_TRY(hipMalloc(&d, 4 * sizeof(uint64_t)));
    hipError_t e = hipMemset(d, 0, 4 * sizeof(uint64_t));
    int rc = e == hipSuccess ? launch_selftest_fast64(n, seed, (unsigned long long*)d, nullptr, (unsigned long long*)d + 3) : hip_fail(e, "hipMemset");
    if (rc == MF_OK) rc = hip_fail(hipMemcpy(max_ulps, (const uint64_t*)d + 3, sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

// ---- host-buffer wrappers ------------------------------------------------------------------------

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};
struct Stream {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};
struct Event {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
};
}  // namespace

int mf_jacobi_f64_host(const double* b, double* x, const double* taps, const double* lam,
                       const double* inv_on, int F, int S, int omega, int iters, float* kernel_ms)
{
    if (!b || !x || !taps || !lam || !inv_on) { set_error("mf_jacobi_f64_host: null pointer"); return MF_ERR_INVALID_ARG; }
    if (F <= 0 || S <= 0 || omega <= 0) { set_error("mf_jacobi_f64_host: bad sizes"); return MF_ERR_INVALID_ARG; }
    const size_t nb = (size_t)F * S * sizeof(double);
    DevBuf db, dx, dt, dl, di;
    Stream st; Event e0, e1;
    MF_HIP_TRY(hipStreamCreate(&st.s));
    MF_HIP_TRY(hipEventCreate(&e0.e));
    MF_HIP_TRY(hipEventCreate(&e1.e));
    MF_HIP_TRY(db.alloc(nb)); MF_HIP_TRY(dx.alloc(nb));
    MF_HIP_TRY(dt.alloc((2 * omega + 1) * sizeof(double)));
    MF_HIP_TRY(dl.alloc(F * sizeof(double))); MF_HIP_TRY(di.alloc(F * sizeof(double)));
    MF_HIP_TRY(hipMemcpyAsync(db.p, b, nb, hipMemcpyHostToDevice, st.s));
    MF_HIP_TRY(hipMemcpyAsync(dt.p, taps, (2 * omega + 1) * sizeof(double), hipMemcpyHostToDevice, st.s));
    MF_HIP_TRY(hipMemcpyAsync(dl.p, lam, F * sizeof(double), hipMemcpyHostToDevice, st.s));
    MF_HIP_TRY(hipMemcpyAsync(di.p, inv_on, F * sizeof(double), hipMemcpyHostToDevice, st.s));
    MF_HIP_TRY(hipEventRecord(e0.e, st.s));
    int rc = mf_jacobi_f64((const double*)db.p, (double*)dx.p, (const double*)dt.p, (const double*)dl.p,
                           (const double*)di.p, F, S, omega, iters, st.s);
    if (rc != MF_OK) return rc;
    MF_HIP_TRY(hipEventRecord(e1.e, st.s));
    MF_HIP_TRY(hipMemcpyAsync(x, dx.p, nb, hipMemcpyDeviceToHost, st.s));
    MF_HIP_TRY(hipStreamSynchronize(st.s));
    if (kernel_ms) MF_HIP_TRY(hipEventElapsedTime(kernel_ms, e0.e, e1.e));
    return MF_OK;
}

}  // extern "C"
