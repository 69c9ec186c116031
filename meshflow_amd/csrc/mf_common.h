// Shared declarations of libmeshflow_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/meshflow_hip.h"

namespace mf {

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define MF_HIP_TRY(expr)                                   \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return mf::hip_fail(_e, #expr); \
    } while (0)

// Compact per-cell bounding box that follows the records in the cell table.
struct alignas(8) CellBox { int16_t x0, y0, x1, y1; };

inline size_t table_records(int n, int R, int C) { return (size_t)n * R * C; }
// wavefronts (64 cells each) the cell-table kernel spends on one frame = reach slots per frame
__host__ __device__ inline int reach_parts(int R, int C) { return (R * C + 63) / 64; }

// Layout of the cell table blob (mf_cell_table_bytes): records | boxes | edges | uedges | plan | regions | reach | grid.
//   records: n*R*C x MF_CELL_DOUBLES float64      (ABI, include/meshflow_hip.h)
//   boxes:   n*R*C x CellBox                      compact copy of the record's bbox
//   edges:   n*R*C x MF_EDGE_FLOATS float32       4 affine edge functions {a, b, c} scaled by their error bound, then the 4 bounds
//   uedges:  n*R*C x MF_UEDGE_FLOATS float32      the same 4 functions in units of 1/32 pixel (what the plan kernel classifies with)
//   plan:    n x ceil(H/8) x ceil(W/32) x 16 B    per 32x8-pixel footprint: candidate cells, descending
//   regions: n x ceil(H/8) x ceil(W/32) x 8 B     per footprint: source region the warp kernel stages in LDS
//   reach:   n x reach_parts(R, C) x 4 int32      per frame and cell-table wavefront: max extent of a box beyond its grid rect
//   grid:    (C+1) + (R+1) int32                  vertex x / y pixel coordinates
//   bounds:  4 int32                              clip-level rectangle {left, top, right, bottom} of the table's frames: set to the defaults
//                                                 by the cell-table kernel, folded into by every warp / crop-scan launch on the table
#define MF_EDGE_FLOATS 16
#define MF_UEDGE_FLOATS 12
#define MF_FOOT_W 32
#define MF_FOOT_H 8
// Plan entry (uint16): bits 0-11 cell index, bit 14 = entry valid, bit 15 = IN (every pixel of the footprint
// passes the cell's mask test).  Up to 8 entries in descending cell order; the list ends at the first IN
// entry or the first invalid one.  Entry 7 == 0xFFFF: too many candidates -- entries 0-3 then hold the
// cell range r_lo, r_hi, c_lo, c_hi and the warp kernel tests every cell of the range.
// Lists of at most 4 entries carry an edge code per entry in e[4 + i] (bit 15 set, bit 14 clear), bits 0-5: 0-3 = of the
// cell's four mask-edge functions only this one can fail inside the footprint (the others are > +1 at all four
// corners); 4 = test all four; 8 | a | b << 4 = only edges a and b can fail (a < b).
#define MF_PLAN_CODES 0x8000u
#define MF_PLAN_VALID 0x4000u
#define MF_PLAN_IN 0x8000u
#define MF_PLAN_OVERFLOW 0xFFFFu
// A list that consists of ONE IN entry leaves entry 1 unused (bit 14 clear); its bit 0 then certifies the cell's projective
// denominator on this footprint: 0.52 < w < 1.9 at the four corners (hence on every pixel: w is affine) and |h6| <= 0.9 * 2.5e-4 *
// min(w)^2, the condition of the warp kernel's reciprocal guess -- the kernel skips both per-pixel tests.
#define MF_PLAN_UNIT 0x0001u
// ... and MF_PLAN_HOT (only with UNIT) that the footprint needs nothing else either: it lies completely inside the frame and its source
// region is STAGED and DEEP (below).  The warp kernel then runs its straight-line path: no lane masks, no per-pixel checks.
// (bit 13: clear in every valid entry -- cell indices take bits 0-11 -- and in the raw row / column numbers of an overflow list, so
// the kernel tests this one bit without looking at the rest of the list)
#define MF_PLAN_HOT 0x2000u
// ... and MF_PLAN_FAST64 (only with HOT) the premises of the warp kernel's cheap float64 coordinate chain (warp_coords.h,
// cell_coords_fast): at every pixel of the footprint |h0| x + |h1| y + |h2| <= 8 (h0 x + h1 y + h2), the same for the second row,
// and |h6| x + |h7| y + |h8| <= 2.5.
#define MF_PLAN_FAST64 0x0002u
// ... and MF_PLAN_BORDER in the same unused entry 1 of a ONE-entry list (with or without UNIT / IN; never with HOT): the "border" path of the
// warp kernel.  The single candidate is IN or MIXED with a one- / two-edge code (e[4]), its denominator is certified like UNIT's, the
// footprint is whole, and its region is STAGED | BORDER (below): every tap of every COVERED pixel lies in the window or on the one
// ring of pixels around the frame that the kernel paints into the window in the border colour -- so these footprints (the ring along
// the frame border of a stabilised clip, ~3 % of all) run the staged gather instead of clamped taps + selects.
#define MF_PLAN_BORDER 0x1000u          // (bit 12: clear in the raw row / column numbers of an overflow list, like bit 13)
// A list of exactly TWO cells leaves entries 2 and 3 unused; MF_PLAN_HOT in entry 2 then certifies the "pair" shape: the first
// (later, winning) cell is MIXED with ONE mask edge that can fail inside the footprint (its code in e[4]); whatever it does not take
// belongs to the second cell (which is IN, or single-edge with the pair covering every pixel); both denominators stay in
// (0.52, 1.9); the footprint is whole and its region STAGED and DEEP.  The kernel decides ownership with one float32 edge function
// per pixel and never looks at the second cell's edges.
// A short list (2-4 cells) whose MIXED entries all have a one- or two-edge code carries MF_PLAN_HOT in its first edge-code word e[4]
// (bits 6-7 of that word: entries - 1) when the footprint is whole, its region STAGED and interior (every tap two pixels inside the
// frame) and every denominator in (0.52, 1.9): the "multi" path of the kernel -- ownership from the coded edges only, coverage
// checked at run time (a pixel without owner sends the wavefront to the general code).
// ... and in the same entry 2: MF_PLAN_PAIR_FAST = BOTH cells satisfy the premises of the cheap coordinate chain (MF_PLAN_FAST64's),
// so the kernel may take its lane-uniform form of the pair
// path; MF_PLAN_PAIR_VERT = the deciding edge is closer to vertical than to horizontal: transposed lanes (a lane = 1 column x 4 rows).
#define MF_PLAN_PAIR_FAST 0x0001u
#define MF_PLAN_PAIR_VERT 0x0002u
// ... and bit 12 of the first edge-code word e[4] (next to its MF_PLAN_HOT = the multi path): every listed cell satisfies those premises.
#define MF_PLAN_MULTI_FAST 0x1000u
#define MF_PLAN_COUNT_SHIFT 6
struct alignas(16) FootPlan { uint16_t e[8]; };
// Source region of a footprint (FootRegion).  STAGED: every bilinear tap of every pixel of the footprint lies in columns sx0 ..
// sx0+MF_STAGE_COLS-1 and rows sy0 .. sy0+MF_STAGE_ROWS-1 of the source frame, and rows sy0 .. sy0+MF_STAGE_ROWS are inside the
// frame.  The warp kernel then copies MF_STAGE_CHUNKS 16-byte chunks (rows of MF_STAGE_PITCH bytes starting at the dword that
// holds column sx0, byte bs = 3 sx0 & ~3 of the row) into LDS with two global->LDS loads per lane and reads the taps from there.
// What the kernel needs is stored ready-made (the scalar unit is as busy as the vector unit there):
//   flags_origin: bit 31 STAGED, bit 30 DEEP, bits 0-22 origin = MF_STAGE_PITCH sy0 + bs  (tap (ix, iy) sits at LDS byte
//                 MF_STAGE_PITCH iy + 3 ix - origin of the window)
//   src_dwords:   (row_bytes sy0 + bs) / 4, the window's first dword in the frame (a frame is below 4 GB)
struct alignas(8) FootRegion { uint32_t flags_origin, src_dwords; };
#define MF_REGION_ORIGIN_MASK 0x007FFFFFu
#define MF_STAGE_PITCH 160
#define MF_STAGE_ROWS 12
#define MF_STAGE_COLS 52
#define MF_REGION_STAGED 0x80000000u
// bit 30 = DEEP (only with STAGED): the candidate list ends with an IN cell, or consists of two single-edge cells whose masks
// provably overlap across the footprint (either way every pixel has an owner), and the region
// stays two pixels inside the frame, so the warp kernel needs neither the interior check nor the crop flags.
#define MF_REGION_DEEP 0x40000000u
// bit 29 = COMPACT (only on the certified shapes -- HOT, PAIR, MULTI footprints: whole, interior, STAGED, NOFLAG; DEEP unless the multi path has
// to check coverage): every tap of every pixel, whichever listed cell owns it, lies in MF_COMPACT_ROWS rows of MF_COMPACT_PITCH bytes
// starting at the dword that holds column sx0 of row sy0 -- 63 chunks of 16 bytes, ONE global->LDS load per wavefront; origin and
// src_dwords then refer to that layout (origin = MF_COMPACT_PITCH sy0 + bs).  The warp kernel maps lanes to footprint rows differently
// on such a window (rows 0, 2, 4, 6 in lanes 0-31: no LDS bank conflicts at this pitch, warp_body.h).
#define MF_REGION_COMPACT 0x20000000u
#define MF_COMPACT_PITCH 112
// bit 28 = NOFLAG (with or without STAGED): no pixel of the footprint can pass one of the four crop-boundary tests of mfs.py:1075-1098
// -- every source coordinate any listed cell can give it lies more than one pixel inside the frame's first / last column and row --
// so the scan-only pass (crop_scan_kernel, warp.hip) skips it.  DEEP implies it.
#define MF_REGION_NOFLAG 0x10000000u
// bit 27 = BORDER (only with STAGED, never with DEEP): the window of a border-path footprint (MF_PLAN_BORDER).  Rows sy0 .. sy0 + 11 lie
// inside the frame (sy0 <= H - 12: the kernel does not fetch a 13th row for it); bits 23-26 say which pixels just OUTSIDE the frame the
// taps can reach and the kernel therefore paints in the border colour after the copy: column -1 (the three bytes in front of each
// window row; the window then starts at byte 0 of the frame rows and needs no column beyond 51), column W (the three bytes behind
// column W-1; the window then ends with the frame rows), row -1 (the LDS row in front of the window, sy0 = 0), row H (the row behind
// it, sy0 = H - 12).
#define MF_REGION_BORDER 0x08000000u
#define MF_REGION_PAINT_LEFT 0x04000000u
#define MF_REGION_PAINT_RIGHT 0x02000000u
#define MF_REGION_PAINT_TOP 0x01000000u
#define MF_REGION_PAINT_BOTTOM 0x00800000u
#define MF_COMPACT_ROWS 9
#define MF_STAGE_CHUNKS 128            // two 16-byte chunks per lane: 12 rows x 10 chunks + 8 chunks of a 13th row (unused)
struct TableView {
    double* records; CellBox* boxes; float* edges; float* uedges; FootPlan* plan; FootRegion* regions; int32_t* reach; int32_t* grid; int32_t* bounds;
};
inline size_t plan_count(int n, int W, int H)
{
    return (size_t)n * ((H + MF_FOOT_H - 1) / MF_FOOT_H) * ((W + MF_FOOT_W - 1) / MF_FOOT_W);
}
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t plan_offset(int n, int R, int C)
{
    return align16(table_records(n, R, C) * (MF_CELL_DOUBLES * sizeof(double) + sizeof(CellBox) + (MF_EDGE_FLOATS + MF_UEDGE_FLOATS) * sizeof(float)));
}
inline size_t table_bytes(int n, int W, int H, int R, int C)
{
    return plan_offset(n, R, C) + plan_count(n, W, H) * (sizeof(FootPlan) + sizeof(FootRegion)) +
           (size_t)n * reach_parts(R, C) * 4 * sizeof(int32_t) + (size_t)(R + C + 2) * sizeof(int32_t) + 4 * sizeof(int32_t);
}
inline TableView table_view(void* blob, int n, int W, int H, int R, int C);
// The part of a table that belongs to frames f0 ... (the per-frame sections advanced, the vertex grid shared): what launch_warp /
// launch_crop_scan need to work on a chunk of a clip whose table was built in one go.
inline TableView table_slice(const TableView& t, int f0, int W, int H, int R, int C)
{
    TableView v = t;
    const size_t rec = table_records(f0, R, C), fp = (size_t)f0 * ((H + MF_FOOT_H - 1) / MF_FOOT_H) * ((W + MF_FOOT_W - 1) / MF_FOOT_W);
    v.records += rec * MF_CELL_DOUBLES; v.boxes += rec; v.edges += rec * MF_EDGE_FLOATS; v.uedges += rec * MF_UEDGE_FLOATS;
    v.plan += fp; v.regions += fp; v.reach += (size_t)f0 * reach_parts(R, C) * 4;
    return v;
}
inline TableView table_view(void* blob, int n, int W, int H, int R, int C)
{
    const size_t nrec = table_records(n, R, C);
    TableView v;
    v.records = (double*)blob;
    v.boxes = (CellBox*)(v.records + nrec * MF_CELL_DOUBLES);
    v.edges = (float*)(v.boxes + nrec);
    v.uedges = v.edges + nrec * MF_EDGE_FLOATS;
    v.plan = (FootPlan*)((char*)blob + plan_offset(n, R, C));
    v.regions = (FootRegion*)(v.plan + plan_count(n, W, H));
    v.reach = (int32_t*)(v.regions + plan_count(n, W, H));
    v.grid = v.reach + (size_t)n * reach_parts(R, C) * 4;
    v.bounds = v.grid + (R + C + 2);
    return v;
}

// a.lo * b.lo + a.hi * b.hi + c on 16-bit halves (v_dot2_u32_u16): the horizontal lerp of the warp's and the crop-resize's uint8 blends
__device__ __forceinline__ uint32_t udot2(uint32_t a, uint32_t b, uint32_t c)
{
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_udot2(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b), c, false);
}

// n / d for n < 2^31 as (n * m) >> (32 + s), m = ceil(2^(31 + ceil(log2 d)) / d): exact because the excess m d - 2^p is below
// d <= 2^(p - 31).  d == 1 is passed through.
struct FastDiv {
    uint32_t d, m, s;
    __device__ __forceinline__ uint32_t quotient(uint32_t n) const { return d == 1u ? n : (__umulhi(n, m) >> s); }
};
inline FastDiv make_fast_div(uint32_t d)
{
    FastDiv f;
    f.d = d; f.m = 0; f.s = 0;
    if (d > 1u) {
        uint32_t l = 0;
        while ((1ull << l) < d) ++l;                       // ceil(log2 d) >= 1
        const unsigned p = 31u + l;
        f.m = (uint32_t)(((1ull << p) + d - 1) / d);
        f.s = l - 1u;
    }
    return f;
}
// XCD-aware tile order (workgroups go to the 8 XCDs round-robin by linear id, each XCD has its own L2): workgroup L of a
// 1-D grid of 8 * per_xcd takes tile (L % 8) * per_xcd + L / 8, so every XCD sweeps one contiguous eighth of the tiles
// in raster order and rows shared by neighbouring tiles are fetched once per L2.  tile -> (frame, tile row, tile col).
struct TileOrder {
    uint32_t tiles, per_xcd;
    FastDiv by_frame, by_row;
    __device__ __forceinline__ bool decode(uint32_t block, int& f, int& ty, int& tx) const
    {
        const uint32_t tile = (block & 7u) * per_xcd + (block >> 3);
        if (tile >= tiles) return false;
        f = (int)by_frame.quotient(tile);
        const uint32_t in_frame = tile - (uint32_t)f * by_frame.d;
        ty = (int)by_row.quotient(in_frame);
        tx = (int)(in_frame - (uint32_t)ty * by_row.d);
        return true;
    }
};
inline bool make_tile_order(int tiles_x, int tiles_y, int n, TileOrder& o)
{
    const long long tiles = (long long)tiles_x * tiles_y * n;
    if ((tiles + 7) / 8 * 8 > 0x7FFFFFFFll) return false;
    o.tiles = (uint32_t)tiles;
    o.per_xcd = (uint32_t)((tiles + 7) / 8);
    o.by_frame = make_fast_div((uint32_t)(tiles_x * tiles_y));
    o.by_row = make_fast_div((uint32_t)tiles_x);
    return true;
}



// Pixel format of a frame stack: the _u8c3 / _u16c3 / _u8c1 / _u8c4 calls of include/meshflow_hip.h.  Every layer takes the format as this
// one parameter; a new format is a row here plus its kernels.
// Px::MAPS is no frame format: the warp that reads no frame and writes the float32 coordinate maps (u, v) themselves, [H][W][2] per
// frame (mf_warp_maps_f32, warp_maps.hip) -- "2 channels of 4 bytes" as far as launch_warp's frame stride goes.
// Px::PLANE_*: no picture either -- the side planes [n][H][W] that travel with a video (mf_warp_plane_f32, mf_warp_plane_nearest,
// warp_planes.hip): float32 sampled like cv2.remap INTER_LINEAR of CV_32FC1, or elements of 1, 2, 4 or 8 bytes copied as bits like
// INTER_NEAREST.  One channel of px_sample_bytes bytes; the pixel calls (launch_crop_resize*, the clip and host pipelines) never see them.
// Px::NV12_UV: the interleaved half-resolution chroma plane of an NV12 clip (mf_warp_nv12, warp_nv12.hip): [n][H/2][W/2] pixels of two bytes,
// U first, sampled at half the luma coordinates of the even luma pixels.  W and H stay the LUMA frame's everywhere (the cell table's); only
// launch_warp's frame stride (px_frame_bytes) and the kernel's tail know the plane's own size.  The luma plane is a Px::U8C1 stack.
// Px::U16C1: the luma planes of a P010 / P012 / P016 clip (mf_warp_p010, warp_c1_16.hip): [n][H][W] uint16 samples, sampled like channel 0 of a
// Px::U16C3 stack (cv2.remap of CV_16UC1).  No public frame format: only the P010 entries launch it.
// Px::P010_UV: the interleaved half-resolution chroma plane of such a clip (warp_p010.hip): [n][H/2][W/2] pixels of two uint16 samples, U
// first -- Px::NV12_UV's geometry and lane mapping with Px::U16C3's arithmetic.
// Px::NV16_UV: the interleaved half-WIDTH chroma plane of an NV16 (4:2:2) clip (mf_warp_nv16, warp_nv16.hip): [n][H][W/2] pixels of two bytes, U
// first, sampled at (u / 2, v) of the even luma pixels of every row; H of either parity.  Luma: Px::U8C1.
// Px::P210_UV: the interleaved half-WIDTH chroma plane of a P210 / P212 / P216 (10-bit 4:2:2) clip (mf_warp_p210, warp_p210.hip): [n][H][W/2]
// pixels of two uint16 samples, U first -- Px::NV16_UV's geometry (every row emits, only x is halved, H of either parity) with Px::P010_UV's
// arithmetic and border word.  Luma: Px::U16C1.
enum class Px { U8C3, U16C3, U8C1, U8C4, MAPS, PLANE_F32, PLANE_N1, PLANE_N2, PLANE_N4, PLANE_N8, NV12_UV, U16C1, P010_UV, NV16_UV, P210_UV };
// (the interleaved chroma plane of a semi-planar clip, and the ones with as many rows as luma)
constexpr bool px_is_chroma(Px p) { return p == Px::NV12_UV || p == Px::P010_UV || p == Px::NV16_UV || p == Px::P210_UV; }
constexpr bool px_is_chroma422(Px p) { return p == Px::NV16_UV || p == Px::P210_UV; }
constexpr bool px_is_plane(Px p) { return p == Px::PLANE_F32 || p == Px::PLANE_N1 || p == Px::PLANE_N2 || p == Px::PLANE_N4 || p == Px::PLANE_N8; }
constexpr int px_channels(Px p)
{
    return p == Px::U8C1 || p == Px::U16C1 || px_is_plane(p) ? 1 : p == Px::U8C4 ? 4 : p == Px::MAPS || px_is_chroma(p) ? 2 : 3;
}
// (the formats whose samples, and border samples, are uint16)
constexpr bool px_is_u16(Px p) { return p == Px::U16C3 || p == Px::U16C1 || p == Px::P010_UV || p == Px::P210_UV; }
constexpr int px_sample_bytes(Px p)
{
    return px_is_u16(p) || p == Px::PLANE_N2 ? 2 : p == Px::MAPS || p == Px::PLANE_F32 || p == Px::PLANE_N4 ? 4 : p == Px::PLANE_N8 ? 8 : 1;
}
constexpr int px_bytes(Px p) { return px_channels(p) * px_sample_bytes(p); }
constexpr const char* px_name(Px p)
{
    return p == Px::U8C3 ? "u8c3" : p == Px::U16C3 ? "u16c3" : p == Px::U8C1 ? "u8c1" : p == Px::U8C4 ? "u8c4" : p == Px::MAPS ? "maps_f32" :
           p == Px::PLANE_F32 ? "plane_f32" : p == Px::NV12_UV ? "nv12_uv" : p == Px::U16C1 ? "u16c1" : p == Px::P010_UV ? "p010_uv" : p == Px::NV16_UV ? "nv16_uv" : p == Px::P210_UV ? "p210_uv" : "plane_nearest";
}
// Bytes of one frame of a stack of format p in a clip of W x H (luma) pixels: launch_warp's frame stride.  A chroma plane has W / 2 pixels a row (W
// even) and H / 2 rows (NV12, P010: H even) or H rows (NV16, P210: H of either parity); everything else has W H pixels.
constexpr size_t px_frame_bytes(Px p, int W, int H)
{
    const bool chroma = px_is_chroma(p);
    return (size_t)(chroma ? W / 2 : W) * (size_t)(chroma && !px_is_chroma422(p) ? H / 2 : H) * (size_t)px_bytes(p);
}
static_assert(px_frame_bytes(Px::NV12_UV, 6, 4) == 12 && px_frame_bytes(Px::P010_UV, 6, 4) == 24, "4:2:0 chroma: (W / 2) (H / 2) pixels of 2 or 4 bytes");
static_assert(px_frame_bytes(Px::NV16_UV, 6, 3) == 18 && px_frame_bytes(Px::U8C3, 6, 3) == 54, "4:2:2 chroma: (W / 2) H pixels of 2 bytes; a frame: W H pixels");
static_assert(px_frame_bytes(Px::P210_UV, 6, 3) == 36 && px_frame_bytes(Px::U16C1, 6, 3) == 36, "10-bit 4:2:2: chroma (W / 2) H pixels of 4 bytes, as many bytes as luma");
// The border colour as the warp kernels take it, from the caller's px_channels(p) samples: B | G << 8 | R << 16 (u8c3),
// B | G << 16 | R << 32 (u16c3), the byte (u8c1), B | G << 8 | R << 16 | A << 24 (u8c4), U | V << 8 (nv12_uv, nv16_uv), the sample (u16c1), U | V << 16 (p010_uv, p210_uv).
inline uint64_t pack_border(Px p, const void* samples)
{
    uint64_t v = 0;
    for (int c = 0; c < px_channels(p); ++c)
        v |= (px_is_u16(p) ? (uint64_t)((const uint16_t*)samples)[c] : (uint64_t)((const uint8_t*)samples)[c]) << (8 * px_sample_bytes(p) * c);
    return v;
}

// Launch constants of the warp kernel (host-made: the kernel's scalar unit has none to spare).  Grid = (8 * per_xcd, frames): the
// workgroups of a frame go to the 8 XCDs round-robin by blockIdx.x, workgroup L takes footprint (L % 8) * per_xcd + L / 8, so
// every XCD sweeps one contiguous eighth of each frame in raster order.  All table offsets are 32-bit: launch_warp cuts a clip
// that would overflow them into several launches.
struct WarpGeom {
    uint32_t per_frame, per_xcd, nfx;            // footprints per frame, per XCD and frame, per row
    uint32_t div_m, div_s, div_pass;             // t / nfx = (mulhi(t, div_m) + (t & div_pass)) >> div_s
    uint32_t frame_bytes, row_bytes;             // 3 W H, 3 W
    uint32_t rec_frame_bytes, edge_frame_bytes;  // R C records / edge sets of one frame
    uint32_t cell_mul_x, cell_mul_y, mesh_cols, cell_last;   // the cell under a pixel of the UNWARPED grid: (mulhi(x, cell_mul_x), mulhi(y, cell_mul_y));
                                                 // row length C; R C - 1 (the speculative matrix load of the hot path, warp_body.h)
};

// Launchers (defined next to their kernels).
int launch_jacobi(const double* b, double* x, const double* taps, const double* lam, const double* inv_on,
                  int F, int S, int omega, int iters, hipStream_t st);
int launch_cell_table(const double* unstab, const double* stab, int n, int W, int H, int R, int C,
                      const TableView& tv, int32_t* crop, int32_t* status, hipStream_t st, bool first_of_table = true);
// (first_of_table: this launch also resets the table's clip-level rectangle -- false for the later frame ranges of a table that is
// built in several launches)
// warp.hip: the mesh warp of n frames of format px (border: pack_border's word), cut into launches of at most 65,535 frames
int launch_warp(Px px, const void* frames, void* out, const TableView& tv, int n, int W, int H, int R, int C,
                uint64_t border, int32_t* crop, hipStream_t st);
// One launch of launch_warp: frames f0 .. f0 + m - 1, every pointer already advanced to frame f0.
struct WarpRange {
    const FootPlan* plan; const FootRegion* regions; const double* records; const float* edges;
    const void* frames; void* out; int32_t* crop; int32_t* bounds; int m;
};
void launch_warp8c1_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border, bool stage, hipStream_t st);  // warp_c1.hip
void launch_warp8c4_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border, bool stage, hipStream_t st);  // warp_c4.hip
void launch_maps_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, hipStream_t st);  // warp_maps.hip (r.frames unused, r.out: float32 maps)
void launch_plane_range(Px px, const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint64_t fill, hipStream_t st);  // warp_planes.hip (fill: the element's bits)
void launch_nv12_chroma_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border_uv, hipStream_t st);  // warp_nv12.hip (r.crop, r.bounds unused)
void launch_nv16_chroma_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border_uv, hipStream_t st);  // warp_nv16.hip (r.crop, r.bounds unused)
void launch_warp16c1_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border, hipStream_t st);  // warp_c1_16.hip
void launch_p010_chroma_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border_uv, hipStream_t st);  // warp_p010.hip (r.crop, r.bounds unused)
void launch_p210_chroma_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border_uv, hipStream_t st);  // warp_p210.hip (r.crop, r.bounds unused)
int launch_crop_scan(const TableView& tv, int n, int W, int H, int R, int C, int32_t* crop, hipStream_t st);
int check_d16_zero_fill(hipStream_t st);          // warp.hip: one-time device check the byte-tap kernels rely on
int launch_selftest_recip(unsigned long long n, unsigned long long seed, unsigned long long* d_mismatches, hipStream_t st);
int launch_selftest_fast64(unsigned long long n, unsigned long long seed, unsigned long long* d_counters, hipStream_t st, unsigned long long* d_margin = nullptr);
size_t crop_resize_workspace_bytes(int W, int H);
// resize.hip: every check of a crop-resize call, then the format's tables and kernel
int launch_crop_resize(Px px, const void* frames, void* out, int n, int W, int H, int left, int top, int right,
                       int bottom, void* work, hipStream_t st);
// resize_tables_kernel's tables (u8c3, u8c1) for the rectangle in `work` (W x-entries, then H y-entries; x: ofs = sx, w = 16 a0 | 16 a1 << 16
// (pre-scaled, see resize_kernel);  y: ofs = sy0 | sy1 << 16, w = b0 | b1 << 16)
struct ResizeTab { int32_t ofs; uint32_t w; };
// resize16_tables_kernel's (resize16_body.h): x: ofs = sx (clamped into the crop), f = its fraction (0 where clamped);  y: ofs = sy0 | sy1 << 16
// (clipped rows), f = the fraction
struct Resize16Tab { int32_t ofs; float f; };
static_assert(sizeof(Resize16Tab) == 8, "the 8-bit call's workspace holds the tables");
// resize.hip: every check of a crop-resize call to an oW x oH output, then the format's tables and kernel (oW x oH == W x H: launch_crop_resize)
int launch_crop_resize_to(Px px, const void* frames, void* out, int n, int W, int H, int left, int top, int right, int bottom, int oW, int oH,
                          void* work, hipStream_t st);
// What those two launch behind their checks (the host units of the kernel headers; `up`: oW >= cw and oH >= ch, which instantiation):
// resize16.hip: resize16_body.h's tables of the cw x ch crop for oW x oH in the same workspace, then resize16_kernel (oW x oH == W x H) or
// resize16_to_kernel
int launch_resize16(const uint16_t* frames, uint16_t* out, int W, int H, int left, int top, int cw, int ch, int oW, int oH,
                    const TileOrder& order, void* work, hipStream_t st);
// resize_c1.hip: resize8c1_kernel, or resize8c1_to_kernel for an oW x oH output, on resize.hip's tables (already built in `work`), and their
// tile rows
int launch_resize8c1(const uint8_t* frames, uint8_t* out, int n, int W, int H, int left, int top, int cw, const void* work,
                     const TileOrder& order, hipStream_t st);
int launch_resize8c1_to(const uint8_t* frames, uint8_t* out, int n, int W, int H, int left, int top, int cw, int oW, int oH, bool up,
                        const void* work, const TileOrder& order, hipStream_t st);
int resize8c1_tile_rows(bool up);
// resize_c4.hip: the u8c4 kernels on resize.hip's tables for an oW x oH output (oW x oH == W x H: the same-size call), and their tile rows
int launch_resize8c4(const uint8_t* frames, uint8_t* out, int n, int W, int H, int left, int top, int cw, int oW, int oH, bool up,
                     const void* work, const TileOrder& order, hipStream_t st);
int resize8c4_tile_rows(bool up);
// resize.hip: every format's output rows per tile, and whether the widest span of 256 output pixels fits a staged row (which `down`
// instantiation a launcher picks)
int resize_to_tile_rows(Px px, bool up);
bool resize_span_fits(int cw, int oW, int px_bytes, int slack, int pitch);
// resize_dev.hip: mf_crop_resize_dev_*: the host-side checks, then the tables and the kernels that read the rectangle from d_bounds
int launch_crop_resize_dev(Px px, const void* frames, void* out, int n, int W, int H, const int32_t* d_bounds, int oW, int oH, void* work,
                           int32_t* d_status, hipStream_t st);
// resize_planes.hip / resize_planes_dev.hip: mf_crop_resize_plane_* and mf_crop_resize_dev_plane_* -- every check of the call, the tables,
// the kernel.  elem_bytes == 0: the float32 linear call; 1, 2, 4, 8: the nearest one on elements of that size.
int launch_crop_resize_plane(int elem_bytes, const void* planes, void* out, int n, int W, int H, int left, int top, int right, int bottom,
                             int oW, int oH, void* work, hipStream_t st);
int launch_crop_resize_plane_dev(int elem_bytes, const void* planes, void* out, int n, int W, int H, const int32_t* d_bounds, int oW, int oH,
                                 void* work, int32_t* d_status, hipStream_t st);
// resize_uv.hip / resize_uv_dev.hip: the chroma half of mf_crop_resize_nv12 / mf_crop_resize_dev_nv12 (W, H, oW, oH and the rectangle are the
// LUMA frame's; `tabs`: the chroma tables' part of the workspace, behind the luma tables) -- resize_uv_body.h's tables, then its kernel.  The
// calls' checks are capi.hip's; resize_uv_tile_order: the kernel's tiles (false: too many).
size_t crop_resize_nv12_workspace_bytes(int oW, int oH);
bool resize_uv_tile_order(int oW, int oH, int n, TileOrder& order);
int launch_resize_uv(const uint8_t* uv, uint8_t* out_uv, int W, int H, int left, int top, int right, int bottom, int oW, int oH, void* tabs,
                     const TileOrder& order, hipStream_t st);
int launch_resize_uv_dev(const uint8_t* uv, uint8_t* out_uv, int W, int H, const int32_t* d_bounds, int oW, int oH, void* tabs,
                         const TileOrder& order, hipStream_t st);
// resize_uv422.hip / resize_uv422_dev.hip: the chroma half of mf_crop_resize_nv16 / mf_crop_resize_dev_nv16, the same way -- resize_uv422_body.h's
// x tables in `tabs` (behind the luma tables), then its kernel on them and on `luma_ytab`, the y table the luma call has just built (oH entries)
size_t crop_resize_nv16_workspace_bytes(int oW, int oH);
bool resize_uv422_tile_order(int oW, int oH, int n, TileOrder& order);
int launch_resize_uv422(const uint8_t* uv, uint8_t* out_uv, int W, int H, int left, int top, int right, int bottom, int oW, int oH,
                        const void* luma_ytab, void* tabs, const TileOrder& order, hipStream_t st);
int launch_resize_uv422_dev(const uint8_t* uv, uint8_t* out_uv, int W, int H, const int32_t* d_bounds, int oW, int oH, const void* luma_ytab,
                            void* tabs, const TileOrder& order, hipStream_t st);
// resize16.hip / resize_dev.hip: resize16_tables_kernel's / resize16_tables_dev_kernel's tables for (oW, oH) in `work`, on their own
int launch_resize16_tables(int cw, int ch, int oW, int oH, void* work, hipStream_t st);
int launch_resize16_tables_dev(const int32_t* d_bounds, int W, int H, int oW, int oH, void* work, int32_t* d_status, hipStream_t st);
// resize_hdr.hip / resize_hdr_dev.hip: mf_crop_resize_p010 / mf_crop_resize_dev_p010 behind capi.hip's checks (W, H, oW, oH and the rectangle are
// the LUMA frame's; `work`: the luma tables, then the chroma tables) -- the luma tables above, resize_hdr_body.h's luma kernel, its chroma
// tables and its chroma kernel.  resize_hdr_tile_orders: the two kernels' tiles (false: too many).
size_t crop_resize_p010_workspace_bytes(int oW, int oH);
bool resize_hdr_tile_orders(int oW, int oH, int n, TileOrder& luma, TileOrder& chroma);
int launch_resize_hdr(const uint16_t* y, const uint16_t* uv, uint16_t* out_y, uint16_t* out_uv, int W, int H, int left, int top, int right,
                      int bottom, int oW, int oH, void* work, const TileOrder& luma, const TileOrder& chroma, hipStream_t st);
int launch_resize_hdr_dev(const uint16_t* y, const uint16_t* uv, uint16_t* out_y, uint16_t* out_uv, int W, int H, const int32_t* d_bounds, int oW,
                          int oH, void* work, int32_t* d_status, const TileOrder& luma, const TileOrder& chroma, hipStream_t st);
// ... and mf_crop_resize_p210 / mf_crop_resize_dev_p210 (10-bit 4:2:2) in the same two units: the same luma tables and luma kernel, then
// resize_wide422_body.h's x table (oW/2 entries behind the luma tables) and its chroma kernel on the luma call's own y table
size_t crop_resize_p210_workspace_bytes(int oW, int oH);
bool resize_p210_tile_orders(int oW, int oH, int n, TileOrder& luma, TileOrder& chroma);
int launch_resize_p210(const uint16_t* y, const uint16_t* uv, uint16_t* out_y, uint16_t* out_uv, int W, int H, int left, int top, int right,
                       int bottom, int oW, int oH, void* work, const TileOrder& luma, const TileOrder& chroma, hipStream_t st);
int launch_resize_p210_dev(const uint16_t* y, const uint16_t* uv, uint16_t* out_y, uint16_t* out_uv, int W, int H, const int32_t* d_bounds, int oW,
                           int oH, void* work, int32_t* d_status, const TileOrder& luma, const TileOrder& chroma, hipStream_t st);
size_t vertex_motion_workspace_bytes(int total_features, int max_per_pair, int P, int R, int C);
int launch_vertex_motion(const double* early, const double* late, const int32_t* offsets, const double* hom, int P,
                         int total_features, int max_per_pair, int W, int H, int R, int C, int ell_rows, int ell_cols,
                         float* vel, double* disp, void* work, int32_t* status, hipStream_t st);
// online_smooth.hip: mf_online_smooth_f64 behind capi.hip's checks
int launch_online_smooth(const float* vel, const double* lam_known, const double* taps, int n, int S, int omega, int L, int iters,
                         double beta, double lam_newest, long long seen, double* c_state, double* q_state, double* lam_state,
                         double* c_out, double* p_out, hipStream_t st);
// ... and mf_online_smooth_lag_f64: the same launches, the sweep kernel's lagged instantiation
int launch_online_smooth_lag(const float* vel, const double* lam_known, const double* taps, int n, int S, int omega, int L, int lag, int iters,
                             double beta, double lam_newest, long long seen, double* c_state, double* q_state, double* lam_state,
                             double* c_out, double* p_out, hipStream_t st);
// ... and mf_online_smooth_group_f64: K rows of n frames, row r on the state slices of stream ids[r] of B
int launch_online_smooth_group(const float* vel, const double* lam_known, const double* taps, const int32_t* ids, const long long* seen, int K,
                               int B, int n, int S, int omega, int L, int iters, double beta, double lam_newest, double* c_state, double* q_state,
                               double* lam_state, double* c_out, double* p_out, hipStream_t st);
// ... and mf_online_smooth_group_lag_f64: the group's launches, the sweep kernel's lagged twin
int launch_online_smooth_group_lag(const float* vel, const double* lam_known, const double* taps, const int32_t* ids, const long long* seen,
                                   int K, int B, int n, int S, int omega, int L, int lag, int iters, double beta, double lam_newest,
                                   double* c_state, double* q_state, double* lam_state, double* c_out, double* p_out, hipStream_t st);
// cuts.hip: mf_frame_signature_u8, mf_cut_distance_i32 and mf_cut_distance_pairs_i32 behind capi.hip's checks
int launch_frame_signature(const uint8_t* luma, int n, int W, int H, int32_t* sig, hipStream_t st);
int launch_cut_distance(const int32_t* prev, const int32_t* sig, int n, int32_t* dist, hipStream_t st);
int launch_cut_distance_pairs(const int32_t* prev, const int32_t* sig, int n, int32_t* dist, hipStream_t st);
// path_limit.hip: mf_path_limit_f64 behind capi.hip's checks
int launch_path_limit(const double* unstab, const double* stab, int n, int W, int H, int R, int C, int left, int top, int right, int bottom,
                      double guard, int steps, int rise, const int32_t* k_prev, int32_t* k_raw, int32_t* k, double* out, hipStream_t st);
// ... and mf_path_limit_group_f64: K frames of K streams, k_prev [K]
int launch_path_limit_group(const double* unstab, const double* stab, int K, int W, int H, int R, int C, int left, int top, int right, int bottom,
                            double guard, int steps, int rise, const int32_t* k_prev, int32_t* k_raw, int32_t* k, double* out, hipStream_t st);
int launch_selftest_sqrt(unsigned long long n, unsigned long long seed, unsigned long long* d_mismatches, hipStream_t st);
int launch_stability_score(const double* stab, int F, int S, double* ratio, double* score, hipStream_t st);
int launch_crop_reduce(const int32_t* crop, int n, int W, int H, int32_t* bounds, hipStream_t st);

}  // namespace mf
