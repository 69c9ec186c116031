/* meshflow_hip.h -- C ABI of libmeshflow_hip.so (MI355X / gfx950).
 *
 * The reference (how4rd/meshflow, `mfs.py` = meshflowstabilizer.py) is pure Python and has no FFI layer;
 * its drop-in boundary is the pair of private methods called from stabilize() at mfs.py:150-158:
 *
 *   _get_stabilized_vertex_displacements        mfs.py:632-710   -> mf_jacobi_f64
 *   _get_stabilized_frames_and_crop_boundaries  mfs.py:909-1108  -> mf_cell_table_f64 + mf_warp_u8c3
 *
 * and the steps either side of them:
 *
 *   _crop_frames                                mfs.py:1111-1157 -> mf_crop_resize_u8c3
 *   vertex-motion accumulation after the tracker  mfs.py:268-282, 316-362, 365-452 -> mf_vertex_motion_f64
 *   _compute_stability_score                    mfs.py:1216-1259 -> mf_stability_score_f64
 *
 * Every entry point takes plain pointers and sizes.  Pointers named d_* are DEVICE pointers
 * (hipMalloc / torch tensors' data_ptr()); `stream` is a hipStream_t passed as void* (NULL = the
 * default stream).  Kernel entry points are asynchronous on `stream`.  Return value: 0 on success,
 * a negative MF_ERR_* otherwise; mf_last_error() gives a thread-local message.  No CPU fallback
 * exists: without a GPU every compute entry point fails with MF_ERR_HIP.
 *
 * The Python binding is meshflow_amd/_lib.py (ctypes); INTEGRATION.md shows the stub a maintainer of
 * the reference would add.
 */
#ifndef MESHFLOW_HIP_H
#define MESHFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MF_ABI_VERSION 1

#define MF_OK 0
#define MF_ERR_INVALID_ARG (-1)   /* bad size / null pointer / unsupported shape */
#define MF_ERR_HIP (-2)           /* a HIP runtime call failed (see mf_last_error) */
#define MF_ERR_DEGENERATE (-3)    /* a mesh cell has no homography (cv2.findHomography would return None) */

/* Per-cell record written by mf_cell_table_f64 and read by mf_warp_u8c3: MF_CELL_DOUBLES float64.
 *   [0..8]   M    = inverse of the unstabilized->stabilized homography (what cv2.warpPerspective
 *                   evaluates, mfs.py:1041, 1052)
 *   [9..17]  Hi   = stabilized->unstabilized homography (cv2.perspectiveTransform, mfs.py:1042, 1054)
 *   [18..21] rect = L, T, Rt, B: inclusive pixel rect of the unstabilized cell (mfs.py:1045-1048)
 *   [22..25] bbox = x0, y0, x1, y1: inclusive, frame-clamped box outside which the cell's warped mask
 *                   is certainly zero (x0 > x1: empty)
 *   [26]     status: 0 ok, 1 degenerate
 *   [27..31] reserved
 * The table blob of n frames (mf_cell_table_bytes) holds n*R*C records followed by private acceleration
 * data of the warp kernel (compact boxes, edge functions, per-footprint candidate plan and source region, per-frame
 * reach, vertex grid). */
#define MF_CELL_DOUBLES 32
#define MF_CELL_OFF_M 0
#define MF_CELL_OFF_HI 9
#define MF_CELL_OFF_RECT 18
#define MF_CELL_OFF_BBOX 22
#define MF_CELL_OFF_STATUS 26

int mf_abi_version(void);
const char* mf_last_error(void);

/* ---- device plumbing (for hosts that do not bring their own allocator) ---- */
int mf_device_count(int* count);
int mf_set_device(int device);                            /* + the one-time device check of the byte-tap kernels */
int mf_malloc(void** d_ptr, size_t bytes);
int mf_free(void* d_ptr);
int mf_malloc_host(void** h_ptr, size_t bytes);          /* pinned host memory */
int mf_free_host(void* h_ptr);
int mf_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);
int mf_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);
int mf_stream_synchronize(void* stream);

/* ---- kernel 1: Jacobi temporal smoothing (mfs.py:844-878 for every vertex, mfs.py:695-704) ----
 * d_b, d_x: [F][S] float64, frame-major, S = (R+1)*(C+1)*2 independent series (the layout of the
 * reference's (F, R+1, C+1, 2) arrays).  x_start = b (mfs.py:699-703).  `iters` true Jacobi sweeps of
 *   x_new[t] = inv_on[t] * (b[t] + 2*lam[t] * sum_{d=-omega..omega, 0<=t+d<F} taps[d+omega]*x[t+d])
 * i.e. x <- diag(1/on) (b - off x) with off[t,t+d] = -2*lam[t]*taps[d+omega] (band includes d = 0,
 * mfs.py:767-781).  d_taps: [2*omega+1], d_lam, d_inv_on: [F].  d_b and d_x may not alias.
 * Any F, any omega (as the reference: mfs.py:193-213 reads every frame of the file): clips of up to 9,728 frames are swept with the
 * whole time axis of a series in LDS; longer ones in time tiles with a halo of (sweeps per launch) x omega frames -- bit-identical -- which
 * takes ceil(iters / k) launches and, from the second launch on, ONE scratch array of F*S doubles (hipMallocAsync / hipFreeAsync on
 * `stream`); radii beyond 246 on such clips go sweep by sweep through global memory.  Every output sums its taps in ascending order from
 * zero with one fma each, whatever the form. */
int mf_jacobi_f64(const double* d_b, double* d_x, const double* d_taps, const double* d_lam,
                  const double* d_inv_on, int F, int S, int omega, int iters, void* stream);

/* ---- kernel 2a: per-cell homography table (mfs.py:881-906, 964-967, 1025-1027, 1039-1048) ----
 * d_unstab, d_stab: [n][(R+1)*(C+1)][2] float64 vertex displacements of the n frames to warp.
 * d_table: mf_cell_table_bytes(n, W, H, R, C) bytes, 16-byte aligned.  d_crop: [n][4] int32, initialised here to the
 * per-frame defaults {0, 0, W-1, H-1} = {left, top, right, bottom} (mfs.py:992-995).
 * d_status: one int32, incremented once per degenerate cell (zero it before the call). */
size_t mf_cell_table_bytes(int n, int W, int H, int R, int C);
/* Byte offset, inside the table blob, of the CLIP-LEVEL rectangle of the table's n frames: 4 int32 {max left, max top, min right,
 * min bottom} (mfs.py:1103-1106).  mf_cell_table_f64 sets it to the defaults {0, 0, W-1, H-1}; every mf_warp_u8c3 / mf_crop_scan_f64 on
 * the table folds its frames' values into it next to the per-frame rows of d_crop -- after the warp (or the scan) of all n frames it
 * equals what mf_crop_reduce computes from d_crop, without that launch. */
size_t mf_cell_table_bounds_offset(int n, int W, int H, int R, int C);
int mf_cell_table_f64(const double* d_unstab, const double* d_stab, int n, int W, int H, int R, int C,
                      void* d_table, int32_t* d_crop, int32_t* d_status, void* stream);

/* ---- kernel 2b: mesh warp + crop-boundary scan (mfs.py:1017-1019, 1050-1098) ----
 * d_frames, d_out: [n][H][W][3] uint8 (BGR).  For every output pixel: owner = last cell in row-major
 * order whose warped mask is non-zero (mfs.py:1060-1061); source coordinates from that cell's Hi
 * (mfs.py:1054); cv2.remap bilinear, constant border colour (mfs.py:1063-1069); the four edge scans
 * of mfs.py:1075-1098 are folded into d_crop[f] = {left, top, right, bottom} with atomic max/min.
 * d_frames and d_out may not alias. */
int mf_warp_u8c3(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                 int R, int C, const uint8_t border_bgr[3], int32_t* d_crop, void* stream);

/* ---- the crop-boundary scan WITHOUT the pixels (mfs.py:1075-1098) ----
 * The four per-frame edge scans look at the coordinate maps only, i.e. at nothing but the cell table: this fills
 * d_crop[f] = {left, top, right, bottom} for the n frames of d_table exactly as mf_warp_u8c3 does (same ownership and coordinate
 * arithmetic, atomic max/min into the defaults mf_cell_table_f64 wrote), visiting only the footprints that can set a flag (a few
 * per cent: the ring along the frame border) and touching no frame.  With it the clip-level rectangle (mf_crop_reduce, and the
 * 16-byte all-reduce of a sharded clip) is known BEFORE the first pixel moves, so _crop_frames (mfs.py:159) can follow the warp
 * chunk by chunk.  Running mf_warp_u8c3 on the same d_crop afterwards changes nothing (max/min of equal values). */
int mf_crop_scan_f64(const void* d_table, int n, int W, int H, int R, int C, int32_t* d_crop, void* stream);

/* ---- the same three calls with the clip-level rectangle in the CALLER's memory ----
 * mf_cell_table_f64 / mf_warp_u8c3 / mf_crop_scan_f64 with d_bounds[4] int32 {max left, max top, min right, min bottom}
 * (mfs.py:1103-1106) in place of the four words inside the table blob (mf_cell_table_bounds_offset): the cell table sets the defaults
 * {0, 0, W-1, H-1} there, the warp / the scan fold their frames' values into it.  A pipeline that reuses one table for clip after clip
 * gives every clip its own 16 bytes: a rectangle handed to a consumer is never rewritten by a later clip. */
int mf_cell_table_bounds_f64(const double* d_unstab, const double* d_stab, int n, int W, int H, int R, int C,
                             void* d_table, int32_t* d_crop, int32_t* d_status, int32_t* d_bounds, void* stream);
int mf_warp_bounds_u8c3(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                        int R, int C, const uint8_t border_bgr[3], int32_t* d_crop, int32_t* d_bounds, void* stream);
int mf_crop_scan_bounds_f64(const void* d_table, int n, int W, int H, int R, int C, int32_t* d_crop, int32_t* d_bounds, void* stream);

/* ---- kernels 2a + 2b + the rectangle for a clip RESIDENT in HBM, overlapped inside the clip (csrc/clippipe.hip) ----
 * _get_stabilized_frames_and_crop_boundaries (mfs.py:909-1108) as ONE call: mf_cell_table_f64 + mf_crop_scan_f64 + mf_crop_reduce on a
 * PREP stream, mf_warp_u8c3 on `stream`, the clip cut into `chunks` frame ranges (1..32; 4 is a good value) so that warp(k) waits for
 * table(k) only and everything else runs beside the warp.  d_unstab / d_stab / d_frames / d_out / d_table / d_crop / d_status as for the
 * three calls it replaces (d_status is incremented, not reset); d_bounds: [4] int32 = the clip-level rectangle {max left, max top,
 * min right, min bottom} of these n frames, FINAL on the prep stream right after the tables -- long before the last warp ends (a
 * sharded run issues its 16-byte all-reduce there).  prep_stream: the caller's (work already queued on it -- e.g. the Jacobi sweep that
 * produces d_stab -- precedes the tables; `stream` is NOT waited for, so the caller orders reuse of d_table / d_crop itself), or NULL =
 * an internal per-device stream that starts after everything queued on `stream` so far; prep_stream == stream: everything in order on
 * one stream.  On return `stream` has been made to wait for the prep work: stream order implies d_out, d_crop and d_bounds are final.
 * chunks <= 0: IN ORDER -- the whole table on `stream`, then the warp alone, then (prep_stream NULL or == stream) the rectangle from the
 * warp's own scan by one reduction; with a prep stream of the caller's the rectangle is taken EARLY from the table there (crop scan +
 * reduction beside the start of the warp), so that a sharded run's all-reduce hides behind the warp.  This is the faster arrangement on
 * an MI355X (kernels running beside the warp kernel cost it more than they take alone); the chunked one gives the rectangle earliest. */
int mf_warp_clip_u8c3(const uint8_t* d_frames, uint8_t* d_out, const double* d_unstab, const double* d_stab, int n, int W, int H,
                      int R, int C, const uint8_t border_bgr[3], void* d_table, int32_t* d_crop, int32_t* d_bounds, int32_t* d_status,
                      int chunks, void* prep_stream, void* stream);

/* ---- the same warp for uint16 frames (mfs.py:1063-1069: cv2.remap takes CV_16UC3 unchanged) ----
 * d_frames, d_out: [n][H][W][3] uint16 (BGR), 2-byte aligned is enough; all offsets are 64-bit.  Ownership, coordinates, the crop
 * flags and the clip rectangle are those of the uint8 calls on the same table (d_crop / d_bounds come out identical); the pixels follow
 * cv2.remap's 16U bilinear path (imgwarp.cpp remapBilinear<Cast<float, ushort>, RemapNoVec, float>): the same 1/32-pixel map
 * quantisation, float32 weights (1 - fy/32)(1 - fx/32) ..., t = ((S00 w0 + S01 w1) + S10 w2) + S11 w3 in float32 (each product and sum
 * rounded, no FMA), out = min(rint_half_even(t), 65535); outside taps are border_bgr[k] as given (the default (0, 0, 255) is NOT scaled
 * to 16 bits), a 2 x 2 footprint wholly outside gives border_bgr.  mf_warp_clip_u16c3 is mf_warp_clip_u8c3 with the same `chunks` /
 * `prep_stream` semantics.  Null pointers, d_frames == d_out, bad sizes and R or C > 64 return MF_ERR_INVALID_ARG before anything is
 * launched (the clip call: before its cell table). */
int mf_warp_u16c3(const uint16_t* d_frames, uint16_t* d_out, const void* d_table, int n, int W, int H,
                  int R, int C, const uint16_t border_bgr[3], int32_t* d_crop, void* stream);
int mf_warp_bounds_u16c3(const uint16_t* d_frames, uint16_t* d_out, const void* d_table, int n, int W, int H,
                         int R, int C, const uint16_t border_bgr[3], int32_t* d_crop, int32_t* d_bounds, void* stream);
int mf_warp_clip_u16c3(const uint16_t* d_frames, uint16_t* d_out, const double* d_unstab, const double* d_stab, int n, int W, int H,
                       int R, int C, const uint16_t border_bgr[3], void* d_table, int32_t* d_crop, int32_t* d_bounds, int32_t* d_status,
                       int chunks, void* prep_stream, void* stream);

/* ---- the same warp for single-channel uint8 frames (mfs.py:942, 1063-1069: the reference reads shape[:2] only and hands a grey frame
 * to cv2.remap with borderValue = color_outside_image_area_bgr, of which a 1-channel image uses the first component) ----
 * d_frames, d_out: [n][H][W] uint8, any alignment (a 4-byte aligned clip gets the staged taps).  cv2.remap's 8-bit path works per
 * channel, so the output is byte for byte channel 0 of mf_warp_u8c3 on the frames repeated three times with border (b, b, b); the
 * ownership, coordinates, crop flags and clip rectangle are the uint8 BGR call's on the same table (d_crop / d_bounds identical).
 * border: the border byte (saturate_cast<uchar>(borderValue[0])).  Limits: 2 <= W, H <= 32,767, R, C <= 64.  mf_warp_clip_u8c1 is
 * mf_warp_clip_u8c3 (mfs.py:909-1108) with the same `chunks` / `prep_stream` semantics; it refuses what its warp would refuse before
 * the cell table is launched.  Null pointers, d_frames == d_out and bad sizes return MF_ERR_INVALID_ARG before anything is launched. */
int mf_warp_u8c1(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                 int R, int C, uint8_t border, int32_t* d_crop, void* stream);
int mf_warp_bounds_u8c1(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                        int R, int C, uint8_t border, int32_t* d_crop, int32_t* d_bounds, void* stream);
int mf_warp_clip_u8c1(const uint8_t* d_frames, uint8_t* d_out, const double* d_unstab, const double* d_stab, int n, int W, int H,
                      int R, int C, uint8_t border, void* d_table, int32_t* d_crop, int32_t* d_bounds, int32_t* d_status,
                      int chunks, void* prep_stream, void* stream);

/* ---- the same warp for 4-channel uint8 frames (B G R A, or R G B A: the kernels do not care which colour comes first) ----
 * d_frames, d_out: [n][H][W][4] uint8, any alignment (a 4-byte aligned clip gets the staged taps); all offsets are 64-bit.  cv2.remap's 8-bit
 * path works per channel, so out[..., 0:3] is byte for byte mf_warp_u8c3 of frames[..., 0:3] with border (b, g, r), and out[..., 3] is
 * byte for byte mf_warp_u8c1 of frames[..., 3] with border a; the ownership, coordinates, crop flags, clip rectangle and degenerate-mesh
 * status are the uint8 BGR call's on the same table (d_crop / d_bounds identical).  border_bgra: {b, g, r, a} as given.  A caller that
 * holds a 3-component border (cv::Scalar(b, g, r) pads to (b, g, r, 0), as the reference's color_outside_image_area_bgr does) passes
 * a = 0: the area the warp uncovers then comes out with alpha 0, and with input alpha 255 the output alpha is 255 x coverage with the
 * bilinear soft edge.  Limits: 2 <= W, H <= 32,767, R, C <= 64.  mf_warp_clip_u8c4 is mf_warp_clip_u8c3 (mfs.py:909-1108) with the same
 * `chunks` / `prep_stream` semantics; it refuses what its warp would refuse before the cell table is launched.  Null pointers,
 * d_frames == d_out and bad sizes return MF_ERR_INVALID_ARG before anything is launched. */
int mf_warp_u8c4(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                 int R, int C, const uint8_t border_bgra[4], int32_t* d_crop, void* stream);
int mf_warp_bounds_u8c4(const uint8_t* d_frames, uint8_t* d_out, const void* d_table, int n, int W, int H,
                        int R, int C, const uint8_t border_bgra[4], int32_t* d_crop, int32_t* d_bounds, void* stream);
int mf_warp_clip_u8c4(const uint8_t* d_frames, uint8_t* d_out, const double* d_unstab, const double* d_stab, int n, int W, int H,
                      int R, int C, const uint8_t border_bgra[4], void* d_table, int32_t* d_crop, int32_t* d_bounds, int32_t* d_status,
                      int chunks, void* prep_stream, void* stream);

/* ---- the warp's float32 coordinate maps instead of pixels (mfs.py:983-984, 1054-1061: frame_stabilized_x_y, what cv2.remap is given at
 * mfs.py:1063-1069) ----
 * d_maps: [count][H][W][2] float32, x first, 8-byte aligned (16-byte aligned stacks get 16-byte stores); all offsets are 64-bit.  For the
 * frames first .. first + count - 1 of d_table (n, W, H, R, C describe the table, as for mf_crop_scan_f64) every output pixel gets the source
 * coordinates the pixel warps sample at, bit for bit: owner = last cell in row-major order whose warped mask is non-zero (cells with a
 * non-zero status own nothing), (u, v) = float32(((x m0 + y m1) + m2) (1/w)), float32(((x m3 + y m4) + m5) (1/w)) from that cell's
 * inverse homography in float64, (0, 0) where |w| <= FLT_EPSILON (cv2.perspectiveTransform); a pixel NO cell owns holds
 * (float32(W + 1), float32(H + 1)), the map template of mfs.py:983-984, which cv2.remap answers with the border colour.  No frame is read:
 * a caller samples any layer that must move with the video -- labels, depth, float32 planes -- with a sampler of its own.  The four edge scans
 * (mfs.py:1075-1098) of these frames are folded into d_crop (the table's [n][4] rows; rows outside the range are not touched) and the clip
 * rectangle exactly as mf_warp_u8c3 does: running it before or after a pixel warp on the same table changes nothing.  mf_warp_maps_bounds_f32:
 * the rectangle in the caller's d_bounds[4], as mf_warp_bounds_u8c3.  count == 0 is a no-op.  first < 0, count < 0, first + count > n, null
 * pointers, a misaligned d_maps, bad sizes, W or H outside 2 .. 32,767 and R or C > 64 return MF_ERR_INVALID_ARG before anything is launched. */
int mf_warp_maps_f32(const void* d_table, float* d_maps, int n, int W, int H, int R, int C, int first, int count, int32_t* d_crop,
                     void* stream);
int mf_warp_maps_bounds_f32(const void* d_table, float* d_maps, int n, int W, int H, int R, int C, int first, int count, int32_t* d_crop,
                            int32_t* d_bounds, void* stream);

/* ---- side planes: what travels with a video without being a picture -- depth, disparity, flow components, confidence (float32), labels and
 * masks (any element of 1, 2, 4 or 8 bytes) -- warped with the arrays the reference hands to cv2.remap at mfs.py:1063-1069 and cropped like
 * _crop_frames (mfs.py:1111-1157), so that a plane moves exactly as its colour frame does.  Planes are [n][H][W], contiguous.
 * mf_warp_plane_f32: cv2.remap(plane, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, borderValue = fill) on CV_32FC1 with the maps of
 * mf_warp_maps_f32: sx = cvRound(32 u), ix = sat_short(sx >> 5), fx = sx & 31 (the 8-bit path's quantisation), BilinearTab_f's exact float32
 * weights, t = ((S00 w0 + S01 w1) + S10 w2) + S11 w3 with every product and sum rounded on its own, out = t -- mf_warp_u16c3 on one channel
 * without saturate_cast.  A 2 x 2 footprint wholly outside the plane gives fill exactly, otherwise each outside tap is fill inside the sum;
 * a pixel no cell owns samples (W + 1, H + 1) and comes out as fill.  Every operation is an IEEE binary32 operation rounded on its own,
 * subnormals are kept, and no sample's value is looked at: all four products are always formed, so a tap of +-Inf or NaN with weight 0 gives
 * NaN (0 * Inf) and with a positive weight +-Inf or NaN; an outside tap is fill inside the sum (an infinite fill with weight 0: NaN); a footprint
 * wholly outside and an unowned pixel carry fill's own bits (-0.0 stays -0.0, a NaN fill gives a NaN).  A NaN's sign and payload are unspecified.
 * mf_warp_plane_nearest: cv2.remap(..., INTER_NEAREST, BORDER_CONSTANT) on elements of elem_bytes = 1, 2, 4 or 8 bytes: ix =
 * sat_short(cvRound(u)), iy = sat_short(cvRound(v)), float32 coordinates rounded half to even; the element is copied as bits where
 * 0 <= ix < W and 0 <= iy < H, otherwise the result is the low elem_bytes bytes of fill_bits.
 * Both fold the four edge scans (mfs.py:1075-1098) into d_crop and the clip rectangle exactly as mf_warp_u8c3 does -- a caller that warps
 * planes only gets the rectangle a frames caller gets; d_bounds (may be NULL): the rectangle in the caller's int32[4] as mf_warp_bounds_u8c3,
 * else in the table's own words.  All offsets are 64-bit.  Nothing outside the planes' bytes is read.  Refused with MF_ERR_INVALID_ARG before
 * anything is launched: null pointers, d_planes == d_out, n <= 0, W or H outside 2 .. 32,767, R or C outside 1 .. 64, an elem_bytes other
 * than 1, 2, 4, 8, a d_planes or d_out that is not aligned to its element. */
int mf_warp_plane_f32(const float* d_planes, float* d_out, const void* d_table, int n, int W, int H, int R, int C, float fill,
                      int32_t* d_crop, int32_t* d_bounds, void* stream);
int mf_warp_plane_nearest(const void* d_planes, void* d_out, const void* d_table, int n, int W, int H, int R, int C, int elem_bytes,
                          uint64_t fill_bits, int32_t* d_crop, int32_t* d_bounds, void* stream);
/* _crop_frames (mfs.py:1111-1157, cv2.resize at :1150-1155) for such planes: the inclusive rectangle scaled to out_W x out_H (the reference's
 * own call: out_W, out_H = W, H); d_out holds n * out_H * out_W elements.
 * mf_crop_resize_plane_f32: cv2.resize INTER_LINEAR on CV_32FC1 -- the index and fraction tables of mf_crop_resize_u8c3, float32 coefficients
 * (1 - f, f), t = S[sx] a0 + S[sx+1] a1, out = t0 b0 + t1 b1, float32, unfused: mf_crop_resize_to_u16c3 without saturate_cast; a crop exactly
 * twice the output in both axes takes INTER_AREA's fast path, (((S00 + S01) + S10) + S11) * 0.25f, in that order (the first sum may overflow).
 * On non-finite samples, signed zeros and subnormals (kept, never flushed) it is cv::resize's code path by path: the output columns whose sx was
 * clamped to the crop's last column are HResizeLinear's one-tap tail t = S[crop_w - 1] (an infinity there stays an infinity; the columns
 * clamped on the left stay two-tap, S[0] * 1 + S[1] * 0), the vertical pass always has two taps (a row of weight 0 that holds an infinity
 * gives NaN), and a crop of the output's own size is cv::resize's copy: the samples' bits, -0.0 and NaN payloads included, host and device
 * rectangle alike.  Integer-valued and finite non-negative data cannot tell these from the plain two-tap arithmetic.
 * mf_crop_resize_plane_nearest: cv2.resize INTER_NEAREST on elements of elem_bytes = 1, 2, 4 or 8 bytes: sx = min(floor(x * (1.0 / (out_W /
 * crop_w))), crop_w - 1) in float64, the same for y, the element copied as bits.
 * d_work: mf_crop_resize_workspace_bytes(out_W, out_H) bytes (the tables).  mf_crop_resize_dev_plane_*: the rectangle read by the kernels from
 * d_bounds when they execute, d_status as in mf_crop_resize_dev_u8c3 -- an unusable rectangle adds 1 to *d_status and nothing is read or written.
 * Refused with MF_ERR_INVALID_ARG before anything is launched: null pointers, d_planes == d_out, n <= 0, W, H, out_W or out_H outside
 * 1 .. 32,767, too many tiles, a bad elem_bytes, misaligned planes, and (host rectangle) an empty or out-of-plane rectangle. */
int mf_crop_resize_plane_f32(const float* d_planes, float* d_out, int n, int W, int H, int left, int top, int right, int bottom, int out_W,
                             int out_H, void* d_work, void* stream);
int mf_crop_resize_plane_nearest(const void* d_planes, void* d_out, int n, int W, int H, int left, int top, int right, int bottom, int out_W,
                                 int out_H, int elem_bytes, void* d_work, void* stream);
int mf_crop_resize_dev_plane_f32(const float* d_planes, float* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                                 void* d_work, int32_t* d_status, void* stream);
int mf_crop_resize_dev_plane_nearest(const void* d_planes, void* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                                     int elem_bytes, void* d_work, int32_t* d_status, void* stream);

/* ---- NV12 clips: the 4:2:0 surfaces hardware decoders and encoders exchange -- a full-resolution luma plane and one interleaved
 * half-resolution chroma plane -- warped from ONE cell table with the arrays the reference hands to cv2.remap at mfs.py:1063-1069, without a
 * conversion to BGR and back.  A clip is two contiguous stacks: d_y [n][H][W] uint8 and d_uv [n][H/2][W/2][2] uint8, U first; W and H are even,
 * 2 .. 32,767.  (Pitched surfaces and surfaces that keep a frame's two planes together are not taken: one plane stack per pointer.)
 * Luma: d_out_y is byte for byte mf_warp_u8c1 of d_y with border border_yuv[0] -- that very launch; the per-frame crop values in d_crop, the
 * clip rectangle and the ownership are that call's.
 * Chroma: chroma is DEFINED as sited at the even luma sample: output chroma sample (cx, cy) of frame f takes the float32 map (u, v) of luma
 * pixel (2 cx, 2 cy) -- exactly what mf_warp_maps_f32 returns for it, (W + 1, H + 1) for a pixel no cell owns included --, halves it in float32
 * (uc = u * 0.5f, vc = v * 0.5f: exact) and applies cv2.remap's 8-bit fixed-point INTER_LINEAR with BORDER_CONSTANT to the (H/2, W/2)
 * two-channel plane: sx = cvRound(32 uc), ix = sat_short(sx >> 5), fx = sx & 31 (the same in y), weights from the 2^15 table, out = (sum w s +
 * 2^14) >> 15 per channel.  A 2 x 2 tap footprint wholly outside the plane gives (border_yuv[1], border_yuv[2]), otherwise each outside tap is
 * that border sample inside the sum; an unowned pixel halves to ((W + 1) / 2, (H + 1) / 2), which lies outside the plane.  U and V never mix.
 * (No quarter-pixel correction for left- or centre-sited chroma is applied.)  The chroma launch follows the luma launch on the same stream; it
 * reads nothing outside the plane's bytes and touches neither d_crop nor the rectangle.  All plane offsets are 64-bit.
 * border_yuv: {Y, U, V} as given; BT.601 limited-range red, the reference's default BGR (0, 0, 255), is (81, 90, 240).
 * mf_warp_bounds_nv12: the rectangle in the caller's d_bounds[4], as mf_warp_bounds_u8c1.
 * Refused with MF_ERR_INVALID_ARG before anything is launched: null pointers, n <= 0, any two of the four planes overlapping, an odd W or H, W
 * or H outside 2 .. 32,767, R or C outside 1 .. 64, a d_uv or d_out_uv that is not 2-byte aligned. */
int mf_warp_nv12(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, const void* d_table, int n, int W, int H,
                 int R, int C, const uint8_t border_yuv[3], int32_t* d_crop, void* stream);
int mf_warp_bounds_nv12(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, const void* d_table, int n, int W, int H,
                        int R, int C, const uint8_t border_yuv[3], int32_t* d_crop, int32_t* d_bounds, void* stream);

/* ---- P010 clips: the 4:2:0 layout with 16-bit samples that hardware decoders write for 10-bit and HDR video, warped from ONE cell table like an
 * NV12 clip, without a conversion to 3-channel uint16 and back.  A clip is two contiguous stacks: d_y [n][H][W] uint16 and d_uv
 * [n][H/2][W/2][2] uint16, U first; W and H are even, 2 .. 32,767.  Samples are plain 16-bit numbers, 0 .. 65,535: P010, P012 and P016 differ
 * only in how many low bits a producer leaves zero, so this one entry serves all three.  The OUTPUT's low bits carry the blend's fraction --
 * nothing is masked; a consumer that needs them zero masks them itself.  (Pitched surfaces and surfaces that keep a frame's two planes
 * together are not taken: one plane stack per pointer.)
 * Luma: d_out_y is, bit for bit, channel 0 of mf_warp_u16c3 applied to the clip stack(Y, Y, Y) with border (b, b, b), b = border_yuv[0]:
 * cv2.remap INTER_LINEAR / BORDER_CONSTANT of CV_16UC1 -- the 8-bit map quantisation (sx = cvRound(32 u), ix = sx >> 5, fx = sx & 31), the
 * float32 BilinearTab_f weights, the chain ((S00 w0 + S01 w1) + S10 w2) + S11 w3 with every product and sum rounded on its own, then
 * saturate_cast<ushort>; a 2 x 2 footprint wholly outside the frame gives the border sample itself.  The per-frame crop values in d_crop, the
 * clip rectangle and the degenerate-cell status are written by this launch and are exactly what mf_warp_u16c3 (and mf_warp_u8c1) writes on
 * the same table.
 * Chroma: sited at the even luma sample, as for NV12: output chroma sample (cx, cy) of frame f takes the float32 map (u, v) of luma pixel
 * (2 cx, 2 cy) -- exactly what mf_warp_maps_f32 returns for it, (W + 1, H + 1) for a pixel no cell owns included --, halves it in float32 (exact)
 * and applies the CV_16U arithmetic above per channel on the (H/2, W/2) two-channel plane with border (border_yuv[1], border_yuv[2]).  U and V
 * never mix.  The chroma launch follows the luma launch on the same stream; it reads nothing outside the plane's bytes and touches neither
 * d_crop nor the rectangle.  All plane offsets are 64-bit.
 * border_yuv: {Y, U, V} as given; BT.601 limited-range red at 10 bits in P010's high bits is (81 << 8, 90 << 8, 240 << 8) = (20736, 23040, 61440).
 * mf_warp_bounds_p010: the rectangle in the caller's d_bounds[4], as mf_warp_bounds_u16c3.
 * Refused with MF_ERR_INVALID_ARG before anything is launched: null pointers, n <= 0, any two of the four planes overlapping, an odd W or H, W
 * or H outside 2 .. 32,767, R or C outside 1 .. 64, a plane pointer that is not 2-byte aligned. */
int mf_warp_p010(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, const void* d_table, int n, int W, int H,
                 int R, int C, const uint16_t border_yuv[3], int32_t* d_crop, void* stream);
int mf_warp_bounds_p010(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, const void* d_table, int n, int W, int H,
                        int R, int C, const uint16_t border_yuv[3], int32_t* d_crop, int32_t* d_bounds, void* stream);

/* ---- NV16 clips: the 4:2:2 layout of capture cards, SDI / HDMI grabbers and webcams in its semi-planar form -- a full-resolution luma plane
 * and one interleaved chroma plane of half the WIDTH and the full height -- warped from ONE cell table like an NV12 clip, with the arrays the
 * reference hands to cv2.remap at mfs.py:1063-1069, without a conversion to BGR and without dropping chroma rows.  A clip is two contiguous stacks: d_y [n][H][W] uint8 and d_uv [n][H][W/2][2] uint8, U first; W is
 * even, H of either parity, both 2 .. 32,767.  The packed forms (YUY2, UYVY) come in and go out through mf_unpack_422_u8 / mf_pack_422_u8 below.
 * Luma: d_out_y is byte for byte mf_warp_u8c1 of d_y with border border_yuv[0] -- that very launch; the per-frame crop values in d_crop, the
 * clip rectangle and the ownership are that call's.
 * Chroma: chroma is DEFINED as sited at the even luma sample of the same row: output chroma sample (cx, y) of frame f takes the float32 map
 * (u, v) of luma pixel (2 cx, y) -- exactly what mf_warp_maps_f32 returns for it, (W + 1, H + 1) for a pixel no cell owns included --, halves u
 * in float32 (uc = u * 0.5f: exact; vc = v as it is) and applies cv2.remap's 8-bit fixed-point INTER_LINEAR with BORDER_CONSTANT to the
 * (H, W/2) two-channel plane: sx = cvRound(32 uc), ix = sat_short(sx >> 5), fx = sx & 31 (the same in y), weights from the 2^15 table, out =
 * (sum w s + 2^14) >> 15 per channel.  A 2 x 2 tap footprint wholly outside the plane gives (border_yuv[1], border_yuv[2]), otherwise each
 * outside tap is that border sample inside the sum; an unowned pixel lands at ((W + 1) / 2, H + 1), which lies outside the plane.  U and V
 * never mix.  (No sub-pixel correction for other chroma sitings is applied.)  The chroma launch follows the luma launch on the same stream; it
 * reads nothing outside the plane's bytes and touches neither d_crop nor the rectangle.  All plane offsets are 64-bit.
 * border_yuv: {Y, U, V} as given; BT.601 limited-range red, the reference's default BGR (0, 0, 255), is (81, 90, 240).
 * mf_warp_bounds_nv16: the rectangle in the caller's d_bounds[4], as mf_warp_bounds_u8c1.
 * Refused with MF_ERR_INVALID_ARG before anything is launched: null pointers, n <= 0, any two of the four planes overlapping (the chroma stacks
 * are n W H bytes), an odd W, W or H outside 2 .. 32,767, R or C outside 1 .. 64, a d_uv or d_out_uv that is not 2-byte aligned.
 * 10-bit 4:2:2 is the P210 section below (mf_warp_p210, mf_crop_resize_p210, mf_unpack_y210_u16).  Not provided for 4:2:2: the clip pipelines
 * (mf_clip_*), v210. */
int mf_warp_nv16(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, const void* d_table, int n, int W, int H,
                 int R, int C, const uint8_t border_yuv[3], int32_t* d_crop, void* stream);
int mf_warp_bounds_nv16(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, const void* d_table, int n, int W, int H,
                        int R, int C, const uint8_t border_yuv[3], int32_t* d_crop, int32_t* d_bounds, void* stream);

/* Packed 4:2:2 against the NV16 pair.  d_packed [n][H][W][2] uint8 with W even is a flat stream of 4-byte words; word k covers luma pixels 2k
 * and 2k + 1 of the flat [n][H][W] stream (W is even, so no row or frame boundary falls inside a word).  order 0, yuyv (YUY2): bytes Y0 U Y1 V;
 * order 1, uyvy (2vuy): bytes U Y0 V Y1.  mf_unpack_422_u8 writes y[2k] = Y0, y[2k + 1] = Y1, uv[2k] = U, uv[2k + 1] = V -- exactly the NV16
 * pair d_y [n][H][W], d_uv [n][H][W/2][2]; mf_pack_422_u8 is the inverse.  The warp of a packed clip is unpack, mf_warp_nv16, pack.
 * One streaming kernel each: dwordx4 loads and 16-byte stores where the addresses allow them, narrower accesses where they do not -- no access
 * is wider than its address's alignment; 64-bit indices, any clip length.
 * Refused with MF_ERR_INVALID_ARG before anything is launched: a null pointer, n < 1, W odd or outside 2 .. 32,767, H outside 1 .. 32,767, an
 * order other than 0 or 1, a d_packed that is not 4-byte aligned, a d_y or d_uv that is not 2-byte aligned (whole frames of contiguous stacks
 * always are), any overlap of the three buffers. */
int mf_unpack_422_u8(const uint8_t* d_packed, uint8_t* d_y, uint8_t* d_uv, int n, int W, int H, int order, void* stream);
int mf_pack_422_u8(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_packed, int n, int W, int H, int order, void* stream);
/* _crop_frames (mfs.py:1111-1157) for an NV16 clip -- d_y [n][H][W], d_uv [n][H][W/2][2], U first, as mf_warp_nv16 takes them -- to d_out_y
 * [n][out_H][out_W] and d_out_uv [n][out_H][out_W/2][2], without a conversion to BGR and without dropping chroma rows.  W and out_W are even,
 * H and out_H of either parity, all four 2 .. 32,767; the rectangle is inclusive, in luma pixels, of any parity, usable under the rule of
 * mf_crop_resize_u8c3.  DEFINED here, modelled on cv2.resize (OpenCV 4.5 - 4.10), not pinned (like mf_crop_resize_nv12's chroma).  A packed
 * clip goes through mf_unpack_422_u8, this call, mf_pack_422_u8.
 * Luma: d_out_y is byte for byte mf_crop_resize_to_u8c1 of d_y (mf_crop_resize_dev_u8c1 for the device rectangle) -- that very launch.
 * Chroma, x axis: exactly mf_crop_resize_nv12's.  Output chroma sample cx sits on output luma pixel 2 cx, and its source is that pixel's luma
 * source position, made absolute in the frame and halved.  With cw = right - left + 1, scale_x = 1.0 / ((double)out_W / (double)cw) (the luma
 * tables' value), c1 = right >> 1 and c0 = min((left + 1) >> 1, c1) -- the chroma samples whose siting luma pixel lies inside the crop --:
 *   fc = (float)(((double)left + (((double)(2 cx) + 0.5) * scale_x - 0.5)) * 0.5);  s = floor(fc);  f = fc - (float)s
 *   s < c0 -> (s, f) = (c0, 0);  s >= c1 -> (c1, 0);  a0 = cvRound((1 - f) * 2048), a1 = cvRound(f * 2048)
 * Chroma, y axis: chroma has luma's rows, so output chroma row y takes the LUMA table's own entry for row y: with ch = bottom - top + 1 and
 * scale_y = 1.0 / ((double)out_H / (double)ch), fy = (float)(((double)y + 0.5) * scale_y - 0.5), sy = floor(fy), the rows are top + clip(sy, 0,
 * ch - 1) and top + clip(sy + 1, 0, ch - 1), the weights b0 = cvRound((1 - (fy - sy)) * 2048), b1 = cvRound((fy - sy) * 2048), kept where a row was
 * clipped.  No second y table, nothing halved.
 * Then mf_crop_resize_u8c3's two passes per channel: t = S[s] a0 + S[s+1] a1, out = (((b0 (t0 >> 4)) >> 16) + ((b1 (t1 >> 4)) >> 16) + 2) >> 2.
 * U and V never mix; no INTER_AREA special case (for 8-bit data it is this arithmetic).  Nothing outside chroma columns c0 .. c1 and rows
 * top .. bottom of the frame's own chroma plane influences the result, and no byte outside the d_uv stack is read: where s == c1 only the 2-byte
 * sample is read.  Consequences: the full-frame rectangle at out_W x out_H == W x H is a copy of d_uv; a rectangle with an even left at its own
 * size is a copy of the sub-plane, for any top; where left is even and out_W == cw, the y axis is luma's byte for byte.
 * d_work: mf_crop_resize_nv16_workspace_bytes(out_W, out_H) bytes (the luma tables, then out_W / 2 chroma x entries).  The luma launch goes
 * first, then chroma, on the same stream.  mf_crop_resize_dev_nv16: the rectangle read from d_bounds when the kernels execute; one that cannot be
 * used adds exactly 1 to *d_status (the luma tables kernel does, once) and leaves both outputs and the workspace untouched: the chroma kernels
 * return before they read anything, the luma y table included (d_status as in mf_crop_resize_dev_u8c3).
 * Refused with MF_ERR_INVALID_ARG before anything is launched: null pointers, n <= 0, any two of the four plane stacks overlapping, an odd W or
 * out_W, a W, H, out_W or out_H outside 2 .. 32,767, a d_uv or d_out_uv that is not 2-byte aligned, too many tiles, and (host rectangle) an
 * empty or out-of-frame rectangle.  An odd H or out_H is not refused. */
size_t mf_crop_resize_nv16_workspace_bytes(int out_W, int out_H);
int mf_crop_resize_nv16(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, int n, int W, int H, int left, int top,
                        int right, int bottom, int out_W, int out_H, void* d_work, void* stream);
int mf_crop_resize_dev_nv16(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, int n, int W, int H,
                            const int32_t* d_bounds, int out_W, int out_H, void* d_work, int32_t* d_status, void* stream);

/* ---- P210 clips: 10-bit 4:2:2 -- what SDI / HDMI capture, ProRes and XAVC decoders and contribution feeds deliver -- in its semi-planar form:
 * NV16's geometry with P010's samples.  A clip is two contiguous stacks: d_y [n][H][W] uint16 and d_uv [n][H][W/2][2] uint16, U first; W is
 * even, H of either parity, both 2 .. 32,767.  Samples are plain 16-bit numbers, 0 .. 65535, nothing is masked: P210, P212 and P216 are the
 * same bytes to these calls.  The packed form (Y210 / Y216) comes in and goes out through mf_unpack_y210_u16 / mf_pack_y210_u16 below.  Warped
 * from ONE cell table with the arrays the reference hands to cv2.remap at mfs.py:1063-1069.
 * Luma: d_out_y is bit for bit mf_warp_p010's luma (cv2.remap of CV_16UC1: channel 0 of mf_warp_u16c3 on stack(Y, Y, Y)) -- that very launch;
 * the per-frame crop values in d_crop, the clip rectangle and the ownership are that call's.
 * Chroma: sited at the even luma sample of the same row, as in mf_warp_nv16: output chroma sample (cx, y) of frame f takes the float32 map
 * (u, v) of luma pixel (2 cx, y) -- what mf_warp_maps_f32 returns for it, (W + 1, H + 1) for a pixel no cell owns included --, halves u in
 * float32 (uc = u * 0.5f: exact; vc = v as it is) and samples the (H, W/2) two-channel plane with mf_warp_p010's chroma arithmetic: cv2.remap's
 * fixed-point coordinates (sx = cvRound(32 uc), ix = sat_short(sx >> 5), fx = sx & 31, the same in y) and CV_16U float weights per channel.  A
 * 2 x 2 tap footprint wholly outside the plane -- an unowned pixel's, at ((W + 1) / 2, H + 1), among them -- gives (border_yuv[1],
 * border_yuv[2]) itself; otherwise each outside tap is that border sample inside the sum.  U and V never mix.  The chroma launch follows the
 * luma launch on the same stream; it reads nothing outside the plane's bytes and touches neither d_crop nor the rectangle.  All plane offsets
 * are 64-bit.
 * border_yuv: {Y, U, V} as given.  mf_warp_bounds_p210: the rectangle in the caller's d_bounds[4], as mf_warp_bounds_u8c1.
 * Refused with MF_ERR_INVALID_ARG before anything is launched: null pointers, n <= 0, any two of the four planes overlapping (each stack is
 * 2 n W H bytes), an odd W, W or H outside 2 .. 32,767, R or C outside 1 .. 64, a plane pointer that is not 2-byte aligned.  An odd H is not
 * refused.
 * Not provided: v210 (three 10-bit samples per 32-bit word), kernels that warp or crop the packed words directly, the host and clip pipelines
 * (mf_*_host_frames, mf_clip_*). */
int mf_warp_p210(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, const void* d_table, int n, int W, int H,
                 int R, int C, const uint16_t border_yuv[3], int32_t* d_crop, void* stream);
int mf_warp_bounds_p210(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, const void* d_table, int n, int W, int H,
                        int R, int C, const uint16_t border_yuv[3], int32_t* d_crop, int32_t* d_bounds, void* stream);

/* Packed Y210 / Y216 against the P210 pair.  d_packed [n][H][W][2] uint16 with W even is a flat stream of 8-byte words Y0 U Y1 V; word k covers
 * luma pixels 2k and 2k + 1 of the flat [n][H][W] stream.  mf_unpack_y210_u16 writes y[2k] = Y0, y[2k + 1] = Y1, uv[2k] = U, uv[2k + 1] = V --
 * exactly the P210 pair; mf_pack_y210_u16 is the inverse.  Samples move as bits (nothing masked or shifted); there is one sample order.  The
 * warp of a packed clip is unpack, mf_warp_p210, pack.  One streaming kernel each: dwordx4 loads and 16-byte stores where the addresses allow
 * them, narrower accesses where they do not -- no access is wider than its address's alignment; 64-bit indices, any clip length.
 * Alignment contract: d_packed 8-byte aligned (a word is never split), d_y and d_uv 2-byte aligned.
 * Refused with MF_ERR_INVALID_ARG before anything is launched: a null pointer, n < 1, W odd or outside 2 .. 32,767, H outside 1 .. 32,767, a
 * d_packed that is not 8-byte aligned, a d_y or d_uv that is not 2-byte aligned, any overlap of the three buffers. */
int mf_unpack_y210_u16(const uint16_t* d_packed, uint16_t* d_y, uint16_t* d_uv, int n, int W, int H, void* stream);
int mf_pack_y210_u16(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_packed, int n, int W, int H, void* stream);
/* _crop_frames (mfs.py:1111-1157) for a P210 clip -- d_y [n][H][W], d_uv [n][H][W/2][2] uint16, U first, as mf_warp_p210 takes them -- to
 * d_out_y [n][out_H][out_W] and d_out_uv [n][out_H][out_W/2][2].  W and out_W are even, H and out_H of either parity, all four 2 .. 32,767; the
 * rectangle is inclusive, in luma pixels, of any parity.  DEFINED here, modelled on cv2.resize (OpenCV 4.5 - 4.10), not pinned.
 * Luma: d_out_y is bit for bit mf_crop_resize_p010's luma -- that very launch: the float path of CV_16UC1, and INTER_AREA's
 * (S00 + S01 + S10 + S11 + 2) >> 2 where 2 out_W == cw and 2 out_H == ch.
 * Chroma, x axis: exactly mf_crop_resize_p010's (column s clamped into c0 .. c1, float32 fraction f, weights (1 - f, f) as they are).
 * Chroma, y axis: chroma has luma's rows, so output chroma row y takes the LUMA table's own entry for row y: with ch = bottom - top + 1 and
 * scale_y = 1.0 / ((double)out_H / (double)ch), fy = (float)(((double)y + 0.5) * scale_y - 0.5), sy = floor(fy), the rows are top + clip(sy, 0,
 * ch - 1) and top + clip(sy + 1, 0, ch - 1) and the weights (1 - (fy - sy), fy - sy) in float32, kept where a row was clipped.  No second y
 * table, nothing halved.  Then per channel t = float(S[s]) a0 + float(S[s+1]) a1, out = min(rint(t0 b0 + t1 b1), 65535), every product and sum
 * rounded on its own.  U and V never mix.  Chroma has NO area branch: at exactly 2x down, where luma takes the box, chroma takes this float
 * path on the luma table's entries.  Nothing outside chroma columns c0 .. c1 and rows top .. bottom influences the result, and no byte outside
 * the d_uv stack is read (where s == c1 only that one 4-byte sample is loaded).  The full-frame rectangle at out_W x out_H == W x H is a copy
 * of both planes.
 * d_work: mf_crop_resize_p210_workspace_bytes(out_W, out_H) bytes (the luma tables, then out_W / 2 chroma x entries of 8 bytes).  The luma
 * launch goes first, then chroma, on the same stream.  mf_crop_resize_dev_p210: the rectangle read from d_bounds when the kernels execute; one
 * that cannot be used adds exactly 1 to *d_status (the luma tables kernel does, once) and leaves both outputs and the workspace untouched: the
 * chroma kernels return before they read anything, the luma y table included.
 * Refused with MF_ERR_INVALID_ARG before anything is launched: null pointers, n <= 0, any two of the four plane stacks overlapping, an odd W or
 * out_W, a W, H, out_W or out_H outside 2 .. 32,767, a plane pointer that is not 2-byte aligned, too many tiles, and (host rectangle) an empty
 * or out-of-frame rectangle.  An odd H or out_H is not refused. */
size_t mf_crop_resize_p210_workspace_bytes(int out_W, int out_H);
int mf_crop_resize_p210(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, int n, int W, int H, int left, int top,
                        int right, int bottom, int out_W, int out_H, void* d_work, void* stream);
int mf_crop_resize_dev_p210(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, int n, int W, int H,
                            const int32_t* d_bounds, int out_W, int out_H, void* d_work, int32_t* d_status, void* stream);

/* Clip-level crop bounds (mfs.py:1103-1106): {max left, max top, min right, min bottom} over n frames.
 * d_bounds: [4] int32. */
int mf_crop_reduce(const int32_t* d_crop, int n, int W, int H, int32_t* d_bounds, void* stream);

/* ---- next row on the path: crop + bilinear resize (mfs.py:1111-1157, called at mfs.py:159) ----
 * Crops each of the n frames to the inclusive rectangle {left, top, right, bottom} (the clip-level crop
 * bounds) and scales it back to W x H exactly like cv2.resize(crop, (W, H)) with the default INTER_LINEAR on
 * 8-bit data (two-pass 11-bit fixed point).  d_work: mf_crop_resize_workspace_bytes(W, H) bytes of scratch.
 * An empty or out-of-frame rectangle is MF_ERR_INVALID_ARG (cv2.resize fails on an empty source). */
size_t mf_crop_resize_workspace_bytes(int W, int H);
int mf_crop_resize_u8c3(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right,
                        int bottom, void* d_work, void* stream);
/* The same for uint16 frames (mfs.py:1150-1155: cv2.resize takes CV_16UC3 unchanged): resize.cpp's float path (resizeGeneric_ with
 * HResizeLinear<ushort, float, float> + VResizeLinear<ushort, float, float, Cast<float, ushort>>) -- the 8-bit index and fraction
 * tables, float32 coefficients (1 - f, f), t = S[sx] a0 + S[sx+1] a1 and out = saturate_cast<ushort>(t0 b0 + t1 b1), float32, unfused,
 * rounded half to even.  The same workspace size; the same refusals. */
int mf_crop_resize_u16c3(const uint16_t* d_frames, uint16_t* d_out, int n, int W, int H, int left, int top, int right,
                         int bottom, void* d_work, void* stream);
/* The same for single-channel uint8 frames [n][H][W] (mfs.py:1129, 1150-1155: cv2.resize of a 2-D frame): output = channel 0 of
 * mf_crop_resize_u8c3 on the frames repeated three times (the same tables, the same workspace size).  1 <= W, H <= 32,767; the same
 * refusals. */
int mf_crop_resize_u8c1(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right,
                        int bottom, void* d_work, void* stream);
/* The same for 4-channel uint8 frames [n][H][W][4]: channels 0-2 of the output are mf_crop_resize_u8c3 of frames[..., 0:3], channel 3 is
 * mf_crop_resize_u8c1 of frames[..., 3] (cv2.resize's 8-bit path works per channel; the same tables, the same workspace size).
 * 1 <= W, H <= 32,767; the same refusals. */
int mf_crop_resize_u8c4(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right,
                        int bottom, void* d_work, void* stream);
/* _crop_frames to a caller-chosen output size: the same crop, scaled to out_W x out_H exactly like cv2.resize(crop, (out_W, out_H)) with
 * INTER_LINEAR, for the four formats above (u16c3: where the crop is exactly twice the output in both axes, cv::resize takes INTER_AREA's
 * fast path, (S00 + S01 + S10 + S11 + 2) >> 2, rounded half up; for 8-bit data that equals the bilinear result).  d_out holds
 * n * out_H * out_W * channels samples.  d_work: mf_crop_resize_workspace_bytes(out_W, out_H) bytes suffice (the tables have one entry per
 * OUTPUT column and row; no separate workspace call).  out_W, out_H == W, H is the call above, byte for byte.  Refused with
 * MF_ERR_INVALID_ARG before anything is launched or written: null pointers, d_frames == d_out, out_W or out_H outside 1 .. 32,767, too
 * many tiles, an empty or out-of-frame rectangle, and every refusal of the call above. */
int mf_crop_resize_to_u8c3(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right, int bottom,
                           int out_W, int out_H, void* d_work, void* stream);
int mf_crop_resize_to_u16c3(const uint16_t* d_frames, uint16_t* d_out, int n, int W, int H, int left, int top, int right, int bottom,
                            int out_W, int out_H, void* d_work, void* stream);
int mf_crop_resize_to_u8c1(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right, int bottom,
                           int out_W, int out_H, void* d_work, void* stream);
int mf_crop_resize_to_u8c4(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, int left, int top, int right, int bottom,
                           int out_W, int out_H, void* d_work, void* stream);
/* _crop_frames (mfs.py:1111-1157) from a rectangle that stays on the device: the call above with {left, top, right, bottom} read by the
 * kernels from d_bounds ([4] int32 in device memory, e.g. what mf_warp_bounds_* / mf_warp_clip_* / mf_crop_reduce leave there) when they
 * EXECUTE, in stream order.  The host never reads the rectangle and the call never synchronises (for u8c3, once the device has been probed:
 * mf_set_device does that).  The same size: out_W = W, out_H = H.  For a usable rectangle d_out and the tables in d_work
 * (mf_crop_resize_workspace_bytes(out_W, out_H) bytes) are byte for byte those of mf_crop_resize_to_* with the same four numbers.
 * d_status: [1] int32 of the caller's, zeroed by the caller.  A rectangle that cannot be used -- right < left, bottom < top, a negative
 * edge, right >= W or bottom >= H, the device twin of the MF_ERR_INVALID_ARG refusal above -- adds 1 to *d_status, once per call; every
 * kernel of the call then returns before it reads a frame byte or writes a byte of d_out or d_work.  Nothing faults, whatever the 16
 * bytes hold; the return value cannot tell (it is MF_OK), *d_status is read whenever the caller next synchronises.
 * Refused on the host with MF_ERR_INVALID_ARG, nothing launched or written: null pointers (d_bounds and d_status included), d_frames ==
 * d_out, n < 1, W, H, out_W or out_H outside 1 .. 32,767, too many tiles. */
int mf_crop_resize_dev_u8c3(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                            void* d_work, int32_t* d_status, void* stream);
int mf_crop_resize_dev_u16c3(const uint16_t* d_frames, uint16_t* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                             void* d_work, int32_t* d_status, void* stream);
int mf_crop_resize_dev_u8c1(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                            void* d_work, int32_t* d_status, void* stream);
int mf_crop_resize_dev_u8c4(const uint8_t* d_frames, uint8_t* d_out, int n, int W, int H, const int32_t* d_bounds, int out_W, int out_H,
                            void* d_work, int32_t* d_status, void* stream);
/* _crop_frames (mfs.py:1111-1157) for an NV12 clip -- d_y [n][H][W], d_uv [n][H/2][W/2][2], U first, as mf_warp_nv12 takes them -- to d_out_y
 * [n][out_H][out_W] and d_out_uv [n][out_H/2][out_W/2][2], without a conversion to BGR and back.  W, H, out_W and out_H are even, 2 .. 32,767;
 * the rectangle is inclusive, in luma pixels, of any parity.  DEFINED here, modelled on cv2.resize, not pinned (like mf_warp_nv12's chroma).
 * Luma: d_out_y is byte for byte mf_crop_resize_to_u8c1 of d_y (mf_crop_resize_dev_u8c1 for the device rectangle) -- that very launch.
 * Chroma is sited at the even luma sample: output chroma sample cx sits on output luma pixel 2 cx, and its source is that pixel's luma source
 * position, made absolute in the frame and halved.  With cw = right - left + 1, scale_x = 1.0 / ((double)out_W / (double)cw) (the luma tables'
 * value), c1 = right >> 1 and c0 = min((left + 1) >> 1, c1) -- the chroma samples whose siting luma pixel lies inside the crop --:
 *   fc = (float)(((double)left + (((double)(2 cx) + 0.5) * scale_x - 0.5)) * 0.5);  s = floor(fc);  f = fc - (float)s
 *   s < c0 -> (s, f) = (c0, 0);  s >= c1 -> (c1, 0);  a0 = cvRound((1 - f) * 2048), a1 = cvRound(f * 2048)
 * the y axis the same with top, bottom, out_H and cy, except that (as in cv2) the two row indices are clipped to [r0, r1] and the weights kept.
 * Then mf_crop_resize_u8c3's two passes per channel: t = S[s] a0 + S[s+1] a1, out = (((b0 (t0 >> 4)) >> 16) + ((b1 (t1 >> 4)) >> 16) + 2) >> 2.
 * U and V never mix; no INTER_AREA special case.  Nothing outside columns c0 .. c1 and rows r0 .. r1 of the frame's own chroma plane influences
 * the result, and no byte outside the d_uv stack is read.  The full-frame rectangle at out_W x out_H == W x H is a copy of d_uv.
 * d_work: mf_crop_resize_nv12_workspace_bytes(out_W, out_H) bytes (the luma tables, then the chroma tables).  The luma launch goes first, then
 * chroma, on the same stream.  mf_crop_resize_dev_nv12: the rectangle read from d_bounds when the kernels execute; one that cannot be used adds
 * exactly 1 to *d_status and leaves both outputs and the workspace untouched (d_status as in mf_crop_resize_dev_u8c3).
 * Refused with MF_ERR_INVALID_ARG before anything is launched: null pointers, n <= 0, any two of the four plane stacks overlapping, an odd W, H,
 * out_W or out_H or one outside 2 .. 32,767, a d_uv or d_out_uv that is not 2-byte aligned, too many tiles, and (host rectangle) an empty or
 * out-of-frame rectangle. */
size_t mf_crop_resize_nv12_workspace_bytes(int out_W, int out_H);
int mf_crop_resize_nv12(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, int n, int W, int H, int left, int top,
                        int right, int bottom, int out_W, int out_H, void* d_work, void* stream);
int mf_crop_resize_dev_nv12(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_out_y, uint8_t* d_out_uv, int n, int W, int H,
                            const int32_t* d_bounds, int out_W, int out_H, void* d_work, int32_t* d_status, void* stream);
/* _crop_frames (mfs.py:1111-1157) for a P010 clip -- d_y [n][H][W] uint16, d_uv [n][H/2][W/2][2] uint16, U first, as mf_warp_p010 takes them -- to
 * d_out_y [n][out_H][out_W] and d_out_uv [n][out_H/2][out_W/2][2], without a conversion to 3-channel uint16 and back.  W, H, out_W and out_H are
 * even, 2 .. 32,767; the rectangle is inclusive, in luma pixels, of any parity.  Samples are plain 16-bit numbers; nothing is masked.  DEFINED
 * here, modelled on cv2.resize (OpenCV 4.5-4.10), not pinned.
 * Luma: d_out_y is, bit for bit, channel 0 of mf_crop_resize_to_u16c3 (mf_crop_resize_dev_u16c3 for the device rectangle) applied to the clip
 * stack(Y, Y, Y): cv2.resize INTER_LINEAR of CV_16UC1 -- that call's tables for (out_W, out_H), float32 weights (1 - f, f),
 * t = float(S[sx]) a0 + float(S[sx+1]) a1, out = min(rint(t0 b0 + t1 b1), 65535), every product and sum rounded on its own; where
 * 2 out_W == cw and 2 out_H == ch, INTER_AREA's (S00 + S01 + S10 + S11 + 2) >> 2 instead.
 * Chroma is sited at the even luma sample, exactly as for mf_crop_resize_nv12: with cw = right - left + 1,
 * scale_x = 1.0 / ((double)out_W / (double)cw), c1 = right >> 1 and c0 = min((left + 1) >> 1, c1):
 *   fc = (float)(((double)left + (((double)(2 cx) + 0.5) * scale_x - 0.5)) * 0.5);  s = floor(fc);  f = fc - (float)s
 *   s < c0 -> (s, f) = (c0, 0);  s >= c1 -> (c1, 0)
 * the y axis the same with top, bottom, out_H and cy, except that the two row indices are clipped to [r0, r1] and the fraction kept.  Then the
 * 16-bit float arithmetic above per channel with the float32 weights (1 - f, f) -- no 2048 quantisation.  U and V never mix.  Chroma has NO
 * area branch: at exactly 2x down an even `left` gives f = 0.25, not a box, so chroma takes the float path everywhere.  Nothing outside columns
 * c0 .. c1 and rows r0 .. r1 of the frame's own chroma plane influences the result, and no byte outside the d_uv stack is read (where s == c1
 * only that one sample is loaded).  The full-frame rectangle at out_W x out_H == W x H is a copy of both planes.
 * d_work: mf_crop_resize_p010_workspace_bytes(out_W, out_H) bytes (the luma tables, mf_crop_resize_workspace_bytes(out_W, out_H), then
 * out_W/2 + out_H/2 chroma entries of 8 bytes).  The luma launch goes first, then chroma, on the same stream.  mf_crop_resize_dev_p010: the
 * rectangle read from d_bounds when the kernels execute; one that cannot be used adds exactly 1 to *d_status, once per call, and leaves both
 * outputs and the workspace untouched (d_status as in mf_crop_resize_dev_u16c3).
 * Refused with MF_ERR_INVALID_ARG before anything is launched: null pointers, n <= 0, any two of the four plane stacks overlapping, an odd W, H,
 * out_W or out_H or one outside 2 .. 32,767, a plane pointer that is not 2-byte aligned, too many tiles, and (host rectangle) an empty or
 * out-of-frame rectangle. */
size_t mf_crop_resize_p010_workspace_bytes(int out_W, int out_H);
int mf_crop_resize_p010(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, int n, int W, int H, int left, int top,
                        int right, int bottom, int out_W, int out_H, void* d_work, void* stream);
int mf_crop_resize_dev_p010(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_out_y, uint16_t* d_out_uv, int n, int W, int H,
                            const int32_t* d_bounds, int out_W, int out_H, void* d_work, int32_t* d_status, void* stream);

/* ---- the tracker in front of it: FAST corners and pyramidal Lucas-Kanade per sub-frame (mfs.py:492-516, 581-629) ----
 * What the reference asks of cv2.FastFeatureDetector_create().detect and cv2.calcOpticalFlowPyrLK (their defaults), for one-channel uint8
 * images ONLY (grey clips, NV12 luma): bit for bit what tests/track_model.py computes, which restates OpenCV 4.5-4.10 with the five sums of
 * an LK window taken exactly in integers and rounded to float32 once (cv2 accumulates them in float32 in a SIMD-dependent order).  The
 * RANSAC outlier step and the homography are the caller's (meshflow_amd/host.py; the outlier step also as mf_ransac_inliers_f32 below).
 * Sub-frames: as at mfs.py:493-504 a W x H frame is cut into sub-frames of ceil(W / sub_cols) x ceil(H / sub_rows) pixels, the last column /
 * row smaller; there are S = ceil(W / sub_w) * ceil(H / sub_h) of them (possibly fewer than sub_rows * sub_cols), numbered left outer, top
 * inner.  EACH SUB-FRAME IS AN IMAGE OF ITS OWN: FAST's 3-pixel margin, the pyramid's and the derivative's borders fall at its edges, and
 * coordinates are relative to its top-left pixel.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): W, H in 1 .. 32,767; sub_rows in 1 .. H, sub_cols in 1 .. W; every sub-frame at least
 * MF_TRACK_MIN_SUBFRAME pixels wide and high (a reflect-101 border needs two samples; sub-frames below 7 pixels simply have no corners);
 * max_per_subframe in 1 .. MF_TRACK_MAX_PER_SUBFRAME; threshold in 1 .. 254; n (images, or pairs) >= 1 with 2 * n * S <= 65,535 (cut longer
 * clips into chunks); null pointers; early and late stacks that overlap the outputs.
 * mf_fast_corners_u8: d_grey [n][H][W].  d_points [n][S][max_per_subframe][2] float32 (x, y), row-major order (y outer, x inner) -- if a
 * sub-frame has more corners than max_per_subframe, the first ones in that order are kept; d_counts [n][S] int32 the TRUE number of corners;
 * d_status [n][S] int32, bit MF_TRACK_OVERFLOW set where the true count exceeds max_per_subframe, 0 otherwise.  Entries of d_points behind a
 * sub-frame's corners are not written.
 * mf_lk_track_u8: d_early, d_late [n_pairs][H][W] (for the adjacent pairs of a clip: d_late = d_early + W * H); d_points, d_counts as above
 * (counts above max_per_subframe are read as max_per_subframe).  d_moved [n_pairs][S][max_per_subframe][2] float32 the tracked positions,
 * d_found [n_pairs][S][max_per_subframe] uint8 cv2's status; entries behind a sub-frame's corners are not written.
 * d_work: mf_track_workspace_bytes(...) bytes (n_pairs: the larger of both calls' n), 16-byte aligned: the corner mask of the first call, the
 * pyramid levels 1-3 of both stacks of the second (each level as large as the largest sub-frame's; a frame shared by two pairs is reduced
 * twice).  0 for arguments outside the limits.  Both calls are asynchronous on `stream`. */
#define MF_TRACK_MIN_SUBFRAME 2
#define MF_TRACK_MAX_PER_SUBFRAME 16384
#define MF_TRACK_OVERFLOW 1
size_t mf_track_workspace_bytes(int n_pairs, int W, int H, int sub_rows, int sub_cols, int max_per_subframe);
int mf_fast_corners_u8(const uint8_t* d_grey, int n, int W, int H, int sub_rows, int sub_cols, int max_per_subframe, int threshold,
                       float* d_points, int32_t* d_counts, int32_t* d_status, void* d_work, void* stream);
int mf_lk_track_u8(const uint8_t* d_early, const uint8_t* d_late, int n_pairs, int W, int H, int sub_rows, int sub_cols,
                   int max_per_subframe, const float* d_points, const int32_t* d_counts, float* d_moved, uint8_t* d_found, void* d_work,
                   void* stream);

/* ---- between the two: outlier rejection per sub-frame and the packing of the survivors (mfs.py:564-579, 614, 626; 521, 578) ----
 * What the reference asks of cv2.findHomography(..., method=cv2.RANSAC)[1] per sub-frame, as a specification of its own that a kernel can
 * equal: bit for bit tests/ransac_model.py (stateless hash sampling, cv2's degenerate-sample test, a closed-form 4-point fit in float64, a
 * division-free error test, three times cv2's adaptive iteration count, the best sample's consensus set as the mask; that file lists
 * where it deviates from cv2 and from meshflow_amd/host.py's ransac_inliers).  The homography over the survivors stays with the caller
 * (host.lsq_homography).
 * Layouts: d_points, d_moved [n_pairs][S][max_per_subframe][2] float32, d_counts [n_pairs][S] int32 and d_found [n_pairs][S][max_per_subframe]
 * uint8 as mf_fast_corners_u8 / mf_lk_track_u8 leave them (counts above max_per_subframe are read as max_per_subframe, negative ones as 0).
 * mf_ransac_inliers_f32: the candidates of a sub-frame are its points i < count with d_found != 0, k of them.  d_inlier [n_pairs][S]
 * [max_per_subframe] uint8: 1 for the candidates in the consensus set of the best hypothesis, 0 everywhere else (every entry is written).
 * d_info [n_pairs][S][4] int32: {status, k, inliers, iterations run}; status MF_RANSAC_OK, MF_RANSAC_TOO_FEW (count, k below min_features
 * -- mfs.py:614, 626 -- or k < 4; no iteration runs) or MF_RANSAC_NO_CONSENSUS (no sample had 4 inliers; collinear or identical points end
 * here after max_iters skipped iterations): the sub-frame then contributes nothing, which is what the caller of cv2 does with a None mask.
 * d_work: mf_ransac_workspace_bytes(...) bytes, 16-byte aligned: the compacted candidates of sub-frames that hold more than 1,024 of them (16
 * bytes for max_per_subframe <= 1,024); 0 for arguments outside the limits.
 * mf_track_gather_f64: per pair the inliers of the sub-frames with status MF_RANSAC_OK, sub-frame order outer, point order inner, as float64
 * (x, y) = float32 coordinate + the sub-frame's integer offset (column * sub_w, row * sub_h) (mfs.py:578: exact), back to back in d_early,
 * d_late [total][2] -- capacity n_pairs * S * max_per_subframe pairs -- with d_offsets [n_pairs + 1] int32: the layout mf_vertex_motion_f64
 * takes.  A pair with fewer than min_features survivors (mfs.py:521) gets an empty range and MF_TRACK_PAIR_TOO_FEW in d_pair_status
 * [n_pairs] int32, 0 otherwise.  No atomics: the order is part of the contract.  S = the sub-frames of W x H cut sub_rows x sub_cols.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): n_pairs >= 1 and S >= 1 with 2 * n_pairs * S <= 65,535; max_per_subframe in 1 ..
 * MF_TRACK_MAX_PER_SUBFRAME; the tracker's limits on W, H, sub_rows, sub_cols; threshold finite and > 0; 0 < confidence < 1; max_iters in
 * 1 .. MF_RANSAC_MAX_ITERS; min_features >= 1; null pointers; float and int arrays 8- / 4-byte aligned; outputs that overlap inputs or each other.
 * Both calls are asynchronous on `stream`. */
#define MF_RANSAC_OK 0
#define MF_RANSAC_TOO_FEW 1
#define MF_RANSAC_NO_CONSENSUS 2
#define MF_RANSAC_MAX_ITERS 65536
#define MF_TRACK_PAIR_TOO_FEW 1
size_t mf_ransac_workspace_bytes(int n_pairs, int S, int max_per_subframe);
int mf_ransac_inliers_f32(const float* d_points, const float* d_moved, const int32_t* d_counts, const uint8_t* d_found, int n_pairs, int S,
                          int max_per_subframe, int min_features, double threshold, double confidence, int max_iters, uint32_t seed,
                          uint8_t* d_inlier, int32_t* d_info, void* d_work, void* stream);
int mf_track_gather_f64(const float* d_points, const float* d_moved, const uint8_t* d_inlier, const int32_t* d_info, int n_pairs, int W, int H,
                        int sub_rows, int sub_cols, int max_per_subframe, int min_features, double* d_early, double* d_late,
                        int32_t* d_offsets, int32_t* d_pair_status, void* stream);

/* ---- the homography over a pair's survivors (mfs.py:524-526) ----
 * What the reference asks of cv2.findHomography(early, late)[0] per pair, as a specification of its own that a kernel can equal:
 * bit for bit tests/homography_model.py (Hartley's similarity exactly as meshflow_amd/host.py's _normalisation defines it, the 9 x 9 normal matrix
 * of the DLT rows from 24 sums -- the 2K x 9 matrix is never formed --, its smallest eigenvector by cyclic Jacobi rotations, the way back
 * in closed form, h22 = 1; that file lists where it deviates from host.lsq_homography and from cv2: no Levenberg-Marquardt refinement, no
 * SVD).  Every sum over a pair's points has ONE order, the same for every launch: 256 strided partial sums from +0.0, a halving tree per
 * 64 of them, (w0 + w1) + (w2 + w3).  No atomics: the order is part of the contract.
 * Layouts: d_early, d_late [K_total][2] float64 and d_offsets [n_pairs + 1] int32 as mf_track_gather_f64 leaves them and
 * mf_vertex_motion_f64 takes them.  A pair whose range is not 0 <= d_offsets[p] <= d_offsets[p + 1] <= K_total is read as empty: no load
 * leaves d_early / d_late whatever d_offsets holds.  d_h [n_pairs][9] float64, row-major, what mf_vertex_motion_f64 takes as d_hom.
 * d_info [n_pairs][4] int32: {status, K, sweeps run, index of the chosen eigenvalue}.  d_diag [n_pairs][8] float64: {early scale, late
 * scale, early centroid x, y, late centroid x, y, smallest eigenvalue, second smallest}: a mismatch against the model names its stage.
 * Refusals per pair -- d_h is then the IDENTITY, so that later stages stay defined until the caller has looked, and d_diag is 0 where
 * undefined --: MF_HFIT_TOO_FEW (K < 4), MF_HFIT_COLLINEAR (either cloud on one line or one point: the smaller eigenvalue of its centred
 * second moments <= 1e-18 max(larger, 1); non-finite coordinates end here too), MF_HFIT_AT_INFINITY (|h22| <= 1e-12 max |h|, host.py's
 * test) and MF_HFIT_NOT_CONVERGED (a rotation in each of 30 sweeps: never expected).
 * d_work: mf_homography_fit_workspace_bytes(n_pairs) bytes, 8-byte aligned: 24 doubles per pair between the two kernels; 0 for n_pairs
 * outside the limits.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): n_pairs in 0 .. 32,767 (the tracker's own: 2 * n_pairs * S <= 65,535), K_total >= 0; null
 * pointers (d_early and d_late may be null where K_total is 0); float64 and int32 arrays 8- / 4-byte aligned; outputs that overlap inputs,
 * the workspace or each other.  n_pairs == 0 succeeds and launches nothing.  Asynchronous on `stream`. */
#define MF_HFIT_OK 0
#define MF_HFIT_TOO_FEW 1
#define MF_HFIT_COLLINEAR 2
#define MF_HFIT_AT_INFINITY 3
#define MF_HFIT_NOT_CONVERGED 4
#define MF_HFIT_MAX_PAIRS 32767
size_t mf_homography_fit_workspace_bytes(int n_pairs);
int mf_homography_fit_f64(const double* d_early, const double* d_late, const int32_t* d_offsets, int n_pairs, int K_total, double* d_h,
                          int32_t* d_info, double* d_diag, void* d_work, void* stream);

/* ---- the scores from tracked features: cropping ratio and distortion score (mfs.py:1196-1212 after the tracker) ----
 * The reference tracks (unstabilized frame t, cropped frame t) and reads two numbers off each homography: 1 / (h00 h11), and the ratio of
 * the two largest eigenvalue magnitudes of its affine part; the clip's cropping ratio is the float32 mean of the first, its distortion
 * score the float32 MINIMUM of the second (the code's choice at mfs.py:1212; its docstring says "greatest").  Bit for bit
 * tests/scores_model.py: the eigenvalues of the 2 x 2 block in closed form from float64 + - * / and sqrt (not np.linalg.eigvals, which no
 * kernel equals bit for bit; the two agree within one float32 ulp, tests/test_scores_model.py), IEEE throughout -- a zero h00 h11 gives an
 * infinity, nothing is refused -- and every float32 NaN is the quiet NaN 0x7FC00000.
 * d_h [pairs][9] float64, row-major, as mf_homography_fit_f64 leaves them.  d_info: that call's record [pairs][4] int32, or null.  With a
 * record only the pairs whose status is MF_HFIT_OK are scored (a refused pair holds the identity, which is no measurement); without one,
 * all are.  d_pair_scores [pairs][2] float32: {ratio, distortion} of each pair, two NaNs where it was not scored.  d_scores float[2]:
 * {cropping_ratio, distortion_score}, two NaNs where no pair was scored; the distortion score is a NaN where any scored pair's is.
 * d_record int32[2]: {pairs scored, the first pair that was not scored or -1}.
 * The mean is float32(sum / count) with the float64 sum in ONE order, the homography fit's: 256 strided partial sums from +0.0, a halving
 * tree per 64 of them, (w0 + w1) + (w2 + w3); the minimum folds in the same order.  No atomics.  One launch of one 256-lane workgroup.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): 1 <= pairs <= MF_SCORES_MAX_PAIRS (1,048,576); null pointers other than d_info; d_h
 * 8-byte and the other arrays 4-byte aligned; outputs that overlap inputs or each other.  Asynchronous on `stream`. */
#define MF_SCORES_MAX_PAIRS 1048576
int mf_feature_scores_f64(const double* d_h, const int32_t* d_info, int pairs, float* d_pair_scores, float* d_scores, int32_t* d_record,
                          void* stream);

/* ---- the luma of a colour or 16-bit clip: what the tracker calls above take (cv2's conversion in front of FAST, mfs.py:505-516) ----
 * d_src: a contiguous stack of n frames of H x W pixels; d_dst: [n][H][W] uint8.  Bit for bit tests/luma_model.py, integers only:
 *   mf_luma_u8c3   [n][H][W][3] uint8 BGR:   (b 3735 + g 19235 + r 9798 + 16384) >> 15 -- OpenCV's 8U COLOR_BGR2GRAY, 15-bit coefficients
 *                  that sum to 32768
 *   mf_luma_u8c4   [n][H][W][4] uint8 BGRA:  the same on channels 0-2; channel 3 is ignored (COLOR_BGRA2GRAY)
 *   mf_luma_u16c3  [n][H][W][3] uint16 BGR:  y16 = (b 1868 + g 9617 + r 4899 + 8192) >> 14 -- OpenCV's 16U path, 14-bit coefficients that sum
 *                  to 16384 --, then y16 >> 8
 *   mf_luma_u16    [n][H][W] uint16:       y >> 8 -- the luma plane of a P010 / P012 / P016 clip, whose samples are MSB-aligned
 * red_first = 1 swaps the roles of channels 0 and 2 (COLOR_RGB2GRAY / RGBA).  A 16-bit value becomes a byte by TRUNCATION (>> 8, no
 * rounding): cv2's FAST takes no 16-bit image, so this rule is the library's own, one rule for BGR and for P010.  The constants are restated
 * from OpenCV 4.5-4.10; tests/test_cv2_luma_crosscheck.py compares them with cv2 where there is one.
 * One launch per 2^28 pixels over the flat pixel stream, 64-bit pixel indices (n * W * H may exceed 2^32).  d_src and d_dst may start at any byte
 * (a uint16 source: at any even byte); 16-byte accesses are used where the addresses allow them, narrower ones elsewhere.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): null pointers; n < 1; W or H outside 1 .. 32,767; red_first outside {0, 1}; a uint16 source
 * at an odd address; a destination that overlaps the source.  Asynchronous on `stream`. */
int mf_luma_u8c3(const void* d_src, int n, int W, int H, int red_first, uint8_t* d_dst, void* stream);
int mf_luma_u8c4(const void* d_src, int n, int W, int H, int red_first, uint8_t* d_dst, void* stream);
int mf_luma_u16c3(const void* d_src, int n, int W, int H, int red_first, uint8_t* d_dst, void* stream);
int mf_luma_u16(const void* d_src, int n, int W, int H, uint8_t* d_dst, void* stream);

/* ---- the row before the path: vertex-motion accumulation (mfs.py:236-452 from the matched features on) ----
 * Replaces the Python loops of _get_vertex_nearby_feature_residual_velocities (mfs.py:365-452), the medians, global
 * motion and median blur of _get_unstabilized_vertex_velocities (mfs.py:316-362, everything after the tracker call)
 * and the running sum of _get_unstabilized_vertex_displacements_and_homographies (mfs.py:268-282).  The tracker
 * itself (_get_matched_features_and_homography, mfs.py:455-629: FAST / LK / RANSAC) stays with the caller.
 * d_early, d_late: [total_features][2] float64 (x, y), the features of the P frame pairs back to back;
 * d_offsets: [P+1] int32, pair p owns features d_offsets[p] .. d_offsets[p+1]-1 (an empty range = no features);
 * max_per_pair >= every range length; d_hom: [P][9] float64 early-to-late homographies.
 * d_velocities: [P][(R+1)*(C+1)][2] float32 (what _get_unstabilized_vertex_velocities returns per pair);
 * d_displacements: [P+1][(R+1)*(C+1)][2] float64, [0] = 0 (mfs.py:271).
 * d_work: mf_vertex_motion_workspace_bytes(...) bytes, 16-byte aligned.  d_status: one int32 (zero it before the
 * call); non-zero afterwards = the reference's math.sqrt would have raised ValueError (mfs.py:444). */
size_t mf_vertex_motion_workspace_bytes(int total_features, int max_per_pair, int P, int R, int C);
int mf_vertex_motion_f64(const double* d_early, const double* d_late, const int32_t* d_offsets, const double* d_hom,
                         int P, int total_features, int max_per_pair, int W, int H, int R, int C,
                         int ellipse_rows, int ellipse_cols, float* d_velocities, double* d_displacements,
                         void* d_work, int32_t* d_status, void* stream);

/* ---- online path smoothing: blocks of frames pushed in, a sliding window per frame, zero latency ----
 * The reference has the offline optimisation only (mfs.py:632-710); this is a specification of the project's own, bit for bit
 * tests/online_model.py.  Per series s of S = (R+1)(C+1)*2, frames numbered from 0 since the session began, `seen` of them before this call:
 *   path     C_0 = 0, C_t = C_{t-1} + (double)v_t: the sequential float64 running sum of mf_vertex_motion_f64's d_displacements, formed
 *            here from the velocities and the one carried C -- a stream pushed in blocks of any sizes yields the bits of one block
 *   window   xi has newest frame xi and covers Phi = [max(0, xi - window + 1), xi]; taps w_d = exp(-((3 / omega) d)^2), 1 <= d <= omega,
 *            made on the host (d_taps [omega] float64, d_taps[d - 1] = w_d); no d = 0 tap
 *   weights  lam_t for t < xi is the adaptive weight of pair (t -> t + 1), known once frame t + 1 has arrived; lam_xi = lam_newest, the
 *            weight of the identity homography (what the reference gives its last frame, mfs.py:273-274, 757)
 *   start    x_t = q_t, window xi - 1's solution, for t < xi; x_xi = C_xi + (q_{xi-1} - C_{xi-1}); x_0 = C_0 in window 0
 *   sweep    `iters` times, every t of Phi: acc = sum w_|d| x_{t+d} and sw = sum w_|d| over d = -omega .. omega ascending, without d = 0
 *            and every t + d outside Phi, both from 0.0, a rounded multiply then a rounded add per term (no fma);
 *            x'_t = ((C_t + beta q_t) + (2 lam_t) acc) / ((1 + beta) + (2 lam_t) sw) for t < xi and
 *            x'_xi = (C_xi + (2 lam_xi) acc) / (1.0 + (2 lam_xi) sw) -- the newest frame has no q --, IEEE division
 *   result   P_xi = x_xi after the last sweep; the whole x is window xi + 1's q
 * One block of n new frames: d_vel [n][S] float32, row i the velocity of the pair that ENDS at new frame i (mf_vertex_motion_f64's
 * d_velocities); d_lam_known [n] float64, entry i the weight of the frame BEFORE new frame i.  Row 0 / entry 0 are not read when seen is 0.
 * d_c_out, d_p_out [n][S] float64: C and P of the new frames, mf_jacobi_f64's [F][S] layout.
 * State, updated in place, zeroed by the caller before the first call (seen = 0 reads none of it): d_c_state, d_q_state [window - 1][S]
 * and d_lam_state [window - 1] float64; afterwards row j holds frame seen + n - (window - 1) + j, zeros where that frame does not exist,
 * and the last row of d_lam_state holds lam_newest.  The caller adds n to `seen`.
 * The n windows run in order inside ONE launch of one wavefront per series (frame t in lane t mod window; x in 1 KB of LDS); a second,
 * 64-lane launch behind it shifts d_lam_state, which every wavefront of the first reads.  No atomics; a second call on the same inputs
 * gives the same bytes; a non-finite value stays in its series.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): n >= 1, S >= 1; window in 2 .. MF_ONLINE_MAX_WINDOW; omega in 1 .. MF_ONLINE_MAX_OMEGA;
 * iters in 1 .. MF_ONLINE_MAX_ITERS; beta and lam_newest finite and >= 0; seen >= 0; null pointers; d_vel 4-byte and every float64 array
 * 8-byte aligned; outputs that overlap inputs, the state or each other; state arrays that overlap inputs or each other.
 * Asynchronous on `stream`. */
#define MF_ONLINE_MAX_WINDOW 64
#define MF_ONLINE_MAX_OMEGA 64
#define MF_ONLINE_MAX_ITERS 1000
int mf_online_smooth_f64(const float* d_vel, const double* d_lam_known, const double* d_taps, int n, int S, int omega, int window, int iters,
                         double beta, double lam_newest, int64_t seen, double* d_c_state, double* d_q_state, double* d_lam_state,
                         double* d_c_out, double* d_p_out, void* stream);

/* ---- online path smoothing with a fixed lag: each frame handed out `lag` windows after it arrived ----
 * mf_online_smooth_f64 with one more argument, `lag` in 0 .. window - 1, and another choice of what is handed out; bit for bit
 * tests/online_lag_model.py.  Window xi's solution holds, beside x_xi, refined values of the frames before it; with lag frames of look-ahead
 *   P^lag_t = x_t in window t + lag's solution after its last sweep;  C^lag_t = C_t.
 * d_c_out, d_p_out [n][S] float64: row i holds C and x of frame seen + i - lag as they stand after window seen + i's last sweep.  A row whose
 * frame does not exist (seen + i - lag < 0) is written as 0.0 in both arrays: no output byte is left undefined.  lag = 0 gives
 * mf_online_smooth_f64's bytes.
 * The solve, the state update and the second (weights) launch are mf_online_smooth_f64's: the state after a call does not depend on lag,
 * which selects what is handed out and never enters the arithmetic.  When the stream ends, the frames not yet handed out are the last
 * min(lag, seen) rows of d_c_state / d_q_state, oldest first: the final window's solution.
 * The same mapping, from the sweep kernel's second instantiation: the lane whose frame has age `lag` in the window stores its own C and x,
 * where the plain kernel's newest lane does.  No atomics; a second call on the same inputs gives the same bytes.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): those of mf_online_smooth_f64, then lag outside 0 .. window - 1.
 * Asynchronous on `stream`. */
int mf_online_smooth_lag_f64(const float* d_vel, const double* d_lam_known, const double* d_taps, int n, int S, int omega, int window, int lag,
                             int iters, double beta, double lam_newest, int64_t seen, double* d_c_state, double* d_q_state,
                             double* d_lam_state, double* d_c_out, double* d_p_out, void* stream);

/* ---- online path smoothing of a group: K rows of n frames, each row a different stream of B, in one pair of launches ----
 * mf_online_smooth_f64 per row, bit for bit (tests/online_model.py remains the specification): row r is the single call on
 *   d_vel + r n S, d_lam_known + r n, d_c_out + r n S, d_p_out + r n S      the row's velocities [n][S], weights [n] and outputs [n][S]
 *   seen = d_seen[r]                                                        that stream's frames so far, [K] int64 ON THE DEVICE
 *   d_c_state + id (window - 1) S, d_q_state likewise, d_lam_state + id (window - 1)     with id = d_ids[r], [K] int32 on the device
 * with the same operations in the same order, no fma, IEEE division.  d_c_state, d_q_state [B][window - 1][S] and d_lam_state [B][window - 1]
 * are the states of B streams stacked; d_taps, omega, window, iters, beta and lam_newest are shared by the rows.
 * A row with d_seen[r] == 0 reads nothing of its stream's state (a per-stream reset is that zero, no memset); a stream not named in d_ids
 * keeps its state bytes; a row whose id is outside 0 .. B - 1 or whose d_seen[r] is negative touches no memory at all, its output rows
 * included.  The ids of one call must be DISTINCT: that is the caller's duty, the library cannot see them without a wait (two rows on one
 * stream would race on its state; every access still lies inside the stacks).  The caller adds n to each pushed stream's count.
 * Two launches whatever K and n are: the sweep on a grid (S, K), one wavefront per workgroup, workgroup (s, r) series s of row r; then one
 * workgroup per row shifts that stream's weights.  No atomics; a second call on the same inputs gives the same bytes; a non-finite value
 * stays in its series of its stream.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): those of mf_online_smooth_f64 (there is no host `seen`), plus K < 1, B < 1, K > B,
 * K > MF_ONLINE_GROUP_MAX_ROWS, null d_ids or d_seen, d_ids not 4-byte or d_seen not 8-byte aligned; the overlap rules take d_ids and d_seen
 * as inputs, the K n rows as the outputs and the whole stacks as the state.  Asynchronous on `stream`. */
#define MF_ONLINE_GROUP_MAX_ROWS 65535
int mf_online_smooth_group_f64(const float* d_vel, const double* d_lam_known, const double* d_taps, const int32_t* d_ids, const int64_t* d_seen,
                               int K, int B, int n, int S, int omega, int window, int iters, double beta, double lam_newest, double* d_c_state,
                               double* d_q_state, double* d_lam_state, double* d_c_out, double* d_p_out, void* stream);

/* ---- online path smoothing of a group with a fixed lag: mf_online_smooth_lag_f64 per row ----
 * mf_online_smooth_group_f64 with one more argument, `lag` in 0 .. window - 1, shared by the rows; row r is mf_online_smooth_lag_f64 on the
 * slices mf_online_smooth_group_f64 names, bit for bit (tests/online_lag_model.py is the specification): row i of row r's outputs holds C and
 * x of frame d_seen[r] + i - lag as they stand after window d_seen[r] + i's last sweep, 0.0 in both arrays where that frame does not exist.
 * Of row r's n output rows the trailing max(0, d_seen[r] + n - lag) - max(0, d_seen[r] - lag) are frames, so rows of one call may differ in
 * how many they hand out.  The state after a call does not depend on lag; the frames a stream still owes are the last min(lag, seen) rows of
 * its slices of d_c_state / d_q_state.  lag = 0 gives mf_online_smooth_group_f64's bytes.
 * The same two launches: the sweep on a grid (S, K) from the group kernel's lagged twin, then mf_online_smooth_group_f64's own weights launch.
 * A row whose id is outside 0 .. B - 1 or whose d_seen[r] is negative touches no memory; distinct ids are the caller's duty.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): those of mf_online_smooth_group_f64, then lag outside 0 .. window - 1.
 * Asynchronous on `stream`. */
int mf_online_smooth_group_lag_f64(const float* d_vel, const double* d_lam_known, const double* d_taps, const int32_t* d_ids, const int64_t* d_seen,
                                   int K, int B, int n, int S, int omega, int window, int lag, int iters, double beta, double lam_newest,
                                   double* d_c_state, double* d_q_state, double* d_lam_state, double* d_c_out, double* d_p_out, void* stream);

/* ---- the pixels a lagged group owes: store K new frames in a ring and hand out the frames whose slots they take, in one launch ----
 * A specification of the project's own, bit for bit tests/ring_model.py (`exchange`).  d_ring [B][lag][N] bytes: frame t of stream b lives in
 * slot t mod lag while it is owed.  d_new [K][N]: one new frame per row.  d_rows [K][3] int32 ON THE DEVICE: (id, slot, out_row) per row.
 *   out_row >= 0   d_out[out_row] = d_ring[id][slot], then d_ring[id][slot] = d_new[r]
 *   out_row <  0   d_ring[id][slot] = d_new[r] only
 * d_out [K][N]: room for K frames, of which the first M <= K are written, M the number of rows that hand a frame out; the caller numbers
 * them 0 .. M - 1 (the rows are on the device, so the library takes d_out as K frames long).  A row whose id is outside
 * 0 .. B - 1, whose slot is outside 0 .. lag - 1 or whose out_row is K or more touches no memory.  The ids of one call must be DISTINCT: the
 * caller's duty, as in mf_online_smooth_group_f64 (every access still lies inside the arrays).  Planes of 16-bit samples go through as bytes.
 * One launch on a grid (ceil(N / 4096), K): each lane loads its 16 bytes of the ring and of the new frame, then stores both -- every ring
 * byte is read by the lane that overwrites it, so there are no barriers and no atomics.  16-byte accesses where N is a multiple of 16 and
 * d_ring, d_new and d_out are 16-byte aligned, byte accesses otherwise; nothing past a frame's last byte is read or written.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): K < 1, B < 1, lag < 1, N < 1, K > MF_ONLINE_GROUP_MAX_ROWS; N > MF_RING_MAX_FRAME_BYTES or
 * B lag N above 2^62; a null pointer; d_rows not 4-byte aligned; d_out [K][N] overlapping d_ring or d_new; d_new overlapping d_ring.
 * Asynchronous on `stream`. */
#define MF_RING_MAX_FRAME_BYTES ((int64_t)4096 * 2147483647)
int mf_ring_exchange_u8(uint8_t* d_ring, const uint8_t* d_new, uint8_t* d_out, const int32_t* d_rows, int K, int B, int lag, int64_t N, void* stream);

/* ---- scene cuts: a per-frame signature of tile histograms of luma, and the distance of adjacent signatures ----
 * The reference has nothing of the kind; this is a specification of the project's own, bit for bit tests/cuts_model.py, integers only -- any
 * order of summation gives the same bytes.
 *   signature  of an H x W uint8 frame: 4 x 4 tiles; tile row i covers rows [floor(i H / 4), floor((i + 1) H / 4)), tile columns split W the
 *              same way (a tile is empty where H < 4 or W < 4); 16 counters per tile, counter b = the number of the tile's pixels with
 *              value >> 4 == b; layout [tile_row][tile_col][bin], MF_CUT_COUNTERS = 256 int32 per frame, which sum to H W
 *   distance   D(a, b) = the sum over the 256 counters of |a - b|, 0 .. 2 H W; with W, H <= 32,767 that is below 2^31
 *   decision   the caller's, on the host: frame t starts a new shot iff D_t > floor(threshold * 2 H W) (meshflow_amd/ops.py, find_cuts)
 * mf_frame_signature_u8: d_luma is a contiguous [n][H][W] uint8 stack that may start at any byte (16-byte loads where the address allows,
 * narrower ones elsewhere); d_sig [n][256] int32 is OVERWRITTEN -- the call clears it itself (a memset on `stream`), then one launch per 2^20
 * workgroups adds every strip of a tile to it with integer atomic adds, which commute: a second call gives the same bytes.  Pixel indices are
 * 64-bit (n * W * H may exceed 2^32).
 * mf_cut_distance_i32: d_dist [n] int32; d_dist[0] = D(d_sig_prev, d_sig[0]) where d_sig_prev ([256] int32) is given, else 0;
 * d_dist[i] = D(d_sig[i - 1], d_sig[i]) for the rest.  One launch, no atomics.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): null pointers other than d_sig_prev; n < 1; W or H outside 1 .. MF_CUT_MAX_DIM (32,767);
 * d_sig, d_dist or d_sig_prev not 4-byte aligned; an output that overlaps an input.  Asynchronous on `stream`. */
#define MF_CUT_COUNTERS 256
#define MF_CUT_MAX_DIM 32767
int mf_frame_signature_u8(const uint8_t* d_luma, int n, int W, int H, int32_t* d_sig, void* stream);
int mf_cut_distance_i32(const int32_t* d_sig_prev, const int32_t* d_sig, int n, int32_t* d_dist, void* stream);
/* mf_cut_distance_pairs_i32: the rows are frames of n different streams, each with a predecessor of its own: d_dist[r] = D(d_prev[r], d_sig[r])
 * for d_prev, d_sig [n][256] int32 -- mf_cut_distance_i32's arithmetic, one launch of one workgroup per row, no atomics.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): a null pointer; n < 1; an array not 4-byte aligned; d_dist overlapping either stack.
 * Asynchronous on `stream`. */
int mf_cut_distance_pairs_i32(const int32_t* d_prev, const int32_t* d_sig, int n, int32_t* d_dist, void* stream);

/* ---- path limit: scale a frame's correction so that the mesh still covers a fixed crop rectangle ----
 * The reference has nothing of the kind (its rectangle is a reduction over the whole clip, mfs.py:1103-1106); this is a specification of the
 * project's own, bit for bit tests/path_limit_model.py: float64, the operations in the stated order, each rounded by itself, no fma.
 * d_unstab, d_stab [n][S] float64, S = (R+1)(C+1)*2: the unstabilized path c and the stabilized path p in mf_cell_table_f64's layout.  The
 * warp puts vertex v at g_v + (p_v - c_v), g the integer vertex grid of mfs.py:881-906 as mf_cell_table_f64 forms it.
 *   candidate  k in 1 .. steps (K) has f = (double)k / (double)K; vertex v lies at g_v + f * d_v, d_v = p_v - c_v
 *   polygon    the mesh's perimeter, B = 2 (R + C) vertices: row 0 from column 0 to C-1; column C from row 0 to R-1; row R from column C down
 *              to 1; column 0 from row R down to 1; edge e joins vertex e to vertex (e + 1) mod B.  Interior vertices play no part
 *   rectangle  (left, top, right, bottom) inclusive, mf_crop_resize_u8c3's convention, widened: x0 = left - guard, x1 = right + guard,
 *              y0 = top - guard, y1 = bottom + guard; centre cx = (x0 + x1) * 0.5, cy alike
 *   passes     candidate k passes iff (a) every edge (A, B) is clear of the rectangle -- its bounding box is disjoint from it
 *              (min(ax,bx) > x1, or max(ax,bx) < x0, or the same in y; min(a,b) = a < b ? a : b, max(a,b) = a > b ? a : b), or the cross
 *              products (bx-ax)*(py-ay) - (by-ay)*(px-ax) of the four corners are all > 0, or all < 0 -- and (b) the crossing number of the
 *              centre's rightward ray is odd: an edge counts iff (ay > cy) != (by > cy) and s = (bx-ax)*(cy-ay) - (by-ay)*(cx-ax) has the
 *              sign of by - ay.  Every predicate is affirmative: a NaN makes none true
 *   k_raw_t    the largest k such that every candidate 1 .. k passes; candidate 0 is never tested
 *   k_t        min(k_raw_t, k_{t-1} + rise), k_{-1} = *d_k_prev clamped to 0 .. K, or K where d_k_prev is null: the drop is immediate, the
 *              recovery slew-limited; evaluated as min(K, min_i (k_raw_{t-i} + rise * i), k_prev + rise * (t + 1)) over i <= 63
 *   path       d_out row t = p_t bit for bit when k_t == K, c_t bit for bit when k_t == 0, else c + f * (p - c) with f = (double)k_t / (double)K
 * d_k_raw, d_k [n] int32 and d_out [n][S] float64 are outputs.  Two launches on `stream`, one 64-lane workgroup per frame each: the first
 * stages the boundary in LDS (32 bytes per vertex) and lane j tests candidate j + 1, a ballot gives k_raw; the second takes an integer
 * minimum over the 64 terms and writes the path.  d_k_prev is read on the device, never by the host; the call never waits.  No atomics; a
 * second call on the same inputs gives the same bytes.
 * Limits (MF_ERR_INVALID_ARG, nothing launched): n < 1; R or C < 1; 2 (R + C) > MF_PATH_LIMIT_MAX_BOUNDARY; W or H < 2; a rectangle that is
 * not 0 <= left <= right <= W-1 and 0 <= top <= bottom <= H-1; steps outside 1 .. MF_PATH_LIMIT_MAX_STEPS; rise outside 1 .. steps; guard
 * negative or not finite; a null pointer other than d_k_prev; a float64 array not 8-byte or an int32 array not 4-byte aligned; an output that
 * overlaps an input or another output.  Asynchronous on `stream`. */
#define MF_PATH_LIMIT_MAX_STEPS 64
#define MF_PATH_LIMIT_MAX_BOUNDARY 1024
int mf_path_limit_f64(const double* d_unstab, const double* d_stab, int n, int W, int H, int R, int C, int left, int top, int right, int bottom,
                      double guard, int steps, int rise, const int32_t* d_k_prev, int32_t* d_k_raw, int32_t* d_k, double* d_out, void* stream);
/* mf_path_limit_group_f64: K rows, each ONE frame of a different stream: nothing is chained between the rows.  d_k_prev [K] int32 holds each
 * row's carried step; row r gets the bytes of a one-frame mf_path_limit_f64 call with that word as *d_k_prev:
 *   k_r = min(K_steps, k_raw_r, clamp(d_k_prev[r], 0, K_steps) + rise);  a NEGATIVE d_k_prev[r] says that nothing is carried -- the null
 *   d_k_prev of the single call -- and leaves the rise term out.
 * The candidate test is mf_path_limit_f64's launch as it is (it is per frame); the second launch forms k_r and scales the row with the same
 * statement.  Limits: those of mf_path_limit_f64 with K in the place of n, and d_k_prev, K words, must be given.  Asynchronous on `stream`. */
int mf_path_limit_group_f64(const double* d_unstab, const double* d_stab, int K, int W, int H, int R, int C, int left, int top, int right, int bottom,
                            double guard, int steps, int rise, const int32_t* d_k_prev, int32_t* d_k_raw, int32_t* d_k, double* d_out, void* stream);

/* ---- stability score (mfs.py:1216-1259) of device-resident vertex paths ----
 * d_stab: [F][S] float64 as for mf_jacobi_f64 (S = V*2: x and y of every vertex interleaved).  Per series the fraction of
 * the velocity profile's spectral energy that sits in DFT bins 1..5 (five direct sums + Parseval for the total);
 * d_series: [S] float64 receives those fractions, d_score: [1] float64 the clip-level score
 * (mean over x series + mean over y series) / 2.  F >= 2; with fewer than 7 frames the slice [1:6] of mfs.py:1250-1251 holds
 * fewer bins (bins 1..min(5, F-2)), exactly as in the reference.  Agrees with np.fft to float64 rounding. */
int mf_stability_score_f64(const double* d_stab, int F, int S, double* d_series, double* d_score, void* stream);

/* Device self-test: sqrt() on (0, 0.25] (the ellipse half-width, mfs.py:444) must be correctly rounded; *mismatches
 * receives the number of inputs where it is not (must be 0).  Synchronous. */
int mf_selftest_sqrt(uint64_t n, uint64_t seed, uint64_t* mismatches);

/* Device self-test: the warp kernel's trimmed reciprocal (exact for 0.5 <= |w| <= 2) against IEEE 1.0/w on
 * n hashed inputs; *mismatches receives the number of differing bit patterns (must be 0). Synchronous. */
int mf_selftest_recip(uint64_t n, uint64_t seed, uint64_t* mismatches);

/* Device self-test: the warp kernel's cheap float64 coordinate chain + float32-midpoint guard (hot footprints)
 * against cv2.perspectiveTransform's own arithmetic on n hashed (matrix, position) cases that satisfy the plan's premises.
 * counters[0] = float32 coordinates that differ from the exact chain's WITHOUT the guard raising its flag (must be 0),
 * counters[1] = values the guard flagged (each sends its wavefront to the exact chain), counters[2] = values tested.
 * Synchronous. */
int mf_selftest_fast64(uint64_t n, uint64_t seed, uint64_t counters[3]);

/* ... and how far the cheap chain's float64 values lie from the exact chain's on the same cases: *max_ulps receives the largest
 * distance in float64 ulps (the certified bound is 118, the guard's window 512).  Synchronous. */
int mf_selftest_fast64_margin(uint64_t n, uint64_t seed, double* max_ulps);

/* ---- host-buffer convenience wrappers (synchronous; H2D, kernels, D2H on an internal stream) ----
 * These are what a ctypes stub inside the reference's two methods would call.
 * kernel_ms (optional) receives the device time of the kernels alone, measured with HIP events.
 * The warp wrappers do NOT work in place: input and output frames may not overlap in memory (MF_ERR_INVALID_ARG), also for the
 * contiguous mf_warp_u8c3_host.  On any error return the contents of the output buffers are undefined (a failure that is known
 * before the first frame moves -- bad arguments, a degenerate mesh or an empty rectangle in the crop variant -- leaves them untouched). */
int mf_jacobi_f64_host(const double* b, double* x, const double* taps, const double* lam,
                       const double* inv_on, int F, int S, int omega, int iters, float* kernel_ms);
int mf_warp_u8c3_host(const uint8_t* frames, uint8_t* out, const double* unstab, const double* stab,
                      int n, int W, int H, int R, int C, const uint8_t border_bgr[3],
                      int32_t* crop /* [n][4] */, float* kernel_ms);
/* The same for frames that are separate allocations (the reference's Python lists of per-frame arrays, mfs.py:997, 1100):
 * frames[i] / out[i] point to frame i, H*W*3 bytes each.  mf_warp_u8c3_host is this with frames[i] = frames + i*H*W*3.
 * Both move the clip in chunks of ~16 MB (3 frames at 1080p, 1 at 4K) on four upload and four download threads with their own
 * HIP streams (each takes the next chunk when it is free; plus eight threads that fault the output pages in ahead of the downloads)
 * through a RING of ~720 MB of chunk buffers per direction (40 slots at 1080p, 30 at 4K) -- device memory is O(chunk) whatever the
 * length of the clip (1.5 GB of ring, ~1.75 GB in all at the peak, for any 1080p or 4K clip); a chunk is warped
 * as soon as it has landed (its cell table + plan are built right in front of its warp) and travels back while later chunks are still
 * going up (pageable memory is fine; memory from mf_malloc_host makes the copies truly asynchronous).  MF_PIPE_CHUNK (frames per
 * chunk) / MF_PIPE_SLOTS / MF_PIPE_UP / MF_PIPE_DOWN / MF_PIPE_POPULATE in the environment retune it
 * (read at every call; MF_PIPE_TRACE=1 prints the call's wall-clock milestones on stderr, 2 also every chunk's copy intervals).  Input and output frames must NOT overlap in memory (MF_ERR_INVALID_ARG): output pages are touched
 * while the input is still being read.  Device buffers and streams are kept between calls, grow-only, ONE CACHE PER DEVICE
 * (the calling thread's current device, mf_set_device): calls on one device are serialised, calls on different devices
 * from different host threads run concurrently; mf_host_cache_release() frees all of them. */
int mf_warp_u8c3_host_frames(const uint8_t* const* frames, uint8_t* const* out, const double* unstab, const double* stab,
                             int n, int W, int H, int R, int C, const uint8_t border_bgr[3],
                             int32_t* crop /* [n][4] */, float* kernel_ms);
/* ... followed by the next step of stabilize(), _crop_frames (mfs.py:159, 1111-1157), in the same pipeline: before any frame
 * moves, the cell tables of the whole clip are built (piece by piece, into one scratch table) and the clip-level rectangle
 * {max left, max top, min right, min bottom} (mfs.py:1103-1106) taken from them (mf_crop_scan_f64 + mf_crop_reduce: the edge scans look
 * at the coordinate maps only) and written to
 * bounds[4]; then every chunk goes up, is warped, cropped to the rectangle and resized back to W x H (mf_crop_resize_u8c3) and comes
 * down in ONE phase, both PCIe directions busy throughout: cropped[i] receives frame i of what stabilize() hands to the encoder.
 * `out` (the uncropped stabilized frames) may be NULL: they then never cross PCIe.  A degenerate mesh (MF_ERR_DEGENERATE) or an empty
 * rectangle (MF_ERR_INVALID_ARG: cv2.resize fails on an empty source) ends the call before any frame is uploaded or any output byte
 * written; bounds[] and crop[] are written in the second case. */
int mf_warp_crop_u8c3_host_frames(const uint8_t* const* frames, uint8_t* const* out /* may be NULL */, uint8_t* const* cropped,
                                  const double* unstab, const double* stab, int n, int W, int H, int R, int C,
                                  const uint8_t border_bgr[3], int32_t* crop /* [n][4] */, int32_t bounds[4], float* kernel_ms);
/* _crop_frames (mfs.py:1111-1157, called at mfs.py:159) BY ITSELF on host frames: frames[i] (H*W*3 bytes each) are cropped to the
 * inclusive rectangle {left, top, right, bottom} and scaled back to W x H (mf_crop_resize_u8c3) into cropped[i], through the same
 * ring of chunk buffers and copy threads as the warp wrappers (upload, resize, download of the chunks all overlap).  An empty or
 * out-of-frame rectangle is MF_ERR_INVALID_ARG before any output byte is written. */
int mf_crop_resize_u8c3_host_frames(const uint8_t* const* frames, uint8_t* const* cropped, int n, int W, int H, int left, int top,
                                    int right, int bottom, float* kernel_ms);
/* The three host calls for single-channel uint8 frames (mfs.py:909-1108 and 1111-1157 on 2-D frames, mfs.py:942, 1129): frames[i] /
 * out[i] / cropped[i] point to H*W bytes each; the border byte as in mf_warp_u8c1.  The same ring: chunks are sized by bytes (~8 frames of
 * 1080p grey per chunk), the same up-front crop scan, overlap refusal and degenerate-mesh refusal before any output byte.  The frames and
 * crop values are those of mf_warp_u8c1 / mf_crop_resize_u8c1.  Limits: 2 <= W, H <= 32,767 (1 for the resize alone), R, C <= 64. */
int mf_warp_u8c1_host_frames(const uint8_t* const* frames, uint8_t* const* out, const double* unstab, const double* stab,
                             int n, int W, int H, int R, int C, uint8_t border, int32_t* crop /* [n][4] */, float* kernel_ms);
int mf_warp_crop_u8c1_host_frames(const uint8_t* const* frames, uint8_t* const* out /* may be NULL */, uint8_t* const* cropped,
                                  const double* unstab, const double* stab, int n, int W, int H, int R, int C,
                                  uint8_t border, int32_t* crop /* [n][4] */, int32_t bounds[4], float* kernel_ms);
int mf_crop_resize_u8c1_host_frames(const uint8_t* const* frames, uint8_t* const* cropped, int n, int W, int H, int left, int top,
                                    int right, int bottom, float* kernel_ms);
/* The warp + crop and the crop-alone host calls to a caller-chosen output size (both formats): cropped[i] points to out_W * out_H * channels
 * bytes (mf_crop_resize_to_u8c3 / _u8c1 of the chunk).  The ring's slots and chunks are sized by the larger of the input and the output
 * frame; the overlap, degenerate-mesh and empty-rectangle refusals are those of the calls above (out_W / out_H outside 1 .. 32,767:
 * MF_ERR_INVALID_ARG before anything moves). */
int mf_warp_crop_to_u8c3_host_frames(const uint8_t* const* frames, uint8_t* const* out /* may be NULL */, uint8_t* const* cropped,
                                     const double* unstab, const double* stab, int n, int W, int H, int R, int C,
                                     const uint8_t border_bgr[3], int out_W, int out_H, int32_t* crop /* [n][4] */, int32_t bounds[4],
                                     float* kernel_ms);
int mf_crop_resize_to_u8c3_host_frames(const uint8_t* const* frames, uint8_t* const* cropped, int n, int W, int H, int left, int top,
                                       int right, int bottom, int out_W, int out_H, float* kernel_ms);
int mf_warp_crop_to_u8c1_host_frames(const uint8_t* const* frames, uint8_t* const* out /* may be NULL */, uint8_t* const* cropped,
                                     const double* unstab, const double* stab, int n, int W, int H, int R, int C,
                                     uint8_t border, int out_W, int out_H, int32_t* crop /* [n][4] */, int32_t bounds[4], float* kernel_ms);
int mf_crop_resize_to_u8c1_host_frames(const uint8_t* const* frames, uint8_t* const* cropped, int n, int W, int H, int left, int top,
                                       int right, int bottom, int out_W, int out_H, float* kernel_ms);
int mf_host_cache_release(void);

/* ---- multi-GPU exchange steps, on RCCL directly: ONE process drives the GPUs 0..ndev-1 of a node ----
 * The path shards by contiguous frame range: every GPU warps its own frames (mf_warp_u8c3 on that device) after a replicated
 * mf_jacobi_f64; these are the only two exchanges.  librccl is opened with dlopen at mf_comm_init_all (error -2 when the
 * box has none).  RCCL errors come back as -1000 - ncclResult_t.  All three calls are synchronous; the device buffers
 * handed in must be complete (mf_stream_synchronize the streams that wrote them first).
 *   mf_comm_init_all(ndev)   ncclCommInitAll over devices 0..ndev-1 (rccl.h:236) + one stream per device
 *   mf_allreduce_crop        d_bounds[g]: {left, top, right, bottom} int32 on device g (that shard's mf_crop_reduce result);
 *                            afterwards every device holds the clip-level rectangle {max, max, min, min} (mfs.py:1103-1106):
 *                            16 bytes, one grouped call (ncclAllReduce max on the first pair, min on the second)
 *   mf_gather_frames         d_shards[g] (shard_bytes[g] bytes on device g, the stabilized frames of rank g's frame range) ->
 *                            d_dst on device `root`, back to back in rank order: one group of ncclSend / ncclRecv with
 *                            per-rank byte counts (shards are ragged when ndev does not divide the frame count)
 *   mf_comm_destroy          frees the communicators and streams
 * STATUS: exercised with ONE rank only (tests/test_gpu_nccl_one_rank.py; no multi-GPU node was ever available to the build).  It is
 * the exchange for a single-process C/C++ host that binds this library directly; the Python product and
 * `bench.py --gpus N` do NOT use it -- their one exchange implementation is meshflow_amd/dist.py (one process per GPU,
 * torch.distributed: "nccl" = RCCL), covered at world_size 2 and 8 under gloo (tests/test_dist_gloo.py, tests/test_dist_gloo8.py). */
int mf_comm_init_all(int ndev);
int mf_comm_size(int* ndev);
int mf_allreduce_crop(int32_t* const* d_bounds);
int mf_gather_frames(const uint8_t* const* d_shards, const size_t* shard_bytes, uint8_t* d_dst, int root);
int mf_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* MESHFLOW_HIP_H */
