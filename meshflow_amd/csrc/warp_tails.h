// The tails of footprint_body's other formats (device only, included through warp_body.h): the lane's four pixels at source coordinates
// (u, v) -- taps, blend, crop flags, store -- for uint16 BGR, grey, 4-channel uint8, the coordinate maps, the side planes, the luma plane of a P010 clip
// and the chroma plane of every semi-planar YUV clip (remap_store_chroma: NV12, NV16, P010, P210).
#ifndef MF_WARP_TAILS_H
#define MF_WARP_TAILS_H
#include "warp_coords.h"

namespace mf {

// ---- uint16 frames: cv2.remap of CV_16UC3 (imgwarp.cpp RemapInvoker + remapBilinear<Cast<float, ushort>, RemapNoVec, float>) ----------
// The map quantisation is the 8-bit one (sx = cvRound(32 u), ix = sx >> 5, fx = sx & 31); the weights are BilinearTab_f[fy][fx] =
// {(1 - fy/32)(1 - fx/32), (1 - fy/32) fx/32, fy/32 (1 - fx/32), fy/32 fx/32}, float32 and exact (dyadic); the blend is the scalar
// float32 chain ((S00 w0 + S01 w1) + S10 w2) + S11 w3 with every product and sum rounded on its own (no FMA: -ffp-contract=off), and
// out = saturate_cast<ushort>(t) = min(rint(t), 65535).  Products of 16-bit samples and 10-bit weights need 26 bits: they DO round, so
// the integer tricks of the 8-bit blend do not carry over.
__device__ __forceinline__ uint32_t blend16(float s00, float s01, float s10, float s11, float w0, float w1, float w2, float w3)
{
    const float t = ((s00 * w0 + s01 * w1) + s10 * w2) + s11 * w3;     // (t >= 0: non-negative samples and weights)
    return min((uint32_t)rintf(t), 65535u);
}
// ... for two pixels at once: the same chain per element, on packed float32 (v_pk_mul_f32 / v_pk_add_f32 round each element like the
// scalar instructions)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 blend16x2(f32x2 s00, f32x2 s01, f32x2 s10, f32x2 s11, f32x2 w0, f32x2 w1, f32x2 w2, f32x2 w3)
{
    return ((s00 * w0 + s01 * w1) + s10 * w2) + s11 * w3;
}

// Footprint-level tail of the U16 instantiation of footprint_body: the lane's four pixels at source coordinates (u, v) -- taps, blend,
// crop flags, store.  Deep-interior footprints (every tap two pixels inside the frame, no crop flag possible) take each pixel's two tap
// rows as one 12-byte load apiece (the frame may be only 2-byte aligned: unaligned dword loads); the others take every tap at its
// position clamped into the frame and replace outside taps by the border colour, and a 2 x 2 footprint wholly outside the frame gives the
// border colour itself (float products of the border colour need not sum back to it exactly).  All offsets are 64-bit.
__device__ __forceinline__ void remap_store_u16(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W, int H,
                                                const uint16_t* __restrict__ frames, uint16_t* __restrict__ out, uint64_t border16,
                                                int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint64_t frame_samples = 3ull * (uint64_t)((uint32_t)W * (uint32_t)H);
    const uint16_t* __restrict__ src = frames + (uint64_t)f * frame_samples;
    uint16_t* __restrict__ dst = out + (uint64_t)f * frame_samples;
    uint32_t bx[4], by[4];
    fixed_point(u, v, bx, by);
    const bool deep = deep_interior(bx, by, W, H);
    const bool fast = __ballot(active && !deep) == 0;
    uint32_t o[4][3];                                                   // the lane's 12 output samples
    int c_left = 0, c_top = 0, c_right = W - 1, c_bottom = H - 1;
    if (active) {
        if (fast) {
            // taps as float, [pixel][channel][S00, S01, S10, S11]; then pixels 0 + 1 and 2 + 3 blended pairwise (weights too)
            float sv[4][3][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ix = __builtin_amdgcn_ubfe(bx[j], 5, 17), iy = __builtin_amdgcn_ubfe(by[j], 5, 17);
                const uint16_t* __restrict__ p0 = src + 3ull * (uint64_t)(iy * (uint32_t)W + ix);
                uint32_t a[3], b[3];                                    // B0 G0 | R0 B1 | G1 R1 of rows iy and iy + 1
                __builtin_memcpy(a, p0, 12);
                __builtin_memcpy(b, p0 + 3ull * (uint32_t)W, 12);
                const uint32_t ha[6] = { a[0] & 0xFFFFu, a[0] >> 16, a[1] & 0xFFFFu, a[1] >> 16, a[2] & 0xFFFFu, a[2] >> 16 };
                const uint32_t hb[6] = { b[0] & 0xFFFFu, b[0] >> 16, b[1] & 0xFFFFu, b[1] >> 16, b[2] & 0xFFFFu, b[2] >> 16 };
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sv[j][c][0] = (float)ha[c]; sv[j][c][1] = (float)ha[3 + c];
                    sv[j][c][2] = (float)hb[c]; sv[j][c][3] = (float)hb[3 + c];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j += 2) {
                const f32x2 ax = f32x2{ (float)(bx[j] & 31u), (float)(bx[j + 1] & 31u) } * 0.03125f;
                const f32x2 ay = f32x2{ (float)(by[j] & 31u), (float)(by[j + 1] & 31u) } * 0.03125f;
                const f32x2 ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                const f32x2 w0 = ay0 * ax0, w1 = ay0 * ax, w2 = ay * ax0, w3 = ay * ax;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const f32x2 t = blend16x2(f32x2{ sv[j][c][0], sv[j + 1][c][0] }, f32x2{ sv[j][c][1], sv[j + 1][c][1] },
                                              f32x2{ sv[j][c][2], sv[j + 1][c][2] }, f32x2{ sv[j][c][3], sv[j + 1][c][3] }, w0, w1, w2, w3);
                    // (no clamp: the seven roundings of the chain move t by less than 7 * 2^-9 from the exact blend, a convex combination of
                    // samples <= 65535, so rint(t) <= 65535 -- saturate_cast's clamp never acts here)
                    o[j][c] = (uint32_t)rintf(t.x);
                    o[j + 1][c] = (uint32_t)rintf(t.y);
                }
            }
        } else {
            // frame borders, uncovered pixels (at (W+1, H+1)), crop flags, out-of-range coordinates
            const float fWm1 = (float)(W - 1), fHm1 = (float)(H - 1);
            const bool narrow = narrow_coords(bx, by);
            const uint32_t cval[3] = { (uint32_t)(border16 & 0xFFFFu), (uint32_t)((border16 >> 16) & 0xFFFFu), (uint32_t)((border16 >> 32) & 0xFFFFu) };
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float uu = u[j], vv = v[j];
                const int x = x0 + j;
                if (x < W) {                                            // crop-boundary scan, mfs.py:1075-1098 (exact: Sterbenz)
                    if (fabsf(uu) < 1.0f) c_left = max(c_left, x);
                    if (fabsf(uu - fWm1) < 1.0f) c_right = min(c_right, x);
                    if (fabsf(vv) < 1.0f) c_top = max(c_top, y);
                    if (fabsf(vv - fHm1) < 1.0f) c_bottom = min(c_bottom, y);
                }
                const int sxx = fixed_coord(narrow, bx[j], uu), syy = fixed_coord(narrow, by[j], vv);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                if (ix >= W || ix + 1 < 0 || iy >= H || iy + 1 < 0) {  // the 2 x 2 footprint lies wholly outside: cval
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[j][c] = cval[c];
                    continue;
                }
                const ClampedTaps t = clamped_taps(ix, iy, W, H);
                const uint16_t* __restrict__ q00 = src + 3ull * (uint64_t)(t.r0 + t.cx0);
                const uint16_t* __restrict__ q01 = src + 3ull * (uint64_t)(t.r0 + t.cx1);
                const uint16_t* __restrict__ q10 = src + 3ull * (uint64_t)(t.r1 + t.cx0);
                const uint16_t* __restrict__ q11 = src + 3ull * (uint64_t)(t.r1 + t.cx1);
                const float ax = (float)(sxx & 31) * 0.03125f, ay = (float)(syy & 31) * 0.03125f;
                const float ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                const float w0 = ay0 * ax0, w1 = ay0 * ax, w2 = ay * ax0, w3 = ay * ax;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t s00 = t.in_x0 && t.in_y0 ? (uint32_t)q00[c] : cval[c], s01 = t.in_x1 && t.in_y0 ? (uint32_t)q01[c] : cval[c];
                    const uint32_t s10 = t.in_x0 && t.in_y1 ? (uint32_t)q10[c] : cval[c], s11 = t.in_x1 && t.in_y1 ? (uint32_t)q11[c] : cval[c];
                    o[j][c] = blend16((float)s00, (float)s01, (float)s10, (float)s11, w0, w1, w2, w3);
                }
            }
        }
    }
    if (!fast) crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
    if (active) {
        uint16_t* __restrict__ d = dst + 3ull * (uint64_t)((uint32_t)y * (uint32_t)W + (uint32_t)x0);
        if (x0 + 3 < W) {                                               // 24 bytes at a 2-byte aligned address: unaligned dword stores
            uint32_t w[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) w[k] = o[(2 * k) / 3][(2 * k) % 3] | (o[(2 * k + 1) / 3][(2 * k + 1) % 3] << 16);
            __builtin_memcpy(d, w, 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < W) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[3 * j + c] = (uint16_t)o[j][c];
                }
        }
    }
}

// ---- single-channel uint8 frames: cv2.remap of CV_8UC1 -- the 8-bit fixed-point path of every channel of CV_8UC3, on one channel ------
// out = (sum w_k s_k + 2^14) >> 15 with w = 32 (32 - fx or fx)(32 - fy or fy) (BilinearTab_i) = (t0 (32 - fy) + t1 fy + 512) >> 10, t0 / t1
// the horizontal lerps of the two tap rows.
__device__ __forceinline__ uint32_t blend_c1(uint32_t s00, uint32_t s01, uint32_t s10, uint32_t s11, uint32_t sx, uint32_t sy)
{
    const uint32_t fx = sx & 31u, fy = sy & 31u;
    const uint32_t t0 = umad24(s01, fx, __umul24(s00, 32u - fx)), t1 = umad24(s11, fx, __umul24(s10, 32u - fx));
    return (umad24(t1, fy, __umul24(t0, 32u - fy)) + 512u) >> 10;
}

// The grey window: the plan's STAGED window (cut for 3-byte pixels) re-cut for 1-byte pixels.  The region words give the window's first
// row sy0 and byte column bs = 3 sx0 & ~3 only as origin = P sy0 + bs and src = 3 W sy0 + bs (P = 160, or 112 for COMPACT), so sy0 =
// (src - origin) / (3 W - P) (exact in float32: the quotient is below 2^15 and the error of the two roundings below 1e-2) and the first grey
// column is bs / 3 <= sx0.  The window copies MF_C1_PITCH bytes of each row from column gx = min(bs / 3 & ~3, W - MF_C1_PITCH): every tap
// the plan certifies (columns sx0 .. sx0 + 53 at most: MF_STAGE_COLS + 2, or clamped to W - 1) lies in it, and the copy never leaves the
// frame (the plan stages only frames with W % 4 == 0, and the grey window only frames of at least MF_C1_PITCH columns).
constexpr int MF_C1_PITCH = 80;             // 5 chunks of 16 bytes: rows 0..7 of a footprint start 20 banks apart (0, 20, 8, 28, ...)
struct GreyWindow { bool on; uint32_t row0, col0; };

// Footprint-level tail of the GREY instantiation of footprint_body: the lane's four pixels at source coordinates (u, v) -- taps, blend,
// crop flags, store.  Deep-interior footprints take their taps from the grey window in LDS when the plan staged one (`win.on`), else four
// byte loads per pixel from the frame; the others take every tap at its position clamped into the frame and replace outside taps by
// `border` (byte loads only: nothing outside the frame is ever read).  All frame offsets are 64-bit.
__device__ __forceinline__ void remap_store_u8c1(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W, int H,
                                                 const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, uint32_t border,
                                                 int32_t* __restrict__ crop, int32_t* __restrict__ clip, const GreyWindow& win,
                                                 const uint8_t* s_win)
{
    const uint64_t frame_px = (uint64_t)((uint32_t)W * (uint32_t)H);
    const uint8_t* __restrict__ src = frames + (uint64_t)f * frame_px;
    uint8_t* __restrict__ dst = out + (uint64_t)f * frame_px;
    uint32_t bx[4], by[4];
    fixed_point(u, v, bx, by);
    const bool deep = deep_interior(bx, by, W, H);
    const bool fast = __ballot(active && !deep) == 0;
    uint32_t o[4];                                                      // the lane's 4 output bytes
    int c_left = 0, c_top = 0, c_right = W - 1, c_bottom = H - 1;
    if (win.on) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the grey window has landed in LDS
    if (active) {
        if (fast && win.on) {
            const lds_bytes_t w = lds_ptr(s_win);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ix = __builtin_amdgcn_ubfe(bx[j], 5, 17), iy = __builtin_amdgcn_ubfe(by[j], 5, 17);
                const uint32_t a = umad24(iy - win.row0, (uint32_t)MF_C1_PITCH, ix - win.col0);
                o[j] = blend_c1(w[a], w[a + 1], w[a + MF_C1_PITCH], w[a + MF_C1_PITCH + 1], bx[j], by[j]);
            }
        } else if (fast) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ix = __builtin_amdgcn_ubfe(bx[j], 5, 17), iy = __builtin_amdgcn_ubfe(by[j], 5, 17);
                const uint8_t* __restrict__ p = src + (uint64_t)(iy * (uint32_t)W + ix);
                o[j] = blend_c1(p[0], p[1], p[W], p[W + 1], bx[j], by[j]);
            }
        } else {
            // frame borders, uncovered pixels (at (W+1, H+1)), crop flags, out-of-range coordinates
            const float fWm1 = (float)(W - 1), fHm1 = (float)(H - 1);
            const bool narrow = narrow_coords(bx, by);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float uu = u[j], vv = v[j];
                const int x = x0 + j;
                if (x < W) {                                            // crop-boundary scan, mfs.py:1075-1098 (exact: Sterbenz)
                    if (fabsf(uu) < 1.0f) c_left = max(c_left, x);
                    if (fabsf(uu - fWm1) < 1.0f) c_right = min(c_right, x);
                    if (fabsf(vv) < 1.0f) c_top = max(c_top, y);
                    if (fabsf(vv - fHm1) < 1.0f) c_bottom = min(c_bottom, y);
                }
                const int sxx = fixed_coord(narrow, bx[j], uu), syy = fixed_coord(narrow, by[j], vv);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                // (a 2 x 2 footprint wholly outside needs no special case: four border taps with weights summing to 1024 give the border)
                const ClampedTaps t = clamped_taps(ix, iy, W, H);
                const uint32_t s00 = src[t.r0 + t.cx0], s01 = src[t.r0 + t.cx1], s10 = src[t.r1 + t.cx0], s11 = src[t.r1 + t.cx1];
                o[j] = blend_c1(t.in_x0 && t.in_y0 ? s00 : border, t.in_x1 && t.in_y0 ? s01 : border, t.in_x0 && t.in_y1 ? s10 : border,
                                t.in_x1 && t.in_y1 ? s11 : border, (uint32_t)sxx, (uint32_t)syy);
            }
        }
    }
    if (!fast) crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
    if (active) {
        uint8_t* __restrict__ d = dst + (uint32_t)y * (uint32_t)W + (uint32_t)x0;
        if (x0 + 3 < W) {                                               // 4 bytes, dword-aligned when W % 4 == 0 (else an unaligned store)
            const uint32_t w4 = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
            __builtin_memcpy(d, &w4, 4);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < W) d[j] = (uint8_t)o[j];
        }
    }
}

// ---- 4-channel uint8 frames: cv2.remap of CV_8UC4 -- the 8-bit fixed-point path of CV_8UC3 on four channels: channels 0-2 come out as the
// u8c3 warp's, channel 3 as the u8c1 warp's on the alpha plane ------------------------------------------------------------------------------
// The 4-byte window: the plan's STAGED window (cut for 3-byte pixels) re-cut for 4-byte pixels, with the grey window's words (GreyWindow: first
// row, first column).  sy0 and bs as for the grey window; the first column is gx = min(bs / 3, W - MF_C4_COLS) >= sx0 - 1 (bs >= 3 sx0 - 3), and
// MF_C4_COLS columns from there hold every tap the plan certifies (columns sx0 .. sx0 + 53 at most, or clamped to W - 1) while the copy never
// leaves the frame (the window is taken only for frames of at least MF_C4_COLS columns).  A row is MF_C4_PITCH = 14 chunks of 16 bytes; 12 rows
// (9 for COMPACT regions) are at most 168 chunks: three global->LDS loads per lane, 2,688 bytes of LDS.  A pixel's two horizontal taps are 8
// contiguous dword-aligned bytes there.
constexpr int MF_C4_COLS = 56;
constexpr int MF_C4_PITCH = 4 * MF_C4_COLS;

// The blend of one 4-byte pixel from its taps p00 / p01 (row iy, columns ix and ix + 1) and p10 / p11 (row iy + 1) at fixed-point coordinates
// (sx, sy): per channel the two horizontal neighbours in the 16-bit halves of one register (one v_perm_b32 per tap row), both lerped vertically
// at once, then v_dot2_u32_u16 horizontally with the weights scaled so that the rounded byte lands in byte 2 -- blend_pixel's arithmetic,
// (sum w_k s_k + 2^14) >> 15 per channel.  Returns B | G << 8 | R << 16 | A << 24.
__device__ __forceinline__ uint32_t blend_c4(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t sx, uint32_t sy)
{
    const uint32_t fy = sy & 31u, wy = 32u - fy;
    const uint32_t wq = umad24(sx & 31u, 0x3FFFC0u, 2048u);               // 64 (32 - fx) | 64 fx << 16
    uint32_t o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t sel = 0x0C040C00u + 0x00010001u * (uint32_t)c;     // byte c of the first tap, byte c of the second in bits 16-23
        const uint32_t vc = umad24(__builtin_amdgcn_perm(p11, p10, sel), fy, __umul24(__builtin_amdgcn_perm(p01, p00, sel), wy));
        o[c] = udot2(vc, wq, 32768u);
    }
    return __builtin_amdgcn_perm(o[1], o[0], 0x0C0C0602u) | __builtin_amdgcn_perm(o[3], o[2], 0x06020C0Cu);
}

// Footprint-level tail of the U8C4 instantiation of footprint_body: the lane's four pixels at source coordinates (u, v) -- taps, blend, crop
// flags, one 16-byte store.  Deep-interior footprints take their taps from the 4-byte window in LDS when the plan staged one (`win.on`: two
// dword-pair reads per pixel), else two 8-byte loads per pixel from the frame; the others take every tap at its position clamped into the frame
// and replace outside taps by `border` (the whole B G R A word).  All frame offsets are 64-bit.
__device__ __forceinline__ void remap_store_u8c4(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W, int H,
                                                 const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, uint32_t border,
                                                 int32_t* __restrict__ crop, int32_t* __restrict__ clip, const GreyWindow& win,
                                                 const uint8_t* s_win)
{
    const uint64_t frame_bytes = 4ull * (uint64_t)((uint32_t)W * (uint32_t)H);
    const uint8_t* __restrict__ src = frames + (uint64_t)f * frame_bytes;
    uint8_t* __restrict__ dst = out + (uint64_t)f * frame_bytes;
    uint32_t bx[4], by[4];
    fixed_point(u, v, bx, by);
    const bool deep = deep_interior(bx, by, W, H);
    const bool fast = __ballot(active && !deep) == 0;
    uint32_t o[4];                                                      // the lane's 4 output pixels
    int c_left = 0, c_top = 0, c_right = W - 1, c_bottom = H - 1;
    if (win.on) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the 4-byte window has landed in LDS
    if (active) {
        if (fast && win.on) {
            typedef const __attribute__((address_space(3))) uint32_t* lds_words_t;
            const lds_words_t w = (lds_words_t)lds_ptr(s_win);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ix = __builtin_amdgcn_ubfe(bx[j], 5, 17), iy = __builtin_amdgcn_ubfe(by[j], 5, 17);
                const uint32_t a = umad24(iy - win.row0, (uint32_t)(MF_C4_PITCH / 4), ix - win.col0);       // in dwords
                o[j] = blend_c4(w[a], w[a + 1], w[a + MF_C4_PITCH / 4], w[a + MF_C4_PITCH / 4 + 1], bx[j], by[j]);
            }
        } else if (fast) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ix = __builtin_amdgcn_ubfe(bx[j], 5, 17), iy = __builtin_amdgcn_ubfe(by[j], 5, 17);
                const uint8_t* __restrict__ p = src + 4ull * (uint64_t)(iy * (uint32_t)W + ix);
                uint2 a, b;                                             // pixels ix and ix + 1 of rows iy and iy + 1
                __builtin_memcpy(&a, p, 8);
                __builtin_memcpy(&b, p + 4ull * (uint32_t)W, 8);
                o[j] = blend_c4(a.x, a.y, b.x, b.y, bx[j], by[j]);
            }
        } else {
            // frame borders, uncovered pixels (at (W+1, H+1)), crop flags, out-of-range coordinates
            const float fWm1 = (float)(W - 1), fHm1 = (float)(H - 1);
            const bool narrow = narrow_coords(bx, by);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float uu = u[j], vv = v[j];
                const int x = x0 + j;
                if (x < W) {                                            // crop-boundary scan, mfs.py:1075-1098 (exact: Sterbenz)
                    if (fabsf(uu) < 1.0f) c_left = max(c_left, x);
                    if (fabsf(uu - fWm1) < 1.0f) c_right = min(c_right, x);
                    if (fabsf(vv) < 1.0f) c_top = max(c_top, y);
                    if (fabsf(vv - fHm1) < 1.0f) c_bottom = min(c_bottom, y);
                }
                const int sxx = fixed_coord(narrow, bx[j], uu), syy = fixed_coord(narrow, by[j], vv);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                // (a 2 x 2 footprint wholly outside needs no special case: four border taps with weights summing to 1024 give the border)
                const ClampedTaps t = clamped_taps(ix, iy, W, H);
                uint32_t p00, p01, p10, p11;
                __builtin_memcpy(&p00, src + 4ull * (t.r0 + t.cx0), 4);
                __builtin_memcpy(&p01, src + 4ull * (t.r0 + t.cx1), 4);
                __builtin_memcpy(&p10, src + 4ull * (t.r1 + t.cx0), 4);
                __builtin_memcpy(&p11, src + 4ull * (t.r1 + t.cx1), 4);
                o[j] = blend_c4(t.in_x0 && t.in_y0 ? p00 : border, t.in_x1 && t.in_y0 ? p01 : border, t.in_x0 && t.in_y1 ? p10 : border,
                                t.in_x1 && t.in_y1 ? p11 : border, (uint32_t)sxx, (uint32_t)syy);
            }
        }
    }
    if (!fast) crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
    if (active) {
        uint8_t* __restrict__ d = dst + 4u * ((uint32_t)y * (uint32_t)W + (uint32_t)x0);
        if (x0 + 3 < W) {                                               // 16 bytes: one store (16-byte aligned on an aligned stack)
            const uint4 q = make_uint4(o[0], o[1], o[2], o[3]);
            __builtin_memcpy(d, &q, 16);
            // (the compiler would otherwise merge the stores of the three call sites in footprint_body into one shared dwordx3 store behind
            // a dword store of each: it does not move code across an asm statement)
            asm volatile("" ::: "memory");
        } else {                                                        // (a loop: its stores do not merge with the 16-byte one)
            const int m = W - x0;
#pragma unroll 1
            for (int j = 0; j < m; ++j) __builtin_memcpy(d + 4 * j, &o[j], 4);
        }
    }
}

// ---- the coordinate maps themselves: frame_stabilized_x_y of mfs.py:1054-1061, the arrays cv2.remap gets at mfs.py:1063-1069 ------------
// Footprint-level tail of the MAPS instantiation of footprint_body: the lane's four pixels' source coordinates (u, v) go to
// maps[f][y][x0 + j] = {u, v} as they are -- float32 [H][W][2], x first; a pixel no cell owns holds (W+1, H+1) already (mfs.py:983-984).
// The lane's four pixels are 32 contiguous bytes: two 16-byte stores where that address is 16-byte aligned (always, for an even W and an
// aligned stack; every other row for an odd W), else 8 bytes per pixel, and per pixel too in the lane that overhangs the right edge
// (x < W).  `maps` is 8-byte aligned at least; all offsets are 64-bit (300 frames of 1080p are 4.98 GB).
__device__ __forceinline__ void maps_store_f32(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W, int H,
                                               float* __restrict__ maps)
{
    if (!active) return;                                                // (y < H and x0 < W)
    float* __restrict__ d = maps + 2ull * ((uint64_t)f * (uint64_t)((uint32_t)W * (uint32_t)H) + (uint64_t)((uint32_t)y * (uint32_t)W + (uint32_t)x0));
    if (x0 + 3 < W && ((uintptr_t)d & 15u) == 0) {
        *reinterpret_cast<float4*>(d) = make_float4(u[0], v[0], u[1], v[1]);
        *reinterpret_cast<float4*>(d + 4) = make_float4(u[2], v[2], u[3], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < W) *reinterpret_cast<float2*>(d + 2 * j) = make_float2(u[j], v[j]);
    }
}

// ---- side planes [n][H][W]: what travels with a video without being a picture (depth, flow, labels, masks) ---------------------------
// Footprint-level tail of the PLANE_F32 instantiation of footprint_body: cv2.remap INTER_LINEAR / BORDER_CONSTANT of CV_32FC1
// (remapBilinear<Cast<float, float>, RemapNoVec, float>) -- remap_store_u16 on one float32 channel without saturate_cast: the 8-bit map
// quantisation, BilinearTab_f's exact weights, t = ((S00 w0 + S01 w1) + S10 w2) + S11 w3 with every product and sum rounded on its own,
// out = t.  Deep-interior footprints take each pixel's two tap rows as one 8-byte load apiece (4-byte aligned); the others take every tap at
// its position clamped into the plane and replace outside taps by `fill`, and a 2 x 2 footprint wholly outside gives `fill` itself.  Nothing
// outside the plane's bytes is read.  The lane's four results are 16 contiguous bytes: one 16-byte store where that address is 16-byte
// aligned, else 4 bytes per pixel, and per pixel too in the lane that overhangs the right edge (maps_store_f32's rule).  All offsets are
// 64-bit.
__device__ __forceinline__ void remap_store_plane_f32(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W, int H,
                                                      const float* __restrict__ planes, float* __restrict__ out, float fill,
                                                      int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint64_t plane_elems = (uint64_t)((uint32_t)W * (uint32_t)H);
    const float* __restrict__ src = planes + (uint64_t)f * plane_elems;
    uint32_t bx[4], by[4];
    fixed_point(u, v, bx, by);
    const bool deep = deep_interior(bx, by, W, H);
    const bool fast = __ballot(active && !deep) == 0;
    float o[4] = { fill, fill, fill, fill };
    int c_left = 0, c_top = 0, c_right = W - 1, c_bottom = H - 1;
    if (active) {
        if (fast) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ix = __builtin_amdgcn_ubfe(bx[j], 5, 17), iy = __builtin_amdgcn_ubfe(by[j], 5, 17);
                const float* __restrict__ p0 = src + (uint64_t)(iy * (uint32_t)W + ix);
                float a[2], b[2];                                       // S00 S01 of row iy, S10 S11 of row iy + 1
                __builtin_memcpy(a, p0, 8);
                __builtin_memcpy(b, p0 + (uint32_t)W, 8);
                const float ax = (float)(bx[j] & 31u) * 0.03125f, ay = (float)(by[j] & 31u) * 0.03125f;
                const float ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                o[j] = ((a[0] * (ay0 * ax0) + a[1] * (ay0 * ax)) + b[0] * (ay * ax0)) + b[1] * (ay * ax);
            }
        } else {
            // plane borders, uncovered pixels (at (W+1, H+1)), crop flags, out-of-range coordinates
            const float fWm1 = (float)(W - 1), fHm1 = (float)(H - 1);
            const bool narrow = narrow_coords(bx, by);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float uu = u[j], vv = v[j];
                const int x = x0 + j;
                if (x < W) {                                            // crop-boundary scan, mfs.py:1075-1098 (exact: Sterbenz)
                    if (fabsf(uu) < 1.0f) c_left = max(c_left, x);
                    if (fabsf(uu - fWm1) < 1.0f) c_right = min(c_right, x);
                    if (fabsf(vv) < 1.0f) c_top = max(c_top, y);
                    if (fabsf(vv - fHm1) < 1.0f) c_bottom = min(c_bottom, y);
                }
                const int sxx = fixed_coord(narrow, bx[j], uu), syy = fixed_coord(narrow, by[j], vv);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                if (ix >= W || ix + 1 < 0 || iy >= H || iy + 1 < 0) continue;       // the 2 x 2 footprint lies wholly outside: fill
                const ClampedTaps t = clamped_taps(ix, iy, W, H);
                const float q00 = src[(uint64_t)(t.r0 + t.cx0)], q01 = src[(uint64_t)(t.r0 + t.cx1)];
                const float q10 = src[(uint64_t)(t.r1 + t.cx0)], q11 = src[(uint64_t)(t.r1 + t.cx1)];
                const float s00 = t.in_x0 && t.in_y0 ? q00 : fill, s01 = t.in_x1 && t.in_y0 ? q01 : fill;
                const float s10 = t.in_x0 && t.in_y1 ? q10 : fill, s11 = t.in_x1 && t.in_y1 ? q11 : fill;
                const float ax = (float)(sxx & 31) * 0.03125f, ay = (float)(syy & 31) * 0.03125f;
                const float ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                o[j] = ((s00 * (ay0 * ax0) + s01 * (ay0 * ax)) + s10 * (ay * ax0)) + s11 * (ay * ax);
            }
        }
    }
    if (!fast) crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
    if (active) {
        float* __restrict__ d = out + (uint64_t)f * plane_elems + (uint64_t)((uint32_t)y * (uint32_t)W + (uint32_t)x0);
        if (x0 + 3 < W && ((uintptr_t)d & 15u) == 0) {
            *reinterpret_cast<float4*>(d) = make_float4(o[0], o[1], o[2], o[3]);
            // (as in remap_store_u8c4: the compiler would otherwise split this store into a dword every path shares and a dwordx3; it does
            // not move code across an asm statement)
            asm volatile("" ::: "memory");
        } else {                                                        // (a loop: its stores do not merge with the 16-byte one)
            const int m = min(4, W - x0);
#pragma unroll 1
            for (int j = 0; j < m; ++j) d[j] = j == 0 ? o[0] : j == 1 ? o[1] : j == 2 ? o[2] : o[3];      // (selects: o stays in registers)
        }
    }
}

// Footprint-level tail of the PLANE_N* instantiations: cv2.remap INTER_NEAREST / BORDER_CONSTANT on elements of ES = 1, 2, 4 or 8 bytes
// (remapNearest): ix = sat_short(cvRound(u)), iy = sat_short(cvRound(v)) -- float32 coordinates rounded half to even; the saturation cannot
// change the inside test, W and H are below 32,768 --, the element copied as bits where 0 <= ix < W and 0 <= iy < H, `fill` (the element's
// bit pattern) otherwise.  Every load goes to the position clamped into the plane.  SCAN: the four crop tests on every pixel (the general
// path; a hot or pair footprint is certified DEEP, no pixel of it can pass one).  The lane's four elements are 4 ES contiguous bytes: stores of
// min(4 ES, 16) bytes where the address is aligned to that, else per element, and per element in the lane that overhangs the right edge.
template <int ES> struct PlaneElem;
template <> struct PlaneElem<1> { typedef uint8_t type; };
template <> struct PlaneElem<2> { typedef uint16_t type; };
template <> struct PlaneElem<4> { typedef uint32_t type; };
template <> struct PlaneElem<8> { typedef uint64_t type; };
template <int ES, bool SCAN>
__device__ __forceinline__ void remap_store_plane_nearest(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W,
                                                          int H, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, uint64_t fill,
                                                          int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    typedef typename PlaneElem<ES>::type T;
    const uint64_t plane_elems = (uint64_t)((uint32_t)W * (uint32_t)H);
    const T* __restrict__ src = reinterpret_cast<const T*>(planes) + (uint64_t)f * plane_elems;
    const float fWm1 = (float)(W - 1), fHm1 = (float)(H - 1);
    T o[4];
    int c_left = 0, c_top = 0, c_right = W - 1, c_bottom = H - 1;
    if (active) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float uu = u[j], vv = v[j];
            const int x = x0 + j;
            if (SCAN && x < W) {                                        // crop-boundary scan, mfs.py:1075-1098 (exact: Sterbenz)
                if (fabsf(uu) < 1.0f) c_left = max(c_left, x);
                if (fabsf(uu - fWm1) < 1.0f) c_right = min(c_right, x);
                if (fabsf(vv) < 1.0f) c_top = max(c_top, y);
                if (fabsf(vv - fHm1) < 1.0f) c_bottom = min(c_bottom, y);
            }
            const int ix = cv_round_f32(uu), iy = cv_round_f32(vv);
            const bool inside = (unsigned)ix < (unsigned)W && (unsigned)iy < (unsigned)H;
            const uint32_t cx = (uint32_t)min(max(ix, 0), W - 1), cy = (uint32_t)min(max(iy, 0), H - 1);
            const T s = src[(uint64_t)(cy * (uint32_t)W + cx)];
            o[j] = inside ? s : (T)fill;
        }
    }
    if (SCAN) crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
    if (active) {
        T* __restrict__ d = reinterpret_cast<T*>(out) + (uint64_t)f * plane_elems + (uint64_t)((uint32_t)y * (uint32_t)W + (uint32_t)x0);
        constexpr uint32_t VB = 4 * ES < 16 ? 4 * ES : 16;              // the widest store the lane's 4 ES bytes fill
        if (x0 + 3 < W && ((uintptr_t)d & (VB - 1u)) == 0) {
            __builtin_memcpy(__builtin_assume_aligned(d, VB), o, 4 * ES);
            asm volatile("" ::: "memory");                              // (keeps the wide store whole, as in remap_store_plane_f32)
        } else {                                                        // (a loop: its stores do not merge with the wide one)
            const int m = min(4, W - x0);
#pragma unroll 1
            for (int j = 0; j < m; ++j) d[j] = j == 0 ? o[0] : j == 1 ? o[1] : j == 2 ? o[2] : o[3];      // (selects: o stays in registers)
        }
    }
}

// The planes' tail by format (`fill`: the element's bit pattern in the low bytes; float32 bits for PLANE_F32)
template <Px PX, bool SCAN>
__device__ __forceinline__ void remap_store_plane(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W, int H,
                                                  const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, uint64_t fill,
                                                  int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    if constexpr (PX == Px::PLANE_F32)
        remap_store_plane_f32(u, v, f, x0, y, active, W, H, reinterpret_cast<const float*>(planes), reinterpret_cast<float*>(out),
                              __uint_as_float((uint32_t)fill), crop, clip);
    else
        remap_store_plane_nearest<px_sample_bytes(PX), SCAN>(u, v, f, x0, y, active, W, H, planes, out, fill, crop, clip);
}

// ---- the luma plane of a P010 / P012 / P016 clip: cv2.remap's CV_16U arithmetic (blend16 at the head of this file) on one channel -----------
// Footprint-level tail of the U16C1 instantiation of footprint_body: remap_store_u16 on one channel -- out is, bit for bit, channel 0 of
// remap_store_u16 on the plane repeated three times.  Deep-interior footprints (every tap two pixels inside the frame, no crop flag possible)
// take each pixel's two tap rows as one 4-byte load apiece (the frame may be only 2-byte aligned: unaligned dword loads) and blend pixels
// 0 + 1 and 2 + 3 pairwise; the others take every tap at its position clamped into the frame and replace outside taps by `border`, and a
// 2 x 2 footprint wholly outside the frame gives `border` itself.  The four crop tests and crop_fold as in remap_store_u16.  The lane's four
// samples go out as one 8-byte store where all four lie inside the row.  All offsets are 64-bit.
__device__ __forceinline__ void remap_store_u16c1(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W, int H,
                                                  const uint16_t* __restrict__ frames, uint16_t* __restrict__ out, uint32_t border,
                                                  int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint64_t frame_samples = (uint64_t)((uint32_t)W * (uint32_t)H);
    const uint16_t* __restrict__ src = frames + (uint64_t)f * frame_samples;
    uint16_t* __restrict__ dst = out + (uint64_t)f * frame_samples;
    uint32_t bx[4], by[4];
    fixed_point(u, v, bx, by);
    const bool deep = deep_interior(bx, by, W, H);
    const bool fast = __ballot(active && !deep) == 0;
    uint32_t o[4];                                                      // the lane's 4 output samples
    int c_left = 0, c_top = 0, c_right = W - 1, c_bottom = H - 1;
    if (active) {
        if (fast) {
            float sv[4][4];                                             // taps as float, [pixel][S00, S01, S10, S11]
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ix = __builtin_amdgcn_ubfe(bx[j], 5, 17), iy = __builtin_amdgcn_ubfe(by[j], 5, 17);
                const uint16_t* __restrict__ p0 = src + (uint64_t)(iy * (uint32_t)W + ix);
                uint32_t a, b;                                          // S00 | S01 << 16 of row iy, S10 | S11 << 16 of row iy + 1
                __builtin_memcpy(&a, p0, 4);
                __builtin_memcpy(&b, p0 + (uint32_t)W, 4);
                sv[j][0] = (float)(a & 0xFFFFu); sv[j][1] = (float)(a >> 16);
                sv[j][2] = (float)(b & 0xFFFFu); sv[j][3] = (float)(b >> 16);
            }
#pragma unroll
            for (int j = 0; j < 4; j += 2) {
                const f32x2 ax = f32x2{ (float)(bx[j] & 31u), (float)(bx[j + 1] & 31u) } * 0.03125f;
                const f32x2 ay = f32x2{ (float)(by[j] & 31u), (float)(by[j + 1] & 31u) } * 0.03125f;
                const f32x2 ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                const f32x2 t = blend16x2(f32x2{ sv[j][0], sv[j + 1][0] }, f32x2{ sv[j][1], sv[j + 1][1] }, f32x2{ sv[j][2], sv[j + 1][2] },
                                          f32x2{ sv[j][3], sv[j + 1][3] }, ay0 * ax0, ay0 * ax, ay * ax0, ay * ax);
                o[j] = (uint32_t)rintf(t.x);                            // (no clamp: rint(t) <= 65535 here, see remap_store_u16)
                o[j + 1] = (uint32_t)rintf(t.y);
            }
        } else {
            // frame borders, uncovered pixels (at (W+1, H+1)), crop flags, out-of-range coordinates
            const float fWm1 = (float)(W - 1), fHm1 = (float)(H - 1);
            const bool narrow = narrow_coords(bx, by);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float uu = u[j], vv = v[j];
                const int x = x0 + j;
                if (x < W) {                                            // crop-boundary scan, mfs.py:1075-1098 (exact: Sterbenz)
                    if (fabsf(uu) < 1.0f) c_left = max(c_left, x);
                    if (fabsf(uu - fWm1) < 1.0f) c_right = min(c_right, x);
                    if (fabsf(vv) < 1.0f) c_top = max(c_top, y);
                    if (fabsf(vv - fHm1) < 1.0f) c_bottom = min(c_bottom, y);
                }
                const int sxx = fixed_coord(narrow, bx[j], uu), syy = fixed_coord(narrow, by[j], vv);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                o[j] = border;
                if (ix >= W || ix + 1 < 0 || iy >= H || iy + 1 < 0) continue;       // the 2 x 2 footprint lies wholly outside: the border sample
                const ClampedTaps t = clamped_taps(ix, iy, W, H);
                const uint32_t q00 = src[(uint64_t)(t.r0 + t.cx0)], q01 = src[(uint64_t)(t.r0 + t.cx1)];
                const uint32_t q10 = src[(uint64_t)(t.r1 + t.cx0)], q11 = src[(uint64_t)(t.r1 + t.cx1)];
                const uint32_t s00 = t.in_x0 && t.in_y0 ? q00 : border, s01 = t.in_x1 && t.in_y0 ? q01 : border;
                const uint32_t s10 = t.in_x0 && t.in_y1 ? q10 : border, s11 = t.in_x1 && t.in_y1 ? q11 : border;
                const float ax = (float)(sxx & 31) * 0.03125f, ay = (float)(syy & 31) * 0.03125f;
                const float ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                o[j] = blend16((float)s00, (float)s01, (float)s10, (float)s11, ay0 * ax0, ay0 * ax, ay * ax0, ay * ax);
            }
        }
    }
    if (!fast) crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
    if (active) {
        uint16_t* __restrict__ d = dst + (uint64_t)((uint32_t)y * (uint32_t)W + (uint32_t)x0);
        if (x0 + 3 < W) {                                               // 8 bytes at a 2-byte aligned address: one unaligned store
            const uint2 q = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
            __builtin_memcpy(d, &q, 8);
            asm volatile("" ::: "memory");                              // (keeps the store whole across footprint_body's three call sites, as in remap_store_u8c4)
        } else {                                                        // (a loop: its stores do not merge with the 8-byte one)
            const int m = W - x0;
#pragma unroll 1
            for (int j = 0; j < m; ++j) d[j] = (uint16_t)(j == 0 ? o[0] : j == 1 ? o[1] : j == 2 ? o[2] : o[3]);   // (selects: o stays in registers)
        }
    }
}

// ---- the interleaved chroma plane of a semi-planar YUV clip (NV12, NV16, P010): cv2.remap of a two-channel plane at the luma coordinates ----
// The blend of one two-byte pixel from its tap rows `a` (row iy: U0 V0 U1 V1, the pixels ix and ix + 1) and `b` (row iy + 1) at fixed-point
// coordinates (sx, sy): blend_c4's arithmetic on two channels -- the two horizontal neighbours of a channel are bytes c and c + 2 of a tap
// row, lerped vertically at once in 16-bit fields, then v_dot2_u32_u16 horizontally: (sum w_k s_k + 2^14) >> 15 per channel.  Returns U | V << 8.
__device__ __forceinline__ uint32_t blend_uv(uint32_t a, uint32_t b, uint32_t sx, uint32_t sy)
{
    const uint32_t fy = sy & 31u, wy = 32u - fy;
    const uint32_t wq = umad24(sx & 31u, 0x3FFFC0u, 2048u);               // 64 (32 - fx) | 64 fx << 16
    const uint32_t vu = umad24(b & 0x00FF00FFu, fy, __umul24(a & 0x00FF00FFu, wy));
    const uint32_t vv = umad24((b >> 8) & 0x00FF00FFu, fy, __umul24((a >> 8) & 0x00FF00FFu, wy));
    return __builtin_amdgcn_perm(udot2(vv, wq, 32768u), udot2(vu, wq, 32768u), 0x0C0C0602u);
}

// Footprint-level tail of the NV12_UV, NV16_UV, P010_UV and P210_UV instantiations of footprint_body.  The lane owns four consecutive LUMA pixels of
// row y at coordinates (u, v) -- the maps kernel's, bit for bit -- and chroma is sited at the even luma sample: a lane that emits writes the
// chroma samples x0 / 2 and x0 / 2 + 1 of its chroma row from its pixels 0 and 2.  A sample's source position is its luma pixel's, halved in
// float32 (exact) along every axis the plane subsamples, then cv2.remap's 8-bit fixed point on the (Hc, Wc) plane of pixels of two samples T,
// U first: a pixel no cell owns, at (W + 1, H + 1), lands outside that plane and comes out as the border like any other.  Deep-interior
// footprints (wave-uniform: the test, the clamped taps and the ballot are all on (Wc, Hc)) take each sample's two tap rows as one load of two
// pixels apiece (the plane is only 2-byte aligned: unaligned loads); the others take every tap as a one-pixel load at its position clamped
// into the plane and replace outside taps by `border`.  Nothing outside the plane's bytes is read, no crop value is touched (the luma launch
// owns them), and the lane's two samples go out as one store of two pixels (of one in the lane that holds the last sample of a row with
// W % 4 == 2; an unaligned store where W % 4 == 2 or the plane is only 2-byte aligned).  All plane offsets are 64-bit, in units of T.
// NV12_UV (4:2:0, T = uint8): Wc = W / 2, Hc = H / 2; the lanes of even rows emit, into chroma row y / 2, the lanes of odd rows nothing; the
// position is (u / 2, v / 2), an unowned pixel's ((W + 1) / 2, (H + 1) / 2).  Pixels are 2 bytes, `border` is U | V << 8, the blend is
// blend_uv's integer one: a 2 x 2 footprint wholly outside needs no special case.
// NV16_UV (4:2:2, T = uint8): NV12_UV with chroma rows that are the luma rows -- Wc = W / 2, Hc = H, H of either parity (the plane has W H
// bytes per frame); EVERY row's lanes emit, into chroma row y; the position is (u / 2, v), v staying what it is, an unowned pixel's
// ((W + 1) / 2, H + 1).
// P010_UV (4:2:0, T = uint16): NV12_UV's lane mapping and coordinates with the CV_16U arithmetic.  Pixels are 4 bytes, a tap is one word
// U | V << 16 and so is `border`; the pair goes through blend16x2 with the sample's four weights computed once, so U and V never mix.  Float
// products of the border need not sum back to it, so a 2 x 2 footprint wholly outside the plane -- an unowned pixel's among them -- gives
// `border` itself.  The deep-interior blend needs no clamp (rint(t) <= 65535 there, see remap_store_u16); the other saturates like blend16.
// P210_UV (4:2:2, T = uint16): the product of the two rows above and no text of its own -- NV16_UV's geometry (Wc = W / 2, Hc = H of either
// parity, every row's lanes emit into chroma row y, the position is (u / 2, v), an unowned pixel's ((W + 1) / 2, H + 1)) with P010_UV's
// pixels, taps, border word, blend16x2 arithmetic and whole-footprint-outside rule.  The body takes no branch that one of those two does not.
template <Px PX>
__device__ __forceinline__ void remap_store_chroma(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W, int H,
                                                   const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, uint32_t border)
{
    static_assert(px_is_chroma(PX), "the semi-planar chroma planes");
    constexpr bool HALF_ROWS = PX == Px::NV12_UV || PX == Px::P010_UV, U16 = PX == Px::P010_UV || PX == Px::P210_UV;
    typedef typename PlaneElem<U16 ? 2 : 1>::type T;
    const int Wc = W >> 1, Hc = HALF_ROWS ? H >> 1 : H;
    const uint64_t plane_samples = 2ull * (uint64_t)((uint32_t)Wc * (uint32_t)Hc);
    const T* __restrict__ src = reinterpret_cast<const T*>(planes) + (uint64_t)f * plane_samples;
    const bool emit = HALF_ROWS ? active && (y & 1) == 0 : active;      // (x0 is a multiple of 4: pixels 0 and 2 are even columns)
    const bool two = x0 + 2 < W;                                        // (the lane's second sample exists; its pixel 2 stands in for nothing else)
    // the lane's two samples twice over, so that the four-pixel helpers of warp_coords.h serve (the duplicates fold away)
    const float h0 = u[0] * 0.5f, g0 = HALF_ROWS ? v[0] * 0.5f : v[0], h1 = two ? u[2] * 0.5f : h0, g1 = two ? (HALF_ROWS ? v[2] * 0.5f : v[2]) : g0;
    const float uc[4] = { h0, h1, h0, h1 }, vc[4] = { g0, g1, g0, g1 };
    uint32_t bx[4], by[4];
    fixed_point(uc, vc, bx, by);
    const bool deep = deep_interior(bx, by, Wc, Hc);
    const bool fast = __ballot(emit && !deep) == 0;
    uint32_t o[2];                                                      // the lane's two output pixels, U | V << 8 (U | V << 16 for U16)
    if (emit) {
        if (fast) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t ix = __builtin_amdgcn_ubfe(bx[j], 5, 17), iy = __builtin_amdgcn_ubfe(by[j], 5, 17);
                const T* __restrict__ p = src + 2ull * (uint64_t)(iy * (uint32_t)Wc + ix);
                if constexpr (U16) {
                    uint2 a, b;                                         // pixels ix and ix + 1 of rows iy and iy + 1
                    __builtin_memcpy(&a, p, 8);
                    __builtin_memcpy(&b, p + 2u * (uint32_t)Wc, 8);
                    const float ax = (float)(bx[j] & 31u) * 0.03125f, ay = (float)(by[j] & 31u) * 0.03125f;
                    const float ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                    const float w0 = ay0 * ax0, w1 = ay0 * ax, w2 = ay * ax0, w3 = ay * ax;
                    const f32x2 t = blend16x2(f32x2{ (float)(a.x & 0xFFFFu), (float)(a.x >> 16) }, f32x2{ (float)(a.y & 0xFFFFu), (float)(a.y >> 16) },
                                              f32x2{ (float)(b.x & 0xFFFFu), (float)(b.x >> 16) }, f32x2{ (float)(b.y & 0xFFFFu), (float)(b.y >> 16) },
                                              f32x2{ w0, w0 }, f32x2{ w1, w1 }, f32x2{ w2, w2 }, f32x2{ w3, w3 });
                    o[j] = (uint32_t)rintf(t.x) | ((uint32_t)rintf(t.y) << 16);     // (no clamp: rint(t) <= 65535 here, see remap_store_u16)
                } else {
                    uint32_t a, b;                                      // pixels ix and ix + 1 of rows iy and iy + 1
                    __builtin_memcpy(&a, p, 4);
                    __builtin_memcpy(&b, p + 2u * (uint32_t)Wc, 4);
                    o[j] = blend_uv(a, b, bx[j], by[j]);
                }
            }
        } else {
            // plane borders, uncovered pixels, out-of-range coordinates
            const bool narrow = narrow_coords(bx, by);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int sxx = fixed_coord(narrow, bx[j], uc[j]), syy = fixed_coord(narrow, by[j], vc[j]);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                if constexpr (U16) {
                    o[j] = border;
                    if (ix >= Wc || ix + 1 < 0 || iy >= Hc || iy + 1 < 0) continue; // the 2 x 2 footprint lies wholly outside: the border pixel
                }
                const ClampedTaps t = clamped_taps(ix, iy, Wc, Hc);
                if constexpr (U16) {
                    uint32_t p00, p01, p10, p11;
                    __builtin_memcpy(&p00, src + 2ull * (uint64_t)(t.r0 + t.cx0), 4);
                    __builtin_memcpy(&p01, src + 2ull * (uint64_t)(t.r0 + t.cx1), 4);
                    __builtin_memcpy(&p10, src + 2ull * (uint64_t)(t.r1 + t.cx0), 4);
                    __builtin_memcpy(&p11, src + 2ull * (uint64_t)(t.r1 + t.cx1), 4);
                    p00 = t.in_x0 && t.in_y0 ? p00 : border; p01 = t.in_x1 && t.in_y0 ? p01 : border;
                    p10 = t.in_x0 && t.in_y1 ? p10 : border; p11 = t.in_x1 && t.in_y1 ? p11 : border;
                    const float ax = (float)(sxx & 31) * 0.03125f, ay = (float)(syy & 31) * 0.03125f;
                    const float ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                    const float w0 = ay0 * ax0, w1 = ay0 * ax, w2 = ay * ax0, w3 = ay * ax;
                    const f32x2 t2 = blend16x2(f32x2{ (float)(p00 & 0xFFFFu), (float)(p00 >> 16) }, f32x2{ (float)(p01 & 0xFFFFu), (float)(p01 >> 16) },
                                               f32x2{ (float)(p10 & 0xFFFFu), (float)(p10 >> 16) }, f32x2{ (float)(p11 & 0xFFFFu), (float)(p11 >> 16) },
                                               f32x2{ w0, w0 }, f32x2{ w1, w1 }, f32x2{ w2, w2 }, f32x2{ w3, w3 });
                    o[j] = min((uint32_t)rintf(t2.x), 65535u) | (min((uint32_t)rintf(t2.y), 65535u) << 16);  // saturate_cast<ushort>, as blend16
                } else {
                    // (a 2 x 2 footprint wholly outside needs no special case: four border taps with weights summing to 1024 give the border)
                    uint16_t p00, p01, p10, p11;
                    __builtin_memcpy(&p00, src + 2ull * (uint64_t)(t.r0 + t.cx0), 2);
                    __builtin_memcpy(&p01, src + 2ull * (uint64_t)(t.r0 + t.cx1), 2);
                    __builtin_memcpy(&p10, src + 2ull * (uint64_t)(t.r1 + t.cx0), 2);
                    __builtin_memcpy(&p11, src + 2ull * (uint64_t)(t.r1 + t.cx1), 2);
                    const uint32_t q00 = t.in_x0 && t.in_y0 ? (uint32_t)p00 : border, q01 = t.in_x1 && t.in_y0 ? (uint32_t)p01 : border;
                    const uint32_t q10 = t.in_x0 && t.in_y1 ? (uint32_t)p10 : border, q11 = t.in_x1 && t.in_y1 ? (uint32_t)p11 : border;
                    o[j] = blend_uv(q00 | (q01 << 16), q10 | (q11 << 16), (uint32_t)sxx, (uint32_t)syy);
                }
            }
        }
        T* __restrict__ d = reinterpret_cast<T*>(out) + (uint64_t)f * plane_samples +
                            2ull * (uint64_t)((uint32_t)(HALF_ROWS ? y >> 1 : y) * (uint32_t)Wc + (uint32_t)(x0 >> 1));
        if constexpr (U16) {
            if (two) {                                                  // 8 bytes at a 2-byte aligned address: one unaligned store
                const uint2 q = make_uint2(o[0], o[1]);
                __builtin_memcpy(d, &q, 8);
            } else {
                __builtin_memcpy(d, &o[0], 4);
            }
        } else {
            if (two) {                                                  // 4 bytes, dword-aligned unless W % 4 == 2 or the plane is not (then an unaligned store)
                const uint32_t w4 = o[0] | (o[1] << 16);
                __builtin_memcpy(d, &w4, 4);
            } else {
                const uint16_t w2 = (uint16_t)o[0];
                __builtin_memcpy(d, &w2, 2);
            }
        }
    }
}

}  // namespace mf
#endif  // MF_WARP_TAILS_H
