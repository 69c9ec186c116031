// Crop + resize of the side planes of a video [n][H][W] -- _crop_frames (mfs.py:1111-1157, cv2.resize at :1150-1155) applied to a plane that
// travels with the colour frames -- to an oW x oH output, from a rectangle the host knows (resize_planes.hip) or one in device memory
// (resize_planes_dev.hip, under MF_RESIZE_DEV and other kernel names: resize_rect.h).
//
// float32, INTER_LINEAR (resize.cpp: HResizeLinear<float, float, float> + VResizeLinear<float, float, float, Cast<float, float>>): resize16_body.h
// without saturate_cast -- the 8-bit index and fraction tables, float32 coefficients (1 - f, f),
//   horizontal  t   = S[sx] a0 + S[sx+1] a1                               (float32, unfused; the columns left of xmax)
//               t   = S[cw-1]                                             (HResizeLinear's one-tap tail S * 1.0f from xmax on: the columns whose
//                                                                          sx was clamped to the crop's last column -- no product with 0, so an
//                                                                          infinity there stays an infinity)
//   vertical    out = t0 b0 + t1 b1                                       (float32, unfused, always two taps)
// where the crop is exactly twice the output in both axes, INTER_AREA's fast path in its scalar order, (((S00 + S01) + S10) + S11) * 0.25f,
// and where the crop has the output's own size, cv::resize's `dsize == ssize` copy: the sample's bits (-0.0, NaN payloads), no arithmetic.
// Nothing looks at a sample's value; subnormals are kept (the build flushes nothing); a weight of 0 does not exclude a tap.
// Elements of 1, 2, 4 or 8 bytes, INTER_NEAREST (resizeNN): sx = min(floor(x * (1.0 / (oW / cw))), cw - 1) in float64, the same for y, and
// the element copied as bits.
// plane_resize_tables builds either pair of tables on the device in the workspace mf_crop_resize_workspace_bytes(oW, oH) sizes (8 bytes per
// output column and row); the kernels: one thread per output pixel, a workgroup per 256 pixels of an output row, taps straight from the plane.
#ifndef MF_RESIZE_PLANES_BODY_H
#define MF_RESIZE_PLANES_BODY_H
#include "mf_common.h"
#include "resize_rect.h"

namespace mf {

// which of cv::resize's three INTER_LINEAR routes a float32 crop of cw x ch takes to oW x oH
enum PlanePath : int { PLANE_PATH_LINEAR = 0, PLANE_PATH_AREA = 1, PLANE_PATH_COPY = 2 };
__host__ __device__ __forceinline__ int plane_f32_path(int cw, int ch, int oW, int oH)
{
    return cw == oW && ch == oH ? PLANE_PATH_COPY : 2 * oW == cw && 2 * oH == ch ? PLANE_PATH_AREA : PLANE_PATH_LINEAR;
}
// the host knows the rectangle and passes the route; a device rectangle decides it in the kernel (wavefront-uniform)
#ifdef MF_RESIZE_DEV
#define MF_PLANE_PATH_ARG
#define MF_PLANE_PATH_LOAD const int path = plane_f32_path(cw, ch, oW, oH);
#else
#define MF_PLANE_PATH_ARG int path,
#define MF_PLANE_PATH_LOAD
#endif

// nearest == 0: resize16_tables_kernel's tables (x: ofs = sx clamped into the crop, f = its fraction, 0 where clamped;  y: ofs = sy0 | sy1 << 16
// of the clipped rows, f = the fraction);  nearest != 0: ofs = the one source column / row, f = 0
__global__ __launch_bounds__(256) void plane_resize_tables(MF_TABLES_ARGS, int nearest, Resize16Tab* __restrict__ xtab,
                                                           Resize16Tab* __restrict__ ytab)
{
    MF_TABLES_LOAD(W, H)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (nearest) {
        if (i < W) { xtab[i].ofs = min((int)floor((double)i * scale_x), cw - 1); xtab[i].f = 0.0f; }
        if (i < H) { ytab[i].ofs = min((int)floor((double)i * scale_y), ch - 1); ytab[i].f = 0.0f; }
        return;
    }
    if (i < W) {
        float fx = (float)(((double)i + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= (float)sx;
        if (sx < 0) { fx = 0.0f; sx = 0; }
        if (sx >= cw - 1) { fx = 0.0f; sx = cw - 1; }
        xtab[i].ofs = sx;
        xtab[i].f = fx;
    }
    if (i < H) {
        float fy = (float)(((double)i + 0.5) * scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int sy0 = min(max(sy, 0), ch - 1), sy1 = min(max(sy + 1, 0), ch - 1);
        ytab[i].ofs = sy0 | (sy1 << 16);
        ytab[i].f = fy;
    }
}

// `path`: plane_f32_path.  PLANE_PATH_AREA: the tables give sx = 2 dx, sy0 = 2 dy, sy1 = 2 dy + 1, the four taps of the 2 x 2 block;
// PLANE_PATH_COPY: they give sx = dx, sy0 = dy, and s0[0] is the sample itself
__global__ __launch_bounds__(256) void plane_resize_f32(const float* __restrict__ planes, float* __restrict__ out, int W, int H,
                                                        MF_RECT_ARGS, int oW, int oH, MF_PLANE_PATH_ARG const Resize16Tab* __restrict__ xtab,
                                                        const Resize16Tab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    MF_PLANE_PATH_LOAD
    int f, y, tx;
    if (!order.decode(blockIdx.x, f, y, tx)) return;
    const int x = tx * 256 + (int)threadIdx.x;
    if (x >= oW) return;
    const float* __restrict__ src = planes + (uint64_t)f * (uint64_t)((uint32_t)W * (uint32_t)H);
    const Resize16Tab xt = xtab[x], yt = ytab[y];
    const float a1 = xt.f, a0 = 1.0f - xt.f, b1 = yt.f, b0 = 1.0f - yt.f;
    const uint32_t sx = (uint32_t)(left + xt.ofs);
    const float* __restrict__ p0 = src + (uint64_t)((uint32_t)(top + (yt.ofs & 0xFFFF)) * (uint32_t)W + sx);
    const float* __restrict__ p1 = src + (uint64_t)((uint32_t)(top + (yt.ofs >> 16)) * (uint32_t)W + sx);
    float s0[2], s1[2];                                          // columns sx and sx + 1 of rows sy0 and sy1
    const bool two = xt.ofs + 1 < cw;                            // false from xmax on: the crop's last column, nothing to its right is read
    if (two) {
        __builtin_memcpy(s0, p0, 8);
        __builtin_memcpy(s1, p1, 8);
    } else {
        s0[0] = s0[1] = p0[0];
        s1[0] = s1[1] = p1[0];
    }
    float o;
    if (path == PLANE_PATH_COPY) {
        o = s0[0];
    } else if (path == PLANE_PATH_AREA) {
        o = (((s0[0] + s0[1]) + s1[0]) + s1[1]) * 0.25f;
    } else {
        const float t0 = two ? s0[0] * a0 + s0[1] * a1 : s0[0], t1 = two ? s1[0] * a0 + s1[1] * a1 : s1[0];      // (selects, no product with 0)
        o = t0 * b0 + t1 * b1;
    }
    out[(uint64_t)f * (uint64_t)((uint32_t)oW * (uint32_t)oH) + (uint64_t)((uint32_t)y * (uint32_t)oW + (uint32_t)x)] = o;
}

template <typename T>
__global__ __launch_bounds__(256) void plane_resize_nearest(const T* __restrict__ planes, T* __restrict__ out, int W, int H, MF_RECT_ARGS,
                                                            int oW, int oH, const Resize16Tab* __restrict__ xtab,
                                                            const Resize16Tab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    int f, y, tx;
    if (!order.decode(blockIdx.x, f, y, tx)) return;
    const int x = tx * 256 + (int)threadIdx.x;
    if (x >= oW) return;
    const T* __restrict__ src = planes + (uint64_t)f * (uint64_t)((uint32_t)W * (uint32_t)H);
    const uint32_t sx = (uint32_t)(left + min(xtab[x].ofs, cw - 1)), sy = (uint32_t)(top + ytab[y].ofs);     // (the table's clamp, restated: stays in the crop)
    out[(uint64_t)f * (uint64_t)((uint32_t)oW * (uint32_t)oH) + (uint64_t)((uint32_t)y * (uint32_t)oW + (uint32_t)x)] = src[(uint64_t)(sy * (uint32_t)W + sx)];
}

}  // namespace mf

#endif  // MF_RESIZE_PLANES_BODY_H
