// The luma of a resident clip as a uint8 stack (n, H, W): what the device tracker takes, from BGR / BGRA uint8, BGR uint16 and 16-bit luma
// planes.  Bit for bit tests/luma_model.py; the arithmetic is luma_body.h's.  Integers only, no LDS, nothing kept between pixels.
//
// luma_kernel<SRC>: ONE kernel over the flat pixel stream of the contiguous stack -- rows and frames do not matter to it.  The stream is cut
// where the DESTINATION is 16-byte aligned:
//   head   the 0 .. 15 pixels in front of the first aligned destination byte (all of a clip shorter than that)
//   runs   16 pixels each, one lane per run: one dwordx4 store, and -- where the run's source is 16-byte aligned as well (then every
//          run's is: a run is 48, 64, 96 or 32 source bytes) -- 3, 4, 6 or 2 dwordx4 loads.  That is the WIDE path, the one torch's own
//          allocations take.  A source that is misaligned against the destination DECLINES it: the run reads its samples one by one (byte or
//          16-bit loads, always aligned) and still stores 16 bytes at once.  No load is ever wider than the alignment of its address.
//   tail   the 0 .. 15 pixels behind the last run
// Head and tail are at most 30 pixels; lanes 0 .. 31 of the first workgroup take one each, sample by sample.
// Indices are 64-bit (1,200 4K frames are 9.95e9 pixels).  A launch is capped at luma::MAX_BLOCKS workgroups = 2^28 pixels, one run per lane
// and no loop in the kernel; the host strides over the rest of a longer clip, launch by launch on the same stream (cfg2's 300 x 1080p: three
// launches).  A capped grid whose lanes loop over the runs measured 8-12 % slower (profiles/luma.md).
// Bounds: run g < runs reads source bytes [B (head + 16 g), B (head + 16 g + 16)) and writes destination bytes [head + 16 g, head + 16 g + 16)
// with head + 16 (g + 1) <= total; head and tail pixels are below total by their own tests.
#include "mf_common.h"
#include "luma_body.h"

namespace mf {

using luma::Traits;
using luma::Weights;

// sample k of a run held in dwords
template <int SRC, int DWORDS> __device__ __forceinline__ uint32_t held(const uint32_t (&w)[DWORDS], int k)
{
    if (Traits<SRC>::sample_bytes == 1) return (w[k >> 2] >> (8 * (k & 3))) & 255u;
    return (w[k >> 1] >> (16 * (k & 1))) & 65535u;
}

// sample k of the stack, from memory
template <int SRC> __device__ __forceinline__ uint32_t fetched(const uint8_t* __restrict__ src, uint64_t k)
{
    if (Traits<SRC>::sample_bytes == 1) return src[k];
    return reinterpret_cast<const uint16_t*>(src)[k];
}

template <int SRC> __device__ __forceinline__ uint32_t pixel(uint32_t s0, uint32_t s1, uint32_t s2, const Weights& w)
{
    if (SRC == luma::U16C1) return s0 >> 8;
    if (SRC == luma::U16C3) return luma::y16(s0, s1, s2, w);
    return luma::y8(s0, s1, s2, w);
}

template <int SRC> __device__ __forceinline__ uint32_t pixel_at(const uint8_t* __restrict__ src, uint64_t p, const Weights& w)
{
    constexpr int C = Traits<SRC>::channels;
    const uint32_t s0 = fetched<SRC>(src, p * C);
    if (C == 1) return pixel<SRC>(s0, 0, 0, w);
    return pixel<SRC>(s0, fetched<SRC>(src, p * C + 1), fetched<SRC>(src, p * C + 2), w);
}

template <int SRC>
__global__ void __launch_bounds__(luma::LANES) luma_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t total, uint32_t head,
                                                           uint64_t runs, uint64_t first, int wide, Weights w)
{
    constexpr int C = Traits<SRC>::channels, RUN = luma::RUN;
    constexpr int PIXEL_BYTES = C * Traits<SRC>::sample_bytes, DWORDS = RUN * PIXEL_BYTES / 4;
    const uint64_t g = first + (uint64_t)blockIdx.x * luma::LANES + threadIdx.x;
    if (g < runs) {
        const uint64_t p = head + g * RUN;
        uint32_t y[RUN];
        if (wide) {
            const uint4* __restrict__ from = reinterpret_cast<const uint4*>(src + p * PIXEL_BYTES);
            uint32_t held_run[DWORDS];
#pragma unroll
            for (int j = 0; j < DWORDS / 4; ++j) {
                const uint4 v = from[j];
                held_run[4 * j] = v.x; held_run[4 * j + 1] = v.y; held_run[4 * j + 2] = v.z; held_run[4 * j + 3] = v.w;
            }
#pragma unroll
            for (int i = 0; i < RUN; ++i)
                y[i] = C == 1 ? pixel<SRC>(held<SRC>(held_run, i), 0, 0, w)
                              : pixel<SRC>(held<SRC>(held_run, C * i), held<SRC>(held_run, C * i + 1), held<SRC>(held_run, C * i + 2), w);
        } else {
#pragma unroll
            for (int i = 0; i < RUN; ++i) y[i] = pixel_at<SRC>(src, p + i, w);
        }
        uint4 out;
        out.x = y[0] | y[1] << 8 | y[2] << 16 | y[3] << 24;
        out.y = y[4] | y[5] << 8 | y[6] << 16 | y[7] << 24;
        out.z = y[8] | y[9] << 8 | y[10] << 16 | y[11] << 24;
        out.w = y[12] | y[13] << 8 | y[14] << 16 | y[15] << 24;
        *reinterpret_cast<uint4*>(dst + p) = out;
    }
    if (first != 0 || blockIdx.x != 0 || threadIdx.x >= 2 * RUN) return;
    const uint32_t t = threadIdx.x;
    if (t < RUN) {
        if (t < head) dst[t] = (uint8_t)pixel_at<SRC>(src, t, w);
    } else {
        const uint64_t p = head + runs * RUN + (t - RUN);
        if (p < total) dst[p] = (uint8_t)pixel_at<SRC>(src, p, w);
    }
}

template <int SRC>
static int luma_entry(const char* name, const void* src, int n, int W, int H, int red_first, uint8_t* dst, void* stream)
{
    constexpr size_t PIXEL_BYTES = (size_t)Traits<SRC>::channels * Traits<SRC>::sample_bytes;
    if (!src || !dst) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: n must be at least 1 (got %d)", name, n); return MF_ERR_INVALID_ARG; }
    if (W < 1 || W > luma::MAX_DIM || H < 1 || H > luma::MAX_DIM) {
        set_error("%s: W and H must be in 1 .. %d (got %d x %d)", name, luma::MAX_DIM, W, H);
        return MF_ERR_INVALID_ARG;
    }
    if (red_first != 0 && red_first != 1) { set_error("%s: red_first must be 0 or 1 (got %d)", name, red_first); return MF_ERR_INVALID_ARG; }
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    if (Traits<SRC>::sample_bytes == 2 && (s & 1)) { set_error("%s: a uint16 source must start at an even address", name); return MF_ERR_INVALID_ARG; }
    const size_t total = (size_t)n * (size_t)W * (size_t)H;                 // below 2^61; its source below 2^64 bytes
    if (s < d + total && d < s + total * PIXEL_BYTES) { set_error("%s: the destination overlaps the source", name); return MF_ERR_INVALID_ARG; }
    size_t head = (16 - (d & 15)) & 15;
    if (head > total) head = total;
    const size_t runs = (total - head) / luma::RUN;
    const int wide = ((s + head * PIXEL_BYTES) & 15) == 0;
    const size_t per_launch = (size_t)luma::MAX_BLOCKS * luma::LANES;
    for (size_t first = 0; first == 0 || first < runs; first += per_launch) {
        const size_t left = runs - first < per_launch ? runs - first : per_launch;
        const size_t blocks = left ? (left + luma::LANES - 1) / luma::LANES : 1;          // (no run at all: the head and tail still want a workgroup)
        hipLaunchKernelGGL(luma_kernel<SRC>, dim3((unsigned)blocks), dim3(luma::LANES), 0, (hipStream_t)stream, (const uint8_t*)src, dst,
                           (uint64_t)total, (uint32_t)head, (uint64_t)runs, (uint64_t)first, wide, luma::weights<SRC>(red_first));
        MF_HIP_TRY(hipGetLastError());
    }
    return MF_OK;
}

}  // namespace mf

using namespace mf;

extern "C" {

int mf_luma_u8c3(const void* d_src, int n, int W, int H, int red_first, uint8_t* d_dst, void* stream)
{
    return luma_entry<luma::U8C3>("mf_luma_u8c3", d_src, n, W, H, red_first, d_dst, stream);
}

int mf_luma_u8c4(const void* d_src, int n, int W, int H, int red_first, uint8_t* d_dst, void* stream)
{
    return luma_entry<luma::U8C4>("mf_luma_u8c4", d_src, n, W, H, red_first, d_dst, stream);
}

int mf_luma_u16c3(const void* d_src, int n, int W, int H, int red_first, uint8_t* d_dst, void* stream)
{
    return luma_entry<luma::U16C3>("mf_luma_u16c3", d_src, n, W, H, red_first, d_dst, stream);
}

int mf_luma_u16(const void* d_src, int n, int W, int H, uint8_t* d_dst, void* stream)
{
    return luma_entry<luma::U16C1>("mf_luma_u16", d_src, n, W, H, 0, d_dst, stream);
}

}  // extern "C"
