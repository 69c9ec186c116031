// Packed 4:2:2 in and out of the NV16 pair (mf_unpack_422_u8, mf_pack_422_u8): what capture cards emit -- YUY2 / YUYV (bytes Y0 U Y1 V) and
// UYVY (U Y0 V Y1) -- against the planes the warp takes, y [n][H][W] and uv [n][H][W/2][2].  Bit for bit tests/nv16_model.py's slicing.
//
// W is even, so a packed clip is a flat stream of 4-byte WORDS, word k holding luma pixels 2k and 2k + 1 and the chroma pair they share: no row
// or frame boundary falls inside a word, and rows and frames do not matter to the kernels.  Per word the packed side moves 4 bytes and `y` and
// `uv` 2 bytes each, in step.  Both kernels follow luma.hip: ONE kernel over the stream, cut where the DESTINATION is 16-byte aligned:
//   head   the words in front of the first aligned destination byte (unpack: 0 .. 7, by `y`; pack: 0 .. 3, by `packed`; all of a shorter clip)
//   runs   8 words each, one lane per run: 32 packed bytes against 16 bytes of `y` and 16 of `uv`
//   tail   the 0 .. 7 words behind the last run
// A run's accesses are as wide as the addresses allow and never wider:
//   unpack  two dwordx4 loads where the run's packed bytes are 16-byte aligned (WIDE_SRC), else eight dword loads (the packed side is 4-byte
//           aligned by contract); one 16-byte store to `y` and one to `uv` where `uv` is in phase with `y` mod 16 (WIDE_DST), else eight 2-byte
//           stores to each (both are 2-byte aligned by contract)
//   pack    one dwordx4 load from `y` and one from `uv` where both are 16-byte aligned at the run (WIDE_SRC), else eight 2-byte loads from each;
//           always two 16-byte stores (the cut aligns them)
// Bytes are separated and merged by v_perm_b32.  Head and tail are at most 14 words; lanes 0 .. 15 of the first workgroup take one each, with
// one dword access on the packed side and one 2-byte access on each plane.
// Indices are 64-bit (1,200 4K frames are 4.98e9 words).  A launch is capped at luma::MAX_BLOCKS workgroups of luma::LANES lanes, one run per
// lane and no loop in the kernel; the host strides over the rest of a longer clip, launch by launch on the same stream.  No LDS, no atomics,
// nothing kept between words.
// Bounds: run g < runs covers words [head + 8 g, head + 8 g + 8) with head + 8 (g + 1) <= words; head and tail words are below `words` by
// their own tests.  Word k is packed bytes [4 k, 4 k + 4), y bytes [2 k, 2 k + 2) and uv bytes [2 k, 2 k + 2).
#include "mf_common.h"
#include "luma_body.h"

namespace mf {

namespace pack422 {
constexpr int RUN = 8;                      // words per lane: 16 bytes of each plane, 32 packed
// v_perm_b32 selectors on {second word : first word} (bytes 4 .. 7 : 0 .. 3): the even bytes and the odd bytes of the pair
constexpr uint32_t EVEN = 0x06040200u, ODD = 0x07050301u;
// ... and on {b : a}: a0 b0 a1 b1 and a2 b2 a3 b3
constexpr uint32_t ZIP_LO = 0x05010400u, ZIP_HI = 0x07030602u;
}  // namespace pack422

// one word apart: yuyv (order 0) has luma in the even bytes, uyvy (order 1) in the odd ones
__device__ __forceinline__ void split_word(uint32_t w, int order, uint16_t& y2, uint16_t& uv2)
{
    const uint32_t even = __builtin_amdgcn_perm(0u, w, 0x0C0C0200u), odd = __builtin_amdgcn_perm(0u, w, 0x0C0C0301u);
    y2 = (uint16_t)(order ? odd : even);
    uv2 = (uint16_t)(order ? even : odd);
}
__device__ __forceinline__ uint32_t join_word(uint32_t y2, uint32_t uv2, int order)
{
    return order ? __builtin_amdgcn_perm(y2, uv2, pack422::ZIP_LO) : __builtin_amdgcn_perm(uv2, y2, pack422::ZIP_LO);
}

__global__ void __launch_bounds__(luma::LANES) unpack422_kernel(const uint8_t* __restrict__ packed, uint8_t* __restrict__ y, uint8_t* __restrict__ uv,
                                                                uint64_t words, uint32_t head, uint64_t runs, uint64_t first, int wide_src,
                                                                int wide_dst, int order)
{
    constexpr int RUN = pack422::RUN;
    const uint64_t g = first + (uint64_t)blockIdx.x * luma::LANES + threadIdx.x;
    if (g < runs) {
        const uint64_t k = head + g * RUN;
        uint32_t w[RUN];
        if (wide_src) {
            const uint4* __restrict__ from = reinterpret_cast<const uint4*>(packed + 4 * k);
            const uint4 a = from[0], b = from[1];
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        } else {
            const uint32_t* __restrict__ from = reinterpret_cast<const uint32_t*>(packed + 4 * k);
#pragma unroll
            for (int i = 0; i < RUN; ++i) w[i] = from[i];
        }
        const uint32_t sel_y = order ? pack422::ODD : pack422::EVEN, sel_uv = order ? pack422::EVEN : pack422::ODD;
        uint32_t yy[RUN / 2], cc[RUN / 2];
#pragma unroll
        for (int i = 0; i < RUN / 2; ++i) {
            yy[i] = __builtin_amdgcn_perm(w[2 * i + 1], w[2 * i], sel_y);
            cc[i] = __builtin_amdgcn_perm(w[2 * i + 1], w[2 * i], sel_uv);
        }
        if (wide_dst) {
            *reinterpret_cast<uint4*>(y + 2 * k) = make_uint4(yy[0], yy[1], yy[2], yy[3]);
            *reinterpret_cast<uint4*>(uv + 2 * k) = make_uint4(cc[0], cc[1], cc[2], cc[3]);
        } else {
            uint16_t* __restrict__ ty = reinterpret_cast<uint16_t*>(y + 2 * k);
            uint16_t* __restrict__ tc = reinterpret_cast<uint16_t*>(uv + 2 * k);
#pragma unroll
            for (int i = 0; i < RUN; ++i) {
                ty[i] = (uint16_t)(yy[i >> 1] >> (16 * (i & 1)));
                tc[i] = (uint16_t)(cc[i >> 1] >> (16 * (i & 1)));
            }
        }
    }
    if (first != 0 || blockIdx.x != 0 || threadIdx.x >= 2 * RUN) return;
    const uint32_t t = threadIdx.x;
    const uint64_t k = t < RUN ? t : head + runs * RUN + (t - RUN);
    if (t < RUN ? t < head : k < words) {
        uint16_t y2, uv2;
        split_word(reinterpret_cast<const uint32_t*>(packed)[k], order, y2, uv2);
        reinterpret_cast<uint16_t*>(y)[k] = y2;
        reinterpret_cast<uint16_t*>(uv)[k] = uv2;
    }
}

__global__ void __launch_bounds__(luma::LANES) pack422_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ uv, uint8_t* __restrict__ packed,
                                                              uint64_t words, uint32_t head, uint64_t runs, uint64_t first, int wide_src, int order)
{
    constexpr int RUN = pack422::RUN;
    const uint64_t g = first + (uint64_t)blockIdx.x * luma::LANES + threadIdx.x;
    if (g < runs) {
        const uint64_t k = head + g * RUN;
        uint32_t yy[RUN / 2], cc[RUN / 2];
        if (wide_src) {
            const uint4 a = *reinterpret_cast<const uint4*>(y + 2 * k), b = *reinterpret_cast<const uint4*>(uv + 2 * k);
            yy[0] = a.x; yy[1] = a.y; yy[2] = a.z; yy[3] = a.w;
            cc[0] = b.x; cc[1] = b.y; cc[2] = b.z; cc[3] = b.w;
        } else {
            const uint16_t* __restrict__ fy = reinterpret_cast<const uint16_t*>(y + 2 * k);
            const uint16_t* __restrict__ fc = reinterpret_cast<const uint16_t*>(uv + 2 * k);
#pragma unroll
            for (int i = 0; i < RUN / 2; ++i) {
                yy[i] = (uint32_t)fy[2 * i] | ((uint32_t)fy[2 * i + 1] << 16);
                cc[i] = (uint32_t)fc[2 * i] | ((uint32_t)fc[2 * i + 1] << 16);
            }
        }
        uint32_t w[RUN];
#pragma unroll
        for (int i = 0; i < RUN / 2; ++i) {
            // yuyv: Y0 U Y1 V -- luma is the low operand's bytes; uyvy: the chroma's
            const uint32_t lo = order ? cc[i] : yy[i], hi = order ? yy[i] : cc[i];
            w[2 * i] = __builtin_amdgcn_perm(hi, lo, pack422::ZIP_LO);
            w[2 * i + 1] = __builtin_amdgcn_perm(hi, lo, pack422::ZIP_HI);
        }
        uint4* __restrict__ to = reinterpret_cast<uint4*>(packed + 4 * k);
        to[0] = make_uint4(w[0], w[1], w[2], w[3]);
        to[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    if (first != 0 || blockIdx.x != 0 || threadIdx.x >= 2 * RUN) return;
    const uint32_t t = threadIdx.x;
    const uint64_t k = t < RUN ? t : head + runs * RUN + (t - RUN);
    if (t < RUN ? t < head : k < words)
        reinterpret_cast<uint32_t*>(packed)[k] =
            join_word(reinterpret_cast<const uint16_t*>(y)[k], reinterpret_cast<const uint16_t*>(uv)[k], order);
}

// The checks of both entries (nothing is launched where one fails), then the launches.  `to_planes`: unpack.
static int pack422_entry(const char* name, bool to_planes, const uint8_t* packed, const uint8_t* y, const uint8_t* uv, int n, int W, int H, int order,
                         void* stream)
{
    constexpr size_t RUN = pack422::RUN;
    if (!packed || !y || !uv) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: n must be at least 1 (got %d)", name, n); return MF_ERR_INVALID_ARG; }
    if (W < 2 || W > luma::MAX_DIM || (W & 1)) { set_error("%s: W must be even and in 2 .. %d (got %d)", name, luma::MAX_DIM, W); return MF_ERR_INVALID_ARG; }
    if (H < 1 || H > luma::MAX_DIM) { set_error("%s: H must be in 1 .. %d (got %d)", name, luma::MAX_DIM, H); return MF_ERR_INVALID_ARG; }
    if (order != 0 && order != 1) { set_error("%s: order must be 0 (yuyv) or 1 (uyvy) (got %d)", name, order); return MF_ERR_INVALID_ARG; }
    const uintptr_t p = (uintptr_t)packed, a = (uintptr_t)y, c = (uintptr_t)uv;
    if (p & 3u) { set_error("%s: d_packed must be 4-byte aligned", name); return MF_ERR_INVALID_ARG; }
    if ((a | c) & 1u) { set_error("%s: d_y and d_uv must be 2-byte aligned", name); return MF_ERR_INVALID_ARG; }
    const size_t words = (size_t)n * (size_t)(W / 2) * (size_t)H;           // below 2^60
    const struct { uintptr_t at; size_t bytes; const char* what; } b[3] = { { p, 4 * words, "d_packed" }, { a, 2 * words, "d_y" }, { c, 2 * words, "d_uv" } };
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (b[i].at < b[j].at + b[j].bytes && b[j].at < b[i].at + b[i].bytes) {
                set_error("%s: %s and %s overlap", name, b[i].what, b[j].what);
                return MF_ERR_INVALID_ARG;
            }
    // the cut: by `y` (2 bytes per word) for unpack, by `packed` (4 bytes per word) for pack
    size_t head = to_planes ? ((16 - (a & 15)) & 15) / 2 : ((16 - (p & 15)) & 15) / 4;
    if (head > words) head = words;
    const size_t runs = (words - head) / RUN;
    const bool planes_in_phase = ((a + 2 * head) & 15) == 0 && ((c + 2 * head) & 15) == 0;
    const int wide_src = to_planes ? ((p + 4 * head) & 15) == 0 : planes_in_phase;
    const int wide_dst = planes_in_phase;                                   // (unpack only; pack's destination is aligned by the cut)
    const size_t per_launch = (size_t)luma::MAX_BLOCKS * luma::LANES;
    for (size_t first = 0; first == 0 || first < runs; first += per_launch) {
        const size_t left = runs - first < per_launch ? runs - first : per_launch;
        const size_t blocks = left ? (left + luma::LANES - 1) / luma::LANES : 1;          // (no run at all: the head and tail still want a workgroup)
        if (to_planes)
            hipLaunchKernelGGL(unpack422_kernel, dim3((unsigned)blocks), dim3(luma::LANES), 0, (hipStream_t)stream, packed, const_cast<uint8_t*>(y),
                               const_cast<uint8_t*>(uv), (uint64_t)words, (uint32_t)head, (uint64_t)runs, (uint64_t)first, wide_src, wide_dst, order);
        else
            hipLaunchKernelGGL(pack422_kernel, dim3((unsigned)blocks), dim3(luma::LANES), 0, (hipStream_t)stream, y, uv, const_cast<uint8_t*>(packed),
                               (uint64_t)words, (uint32_t)head, (uint64_t)runs, (uint64_t)first, wide_src, order);
        MF_HIP_TRY(hipGetLastError());
    }
    return MF_OK;
}

}  // namespace mf

using namespace mf;

extern "C" {

int mf_unpack_422_u8(const uint8_t* d_packed, uint8_t* d_y, uint8_t* d_uv, int n, int W, int H, int order, void* stream)
{
    return pack422_entry("mf_unpack_422_u8", true, d_packed, d_y, d_uv, n, W, H, order, stream);
}

int mf_pack_422_u8(const uint8_t* d_y, const uint8_t* d_uv, uint8_t* d_packed, int n, int W, int H, int order, void* stream)
{
    return pack422_entry("mf_pack_422_u8", false, d_packed, d_y, d_uv, n, W, H, order, stream);
}

}  // extern "C"
