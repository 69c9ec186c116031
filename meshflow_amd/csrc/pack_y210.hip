// Packed 10-bit 4:2:2 in and out of the P210 pair (mf_unpack_y210_u16, mf_pack_y210_u16): Y210 / Y216 -- uint16 samples Y0 U Y1 V, what
// capture SDKs and hardware decoders hand over for 10-bit 4:2:2 -- against the planes the warp takes, y [n][H][W] and uv [n][H][W/2][2], all
// uint16.  Samples are plain 16-bit numbers and move as bits: nothing is masked or shifted, so Y210, Y212 and Y216 are the same call.  Bit for
// bit tests/p210_model.py's slicing.  One sample order only (there is no 16-bit UYVY in use).
//
// W is even, so a packed clip is a flat stream of 8-byte WORDS, word k holding luma pixels 2k and 2k + 1 and the chroma pair they share: no row
// or frame boundary falls inside a word, and rows and frames do not matter to the kernels.  Per word the packed side moves 8 bytes and `y` and
// `uv` 4 bytes each, in step.  Both kernels follow pack422.hip: ONE kernel over the stream, cut where the DESTINATION is 16-byte aligned:
//   head   the words in front of the first aligned destination byte (unpack: 0 .. 3, by `y`; pack: 0 or 1, by `packed`; all of a shorter clip)
//   runs   4 words each, one lane per run: 32 packed bytes against 16 bytes of `y` and 16 of `uv`
//   tail   the 0 .. 3 words behind the last run
// Alignment contract: `packed` is 8-byte aligned (a word is never split; refused otherwise), `y` and `uv` 2-byte aligned (their samples).
// A run's accesses are as wide as the addresses allow and never wider:
//   unpack  two dwordx4 loads where the run's packed bytes are 16-byte aligned (WIDE_SRC), else four dwordx2 loads; one 16-byte store to `y`
//           and one to `uv` where both are 16-byte aligned at the run (WIDE_DST), else eight 2-byte stores to each.  A `y` that is not 4-byte
//           aligned never comes to a 16-byte boundary in whole words: head = 0 and every run takes the 2-byte stores.
//   pack    one dwordx4 load from `y` and one from `uv` where both are 16-byte aligned at the run (WIDE_SRC), else eight 2-byte loads from each;
//           always two 16-byte stores (the cut aligns them)
// The planes' 2-byte accesses go through volatile pointers: left to itself the compiler merges neighbouring ones into unaligned dword and
// dwordx4 accesses (gfx950's global memory would serve them), which is wider than the contract allows; volatile keeps each its own
// 2-byte load or store (flat_load_ushort / flat_store_short in the listing) at the cost of the cache bypass -- paid on the narrow layouts and the six head and tail words only.
// Halves are separated and merged by v_perm_b32.  Head and tail are at most 6 words; lanes 0 .. 7 of the first workgroup take one each, with
// one 8-byte access on the packed side and two 2-byte accesses on each plane.
// Indices are 64-bit.  A launch is capped at luma::MAX_BLOCKS workgroups of luma::LANES lanes, one run per lane and no loop in the kernel; the
// host strides over the rest of a longer clip, launch by launch on the same stream.  No LDS, no atomics, nothing kept between words.
// Bounds: run g < runs covers words [head + 4 g, head + 4 g + 4) with head + 4 (g + 1) <= words; head and tail words are below `words` by
// their own tests.  Word k is packed bytes [8 k, 8 k + 8), y bytes [4 k, 4 k + 4) and uv bytes [4 k, 4 k + 4).
#include "mf_common.h"
#include "luma_body.h"

namespace mf {

namespace y210 {
constexpr int RUN = 4;                      // words per lane: 16 bytes of each plane, 32 packed
// v_perm_b32 selectors on {b : a} (bytes 4 .. 7 : 0 .. 3): the low halves a.lo | b.lo << 16 and the high halves a.hi | b.hi << 16.
// Unpack: {Y1 V : Y0 U} gives Y0 Y1 and U V.  Pack: {U V : Y0 Y1} gives Y0 U and Y1 V.
constexpr uint32_t LO = 0x05040100u, HI = 0x07060302u;
}  // namespace y210

__global__ void __launch_bounds__(luma::LANES) unpack_y210_kernel(const uint16_t* __restrict__ packed, uint16_t* __restrict__ y,
                                                                  uint16_t* __restrict__ uv, uint64_t words, uint32_t head, uint64_t runs,
                                                                  uint64_t first, int wide_src, int wide_dst)
{
    constexpr int RUN = y210::RUN;
    const uint64_t g = first + (uint64_t)blockIdx.x * luma::LANES + threadIdx.x;
    if (g < runs) {
        const uint64_t k = head + g * RUN;
        uint32_t w[2 * RUN];
        if (wide_src) {
            const uint4* __restrict__ from = reinterpret_cast<const uint4*>(packed + 4 * k);
            const uint4 a = from[0], b = from[1];
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        } else {
            const uint2* __restrict__ from = reinterpret_cast<const uint2*>(packed + 4 * k);
#pragma unroll
            for (int i = 0; i < RUN; ++i) {
                const uint2 a = from[i];
                w[2 * i] = a.x;
                w[2 * i + 1] = a.y;
            }
        }
        uint32_t yy[RUN], cc[RUN];
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            yy[i] = __builtin_amdgcn_perm(w[2 * i + 1], w[2 * i], y210::LO);
            cc[i] = __builtin_amdgcn_perm(w[2 * i + 1], w[2 * i], y210::HI);
        }
        if (wide_dst) {
            *reinterpret_cast<uint4*>(y + 2 * k) = make_uint4(yy[0], yy[1], yy[2], yy[3]);
            *reinterpret_cast<uint4*>(uv + 2 * k) = make_uint4(cc[0], cc[1], cc[2], cc[3]);
        } else {
            volatile uint16_t* ty = y + 2 * k;                   // (volatile: see the head of the file -- kept as 2-byte accesses)
            volatile uint16_t* tc = uv + 2 * k;
#pragma unroll
            for (int i = 0; i < 2 * RUN; ++i) {
                ty[i] = (uint16_t)(yy[i >> 1] >> (16 * (i & 1)));
                tc[i] = (uint16_t)(cc[i >> 1] >> (16 * (i & 1)));
            }
        }
    }
    if (first != 0 || blockIdx.x != 0 || threadIdx.x >= 2 * RUN) return;
    const uint32_t t = threadIdx.x;
    const uint64_t k = t < RUN ? t : head + runs * RUN + (t - RUN);
    if (t < RUN ? t < head : k < words) {
        const uint2 a = reinterpret_cast<const uint2*>(packed)[k];
        volatile uint16_t* ty = y + 2 * k;
        volatile uint16_t* tc = uv + 2 * k;
        ty[0] = (uint16_t)a.x;
        tc[0] = (uint16_t)(a.x >> 16);
        ty[1] = (uint16_t)a.y;
        tc[1] = (uint16_t)(a.y >> 16);
    }
}

__global__ void __launch_bounds__(luma::LANES) pack_y210_kernel(const uint16_t* __restrict__ y, const uint16_t* __restrict__ uv,
                                                                uint16_t* __restrict__ packed, uint64_t words, uint32_t head, uint64_t runs,
                                                                uint64_t first, int wide_src)
{
    constexpr int RUN = y210::RUN;
    const uint64_t g = first + (uint64_t)blockIdx.x * luma::LANES + threadIdx.x;
    if (g < runs) {
        const uint64_t k = head + g * RUN;
        uint32_t yy[RUN], cc[RUN];
        if (wide_src) {
            const uint4 a = *reinterpret_cast<const uint4*>(y + 2 * k), b = *reinterpret_cast<const uint4*>(uv + 2 * k);
            yy[0] = a.x; yy[1] = a.y; yy[2] = a.z; yy[3] = a.w;
            cc[0] = b.x; cc[1] = b.y; cc[2] = b.z; cc[3] = b.w;
        } else {
            const volatile uint16_t* fy = y + 2 * k;             // (volatile: see the head of the file -- kept as 2-byte accesses)
            const volatile uint16_t* fc = uv + 2 * k;
#pragma unroll
            for (int i = 0; i < RUN; ++i) {
                yy[i] = (uint32_t)fy[2 * i] | ((uint32_t)fy[2 * i + 1] << 16);
                cc[i] = (uint32_t)fc[2 * i] | ((uint32_t)fc[2 * i + 1] << 16);
            }
        }
        uint32_t w[2 * RUN];
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            w[2 * i] = __builtin_amdgcn_perm(cc[i], yy[i], y210::LO);
            w[2 * i + 1] = __builtin_amdgcn_perm(cc[i], yy[i], y210::HI);
        }
        uint4* __restrict__ to = reinterpret_cast<uint4*>(packed + 4 * k);
        to[0] = make_uint4(w[0], w[1], w[2], w[3]);
        to[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    if (first != 0 || blockIdx.x != 0 || threadIdx.x >= 2 * RUN) return;
    const uint32_t t = threadIdx.x;
    const uint64_t k = t < RUN ? t : head + runs * RUN + (t - RUN);
    if (t < RUN ? t < head : k < words) {
        const volatile uint16_t* fy = y + 2 * k;
        const volatile uint16_t* fc = uv + 2 * k;
        uint2 a;
        a.x = (uint32_t)fy[0] | ((uint32_t)fc[0] << 16);
        a.y = (uint32_t)fy[1] | ((uint32_t)fc[1] << 16);
        reinterpret_cast<uint2*>(packed)[k] = a;
    }
}

// The checks of both entries (nothing is launched where one fails), then the launches.  `to_planes`: unpack.
static int y210_entry(const char* name, bool to_planes, const uint16_t* packed, const uint16_t* y, const uint16_t* uv, int n, int W, int H,
                      void* stream)
{
    constexpr size_t RUN = y210::RUN;
    if (!packed || !y || !uv) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: n must be at least 1 (got %d)", name, n); return MF_ERR_INVALID_ARG; }
    if (W < 2 || W > luma::MAX_DIM || (W & 1)) { set_error("%s: W must be even and in 2 .. %d (got %d)", name, luma::MAX_DIM, W); return MF_ERR_INVALID_ARG; }
    if (H < 1 || H > luma::MAX_DIM) { set_error("%s: H must be in 1 .. %d (got %d)", name, luma::MAX_DIM, H); return MF_ERR_INVALID_ARG; }
    const uintptr_t p = (uintptr_t)packed, a = (uintptr_t)y, c = (uintptr_t)uv;
    if (p & 7u) { set_error("%s: d_packed must be 8-byte aligned", name); return MF_ERR_INVALID_ARG; }
    if ((a | c) & 1u) { set_error("%s: d_y and d_uv must be 2-byte aligned", name); return MF_ERR_INVALID_ARG; }
    const size_t words = (size_t)n * (size_t)(W / 2) * (size_t)H;           // below 2^60
    const struct { uintptr_t at; size_t bytes; const char* what; } b[3] = { { p, 8 * words, "d_packed" }, { a, 4 * words, "d_y" }, { c, 4 * words, "d_uv" } };
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (b[i].at < b[j].at + b[j].bytes && b[j].at < b[i].at + b[i].bytes) {
                set_error("%s: %s and %s overlap", name, b[i].what, b[j].what);
                return MF_ERR_INVALID_ARG;
            }
    // the cut: by `y` (4 bytes per word; none where y is not 4-byte aligned) for unpack, by `packed` (8 bytes per word) for pack
    size_t head = to_planes ? ((a & 3u) ? 0 : ((16 - (a & 15)) & 15) / 4) : ((16 - (p & 15)) & 15) / 8;
    if (head > words) head = words;
    const size_t runs = (words - head) / RUN;
    const bool planes_in_phase = ((a + 4 * head) & 15) == 0 && ((c + 4 * head) & 15) == 0;
    const int wide_src = to_planes ? ((p + 8 * head) & 15) == 0 : planes_in_phase;
    const int wide_dst = planes_in_phase;                                   // (unpack only; pack's destination is aligned by the cut)
    const size_t per_launch = (size_t)luma::MAX_BLOCKS * luma::LANES;
    for (size_t first = 0; first == 0 || first < runs; first += per_launch) {
        const size_t left = runs - first < per_launch ? runs - first : per_launch;
        const size_t blocks = left ? (left + luma::LANES - 1) / luma::LANES : 1;          // (no run at all: the head and tail still want a workgroup)
        if (to_planes)
            hipLaunchKernelGGL(unpack_y210_kernel, dim3((unsigned)blocks), dim3(luma::LANES), 0, (hipStream_t)stream, packed, const_cast<uint16_t*>(y),
                               const_cast<uint16_t*>(uv), (uint64_t)words, (uint32_t)head, (uint64_t)runs, (uint64_t)first, wide_src, wide_dst);
        else
            hipLaunchKernelGGL(pack_y210_kernel, dim3((unsigned)blocks), dim3(luma::LANES), 0, (hipStream_t)stream, y, uv, const_cast<uint16_t*>(packed),
                               (uint64_t)words, (uint32_t)head, (uint64_t)runs, (uint64_t)first, wide_src);
        MF_HIP_TRY(hipGetLastError());
    }
    return MF_OK;
}

}  // namespace mf

using namespace mf;

extern "C" {

int mf_unpack_y210_u16(const uint16_t* d_packed, uint16_t* d_y, uint16_t* d_uv, int n, int W, int H, void* stream)
{
    return y210_entry("mf_unpack_y210_u16", true, d_packed, d_y, d_uv, n, W, H, stream);
}

int mf_pack_y210_u16(const uint16_t* d_y, const uint16_t* d_uv, uint16_t* d_packed, int n, int W, int H, void* stream)
{
    return y210_entry("mf_pack_y210_u16", false, d_packed, d_y, d_uv, n, W, H, stream);
}

}  // extern "C"
