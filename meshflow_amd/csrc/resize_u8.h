// The device pieces every 8-bit crop-resize kernel shares (resize_body.h: u8c3, resize_c1_body.h: u8c1, resize_c4_body.h: u8c4), each defined
// here once: the tile constants, a wavefront's tile (Tile8: decode, geometry, the test that a staged copy stays inside the frame stack, the
// global->LDS copy of its source rows), and the BGR row passes (hpass_row, vpass_store) of resize_body.h.
#pragma once
#include "mf_common.h"

namespace mf {

// B | G << 8 | R << 16 of the pixel at byte offset o; the 4-byte load of the very last pixel of the stack is
// shifted back by one byte instead of running past the allocation.
__device__ __forceinline__ uint32_t load_bgr(const uint8_t* __restrict__ frame, uint32_t o, size_t limit)
{
    uint32_t v;
    if ((size_t)o + 4 <= limit) {
        __builtin_memcpy(&v, frame + o, 4);
    } else if (o != 0) {
        __builtin_memcpy(&v, frame + o - 1, 4);
        v >>= 8;
    } else {                                             // a stack of ONE pixel: nothing in front of it either
        v = (uint32_t)frame[0] | (uint32_t)frame[1] << 8 | (uint32_t)frame[2] << 16;
    }
    return v & 0xFFFFFFu;
}

// Tiles: a workgroup is kWaves wavefronts that never cooperate; a wavefront owns kRows consecutive output rows x 256 pixels, a lane 4
// consecutive pixels per row.  _crop_frames only ever scales UP (the crop lies inside the frame), so consecutive output rows advance by at
// most one source row and the kRows output rows read at most kSrcRows source rows.
constexpr int kRows = 8;              // output rows per wavefront
constexpr int kWaves = 4;             // wavefronts per workgroup
constexpr int kSrcRows = kRows + 1;   // source rows a wavefront stages
constexpr int kRowPitch = 800;        // u8c3: bytes of one staged source row in LDS, 50 chunks of 16 bytes (256 output px + slack)
constexpr int kC1RowPitch = 272;      // u8c1: 17 chunks, 258 bytes + up to 3 of misalignment in front

// High 32 bits of the product of two 24-bit values (v_mul_hi_u32_u24).
__device__ __forceinline__ uint32_t mulhi_u24(uint32_t a, uint32_t b)
{
    return (uint32_t)(((unsigned long long)(a & 0xFFFFFFu) * (unsigned long long)(b & 0xFFFFFFu)) >> 32);
}

// One wavefront's tile of an 8-bit crop-resize, the part that does not depend on the pixel format beyond its BPP bytes per pixel: ROWS
// consecutive output rows x 256 output pixels (a lane: 4 consecutive pixels per row) of frame f, source pitch W and frame W H BPP bytes,
// output oW x oH (the same-size kernels: oW = W, oH = H); the tables are resize_tables_kernel's for (oW, oH).  The tile's source rows go to
// LDS slots: slot i holds source row r_first + i (!PAIRS, an upscale: consecutive output rows advance by at most one source row), or row h
// of output row ya + q for i = 2q + h (PAIRS: exactly the two rows of each output row, nothing unused copied).
template <int BPP, int ROWS, bool PAIRS>
struct Tile8 {
    int wave, lane;
    int ya, rows, x0;                        // first output row and how many; the lane's first output pixel
    const uint8_t* src;                      // frame f; `limit` bytes from here to the end of the stack, `base` its address
    uint8_t* dst;
    size_t limit, base;
    // span of source columns the wavefront touches: taps sx .. sx+1 for its first .. last pixel (the tables are monotone), in bytes, and of
    // source rows: sy0 of its first .. sy1 of its last output row
    uint32_t sx_first, span;
    int r_first, r_last, nsrc;
    const ResizeTab* ytab;
    int W, left, top;

    // false: the workgroup or the wavefront has no tile (nothing read or written yet)
    __device__ __forceinline__ bool decode(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n, int W_, int H, int left_, int top_,
                                           int oW, int oH, const ResizeTab* __restrict__ xtab, const ResizeTab* __restrict__ ytab_,
                                           const TileOrder& order)
    {
        int f, tile_y, tile_x;
        if (!order.decode(blockIdx.x, f, tile_y, tile_x)) return false;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
        ya = (tile_y * kWaves + wave) * ROWS;
        const int xw = tile_x * 256;
        x0 = xw + lane * 4;
        if (ya >= oH) return false;
        rows = min(ROWS, oH - ya);
        const size_t frame_bytes = (size_t)W_ * H * BPP, out_frame_bytes = (size_t)oW * oH * BPP;
        src = frames + (size_t)f * frame_bytes;
        dst = out + (size_t)f * out_frame_bytes;
        limit = (size_t)(n - f) * frame_bytes;
        base = (size_t)(uintptr_t)src;
        ytab = ytab_, W = W_, left = left_, top = top_;
        sx_first = (uint32_t)xtab[xw].ofs;
        span = (uint32_t)BPP * ((uint32_t)xtab[min(xw + 255, oW - 1)].ofs + 2u - sx_first);
        r_first = ytab[ya].ofs & 0xFFFF, r_last = ytab[ya + rows - 1].ofs >> 16;
        nsrc = PAIRS ? 2 * rows : r_last - r_first + 1;
        return true;
    }
    // the source row (in the crop) slot i holds
    __device__ __forceinline__ int src_row(int i) const
    {
        if (!PAIRS) return r_first + i;
        const int32_t o = ytab[ya + (i >> 1)].ofs;
        return (i & 1) ? (o >> 16) : (o & 0xFFFF);
    }
    // byte offset in the frame of the first tap of source row r: ((top + r) W + left + sx_first) BPP
    __device__ __forceinline__ size_t g_of(int r) const { return ((size_t)(top + r) * (size_t)W + (size_t)left + sx_first) * (size_t)BPP; }
    // Bytes in front of slot i's first tap: a copy starts at the dword holding the tap.  !PAIRS: the rows are consecutive, so the
    // misalignment advances by (BPP W) & 3 per slot and nothing is loaded for it.
    __device__ __forceinline__ uint32_t mis_of(int i) const
    {
        if (!PAIRS) return ((uint32_t)(base + g_of(r_first)) + (uint32_t)i * (uint32_t)(BPP * W)) & 3u;
        return (uint32_t)((base + g_of(src_row(i))) & 3u);
    }
    // Whether the tile is staged: it has LDS at all (PITCH > 0), its rows fit the SLOTS, its span plus the format's SLACK bytes (the misalignment
    // in front of the first tap, and the margin the format keeps behind the last) fit a PITCH-byte row, and every copy stays inside the frame
    // stack.  The rows are monotone, so the first and the last staged row bound every copy: behind, PITCH bytes from the last row's first tap
    // (conservative by the misalignment); in front, the 3 bytes a copy may start before its tap -- or, ALIGNED (4-byte pixels), a 4-byte
    // aligned stack, where every tap is a dword of its own and no copy starts in front of it.
    template <int SLOTS, int PITCH, int SLACK, bool ALIGNED>
    __device__ __forceinline__ bool fits(const uint8_t* frames) const
    {
        return PITCH > 0 && nsrc <= SLOTS && span + (uint32_t)SLACK <= (uint32_t)PITCH &&
               (ALIGNED ? ((uintptr_t)frames & 3u) == 0 : g_of(r_first) >= 3u) && g_of(r_last) + (size_t)PITCH <= limit;
    }
    // The staged copy, the column table entries of the lane's four pixels, and the one wait for both.  Slot i is the STRIDE bytes at
    // lds + i STRIDE; the wavefront copies PITCH bytes of each source row there, from the dword holding the row's first tap, with one 16-byte
    // global->LDS load per lane and chunk (the LDS address of such a load is wavefront-uniform: the lanes land 16 bytes apart).
    template <int PITCH, int STRIDE, bool ALIGNED>
    __device__ __forceinline__ void stage_rows(bool staged, uint8_t* lds, const ResizeTab* __restrict__ xtab, int oW, ResizeTab (&xt)[4]) const
    {
        // A row of at most 64 chunks (u8c3 and u8c1 `up`) is one load per lane: which lanes have a chunk is decided once, in front of the row
        // loop, as the same-size kernels did (per row it cost u8c1 3-5 %, profiles/crop_resize_one_body.md); wider rows decide per chunk.
        constexpr int CHUNKS = PITCH / 16;
        if (staged && (CHUNKS > 64 || lane < CHUNKS)) {
            const size_t g_first = g_of(r_first), row_bytes = (size_t)W * (size_t)BPP;
#pragma unroll 1
            for (int i = 0; i < nsrc; ++i) {
                const size_t g = PAIRS ? g_of(src_row(i)) : g_first + (size_t)i * row_bytes;     // (consecutive rows advance by a row)
                const uint8_t* const a = src + (ALIGNED ? g : g - ((base + g) & 3u));
#pragma unroll
                for (int c = 0; c < CHUNKS; c += 64) {
                    if (CHUNKS <= 64 || lane + c < CHUNKS) {
                        uint32_t o = (uint32_t)(lane + c) << 4;
                        asm("" : "+v"(o));
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a + o),
                                                         (__attribute__((address_space(3))) void*)(lds + i * STRIDE + c * 16), 16, 0, 0);
                    }
                }
            }
        }
        if (x0 < oW) {
#pragma unroll
            for (int j = 0; j < 4; ++j) xt[j] = xtab[min(x0 + j, oW - 1)];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // staged rows (and the column table) have landed
    }
};

// The horizontal pass of ONE staged source row for the lane's four pixels.  The wavefront has copied the span of the row it needs into LDS
// (from the dword holding its first tap, 16-byte global->LDS chunks); at[j] is the LDS byte address of pixel j's first tap there.
// t = S[sx] a0 + S[sx+1] a1 per channel (v_dot2_u32_u16 with the weights pre-scaled by 16: T = 16 t < 2^24), returned as
// T & ~255 = 256 (t >> 4), what the vertical pass multiplies.  The taps are byte loads with immediate offsets: ds_read_u8 puts S[sx] into
// the low byte of one register, ds_read_u8_d16_hi S[sx+1] into bits 16-23 of another (with SRAM ECC a d16 load zeroes the other half of its
// destination: check_d16_zero_fill), one v_or_b32 joins them.  All 24 loads and their wait sit in ONE asm block: nothing can be scheduled
// between issue and wait.
__device__ __forceinline__ void hpass_row(const uint32_t (&at)[4], const uint32_t (&w)[4], uint32_t (&T)[4][3])
{
    uint32_t lo[4][3], hi[4][3];
    asm volatile("ds_read_u8 %0, %24 offset:0\n\tds_read_u8_d16_hi %1, %24 offset:3\n\t"
                 "ds_read_u8 %2, %24 offset:1\n\tds_read_u8_d16_hi %3, %24 offset:4\n\t"
                 "ds_read_u8 %4, %24 offset:2\n\tds_read_u8_d16_hi %5, %24 offset:5\n\t"
                 "ds_read_u8 %6, %25 offset:0\n\tds_read_u8_d16_hi %7, %25 offset:3\n\t"
                 "ds_read_u8 %8, %25 offset:1\n\tds_read_u8_d16_hi %9, %25 offset:4\n\t"
                 "ds_read_u8 %10, %25 offset:2\n\tds_read_u8_d16_hi %11, %25 offset:5\n\t"
                 "ds_read_u8 %12, %26 offset:0\n\tds_read_u8_d16_hi %13, %26 offset:3\n\t"
                 "ds_read_u8 %14, %26 offset:1\n\tds_read_u8_d16_hi %15, %26 offset:4\n\t"
                 "ds_read_u8 %16, %26 offset:2\n\tds_read_u8_d16_hi %17, %26 offset:5\n\t"
                 "ds_read_u8 %18, %27 offset:0\n\tds_read_u8_d16_hi %19, %27 offset:3\n\t"
                 "ds_read_u8 %20, %27 offset:1\n\tds_read_u8_d16_hi %21, %27 offset:4\n\t"
                 "ds_read_u8 %22, %27 offset:2\n\tds_read_u8_d16_hi %23, %27 offset:5\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(lo[0][0]), "=&v"(hi[0][0]), "=&v"(lo[0][1]), "=&v"(hi[0][1]), "=&v"(lo[0][2]), "=&v"(hi[0][2]),
                   "=&v"(lo[1][0]), "=&v"(hi[1][0]), "=&v"(lo[1][1]), "=&v"(hi[1][1]), "=&v"(lo[1][2]), "=&v"(hi[1][2]),
                   "=&v"(lo[2][0]), "=&v"(hi[2][0]), "=&v"(lo[2][1]), "=&v"(hi[2][1]), "=&v"(lo[2][2]), "=&v"(hi[2][2]),
                   "=&v"(lo[3][0]), "=&v"(hi[3][0]), "=&v"(lo[3][1]), "=&v"(hi[3][1]), "=&v"(lo[3][2]), "=&v"(hi[3][2])
                 : "v"(at[0]), "v"(at[1]), "v"(at[2]), "v"(at[3]) : "memory");
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[j][c] = udot2(lo[j][c] | hi[j][c], w[j], 0u) & ~255u;
}

// The vertical pass + store of one output row: out = (((b0 (t0 >> 4)) >> 16) + ((b1 (t1 >> 4)) >> 16) + 2) >> 2, each product's
// high half by one v_mul_hi_u32_u24 of (256 b) and (256 (t >> 4)).  No saturation needed: each weight pair sums to 2048 +- 1 (two
// cvRound of complementary fractions), so t <= 255 * 2049, t >> 4 <= 32655 and the two high halves sum to at most
// 2049 * 32655 / 65536 < 1021, i.e. (sum + 2) >> 2 <= 255 -- cv2's saturate_cast never triggers either.
__device__ __forceinline__ void vpass_store(const uint32_t (&T0)[4][3], const uint32_t (&T1)[4][3], uint32_t b0s, uint32_t b1s,
                                            uint8_t* __restrict__ dst, uint32_t o, int x0, int W)
{
    uint32_t px[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t vB = (mulhi_u24(b0s, T0[j][0]) + mulhi_u24(b1s, T1[j][0]) + 2u) >> 2;
        const uint32_t vG = (mulhi_u24(b0s, T0[j][1]) + mulhi_u24(b1s, T1[j][1]) + 2u) >> 2;
        const uint32_t vR = (mulhi_u24(b0s, T0[j][2]) + mulhi_u24(b1s, T1[j][2]) + 2u) >> 2;
        px[j] = vB | (vG << 8) | (vR << 16);
    }
    if (x0 + 3 < W) {
        uint3 d;
        d.x = px[0] | (px[1] << 24);
        d.y = (px[1] >> 8) | (px[2] << 16);
        d.z = (px[2] >> 16) | (px[3] << 8);
        if ((W & 3) == 0) *reinterpret_cast<uint3*>(dst + o) = d;
        else __builtin_memcpy(dst + o, &d, 12);                  // (a row of W % 4 != 0 starts anywhere: one unaligned 12-byte store)
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < W) {
                dst[o + 3 * j + 0] = (uint8_t)(px[j]);
                dst[o + 3 * j + 1] = (uint8_t)(px[j] >> 8);
                dst[o + 3 * j + 2] = (uint8_t)(px[j] >> 16);
            }
    }
}

}  // namespace mf
