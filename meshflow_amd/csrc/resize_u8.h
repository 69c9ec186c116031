// The device helpers and tile constants every 8-bit crop-resize kernel shares (resize_body.h, resize_c1_body.h, resize_c4_body.h,
// resize_to_body.h), each defined here once; the BGR row passes (hpass_row, vpass_store) are resize_kernel's and resize_to_kernel's.
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
