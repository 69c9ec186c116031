// The uint8 BGR warp's taps and blend (device only, included through warp_body.h): from the staged window in LDS, or straight from the frame.
#ifndef MF_WARP_TAPS_U8C3_H
#define MF_WARP_TAPS_U8C3_H
#include "warp_coords.h"

namespace mf {

// Taps + blend of a footprint with a staged window.  The taps come from the staged window by BYTE loads with immediate offsets, already in the
// layout the blend wants -- per pixel and channel the two horizontal neighbours in the 16-bit halves of one register (X0 | X1 << 16),
// for rows iy and iy + 1: ds_read_u8 delivers X0 in the low byte of one register, ds_read_u8_d16_hi X1 in bits 16-23 of another
// (with SRAM ECC a d16 load zeroes the other half instead of preserving it: measured), and one v_or_b32 (a 2-cycle instruction) joins
// them.  Against three ds_read2_b32 + four v_alignbyte_b32 + six v_perm_b32 per pixel that is 28 VALU issue cycles per pixel less
// (the LDS pipe takes 12 byte loads per pixel instead; it has the room).  The compiler does not see these loads, so the waits are
// placed here.
struct TapRegs { uint32_t lo[6], hi[6]; };      // {B, G, R} of row iy, then of row iy + 1: X0 in lo (byte 0), X1 in hi (byte 2)

// Tap address of one pixel: LDS byte address of its top-left tap's B.
template <int PITCH>
__device__ __forceinline__ uint32_t tap_address(uint32_t bxj, uint32_t byj, uint32_t lds_origin)
{
    // ix = bits[5..21] of the raw float; bits[22..28] (the 1.5*2^23 pattern, constant) ride along in the 24-bit multiplier
    // operand and are taken out again through the origin
    return umad24(byj >> 5, (uint32_t)PITCH, umad24(bxj >> 5, 3u, 0u - lds_origin - MAGIC_HI * (3u + (uint32_t)PITCH)));
}

// The 24 byte loads of TWO pixels and their wait in ONE asm block: the compiler does not see LDS loads issued from inline asm, so nothing
// -- no copy, no spill, no reordering under another compiler version or flag -- can come between a load and the wait that makes its
// register valid.  (Row pitch in the immediates: one instantiation per window layout.)
#define MF_TAP_LOADS(R0, R1, R2, R3, R4, R5, R6, R7, R8, R9, R10, R11, A, P0, P1, P2, P3, P4, P5)                                    \
    "ds_read_u8 " R0 ", " A " offset:0\n\tds_read_u8_d16_hi " R1 ", " A " offset:3\n\t"                                              \
    "ds_read_u8 " R2 ", " A " offset:1\n\tds_read_u8_d16_hi " R3 ", " A " offset:4\n\t"                                              \
    "ds_read_u8 " R4 ", " A " offset:2\n\tds_read_u8_d16_hi " R5 ", " A " offset:5\n\t"                                              \
    "ds_read_u8 " R6 ", " A " offset:" P0 "\n\tds_read_u8_d16_hi " R7 ", " A " offset:" P3 "\n\t"                                    \
    "ds_read_u8 " R8 ", " A " offset:" P1 "\n\tds_read_u8_d16_hi " R9 ", " A " offset:" P4 "\n\t"                                    \
    "ds_read_u8 " R10 ", " A " offset:" P2 "\n\tds_read_u8_d16_hi " R11 ", " A " offset:" P5 "\n\t"
#define MF_TAP_PAIR_ASM(P0, P1, P2, P3, P4, P5)                                                                                     \
    asm volatile(MF_TAP_LOADS("%0", "%1", "%2", "%3", "%4", "%5", "%6", "%7", "%8", "%9", "%10", "%11", "%24", P0, P1, P2, P3, P4, P5)   \
                 MF_TAP_LOADS("%12", "%13", "%14", "%15", "%16", "%17", "%18", "%19", "%20", "%21", "%22", "%23", "%25", P0, P1, P2, P3, P4, P5) \
                 "s_waitcnt lgkmcnt(0)"                                                                                             \
                 : "=&v"(t.lo[0]), "=&v"(t.hi[0]), "=&v"(t.lo[1]), "=&v"(t.hi[1]), "=&v"(t.lo[2]), "=&v"(t.hi[2]),                  \
                   "=&v"(t.lo[3]), "=&v"(t.hi[3]), "=&v"(t.lo[4]), "=&v"(t.hi[4]), "=&v"(t.lo[5]), "=&v"(t.hi[5]),                  \
                   "=&v"(u.lo[0]), "=&v"(u.hi[0]), "=&v"(u.lo[1]), "=&v"(u.hi[1]), "=&v"(u.lo[2]), "=&v"(u.hi[2]),                  \
                   "=&v"(u.lo[3]), "=&v"(u.hi[3]), "=&v"(u.lo[4]), "=&v"(u.hi[4]), "=&v"(u.lo[5]), "=&v"(u.hi[5])                   \
                 : "v"(at0), "v"(at1) : "memory")
template <int PITCH>
__device__ __forceinline__ void taps_pair(uint32_t at0, uint32_t at1, TapRegs& t, TapRegs& u)
{
    static_assert(PITCH == MF_STAGE_PITCH || PITCH == MF_COMPACT_PITCH, "one asm string per window pitch");
    static_assert(MF_STAGE_PITCH == 160 && MF_COMPACT_PITCH == 112, "the immediate offsets below are the pitch + 0..5");
    if (PITCH == MF_STAGE_PITCH) MF_TAP_PAIR_ASM("160", "161", "162", "163", "164", "165");
    else MF_TAP_PAIR_ASM("112", "113", "114", "115", "116", "117");
}

// (Round 6, measured and dropped, profiles/r06_ab_trims.txt: the four weights as two packed pairs -- v_pk_mad_u16 with the clamp bit for
// 64 (32 - fx)(32 - fy) = 65536 -> 65535, v_pk_mul_lo_u16 -- and two chained v_dot2_u32_u16 per channel instead of v_mul + v_mad + dot2:
// 16 issue cycles per wavefront less by the table, byte-identical, +0.7...1.6 % SLOWER; and the tap address as two hand-placed
// v_mad_u32_u24: 8 cycles less, -0.3 % / -0.3 % / +1.6 %.  Neither the issue-cycle table nor the energy table (profiles/r03_ubench_power.txt) predicts that; cause not identified.)
__device__ __forceinline__ void blend_pixel(uint32_t bxj, uint32_t byj, const TapRegs& t, uint32_t& oB, uint32_t& oG, uint32_t& oR)
{
    // vertical lerp of both 16-bit fields at once (each <= 255 * 32: no carry between them)
    const uint32_t fy = byj & 31u, wy = 32u - fy;
    const uint32_t vB = umad24(t.lo[3] | t.hi[3], fy, __umul24(t.lo[0] | t.hi[0], wy));
    const uint32_t vG = umad24(t.lo[4] | t.hi[4], fy, __umul24(t.lo[1] | t.hi[1], wy));
    const uint32_t vR = umad24(t.lo[5] | t.hi[5], fy, __umul24(t.lo[2] | t.hi[2], wy));
    // horizontal lerp: v_dot2_u32_u16 with the weight pair (32 - fx, fx) scaled by 64, so that ((sum + 512) >> 10) lands in byte 2:
    // (sum + 512) * 64 < 2^24
    const uint32_t fx = bxj & 31u;
    const uint32_t wq = umad24(fx, 0x3FFFC0u, 2048u);           // 64 (32 - fx) | 64 fx << 16
    oB = udot2(vB, wq, 32768u);
    oG = udot2(vG, wq, 32768u);
    oR = udot2(vR, wq, 32768u);
}

// The 2 x 2 taps of ONE pixel from four separate LDS positions (the per-tap path of frame-border footprints: every tap at its position
// clamped into the frame, a00 / a01 = row iy at columns ix / ix + 1, a10 / a11 = row iy + 1), in the blend's layout.  Loads and wait in
// one asm block: nothing can be scheduled between them.
__device__ __forceinline__ void taps_clamped(uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11, TapRegs& t)
{
    asm volatile("ds_read_u8 %0, %12 offset:0\n\tds_read_u8_d16_hi %1, %13 offset:0\n\t"
                 "ds_read_u8 %2, %12 offset:1\n\tds_read_u8_d16_hi %3, %13 offset:1\n\t"
                 "ds_read_u8 %4, %12 offset:2\n\tds_read_u8_d16_hi %5, %13 offset:2\n\t"
                 "ds_read_u8 %6, %14 offset:0\n\tds_read_u8_d16_hi %7, %15 offset:0\n\t"
                 "ds_read_u8 %8, %14 offset:1\n\tds_read_u8_d16_hi %9, %15 offset:1\n\t"
                 "ds_read_u8 %10, %14 offset:2\n\tds_read_u8_d16_hi %11, %15 offset:2\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(t.lo[0]), "=&v"(t.hi[0]), "=&v"(t.lo[1]), "=&v"(t.hi[1]), "=&v"(t.lo[2]), "=&v"(t.hi[2]),
                   "=&v"(t.lo[3]), "=&v"(t.hi[3]), "=&v"(t.lo[4]), "=&v"(t.hi[4]), "=&v"(t.lo[5]), "=&v"(t.hi[5])
                 : "v"(a00), "v"(a01), "v"(a10), "v"(a11) : "memory");
}

// (two pixels' loads in flight at a time: 24 registers; a software pipeline with counted lgkmcnt waits measured the same.  Round 6: the
// taps as 16-bit loads -- three per tap row instead of six byte loads, one v_perm_b32 per channel and row instead of a v_or_b32 -- are
// byte-identical and 3.9 x slower: a ds_read_u16 at an ODD byte address costs 56 cycles per wave64 instruction against 1.9 at an even
// one, and a tap row starts at byte 3 ix; tools/ubench_lds_u16.hip, profiles/r06_ubench_lds_u16.txt.)
template <int PITCH = LDS_PITCH>
__device__ __forceinline__ void gather_blend_sums(const uint32_t (&bx)[4], const uint32_t (&by)[4], uint32_t lds_origin,
                                                  uint32_t (&oB)[4], uint32_t (&oG)[4], uint32_t (&oR)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
        TapRegs t0, t1;
        taps_pair<PITCH>(tap_address<PITCH>(bx[j], by[j], lds_origin), tap_address<PITCH>(bx[j + 1], by[j + 1], lds_origin), t0, t1);
        blend_pixel(bx[j], by[j], t0, oB[j], oG[j], oR[j]);
        blend_pixel(bx[j + 1], by[j + 1], t1, oB[j + 1], oG[j + 1], oR[j + 1]);
    }
}
template <int PITCH = LDS_PITCH>
__device__ __forceinline__ uint3 gather_blend_staged(const uint32_t (&bx)[4], const uint32_t (&by)[4], uint32_t lds_origin)
{
    uint32_t oB[4], oG[4], oR[4];
    gather_blend_sums<PITCH>(bx, by, lds_origin, oB, oG, oR);
    // the 12 result bytes sit in byte 2 of the 12 sums: 6 v_perm_b32 + 3 v_or_b32 gather them into B0 G0 R0 B1 | G1 R1 B2 G2 |
    // R2 B3 G3 R3
    const uint32_t pair = 0x0C0C0602u, pair_hi = 0x06020C0Cu;
    uint3 d;
    d.x = __builtin_amdgcn_perm(oB[1], oR[0], pair_hi) | __builtin_amdgcn_perm(oG[0], oB[0], pair);
    d.y = __builtin_amdgcn_perm(oG[2], oB[2], pair_hi) | __builtin_amdgcn_perm(oR[1], oG[1], pair);
    d.z = __builtin_amdgcn_perm(oR[3], oG[3], pair_hi) | __builtin_amdgcn_perm(oB[3], oR[2], pair);
    return d;
}

// ... whichever layout the footprint's window has (wave-uniform)
__device__ __forceinline__ uint3 gather_blend_window(bool compact, const uint32_t (&bx)[4], const uint32_t (&by)[4], uint32_t lds_origin)
{
    if (compact) return gather_blend_staged<MF_COMPACT_PITCH>(bx, by, lds_origin);
    return gather_blend_staged<LDS_PITCH>(bx, by, lds_origin);
}

// The 2 x 2 taps of the lane's four pixels straight from the frame (two unaligned 8-byte loads per pixel), for footprints without a
// staged window: a[j] = B0 G0 R0 B1 | G1 R1 . . of row iy (pixel ix, pixel ix+1), b[j] the same of row iy + 1.
__device__ __forceinline__ void gather_global(const uint32_t (&bx)[4], const uint32_t (&by)[4], const uint8_t* __restrict__ src, int W, uint2 (&a)[4], uint2 (&b)[4])
{
    const uint8_t* __restrict__ src1 = src + 3u * (uint32_t)W;   // row iy + 1
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // ix = sx >> 5 = bits[5..21] (0x4B400000 >> 5 has no low 17 bits), same for iy
        const uint32_t t = umad24(__builtin_amdgcn_ubfe(by[j], 5, 17), (uint32_t)W, __builtin_amdgcn_ubfe(bx[j], 5, 17));
        const uint32_t o = t + (t << 1);
        __builtin_memcpy(&a[j], src + o, 8);
        __builtin_memcpy(&b[j], src1 + o, 8);
    }
}

// cv2.remap's bilinear blend (integer, 1/32-pixel weights) of the lane's four pixels from gather_global's layout: the 12 output bytes
// B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3.
__device__ __forceinline__ uint3 blend(const uint32_t (&bx)[4], const uint32_t (&by)[4], const uint2 (&a)[4], const uint2 (&b)[4])
{
    uint3 d;
    uint32_t oB[4], oG[4], oR[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // a[j].x = B0 G0 R0 B1, a[j].y = G1 R1 . .   (pixel ix, pixel ix+1 of row iy; b: row iy+1)
        // per channel the two horizontal neighbours side by side in 16-bit fields: X0 | X1 << 16
        const uint32_t Ba = __builtin_amdgcn_perm(a[j].y, a[j].x, 0x0C030C00u), Bb = __builtin_amdgcn_perm(b[j].y, b[j].x, 0x0C030C00u);
        const uint32_t Ga = __builtin_amdgcn_perm(a[j].y, a[j].x, 0x0C040C01u), Gb = __builtin_amdgcn_perm(b[j].y, b[j].x, 0x0C040C01u);
        const uint32_t Ra = __builtin_amdgcn_perm(a[j].y, a[j].x, 0x0C050C02u), Rb = __builtin_amdgcn_perm(b[j].y, b[j].x, 0x0C050C02u);
        // vertical lerp of both fields at once (each <= 255 * 32: no carry between them)
        const uint32_t fy = by[j] & 31u, wy = 32u - fy;
        const uint32_t vB = umad24(Bb, fy, __umul24(Ba, wy));
        const uint32_t vG = umad24(Gb, fy, __umul24(Ga, wy));
        const uint32_t vR = umad24(Rb, fy, __umul24(Ra, wy));
        // horizontal lerp: v_dot2_u32_u16 with the weight pair (32 - fx, fx) scaled by 64, so that ((sum + 512) >> 10)
        // lands in byte 2:  (sum + 512) * 64 < 2^24
        const uint32_t fx = bx[j] & 31u;
        const uint32_t wq = umad24(fx, 0x3FFFC0u, 2048u);       // 64 (32 - fx) | 64 fx << 16
        oB[j] = udot2(vB, wq, 32768u);
        oG[j] = udot2(vG, wq, 32768u);
        oR[j] = udot2(vR, wq, 32768u);
    }
    // the 12 result bytes sit in byte 2 of the 12 sums: 6 v_perm_b32 + 3 v_or_b32 gather them into B0 G0 R0 B1 | G1 R1 B2 G2 |
    // R2 B3 G3 R3  (pair = byte 2 of `lo` then byte 2 of `hi` in the two low bytes, zeros above)
    const uint32_t pair = 0x0C0C0602u;
    const uint32_t pair_hi = 0x06020C0Cu;                         // the same pair in the two high bytes: v_or joins them
    d.x = __builtin_amdgcn_perm(oB[1], oR[0], pair_hi) | __builtin_amdgcn_perm(oG[0], oB[0], pair);
    d.y = __builtin_amdgcn_perm(oG[2], oB[2], pair_hi) | __builtin_amdgcn_perm(oR[1], oG[1], pair);
    d.z = __builtin_amdgcn_perm(oR[3], oG[3], pair_hi) | __builtin_amdgcn_perm(oB[3], oR[2], pair);
    return d;
}

}  // namespace mf
#endif  // MF_WARP_TAPS_U8C3_H
