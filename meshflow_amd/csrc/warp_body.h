// What the warp translation units share (warp.hip, warp_c1.hip, warp_c4.hip, warp_maps.hip): the constants, the coordinate, ownership
// and tap helpers, the per-format stores and footprint_body.  The design note is at the head of warp.hip.
#ifndef MF_WARP_BODY_H
#define MF_WARP_BODY_H
#include "mf_common.h"

#include <type_traits>

// At most 80 scalar registers: a CU admits min(8, 800 / (ceil(sgpr / 16) * 16 + 16)) workgroups of 256 threads
// (MI355X_MICROARCH.md), i.e. 7 with the 94 the compiler would take and 8 with 80 (the excess is kept in VGPR lanes, the kernel
// stays at 64 VGPRs): -1.7 % kernel time.
#define MF_WARP_ATTR __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(8, 8)))

namespace mf {

// The cell table is written by earlier kernels and only read here: pointers into it live in the constant address space, so
// that wave-uniform reads stay scalar loads (s_load) whatever else the kernel does (the global->LDS copies count as memory
// writes for the compiler, which otherwise turns later record reads into per-lane vector loads and spends 40 VGPRs on them).
typedef const __attribute__((address_space(4))) double* crec_t;
typedef const __attribute__((address_space(4))) float* cedge_t;

// Workgroup = ONE wavefront (its tile = its 32 x 8 footprint).  Wavefronts never cooperate (no barrier, no shared LDS data), and
// a multi-wave workgroup keeps the slots of its finished wavefronts until the slowest one -- often on a slower ownership
// path -- is done: 4 x 1 wavefronts 1.516 ms (cfg2) / 3.410 (cfg3), 2 x 1: 1.505 / 3.392, 1 x 1: 1.492 / 3.326; 4 x 2 and 4 x 4
// (fewer dispatches) 1.65 / 1.89.
// (Round 5, at the final kernels -- the launch rate is per WORKGROUP, an empty kernel of 4-wave workgroups launches 4 x as many
// wavefronts per ns, tools/ubench_launch.hip -- 2 / 4 wavefronts per workgroup again: config 2 +3.6 / +4.1 %, config 3 +4.7 / +4.3 %,
// 4K +3.4 / +4.1 %, an all-hot footprint stream +-0: the dispatcher is not what the kernel waits for.)
// More than one footprint per wavefront (a vertical stack, or a run along x with the next footprint's plan and window prefetched
// into a second LDS buffer behind counted vmcnt waits) is slower as well: 2 per wavefront +4 %, 4 per wavefront +9 %.
// (Round 5: a wavefront that takes the hot footprint BELOW its own as well when both have the same owner -- one plan round trip, one
// matrix, two windows, two batches of pixels, everything else through the regular code one footprint after the other; zero scratch,
// byte-identical -- all-hot stream -0.7 %, 4K -0.2 %, config 2 +2.4 %, config 3 +5.2 %: what a wavefront does once per footprint is
// not what bounds the kernel.  DESIGN.md section 4.3.)
constexpr int FOOT_W = MF_FOOT_W;   // 8 lanes x 4 pixels
constexpr int FOOT_H = MF_FOOT_H;   // 64 lanes / 8
constexpr int MAX_MESH = 64;    // R, C <= 64
// The float32 edge functions are stored scaled by their own evaluation error bound (cell_table.hip): beyond +-1 their sign is the
// exact function's sign; inside the band the float64 comparison decides.
constexpr float EDGE_BAND = 1.0f;
// A pixel's owner is kept as the byte offset of the owner's row in the wavefront's s_hi block (80-byte rows, one per list
// entry).  Row 8 holds the matrix {0, 0, W+1; 0, 0, H+1; 0, 0, 1}: a pixel no cell covers runs through the same arithmetic and
// comes out at exactly (W+1, H+1) (mfs.py:983-984) -- no special case, no select, in the coordinate code.
constexpr uint32_t OWN_ROW = 80, OWN_NONE = 8 * OWN_ROW;
constexpr int LDS_PITCH = MF_STAGE_PITCH;
constexpr int LDS_WINDOW_BYTES = MF_STAGE_CHUNKS * 16;
// In front of the window: room for the LDS row of frame row -1 (and the pixel of column -1 in front of it) that the border path paints
// in the border colour; the row of frame row H lands behind row 11, inside the window's own bytes.
constexpr int LDS_WINDOW_PAD = 176;

// LDS pointer of a __shared__ object WITHOUT the generic -> LDS conversion (which comes with a null check: s_mov src_shared_base + s_cmp +
// s_cselect, three scalar instructions per global->LDS copy, and the scalar unit is as loaded as the vector unit here): the low
// 32 bits of a generic address into LDS are the LDS address.
typedef __attribute__((address_space(3))) uint8_t* lds_bytes_t;
__device__ __forceinline__ lds_bytes_t lds_ptr(const void* shared_object)
{
    return (lds_bytes_t)(uintptr_t)(uint32_t)(uintptr_t)shared_object;
}

// a * b + c on the 24-bit multiplier.  The empty asm makes `c` opaque so that the compiler keeps two chained
// v_mad_u32_u24 instead of re-associating them into mul + mul + add3 (no instruction is emitted by it, so the
// compiler still pads every hazard itself).
__device__ __forceinline__ uint32_t umad24(uint32_t a, uint32_t b, uint32_t c)
{
    asm("" : "+v"(c));
    return __umul24(a, b) + c;
}

// min(a, b, c) in ONE instruction (the compiler re-associates a chain of min() into more v_min_u32 than needed)
__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// bits [5..28] of the raw float 32u + 1.5*2^23 are (sx >> 5) + MAGIC_HI for 0 <= sx < 2^22
constexpr uint32_t MAGIC_HI = (0x4B400000u >> 5) & 0xFFFFFFu;

// a.lo * b.lo + a.hi * b.hi + c on 16-bit halves (v_dot2_u32_u16)
__device__ __forceinline__ uint32_t udot2(uint32_t a, uint32_t b, uint32_t c)
{
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_udot2(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b), c, false);
}

__device__ __forceinline__ int cv_round_f32(float v)
{
    const float r = rintf(v);
    return (r >= -2147483648.0f && r < 2147483648.0f) ? (int)r : (int)0x80000000;
}

// OpenCV's mask test, exactly (imgwarp.cpp WarpPerspectiveInvoker: 64-wide destination blocks).
// (OpenCV's block is min(1024 / min(16, H), W) pixels wide: 64 for every frame of 16 rows or more -- or narrower than 64 pixels, which
// is one block either way.  A frame under 16 rows tall AND over 64 pixels wide would get wider blocks, i.e. one rounding of x-dependent
// terms placed differently: visible only on an exact rounding tie at a mask edge.  Not modelled -- here, in oracle/warp_oracle.c and in
// oracle/meshflow_oracle.py alike; tests/test_cv2_crosscheck.py is where a real OpenCV would show it.)
__device__ __forceinline__ bool mask_test_exact(const double* __restrict__ M, int lo_x, int hi_x, int lo_y, int hi_y,
                                             int x, int y)
{
    const double xb = (double)(x & ~63), x1 = (double)(x & 63), yy = (double)y;
    const double X0 = (M[0] * xb + M[1] * yy) + M[2];
    const double Y0 = (M[3] * xb + M[4] * yy) + M[5];
    const double W0 = (M[6] * xb + M[7] * yy) + M[8];
    const double Wd = W0 + M[6] * x1;
    const double Ws = Wd != 0.0 ? 32.0 / Wd : 0.0;
    const double fX = fmax(-2147483648.0, fmin(2147483647.0, (X0 + M[0] * x1) * Ws));
    const double fY = fmax(-2147483648.0, fmin(2147483647.0, (Y0 + M[3] * x1) * Ws));
    const int X = (int)rint(fX);
    const int Y = (int)rint(fY);
    // non-zero bilinear sample of the 255-filled rect <=> a tap with non-zero weight lies on it
    return X > lo_x && X < hi_x && Y > lo_y && Y < hi_y;
}

// 1/w with the exact bits of IEEE division for 0.5 <= |w| <= 2: the compiler's own f64 division sequence
// (v_div_scale / v_rcp / 2 Newton steps / residual / v_div_fmas / v_div_fixup) without the scaling and
// special-case steps, which are the identity in that range.  tests/test_gpu_parity.py checks it against
// 1.0 / w on random inputs (mf_selftest_recip).
__device__ __forceinline__ double recip_unit_range(double w)
{
    double r = __builtin_amdgcn_rcp(w);
    double e = __builtin_fma(-w, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-w, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-w, r, 1.0);
    return __builtin_fma(e, r, r);
}

// 1/w for the lane's pixels 1..3 WITHOUT v_rcp_f64 (16 issue cycles) and with one Newton step less: the denominators of
// consecutive pixels differ by h6 (w_j = w_0 + j h6 up to rounding), so with r0 = 1/w_0
//     1/w_j = r0 (1 - e + e^2 - ...),  e = j h6 r0,
// and the second-order guess g = r0 - j c1 + j^2 c2 (c1 = h6 r0^2, c2 = h6^2 r0^3) is within e^3 (1 + e) of 1/w_j.  One Newton
// step squares that; the residual-correction step of recip_unit_range then delivers the correctly rounded quotient exactly as
// it does there, where its input is also an approximation good to about one ulp.  The caller guarantees |c1| <= 2.5e-4, i.e.
// e <= 3 |c1| / |r0| <= 1.5e-3 (|r0| > 1/2), so the Newton step leaves a relative error below (1.002 * 3.4e-9)^2 < 2^-56.
// mf_selftest_recip checks it against IEEE division on hashed (w_0, h6, j).
constexpr double RECIP_GUESS_LIMIT = 2.5e-4;
__device__ __forceinline__ double recip_guess(double r0, double c1, double c2, double j)
{
    return __builtin_fma(j * j, c2, __builtin_fma(-j, c1, r0));
}
__device__ __forceinline__ double recip_from_guess(double w, double g)
{
    double e = __builtin_fma(-w, g, 1.0);
    g = __builtin_fma(g, e, g);
    e = __builtin_fma(-w, g, 1.0);
    return __builtin_fma(e, g, g);
}

// Source coordinates of the lane's four pixels under cell `rec`'s inverse homography:
// cv2.perspectiveTransform (matmul.simd.hpp) -- float32 point, float64 matrix, float32 result.
// SELECT = false: every pixel takes the new coordinates; true: only those in `pass`.
// `certified` (wave-uniform): the plan has checked on the footprint's corners that the denominator stays inside (0.52, 1.9) and
// that the reciprocal guess applies (MF_PLAN_UNIT) -- both tests are then skipped.
template <bool SELECT>
__device__ __forceinline__ void cell_coords(crec_t rec, double xs0, double yy, int x0, uint32_t pass,
                                            float (&u)[4], float (&v)[4], bool certified = false)
{
    (void)x0;
    double Hi[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Hi[i] = rec[MF_CELL_OFF_HI + i];
    const double t6 = yy * Hi[7], t0 = yy * Hi[1], t3 = yy * Hi[4];
    double w4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w4[j] = ((xs0 + (double)j) * Hi[6] + t6) + Hi[8];     // (xs0 + j is exact: small integers)
    // pixel 0: full reciprocal; pixels 1..3 start from it (recip_guess).  A cell whose denominator leaves [0.5, 2) or
    // changes too fast along x for the guess (strong perspective: |h6| / w^2 > 2.5e-4 per pixel) takes the generic division.
    bool fast_ok = certified;
    if (!certified) {
        uint32_t eor = 0;                                      // |w| in [0.5, 2) <=> frexp exponent in {0, 1}
#pragma unroll
        for (int j = 0; j < 4; ++j) eor |= (uint32_t)__builtin_amdgcn_frexp_exp(w4[j]);
        // (the test |h6| <= limit * w0^2 is the same condition as |c1| <= limit without waiting for the reciprocal)
        const bool guess_ok = fabs(Hi[6]) <= (0.96 * RECIP_GUESS_LIMIT) * (w4[0] * w4[0]);
        fast_ok = __ballot(eor > 1u || !guess_ok) == 0;
    }
    if (fast_ok) {
        const double iw0 = recip_unit_range(w4[0]);
        const double c1 = Hi[6] * (iw0 * iw0), c2 = (Hi[6] * c1) * iw0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double xs = xs0 + (double)j;
            const double iw = j == 0 ? iw0 : recip_from_guess(w4[j], recip_guess(iw0, c1, c2, (double)j));
            const float un = (float)(((xs * Hi[0] + t0) + Hi[2]) * iw);
            const float vn = (float)(((xs * Hi[3] + t3) + Hi[5]) * iw);
            if (SELECT) {
                const bool p = (pass >> j) & 1u;
                u[j] = p ? un : u[j];
                v[j] = p ? vn : v[j];
            } else {
                u[j] = un;
                v[j] = vn;
            }
        }
    } else {                                                   // far-from-affine cell: generic division
        // (unrolled: a rolled loop indexes u[] / v[] by select chains, and their initial values -- eight moves -- are then
        // hoisted in front of the branch, onto the fast path)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double xs = xs0 + (double)j;
            const double w = w4[j];
            const bool ok = fabs(w) > 1.1920928955078125e-07;
            const double iw = 1.0 / w;
            const float un = ok ? (float)(((xs * Hi[0] + t0) + Hi[2]) * iw) : 0.0f;
            const float vn = ok ? (float)(((xs * Hi[3] + t3) + Hi[5]) * iw) : 0.0f;
            const bool p = !SELECT || ((pass >> j) & 1u);
            u[j] = p ? un : u[j];
            v[j] = p ? vn : v[j];
        }
    }
}

// FAST COORDINATES.  cv2.perspectiveTransform's float64 chain -- (x h0 + y h1) + h2 with every product and sum rounded, the
// correctly rounded 1 / w, the rounded product -- only matters through its float32 conversion.  A cheaper float64 chain (fused
// affine forms, ONE reciprocal of the lane's four denominators refined by ONE Newton step) lands within 118 float64 ulps of the exact
// chain's value (bound: DESIGN.md section 4.3, certified per footprint by the plan: MF_PLAN_FAST64; mf_selftest_fast64_margin measures
// the distance), so both convert to the SAME float32 unless the cheap value lies within that distance of a float32 rounding midpoint,
// i.e. unless the low 29 mantissa bits are within FAST64_WINDOW (4.3 x the bound) of 0x10000000.
// midpoint_key() is below FAST64_NEAR exactly then (one v_lshl_add_u32 on the low dword); a wavefront with any such value redoes its
// coordinates with the exact chain (about one wavefront in 1,000 at config-2 geometry).
constexpr uint32_t FAST64_WINDOW = 512u;
// (low dword << 3) + const: the 29 dropped mantissa bits, shifted to the top of the register and offset so that the window around the
// midpoint pattern 0x10000000 maps to [0, 16 FAST64_WINDOW) -- ONE v_lshl_add_u32 per value; the smallest key of a lane decides.
constexpr uint32_t FAST64_NEAR = 16u * FAST64_WINDOW;
__device__ __forceinline__ uint32_t midpoint_key(double a)
{
    return ((uint32_t)__double_as_longlong(a) << 3) + ((0x10000000u + FAST64_WINDOW) << 3);
}

// Quotients n_j / w_j and m_j / w_j of a lane's four pixels on the cheap chain, whatever matrices the forms came from: ONE reciprocal
// for the four denominators -- R = 1 / (w0 w1 w2 w3) by v_rcp_f64 + ONE Newton step (0.07 < product < 13.1), then 1 / w0 = (R w2 w3) w1
// and so on: nine multiplications; the rounding errors of the w_j themselves cancel (the same values sit in the product), what remains
// is 5 roundings per reciprocal plus what the Newton step leaves: v_rcp_f64 is good to 2^-24.36 (tools/ubench_semantics.hip: 2^26
// evenly spaced mantissas x 8 exponents, profiles/r06_ubench_semantics.txt), one step squares that: 2^-48.7 = 20 u (u = 2^-53) -- a
// second step (rounds 5-6a) took it to 1 u for two more float64 instructions per lane.  Returns the smallest midpoint key of the eight values.
__device__ __forceinline__ uint32_t cheap_quotients(const double (&w)[4], const double (&n)[4], const double (&m)[4], float (&u)[4], float (&v)[4],
                                                    uint32_t* keys = nullptr, double* raw = nullptr)
{
    const double q01 = w[0] * w[1], q23 = w[2] * w[3], pr = q01 * q23;
    double r = __builtin_amdgcn_rcp(pr);
    double e = __builtin_fma(-pr, r, 1.0);
    r = __builtin_fma(r, e, r);
    const double ra = r * q23, rb = r * q01;
    const double g[4] = { ra * w[1], ra * w[0], rb * w[3], rb * w[2] };
    uint32_t key = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double a = n[j] * g[j], b = m[j] * g[j];
        u[j] = (float)a;
        v[j] = (float)b;
        key = j == 0 ? min(midpoint_key(a), midpoint_key(b)) : umin3(key, midpoint_key(a), midpoint_key(b));
        if (keys) { keys[2 * j] = midpoint_key(a); keys[2 * j + 1] = midpoint_key(b); }
        if (raw) { raw[2 * j] = a; raw[2 * j + 1] = b; }
    }
    return key;
}

// The cheap chain for a lane whose four pixels step along x (VERT = false: (x0 + j, y0)) or along y (VERT: (x0, y0 + j), the
// transposed lane mapping of the pair path); returns the smallest midpoint key (< FAST64_NEAR = some value too close to a float32 midpoint).
// `keys` (self-test only): the eight midpoint keys, u then v per pixel.
template <bool VERT>
__device__ __forceinline__ uint32_t coords_fast_dir(const double (&Hi)[9], double xs0, double yy0, float (&u)[4], float (&v)[4], uint32_t* keys = nullptr,
                                                    double* raw = nullptr)
{
    const double t0 = VERT ? yy0 : xs0, o = VERT ? xs0 : yy0;                        // stepping coordinate, the other one
    const double a0 = Hi[VERT ? 1 : 0], a3 = Hi[VERT ? 4 : 3], a6 = Hi[VERT ? 7 : 6];   // coefficients of the stepping coordinate
    const double c0 = __builtin_fma(o, Hi[VERT ? 0 : 1], Hi[2]), c3 = __builtin_fma(o, Hi[VERT ? 3 : 4], Hi[5]), c6 = __builtin_fma(o, Hi[VERT ? 6 : 7], Hi[8]);
    // the affine forms at the lane's first pixel, then + j a (j = 1, 2, 3 are exact constants): one fma per pixel and form
    double w[4], n[4], m[4];
    w[0] = __builtin_fma(t0, a6, c6); n[0] = __builtin_fma(t0, a0, c0); m[0] = __builtin_fma(t0, a3, c3);
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        w[j] = __builtin_fma((double)j, a6, w[0]);
        n[j] = __builtin_fma((double)j, a0, n[0]);
        m[j] = __builtin_fma((double)j, a3, m[0]);
    }
    return cheap_quotients(w, n, m, u, v, keys, raw);
}
// The hot path's coordinates by the cheap chain; false (wave-uniform) when some value is too close to a float32 midpoint.
__device__ __forceinline__ bool coords_fast(const double (&Hi)[9], double xs0, double yy, float (&u)[4], float (&v)[4], uint32_t* keys = nullptr)
{
    return __ballot(coords_fast_dir<false>(Hi, xs0, yy, u, v, keys) < FAST64_NEAR) == 0;
}
__device__ __forceinline__ bool cell_coords_fast(crec_t rec, double xs0, double yy, float (&u)[4], float (&v)[4])
{
    double Hi[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Hi[i] = rec[MF_CELL_OFF_HI + i];
    return coords_fast(Hi, xs0, yy, u, v);
}

// Per-pixel mask test of a MIXED cell for the lane's four pixels; returns the 4-bit pass mask.
// Division-free decision: with Xn = M0 x + M1 y + M2 and Wd = M6 x + M7 y + M8 > 0, OpenCV's
// fX = fl(Xn * fl(32/Wd)) differs from 32 Xn / Wd by < 1e-9 relative, and rint(fX) > lo <=> fX > lo + 1/2
// (lo is even).  So the sign of q = 32 Xn - (lo + 1/2) Wd (and its three siblings) decides the test unless
// |q| <= 1e-6 Wd; only then is the exact arithmetic (division, rint) needed.
__device__ __forceinline__ uint32_t cell_mask_test(crec_t rec, double xs0, double yy, int x0, int y,
                                                   uint32_t unowned)
{
    double M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = rec[MF_CELL_OFF_M + i];
    const double rL = rec[MF_CELL_OFF_RECT + 0], rT = rec[MF_CELL_OFF_RECT + 1];
    const double rR = rec[MF_CELL_OFF_RECT + 2], rB = rec[MF_CELL_OFF_RECT + 3];
    const double loxh = 32.0 * (rL - 1.0) + 0.5, hixh = 32.0 * (rR + 1.0) - 0.5;
    const double loyh = 32.0 * (rT - 1.0) + 0.5, hiyh = 32.0 * (rB + 1.0) - 0.5;
    const double RX = __builtin_fma(M[1], yy, M[2]);
    const double RY = __builtin_fma(M[4], yy, M[5]);
    const double RW = __builtin_fma(M[7], yy, M[8]);
    uint32_t ok = 0, amb = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double xs = xs0 + (double)j;
        const double Wd = __builtin_fma(M[6], xs, RW);
        const double X32 = 32.0 * __builtin_fma(M[0], xs, RX);
        const double Y32 = 32.0 * __builtin_fma(M[3], xs, RY);
        const double qmin = fmin(fmin(__builtin_fma(-loxh, Wd, X32), __builtin_fma(hixh, Wd, -X32)),
                                 fmin(__builtin_fma(-loyh, Wd, Y32), __builtin_fma(hiyh, Wd, -Y32)));
        const double t = 1e-6 * Wd;
        const bool sane = (Wd > 0.25) & (Wd < 4.0);
        const bool yes = sane & (qmin > t), no = sane & (qmin < -t);
        ok |= yes ? (1u << j) : 0u;
        amb |= (yes | no) ? 0u : (1u << j);
    }
    amb &= unowned;
    if (__ballot(amb != 0) != 0) {                             // rare: a pixel within 1e-6 of a mask edge
        const int lo_x = 32 * ((int)rL - 1), hi_x = 32 * ((int)rR + 1);
        const int lo_y = 32 * ((int)rT - 1), hi_y = 32 * ((int)rB + 1);
#pragma unroll 1
        for (int j = 0; j < 4; ++j)
            if (((amb >> j) & 1u) && mask_test_exact(M, lo_x, hi_x, lo_y, hi_y, x0 + j, y)) ok |= 1u << j;
    }
    return ok & unowned;
}

// cv2.remap's fixed point: sx = rint(32 u) by the 1.5*2^23 trick -- the fma rounds 32u + magic once, to nearest even, and the integer
// sits in the low mantissa bits (valid for |32u| < 2^22; anything else lands far outside the "deep interior" window and is redone
// exactly by the generic path).  Raw float bits of 32u + 1.5*2^23: the low 22 bits hold sx for 0 <= sx < 2^22.
__device__ __forceinline__ void fixed_point(const float (&u)[4], const float (&v)[4], uint32_t (&bx)[4], uint32_t (&by)[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bx[j] = __float_as_uint(__builtin_fmaf(u[j], 32.0f, 12582912.0f));
        by[j] = __float_as_uint(__builtin_fmaf(v[j], 32.0f, 12582912.0f));
    }
}

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
    const int lane = threadIdx.x;
    uint32_t bx[4], by[4];
    fixed_point(u, v, bx, by);
    uint32_t dxm = 0, dym = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dxm = max(dxm, bx[j] - (0x4B400000u + 64u));
        dym = max(dym, by[j] - (0x4B400000u + 64u));
    }
    // deep interior (as in footprint_body): 2 <= ix <= W-3 and 2 <= iy <= H-3 for all four pixels
    const bool deep = W >= 5 && H >= 5 && dxm <= (uint32_t)(32 * (W - 3) + 31 - 64) && dym <= (uint32_t)(32 * (H - 3) + 31 - 64);
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
            uint32_t spread = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                spread = max(spread, max(bx[j] - (0x4B400000u - 0x200000u), by[j] - (0x4B400000u - 0x200000u)));
            const bool narrow = __ballot(spread >= 0x400000u) == 0;
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
                const int sxx = narrow ? (int)(bx[j] - 0x4B400000u) : cv_round_f32(uu * 32.0f);
                const int syy = narrow ? (int)(by[j] - 0x4B400000u) : cv_round_f32(vv * 32.0f);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                if (ix >= W || ix + 1 < 0 || iy >= H || iy + 1 < 0) {  // the 2 x 2 footprint lies wholly outside: cval
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[j][c] = cval[c];
                    continue;
                }
                const bool in_x0 = (unsigned)ix < (unsigned)W, in_x1 = (unsigned)(ix + 1) < (unsigned)W;
                const bool in_y0 = (unsigned)iy < (unsigned)H, in_y1 = (unsigned)(iy + 1) < (unsigned)H;
                const uint32_t cx0 = (uint32_t)min(max(ix, 0), W - 1), cx1 = (uint32_t)min(max(ix + 1, 0), W - 1);
                const uint32_t r0 = (uint32_t)min(max(iy, 0), H - 1) * (uint32_t)W, r1 = (uint32_t)min(max(iy + 1, 0), H - 1) * (uint32_t)W;
                const uint16_t* __restrict__ q00 = src + 3ull * (uint64_t)(r0 + cx0);
                const uint16_t* __restrict__ q01 = src + 3ull * (uint64_t)(r0 + cx1);
                const uint16_t* __restrict__ q10 = src + 3ull * (uint64_t)(r1 + cx0);
                const uint16_t* __restrict__ q11 = src + 3ull * (uint64_t)(r1 + cx1);
                const float ax = (float)(sxx & 31) * 0.03125f, ay = (float)(syy & 31) * 0.03125f;
                const float ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                const float w0 = ay0 * ax0, w1 = ay0 * ax, w2 = ay * ax0, w3 = ay * ax;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t s00 = in_x0 && in_y0 ? (uint32_t)q00[c] : cval[c], s01 = in_x1 && in_y0 ? (uint32_t)q01[c] : cval[c];
                    const uint32_t s10 = in_x0 && in_y1 ? (uint32_t)q10[c] : cval[c], s11 = in_x1 && in_y1 ? (uint32_t)q11[c] : cval[c];
                    o[j][c] = blend16((float)s00, (float)s01, (float)s10, (float)s11, w0, w1, w2, w3);
                }
            }
        }
    }
    if (!fast) {
        // crop bounds: wave reduction, then at most one atomic per bound and wavefront (per frame, mfs.py:1075-1098, and the clip-level
        // rectangle, mfs.py:1103-1106)
        const bool any = c_left != 0 || c_top != 0 || c_right != W - 1 || c_bottom != H - 1;
        if (__ballot(any) != 0) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                c_left = max(c_left, __shfl_xor(c_left, off));
                c_top = max(c_top, __shfl_xor(c_top, off));
                c_right = min(c_right, __shfl_xor(c_right, off));
                c_bottom = min(c_bottom, __shfl_xor(c_bottom, off));
            }
            if (lane == 0) {
                if (c_left != 0) { atomicMax(&crop[4 * f + 0], c_left); atomicMax(&clip[0], c_left); }
                if (c_top != 0) { atomicMax(&crop[4 * f + 1], c_top); atomicMax(&clip[1], c_top); }
                if (c_right != W - 1) { atomicMin(&crop[4 * f + 2], c_right); atomicMin(&clip[2], c_right); }
                if (c_bottom != H - 1) { atomicMin(&crop[4 * f + 3], c_bottom); atomicMin(&clip[3], c_bottom); }
            }
        }
    }
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
    const int lane = threadIdx.x;
    uint32_t bx[4], by[4];
    fixed_point(u, v, bx, by);
    uint32_t dxm = 0, dym = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dxm = max(dxm, bx[j] - (0x4B400000u + 64u));
        dym = max(dym, by[j] - (0x4B400000u + 64u));
    }
    // deep interior (as in footprint_body): 2 <= ix <= W-3 and 2 <= iy <= H-3 for all four pixels
    const bool deep = W >= 5 && H >= 5 && dxm <= (uint32_t)(32 * (W - 3) + 31 - 64) && dym <= (uint32_t)(32 * (H - 3) + 31 - 64);
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
            uint32_t spread = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                spread = max(spread, max(bx[j] - (0x4B400000u - 0x200000u), by[j] - (0x4B400000u - 0x200000u)));
            const bool narrow = __ballot(spread >= 0x400000u) == 0;
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
                const int sxx = narrow ? (int)(bx[j] - 0x4B400000u) : cv_round_f32(uu * 32.0f);
                const int syy = narrow ? (int)(by[j] - 0x4B400000u) : cv_round_f32(vv * 32.0f);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                // (a 2 x 2 footprint wholly outside needs no special case: four border taps with weights summing to 1024 give the border)
                const bool in_x0 = (unsigned)ix < (unsigned)W, in_x1 = (unsigned)(ix + 1) < (unsigned)W;
                const bool in_y0 = (unsigned)iy < (unsigned)H, in_y1 = (unsigned)(iy + 1) < (unsigned)H;
                const uint32_t cx0 = (uint32_t)min(max(ix, 0), W - 1), cx1 = (uint32_t)min(max(ix + 1, 0), W - 1);
                const uint32_t r0 = (uint32_t)min(max(iy, 0), H - 1) * (uint32_t)W, r1 = (uint32_t)min(max(iy + 1, 0), H - 1) * (uint32_t)W;
                const uint32_t s00 = src[r0 + cx0], s01 = src[r0 + cx1], s10 = src[r1 + cx0], s11 = src[r1 + cx1];
                o[j] = blend_c1(in_x0 && in_y0 ? s00 : border, in_x1 && in_y0 ? s01 : border, in_x0 && in_y1 ? s10 : border,
                                in_x1 && in_y1 ? s11 : border, (uint32_t)sxx, (uint32_t)syy);
            }
        }
    }
    if (!fast) {
        // crop bounds: wave reduction, then at most one atomic per bound and wavefront (per frame, mfs.py:1075-1098, and the clip-level
        // rectangle, mfs.py:1103-1106)
        const bool any = c_left != 0 || c_top != 0 || c_right != W - 1 || c_bottom != H - 1;
        if (__ballot(any) != 0) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                c_left = max(c_left, __shfl_xor(c_left, off));
                c_top = max(c_top, __shfl_xor(c_top, off));
                c_right = min(c_right, __shfl_xor(c_right, off));
                c_bottom = min(c_bottom, __shfl_xor(c_bottom, off));
            }
            if (lane == 0) {
                if (c_left != 0) { atomicMax(&crop[4 * f + 0], c_left); atomicMax(&clip[0], c_left); }
                if (c_top != 0) { atomicMax(&crop[4 * f + 1], c_top); atomicMax(&clip[1], c_top); }
                if (c_right != W - 1) { atomicMin(&crop[4 * f + 2], c_right); atomicMin(&clip[2], c_right); }
                if (c_bottom != H - 1) { atomicMin(&crop[4 * f + 3], c_bottom); atomicMin(&clip[3], c_bottom); }
            }
        }
    }
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
    const int lane = threadIdx.x;
    uint32_t bx[4], by[4];
    fixed_point(u, v, bx, by);
    uint32_t dxm = 0, dym = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dxm = max(dxm, bx[j] - (0x4B400000u + 64u));
        dym = max(dym, by[j] - (0x4B400000u + 64u));
    }
    // deep interior (as in footprint_body): 2 <= ix <= W-3 and 2 <= iy <= H-3 for all four pixels
    const bool deep = W >= 5 && H >= 5 && dxm <= (uint32_t)(32 * (W - 3) + 31 - 64) && dym <= (uint32_t)(32 * (H - 3) + 31 - 64);
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
            uint32_t spread = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                spread = max(spread, max(bx[j] - (0x4B400000u - 0x200000u), by[j] - (0x4B400000u - 0x200000u)));
            const bool narrow = __ballot(spread >= 0x400000u) == 0;
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
                const int sxx = narrow ? (int)(bx[j] - 0x4B400000u) : cv_round_f32(uu * 32.0f);
                const int syy = narrow ? (int)(by[j] - 0x4B400000u) : cv_round_f32(vv * 32.0f);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                // (a 2 x 2 footprint wholly outside needs no special case: four border taps with weights summing to 1024 give the border)
                const bool in_x0 = (unsigned)ix < (unsigned)W, in_x1 = (unsigned)(ix + 1) < (unsigned)W;
                const bool in_y0 = (unsigned)iy < (unsigned)H, in_y1 = (unsigned)(iy + 1) < (unsigned)H;
                const uint32_t cx0 = (uint32_t)min(max(ix, 0), W - 1), cx1 = (uint32_t)min(max(ix + 1, 0), W - 1);
                const uint32_t r0 = (uint32_t)min(max(iy, 0), H - 1) * (uint32_t)W, r1 = (uint32_t)min(max(iy + 1, 0), H - 1) * (uint32_t)W;
                uint32_t p00, p01, p10, p11;
                __builtin_memcpy(&p00, src + 4ull * (r0 + cx0), 4);
                __builtin_memcpy(&p01, src + 4ull * (r0 + cx1), 4);
                __builtin_memcpy(&p10, src + 4ull * (r1 + cx0), 4);
                __builtin_memcpy(&p11, src + 4ull * (r1 + cx1), 4);
                o[j] = blend_c4(in_x0 && in_y0 ? p00 : border, in_x1 && in_y0 ? p01 : border, in_x0 && in_y1 ? p10 : border,
                                in_x1 && in_y1 ? p11 : border, (uint32_t)sxx, (uint32_t)syy);
            }
        }
    }
    if (!fast) {
        // crop bounds: wave reduction, then at most one atomic per bound and wavefront (per frame, mfs.py:1075-1098, and the clip-level
        // rectangle, mfs.py:1103-1106)
        const bool any = c_left != 0 || c_top != 0 || c_right != W - 1 || c_bottom != H - 1;
        if (__ballot(any) != 0) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                c_left = max(c_left, __shfl_xor(c_left, off));
                c_top = max(c_top, __shfl_xor(c_top, off));
                c_right = min(c_right, __shfl_xor(c_right, off));
                c_bottom = min(c_bottom, __shfl_xor(c_bottom, off));
            }
            if (lane == 0) {
                if (c_left != 0) { atomicMax(&crop[4 * f + 0], c_left); atomicMax(&clip[0], c_left); }
                if (c_top != 0) { atomicMax(&crop[4 * f + 1], c_top); atomicMax(&clip[1], c_top); }
                if (c_right != W - 1) { atomicMin(&crop[4 * f + 2], c_right); atomicMin(&clip[2], c_right); }
                if (c_bottom != H - 1) { atomicMin(&crop[4 * f + 3], c_bottom); atomicMin(&clip[3], c_bottom); }
            }
        }
    }
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
// Crop bounds of a tail that scans every pixel itself: wave reduction, then at most one atomic per bound and wavefront (per frame,
// mfs.py:1075-1098, and the clip-level rectangle, mfs.py:1103-1106) -- remap_store_u16's fold.
__device__ __forceinline__ void plane_crop_fold(int c_left, int c_top, int c_right, int c_bottom, uint32_t f, int W, int H,
                                                int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const bool any = c_left != 0 || c_top != 0 || c_right != W - 1 || c_bottom != H - 1;
    if (__ballot(any) == 0) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        c_left = max(c_left, __shfl_xor(c_left, off));
        c_top = max(c_top, __shfl_xor(c_top, off));
        c_right = min(c_right, __shfl_xor(c_right, off));
        c_bottom = min(c_bottom, __shfl_xor(c_bottom, off));
    }
    if (threadIdx.x == 0) {
        if (c_left != 0) { atomicMax(&crop[4 * f + 0], c_left); atomicMax(&clip[0], c_left); }
        if (c_top != 0) { atomicMax(&crop[4 * f + 1], c_top); atomicMax(&clip[1], c_top); }
        if (c_right != W - 1) { atomicMin(&crop[4 * f + 2], c_right); atomicMin(&clip[2], c_right); }
        if (c_bottom != H - 1) { atomicMin(&crop[4 * f + 3], c_bottom); atomicMin(&clip[3], c_bottom); }
    }
}

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
    uint32_t dxm = 0, dym = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dxm = max(dxm, bx[j] - (0x4B400000u + 64u));
        dym = max(dym, by[j] - (0x4B400000u + 64u));
    }
    // deep interior (as in footprint_body): 2 <= ix <= W-3 and 2 <= iy <= H-3 for all four pixels
    const bool deep = W >= 5 && H >= 5 && dxm <= (uint32_t)(32 * (W - 3) + 31 - 64) && dym <= (uint32_t)(32 * (H - 3) + 31 - 64);
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
            uint32_t spread = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                spread = max(spread, max(bx[j] - (0x4B400000u - 0x200000u), by[j] - (0x4B400000u - 0x200000u)));
            const bool narrow = __ballot(spread >= 0x400000u) == 0;
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
                const int sxx = narrow ? (int)(bx[j] - 0x4B400000u) : cv_round_f32(uu * 32.0f);
                const int syy = narrow ? (int)(by[j] - 0x4B400000u) : cv_round_f32(vv * 32.0f);
                const int ix = sxx >> 5, iy = syy >> 5;                 // (saturation to int16 cannot change any decision below)
                if (ix >= W || ix + 1 < 0 || iy >= H || iy + 1 < 0) continue;       // the 2 x 2 footprint lies wholly outside: fill
                const bool in_x0 = (unsigned)ix < (unsigned)W, in_x1 = (unsigned)(ix + 1) < (unsigned)W;
                const bool in_y0 = (unsigned)iy < (unsigned)H, in_y1 = (unsigned)(iy + 1) < (unsigned)H;
                const uint32_t cx0 = (uint32_t)min(max(ix, 0), W - 1), cx1 = (uint32_t)min(max(ix + 1, 0), W - 1);
                const uint32_t r0 = (uint32_t)min(max(iy, 0), H - 1) * (uint32_t)W, r1 = (uint32_t)min(max(iy + 1, 0), H - 1) * (uint32_t)W;
                const float q00 = src[(uint64_t)(r0 + cx0)], q01 = src[(uint64_t)(r0 + cx1)];
                const float q10 = src[(uint64_t)(r1 + cx0)], q11 = src[(uint64_t)(r1 + cx1)];
                const float s00 = in_x0 && in_y0 ? q00 : fill, s01 = in_x1 && in_y0 ? q01 : fill;
                const float s10 = in_x0 && in_y1 ? q10 : fill, s11 = in_x1 && in_y1 ? q11 : fill;
                const float ax = (float)(sxx & 31) * 0.03125f, ay = (float)(syy & 31) * 0.03125f;
                const float ax0 = 1.0f - ax, ay0 = 1.0f - ay;
                o[j] = ((s00 * (ay0 * ax0) + s01 * (ay0 * ax)) + s10 * (ay * ax0)) + s11 * (ay * ax);
            }
        }
    }
    if (!fast) plane_crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
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
    if (SCAN) plane_crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
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

// PX: the pixel format.  STAGE: the clip is 4-byte aligned, so the plan's STAGED windows can be copied by 16-byte global->LDS loads (always
// the case for buffers from hipMalloc / torch; the other instantiation ignores the windows).
// SCAN: the crop-boundary scan ALONE (crop_scan_kernel, warp.hip): the same ownership and coordinate code for footprint t of frame f,
// then only the four edge tests of mfs.py:1075-1098 -- no window, no taps, no blend, no store.  The certified paths (hot, pair,
// multi) are compiled out: their footprints cannot set a crop flag (MF_REGION_DEEP / MF_REGION_NOFLAG) and are never handed in.
// PX = Px::U16C3: the same ownership and coordinates for uint16 BGR frames (warp16_footprint): `frames` / `out` then point to uint16 samples,
// the border colour is `border16` (B | G << 16 | R << 32) and the pixels go through remap_store_u16 at the end of the general path -- the
// plan's staged windows are sized for 3-byte pixels, so this instantiation has no staged path (STAGE = false).
// PX = Px::U8C1: the same for single-channel uint8 frames (warp8c1_footprint): `frames` / `out` hold W H bytes per frame, the border is the
// low byte of `border`, and the pixels go through remap_store_u8c1.  With STAGE (GREY_STAGE below) the plan's STAGED windows (not the
// BORDER ones) are re-cut for 1-byte pixels (GreyWindow) and copied to LDS at the start, like warp_kernel's.
// PX = Px::U8C4: the same for 4-channel uint8 frames (warp8c4_footprint): `frames` / `out` hold 4 W H bytes per frame, the border is the whole
// `border` word, and the pixels go through remap_store_u8c4.  With STAGE (C4_STAGE below) the plan's STAGED windows (not the BORDER ones) are
// re-cut for 4-byte pixels (MF_C4_COLS) and copied to LDS at the start; the hot and pair footprints take the grey warp's shortcuts.
// PX = Px::MAPS: the coordinate maps instead of pixels (maps_footprint, warp_maps.hip): SCAN's body -- ownership, coordinates, the four edge
// tests on every footprint -- plus the store of (u, v) (maps_store_f32): `frames` is unused, `out` points to float32 [n][H][W][2].  No window, no
// taps, no border colour; the hot and pair footprints take the grey warp's shortcuts (they need no window here), everything else the general path.
// PX = Px::PLANE_*: the side planes (plane_footprint, warp_planes.hip): `frames` / `out` hold W H elements of px_sample_bytes(PX) bytes per
// frame, `border16` is the fill value's bit pattern, and the pixels go through remap_store_plane -- taps from global memory like the uint16
// warp (the plan's windows are cut for 3-byte pixels), the hot and pair shortcuts like the maps (they need no window), the general path for the rest.
template <Px PX, bool STAGE, bool SCAN>
__device__ __forceinline__ void footprint_body(const uint32_t f, const uint32_t t, const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions,
                                               const WarpGeom& g, const uint8_t* __restrict__ frames,
                                               const double* __restrict__ records, uint8_t* __restrict__ out,
                                               const float* __restrict__ edges, int n, int W,
                                               int H, int C, uint32_t border, int32_t* __restrict__ crop, int32_t* __restrict__ clip,
                                               uint64_t border16 = 0)
{
    static_assert(!SCAN || (PX == Px::U8C3 && !STAGE), "the crop scan runs the unstaged BGR body");
    static_assert(PX != Px::U16C3 || !STAGE, "the uint16 warp takes its taps from global memory");
    // BGR_STAGE: the uint8 BGR warp of a 4-byte aligned clip -- the staged window and the certified paths (hot, border, pair, multi)
    constexpr bool BGR_STAGE = PX == Px::U8C3 && STAGE && !SCAN;
    constexpr bool U16 = PX == Px::U16C3, GREY = PX == Px::U8C1, GREY_STAGE = GREY && STAGE;
    // C4_STAGE: the 4-channel warp of a 4-byte aligned clip; WIN_STAGE: a re-cut window (grey or 4-byte) and the hot / pair shortcuts on it
    constexpr bool C4 = PX == Px::U8C4, C4_STAGE = C4 && STAGE, WIN_STAGE = GREY_STAGE || C4_STAGE;
    constexpr bool MAPS = PX == Px::MAPS;
    static_assert(!MAPS || (!STAGE && !SCAN), "the maps kernel reads no frame: nothing to stage");
    // NOWIN: the instantiations that take the hot and pair shortcuts without a window (the maps read no frame, the planes tap global memory)
    constexpr bool PLANE = px_is_plane(PX), NOWIN = MAPS || PLANE;
    static_assert(!PLANE || (!STAGE && !SCAN), "the plane warps take their taps from global memory");
    // inverse homographies of the footprint's candidate cells: [entry][Hi0..Hi8, pad] (80-byte rows)
    __shared__ __attribute__((aligned(16))) double s_hi[1][9][10];                // row 8: the "no cell" matrix, see OWN_NONE
    // source region of the footprint: MF_STAGE_ROWS rows of MF_STAGE_PITCH bytes (+ slack for the third dword of the last tap); the 4-byte
    // window's MF_STAGE_ROWS rows of MF_C4_PITCH bytes for U8C4
    __shared__ __attribute__((aligned(16))) uint8_t s_src_all[SCAN || NOWIN ? 16 : C4 ? LDS_WINDOW_PAD + MF_STAGE_ROWS * MF_C4_PITCH
                                                                             : LDS_WINDOW_PAD + LDS_WINDOW_BYTES + 64];
    uint8_t* const s_src = &s_src_all[SCAN || NOWIN ? 0 : LDS_WINDOW_PAD];
    constexpr int wave = 0;
    const uint32_t ty = (__umulhi(t, g.div_m) + (t & g.div_pass)) >> g.div_s, tx = t - ty * g.nfx;
    const int xa = (int)(tx * (uint32_t)FOOT_W), ya = (int)(ty * (uint32_t)FOOT_H);
    const int lane = threadIdx.x;
    // SPECULATIVE matrix load.  A hot wavefront's life starts with three DEPENDENT scalar round trips -- kernel arguments, plan + region
    // words, the owner's inverse homography -- a quarter of its life (profiles/r05_phase_profile_cfg2.txt).  The owner of a hot footprint
    // is almost always the cell under the footprint's centre in the unwarped grid, which needs no plan: its matrix is requested HERE,
    // together with the plan words, and is there when they are.  The plan decides; a wrong guess (the neighbour cell owns the footprint,
    // or it is not hot at all) costs one unused 72-byte scalar load.  Inline asm: the compiler would sink the loads to their only use,
    // behind the plan's round trip; it does not know about them, so the hot path waits for them itself (spec_wait) before the first use.
    typedef uint32_t spec16_t __attribute__((ext_vector_type(16)));
    typedef uint32_t spec2_t __attribute__((ext_vector_type(2)));
    spec16_t hg_lo;
    spec2_t hg_hi;
    // ONLY in the instantiation that has a hot path (BGR_STAGE).  Anywhere else the registers would be dead right behind the asm
    // statement, the compiler would hand them to the plan words' loads two lines further down, and -- scalar loads return out of order
    // -- whichever load lands last would win: a footprint of a frame stack that is not 4-byte aligned (odd frame sizes cut into frame
    // ranges: warp_kernel<false>) then ran on a few bytes of some cell's matrix instead of its plan about once in 200 launches and left
    // rows unwritten (found by a sweep over mf_warp_clip_u8c3's chunkings at the end of round 5).
#ifndef MF_GUARD_SELFTEST
    constexpr bool SPECULATE = BGR_STAGE;                                 // (tools/isa_guard.py finds the hazard from the disassembly alone)
#else       // (tests/test_isa_guard.py builds THIS on purpose -- round 5's bug, the load in the instantiation without a hot path -- to see the guard fail)
    constexpr bool SPECULATE = !SCAN;
#endif
    const uint32_t k_guess = !SPECULATE ? 0u : min(__umulhi((uint32_t)ya + FOOT_H / 2, g.cell_mul_y) * g.mesh_cols + __umulhi((uint32_t)xa + FOOT_W / 2, g.cell_mul_x), g.cell_last);
    if (SPECULATE) {
        const uint64_t gaddr = (uint64_t)(uintptr_t)records + ((uint64_t)f * g.rec_frame_bytes + (uint64_t)k_guess * (uint32_t)(MF_CELL_DOUBLES * sizeof(double)));
        static_assert(MF_CELL_OFF_HI * sizeof(double) == 0x48 && MF_CELL_DOUBLES * sizeof(double) == 256, "offsets in the asm below");
        asm volatile("s_load_dwordx16 %0, %2, 0x48\n\ts_load_dwordx2 %1, %2, 0x88" : "=&s"(hg_lo), "=&s"(hg_hi) : "s"(gaddr));     // (early clobber: the address pair is read by both loads)
    }
    // (Round 6, measured and dropped: RE-ENTRY -- the wavefront jumps back to the kernel's first instruction as the next virtual workgroup, 2 or 4
    // footprints per wavefront with the product's code per trip: half / three quarters of the dispatches and of the end-of-life store waits gone,
    // byte-identical, +-0 -- so neither the launch rate nor a wavefront's latency limits the kernel, profiles/r06_ab_reentry.txt;
    // and -- profiles/r06_ab_prefetch.txt, profiles/README.md: touching the window lines of the footprint this
    // block index takes one or two frames on, to have them in the XCD's L2: +12...24 %; testing t >= per_frame BEHIND the plan's loads so
    // that all kernel arguments arrive in one scalar round trip instead of two: +-0.)
    const uint32_t fp = f * g.per_frame + t;                              // the footprint's slot in plan / regions
    typedef const __attribute__((address_space(4))) uint32_t* cword_t;
    const cword_t pw = (cword_t)(uintptr_t)(reinterpret_cast<const uint8_t*>(plan) + 16u * fp);
    const cword_t rw = (cword_t)(uintptr_t)(reinterpret_cast<const uint8_t*>(regions) + 8u * fp);
    const uint4 pv = make_uint4(pw[0], pw[1], pw[2], pw[3]);             // wave-uniform: scalar loads
    typedef const __attribute__((address_space(4))) uint64_t* cword2_t;
    const uint64_t region = *(cword2_t)rw;                               // both words in one load (the second is needed right after the first)
    const uint32_t rg = (uint32_t)region, src_dwords = (uint32_t)(region >> 32);
    const uint8_t* __restrict__ src = frames + (uint64_t)f * g.frame_bytes;
    const bool staged = BGR_STAGE && (rg & MF_REGION_STAGED) != 0;
    // Lane -> footprint row.  The byte taps are served per group of 32 lanes, bank = dword address mod 32, and the eight lanes of a
    // footprint row take every third bank.  With the wide window (pitch 160 bytes = 40 banks) the rows 0..3 of lanes 0-31 start 0, 8, 16,
    // 24 banks apart: no two lanes on one bank.  With the COMPACT window (pitch 112 bytes = 28 banks) rows 0 and 3 would collide on four
    // banks -- every tap instruction 3.5 instead of 1.8 LDS cycles (tools/ubench_lds_rowmap.hip) -- so there lanes 0-31 take rows 0, 2, 4, 6
    // (0, 24, 16, 8 banks apart) and lanes 32-63 rows 1, 3, 5, 7 (set where the COMPACT copy is issued: wave-uniform).  Every lane still
    // owns four pixels of ONE row.
    uint32_t row = (uint32_t)lane >> 3;
    if (staged) {
        // Source region -> LDS, asynchronously (global_load_lds: no VGPRs, no ds_write).  Two layouts, chosen by the plan:
        //   COMPACT (hot footprints whose taps fit 9 rows x 112 bytes: ~3/4 of them): ONE load, lane i fetches the i-th 16-byte
        //           chunk (7 chunks per row), which lands at LDS offset 16 i.  (Lane 63 fetches the first chunk of a tenth row: unused,
        //           inside the frame because the region is DEEP.)
        //   wide    (12 rows x 160 bytes): lane i fetches the i-th and (64+i)-th chunk (10 chunks per row) -> LDS 16 i, 1024 + 16 i.
        // chunk i sits at row i / P, byte 16 (i % P) of the window = byte (i / P) (row_bytes - 16 P) + 16 i from gbase;
        // uniform base + opaque 32-bit lane offset keeps the address arithmetic 32-bit (saddr + voffset form)
        const uint8_t* __restrict__ gbase = src + ((uint64_t)src_dwords << 2);
        const lds_bytes_t window = lds_ptr(&s_src[0]);
        if (rg & MF_REGION_BORDER) {
            // BORDER window: the 12 rows only (its last row may be the frame's last: there is no 13th to fetch) -- chunks 0..63, then 64..119
            uint32_t o0 = __umul24(((uint32_t)lane * 205u) >> 11, g.row_bytes - (uint32_t)MF_STAGE_PITCH) + ((uint32_t)lane << 4);
            uint32_t o1 = __umul24((((uint32_t)lane + 64u) * 205u) >> 11, g.row_bytes - (uint32_t)MF_STAGE_PITCH) + (((uint32_t)lane << 4) + 1024u);
            asm("" : "+v"(o0));
            asm("" : "+v"(o1));
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + o0), (__attribute__((address_space(3))) void*)window, 16, 0, 0);
            if (lane < MF_STAGE_ROWS * 10 - 64)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + o1), (__attribute__((address_space(3))) void*)(window + 1024), 16, 0, 0);
        } else if (rg & MF_REGION_COMPACT) {
            uint32_t o0 = __umul24(((uint32_t)lane * 37u) >> 8, g.row_bytes - (uint32_t)MF_COMPACT_PITCH) + ((uint32_t)lane << 4);
            asm("" : "+v"(o0));
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + o0), (__attribute__((address_space(3))) void*)window, 16, 0, 0);
            row = (((uint32_t)lane >> 2) & 6u) | ((uint32_t)lane >> 5);
        } else {
            uint32_t o0 = __umul24(((uint32_t)lane * 205u) >> 11, g.row_bytes - (uint32_t)MF_STAGE_PITCH) + ((uint32_t)lane << 4);
            uint32_t o1 = __umul24((((uint32_t)lane + 64u) * 205u) >> 11, g.row_bytes - (uint32_t)MF_STAGE_PITCH) +
                          (((uint32_t)lane << 4) + 1024u);
            asm("" : "+v"(o0));
            asm("" : "+v"(o1));
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + o0), (__attribute__((address_space(3))) void*)window, 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + o1), (__attribute__((address_space(3))) void*)(window + 1024), 16, 0, 0);
        }
    }
    GreyWindow gwin{false, 0u, 0u};
    if constexpr (GREY_STAGE) {
        // the plan's window re-cut for 1-byte pixels (GreyWindow), issued before the coordinate work like warp_kernel's: lane i < 5 rows
        // fetches chunk i (row i / 5, bytes 16 (i % 5) ..) to LDS byte 16 i
        if ((rg & (MF_REGION_STAGED | MF_REGION_BORDER)) == MF_REGION_STAGED && W >= MF_C1_PITCH) {
            const bool cmp = (rg & MF_REGION_COMPACT) != 0;
            const uint32_t P = cmp ? (uint32_t)MF_COMPACT_PITCH : (uint32_t)MF_STAGE_PITCH, rows = cmp ? (uint32_t)MF_COMPACT_ROWS : (uint32_t)MF_STAGE_ROWS;
            const uint32_t origin = rg & MF_REGION_ORIGIN_MASK, sbytes = src_dwords << 2;
            const uint32_t sy0 = __builtin_amdgcn_readfirstlane((uint32_t)((float)(sbytes - origin) / (float)(3u * (uint32_t)W - P) + 0.5f));
            const uint32_t bs = origin - P * sy0;
            const uint32_t gx = min((bs / 3u) & ~3u, (uint32_t)W - (uint32_t)MF_C1_PITCH);
            gwin.on = true; gwin.row0 = sy0; gwin.col0 = gx;
            const uint8_t* __restrict__ gbase = frames + (uint64_t)f * (uint64_t)((uint32_t)W * (uint32_t)H) + (uint64_t)(sy0 * (uint32_t)W + gx);
            if ((uint32_t)lane < 5u * rows) {
                const uint32_t r = ((uint32_t)lane * 205u) >> 10;          // lane / 5 (lane < 64)
                uint32_t o0 = umad24(r, (uint32_t)W, ((uint32_t)lane - 5u * r) << 4);
                asm("" : "+v"(o0));
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + o0), (__attribute__((address_space(3))) void*)lds_ptr(&s_src[0]), 16, 0, 0);
            }
        }
    }
    if constexpr (C4_STAGE) {
        // the plan's window re-cut for 4-byte pixels (MF_C4_COLS), issued before the coordinate work like the grey one: lane i fetches chunks
        // i, 64 + i and 128 + i below 14 rows (row c / 14, bytes 16 (c % 14) ..) to LDS byte 16 c
        if ((rg & (MF_REGION_STAGED | MF_REGION_BORDER)) == MF_REGION_STAGED && W >= MF_C4_COLS) {
            const bool cmp = (rg & MF_REGION_COMPACT) != 0;
            const uint32_t P = cmp ? (uint32_t)MF_COMPACT_PITCH : (uint32_t)MF_STAGE_PITCH, rows = cmp ? (uint32_t)MF_COMPACT_ROWS : (uint32_t)MF_STAGE_ROWS;
            const uint32_t origin = rg & MF_REGION_ORIGIN_MASK, sbytes = src_dwords << 2;
            const uint32_t sy0 = __builtin_amdgcn_readfirstlane((uint32_t)((float)(sbytes - origin) / (float)(3u * (uint32_t)W - P) + 0.5f));
            const uint32_t bs = origin - P * sy0;
            const uint32_t gx = min(bs / 3u, (uint32_t)W - (uint32_t)MF_C4_COLS);
            gwin.on = true; gwin.row0 = sy0; gwin.col0 = gx;
            const uint8_t* __restrict__ gbase = frames + (uint64_t)f * (4ull * (uint64_t)((uint32_t)W * (uint32_t)H)) + 4ull * (uint64_t)(sy0 * (uint32_t)W + gx);
            constexpr uint32_t row_chunks = MF_C4_PITCH / 16;
#pragma unroll
            for (uint32_t c0 = 0; c0 < MF_STAGE_ROWS * row_chunks; c0 += 64) {
                const uint32_t c = (uint32_t)lane + c0;
                if (c < row_chunks * rows) {
                    const uint32_t r = c / row_chunks;
                    uint32_t o0 = umad24(r, 4u * (uint32_t)W, (c - row_chunks * r) << 4);
                    asm("" : "+v"(o0));
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + o0),
                                                     (__attribute__((address_space(3))) void*)(lds_ptr(&s_src[0]) + 16u * c0), 16, 0, 0);
                }
            }
        }
    }
    // (a wavefront must not END with its global->LDS copy in flight: on this stack that is a GPU memory access fault, profiles/README.md
    // round 6: whatever returns below this line waits for the copy first, s_waitcnt vmcnt(0))
    // taps are addressed by absolute LDS byte address (= LDS_PITCH iy + 3 ix - lds_origin): the window base is folded in
    const uint32_t lds_origin = (rg & MF_REGION_ORIGIN_MASK) - (uint32_t)(uintptr_t)&s_src[0];
    const crec_t frec = (crec_t)(uintptr_t)(reinterpret_cast<const uint8_t*>(records) + f * g.rec_frame_bytes);
    const bool compact = BGR_STAGE && (rg & MF_REGION_COMPACT) != 0;
    const int y = ya + (int)row;
    const int x0 = xa + (lane & 7) * 4;                                  // first of this lane's 4 pixels
    const double xs0 = (double)x0, yy = (double)y;

    if (BGR_STAGE && (pv.x & (MF_PLAN_HOT << 16)) != 0) {
        // The plan certifies everything (~2/3 of the footprints at config-2 geometry): ONE cell owns all 256 pixels, its
        // denominator allows the trimmed reciprocal (UNIT), the footprint lies inside the frame, its window is staged and every
        // tap is at least two pixels inside the frame (DEEP: no crop flag either).  Straight-line code, all lanes active.
        float u[4], v[4];
        bool have_coords = false;
        if ((pv.x >> 16) & MF_PLAN_FAST64) {
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(hg_lo), "+s"(hg_hi));      // (the speculative load: long there -- the plan words came behind it)
            double Hi[9];
#pragma unroll
            for (int i = 0; i < 8; ++i) Hi[i] = __hiloint2double((int)hg_lo[2 * i + 1], (int)hg_lo[2 * i]);
            Hi[8] = __hiloint2double((int)hg_hi[1], (int)hg_hi[0]);
            if ((pv.x & 0xFFFu) != k_guess) {                             // (wave-uniform: the guess was the wrong cell)
                const crec_t rec = frec + (pv.x & 0xFFFu) * MF_CELL_DOUBLES;
#pragma unroll
                for (int i = 0; i < 9; ++i) Hi[i] = rec[MF_CELL_OFF_HI + i];
            }
            have_coords = coords_fast(Hi, xs0, yy, u, v);
        }
        if (!have_coords) cell_coords<false>(frec + (pv.x & 0xFFFu) * MF_CELL_DOUBLES, xs0, yy, x0, 0xFu, u, v, true);
        uint32_t bx[4], by[4];
        fixed_point(u, v, bx, by);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the window has landed in LDS
        uint8_t* __restrict__ dst = out + (uint64_t)f * g.frame_bytes;
        const uint3 d = gather_blend_window(compact, bx, by, lds_origin);
        *reinterpret_cast<uint3*>(dst + ((uint32_t)y * (uint32_t)W + (uint32_t)x0) * 3u) = d;     // (STAGED implies W % 4 == 0)
        return;
    }

    if constexpr (WIN_STAGE || NOWIN) {
        if ((NOWIN || gwin.on) && (pv.x & (MF_PLAN_HOT << 16)) != 0) {
            // the HOT footprints of the grey warp (one IN cell, certified denominator, deep, staged): the hot path's coordinates -- the cheap
            // chain where the plan allows it (FAST64), else the trimmed-reciprocal one -- without the general path's ownership code
            const crec_t rec = frec + (pv.x & 0xFFFu) * MF_CELL_DOUBLES;
            float u[4], v[4];
            if (!((pv.x >> 16) & MF_PLAN_FAST64) || !cell_coords_fast(rec, xs0, yy, u, v))
                cell_coords<false>(rec, xs0, yy, x0, 0xFu, u, v, true);
            // (MAPS: a hot footprint is whole and DEEP -- every lane stores, no pixel can pass a crop test)
            if constexpr (MAPS) maps_store_f32(u, v, f, x0, y, true, W, H, reinterpret_cast<float*>(out));
            else if constexpr (PLANE) remap_store_plane<PX, false>(u, v, f, x0, y, true, W, H, frames, out, border16, crop, clip);
            else if constexpr (C4) remap_store_u8c4(u, v, f, x0, y, true, W, H, frames, out, border, crop, clip, gwin, &s_src[0]);
            else remap_store_u8c1(u, v, f, x0, y, true, W, H, frames, out, border, crop, clip, gwin, &s_src[0]);
            return;
        }
    }
    const cedge_t fedge = (cedge_t)(uintptr_t)(reinterpret_cast<const uint8_t*>(edges) + f * g.edge_frame_bytes);
    if constexpr (WIN_STAGE || NOWIN) {
        if ((NOWIN || gwin.on) && (pv.y & MF_PLAN_HOT) != 0) {
            // the PAIR footprints of the grey warp (two cells, certified denominators, deep, staged): warp_kernel's per-pixel pair form --
            // the later cell owns a pixel where its one mask edge passes (one fma), the other cell the rest, both matrices in LDS; a pixel
            // inside the edge's float32 error band leaves the footprint to the general code
            const uint32_t k0 = pv.x & 0xFFFu, k1 = (pv.x >> 16) & 0xFFFu;
            if (lane < 20) {
                uint32_t lo4 = (uint32_t)lane << 2;
                asm("" : "+v"(lo4));
                const uint8_t* __restrict__ g0 = (const uint8_t*)(uintptr_t)(frec + k0 * MF_CELL_DOUBLES + MF_CELL_OFF_HI);
                const uint8_t* __restrict__ g1 = (const uint8_t*)(uintptr_t)(frec + k1 * MF_CELL_DOUBLES + MF_CELL_OFF_HI);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g0 + lo4),
                                                 (__attribute__((address_space(3))) void*)lds_ptr(&s_hi[0][0][0]), 4, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g1 + lo4),
                                                 (__attribute__((address_space(3))) void*)lds_ptr(&s_hi[0][1][0]), 4, 0, 0);
            }
            const cedge_t eb = fedge + k0 * MF_EDGE_FLOATS + 3u * (pv.z & 3u);
            const float rb = __builtin_fmaf(eb[1], (float)y, eb[2]), xf0 = (float)x0;
            uint32_t own[4];
            float near = 1e30f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gb = __builtin_fmaf(eb[0], xf0 + (float)j, rb);
                own[j] = gb > EDGE_BAND ? 0u : OWN_ROW;
                near = fminf(near, fabsf(gb));
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // matrices (and the grey window) have landed in LDS
            if (__ballot(!(near > EDGE_BAND)) == 0) {
                float u[4], v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double* hp = reinterpret_cast<const double*>(reinterpret_cast<const uint8_t*>(&s_hi[0][0][0]) + own[j]);
                    const double2 h01 = *reinterpret_cast<const double2*>(hp), h23 = *reinterpret_cast<const double2*>(hp + 2);
                    const double2 h45 = *reinterpret_cast<const double2*>(hp + 4), h67 = *reinterpret_cast<const double2*>(hp + 6);
                    const double h8 = hp[8];
                    const double xs = xs0 + (double)j;
                    const double iw = recip_unit_range((xs * h67.x + yy * h67.y) + h8);
                    u[j] = (float)(((xs * h01.x + yy * h01.y) + h23.x) * iw);
                    v[j] = (float)(((xs * h23.y + yy * h45.x) + h45.y) * iw);
                }
                if constexpr (MAPS) maps_store_f32(u, v, f, x0, y, true, W, H, reinterpret_cast<float*>(out));
                else if constexpr (PLANE) remap_store_plane<PX, false>(u, v, f, x0, y, true, W, H, frames, out, border16, crop, clip);
                else if constexpr (C4) remap_store_u8c4(u, v, f, x0, y, true, W, H, frames, out, border, crop, clip, gwin, &s_src[0]);
                else remap_store_u8c1(u, v, f, x0, y, true, W, H, frames, out, border, crop, clip, gwin, &s_src[0]);
                return;
            }
        }
    }
    if (BGR_STAGE && ((pv.x >> 16) & (MF_PLAN_VALID | MF_PLAN_BORDER)) == MF_PLAN_BORDER) {
        // BORDER path (the ring of footprints along the frame border of a stabilised clip, and the odd footprint a single cell only partly
        // covers: ~3 %): ONE candidate cell -- IN, or MIXED with one or two coded mask edges -- with a certified denominator; whole
        // footprint; every tap of a covered pixel lies in the staged window or on the ring of pixels just outside the frame, which is
        // painted into the window in the border colour here.  So the taps come from the staged gather like everywhere else: no
        // clamping, no per-tap selects (cv2.remap BORDER_CONSTANT, mfs.py:1063-1069).  Pixels the cell does not cover get the border
        // colour (the map template's (W+1, H+1), mfs.py:983-984) and take no part in the crop scan; a pixel inside the float32 error
        // band of an edge sends the wavefront to the general code.
        const uint32_t k0 = pv.x & 0xFFFu;
        uint32_t cov = 0xFu;
        bool decided = true;
        if (!(pv.x & MF_PLAN_IN)) {
            const uint32_t cd = pv.z & 0x3Fu;
            const cedge_t ed = fedge + k0 * MF_EDGE_FLOATS;
            const cedge_t e1 = ed + 3u * (cd & 3u);
            const cedge_t e2 = ed + 3u * ((cd & 8u) ? ((cd >> 4) & 3u) : (cd & 3u));     // one-edge code: the same edge twice
            const float yf = (float)y, xf0 = (float)x0;
            const float r1 = __builtin_fmaf(e1[1], yf, e1[2]), r2 = __builtin_fmaf(e2[1], yf, e2[2]);
            float near = 1e30f;
            cov = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xf = xf0 + (float)j;
                const float gq = fminf(__builtin_fmaf(e1[0], xf, r1), __builtin_fmaf(e2[0], xf, r2));
                cov |= gq > EDGE_BAND ? (1u << j) : 0u;
                near = fminf(near, fabsf(gq));
            }
            decided = __ballot(!(near > EDGE_BAND)) == 0;           // (NaN coefficients: undecided)
        }
        if (decided) {
            float u[4], v[4];
            cell_coords<false>(frec + k0 * MF_CELL_DOUBLES, xs0, yy, x0, 0xFu, u, v, true);
            // crop-boundary scan of the covered pixels, mfs.py:1075-1098 (exact: Sterbenz, as on the generic path)
            {
                const float fWm1 = (float)(W - 1), fHm1 = (float)(H - 1);
                int c_left = 0, c_top = 0, c_right = W - 1, c_bottom = H - 1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if ((cov >> j) & 1u) {
                        const int x = x0 + j;
                        if (fabsf(u[j]) < 1.0f) c_left = max(c_left, x);
                        if (fabsf(u[j] - fWm1) < 1.0f) c_right = min(c_right, x);
                        if (fabsf(v[j]) < 1.0f) c_top = max(c_top, y);
                        if (fabsf(v[j] - fHm1) < 1.0f) c_bottom = min(c_bottom, y);
                    }
                }
                const bool any = c_left != 0 || c_top != 0 || c_right != W - 1 || c_bottom != H - 1;
                if (__ballot(any) != 0) {
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        c_left = max(c_left, __shfl_xor(c_left, off));
                        c_top = max(c_top, __shfl_xor(c_top, off));
                        c_right = min(c_right, __shfl_xor(c_right, off));
                        c_bottom = min(c_bottom, __shfl_xor(c_bottom, off));
                    }
                    if (lane == 0) {
                        // (per frame, mfs.py:1075-1098, and straight into the clip-level rectangle, mfs.py:1103-1106)
                        if (c_left != 0) { atomicMax(&crop[4 * f + 0], c_left); atomicMax(&clip[0], c_left); }
                        if (c_top != 0) { atomicMax(&crop[4 * f + 1], c_top); atomicMax(&clip[1], c_top); }
                        if (c_right != W - 1) { atomicMin(&crop[4 * f + 2], c_right); atomicMin(&clip[2], c_right); }
                        if (c_bottom != H - 1) { atomicMin(&crop[4 * f + 3], c_bottom); atomicMin(&clip[3], c_bottom); }
                    }
                }
            }
            uint32_t bx[4], by[4];
            fixed_point(u, v, bx, by);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the window has landed in LDS
            // Paint what lies just outside the frame: whole pixels (B, G, R) at the LDS address the gather will form for them -- tap
            // (ix, iy) sits at LDS_PITCH iy + 3 ix - lds_origin.  Column -1 / W for the rows -1 .. 12 of the window (14 lanes each), row
            // -1 / H for the columns that lie completely inside a window row (at most 53 lanes; no tap needs any other).  LDS operations of a wavefront execute
            // in order: the gather below sees these bytes.
            if (rg & (MF_REGION_PAINT_LEFT | MF_REGION_PAINT_RIGHT | MF_REGION_PAINT_TOP | MF_REGION_PAINT_BOTTOM)) {
                // (window origin in the frame from its first dword: row sy0, byte bs of the row -- bs can exceed the LDS pitch, so the
                // LDS origin does not split uniquely)
                const uint32_t first = src_dwords << 2;
                const int sy0 = (int)(first / g.row_bytes), bs = (int)(first - (uint32_t)sy0 * g.row_bytes);
                const int col0 = (bs + 2) / 3;                           // first column that starts inside the window's rows
                const auto paint = [&](int ix, int iy) {
                    const uint32_t at = (uint32_t)LDS_PITCH * (uint32_t)iy + 3u * (uint32_t)ix - lds_origin;      // (mod 2^32, like tap_address)
                    volatile __attribute__((address_space(3))) uint8_t* t = (volatile __attribute__((address_space(3))) uint8_t*)(uintptr_t)at;
                    t[0] = (uint8_t)border; t[1] = (uint8_t)(border >> 8); t[2] = (uint8_t)(border >> 16);
                };
                // (only the columns whose three bytes lie inside the LDS row: a neighbour's would land on the last bytes of the row in front or
                // the first of the row behind, which may be needed)
                const int ncols = (bs + LDS_PITCH - 3) / 3 - col0 + 1;
                if ((rg & MF_REGION_PAINT_TOP) && lane < ncols) paint(col0 + lane, -1);
                if ((rg & MF_REGION_PAINT_BOTTOM) && lane < ncols) paint(col0 + lane, H);
                // (the columns LAST: column -1 of a row shares its bytes with the end of the LDS row in front -- column 52, which no tap
                // needs -- and column W with the start of the row behind; the row paints above reach into both)
                if ((rg & MF_REGION_PAINT_LEFT) && lane < 14) paint(-1, sy0 - 1 + lane);
                if ((rg & MF_REGION_PAINT_RIGHT) && lane < 14) paint(W, sy0 - 1 + lane);
                __builtin_amdgcn_wave_barrier();
            }
            uint3 d = gather_blend_staged(bx, by, lds_origin);
            if (cov != 0xFu) {
                // pixels the cell does not cover: the border colour.  The lane's 12 bytes are B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3.
                const uint32_t b0 = border & 0xFFu, b1 = (border >> 8) & 0xFFu, b2 = (border >> 16) & 0xFFu;
                const uint32_t w0 = b0 | b1 << 8 | b2 << 16 | b0 << 24, w1 = b1 | b2 << 8 | b0 << 16 | b1 << 24, w2 = b2 | b0 << 8 | b1 << 16 | b2 << 24;
                const uint32_t m0 = ((cov & 1u) ? 0x00FFFFFFu : 0u) | ((cov & 2u) ? 0xFF000000u : 0u);
                const uint32_t m1 = ((cov & 2u) ? 0x0000FFFFu : 0u) | ((cov & 4u) ? 0xFFFF0000u : 0u);
                const uint32_t m2 = ((cov & 4u) ? 0x000000FFu : 0u) | ((cov & 8u) ? 0xFFFFFF00u : 0u);
                d.x = (d.x & m0) | (w0 & ~m0);
                d.y = (d.y & m1) | (w1 & ~m1);
                d.z = (d.z & m2) | (w2 & ~m2);
            }
            uint8_t* __restrict__ dstb = out + (uint64_t)f * g.frame_bytes;
            *reinterpret_cast<uint3*>(dstb + ((uint32_t)y * (uint32_t)W + (uint32_t)x0) * 3u) = d;     // (STAGED implies W % 4 == 0; the footprint is whole)
            return;
        }
    }
    if (BGR_STAGE && (pv.y & MF_PLAN_HOT) != 0) {
        // Two cells share the footprint and the plan certifies the rest (a quarter of the footprints at config-2 geometry, 45 % at
        // config 3): the later cell wins wherever ONE of its mask edges passes -- one float32 fma per pixel -- and the other cell
        // owns what is left; denominators, window and interior as on the hot path.  Both inverse homographies go to LDS by
        // global->LDS DMA (one 80-byte load per cell, scalar base address), and every pixel reads its owner's row.
        const uint32_t k0 = pv.x & 0xFFFu, k1 = (pv.x >> 16) & 0xFFFu;
        if (lane < 20) {
            uint32_t lo4 = (uint32_t)lane << 2;
            asm("" : "+v"(lo4));                        // (opaque: keeps the scalar base + 32-bit lane offset addressing form)
            uint64_t b0 = (uint64_t)(uintptr_t)(frec + k0 * MF_CELL_DOUBLES + MF_CELL_OFF_HI), b1 = (uint64_t)(uintptr_t)(frec + k1 * MF_CELL_DOUBLES + MF_CELL_OFF_HI);
            asm("" : "+s"(b0), "+s"(b1));                   // (whole bases in scalar registers: scalar base + 32-bit lane offset addressing)
            const uint8_t* __restrict__ g0 = (const uint8_t*)(uintptr_t)b0;
            const uint8_t* __restrict__ g1 = (const uint8_t*)(uintptr_t)b1;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g0 + lo4),
                                             (__attribute__((address_space(3))) void*)lds_ptr(&s_hi[0][0][0]), 4, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g1 + lo4),
                                             (__attribute__((address_space(3))) void*)lds_ptr(&s_hi[0][1][0]), 4, 0, 0);
        }
        const cedge_t eb = fedge + k0 * MF_EDGE_FLOATS + 3u * (pv.z & 3u);
        if (pv.y & MF_PLAN_PAIR_FAST) {
            // LANE-UNIFORM form.  The edge crosses the footprint, but hardly ever the four pixels of a LANE when the lane's pixels run
            // ALONG it: for a mostly vertical edge (MF_PLAN_PAIR_VERT) the lanes are transposed -- lane l = column l % 32, rows
            // 4 (l / 32) .. + 3 -- for a mostly horizontal one they stay as they are (4 pixels of a row).  When every lane's four
            // pixels have ONE owner (wave-uniform test) the lane reads that owner's matrix from LDS once and runs the hot path's
            // cheap coordinate chain on it (one reciprocal per lane, plan-certified premises for both cells, midpoint guard): 5 LDS
            // matrix reads instead of 20 and 60 float64 operations instead of 100 per lane.  A transposed lane's pixels go back
            // through LDS (the window is no longer needed) to the row-major lanes that store them, 12 bytes each.
            // (two instantiations, chosen by a scalar branch: no per-lane selects on the wave-uniform direction)
            const auto lane_uniform = [&](auto vert_c) -> bool {
                constexpr bool VERT = decltype(vert_c)::value;
                const int px = VERT ? xa + (lane & 31) : x0, py = VERT ? ya + 4 * (lane >> 5) : y;
                // The edge function is affine along the lane, so its values at the lane's first and last pixel decide for all four: both
                // beyond the error band on the same side = one owner (the same evaluation as below -- a x + (b y + c), two fma -- so the
                // scaled band keeps its meaning: beyond +-1 the sign is the exact function's)
                const float g0 = __builtin_fmaf(eb[0], (float)px, __builtin_fmaf(eb[1], (float)py, eb[2]));
                const float g3 = VERT ? __builtin_fmaf(eb[0], (float)px, __builtin_fmaf(eb[1], (float)(py + 3), eb[2]))
                                      : __builtin_fmaf(eb[0], (float)(px + 3), __builtin_fmaf(eb[1], (float)py, eb[2]));
                const float lo = fminf(g0, g3), hi = fmaxf(g0, g3);
                const bool first = lo > EDGE_BAND, second = hi < -EDGE_BAND;         // (NaN coefficients: neither)
                if (__ballot(!(first || second)) != 0) return false;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // matrices and window have landed in LDS
                typedef const __attribute__((address_space(3))) double* lds_d;
                uint32_t hrow = (uint32_t)(uintptr_t)&s_hi[0][0][0] + (first ? 0u : OWN_ROW);
                asm("" : "+v"(hrow));                                    // (one address register + immediate offsets, not a select per load)
                const lds_d hp = (lds_d)(uintptr_t)hrow;
                const double Hl[9] = { hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], hp[7], hp[8] };
                float u[4], v[4];
                if (__ballot(coords_fast_dir<VERT>(Hl, (double)px, (double)py, u, v) < FAST64_NEAR) != 0) return false;
                uint32_t bx[4], by[4];
                fixed_point(u, v, bx, by);
                uint8_t* __restrict__ dst = out + (uint64_t)f * g.frame_bytes;
                uint3 d;
                if (VERT) {
                    uint32_t oB[4], oG[4], oR[4];
                    if (compact) gather_blend_sums<MF_COMPACT_PITCH>(bx, by, lds_origin, oB, oG, oR);
                    else gather_blend_sums<LDS_PITCH>(bx, by, lds_origin, oB, oG, oR);
                    // pixel (column c, row r) as B | G << 8 | R << 16 at word r * 32 + c of the (spent) window buffer ...
                    volatile uint32_t* tw = reinterpret_cast<volatile uint32_t*>(&s_src[0]);
                    const uint32_t at = (uint32_t)(4 * (lane >> 5)) * 32u + (uint32_t)(lane & 31);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        tw[at + 32u * (uint32_t)j] = __builtin_amdgcn_perm(oR[j], __builtin_amdgcn_perm(oG[j], oB[j], 0x0C0C0602u), 0x0C060100u);
                    __builtin_amdgcn_wave_barrier();
                    // ... and every lane takes the four pixels it stores: words 32 row + 4 (l % 8) .. + 3
                    // (its row is y - ya: the lane -> row mapping of the window layout, whatever it is)
                    const uint32_t w0 = 32u * (uint32_t)(y - ya) + 4u * ((uint32_t)lane & 7u);
                    const uint32_t p0 = tw[w0], p1 = tw[w0 + 1], p2 = tw[w0 + 2], p3 = tw[w0 + 3];
                    d.x = p0 | (p1 << 24);
                    d.y = (p1 >> 8) | (p2 << 16);
                    d.z = (p2 >> 16) | (p3 << 8);
                } else {
                    d = gather_blend_window(compact, bx, by, lds_origin);
                }
                *reinterpret_cast<uint3*>(dst + ((uint32_t)y * (uint32_t)W + (uint32_t)x0) * 3u) = d;
                return true;
            };
            if ((pv.y & MF_PLAN_PAIR_VERT) ? lane_uniform(std::true_type{}) : lane_uniform(std::false_type{})) return;
        }
        const float rb = __builtin_fmaf(eb[1], (float)y, eb[2]), xf0 = (float)x0;
        uint32_t own[4];
        float near = 1e30f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gb = __builtin_fmaf(eb[0], xf0 + (float)j, rb);
            own[j] = gb > EDGE_BAND ? 0u : OWN_ROW;
            near = fminf(near, fabsf(gb));
        }
        // (a pixel inside the float32 error band of the edge, or NaN coefficients: the general code below decides exactly)
        if (__ballot(!(near > EDGE_BAND)) == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // matrices and window have landed in LDS
            float u[4], v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double* hp = reinterpret_cast<const double*>(reinterpret_cast<const uint8_t*>(&s_hi[0][0][0]) + own[j]);
                const double2 h01 = *reinterpret_cast<const double2*>(hp), h23 = *reinterpret_cast<const double2*>(hp + 2);
                const double2 h45 = *reinterpret_cast<const double2*>(hp + 4), h67 = *reinterpret_cast<const double2*>(hp + 6);
                const double h8 = hp[8];
                const double xs = xs0 + (double)j;
                const double iw = recip_unit_range((xs * h67.x + yy * h67.y) + h8);
                u[j] = (float)(((xs * h01.x + yy * h01.y) + h23.x) * iw);
                v[j] = (float)(((xs * h23.y + yy * h45.x) + h45.y) * iw);
            }
            uint32_t bx[4], by[4];
            fixed_point(u, v, bx, by);
            uint8_t* __restrict__ dst = out + (uint64_t)f * g.frame_bytes;
            const uint3 d = gather_blend_window(compact, bx, by, lds_origin);
            *reinterpret_cast<uint3*>(dst + ((uint32_t)y * (uint32_t)W + (uint32_t)x0) * 3u) = d;
            return;
        }
    }

    if (BGR_STAGE && (pv.z & MF_PLAN_HOT) != 0) {
        // Two to four cells, each MIXED one with one or two coded mask edges (the four cells around a mesh vertex, three of them, or a
        // pair the pair path did not take); window, interior and denominators certified, coverage not: a pixel that no listed cell
        // takes -- or one inside the float32 error band of an edge -- sends the wavefront to the general code.
        const int ne = (int)((pv.z >> MF_PLAN_COUNT_SHIFT) & 3u) + 1;
        if (lane < 20) {
            uint32_t lo4 = (uint32_t)lane << 2;
            asm("" : "+v"(lo4));                        // (opaque: keeps the scalar base + 32-bit lane offset addressing form)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < ne) {
                    const uint32_t k = ((i < 2 ? pv.x : pv.y) >> (16 * (i & 1))) & 0xFFFu;
                    uint64_t bi = (uint64_t)(uintptr_t)(frec + k * MF_CELL_DOUBLES + MF_CELL_OFF_HI);
                    asm("" : "+s"(bi));
                    const uint8_t* __restrict__ gi = (const uint8_t*)(uintptr_t)bi;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gi + lo4),
                                                     (__attribute__((address_space(3))) void*)lds_ptr(&s_hi[0][i][0]), 4, 0, 0);
                }
            }
        }
        const float yf = (float)y, xf0 = (float)x0;
        uint32_t own[4] = { OWN_NONE, OWN_NONE, OWN_NONE, OWN_NONE };
        float near = 1e30f;
#pragma unroll
        for (int i = 3; i >= 0; --i) {                  // first entry last: it wins
            if (i < ne) {
                const uint32_t ent = (i < 2 ? pv.x : pv.y) >> (16 * (i & 1));
                if (ent & MF_PLAN_IN) {                 // (only the last entry can be IN: it owns what the others leave)
#pragma unroll
                    for (int j = 0; j < 4; ++j) own[j] = OWN_ROW * (uint32_t)i;
                } else {
                    const uint32_t cd = ((i < 2 ? pv.z : pv.w) >> (16 * (i & 1))) & 0x3Fu;
                    const cedge_t ed = fedge + (ent & 0xFFFu) * MF_EDGE_FLOATS;
                    const cedge_t e1 = ed + 3u * (cd & 3u);
                    const cedge_t e2 = ed + 3u * ((cd & 8u) ? ((cd >> 4) & 3u) : (cd & 3u));     // one-edge code: the same edge twice
                    const float r1 = __builtin_fmaf(e1[1], yf, e1[2]), r2 = __builtin_fmaf(e2[1], yf, e2[2]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xf = xf0 + (float)j;
                        const float gq = fminf(__builtin_fmaf(e1[0], xf, r1), __builtin_fmaf(e2[0], xf, r2));
                        own[j] = gq > EDGE_BAND ? OWN_ROW * (uint32_t)i : own[j];
                        near = fminf(near, fabsf(gq));
                    }
                }
            }
        }
        const uint32_t worst = max(max(own[0], own[1]), max(own[2], own[3]));
        if (__ballot(!(near > EDGE_BAND) || worst == OWN_NONE) == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // matrices and window have landed in LDS
            float u[4], v[4];
            bool have = false;
            if (pv.z & MF_PLAN_MULTI_FAST) {
                // every listed cell satisfies the premises of the cheap chain: fused affine forms per pixel from its owner's matrix, one
                // reciprocal for the lane's four denominators, midpoint guard (a flagged wavefront takes the exact chain below)
                double wq[4], nq[4], mq[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double* hp = reinterpret_cast<const double*>(reinterpret_cast<const uint8_t*>(&s_hi[0][0][0]) + own[j]);
                    const double2 h01 = *reinterpret_cast<const double2*>(hp), h23 = *reinterpret_cast<const double2*>(hp + 2);
                    const double2 h45 = *reinterpret_cast<const double2*>(hp + 4), h67 = *reinterpret_cast<const double2*>(hp + 6);
                    const double xs = xs0 + (double)j;
                    nq[j] = __builtin_fma(xs, h01.x, __builtin_fma(yy, h01.y, h23.x));
                    mq[j] = __builtin_fma(xs, h23.y, __builtin_fma(yy, h45.x, h45.y));
                    wq[j] = __builtin_fma(xs, h67.x, __builtin_fma(yy, h67.y, hp[8]));
                }
                have = __ballot(cheap_quotients(wq, nq, mq, u, v) < FAST64_NEAR) == 0;
            }
            if (!have) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double* hp = reinterpret_cast<const double*>(reinterpret_cast<const uint8_t*>(&s_hi[0][0][0]) + own[j]);
                    const double2 h01 = *reinterpret_cast<const double2*>(hp), h23 = *reinterpret_cast<const double2*>(hp + 2);
                    const double2 h45 = *reinterpret_cast<const double2*>(hp + 4), h67 = *reinterpret_cast<const double2*>(hp + 6);
                    const double h8 = hp[8];
                    const double xs = xs0 + (double)j;
                    const double iw = recip_unit_range((xs * h67.x + yy * h67.y) + h8);
                    u[j] = (float)(((xs * h01.x + yy * h01.y) + h23.x) * iw);
                    v[j] = (float)(((xs * h23.y + yy * h45.x) + h45.y) * iw);
                }
            }
            uint32_t bx[4], by[4];
            fixed_point(u, v, bx, by);
            uint8_t* __restrict__ dst = out + (uint64_t)f * g.frame_bytes;
            const uint3 d = gather_blend_window(compact, bx, by, lds_origin);
            *reinterpret_cast<uint3*>(dst + ((uint32_t)y * (uint32_t)W + (uint32_t)x0) * 3u) = d;
            return;
        }
    }

    // Everything else: more candidate cells, uncertified denominators, frame borders, uncovered pixels.
    uint8_t* __restrict__ dst = out + (uint64_t)f * g.frame_bytes;
    const uint32_t limit = (int)f == n - 1 ? g.frame_bytes : 0xFFFFFFFFu;   // only the last frame has nothing behind it
    const float fWm1 = (float)(W - 1), fHm1 = (float)(H - 1);
    const bool fast_store = (W & 3) == 0;
    // active = y < H && x0 < W, built on the scalar unit as a lane mask (rows_in rows of the footprint, and in each the first
    // cols_in groups of four pixels, start inside the frame) and turned into the branch condition without a v_cmp
    const int rows_in = min(FOOT_H, H - ya), cols_in = min(FOOT_W / 4, (W - xa + 3) >> 2);
    const uint32_t row_bits = ((1u << cols_in) - 1u) * 0x01010101u;
    const uint64_t lanes_in = (((uint64_t)row_bits << 32) | row_bits) & (~0ull >> (64 - 8 * rows_in));
    const bool active = __builtin_amdgcn_inverse_ballot_w64(lanes_in);
    {
        // Source coordinates of the lane's 4 pixels; (W+1, H+1) = "no cell covers it" (mfs.py:983-984).
        float u[4], v[4];
        if ((pv.x & (MF_PLAN_IN | MF_PLAN_VALID)) == (MF_PLAN_IN | MF_PLAN_VALID) && (pv.w >> 16) != MF_PLAN_OVERFLOW) {
            // one cell owns the whole footprint (the common case): no per-pixel test, no merging
            cell_coords<false>(frec + (pv.x & 0xFFFu) * MF_CELL_DOUBLES, xs0, yy, x0, 0xFu, u, v, ((pv.x >> 16) & MF_PLAN_UNIT) != 0);
        } else if ((pv.w >> 16) == MF_PLAN_OVERFLOW) {
            // more than 8 candidate cells: test every cell of the recorded range, last cell first
            uint32_t unowned = 0;
            int Wp = W + 1, Hp = H + 1;                      // (opaque: keeps the conversions inside this rare branch)
            asm volatile("" : "+s"(Wp), "+s"(Hp));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u[j] = (float)Wp;
                v[j] = (float)Hp;
                if (x0 + j < W && y < H) unowned |= 1u << j;
            }
            const int r_lo = pv.x & 0xFFFF, c_lo = pv.y & 0xFFFF, c_hi = pv.y >> 16;
            int cr = pv.x >> 16, cc = c_hi;
            bool done = __ballot(unowned != 0) == 0;
            while (!done && cr >= r_lo) {
                const int k = cr * C + cc;
                if (--cc < c_lo) { cc = c_hi; --cr; }
                const crec_t rec = frec + (uint32_t)k * MF_CELL_DOUBLES;
                if (rec[MF_CELL_OFF_STATUS] != 0.0) continue;
                const uint32_t pass = cell_mask_test(rec, xs0, yy, x0, y, unowned);
                if (__ballot(pass != 0) == 0) continue;
                unowned &= ~pass;
                cell_coords<true>(rec, xs0, yy, x0, pass, u, v);
                done = __ballot(unowned != 0) == 0;
            }
        } else {
            // Several cells share the footprint.  (a) their inverse homographies go to LDS; (b) ownership is
            // resolved per pixel, last cell first: a float32 evaluation of the cell's four edge functions
            // decides unless the pixel is within the float32 error band of a mask edge, then the float64 test; (c) every
            // pixel computes its coordinates ONCE with its owner's matrix read from LDS.
            int ne = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t d = i < 2 ? pv.x : i < 4 ? pv.y : i < 6 ? pv.z : pv.w;
                if (ne == i && ((d >> (16 * (i & 1))) & MF_PLAN_VALID)) ne = i + 1;
            }
            // (a) entry e's nine doubles are 18 consecutive dwords of its record: lanes 0..19 copy them (and two dwords of padding)
            // straight into row e of s_hi, one global->LDS load per entry with a scalar base address -- no per-lane cell lookup
            if (lane < 20) {
                uint32_t lo4 = (uint32_t)lane << 2;
            asm("" : "+v"(lo4));                        // (opaque: keeps the scalar base + 32-bit lane offset addressing form)
#pragma unroll 1
                for (int e = 0; e < ne; ++e) {
                    const uint32_t d = e < 2 ? pv.x : e < 4 ? pv.y : e < 6 ? pv.z : pv.w;
                    const uint32_t k = (d >> (16 * (e & 1))) & 0xFFFu;
                    const uint8_t* __restrict__ g = (const uint8_t*)(uintptr_t)(frec + k * MF_CELL_DOUBLES + MF_CELL_OFF_HI);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + lo4),
                                                     (__attribute__((address_space(3))) void*)lds_ptr(&s_hi[wave][e][0]), 4, 0, 0);
                }
            }
            uint32_t own[4];                                            // byte offset of the owner's matrix row (OWN_ROW * entry)
            if (!(rg & MF_REGION_DEEP) && lane < 10) {                  // only uncertified footprints can have uncovered pixels
                int Wp = W + 1, Hp = H + 1;                              // (opaque: keeps the conversions inside this branch)
                asm volatile("" : "+s"(Wp), "+s"(Hp));
                s_hi[wave][8][lane] = lane == 2 ? (double)Wp : lane == 5 ? (double)Hp : lane == 8 ? 1.0 : 0.0;
            }
            const float yf = (float)y, xf0 = (float)x0;
            // The common shape -- exactly two cells, each with ONE mask edge crossing the footprint (a footprint on the
            // border between two cells): one fma per pixel and cell decides, straight-line.
            const uint32_t cd0 = pv.z & 0x3Fu, cd1 = (pv.z >> 16) & 0x3Fu, cd2 = pv.w & 0x3Fu, cd3 = (pv.w >> 16) & 0x3Fu;
            const bool pair = ne == 2 && !(pv.x & MF_PLAN_IN) && !((pv.x >> 16) & MF_PLAN_IN) && cd0 < 4u && cd1 < 4u;
            // four cells around a mesh vertex, each with the two edges that meet there uncertain
            const bool quad = ne == 4 && !((pv.x | (pv.x >> 16) | pv.y | (pv.y >> 16)) & MF_PLAN_IN) &&
                              (cd0 & cd1 & cd2 & cd3 & 8u) != 0;
            bool general = !(pair || quad);
            if (quad) {
                float near = 1e30f;
#pragma unroll
                for (int j = 0; j < 4; ++j) own[j] = OWN_NONE;
#pragma unroll
                for (int i = 3; i >= 0; --i) {                  // first entry last: it wins
                    const uint32_t ent = (i < 2 ? pv.x : pv.y) >> (16 * (i & 1));
                    const uint32_t cd = i == 0 ? cd0 : i == 1 ? cd1 : i == 2 ? cd2 : cd3;
                    const cedge_t ed = fedge + (ent & 0xFFFu) * MF_EDGE_FLOATS;
                    const cedge_t e1 = ed + 3u * (cd & 3u);
                    const cedge_t e2 = ed + 3u * ((cd >> 4) & 3u);
                    const float r1 = __builtin_fmaf(e1[1], yf, e1[2]), r2 = __builtin_fmaf(e2[1], yf, e2[2]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xf = xf0 + (float)j;
                        const float g = fminf(__builtin_fmaf(e1[0], xf, r1), __builtin_fmaf(e2[0], xf, r2));
                        own[j] = g > EDGE_BAND ? OWN_ROW * (uint32_t)i : own[j];
                        near = fminf(near, fabsf(g));
                    }
                }
                general = __ballot(!(near > EDGE_BAND) && active) != 0;
            }
            if (pair) {
                const cedge_t eb = fedge + (pv.x & 0xFFFu) * MF_EDGE_FLOATS + 3u * cd0;            // later cell: wins
                const cedge_t ea = fedge + ((pv.x >> 16) & 0xFFFu) * MF_EDGE_FLOATS + 3u * cd1;
                const float rb = __builtin_fmaf(eb[1], yf, eb[2]), ra = __builtin_fmaf(ea[1], yf, ea[2]);
                float near = 1e30f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xf = xf0 + (float)j;
                    const float gb = __builtin_fmaf(eb[0], xf, rb), ga = __builtin_fmaf(ea[0], xf, ra);
                    own[j] = gb > EDGE_BAND ? 0u : (ga > EDGE_BAND ? OWN_ROW : OWN_NONE);
                    near = fminf(near, fminf(fabsf(gb), fabsf(ga)));
                }
                // a pixel inside the float32 error band of a mask edge (or NaN coefficients): the general path decides exactly
                general = __ballot(!(near > EDGE_BAND) && active) != 0;
            }
            if (general) {
            uint32_t unowned = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                own[j] = OWN_NONE;
                if (x0 + j < W && y < H) unowned |= 1u << j;
            }
            bool done = __ballot(unowned != 0) == 0;
#pragma unroll 1
            for (int i = 0; i < ne && !done; ++i) {
                const uint32_t d = i < 2 ? pv.x : i < 4 ? pv.y : i < 6 ? pv.z : pv.w;
                const uint32_t e = (d >> (16 * (i & 1))) & 0xFFFFu;
                const uint32_t k = e & 0xFFFu;
                uint32_t pass = unowned;                                   // IN: every unowned pixel passes
                if (!(e & MF_PLAN_IN)) {
                    const cedge_t ed = fedge + k * MF_EDGE_FLOATS;
                    // short lists carry an edge code: only one of the four edge functions can fail in this footprint
                    const uint32_t code = ne <= 4 ? (((i < 2 ? pv.z : pv.w) >> (16 * (i & 1))) & 0x3Fu) : 4u;
                    uint32_t ok = 0, amb = 0;
                    if (code < 4u) {
                        const cedge_t e1 = ed + 3u * code;
                        const float rr = __builtin_fmaf(e1[1], yf, e1[2]);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float g = __builtin_fmaf(e1[0], xf0 + (float)j, rr);
                            ok |= g > EDGE_BAND ? (1u << j) : 0u;
                            amb |= ((g > EDGE_BAND) | (g < -EDGE_BAND)) ? 0u : (1u << j);
                        }
                    } else {
                        const float r0 = __builtin_fmaf(ed[1], yf, ed[2]), r1 = __builtin_fmaf(ed[4], yf, ed[5]);
                        const float r2 = __builtin_fmaf(ed[7], yf, ed[8]), r3 = __builtin_fmaf(ed[10], yf, ed[11]);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float xf = xf0 + (float)j;
                            const float g = fminf(fminf(__builtin_fmaf(ed[0], xf, r0), __builtin_fmaf(ed[3], xf, r1)),
                                                  fminf(__builtin_fmaf(ed[6], xf, r2), __builtin_fmaf(ed[9], xf, r3)));
                            ok |= g > EDGE_BAND ? (1u << j) : 0u;
                            amb |= ((g > EDGE_BAND) | (g < -EDGE_BAND)) ? 0u : (1u << j);     // NaN (irregular cell) -> ambiguous
                        }
                    }
                    amb &= unowned;
                    if (__ballot(amb != 0) != 0)
                        ok = (ok & ~amb) | cell_mask_test(frec + k * MF_CELL_DOUBLES, xs0, yy, x0, y, amb);
                    pass = ok & unowned;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) own[j] = ((pass >> j) & 1u) ? OWN_ROW * (uint32_t)i : own[j];
                unowned &= ~pass;
                done = __ballot(unowned != 0) == 0;
            }
            }
            // (c) coordinates, once per pixel, owner's matrix from LDS.  Optimistic: the
            // trimmed reciprocal is applied straight away (keeps one pixel's intermediates live instead of four) and the
            // rare footprint with a denominator outside [0.5, 2) is redone with the generic division.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the matrices (and the window, issued before them) have landed
            uint32_t eor = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double* hp = reinterpret_cast<const double*>(reinterpret_cast<const uint8_t*>(&s_hi[wave][0][0]) + own[j]);
                const double2 h01 = *reinterpret_cast<const double2*>(hp), h23 = *reinterpret_cast<const double2*>(hp + 2);
                const double2 h45 = *reinterpret_cast<const double2*>(hp + 4), h67 = *reinterpret_cast<const double2*>(hp + 6);
                const double h8 = hp[8];
                const double xs = xs0 + (double)j;
                const double w = (xs * h67.x + yy * h67.y) + h8;
                const double nx = (xs * h01.x + yy * h01.y) + h23.x;
                const double ny = (xs * h23.y + yy * h45.x) + h45.y;
                eor |= (uint32_t)__builtin_amdgcn_frexp_exp(w);
                const double iw = recip_unit_range(w);
                const float un = (float)(nx * iw), vn = (float)(ny * iw);
                u[j] = un;
                v[j] = vn;
            }
            if (__ballot(eor > 1u) != 0) {                             // far-from-affine cell: generic division
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double* hp = reinterpret_cast<const double*>(reinterpret_cast<const uint8_t*>(&s_hi[wave][0][0]) + own[j]);
                    const double xs = xs0 + (double)j;
                    const double w = (xs * hp[6] + yy * hp[7]) + hp[8];
                    const bool ok = fabs(w) > 1.1920928955078125e-07;
                    const double iw = 1.0 / w;
                    u[j] = ok ? (float)(((xs * hp[0] + yy * hp[1]) + hp[2]) * iw) : 0.0f;
                    v[j] = ok ? (float)(((xs * hp[3] + yy * hp[4]) + hp[5]) * iw) : 0.0f;
                }
            }
        }

        if (SCAN || MAPS) {
            // The crop-boundary scan alone, mfs.py:1075-1098 (the same tests as on the generic path below; there they run only when
            // some pixel of the footprint is not deep inside the frame -- a pixel that is cannot pass any of them).  MAPS: the same
            // fold, then the coordinates themselves.
            int c_left = 0, c_top = 0, c_right = W - 1, c_bottom = H - 1;
            if (active) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = x0 + j;
                    if (x < W) {
                        if (fabsf(u[j]) < 1.0f) c_left = max(c_left, x);
                        if (fabsf(u[j] - fWm1) < 1.0f) c_right = min(c_right, x);
                        if (fabsf(v[j]) < 1.0f) c_top = max(c_top, y);
                        if (fabsf(v[j] - fHm1) < 1.0f) c_bottom = min(c_bottom, y);
                    }
                }
            }
            const bool any = c_left != 0 || c_top != 0 || c_right != W - 1 || c_bottom != H - 1;
            if (__ballot(any) != 0) {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    c_left = max(c_left, __shfl_xor(c_left, off));
                    c_top = max(c_top, __shfl_xor(c_top, off));
                    c_right = min(c_right, __shfl_xor(c_right, off));
                    c_bottom = min(c_bottom, __shfl_xor(c_bottom, off));
                }
                if (lane == 0) {
                    // (per frame, mfs.py:1075-1098, and straight into the clip-level rectangle, mfs.py:1103-1106)
                    if (c_left != 0) { atomicMax(&crop[4 * f + 0], c_left); atomicMax(&clip[0], c_left); }
                    if (c_top != 0) { atomicMax(&crop[4 * f + 1], c_top); atomicMax(&clip[1], c_top); }
                    if (c_right != W - 1) { atomicMin(&crop[4 * f + 2], c_right); atomicMin(&clip[2], c_right); }
                    if (c_bottom != H - 1) { atomicMin(&crop[4 * f + 3], c_bottom); atomicMin(&clip[3], c_bottom); }
                }
            }
            if constexpr (MAPS) maps_store_f32(u, v, f, x0, y, active, W, H, reinterpret_cast<float*>(out));
            return;
        }
        if constexpr (U16) {
            remap_store_u16(u, v, f, x0, y, active, W, H, reinterpret_cast<const uint16_t*>(frames), reinterpret_cast<uint16_t*>(out), border16,
                            crop, clip);
            return;
        }
        if constexpr (PLANE) {
            remap_store_plane<PX, true>(u, v, f, x0, y, active, W, H, frames, out, border16, crop, clip);
            return;
        }
        if constexpr (GREY) {
            remap_store_u8c1(u, v, f, x0, y, active, W, H, frames, out, border, crop, clip, gwin, &s_src[0]);
            return;
        }
        if constexpr (C4) {
            remap_store_u8c4(u, v, f, x0, y, active, W, H, frames, out, border, crop, clip, gwin, &s_src[0]);
            return;
        }
        // cv2.remap: 1/32-pixel fixed point (round half to even), bilinear gather, store.
        uint32_t bx[4], by[4];
        fixed_point(u, v, bx, by);
        bool fast = true;
        if (!(staged && (rg & MF_REGION_DEEP))) {        // (DEEP: every pixel has an owner and every tap is deep inside: nothing to check)
            uint32_t dxm = 0, dym = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dxm = max(dxm, bx[j] - (0x4B400000u + 64u));
                dym = max(dym, by[j] - (0x4B400000u + 64u));
            }
            // "deep interior": 2 <= ix <= W-3 and 2 <= iy <= H-3 for all four pixels.  Then both taps in x and
            // y are inside the frame, the 8-byte loads stay inside the row, and no crop flag can be set
            // (u >= 2 - 1/64 and u < W - 2, same for v).
            // (a frame of fewer than five columns or rows has no such pixel: the bounds would wrap around as unsigned numbers)
            const bool deep = W >= 5 && H >= 5 && dxm <= (uint32_t)(32 * (W - 3) + 31 - 64) && dym <= (uint32_t)(32 * (H - 3) + 31 - 64);
            fast = __ballot(active && !deep) == 0;
        }
        uint3 d;                                                        // the lane's 12 output bytes
        if (staged) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the window has landed in LDS
        if (fast) {
            // fast path (wave-uniform): every pixel of the footprint samples the deep interior
            if (active) {
                if (staged) {
                    d = gather_blend_window(compact, bx, by, lds_origin);
                } else {
                    uint2 a[4], b[4];
                    gather_global(bx, by, src, W, a, b);
                    d = blend(bx, by, a, b);
                }
            }
        } else {
            // generic path: frame borders, uncovered pixels, crop flags, out-of-range coordinates (3 % of a stabilised clip's
            // footprints -- the ring along the frame border whose pixels sample outside the frame)
            int c_left = 0, c_top = 0, c_right = W - 1, c_bottom = H - 1;
            if (active) {
            // sx = rint(32 u) sits in the low bits of fixed_point's raw floats while |sx| < 2^22; coordinates beyond that (a cell far
            // from affine) take cv2's own rounding with its saturation
            uint32_t spread = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                spread = max(spread, max(bx[j] - (0x4B400000u - 0x200000u), by[j] - (0x4B400000u - 0x200000u)));
            const bool narrow = __ballot(spread >= 0x400000u) == 0;
            const bool has_tail = limit != 0xFFFFFFFFu;      // last frame of the stack: the 4-byte load of its last pixel is shifted back
            uint32_t oB[4], oG[4], oR[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float uu = u[j], vv = v[j];
                const int x = x0 + j;
                // crop-boundary scan, mfs.py:1075-1098: |u - e| < 1.  The float32 differences are exact
                // whenever they are smaller than 1 in magnitude (Sterbenz), so the tests are exact.
                if (x < W) {                                 // (a lane's last pixels may lie beyond the frame when W % 4 != 0)
                    if (fabsf(uu) < 1.0f) c_left = max(c_left, x);
                    if (fabsf(uu - fWm1) < 1.0f) c_right = min(c_right, x);
                    if (fabsf(vv) < 1.0f) c_top = max(c_top, y);
                    if (fabsf(vv - fHm1) < 1.0f) c_bottom = min(c_bottom, y);
                }
                const int sxx = narrow ? (int)(bx[j] - 0x4B400000u) : cv_round_f32(uu * 32.0f);
                const int syy = narrow ? (int)(by[j] - 0x4B400000u) : cv_round_f32(vv * 32.0f);
                const int ix = sxx >> 5, iy = syy >> 5;      // (saturation to int16 cannot change any decision below)
                // The four taps, branch-free: each load goes to the position clamped into the frame and the tap is replaced by the
                // border colour afterwards when it lies outside (a 2 x 2 footprint outside altogether needs no special case: four
                // border-colour taps with weights that sum to 1024 give the border colour exactly).  All sixteen loads of the lane
                // are in flight together.
                const bool in_x0 = (unsigned)ix < (unsigned)W, in_x1 = (unsigned)(ix + 1) < (unsigned)W;
                const bool in_y0 = (unsigned)iy < (unsigned)H, in_y1 = (unsigned)(iy + 1) < (unsigned)H;
                const uint32_t cx0 = (uint32_t)min(max(ix, 0), W - 1), cx1 = (uint32_t)min(max(ix + 1, 0), W - 1);
                if (staged) {
                    // STAGED: the window holds every tap position CLAMPED into the frame (cell_table.hip), so the four taps are LDS
                    // byte loads (a pixel without owner sits at (W+1, H+1): its clamped position may lie outside the window --
                    // whatever the load returns is replaced by the border colour below).  (Unaligned 4-byte LDS loads instead:
                    // +2 % kernel time; two pixels' loads in flight: register spills.)
                    const uint32_t pitch = compact ? (uint32_t)MF_COMPACT_PITCH : (uint32_t)LDS_PITCH;      // (wave-uniform)
                    const uint32_t ra = umad24((uint32_t)min(max(iy, 0), H - 1), pitch, 0u - lds_origin);
                    const uint32_t rb = umad24((uint32_t)min(max(iy + 1, 0), H - 1), pitch, 0u - lds_origin);
                    TapRegs t;
                    taps_clamped(umad24(cx0, 3u, ra), umad24(cx1, 3u, ra), umad24(cx0, 3u, rb), umad24(cx1, 3u, rb), t);
                    const bool i00 = in_x0 && in_y0, i01 = in_x1 && in_y0, i10 = in_x0 && in_y1, i11 = in_x1 && in_y1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const uint32_t bc = (border >> (8 * c)) & 0xFFu;
                        t.lo[c] = i00 ? t.lo[c] : bc;
                        t.hi[c] = i01 ? t.hi[c] : bc << 16;
                        t.lo[3 + c] = i10 ? t.lo[3 + c] : bc;
                        t.hi[3 + c] = i11 ? t.hi[3 + c] : bc << 16;
                    }
                    blend_pixel((uint32_t)sxx, (uint32_t)syy, t, oB[j], oG[j], oR[j]);
                    continue;
                }
                const uint32_t r0 = (uint32_t)min(max(iy, 0), H - 1) * (uint32_t)W, r1 = (uint32_t)min(max(iy + 1, 0), H - 1) * (uint32_t)W;
                const uint32_t o00 = (r0 + cx0) * 3u, o01 = (r0 + cx1) * 3u, o10 = (r1 + cx0) * 3u, o11 = (r1 + cx1) * 3u;
                uint32_t p00, p01, p10, p11;                 // B | G << 8 | R << 16 | (next byte) << 24
                if (has_tail) {
                    const uint32_t k00 = o00 + 4u > limit, k01 = o01 + 4u > limit, k10 = o10 + 4u > limit, k11 = o11 + 4u > limit;
                    __builtin_memcpy(&p00, src + (o00 - k00), 4); p00 >>= 8u * k00;
                    __builtin_memcpy(&p01, src + (o01 - k01), 4); p01 >>= 8u * k01;
                    __builtin_memcpy(&p10, src + (o10 - k10), 4); p10 >>= 8u * k10;
                    __builtin_memcpy(&p11, src + (o11 - k11), 4); p11 >>= 8u * k11;
                } else {
                    __builtin_memcpy(&p00, src + o00, 4);
                    __builtin_memcpy(&p01, src + o01, 4);
                    __builtin_memcpy(&p10, src + o10, 4);
                    __builtin_memcpy(&p11, src + o11, 4);
                }
                p00 = in_x0 && in_y0 ? p00 : border;
                p01 = in_x1 && in_y0 ? p01 : border;
                p10 = in_x0 && in_y1 ? p10 : border;
                p11 = in_x1 && in_y1 ? p11 : border;
                // the blend of the fast path: per channel the two horizontal neighbours in 16-bit fields, both lerped vertically at
                // once, then v_dot2_u32_u16 horizontally (byte 3 of the taps is never selected)
                const uint32_t fy = (uint32_t)syy & 31u, wy = 32u - fy;
                const uint32_t vB = umad24(__builtin_amdgcn_perm(p11, p10, 0x0C040C00u), fy, __umul24(__builtin_amdgcn_perm(p01, p00, 0x0C040C00u), wy));
                const uint32_t vG = umad24(__builtin_amdgcn_perm(p11, p10, 0x0C050C01u), fy, __umul24(__builtin_amdgcn_perm(p01, p00, 0x0C050C01u), wy));
                const uint32_t vR = umad24(__builtin_amdgcn_perm(p11, p10, 0x0C060C02u), fy, __umul24(__builtin_amdgcn_perm(p01, p00, 0x0C060C02u), wy));
                const uint32_t wq = umad24((uint32_t)sxx & 31u, 0x3FFFC0u, 2048u);          // 64 (32 - fx) | 64 fx << 16
                oB[j] = udot2(vB, wq, 32768u);
                oG[j] = udot2(vG, wq, 32768u);
                oR[j] = udot2(vR, wq, 32768u);
            }
            const uint32_t pair = 0x0C0C0602u, pair_hi = 0x06020C0Cu;       // byte 2 of each sum, as in gather_blend_staged
            d.x = __builtin_amdgcn_perm(oB[1], oR[0], pair_hi) | __builtin_amdgcn_perm(oG[0], oB[0], pair);
            d.y = __builtin_amdgcn_perm(oG[2], oB[2], pair_hi) | __builtin_amdgcn_perm(oR[1], oG[1], pair);
            d.z = __builtin_amdgcn_perm(oR[3], oG[3], pair_hi) | __builtin_amdgcn_perm(oB[3], oR[2], pair);
            }
            // Crop bounds (only this path can set one): wave reduction, then at most one atomic per bound and wavefront.
            const bool any = c_left != 0 || c_top != 0 || c_right != W - 1 || c_bottom != H - 1;
            if (__ballot(any) != 0) {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    c_left = max(c_left, __shfl_xor(c_left, off));
                    c_top = max(c_top, __shfl_xor(c_top, off));
                    c_right = min(c_right, __shfl_xor(c_right, off));
                    c_bottom = min(c_bottom, __shfl_xor(c_bottom, off));
                }
                if (lane == 0) {
                    // (per frame, mfs.py:1075-1098, and straight into the clip-level rectangle, mfs.py:1103-1106)
                    if (c_left != 0) { atomicMax(&crop[4 * f + 0], c_left); atomicMax(&clip[0], c_left); }
                    if (c_top != 0) { atomicMax(&crop[4 * f + 1], c_top); atomicMax(&clip[1], c_top); }
                    if (c_right != W - 1) { atomicMin(&crop[4 * f + 2], c_right); atomicMin(&clip[2], c_right); }
                    if (c_bottom != H - 1) { atomicMin(&crop[4 * f + 3], c_bottom); atomicMin(&clip[3], c_bottom); }
                }
            }
        }
        if (active) {                                                   // the lane's 12 output bytes
            const uint32_t o = ((uint32_t)y * (uint32_t)W + (uint32_t)x0) * 3u;
            if (fast_store) {                                           // W % 4 == 0: an active lane's four pixels are all inside
                *reinterpret_cast<uint3*>(dst + o) = d;
            } else if (x0 + 3 < W) {                                    // all four inside, at a byte address of any alignment: one unaligned 12-byte store
                __builtin_memcpy(dst + o, &d, 12);
            } else {
                const int nb = 3 * min(4, W - x0);                       // W % 4 != 0: byte by byte, up to the row end
#pragma unroll 1
                for (int k = 0; k < nb; ++k) {
                    const uint32_t word = k < 4 ? d.x : k < 8 ? d.y : d.z;
                    dst[o + k] = (uint8_t)(word >> (8 * (k & 3)));
                }
            }
        }
    }
}

}  // namespace mf
#endif  // MF_WARP_BODY_H
