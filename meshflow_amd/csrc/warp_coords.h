// The warp kernels' constants and coordinate code (device only, included through warp_body.h): a lane's four source coordinates from a cell's
// inverse homography, the exact mask test, cv2.remap's fixed point, and what every consumer derives from the coordinates.
#ifndef MF_WARP_COORDS_H
#define MF_WARP_COORDS_H
#include "mf_common.h"

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

// ---- what every consumer of the coordinates derives from them: deep interior, exact fixed point, clamped taps, the crop fold -----------
// "Deep interior": 2 <= ix <= W-3 and 2 <= iy <= H-3 for all four pixels of the lane (bx / by: fixed_point's raw floats).  Then both taps in
// x and y are inside the frame, the loads of a tap row stay inside the row, and no crop flag can be set (u >= 2 - 1/64 and u < W - 2, same
// for v).  (A frame of fewer than five columns or rows has no such pixel: the bounds would wrap around as unsigned numbers.)
__device__ __forceinline__ bool deep_interior(const uint32_t (&bx)[4], const uint32_t (&by)[4], int W, int H)
{
    uint32_t dxm = 0, dym = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dxm = max(dxm, bx[j] - (0x4B400000u + 64u));
        dym = max(dym, by[j] - (0x4B400000u + 64u));
    }
    return W >= 5 && H >= 5 && dxm <= (uint32_t)(32 * (W - 3) + 31 - 64) && dym <= (uint32_t)(32 * (H - 3) + 31 - 64);
}

// sx = rint(32 u) sits in the low bits of fixed_point's raw floats while |sx| < 2^22: narrow_coords (wave-uniform) tells whether that holds
// for every pixel of the wavefront; coordinates beyond that (a cell far from affine) take cv2's own rounding with its saturation.
__device__ __forceinline__ bool narrow_coords(const uint32_t (&bx)[4], const uint32_t (&by)[4])
{
    uint32_t spread = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        spread = max(spread, max(bx[j] - (0x4B400000u - 0x200000u), by[j] - (0x4B400000u - 0x200000u)));
    return __ballot(spread >= 0x400000u) == 0;
}
// ... and one coordinate's fixed point by that answer: from its raw float `b`, or from the coordinate `c` itself
__device__ __forceinline__ int fixed_coord(bool narrow, uint32_t b, float c)
{
    return narrow ? (int)(b - 0x4B400000u) : cv_round_f32(c * 32.0f);
}

// The 2 x 2 taps of a pixel that is not deep inside, at (ix, iy): which columns and rows lie inside the frame, and every position clamped
// into it -- each load goes to the clamped position, and a tap that lies outside is replaced by the border value afterwards.
struct ClampedTaps {
    bool in_x0, in_x1, in_y0, in_y1;
    uint32_t cx0, cx1, r0, r1;                  // columns; rows as offsets in pixels (row * W)
};
__device__ __forceinline__ ClampedTaps clamped_taps(int ix, int iy, int W, int H)
{
    ClampedTaps t;
    t.in_x0 = (unsigned)ix < (unsigned)W; t.in_x1 = (unsigned)(ix + 1) < (unsigned)W;
    t.in_y0 = (unsigned)iy < (unsigned)H; t.in_y1 = (unsigned)(iy + 1) < (unsigned)H;
    t.cx0 = (uint32_t)min(max(ix, 0), W - 1); t.cx1 = (uint32_t)min(max(ix + 1, 0), W - 1);
    t.r0 = (uint32_t)min(max(iy, 0), H - 1) * (uint32_t)W; t.r1 = (uint32_t)min(max(iy + 1, 0), H - 1) * (uint32_t)W;
    return t;
}

// The crop bounds of a wavefront from its lanes' (each lane's four edge tests of mfs.py:1075-1098 stay with the caller, next to its pixel
// loop): wave reduction, then at most one atomic per bound and wavefront -- per frame, mfs.py:1075-1098, and straight into the clip-level
// rectangle, mfs.py:1103-1106.
__device__ __forceinline__ void crop_fold(int c_left, int c_top, int c_right, int c_bottom, uint32_t f, int W, int H,
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

}  // namespace mf
#endif  // MF_WARP_COORDS_H
