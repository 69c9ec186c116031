// Kernel 2b: per-frame, per-cell mesh warp with the crop-boundary scan folded in.
//
// Reference (meshflowstabilizer.py, "mfs.py"): for every frame, every mesh cell in row-major order warps a
// full-frame float64 mask (cv2.warpPerspective, mfs.py:1050-1052), transforms ALL pixel coordinates with
// the cell's inverse homography (cv2.perspectiveTransform, mfs.py:1054) and merges them into the frame's
// coordinate map under that mask (np.where, mfs.py:1060-1061); one cv2.remap (bilinear, constant border,
// mfs.py:1063-1069) and four edge scans (mfs.py:1075-1098) follow.  O(R*C*H*W) per frame.
//
// This kernel computes the same result in one pass over output pixels:
//   owner(pixel) = LAST cell in row-major order whose mask test passes  (painter merge)
//   (u, v)       = float32( Hi_owner * (x, y, 1) ), or (W+1, H+1) when no cell covers the pixel
//   crop flags   = |u| < 1, |u-(W-1)| < 1, |v| < 1, |v-(H-1)| < 1  -> atomic max/min per frame
//   out          = cv2.remap fixed-point bilinear of the source frame at (u, v)
// Coordinates are float64 exactly as OpenCV evaluates them (no FMA contraction: -ffp-contract=off), then
// float32, then 1/32-pixel fixed point; interpolation is integer.  The result is bit-identical to the CPU
// oracle (oracle/warp_oracle.c).
//
// Mapping (gfx950).  One wavefront = one workgroup = one 32 x 8 pixel "footprint" of one frame; a lane owns 4 consecutive pixels
// of one row (12 contiguous output bytes -> one global_store_dwordx3).  Grid = (8 * per_xcd, frames): footprints are handed out
// XCD-aware (mf_common.h WarpGeom).  Per footprint:
//   1. footprint_plan_kernel (cell_table.hip) wrote the wave-uniform PLAN (two scalar loads): up to 8 candidate cells in
//      descending order, each IN (all 256 pixels pass its mask test) or MIXED, with -- for short lists -- the one or two mask
//      edges that can fail; the footprint's SOURCE REGION, the window of the source frame that holds every bilinear tap of
//      every pixel, ready-made as LDS origin + first dword in the frame; and certificates: STAGED, DEEP (the footprint lies in
//      the frame, every pixel has an owner and every tap is interior), UNIT (the projective denominator stays in (0.52, 1.9)
//      and varies slowly enough for the reciprocal guess), and the two path bits HOT and PAIR.
//   2. The window goes to LDS asynchronously: two global_load_lds_dwordx4 per lane, issued first, awaited after the
//      coordinate arithmetic.
//   3. HOT (one IN cell, everything certified; ~65 % of footprints at config-2 geometry): straight-line code.  The cell's Hi
//      comes in through scalar loads; 1/w: pixel 0 by v_rcp_f64 + Newton + the residual correction that makes it the IEEE
//      quotient; pixels 1..3 start from pixel 0's reciprocal (second-order guess + ONE Newton step + the same correction).
//   4. PAIR (two cells, ~27 %): the later cell wins where ONE of its mask edges passes (one float32 fma per pixel), the other
//      owns the rest; both Hi go to LDS by global->LDS DMA (one 80-byte load per cell, scalar base address) and a pixel's
//      owner is the byte offset of its matrix row.  A pixel inside the float32 error band of the edge sends the wavefront to 5.
//      MULTI (two to four cells with one- or two-edge codes -- the four cells around a mesh vertex; ~3 %, 14 % with a 32 x 32
//      mesh): the same with up to two edge functions per cell; coverage is checked at run time (a pixel without owner -> 5).
//   5. Everything else: the general last-cell-first loop over the list.  A pixel inside the error band of an edge is decided
//      by a division-free float64 comparison, and by OpenCV's exact arithmetic (division, rint) only within 1e-6 of the edge;
//      "no owner" is a ninth LDS row holding the matrix that maps every pixel to (W+1, H+1) -- the coordinate code has no
//      special case.  Footprints the plan could not certify (frame border, uncovered pixels, oversized or unaligned windows)
//      check per pixel and use either two unaligned 8-byte global loads per pixel or the per-tap path with border colour and
//      crop flags (branch-free: loads at positions clamped into the frame, border colour selected afterwards).
//   6. cv2.remap: sx = rint(32u) via one fma against 1.5*2^23; taps = LDS byte loads straight into the blend's layout (the two
//      horizontal neighbours of a channel in the 16-bit halves of a register); v_mul_u32_u24 + v_mad_u32_u24 lerp both halves
//      vertically at once, v_dot2_u32_u16 lerps horizontally with weights scaled so that the rounded byte lands in byte 2; six
//      v_perm_b32 + three v_or_b32 gather the lane's 12 output bytes.
// Algorithmic HBM traffic: 2*H*W*3 bytes per frame (each source byte read once, each output byte written once); measured
// 1.05x that.  No dense contraction: no MFMA.  What bounds it: vector AND scalar instruction issue, not HBM -- DESIGN.md
// section 4.3, profiles/r02_phase_profile.txt.  Everything a wavefront needs before its pixels is therefore host-made
// (WarpGeom) or plan-made (FootRegion): the hot path issues 222 vector and 74 scalar instructions per wavefront.  The float32
// edge functions come scaled by their own evaluation error bound (cell_table.hip): beyond +-1 their sign is exact.
#include "warp_body.h"
#include <stdlib.h>

#include <algorithm>
#include <atomic>

namespace mf {

// Launch constants of warp_kernel / crop_scan_kernel; returns the frames one launch may cover (the grid's y extent, and 32-bit byte
// offsets into the plan -- 16 B per footprint -- and the records), 0 when a single frame is already too large.
static uint32_t make_warp_geom(int W, int H, int R, int C, WarpGeom& g)
{
    const uint32_t nfx = (uint32_t)((W + FOOT_W - 1) / FOOT_W), nfy = (uint32_t)((H + FOOT_H - 1) / FOOT_H);
    const FastDiv by_row = make_fast_div(nfx);
    g.per_frame = nfx * nfy;
    g.per_xcd = (g.per_frame + 7u) / 8u;
    g.nfx = nfx;
    g.div_m = by_row.m; g.div_s = by_row.s; g.div_pass = nfx == 1u ? 0xFFFFFFFFu : 0u;
    g.frame_bytes = 3u * (uint32_t)W * (uint32_t)H;
    g.row_bytes = 3u * (uint32_t)W;
    g.rec_frame_bytes = (uint32_t)(R * C) * (uint32_t)(MF_CELL_DOUBLES * sizeof(double));
    g.edge_frame_bytes = (uint32_t)(R * C) * (uint32_t)(MF_EDGE_FLOATS * sizeof(float));
    // cell column under pixel x of the unwarped grid ~ floor(x C / (W - 1)) = mulhi(x, 2^32 C / (W - 1)) (a guess: the plan decides)
    g.cell_mul_x = (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, (((uint64_t)C) << 32) / (uint64_t)(W - 1));
    g.cell_mul_y = (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, (((uint64_t)R) << 32) / (uint64_t)(H - 1));
    g.mesh_cols = (uint32_t)C;
    g.cell_last = (uint32_t)(R * C - 1);
    const uint64_t cap = 0xFFFFFFFFull;
    uint64_t per_launch = 65535;
    per_launch = per_launch < cap / (16ull * g.per_frame) ? per_launch : cap / (16ull * g.per_frame);
    per_launch = per_launch < cap / g.rec_frame_bytes ? per_launch : cap / g.rec_frame_bytes;
    return (uint32_t)per_launch;
}

template <bool STAGE_OK>
__global__ __launch_bounds__(64) MF_WARP_ATTR void warp_kernel(const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions,
                                                               WarpGeom g, const uint8_t* __restrict__ frames,
                                                               const double* __restrict__ records, uint8_t* __restrict__ out,
                                                               const float* __restrict__ edges, int n, int W,
                                                               int H, int C, uint32_t border, int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    // XCD-aware footprint order.  Workgroups go to the 8 XCDs round-robin by linear id (blockIdx.x first: gridDim.x is a multiple of
    // 8), and each XCD has its own L2: in raster order the four neighbours of a footprint -- whose staged windows overlap its own
    // by 60 % -- would all run on other XCDs and each L2 would fetch the shared rows again.  Workgroup L of frame blockIdx.y
    // therefore takes footprint (L % 8) * per_xcd + L / 8: every XCD sweeps one contiguous eighth of each frame in raster order.
    // (Everything up to the plan is scalar, with host-made constants and 32-bit offsets: the scalar unit is as loaded as the vector
    // unit in this kernel -- profiles/README.md -- and every s_ instruction here is paid by each of the 2.4 M wavefronts of a clip.)
    const uint32_t f = blockIdx.y;
    // The eighth an XCD sweeps ROTATES with the frame: the footprints along the top and bottom frame border are the expensive ones
    // (per-tap path, crop flags: 2.5 x the average), and with a fixed assignment they all land on XCD 0 and XCD 7, which then
    // finish 9 % after the others (-2.1 % kernel time at config 2, -4 % on the all-hot probe).
    const uint32_t t = ((blockIdx.x + f) & 7u) * g.per_xcd + (blockIdx.x >> 3);
    if (t >= g.per_frame) return;
    footprint_body<Px::U8C3, STAGE_OK, false>(f, t, plan, regions, g, frames, records, out, edges, n, W, H, C, border, crop, clip);
}

// The mesh warp of uint16 frames: warp_kernel's footprint order and ownership / coordinate code (footprint_body's general path: the staged
// windows are sized for 3-byte pixels), cv2.remap's CV_16UC3 arithmetic at the end (remap_store_u16).  The same d_crop rows and clip
// rectangle as warp_kernel on the same table.
__global__ __launch_bounds__(64) void warp16_footprint(const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions,
                                                       WarpGeom g, const uint16_t* __restrict__ frames,
                                                       const double* __restrict__ records, uint16_t* __restrict__ out,
                                                       const float* __restrict__ edges, int n, int W,
                                                       int H, int C, uint64_t border16, int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint32_t f = blockIdx.y;
    const uint32_t t = ((blockIdx.x + f) & 7u) * g.per_xcd + (blockIdx.x >> 3);
    if (t >= g.per_frame) return;
    footprint_body<Px::U16C3, false, false>(f, t, plan, regions, g, reinterpret_cast<const uint8_t*>(frames), records, reinterpret_cast<uint8_t*>(out),
                                            edges, n, W, H, C, 0u, crop, clip, border16);
}

// The crop-boundary scan WITHOUT the pixels (mfs.py:1075-1106 depends on the coordinate maps only, i.e. on the cell table): fills
// crop[f] exactly as warp_kernel does, from the footprints that can set a flag at all.  A wavefront looks at SCAN_GROUP consecutive
// footprints (one lane each reads the footprint's region word: anything the plan certified as DEEP or NOFLAG cannot pass any of
// the four tests) and then runs footprint_body<SCAN> -- ownership and coordinates of the general path, nothing else -- on the
// remaining ones, one after the other: ~4 % of the footprints of a stabilised 1080p clip (the ring along the frame border).
// A host that knows the clip-level rectangle before the first pixel moves can crop + resize each chunk right behind its warp
// (csrc/hostpipe.hip) and, at N > 1, overlap the 16-byte all-reduce with the warp.
constexpr uint32_t SCAN_GROUP = 16;
__global__ __launch_bounds__(64) void crop_scan_kernel(const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions,
                                                       WarpGeom g, const double* __restrict__ records, const float* __restrict__ edges,
                                                       uint32_t total, int n, int W, int H, int C, int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint32_t base = blockIdx.x * SCAN_GROUP, mine = base + threadIdx.x;
    bool need = false;
    if (threadIdx.x < SCAN_GROUP && mine < total) need = (regions[mine].flags_origin & (MF_REGION_DEEP | MF_REGION_NOFLAG)) == 0;
    uint64_t todo = __ballot(need);
    while (todo) {
        const uint32_t bit = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1;
        const uint32_t fp = __builtin_amdgcn_readfirstlane(base + bit);
        const uint32_t f = fp / g.per_frame, t = fp - f * g.per_frame;
        footprint_body<Px::U8C3, false, true>(f, t, plan, regions, g, nullptr, records, nullptr, edges, n, W, H, C, 0u, crop, clip);
        __builtin_amdgcn_wave_barrier();             // (the next footprint reuses the wavefront's s_hi rows)
    }
}

// ---- device self-tests of the coordinate arithmetic, and the d16 probe ----------------------------------------------------------------
// (In this translation unit, between the kernels above and crop_reduce_kernel, on purpose: d16_probe_kernel reaches its result variable
// by an offset from its own place in the code object, and the last kernel of a code object takes the end-of-text padding into its
// listing -- in a file of their own, tools/isa_compare.py reports these kernels as changed.)

// Self-test of recip_unit_range against IEEE division: counts mismatching bit patterns.
__global__ void selftest_recip_kernel(unsigned long long n, unsigned long long seed, unsigned long long* mismatches)
{
    unsigned long long bad = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long z = (i + seed) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        // mantissa from the hash, exponent -1 or 0 (|w| in [0.5, 2)), random sign; a few exact end points
        unsigned long long bits = (z & 0x800FFFFFFFFFFFFFull) | ((0x3FEull + ((z >> 52) & 1ull)) << 52);
        if ((i & 0xFFFFF) == 0) bits = 0x4000000000000000ull;             // 2.0
        if ((i & 0xFFFFF) == 1) bits = 0x3FE0000000000000ull;             // 0.5
        const double w = __longlong_as_double((long long)bits);
        const double a = recip_unit_range(w);
        const double b = 1.0 / w;
        if (__double_as_longlong(a) != __double_as_longlong(b)) ++bad;
        // the neighbour-pixel route: w_j = w + j h6 with |h6| / w^2 up to the limit the kernel accepts (a second hash draws h6)
        unsigned long long z2 = (z ^ 0xD6E8FEB86659FD93ull) * 0x9E3779B97F4A7C15ull;
        z2 ^= z2 >> 29;
        const double frac = (double)(long long)(z2 >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;        // (-1, 1)
        const double scale = (i & 7) == 0 ? 1.0 : (double)((z2 & 1023) + 1) * (1.0 / 1024.0);                // often small, sometimes the limit
        const double h6 = frac * scale * RECIP_GUESS_LIMIT * (w * w);
        const double c1 = h6 * (a * a), c2 = (h6 * c1) * a;
        if (fabs(c1) <= RECIP_GUESS_LIMIT) {
            const double j = (double)(1 + (int)(z2 % 3));
            const double wj = w + j * h6;
            if (fabs(wj) >= 0.5 && fabs(wj) < 2.0) {
                const double g = recip_from_guess(wj, recip_guess(a, c1, c2, j));
                const double q = 1.0 / wj;
                if (__double_as_longlong(g) != __double_as_longlong(q)) ++bad;
            }
        }
    }
    if (bad) atomicAdd(mismatches, bad);
}

int launch_selftest_recip(unsigned long long n, unsigned long long seed, unsigned long long* d_mismatches, hipStream_t st)
{
    hipLaunchKernelGGL(selftest_recip_kernel, dim3(2048), dim3(256), 0, st, n, seed, d_mismatches);
    return hip_fail(hipGetLastError(), "selftest_recip_kernel launch");
}

// Self-test of the cheap coordinate chain (coords_fast) against cv2.perspectiveTransform's own arithmetic on hashed matrices
// and positions that satisfy the plan's MF_PLAN_FAST64 / UNIT / DEEP premises: `missed` counts float32 results that differ from
// the exact chain's WITHOUT their midpoint key raising the flag (must be 0), `flagged` the values whose key did (the fallback rate).
// (`margin`, optional: the largest distance between a cheap value and the exact chain's, in float64 ulps of the latter, as double bits)
__global__ void selftest_fast64_kernel(unsigned long long n, unsigned long long seed, unsigned long long* counters, unsigned long long* margin)
{
    unsigned long long missed = 0, flagged = 0, tested = 0;
    double far = 0.0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long z = (i + seed) * 0x9E3779B97F4A7C15ull;
        double r[11];
        for (int q = 0; q < 11; ++q) {                          // eleven uniform draws in (-1, 1)
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            r[q] = (double)(long long)(z >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
            z += 0x9E3779B97F4A7C15ull;
        }
        // near-identity inverse homography with shift, shear and perspective terms up to what the certificates admit
        const double amp = (i & 3) == 0 ? 1.0 : 0.1;             // a quarter of the cases at the limits
        double Hi[9] = { 1.0 + 0.2 * amp * r[0], 0.2 * amp * r[1], 80.0 * r[2], 0.2 * amp * r[3], 1.0 + 0.2 * amp * r[4], 80.0 * r[5],
                         2.0e-4 * amp * r[6], 2.0e-4 * amp * r[7], 1.0 + 0.3 * amp * r[10] };
        const double xs0 = (double)(4 * (int)((r[8] * 0.5 + 0.5) * 2047.0)), yy = (double)(int)((r[9] * 0.5 + 0.5) * 8191.0);
        // the premises, in float64 on the lane's four pixels (the plan checks them on the footprint's corners); half of the cases
        // step along y (the transposed lanes of the pair path)
        const bool vert = ((i >> 2) & 1) != 0;
        const double x0d = vert ? (double)(int)((r[8] * 0.5 + 0.5) * 8191.0) : xs0, y0d = vert ? (double)(4 * (int)((r[9] * 0.5 + 0.5) * 2047.0)) : yy;
        bool ok = true;
        for (int j = 0; j < 4 && ok; ++j) {
            const double x = vert ? x0d : x0d + j, y = vert ? y0d + j : y0d;
            const double w = (x * Hi[6] + y * Hi[7]) + Hi[8];
            const double nx = (x * Hi[0] + y * Hi[1]) + Hi[2], ny = (x * Hi[3] + y * Hi[4]) + Hi[5];
            ok = w > 0.52 && w < 1.9 &&
                 fabs(Hi[0]) * x + fabs(Hi[1]) * y + fabs(Hi[2]) <= 8.0 * nx && fabs(Hi[3]) * x + fabs(Hi[4]) * y + fabs(Hi[5]) <= 8.0 * ny &&
                 fabs(Hi[6]) * x + fabs(Hi[7]) * y + fabs(Hi[8]) <= 2.5 && nx / w >= 1.0 && ny / w >= 1.0 && nx / w < 32768.0 && ny / w < 32768.0;
        }
        if (!ok) continue;
        float u[4], v[4];
        uint32_t keys[8];
        double raw[8];
        if (vert) (void)coords_fast_dir<true>(Hi, x0d, y0d, u, v, keys, raw);
        else (void)coords_fast_dir<false>(Hi, x0d, y0d, u, v, keys, raw);
        for (int j = 0; j < 4; ++j) {
            const double x = vert ? x0d : x0d + j, y = vert ? y0d + j : y0d;
            const double w = (x * Hi[6] + y * Hi[7]) + Hi[8];
            const double iw = 1.0 / w;
            const double ued = ((x * Hi[0] + y * Hi[1]) + Hi[2]) * iw, ved = ((x * Hi[3] + y * Hi[4]) + Hi[5]) * iw;
            const float ue = (float)ued, ve = (float)ved;
            far = fmax(far, fmax(ldexp(fabs(raw[2 * j] - ued), 52 - ilogb(ued)), ldexp(fabs(raw[2 * j + 1] - ved), 52 - ilogb(ved))));
            tested += 2;
            if (keys[2 * j] < FAST64_NEAR) ++flagged; else if (__float_as_uint(ue) != __float_as_uint(u[j])) ++missed;
            if (keys[2 * j + 1] < FAST64_NEAR) ++flagged; else if (__float_as_uint(ve) != __float_as_uint(v[j])) ++missed;
        }
    }
    if (missed) atomicAdd(&counters[0], missed);
    if (flagged) atomicAdd(&counters[1], flagged);
    if (tested) atomicAdd(&counters[2], tested);
    if (margin) atomicMax(margin, (unsigned long long)__double_as_longlong(far));       // (non-negative doubles order like their bits)
}

int launch_selftest_fast64(unsigned long long n, unsigned long long seed, unsigned long long* d_counters, hipStream_t st, unsigned long long* d_margin)
{
    hipLaunchKernelGGL(selftest_fast64_kernel, dim3(2048), dim3(256), 0, st, n, seed, d_counters, d_margin);
    return hip_fail(hipGetLastError(), "selftest_fast64_kernel launch");
}

// The byte taps (gather_blend_staged here, the staged rows in resize.hip) rely on ds_read_u8_d16_hi ZEROING the low half of its
// destination, which is what a device with SRAM ECC does (every MI300-class part; measured on the MI355X) -- without SRAM ECC the
// low half would be preserved.  Checked once per process on the device in use; a device that behaves differently is refused.
__device__ int d16_probe_result;
__global__ void d16_probe_kernel()
{
    __shared__ uint8_t s[8];
    if (threadIdx.x < 8) s[threadIdx.x] = (uint8_t)(0x11 * (threadIdx.x + 1));
    __syncthreads();
    uint32_t r = 0xFFFFFFFFu;
    const uint32_t at = (uint32_t)(uintptr_t)&s[0];
    asm volatile("ds_read_u8_d16_hi %0, %1 offset:3\n\ts_waitcnt lgkmcnt(0)" : "+v"(r) : "v"(at) : "memory");
    if (threadIdx.x == 0) d16_probe_result = r == 0x00440000u ? 1 : -1;
}
int check_d16_zero_fill(hipStream_t st)
{
    // per DEVICE: 0 unknown, 1 fine, -1 refused  (benign race: every thread computes the same).  The probe synchronises, so
    // mf_set_device() runs it ahead of time; a launcher only gets here first when the host selected the device itself.
    static std::atomic<int> state[64] = {};           // (per-device host threads may get here together)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hip_fail(hipErrorInvalidDevice, "d16 probe: hipGetDevice");
    if (state[dev] == 0) {
        int h = 0;
        hipLaunchKernelGGL(d16_probe_kernel, dim3(1), dim3(64), 0, st);
        hipError_t e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpyFromSymbol(&h, HIP_SYMBOL(d16_probe_result), sizeof h);
        if (e != hipSuccess) return hip_fail(e, "d16 probe");
        state[dev] = h == 1 ? 1 : -1;
    }
    if (state[dev] != 1) {
        set_error("device %d preserves the other half of a d16 LDS load (no SRAM ECC): the byte-tap kernels are not built for it", dev);
        return MF_ERR_INVALID_ARG;
    }
    return MF_OK;
}

int launch_warp(Px px, const void* frames, void* out, const TableView& tv, int n, int W, int H, int R, int C,
                uint64_t border, int32_t* crop, hipStream_t st)
{
    if (px == Px::U8C3)
        if (const int rc = check_d16_zero_fill(st)) return rc;
    // (any number of frames: the launches below take at most 65,535 -- the grid's y extent -- at a time)
    if (n <= 0 || W < 2 || H < 2 || W > 32767 || H > 32767 || R <= 0 || C <= 0 || R > MAX_MESH || C > MAX_MESH) {
        set_error("mf_warp_%s: unsupported shape n=%d W=%d H=%d R=%d C=%d", px_name(px), n, W, H, R, C);
        return MF_ERR_INVALID_ARG;
    }
    WarpGeom g;
    uint64_t per_launch = make_warp_geom(W, H, R, C, g);
    if (per_launch == 0) {
        set_error("mf_warp_%s: frame too large", px_name(px));
        return MF_ERR_INVALID_ARG;
    }
    if (const char* e = getenv("MF_WARP_FRAMES_PER_LAUNCH")) {      // testing aid: forces the multi-launch split on small clips
        const long v = atol(e);
        if (v > 0 && (uint64_t)v < per_launch) per_launch = (uint64_t)v;
    }
    // staging reads dword-aligned 16-byte chunks: needs a 4-byte aligned clip (W % 4 == 0 is checked by the plan); the plan's windows
    // are re-cut for 1- and 4-byte pixels, not for 6-byte ones, so uint16 frames never stage
    const bool stage = px != Px::U16C3 && ((uintptr_t)frames & 3u) == 0;       // (the planes' kernels take no window either: unused there)
    // (Px::MAPS: `frames` is null and stays unused, `out` holds 8 W H bytes per frame; Px::NV12_UV, Px::P010_UV, Px::NV16_UV, Px::P210_UV: the chroma plane's own bytes)
    const size_t frame_bytes = px_frame_bytes(px, W, H);
    for (int f0 = 0; f0 < n; f0 += (int)per_launch) {
        const int m = n - f0 < (int)per_launch ? n - f0 : (int)per_launch;
        const WarpRange r{ tv.plan + (size_t)f0 * g.per_frame, tv.regions + (size_t)f0 * g.per_frame,
                           tv.records + (size_t)f0 * R * C * MF_CELL_DOUBLES, tv.edges + (size_t)f0 * R * C * MF_EDGE_FLOATS,
                           frames ? (const uint8_t*)frames + f0 * frame_bytes : nullptr, (uint8_t*)out + f0 * frame_bytes, crop + 4 * (size_t)f0, tv.bounds, m };
        const dim3 grid(g.per_xcd * 8u, (uint32_t)m);                  // one wavefront per 32 x 8 footprint
        if (px == Px::U8C1)
            launch_warp8c1_range(g, r, W, H, C, (uint32_t)border, stage, st);
        else if (px == Px::U8C4)
            launch_warp8c4_range(g, r, W, H, C, (uint32_t)border, stage, st);
        else if (px == Px::MAPS)
            launch_maps_range(g, r, W, H, C, st);
        else if (px_is_plane(px))
            launch_plane_range(px, g, r, W, H, C, border, st);
        else if (px == Px::NV12_UV)
            launch_nv12_chroma_range(g, r, W, H, C, (uint32_t)border, st);
        else if (px == Px::NV16_UV)
            launch_nv16_chroma_range(g, r, W, H, C, (uint32_t)border, st);
        else if (px == Px::U16C1)
            launch_warp16c1_range(g, r, W, H, C, (uint32_t)border, st);
        else if (px == Px::P010_UV)
            launch_p010_chroma_range(g, r, W, H, C, (uint32_t)border, st);
        else if (px == Px::P210_UV)
            launch_p210_chroma_range(g, r, W, H, C, (uint32_t)border, st);
        else if (px == Px::U16C3)
            hipLaunchKernelGGL(warp16_footprint, grid, dim3(64), 0, st, r.plan, r.regions, g, (const uint16_t*)r.frames, r.records, (uint16_t*)r.out,
                               r.edges, m, W, H, C, border, r.crop, r.bounds);
        else if (stage)
            hipLaunchKernelGGL(warp_kernel<true>, grid, dim3(64), 0, st, r.plan, r.regions, g, (const uint8_t*)r.frames, r.records, (uint8_t*)r.out,
                               r.edges, m, W, H, C, (uint32_t)border, r.crop, r.bounds);
        else
            hipLaunchKernelGGL(warp_kernel<false>, grid, dim3(64), 0, st, r.plan, r.regions, g, (const uint8_t*)r.frames, r.records, (uint8_t*)r.out,
                               r.edges, m, W, H, C, (uint32_t)border, r.crop, r.bounds);
    }
    return hip_fail(hipGetLastError(), px == Px::U8C3 ? "warp_kernel launch" : px == Px::U16C3 ? "warp16_footprint launch" :
                                       px == Px::U8C1 ? "warp8c1_footprint launch" : px == Px::U8C4 ? "warp8c4_footprint launch" : px == Px::MAPS ? "maps_footprint launch" :
                                       px == Px::NV12_UV ? "nv12_chroma_footprint launch" : px == Px::NV16_UV ? "nv16_chroma_footprint launch" : px == Px::U16C1 ? "warp16c1_footprint launch" :
                                       px == Px::P010_UV ? "p010_chroma_footprint launch" : px == Px::P210_UV ? "p210_chroma_footprint launch" : "plane_footprint launch");
}

int launch_crop_scan(const TableView& tv, int n, int W, int H, int R, int C, int32_t* crop, hipStream_t st)
{
    // (any number of frames, like launch_warp: the launches below take per_launch frames at a time)
    if (n <= 0 || W < 2 || H < 2 || W > 32767 || H > 32767 || R <= 0 || C <= 0 || R > MAX_MESH || C > MAX_MESH) {
        set_error("mf_crop_scan_f64: unsupported shape n=%d W=%d H=%d R=%d C=%d", n, W, H, R, C);
        return MF_ERR_INVALID_ARG;
    }
    WarpGeom g;
    const uint32_t per_launch = make_warp_geom(W, H, R, C, g);
    if (per_launch == 0) {
        set_error("mf_crop_scan_f64: frame too large");
        return MF_ERR_INVALID_ARG;
    }
    for (int f0 = 0; f0 < n; f0 += (int)per_launch) {
        const int m = n - f0 < (int)per_launch ? n - f0 : (int)per_launch;
        const uint32_t total = (uint32_t)m * g.per_frame;                  // (per_launch keeps 16 B x total below 2^32)
        hipLaunchKernelGGL(crop_scan_kernel, dim3((total + SCAN_GROUP - 1) / SCAN_GROUP), dim3(64), 0, st,
                           tv.plan + (size_t)f0 * g.per_frame, tv.regions + (size_t)f0 * g.per_frame, g,
                           tv.records + (size_t)f0 * R * C * MF_CELL_DOUBLES, tv.edges + (size_t)f0 * R * C * MF_EDGE_FLOATS, total, m, W, H, C,
                           crop + 4 * (size_t)f0, tv.bounds);
    }
    return hip_fail(hipGetLastError(), "crop_scan_kernel launch");
}

// Clip-level bounds, mfs.py:1103-1106.
__global__ __launch_bounds__(256) void crop_reduce_kernel(const int32_t* __restrict__ crop, int n, int W, int H,
                                                          int32_t* __restrict__ bounds)
{
    __shared__ int32_t red[4][256];
    int l = 0, t = 0, r = W - 1, b = H - 1;
    for (int i = threadIdx.x; i < n; i += 256) {
        l = max(l, crop[4 * i + 0]); t = max(t, crop[4 * i + 1]);
        r = min(r, crop[4 * i + 2]); b = min(b, crop[4 * i + 3]);
    }
    red[0][threadIdx.x] = l; red[1][threadIdx.x] = t; red[2][threadIdx.x] = r; red[3][threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] = max(red[0][threadIdx.x], red[0][threadIdx.x + s]);
            red[1][threadIdx.x] = max(red[1][threadIdx.x], red[1][threadIdx.x + s]);
            red[2][threadIdx.x] = min(red[2][threadIdx.x], red[2][threadIdx.x + s]);
            red[3][threadIdx.x] = min(red[3][threadIdx.x], red[3][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) bounds[threadIdx.x] = red[threadIdx.x][0];
}

int launch_crop_reduce(const int32_t* crop, int n, int W, int H, int32_t* bounds, hipStream_t st)
{
    if (n <= 0) { set_error("mf_crop_reduce: n=%d", n); return MF_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(crop_reduce_kernel, dim3(1), dim3(256), 0, st, crop, n, W, H, bounds);
    return hip_fail(hipGetLastError(), "crop_reduce_kernel launch");
}

}  // namespace mf
