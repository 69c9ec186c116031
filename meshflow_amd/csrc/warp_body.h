// What the warp translation units share (warp.hip, warp_c1.hip, warp_c4.hip, warp_maps.hip, warp_planes.hip, warp_nv12.hip, warp_nv16.hip, warp_c1_16.hip, warp_p010.hip): footprint_body and the blocks its
// paths share.  The constants and the coordinate code are in warp_coords.h, the uint8 BGR taps and blend in warp_taps_u8c3.h, the other
// formats' tails in warp_tails.h; the units include this header only.  The design note is at the head of warp.hip.
#ifndef MF_WARP_BODY_H
#define MF_WARP_BODY_H
#include "mf_common.h"
#include "warp_coords.h"
#include "warp_taps_u8c3.h"
#include "warp_tails.h"

#include <type_traits>

// At most 80 scalar registers: a CU admits min(8, 800 / (ceil(sgpr / 16) * 16 + 16)) workgroups of 256 threads
// (MI355X_MICROARCH.md), i.e. 7 with the 94 the compiler would take and 8 with 80 (the excess is kept in VGPR lanes, the kernel
// stays at 64 VGPRs): -1.7 % kernel time.
#define MF_WARP_ATTR __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(8, 8)))

namespace mf {

// ---- what footprint_body's paths share ------------------------------------------------------------------------------------------------
// One cell's inverse homography to a row of s_hi by global->LDS load: the nine doubles are 18 consecutive dwords of the cell's record, lanes
// 0..19 copy them (and two dwords of padding); `lo4` is the calling lane's byte offset 4 * lane, opaque to the compiler so that the address
// keeps the form scalar base + 32-bit lane offset.  SCALAR_BASE: the whole base is forced into scalar registers first (the certified paths
// of the BGR warp; the other callers leave the choice to the compiler, and the code each gets is the one it had).
template <bool SCALAR_BASE>
__device__ __forceinline__ void stage_matrix(crec_t frec, uint32_t k, const double* row, uint32_t lo4)
{
    uint64_t base = (uint64_t)(uintptr_t)(frec + k * MF_CELL_DOUBLES + MF_CELL_OFF_HI);
    if (SCALAR_BASE) asm("" : "+s"(base));
    const uint8_t* __restrict__ g = (const uint8_t*)(uintptr_t)base;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + lo4), (__attribute__((address_space(3))) void*)lds_ptr(row), 4, 0, 0);
}

// Each of the lane's four pixels' coordinates from its owner's matrix -- the row of s_hi at byte offset own[j] from `hi0` -- through the
// trimmed reciprocal: for footprints whose denominators the plan certifies (MF_PLAN_UNIT).  cv2.perspectiveTransform's chain, as cell_coords.
__device__ __forceinline__ void owner_coords_unit(const double* hi0, const uint32_t (&own)[4], double xs0, double yy, float (&u)[4], float (&v)[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double* hp = reinterpret_cast<const double*>(reinterpret_cast<const uint8_t*>(hi0) + own[j]);
        const double2 h01 = *reinterpret_cast<const double2*>(hp), h23 = *reinterpret_cast<const double2*>(hp + 2);
        const double2 h45 = *reinterpret_cast<const double2*>(hp + 4), h67 = *reinterpret_cast<const double2*>(hp + 6);
        const double h8 = hp[8];
        const double xs = xs0 + (double)j;
        const double iw = recip_unit_range((xs * h67.x + yy * h67.y) + h8);
        u[j] = (float)(((xs * h01.x + yy * h01.y) + h23.x) * iw);
        v[j] = (float)(((xs * h23.y + yy * h45.x) + h45.y) * iw);
    }
}

// The one-edge owner test of a PAIR footprint: the later cell (row 0 of s_hi) owns a pixel where its mask edge `eb` passes -- one float32
// fma per pixel --, the other cell (row 1) the rest.  Returns the smallest |edge function|: a pixel inside the float32 error band of the
// edge (not above EDGE_BAND; NaN coefficients too) leaves the footprint to the general code, which decides exactly.
__device__ __forceinline__ float pair_owner(cedge_t eb, int x0, int y, uint32_t (&own)[4])
{
    const float rb = __builtin_fmaf(eb[1], (float)y, eb[2]), xf0 = (float)x0;
    float near = 1e30f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float gb = __builtin_fmaf(eb[0], xf0 + (float)j, rb);
        own[j] = gb > EDGE_BAND ? 0u : OWN_ROW;
        near = fminf(near, fabsf(gb));
    }
    return near;
}

// The coded mask edges of a MIXED cell on the lane's four pixels: gq[j] = the smaller of the two edge functions the code `cd` names (edge
// cd & 3 and, where bit 3 is set, edge (cd >> 4) & 3; a one-edge code takes the same edge twice) of the cell whose edge record is `ed`.
__device__ __forceinline__ void coded_edges_min(cedge_t ed, uint32_t cd, float xf0, float yf, float (&gq)[4])
{
    const cedge_t e1 = ed + 3u * (cd & 3u);
    const cedge_t e2 = ed + 3u * ((cd & 8u) ? ((cd >> 4) & 3u) : (cd & 3u));
    const float r1 = __builtin_fmaf(e1[1], yf, e1[2]), r2 = __builtin_fmaf(e2[1], yf, e2[2]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xf = xf0 + (float)j;
        gq[j] = fminf(__builtin_fmaf(e1[0], xf, r1), __builtin_fmaf(e2[0], xf, r2));
    }
}

// Where a STAGED window (cut for 3-byte pixels) starts in the frame, for the grey and 4-byte windows re-cut from it: returns its first row sy0
// and sets its byte column bs, from origin = P sy0 + bs and src = 3 W sy0 + bs in the region words (GreyWindow, warp_tails.h, has the derivation).
__device__ __forceinline__ uint32_t recut_origin(uint32_t rg, uint32_t src_dwords, int W, uint32_t& bs)
{
    const uint32_t P = (rg & MF_REGION_COMPACT) != 0 ? (uint32_t)MF_COMPACT_PITCH : (uint32_t)MF_STAGE_PITCH;
    const uint32_t origin = rg & MF_REGION_ORIGIN_MASK, sbytes = src_dwords << 2;
    const uint32_t sy0 = __builtin_amdgcn_readfirstlane((uint32_t)((float)(sbytes - origin) / (float)(3u * (uint32_t)W - P) + 0.5f));
    bs = origin - P * sy0;
    return sy0;
}

// The tail of every format but uint8 BGR (whose taps and blend are footprint_body's own): the lane's four pixels at (u, v) -- taps, blend,
// crop flags, store.  SCAN (the planes' nearest tail only): the four crop tests on every pixel -- the general path; the others test where
// a pixel is not deep inside.
template <Px PX, bool SCAN>
__device__ __forceinline__ void store_tail(const float (&u)[4], const float (&v)[4], uint32_t f, int x0, int y, bool active, int W, int H,
                                           const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, uint32_t border, uint64_t border16,
                                           int32_t* __restrict__ crop, int32_t* __restrict__ clip, const GreyWindow& win, const uint8_t* s_win)
{
    if constexpr (PX == Px::MAPS) maps_store_f32(u, v, f, x0, y, active, W, H, reinterpret_cast<float*>(out));
    else if constexpr (px_is_chroma(PX)) remap_store_chroma<PX>(u, v, f, x0, y, active, W, H, frames, out, border);
    else if constexpr (PX == Px::U16C1)
        remap_store_u16c1(u, v, f, x0, y, active, W, H, reinterpret_cast<const uint16_t*>(frames), reinterpret_cast<uint16_t*>(out), border, crop, clip);
    else if constexpr (px_is_plane(PX)) remap_store_plane<PX, SCAN>(u, v, f, x0, y, active, W, H, frames, out, border16, crop, clip);
    else if constexpr (PX == Px::U16C3)
        remap_store_u16(u, v, f, x0, y, active, W, H, reinterpret_cast<const uint16_t*>(frames), reinterpret_cast<uint16_t*>(out), border16, crop, clip);
    else if constexpr (PX == Px::U8C4) remap_store_u8c4(u, v, f, x0, y, active, W, H, frames, out, border, crop, clip, win, s_win);
    else remap_store_u8c1(u, v, f, x0, y, active, W, H, frames, out, border, crop, clip, win, s_win);
}

// The lane's 12 output bytes (four BGR pixels from column x0 of row y) as one store: for frames with W % 4 == 0, where the address is
// 4-byte aligned and all four pixels lie inside.
__device__ __forceinline__ void store_bgr4(uint8_t* __restrict__ dst, int W, int x0, int y, const uint3& d)
{
    *reinterpret_cast<uint3*>(dst + ((uint32_t)y * (uint32_t)W + (uint32_t)x0) * 3u) = d;
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
// re-cut for 4-byte pixels (MF_C4_COLS) and copied to LDS at the start; the hot and pair footprints take the shortcuts below (WIN_STAGE).
// PX = Px::MAPS: the coordinate maps instead of pixels (maps_footprint, warp_maps.hip): SCAN's body -- ownership, coordinates, the four edge
// tests on every footprint -- plus the store of (u, v) (maps_store_f32): `frames` is unused, `out` points to float32 [n][H][W][2].  No window, no
// taps, no border colour; the hot and pair footprints take the same shortcuts (NOWIN: they need no window here), everything else the general path.
// PX = Px::PLANE_*: the side planes (plane_footprint, warp_planes.hip): `frames` / `out` hold W H elements of px_sample_bytes(PX) bytes per
// frame, `border16` is the fill value's bit pattern, and the pixels go through remap_store_plane -- taps from global memory like the uint16
// warp (the plan's windows are cut for 3-byte pixels), the hot and pair shortcuts like the maps (they need no window), the general path for the rest.
// PX = Px::NV12_UV: the chroma plane of an NV12 clip (nv12_chroma_footprint, warp_nv12.hip) on the LUMA frame's plan: W, H, the footprints, the
// ownership and the coordinates are the luma frame's -- the maps kernel's paths, so (u, v) are its values bit for bit --, `frames` / `out` hold
// (W / 2) (H / 2) pixels of two bytes per frame, the border is U | V << 8 in `border`, and the pixels go through remap_store_chroma, which halves
// the coordinates of the even luma pixels.  Taps from global memory; `crop` / `clip` are never touched (null: the luma launch owns them).
// PX = Px::NV16_UV: the chroma plane of an NV16 clip (nv16_chroma_footprint, warp_nv16.hip): Px::NV12_UV on a plane of full height -- `frames` /
// `out` hold (W / 2) H pixels of two bytes per frame, H of either parity, and the pixels go through remap_store_chroma, where every row emits and
// only the x coordinate is halved.  Taps from global memory, the hot and pair shortcuts (NOWIN), `crop` / `clip` never touched, like NV12.
// PX = Px::U16C1: the luma planes of a P010 clip (warp16c1_footprint, warp_c1_16.hip): `frames` / `out` hold W H uint16 samples per frame, the
// border sample is `border`, and the pixels go through remap_store_u16c1 -- Px::U16C3's arithmetic on one channel, taps from global memory.
// Unlike Px::U16C3 it takes the hot and pair shortcuts (NOWIN), like the float32 plane whose tail has the same shape: one third of the
// uint16 BGR taps leaves the ownership and coordinate code as most of a footprint's work, and the shortcuts are what shortens that.
// PX = Px::P010_UV: the chroma plane of a P010 clip (p010_chroma_footprint, warp_p010.hip): Px::NV12_UV on pixels of two uint16 samples --
// (W / 2) (H / 2) pixels of four bytes per frame, the border is U | V << 16 in `border`, the pixels go through remap_store_chroma's
// uint16 arithmetic.
// PX = Px::P210_UV: the chroma plane of a P210 clip (p210_chroma_footprint, warp_p210.hip): Px::NV16_UV on pixels of two uint16 samples --
// (W / 2) H pixels of four bytes per frame, H of either parity, the border is U | V << 16, remap_store_chroma's uint16 arithmetic on every row.
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
    constexpr bool GREY = PX == Px::U8C1, GREY_STAGE = GREY && STAGE;
    // C4_STAGE: the 4-channel warp of a 4-byte aligned clip; WIN_STAGE: a re-cut window (grey or 4-byte) and the hot / pair shortcuts on it
    constexpr bool C4 = PX == Px::U8C4, C4_STAGE = C4 && STAGE, WIN_STAGE = GREY_STAGE || C4_STAGE;
    constexpr bool MAPS = PX == Px::MAPS;
    static_assert(!MAPS || (!STAGE && !SCAN), "the maps kernel reads no frame: nothing to stage");
    // NOWIN: the instantiations that take the hot and pair shortcuts without a window (the maps read no frame, the planes tap global memory)
    constexpr bool PLANE = px_is_plane(PX), NV12 = PX == Px::NV12_UV, P010 = PX == Px::U16C1 || PX == Px::P010_UV, NV16 = px_is_chroma422(PX);
    constexpr bool NOWIN = MAPS || PLANE || NV12 || P010 || NV16;       // (NV16: either 4:2:2 chroma plane, NV16_UV or P210_UV)
    static_assert(!(PLANE || NV12 || P010 || NV16) || (!STAGE && !SCAN), "the plane and chroma warps take their taps from global memory");
    // inverse homographies of the footprint's candidate cells: [entry][Hi0..Hi8, pad] (80-byte rows)
    __shared__ __attribute__((aligned(16))) double s_hi[1][9][10];                // row 8: the "no cell" matrix, see OWN_NONE
    // source region of the footprint: MF_STAGE_ROWS rows of MF_STAGE_PITCH bytes (+ slack for the third dword of the last tap); the 4-byte
    // window's MF_STAGE_ROWS rows of MF_C4_PITCH bytes for U8C4
    __shared__ __attribute__((aligned(16))) uint8_t s_src_all[SCAN || NOWIN ? 16 : C4 ? LDS_WINDOW_PAD + MF_STAGE_ROWS * MF_C4_PITCH
                                                                             : LDS_WINDOW_PAD + LDS_WINDOW_BYTES + 64];
    uint8_t* const s_src = &s_src_all[SCAN || NOWIN ? 0 : LDS_WINDOW_PAD];
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
            const uint32_t rows = (rg & MF_REGION_COMPACT) ? (uint32_t)MF_COMPACT_ROWS : (uint32_t)MF_STAGE_ROWS;
            uint32_t bs;
            const uint32_t sy0 = recut_origin(rg, src_dwords, W, bs);
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
            const uint32_t rows = (rg & MF_REGION_COMPACT) ? (uint32_t)MF_COMPACT_ROWS : (uint32_t)MF_STAGE_ROWS;
            uint32_t bs;
            const uint32_t sy0 = recut_origin(rg, src_dwords, W, bs);
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
        store_bgr4(dst, W, x0, y, d);                                // (STAGED implies W % 4 == 0)
        return;
    }

    if constexpr (WIN_STAGE || NOWIN) {
        if ((NOWIN || gwin.on) && (pv.x & (MF_PLAN_HOT << 16)) != 0) {
            // the HOT footprints of the grey, 4-channel, maps and plane warps (one IN cell, certified denominator, deep, staged): the hot
            // path's coordinates -- the cheap chain where the plan allows it (FAST64), else the trimmed-reciprocal one -- without the
            // general path's ownership code
            const crec_t rec = frec + (pv.x & 0xFFFu) * MF_CELL_DOUBLES;
            float u[4], v[4];
            if (!((pv.x >> 16) & MF_PLAN_FAST64) || !cell_coords_fast(rec, xs0, yy, u, v))
                cell_coords<false>(rec, xs0, yy, x0, 0xFu, u, v, true);
            // (MAPS: a hot footprint is whole and DEEP -- every lane stores, no pixel can pass a crop test)
            store_tail<PX, false>(u, v, f, x0, y, true, W, H, frames, out, border, border16, crop, clip, gwin, &s_src[0]);
            return;
        }
    }
    const cedge_t fedge = (cedge_t)(uintptr_t)(reinterpret_cast<const uint8_t*>(edges) + f * g.edge_frame_bytes);
    if constexpr (WIN_STAGE || NOWIN) {
        if ((NOWIN || gwin.on) && (pv.y & MF_PLAN_HOT) != 0) {
            // the PAIR footprints of the same warps (two cells, certified denominators, deep, staged): warp_kernel's per-pixel pair form --
            // the later cell owns a pixel where its one mask edge passes (one fma), the other cell the rest, both matrices in LDS; a pixel
            // inside the edge's float32 error band leaves the footprint to the general code
            const uint32_t k0 = pv.x & 0xFFFu, k1 = (pv.x >> 16) & 0xFFFu;
            if (lane < 20) {
                uint32_t lo4 = (uint32_t)lane << 2;
                asm("" : "+v"(lo4));
                stage_matrix<false>(frec, k0, &s_hi[0][0][0], lo4);
                stage_matrix<false>(frec, k1, &s_hi[0][1][0], lo4);
            }
            const cedge_t eb = fedge + k0 * MF_EDGE_FLOATS + 3u * (pv.z & 3u);
            uint32_t own[4];
            const float near = pair_owner(eb, x0, y, own);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // matrices (and the re-cut window) have landed in LDS
            if (__ballot(!(near > EDGE_BAND)) == 0) {
                float u[4], v[4];
                owner_coords_unit(&s_hi[0][0][0], own, xs0, yy, u, v);
                store_tail<PX, false>(u, v, f, x0, y, true, W, H, frames, out, border, border16, crop, clip, gwin, &s_src[0]);
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
            float gq[4], near = 1e30f;
            coded_edges_min(ed, cd, (float)x0, (float)y, gq);
            cov = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cov |= gq[j] > EDGE_BAND ? (1u << j) : 0u;
                near = fminf(near, fabsf(gq[j]));
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
                crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
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
            store_bgr4(dstb, W, x0, y, d);                               // (STAGED implies W % 4 == 0; the footprint is whole)
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
            stage_matrix<true>(frec, k0, &s_hi[0][0][0], lo4);
            stage_matrix<true>(frec, k1, &s_hi[0][1][0], lo4);
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
                store_bgr4(dst, W, x0, y, d);
                return true;
            };
            if ((pv.y & MF_PLAN_PAIR_VERT) ? lane_uniform(std::true_type{}) : lane_uniform(std::false_type{})) return;
        }
        uint32_t own[4];
        const float near = pair_owner(eb, x0, y, own);
        // (a pixel inside the float32 error band of the edge, or NaN coefficients: the general code below decides exactly)
        if (__ballot(!(near > EDGE_BAND)) == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // matrices and window have landed in LDS
            float u[4], v[4];
            owner_coords_unit(&s_hi[0][0][0], own, xs0, yy, u, v);
            uint32_t bx[4], by[4];
            fixed_point(u, v, bx, by);
            uint8_t* __restrict__ dst = out + (uint64_t)f * g.frame_bytes;
            const uint3 d = gather_blend_window(compact, bx, by, lds_origin);
            store_bgr4(dst, W, x0, y, d);
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
                    stage_matrix<true>(frec, k, &s_hi[0][i][0], lo4);
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
                    float gq[4];
                    coded_edges_min(ed, cd, xf0, yf, gq);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        own[j] = gq[j] > EDGE_BAND ? OWN_ROW * (uint32_t)i : own[j];
                        near = fminf(near, fabsf(gq[j]));
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
                owner_coords_unit(&s_hi[0][0][0], own, xs0, yy, u, v);
            }
            uint32_t bx[4], by[4];
            fixed_point(u, v, bx, by);
            uint8_t* __restrict__ dst = out + (uint64_t)f * g.frame_bytes;
            const uint3 d = gather_blend_window(compact, bx, by, lds_origin);
            store_bgr4(dst, W, x0, y, d);
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
                    stage_matrix<false>(frec, k, &s_hi[0][e][0], lo4);
                }
            }
            uint32_t own[4];                                            // byte offset of the owner's matrix row (OWN_ROW * entry)
            if (!(rg & MF_REGION_DEEP) && lane < 10) {                  // only uncertified footprints can have uncovered pixels
                int Wp = W + 1, Hp = H + 1;                              // (opaque: keeps the conversions inside this branch)
                asm volatile("" : "+s"(Wp), "+s"(Hp));
                s_hi[0][8][lane] = lane == 2 ? (double)Wp : lane == 5 ? (double)Hp : lane == 8 ? 1.0 : 0.0;
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
                const double* hp = reinterpret_cast<const double*>(reinterpret_cast<const uint8_t*>(&s_hi[0][0][0]) + own[j]);
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
                    const double* hp = reinterpret_cast<const double*>(reinterpret_cast<const uint8_t*>(&s_hi[0][0][0]) + own[j]);
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
            crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
            if constexpr (MAPS) store_tail<PX, true>(u, v, f, x0, y, active, W, H, frames, out, border, border16, crop, clip, gwin, &s_src[0]);
            return;
        }
        if constexpr (PX != Px::U8C3) {                                 // (the other formats' tails: the crop tests and the fold are theirs)
            store_tail<PX, true>(u, v, f, x0, y, active, W, H, frames, out, border, border16, crop, clip, gwin, &s_src[0]);
            return;
        }
        // cv2.remap: 1/32-pixel fixed point (round half to even), bilinear gather, store.
        uint32_t bx[4], by[4];
        fixed_point(u, v, bx, by);
        bool fast = true;
        if (!(staged && (rg & MF_REGION_DEEP))) {        // (DEEP: every pixel has an owner and every tap is deep inside: nothing to check)
            const bool deep = deep_interior(bx, by, W, H);
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
                const bool narrow = narrow_coords(bx, by);
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
                    const int sxx = fixed_coord(narrow, bx[j], uu), syy = fixed_coord(narrow, by[j], vv);
                    const int ix = sxx >> 5, iy = syy >> 5;      // (saturation to int16 cannot change any decision below)
                    // The four taps, branch-free: each load goes to the position clamped into the frame and the tap is replaced by the
                    // border colour afterwards when it lies outside (a 2 x 2 footprint outside altogether needs no special case: four
                    // border-colour taps with weights that sum to 1024 give the border colour exactly).  All sixteen loads of the lane
                    // are in flight together.
                    const ClampedTaps ct = clamped_taps(ix, iy, W, H);
                    if (staged) {
                        // STAGED: the window holds every tap position CLAMPED into the frame (cell_table.hip), so the four taps are LDS
                        // byte loads (a pixel without owner sits at (W+1, H+1): its clamped position may lie outside the window --
                        // whatever the load returns is replaced by the border colour below).  (Unaligned 4-byte LDS loads instead:
                        // +2 % kernel time; two pixels' loads in flight: register spills.)
                        const uint32_t pitch = compact ? (uint32_t)MF_COMPACT_PITCH : (uint32_t)LDS_PITCH;      // (wave-uniform)
                        const uint32_t ra = umad24((uint32_t)min(max(iy, 0), H - 1), pitch, 0u - lds_origin);
                        const uint32_t rb = umad24((uint32_t)min(max(iy + 1, 0), H - 1), pitch, 0u - lds_origin);
                        TapRegs t;
                        taps_clamped(umad24(ct.cx0, 3u, ra), umad24(ct.cx1, 3u, ra), umad24(ct.cx0, 3u, rb), umad24(ct.cx1, 3u, rb), t);
                        const bool i00 = ct.in_x0 && ct.in_y0, i01 = ct.in_x1 && ct.in_y0, i10 = ct.in_x0 && ct.in_y1, i11 = ct.in_x1 && ct.in_y1;
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
                    const uint32_t o00 = (ct.r0 + ct.cx0) * 3u, o01 = (ct.r0 + ct.cx1) * 3u, o10 = (ct.r1 + ct.cx0) * 3u, o11 = (ct.r1 + ct.cx1) * 3u;
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
                    p00 = ct.in_x0 && ct.in_y0 ? p00 : border;
                    p01 = ct.in_x1 && ct.in_y0 ? p01 : border;
                    p10 = ct.in_x0 && ct.in_y1 ? p10 : border;
                    p11 = ct.in_x1 && ct.in_y1 ? p11 : border;
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
            crop_fold(c_left, c_top, c_right, c_bottom, f, W, H, crop, clip);
        }
        if (active) {                                                   // the lane's 12 output bytes
            const uint32_t o = ((uint32_t)y * (uint32_t)W + (uint32_t)x0) * 3u;
            if (fast_store) {                                           // W % 4 == 0: an active lane's four pixels are all inside
                store_bgr4(dst, W, x0, y, d);
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
