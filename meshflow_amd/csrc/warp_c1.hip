// Kernel 2b for single-channel uint8 frames (mf_warp_u8c1, mf_warp_clip_u8c1, the u8c1 host pipeline): footprint_body's GREY instantiation.
// It lives in a translation unit of its own so that warp.hip's code object -- and with it every existing kernel, instruction for instruction
// (tools/isa_compare.py) -- stays what it is: this file takes footprint_body and its helpers from warp.hip (MF_WARP_BODY_ONLY) and adds the
// grey kernel and its launcher.  Design and measurements: DESIGN.md section 4.8.
#define MF_WARP_BODY_ONLY 1
#include "warp.hip"

namespace mf {

// The mesh warp of single-channel uint8 frames: warp_kernel's footprint order and ownership / coordinate code (footprint_body's general path),
// the plan's staged windows re-cut for 1-byte pixels (STAGE: a 4-byte aligned clip), cv2.remap's 8-bit arithmetic per pixel at the end
// (remap_store_u8c1).  The same d_crop rows and clip rectangle as warp_kernel on the same table.
template <bool STAGE>
__global__ __launch_bounds__(64) void warp8c1_footprint(const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions,
                                                        WarpGeom g, const uint8_t* __restrict__ frames,
                                                        const double* __restrict__ records, uint8_t* __restrict__ out,
                                                        const float* __restrict__ edges, int n, int W,
                                                        int H, int C, uint32_t border, int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint32_t f = blockIdx.y;
    const uint32_t t = ((blockIdx.x + f) & 7u) * g.per_xcd + (blockIdx.x >> 3);
    if (t >= g.per_frame) return;
    footprint_body<false, false, false, true, STAGE>(f, t, plan, regions, g, frames, records, out, edges, n, W, H, C, border, crop, clip);
}

int launch_warp_u8c1(const uint8_t* frames, uint8_t* out, const TableView& tv, int n, int W, int H, int R, int C,
                     uint8_t border, int32_t* crop, hipStream_t st)
{
    if (n <= 0 || W < 2 || H < 2 || W > 32767 || H > 32767 || R <= 0 || C <= 0 || R > MAX_MESH || C > MAX_MESH) {
        set_error("mf_warp_u8c1: unsupported shape n=%d W=%d H=%d R=%d C=%d", n, W, H, R, C);
        return MF_ERR_INVALID_ARG;
    }
    WarpGeom g;
    uint64_t per_launch = make_warp_geom(W, H, R, C, g);
    if (per_launch == 0) {
        set_error("mf_warp_u8c1: frame too large");
        return MF_ERR_INVALID_ARG;
    }
    if (const char* e = getenv("MF_WARP_FRAMES_PER_LAUNCH")) {      // testing aid, as in launch_warp
        const long v = atol(e);
        if (v > 0 && (uint64_t)v < per_launch) per_launch = (uint64_t)v;
    }
    // the grey window is copied in dword-aligned 16-byte chunks: a 4-byte aligned clip (W % 4 == 0 is checked by the plan)
    const bool stage = ((uintptr_t)frames & 3u) == 0;
    const uint64_t frame_px = (uint64_t)W * (uint64_t)H;
    for (int f0 = 0; f0 < n; f0 += (int)per_launch) {
        const int m = n - f0 < (int)per_launch ? n - f0 : (int)per_launch;
        const dim3 grid(g.per_xcd * 8u, (uint32_t)m);
        const FootPlan* pl = tv.plan + (size_t)f0 * g.per_frame;
        const FootRegion* rgn = tv.regions + (size_t)f0 * g.per_frame;
        const uint8_t* fr = frames + (size_t)f0 * frame_px;
        uint8_t* o = out + (size_t)f0 * frame_px;
        const double* rec = tv.records + (size_t)f0 * R * C * MF_CELL_DOUBLES;
        const float* ed = tv.edges + (size_t)f0 * R * C * MF_EDGE_FLOATS;
        if (stage)
            hipLaunchKernelGGL(warp8c1_footprint<true>, grid, dim3(64), 0, st, pl, rgn, g, fr, rec, o, ed, m, W, H, C, (uint32_t)border, crop + 4 * (size_t)f0, tv.bounds);
        else
            hipLaunchKernelGGL(warp8c1_footprint<false>, grid, dim3(64), 0, st, pl, rgn, g, fr, rec, o, ed, m, W, H, C, (uint32_t)border, crop + 4 * (size_t)f0, tv.bounds);
    }
    return hip_fail(hipGetLastError(), "warp8c1_footprint launch");
}

}  // namespace mf
