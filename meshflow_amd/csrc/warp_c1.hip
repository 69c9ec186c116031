// Kernel 2b for single-channel uint8 frames (mf_warp_u8c1, mf_warp_clip_u8c1, the u8c1 host pipeline): footprint_body's GREY instantiation.
// It lives in a translation unit of its own so that warp.hip's code object -- and with it every existing kernel, instruction for instruction
// (tools/isa_compare.py) -- stays what it is: this file takes footprint_body and its helpers from warp_body.h and adds the grey kernel and its
// range launch.  Design and measurements: DESIGN.md section 4.8.
#include "warp_body.h"

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
    footprint_body<Px::U8C1, STAGE, false>(f, t, plan, regions, g, frames, records, out, edges, n, W, H, C, border, crop, clip);
}

// launch_warp's launch for one frame range of a single-channel clip (stage: the clip is 4-byte aligned)
void launch_warp8c1_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border, bool stage, hipStream_t st)
{
    const dim3 grid(g.per_xcd * 8u, (uint32_t)r.m);
    const uint8_t* fr = (const uint8_t*)r.frames;
    uint8_t* o = (uint8_t*)r.out;
    if (stage)
        hipLaunchKernelGGL(warp8c1_footprint<true>, grid, dim3(64), 0, st, r.plan, r.regions, g, fr, r.records, o, r.edges, r.m, W, H, C, border, r.crop, r.bounds);
    else
        hipLaunchKernelGGL(warp8c1_footprint<false>, grid, dim3(64), 0, st, r.plan, r.regions, g, fr, r.records, o, r.edges, r.m, W, H, C, border, r.crop, r.bounds);
}

}  // namespace mf
