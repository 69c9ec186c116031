// Kernel 2b for 4-channel uint8 frames (mf_warp_u8c4, mf_warp_clip_u8c4): footprint_body's U8C4 instantiation.  Like warp_c1.hip, a translation
// unit of its own, so that warp.hip's code object -- and with it every existing kernel, instruction for instruction (tools/isa_compare.py) --
// stays what it is: this file takes footprint_body and its helpers from warp_body.h and adds the 4-channel kernel and its range launch.
// Design and measurements: profiles/u8c4_design.md.
#include "warp_body.h"

namespace mf {

// The mesh warp of B G R A (or R G B A) uint8 frames: warp_kernel's footprint order and ownership / coordinate code (footprint_body's general
// path, plus the grey warp's hot and pair shortcuts), the plan's staged windows re-cut for 4-byte pixels (STAGE: a 4-byte aligned clip), the
// 8-bit fixed-point blend on four channels at the end (remap_store_u8c4).  The same d_crop rows and clip rectangle as warp_kernel on the same table.
template <bool STAGE>
__global__ __launch_bounds__(64) void warp8c4_footprint(const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions,
                                                        WarpGeom g, const uint8_t* __restrict__ frames,
                                                        const double* __restrict__ records, uint8_t* __restrict__ out,
                                                        const float* __restrict__ edges, int n, int W,
                                                        int H, int C, uint32_t border, int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint32_t f = blockIdx.y;
    const uint32_t t = ((blockIdx.x + f) & 7u) * g.per_xcd + (blockIdx.x >> 3);
    if (t >= g.per_frame) return;
    footprint_body<Px::U8C4, STAGE, false>(f, t, plan, regions, g, frames, records, out, edges, n, W, H, C, border, crop, clip);
}

// launch_warp's launch for one frame range of a 4-channel clip (stage: the clip is 4-byte aligned)
void launch_warp8c4_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border, bool stage, hipStream_t st)
{
    const dim3 grid(g.per_xcd * 8u, (uint32_t)r.m);
    const uint8_t* fr = (const uint8_t*)r.frames;
    uint8_t* o = (uint8_t*)r.out;
    if (stage)
        hipLaunchKernelGGL(warp8c4_footprint<true>, grid, dim3(64), 0, st, r.plan, r.regions, g, fr, r.records, o, r.edges, r.m, W, H, C, border, r.crop, r.bounds);
    else
        hipLaunchKernelGGL(warp8c4_footprint<false>, grid, dim3(64), 0, st, r.plan, r.regions, g, fr, r.records, o, r.edges, r.m, W, H, C, border, r.crop, r.bounds);
}

}  // namespace mf
