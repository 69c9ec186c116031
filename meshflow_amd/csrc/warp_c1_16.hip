// Kernel 2b for the luma planes of a P010 / P012 / P016 clip (mf_warp_p010, mf_warp_bounds_p010): footprint_body's U16C1 instantiation -- planes
// [n][H][W] of uint16 samples sampled like cv2.remap INTER_LINEAR / BORDER_CONSTANT of CV_16UC1 at the coordinates the reference hands to
// cv2.remap at mfs.py:1063-1069: channel 0 of the uint16 BGR warp (warp16_footprint, warp.hip) on the plane repeated three times, bit for bit.
// Like warp_c1.hip, warp_c4.hip, warp_maps.hip, warp_planes.hip and warp_nv12.hip a translation unit of its own, so that every existing code
// object stays what it is, instruction for instruction (tools/isa_compare.py): this file takes footprint_body and its helpers from warp_body.h
// and adds the kernel and its range launch.  Contract, registers and measurements: profiles/p010.md.
#include "warp_body.h"

namespace mf {

// warp_kernel's footprint order and ownership / coordinate code: the maps kernel's hot and pair shortcuts (the plan's certificates need no
// window here), footprint_body's general path for everything else, the crop flags folded into the same d_crop rows and clip rectangle as
// every pixel warp on the same table, then remap_store_u16c1: taps from global memory.  `frames` / `out`: [n][H][W] uint16 samples of THIS
// launch's frames; `border`: the border sample.
__global__ __launch_bounds__(64) void warp16c1_footprint(const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions, WarpGeom g,
                                                         const uint16_t* __restrict__ frames, const double* __restrict__ records,
                                                         uint16_t* __restrict__ out, const float* __restrict__ edges, int n, int W, int H, int C,
                                                         uint32_t border, int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint32_t f = blockIdx.y;
    const uint32_t t = ((blockIdx.x + f) & 7u) * g.per_xcd + (blockIdx.x >> 3);
    if (t >= g.per_frame) return;
    footprint_body<Px::U16C1, false, false>(f, t, plan, regions, g, reinterpret_cast<const uint8_t*>(frames), records, reinterpret_cast<uint8_t*>(out),
                                            edges, n, W, H, C, border, crop, clip);
}

// launch_warp's launch for one frame range of uint16 luma planes
void launch_warp16c1_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border, hipStream_t st)
{
    const dim3 grid(g.per_xcd * 8u, (uint32_t)r.m);
    hipLaunchKernelGGL(warp16c1_footprint, grid, dim3(64), 0, st, r.plan, r.regions, g, (const uint16_t*)r.frames, r.records, (uint16_t*)r.out,
                       r.edges, r.m, W, H, C, border, r.crop, r.bounds);
}

}  // namespace mf
