// Kernel 2b WITHOUT the pixels (mf_warp_maps_f32, mf_warp_maps_bounds_f32): footprint_body's MAPS instantiation, which stores the float32 source
// coordinates (u, v) of every output pixel -- the reference's frame_stabilized_x_y, mfs.py:1054-1061, the arrays it hands to cv2.remap at
// mfs.py:1063-1069 -- instead of sampling a frame with them.  Like warp_c1.hip and warp_c4.hip, a translation unit of its own, so that warp.hip's
// code object -- and with it every existing kernel, instruction for instruction (tools/isa_compare.py) -- stays what it is: this file takes
// footprint_body and its helpers from warp_body.h and adds the maps kernel and its range launch.  Design and measurements: profiles/warp_maps.md.
#include "warp_body.h"

namespace mf {

// warp_kernel's footprint order and ownership / coordinate code: the grey warp's hot and pair shortcuts (the plan's certificates need no window
// here), footprint_body's general path for everything else, the crop flags folded into the same d_crop rows and clip rectangle as every pixel
// warp on the same table, then maps_store_f32.  It reads the cell table and nothing else; `maps`: float32 [n][H][W][2] of THIS launch's frames.
__global__ __launch_bounds__(64) void maps_footprint(const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions, WarpGeom g,
                                                     const double* __restrict__ records, float* __restrict__ maps,
                                                     const float* __restrict__ edges, int n, int W, int H, int C,
                                                     int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint32_t f = blockIdx.y;
    const uint32_t t = ((blockIdx.x + f) & 7u) * g.per_xcd + (blockIdx.x >> 3);
    if (t >= g.per_frame) return;
    footprint_body<Px::MAPS, false, false>(f, t, plan, regions, g, nullptr, records, reinterpret_cast<uint8_t*>(maps), edges, n, W, H, C, 0u, crop, clip);
}

// launch_warp's launch for one frame range of the maps (r.out: the range's first frame, r.frames unused)
void launch_maps_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, hipStream_t st)
{
    const dim3 grid(g.per_xcd * 8u, (uint32_t)r.m);
    hipLaunchKernelGGL(maps_footprint, grid, dim3(64), 0, st, r.plan, r.regions, g, r.records, (float*)r.out, r.edges, r.m, W, H, C, r.crop, r.bounds);
}

}  // namespace mf
