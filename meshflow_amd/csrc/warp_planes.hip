// Kernel 2b for the side planes of a video (mf_warp_plane_f32, mf_warp_plane_nearest): footprint_body's PLANE_* instantiations -- float32
// planes [n][H][W] sampled like cv2.remap INTER_LINEAR of CV_32FC1, and elements of 1, 2, 4 or 8 bytes copied like INTER_NEAREST, both
// BORDER_CONSTANT (the arrays the reference hands to cv2.remap at mfs.py:1063-1069, applied to a plane instead of the colour frame).  Like
// warp_c1.hip, warp_c4.hip and warp_maps.hip a translation unit of its own, so that every existing code object stays what it is,
// instruction for instruction (tools/isa_compare.py): this file takes footprint_body and its helpers from warp_body.h and adds the plane
// kernels and their range launch.  Contract, registers and measurements: profiles/planes.md.
#include "warp_body.h"

namespace mf {

// warp_kernel's footprint order and ownership / coordinate code: the maps kernel's hot and pair shortcuts (the plan's certificates need no
// window here either), footprint_body's general path for everything else, the crop flags folded into the same d_crop rows and clip rectangle
// as every pixel warp on the same table, then remap_store_plane: taps from global memory, `fill` where the source lies outside the plane.
// `planes` / `out`: [n][H][W] elements of px_sample_bytes(PX) bytes of THIS launch's frames; `fill`: the element's bit pattern.
template <Px PX>
__global__ __launch_bounds__(64) void plane_footprint(const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions, WarpGeom g,
                                                      const uint8_t* __restrict__ planes, const double* __restrict__ records,
                                                      uint8_t* __restrict__ out, const float* __restrict__ edges, int n, int W, int H, int C,
                                                      uint64_t fill, int32_t* __restrict__ crop, int32_t* __restrict__ clip)
{
    const uint32_t f = blockIdx.y;
    const uint32_t t = ((blockIdx.x + f) & 7u) * g.per_xcd + (blockIdx.x >> 3);
    if (t >= g.per_frame) return;
    footprint_body<PX, false, false>(f, t, plan, regions, g, planes, records, out, edges, n, W, H, C, 0u, crop, clip, fill);
}

template <Px PX>
static void launch_plane(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint64_t fill, hipStream_t st)
{
    const dim3 grid(g.per_xcd * 8u, (uint32_t)r.m);
    hipLaunchKernelGGL(plane_footprint<PX>, grid, dim3(64), 0, st, r.plan, r.regions, g, (const uint8_t*)r.frames, r.records, (uint8_t*)r.out,
                       r.edges, r.m, W, H, C, fill, r.crop, r.bounds);
}

// launch_warp's launch for one frame range of planes of format px
void launch_plane_range(Px px, const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint64_t fill, hipStream_t st)
{
    switch (px) {
    case Px::PLANE_F32: launch_plane<Px::PLANE_F32>(g, r, W, H, C, fill, st); break;
    case Px::PLANE_N1: launch_plane<Px::PLANE_N1>(g, r, W, H, C, fill, st); break;
    case Px::PLANE_N2: launch_plane<Px::PLANE_N2>(g, r, W, H, C, fill, st); break;
    case Px::PLANE_N4: launch_plane<Px::PLANE_N4>(g, r, W, H, C, fill, st); break;
    default: launch_plane<Px::PLANE_N8>(g, r, W, H, C, fill, st); break;
    }
}

}  // namespace mf
