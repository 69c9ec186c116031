// Kernel 2b for the chroma plane of a P210 / P212 / P216 clip -- 10-bit 4:2:2, what SDI / HDMI capture and ProRes / XAVC decoders deliver
// (mf_warp_p210, mf_warp_bounds_p210): footprint_body's P210_UV instantiation -- the interleaved half-WIDTH plane [n][H][W/2][2] of uint16
// samples, U first, sampled like cv2.remap INTER_LINEAR / BORDER_CONSTANT of CV_16UC2 at (u / 2, v) of the coordinates the reference hands to
// cv2.remap at mfs.py:1063-1069 for the even luma pixels of every row.  The luma plane's kernel is warp16c1_footprint (warp_c1_16.hip),
// launched unchanged in front of this one.  A translation unit of its own, like warp_nv16.hip and warp_p010.hip, so that every existing code
// object stays what it is, instruction for instruction (tools/isa_compare.py).  Contract, registers and measurements: profiles/p210.md.
#include "warp_body.h"

namespace mf {

// nv16_chroma_footprint on 4-byte pixels (or p010_chroma_footprint on a plane of full height): the LUMA frame's plan (W, H: the luma size),
// the maps kernel's hot and pair shortcuts, footprint_body's general path for everything else, then remap_store_chroma -- a lane owns four
// consecutive luma pixels, the lanes of EVERY row emit the chroma samples of their pixels 0 and 2 as one 8-byte store.  It reads the cell
// table and the chroma plane, uses no atomic and never touches the crop rows or the clip rectangle.  `uv` / `out`: [n][H][W/2][2] uint16
// samples of THIS launch's frames; `border`: U | V << 16.
__global__ __launch_bounds__(64) void p210_chroma_footprint(const FootPlan* __restrict__ plan, const FootRegion* __restrict__ regions, WarpGeom g,
                                                            const uint16_t* __restrict__ uv, const double* __restrict__ records,
                                                            uint16_t* __restrict__ out, const float* __restrict__ edges, int n, int W, int H, int C,
                                                            uint32_t border)
{
    const uint32_t f = blockIdx.y;
    const uint32_t t = ((blockIdx.x + f) & 7u) * g.per_xcd + (blockIdx.x >> 3);
    if (t >= g.per_frame) return;
    footprint_body<Px::P210_UV, false, false>(f, t, plan, regions, g, reinterpret_cast<const uint8_t*>(uv), records, reinterpret_cast<uint8_t*>(out),
                                              edges, n, W, H, C, border, nullptr, nullptr);
}

// launch_warp's launch for one frame range of chroma planes (r.frames / r.out advanced by px_frame_bytes per frame; r.crop, r.bounds unused)
void launch_p210_chroma_range(const WarpGeom& g, const WarpRange& r, int W, int H, int C, uint32_t border_uv, hipStream_t st)
{
    const dim3 grid(g.per_xcd * 8u, (uint32_t)r.m);
    hipLaunchKernelGGL(p210_chroma_footprint, grid, dim3(64), 0, st, r.plan, r.regions, g, (const uint16_t*)r.frames, r.records, (uint16_t*)r.out,
                       r.edges, r.m, W, H, C, border_uv);
}

}  // namespace mf
