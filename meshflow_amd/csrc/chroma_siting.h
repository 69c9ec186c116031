// Where the chroma samples of a 4:2:0 crop-resize sit: the one definition behind the chroma tables of the NV12 calls (chroma_tables_kernel,
// resize_uv_body.h) and of the P010 calls (hdr_uv_tables_kernel, resize_hdr_body.h).  Every size and edge is the LUMA frame's.
//
// Chroma is sited at the even luma sample, as in the warps: output chroma sample cx sits on output luma pixel 2 cx; its source is that pixel's
// luma source position (cv2.resize's, resize_body.h), made absolute in the frame and halved:
//   scale = 1 / ((double)oW / cw)                                              (the luma tables' own value)
//   fc = float((left + ((2 cx + 0.5) scale - 0.5)) 0.5);  s = floor(fc);  f = fc - s
//   c1 = right >> 1,  c0 = min((left + 1) >> 1, c1)                            (the chroma samples whose siting luma pixel lies in the crop)
//   x axis: s < c0 -> (c0, 0);  s >= c1 -> (c1, 0)        y axis: the two row indices are clipped to [r0, r1] instead, the fraction kept
// The positions are ABSOLUTE chroma columns and rows of the plane; they depend on the parity of left and top.  The float64 operations stand in
// this order: the build is -ffp-contract=off and the tests' models repeat them bit for bit.
// Results leave through references, the fraction declared ahead of the index at the call, and the rows are clipped in a step of their own
// (chroma_tables_kernel rounds its weights in between): in this shape both kernels compile to the listings they had with the arithmetic
// written out in each (tools/isa_compare.py).
#ifndef MF_CHROMA_SITING_H
#define MF_CHROMA_SITING_H
#include "mf_common.h"

namespace mf {

// s and f of output chroma sample i along one axis, before the crop's edges: `lo` the crop's first luma column (row), `scale` that axis' luma
// scale.  The y axis keeps this fraction.
__device__ __forceinline__ void chroma_site(int i, int lo, double scale, int& s, float& f)
{
    f = (float)(((double)lo + (((double)(2 * i) + 0.5) * scale - 0.5)) * 0.5);
    s = (int)floorf(f);
    f -= (float)s;
}

// the first and last chroma column (row) whose siting luma pixel lies in the crop lo .. hi: c0 and c1 (r0 and r1)
__device__ __forceinline__ void chroma_site_range(int lo, int hi, int& first, int& last)
{
    last = hi >> 1;
    first = min((lo + 1) >> 1, last);
}

// x axis: the column sx clamped into c0 .. c1 and its fraction fx, 0 where the column was clamped
__device__ __forceinline__ void chroma_site_x(int i, int lo, double scale, int c0, int c1, int& sx, float& fx)
{
    chroma_site(i, lo, scale, sx, fx);
    if (sx < c0) { fx = 0.0f; sx = c0; }
    if (sx >= c1) { fx = 0.0f; sx = c1; }
}

// y axis: the rows sy and sy + 1 of chroma_site, each clipped into r0 .. r1, as sy0 | sy1 << 16
__device__ __forceinline__ int chroma_site_rows(int sy, int r0, int r1)
{
    const int sy0 = min(max(sy, r0), r1), sy1 = min(max(sy + 1, r0), r1);
    return sy0 | (sy1 << 16);
}

}  // namespace mf

#endif  // MF_CHROMA_SITING_H
