// Scene-cut statistics of a resident luma stack: the per-frame signature of 4 x 4 tile histograms (mf_frame_signature_u8) and the distance of
// adjacent signatures (mf_cut_distance_i32).  Bit for bit tests/cuts_model.py; the arithmetic is cuts_body.h's.  Integers only: any order of
// summation gives the same bytes.
//
// signature_kernel: a streaming read of the n H W bytes.  One workgroup of 256 lanes takes one STRIP of one tile of one frame: the tile's rows
// are cut into `strips` runs of rows (cuts::strips_for: a one-frame push of 1080p becomes 496 workgroups, not 16; 32 frames become 2,048).
//   blocks    a tile row is a run of bytes that starts anywhere (an odd W moves it on every row).  It is read as the 16-byte ALIGNED blocks that
//             cover it, one dwordx4 load per lane and block, with the bytes outside the run zeroed afterwards (cuts::keep) -- those bytes belong
//             to the neighbouring tile, row or frame of the same stack.  Only a block that reaches outside the stack itself (the first and the
//             last one of a stack that does not start or end on a 16-byte boundary) is read byte by byte, and then only its bytes of the run.
//             A row has at most tw / 16 + 2 blocks; the strip's (row, block) pairs are dealt to the lanes in order, two per lane and pass so
//             that two loads are in flight, and a pair past the row's last block is an empty block.
//   counting  per lane, in registers, with no branch on a pixel's value (cuts_body.h): a black frame costs what a noisy one costs, and no two
//             lanes ever share a counter.  No LDS atomics.
//   combining the 256 lanes' sixteen counters go through LDS once ([bin][lane], plain stores), 16 lanes sum each bin, and ONE lane per bin adds
//             the strip's count to d_sig with an integer atomicAdd -- at most 16 adds per workgroup, onto counters the entry has zeroed with
//             a memset on the same stream.  Integer addition commutes, so the bytes do not depend on the order the strips arrive in.  (The
//             other choice, partial signatures and a second pass, needs a workspace the call does not have, and a launch more.)
// Bounds: frame < n, row < H and the run lies inside its row, so every byte read individually is a byte of the stack; a block is loaded whole
// only when [V, V + 16) lies inside [mis, mis + total), the stack's own bytes in the 16-byte grid of its address.  d_sig: frame < n, tile < 16,
// bin < 16.  LDS: [16][256] words, bin < 16, lane < 256.
//
// distance_kernel: one workgroup of 256 lanes per frame, lane c takes counter c of the frame and of the one before (d_sig_prev for frame 0;
// without it frame 0's distance is 0), |a - b| summed over the workgroup in a fixed tree.  No atomics.  A distance is at most 2 H W < 2^31.
// distance_pairs_kernel: the same workgroup with row r's predecessor taken from a second stack, prev[r] (mf_cut_distance_pairs_i32).
#include "mf_common.h"
#include "cuts_body.h"

namespace mf {

__global__ void __launch_bounds__(cuts::LANES) signature_kernel(const uint8_t* __restrict__ grid, uint32_t mis, uint64_t total, int W, int H,
                                                                int strips, int32_t* __restrict__ sig)
{
    constexpr int LANES = cuts::LANES, BINS = cuts::BINS, T = cuts::TILES;
    __shared__ uint32_t part[BINS][LANES];
    const uint32_t tid = threadIdx.x;
    const uint32_t per_frame = (uint32_t)(T * T * strips);
    const uint32_t frame = blockIdx.x / per_frame, rest = blockIdx.x % per_frame;
    const int tile = (int)(rest / (uint32_t)strips), strip = (int)(rest % (uint32_t)strips);
    uint32_t count[BINS];
    if (!cuts::lane_counts(grid, mis, total, W, H, strips, frame, tile, strip, tid, count)) return;          // (workgroup-uniform)

#pragma unroll
    for (int b = 0; b < BINS; ++b) part[b][tid] = count[b];
    __syncthreads();
    const uint32_t bin = tid >> 4, lane16 = tid & 15u;
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < LANES / 16; ++j) sum += part[bin][lane16 + 16 * j];
#pragma unroll
    for (int step = 8; step >= 1; step >>= 1) sum += __shfl_xor(sum, step, 16);
    if (lane16 == 0 && sum != 0) atomicAdd(sig + ((size_t)frame * cuts::COUNTERS + (size_t)tile * BINS + bin), (int32_t)sum);
}

// *dist = the distance of the signatures `before` (null: 0) and `now`, by the workgroup's 256 lanes.
__device__ __forceinline__ void store_distance(const int32_t* __restrict__ before, const int32_t* __restrict__ now, int32_t* __restrict__ dist)
{
    __shared__ uint32_t waves[cuts::LANES / 64];
    const uint32_t tid = threadIdx.x;
    uint32_t d = 0;
    if (before) {
        const int32_t a = before[tid], b = now[tid];
        d = (uint32_t)(a > b ? a - b : b - a);
    }
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) d += __shfl_xor(d, step, 64);
    if ((tid & 63u) == 0) waves[tid >> 6] = d;
    __syncthreads();
    if (tid == 0) *dist = (int32_t)((waves[0] + waves[1]) + (waves[2] + waves[3]));
}

__global__ void __launch_bounds__(cuts::LANES) distance_kernel(const int32_t* __restrict__ prev, const int32_t* __restrict__ sig,
                                                               int32_t* __restrict__ dist)
{
    const size_t frame = blockIdx.x;
    store_distance(frame ? sig + (frame - 1) * cuts::COUNTERS : prev, sig + frame * cuts::COUNTERS, dist + frame);
}

// Row r against ITS OWN predecessor prev[r] (mf_cut_distance_pairs_i32): the rows are frames of different streams.
__global__ void __launch_bounds__(cuts::LANES) distance_pairs_kernel(const int32_t* __restrict__ prev, const int32_t* __restrict__ sig,
                                                                     int32_t* __restrict__ dist)
{
    const size_t row = blockIdx.x;
    store_distance(prev + row * cuts::COUNTERS, sig + row * cuts::COUNTERS, dist + row);
}

int launch_frame_signature(const uint8_t* luma, int n, int W, int H, int32_t* sig, hipStream_t st)
{
    MF_HIP_TRY(hipMemsetAsync(sig, 0, (size_t)n * cuts::COUNTERS * sizeof(int32_t), st));
    const int strips = cuts::strips_for(n, W, H);
    const int per_frame = cuts::TILES * cuts::TILES * strips, frames_per_launch = cuts::MAX_GROUPS / per_frame;         // >= 1: strips <= 8192
    const uintptr_t at = (uintptr_t)luma;
    const uint64_t frame_bytes = (uint64_t)W * (uint64_t)H;
    for (long long first = 0; first < n; first += frames_per_launch) {                    // (64-bit: n may be within a launch of 2^31)
        const int frames = n - first < frames_per_launch ? (int)(n - first) : frames_per_launch;
        // (each launch sees its own frames as the stack: blocks are loaded whole inside them only, which is inside the caller's stack)
        const uintptr_t start = at + (uintptr_t)(first * frame_bytes), mis = start & 15u;
        hipLaunchKernelGGL(signature_kernel, dim3((unsigned)(frames * per_frame)), dim3(cuts::LANES), 0, st,
                           reinterpret_cast<const uint8_t*>(start - mis), (uint32_t)mis, frame_bytes * (uint64_t)frames, W, H, strips,
                           sig + (size_t)first * cuts::COUNTERS);
        MF_HIP_TRY(hipGetLastError());
    }
    return MF_OK;
}

int launch_cut_distance(const int32_t* prev, const int32_t* sig, int n, int32_t* dist, hipStream_t st)
{
    hipLaunchKernelGGL(distance_kernel, dim3((unsigned)n), dim3(cuts::LANES), 0, st, prev, sig, dist);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

int launch_cut_distance_pairs(const int32_t* prev, const int32_t* sig, int n, int32_t* dist, hipStream_t st)
{
    hipLaunchKernelGGL(distance_pairs_kernel, dim3((unsigned)n), dim3(cuts::LANES), 0, st, prev, sig, dist);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

}  // namespace mf
