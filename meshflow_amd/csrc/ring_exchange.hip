// The pixels a lagged group owes (mf_ring_exchange_u8): per plane a ring [B][lag][N] of bytes on the device, frame t of stream b in slot
// t mod lag for as long as it is owed.  One launch per plane per tick stores the K new frames and hands out the frames whose slots they take.
// Bit for bit tests/ring_model.py's `exchange`; include/meshflow_hip.h has the contract.
//
// Per row r of `rows` [K][3] = (id, slot, out_row):
//   out_row >= 0   out[out_row] = ring[id][slot], then ring[id][slot] = new[r]
//   out_row <  0   ring[id][slot] = new[r]
// A row whose id is outside 0 .. B - 1, whose slot is outside 0 .. lag - 1 or whose out_row is K or more touches no memory.
//
// Mapping (gfx950): a streaming kernel in pack422.hip's form -- no LDS, no barriers, no atomics, nothing kept between lanes.  The grid is
// (chunks of CHUNK = 4096 bytes of a frame, K); workgroup (x, r) moves bytes [CHUNK x, min(CHUNK (x + 1), N)) of row r, 256 lanes.
//   wide   N is a multiple of 16 and the three base pointers are 16-byte aligned, so every row of every array is: lane l takes bytes
//          [CHUNK x + 16 l, + 16) with one dwordx4 load from `ring` (an emitting row), one from `new`, then the two dwordx4 stores
//   bytes  anything else: lane l takes bytes CHUNK x + l + 256 j, j = 0 .. 15, one byte each way, each below N by its own test
// Every byte of the ring is read by the lane that overwrites it and by no other, and the rows of one call are different streams (the
// caller's duty, as in the group smoother), so the exchange needs no ordering beyond a lane's own load-before-store.  `ring` is not
// __restrict__: it is read and written; `new` and `out` overlap nothing (the entry refuses an `out` that does; `new` is only read).
// Bounds: x < ceil(N / CHUNK) by the grid, r < K by the grid; wide: 16 l + 16 <= CHUNK and CHUNK x + 16 l < N with N % 16 == 0 gives the whole
// 16 bytes below N; row offsets are (id lag + slot) N < B lag N, r N < K N and out_row N < K N.
#include "mf_common.h"

namespace mf {

namespace ring {
constexpr int LANES = 256, CHUNK = 4096;                    // 16 bytes per lane
}

__global__ void __launch_bounds__(ring::LANES) ring_exchange_kernel(uint8_t* ring_bytes, const uint8_t* __restrict__ fresh, uint8_t* __restrict__ out,
                                                                    const int32_t* __restrict__ rows, int K, int B, int lag, uint64_t N, int wide)
{
    const uint64_t r = blockIdx.y;
    const int id = rows[3 * r], slot = rows[3 * r + 1], out_row = rows[3 * r + 2];
    if ((unsigned)id >= (unsigned)B || (unsigned)slot >= (unsigned)lag || out_row >= K) return;          // (workgroup-uniform)
    uint8_t* held = ring_bytes + ((uint64_t)id * (uint64_t)lag + (uint64_t)slot) * N;
    const uint8_t* __restrict__ from = fresh + r * N;
    const bool emit = out_row >= 0;
    uint8_t* __restrict__ to = out + (emit ? (uint64_t)out_row * N : 0);
    const uint64_t base = (uint64_t)blockIdx.x * ring::CHUNK;
    if (wide) {
        const uint64_t at = base + 16u * threadIdx.x;
        if (at >= N) return;
        const uint4 in = *reinterpret_cast<const uint4*>(from + at);
        if (emit) {
            const uint4 owed = *reinterpret_cast<const uint4*>(held + at);
            *reinterpret_cast<uint4*>(to + at) = owed;
        }
        *reinterpret_cast<uint4*>(held + at) = in;
        return;
    }
#pragma unroll 4
    for (int j = 0; j < ring::CHUNK / ring::LANES; ++j) {
        const uint64_t at = base + threadIdx.x + (uint64_t)j * ring::LANES;
        if (at >= N) break;
        const uint8_t in = from[at];
        if (emit) to[at] = held[at];
        held[at] = in;
    }
}

}  // namespace mf

using namespace mf;

extern "C" {

int mf_ring_exchange_u8(uint8_t* d_ring, const uint8_t* d_new, uint8_t* d_out, const int32_t* d_rows, int K, int B, int lag, int64_t N, void* stream)
{
    const char* name = "mf_ring_exchange_u8";
    if (K < 1 || B < 1 || lag < 1 || N < 1 || K > MF_ONLINE_GROUP_MAX_ROWS) {
        set_error("%s: K, B, lag and N must be at least 1 and K <= %d (got K=%d, B=%d, lag=%d, N=%lld)", name, MF_ONLINE_GROUP_MAX_ROWS, K, B, lag,
                  (long long)N);
        return MF_ERR_INVALID_ARG;
    }
    if (N > MF_RING_MAX_FRAME_BYTES || (unsigned __int128)B * (unsigned)lag * (uint64_t)N > (unsigned __int128)1 << 62) {
        set_error("%s: N must not exceed %lld and the ring B lag N must stay below 2^62 bytes (got B=%d, lag=%d, N=%lld)", name,
                  (long long)MF_RING_MAX_FRAME_BYTES, B, lag, (long long)N);
        return MF_ERR_INVALID_ARG;
    }
    if (!d_ring || !d_new || !d_out || !d_rows) { set_error("%s: null pointer", name); return MF_ERR_INVALID_ARG; }
    if ((uintptr_t)d_rows & 3) { set_error("%s: d_rows must be 4-byte aligned", name); return MF_ERR_INVALID_ARG; }
    // (d_out holds at most K frames: the rows' out_row are on the device, and one of K or more is skipped by the kernel)
    const uintptr_t g = (uintptr_t)d_ring, f = (uintptr_t)d_new, o = (uintptr_t)d_out;
    const size_t frame = (size_t)N, ring_bytes = (size_t)B * (size_t)lag * frame, row_bytes = (size_t)K * frame;
    if ((o < g + ring_bytes && g < o + row_bytes) || (o < f + row_bytes && f < o + row_bytes)) {
        set_error("%s: d_out overlaps d_ring or d_new", name);
        return MF_ERR_INVALID_ARG;
    }
    if (f < g + ring_bytes && g < f + row_bytes) { set_error("%s: d_new overlaps d_ring", name); return MF_ERR_INVALID_ARG; }
    const int wide = frame % 16 == 0 && ((g | f | o) & 15) == 0;
    const size_t chunks = (frame + ring::CHUNK - 1) / ring::CHUNK;         // <= 2^31 - 1 by MF_RING_MAX_FRAME_BYTES
    hipLaunchKernelGGL(ring_exchange_kernel, dim3((unsigned)chunks, (unsigned)K), dim3(ring::LANES), 0, (hipStream_t)stream, d_ring, d_new, d_out,
                       d_rows, K, B, lag, (uint64_t)N, wide);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

}  // extern "C"
