// The frame signature's arithmetic, the same on host and device: integers only (tests/cuts_model.py).
//   tiles     4 x 4; tile row i covers rows [floor(i H / 4), floor((i + 1) H / 4)), tile columns split W the same way (a tile may be empty)
//   counters  16 per tile, counter b = the number of the tile's pixels with value >> 4 == b; [tile_row][tile_col][bin], 256 per frame
// How a lane counts 16 pixels without a branch on their values and without touching memory:
//   Block     16 consecutive bytes of the stack as two 64-bit words; the bytes outside the lane's piece of a tile row are zeroed and counted
//             in `pad`: a zeroed byte lands in bin 0, and `pad` is taken off bin 0 again
//   nibbles   each pixel adds 1 << 4 bin to a 64-bit word of sixteen 4-bit counters; 8 pixels per word, so no nibble passes 8
//   bytes     the even and the odd nibbles of the two words are added into two 64-bit words of eight 8-bit counters: byte m of `even` is
//             bin 2 m, byte m of `odd` bin 2 m + 1.  A block adds at most 16 to a byte, so FLUSH = 14 blocks stay below 256 ...
//   counters  ... and are then added to the lane's sixteen 32-bit counters, which are registers: every index is a compile-time constant
// The cost is the same whatever the pixels are: a flat frame and a noisy one run the same instructions.
#pragma once
#include <stdint.h>

namespace mf {
namespace cuts {

constexpr int TILES = 4;                    // per side
constexpr int BINS = 16;
constexpr int COUNTERS = TILES * TILES * BINS;
constexpr int LANES = 256;
constexpr int FLUSH = 14;                   // blocks between two flushes of the byte counters: 14 * 16 = 224 < 256
constexpr int MAX_DIM = 32767;
constexpr int TARGET_GROUPS = 1024;         // workgroups a launch should have at least, where the frames are large enough to be cut that far
constexpr int GROUP_PIXELS_MIN = LANES * 16;        // ... but no strip below one block per lane,
constexpr int GROUP_PIXELS_MAX = 8 * LANES * 16;    // and none above eight where the clip has frames enough
constexpr int MAX_GROUPS = 1 << 20;         // per launch; the host strides over the frames of a longer clip

__host__ __device__ inline int tile_edge(int i, int size) { return (int)((unsigned)i * (unsigned)size / TILES); }      // i <= 4, size <= 32767

// strips a tile's rows are cut into (the same for all 16 tiles and every frame of a call): from the largest tile, ceil(H / 4) x ceil(W / 4)
inline int strips_for(int n, int W, int H)
{
    const long long th = (H + TILES - 1) / TILES, tile_pixels = th * ((W + TILES - 1) / TILES);
    const long long per_tile = TILES * TILES * (long long)n;
    long long want = (TARGET_GROUPS + per_tile - 1) / per_tile;
    const long long by_size = (tile_pixels + GROUP_PIXELS_MAX - 1) / GROUP_PIXELS_MAX;
    if (want < by_size) want = by_size;
    long long cap = tile_pixels / GROUP_PIXELS_MIN;
    if (cap > th) cap = th;
    if (cap < 1) cap = 1;
    return (int)(want < cap ? want : cap);
}

struct Block { uint64_t lo, hi; uint32_t pad; };

// the k low bytes of a 64-bit word set, k in 0 .. 8
__host__ __device__ inline uint64_t low_bytes(uint32_t k) { return k >= 8 ? ~0ull : (1ull << (8 * k)) - 1ull; }

// keep bytes [from, to) of the block, 0 <= from <= to <= 16
__host__ __device__ inline void keep(Block& b, uint32_t from, uint32_t to)
{
    const uint32_t f0 = from < 8 ? from : 8, t0 = to < 8 ? to : 8;
    b.lo &= low_bytes(t0) & ~low_bytes(f0);
    b.hi &= low_bytes(to - t0) & ~low_bytes(from - f0);
    b.pad = 16 - (to - from);
}

__host__ __device__ inline uint64_t nibbles_of(uint64_t eight_pixels)
{
    const uint32_t w[2] = { (uint32_t)eight_pixels, (uint32_t)(eight_pixels >> 32) };
    uint64_t acc = 0;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += 1ull << ((w[d] >> (8 * k + 2)) & 0x3Cu);          // 4 * (pixel >> 4)
    return acc;
}

struct ByteCounts { uint64_t even, odd; };

__host__ __device__ inline void add_block(ByteCounts& c, const Block& b)
{
    constexpr uint64_t M = 0x0F0F0F0F0F0F0F0Full;
    const uint64_t p = nibbles_of(b.lo), q = nibbles_of(b.hi);
    c.even += (p & M) + (q & M) - b.pad;                  // (bin 0's byte holds at least the pad zeroes: no borrow)
    c.odd += ((p >> 4) & M) + ((q >> 4) & M);
}

__host__ __device__ inline void flush(ByteCounts& c, uint32_t (&count)[BINS])
{
#pragma unroll
    for (int m = 0; m < BINS / 2; ++m) {
        count[2 * m] += (uint32_t)(c.even >> (8 * m)) & 255u;
        count[2 * m + 1] += (uint32_t)(c.odd >> (8 * m)) & 255u;
    }
    c.even = c.odd = 0;
}

// The 16-byte block at grid offset V = (v0 rounded down to 16) + 16 blk of the stack, reduced to the bytes of the run [v0, v1): empty where the
// block lies behind the run, or where `any` is false.  `grid` = the stack's address rounded down to 16 bytes, `mis` = the stack's first byte
// in that grid, `total` its bytes.  A block is loaded whole only where [V, V + 16) lies inside the stack; elsewhere the run's bytes one by one.
struct alignas(16) Quad { uint32_t x, y, z, w; };

__host__ __device__ inline Block fetch(const uint8_t* __restrict__ grid, uint64_t mis, uint64_t total, uint64_t v0, uint64_t v1, uint32_t blk, bool any)
{
    Block b = { 0, 0, 16 };
    const uint64_t V = (v0 & ~15ull) + 16ull * blk;
    if (!any || V >= v1) return b;
    const uint32_t from = v0 > V ? (uint32_t)(v0 - V) : 0u, to = v1 < V + 16 ? (uint32_t)(v1 - V) : 16u;
    if (V >= mis && V + 16 <= mis + total) {
        const Quad v = *reinterpret_cast<const Quad*>(grid + V);
        b.lo = v.x | (uint64_t)v.y << 32;
        b.hi = v.z | (uint64_t)v.w << 32;
        if (from != 0 || to != 16) keep(b, from, to);
        else b.pad = 0;
    } else {
        for (uint32_t k = from; k < to; ++k) {
            const uint64_t px = grid[V + k];
            if (k < 8) b.lo |= px << (8 * k);
            else b.hi |= px << (8 * (k - 8));
        }
        b.pad = 16 - (to - from);
    }
    return b;
}

// What lane `tid` of the workgroup of (frame, tile, strip) counts: the strip's (row, block) pairs q = tid, tid + 256, ... in row-major order, two
// per pass so that two loads are in flight.  A row has at most tw / 16 + 2 blocks (a run of tw bytes that starts at byte a of a block ends in
// block (a + tw - 1) / 16 <= tw / 16 + 1).  False where the strip is empty (the same for every lane of the workgroup).
__host__ __device__ inline bool lane_counts(const uint8_t* __restrict__ grid, uint64_t mis, uint64_t total, int W, int H, int strips, uint32_t frame,
                                            int tile, int strip, uint32_t tid, uint32_t (&count)[BINS])
{
    const int r0 = tile_edge(tile / TILES, H), th = tile_edge(tile / TILES + 1, H) - r0;
    const int c0 = tile_edge(tile % TILES, W), tw = tile_edge(tile % TILES + 1, W) - c0;
    const int ra = r0 + (int)((long long)strip * th / strips), rb = r0 + (int)((long long)(strip + 1) * th / strips);
    if (tw < 1 || rb <= ra) return false;
    const uint32_t nb = (uint32_t)tw / 16u + 2u, items = (uint32_t)(rb - ra) * nb;       // <= 8192 * 514
    const uint32_t drow = LANES / nb, dblk = LANES % nb;
    uint32_t row = tid / nb, blk = tid % nb;
    const uint64_t origin = mis + ((uint64_t)frame * (uint64_t)H + (uint64_t)ra) * (uint64_t)W + (uint64_t)c0;
#pragma unroll
    for (int b = 0; b < BINS; ++b) count[b] = 0;
    ByteCounts bytes = { 0, 0 };
    int pending = 0;
    for (uint32_t q = tid; q < items; q += 2 * LANES) {
        const uint64_t v0 = origin + (uint64_t)row * (uint64_t)W;
        const Block first = fetch(grid, mis, total, v0, v0 + (uint64_t)tw, blk, true);
        blk += dblk; row += drow;
        if (blk >= nb) { blk -= nb; ++row; }
        const uint64_t u0 = origin + (uint64_t)row * (uint64_t)W;
        const Block second = fetch(grid, mis, total, u0, u0 + (uint64_t)tw, blk, q + LANES < items);
        blk += dblk; row += drow;
        if (blk >= nb) { blk -= nb; ++row; }
        add_block(bytes, first);
        add_block(bytes, second);
        pending += 2;
        if (pending == FLUSH) { flush(bytes, count); pending = 0; }
    }
    flush(bytes, count);
    return true;
}

}  // namespace cuts
}  // namespace mf
