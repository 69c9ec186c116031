// The luma of a colour or 16-bit sample, the arithmetic of tests/luma_model.py: integers only, the same on host and device.
//   8-bit  BGR(A):  (b 3735 + g 19235 + r 9798 + 16384) >> 15      OpenCV's 8U COLOR_BGR2GRAY: 15-bit coefficients that sum to 32768
//   16-bit BGR:    ((b 1868 + g 9617 + r 4899 + 8192) >> 14) >> 8   OpenCV's 16U path (14-bit coefficients that sum to 16384), then the high
//                                                                   byte, TRUNCATED: cv2's FAST takes no 16-bit image, so the rule is this
//                                                                   project's own, and the same as for a 16-bit luma plane
//   16-bit plane:   y >> 8                                          P010 / P012 / P016 samples are MSB-aligned
// red_first swaps the roles of channels 0 and 2 (COLOR_RGB2GRAY); channel 3 of a 4-channel pixel is never read into the result.
#pragma once
#include <stdint.h>

namespace mf {
namespace luma {

enum Src { U8C3 = 0, U8C4 = 1, U16C3 = 2, U16C1 = 3 };

constexpr int RUN = 16;                     // pixels per lane: one 16-byte store
constexpr int LANES = 256;
constexpr int MAX_BLOCKS = 1 << 16;         // per launch: 2^24 runs = 2^28 pixels (129 frames of 1080p); the host strides over the rest
constexpr int MAX_DIM = 32767;

template <int SRC> struct Traits;
template <> struct Traits<U8C3> { static constexpr int channels = 3, sample_bytes = 1; };
template <> struct Traits<U8C4> { static constexpr int channels = 4, sample_bytes = 1; };
template <> struct Traits<U16C3> { static constexpr int channels = 3, sample_bytes = 2; };
template <> struct Traits<U16C1> { static constexpr int channels = 1, sample_bytes = 2; };

// the weights of channels 0, 1 and 2
struct Weights { uint32_t c0, c1, c2; };

template <int SRC> __host__ __device__ inline Weights weights(int red_first)
{
    if (Traits<SRC>::sample_bytes == 1) return red_first ? Weights{9798u, 19235u, 3735u} : Weights{3735u, 19235u, 9798u};
    return red_first ? Weights{4899u, 9617u, 1868u} : Weights{1868u, 9617u, 4899u};
}

// (the largest sums are 255 * 32768 + 16384 and 65535 * 16384 + 8192: both below 2^32)
__host__ __device__ inline uint32_t y8(uint32_t s0, uint32_t s1, uint32_t s2, const Weights& w) { return (s0 * w.c0 + s1 * w.c1 + s2 * w.c2 + 16384u) >> 15; }
__host__ __device__ inline uint32_t y16(uint32_t s0, uint32_t s1, uint32_t s2, const Weights& w)
{
    return ((s0 * w.c0 + s1 * w.c1 + s2 * w.c2 + 8192u) >> 14) >> 8;
}

}  // namespace luma
}  // namespace mf
