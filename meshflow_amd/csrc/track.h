// The device tracker's launchers (track_fast.hip, track_pyr.hip, track_lk.hip, track_ransac.hip, track_fit.hip) behind capi.hip's checks.
#pragma once
#include "mf_common.h"
#include "track_body.h"
#include "ransac_body.h"
#include "hfit_body.h"

namespace mf {

// bytes of the mask of corner flags (FAST) and of pyramid levels 1-3 of both stacks (LK); the workspace is the larger of the two
size_t track_mask_bytes(const track::Geom& g, int n);
size_t track_pyramid_bytes(const track::Geom& g, int n_pairs);
// where pyramid level `level` (1-3) starts in the workspace, and the pitch and height of one of its 2 * n_pairs * S sub-images
size_t track_level_offset(const track::Geom& g, int n_pairs, int level);
int launch_fast_corners(const uint8_t* grey, int n, const track::Geom& g, int max_per, int threshold, float* points, int32_t* counts,
                        int32_t* status, void* work, hipStream_t st);
int launch_pyramid(const uint8_t* early, const uint8_t* late, int n_pairs, const track::Geom& g, void* work, hipStream_t st);
int launch_lk_levels(const uint8_t* early, const uint8_t* late, int n_pairs, const track::Geom& g, int max_per, const float* points,
                     const int32_t* counts, float* moved, uint8_t* found, const void* work, hipStream_t st);
// track_ransac.hip: the outlier step per sub-frame (workspace: the compacted candidates of sub-frames beyond ransac::STAGED) and the gather
// of the survivors into mf_vertex_motion_f64's layout
size_t ransac_workspace_bytes(int n_pairs, int S, int max_per);
int launch_ransac(const float* points, const float* moved, const int32_t* counts, const uint8_t* found, int n_pairs, int S, int max_per,
                  int min_features, double threshold, double confidence, int max_iters, uint32_t seed, uint8_t* inlier, int32_t* info, void* work,
                  hipStream_t st);
int launch_track_gather(const float* points, const float* moved, const uint8_t* inlier, const int32_t* info, int n_pairs, const track::Geom& g,
                        int max_per, int min_features, double* early, double* late, int32_t* offsets, int32_t* pair_status, hipStream_t st);
// track_fit.hip: the homography over each pair's packed survivors (workspace: the 23 sums of each pair's normal matrix between its two kernels)
size_t hfit_workspace_bytes(int n_pairs);
int launch_homography_fit(const double* early, const double* late, const int32_t* offsets, int n_pairs, int K_total, double* hom, int32_t* info,
                          double* diag, void* work, hipStream_t st);

}  // namespace mf
