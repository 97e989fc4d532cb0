// Launch interface of the stereo / RGB-D depth stage (stereo.hip) for the extractor's one-call forms (orb.hip).
#pragma once
#include "common.hpp"

namespace uh {

// Everything is device-visible memory.  Counts: n_* bounds the launch; d_n_* (may be NULL) is the device-side count, used as min(*d_n, n).
struct StereoLaunch {
    const uint8_t* left; size_t left_stride; const uint8_t* right; size_t right_stride; int cols, rows;
    const float* l_xy; int l_xy_stride;       // undistorted left positions: x at l_xy[i * stride], y behind it
    const int* l_oct; int l_oct_stride;       // left octaves
    const uint8_t* l_desc;                    // n x 32, 16-byte aligned
    int n_left; const int* d_n_left;
    const uh_keypoint* r_kps; const uint8_t* r_desc;   // right keypoints (pt, octave read) and descriptors (16-byte aligned)
    int n_right; const int* d_n_right;
    float blfx, max_desc_dist;
    float* depth;                             // n_left floats out
    int* match;                               // n_left ints out (matched right index or -1): always written
    int* row_ptr;                             // rows + 1 ints of scratch
    int* row_idx;                             // n_right ints of scratch
};
constexpr int kStereoMaxRows = 8192;          // st_bucket_kernel keeps the row counters in LDS
int stereo_launch(uh_ctx* ctx, const StereoLaunch& a);
int rgbd_launch(uh_ctx* ctx, const uh_keypoint* kps, int n, const int* d_n, const uint16_t* depth_img, size_t stride_px, int cols, int rows,
                float scale, float* depth);

}  // namespace uh
