// Frames shaped like ucoslam::Frame as far as the new-map-point adaptors read it (include/ucoslam_hip/adaptors.hpp: Triangulate,
// NewPointCreator): idx, pose_f2g, und_kpts with pt / octave, scaleFactors, imageParams with fx() fy() cx() cy().
#pragma once
#include <array>
#include <cstdint>
#include <vector>

struct ToyPoint2f { float x, y; };
struct ToyKeyPoint { ToyPoint2f pt; int octave; };   // the fields of cv::KeyPoint that are read
struct ToyImageParams {
    float fx_, fy_, cx_, cy_;
    float fx() const { return fx_; }
    float fy() const { return fy_; }
    float cx() const { return cx_; }
    float cy() const { return cy_; }
};
struct ToyViewFrame {
    uint32_t idx = 0;
    std::array<float, 16> pose_f2g{};   // row-major 4x4, global -> camera
    std::vector<ToyKeyPoint> und_kpts;
    std::vector<float> scaleFactors;
    ToyImageParams imageParams{517.3f, 516.5f, 318.6f, 255.3f};
};
