// Host build of csrc/fuse_math.hpp and csrc/fuse_host.hpp alone (g++, no HIP, no library): tests/test_fuse_host.py loads it and hands it the
// kd-tree the ORACLE built (oracle_kd_export), so that the arithmetic, the walk and the Hamming rule are compared with the oracle without
// any other code of the library in between.  Built with -fsanitize=address,undefined and a main of its own it is also the sanitizer run
// of that code.
#include <cmath>
#include <cstdint>

#include "../../ucoslam-cv3_amd/csrc/fuse_host.hpp"

extern "C" {

// nodes24: {float divlow, divhigh; int32 left, right, leaf_begin; int16 leaf_count, col}.  cam4: fx fy cx cy; bounds4: min_x min_y max_x max_y.
int fu_host_search(const void* nodes24, int n_nodes, const uint32_t* leaf_idx, const double* box4, const float* xy, const int32_t* octave, const uint8_t* kp_desc, int n_kpts,
                   const float* scale, int n_levels, const float* cam4, const int32_t* bounds4, const float* pose16, const float* predict_sf, int predict_levels, int n,
                   const float* pos3d, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc, const uint8_t* skip, float th, float widen,
                   float max_desc_dist, int32_t* best_kp, float* best_dist, uint8_t* status) {
    if (predict_levels < 2 || predict_levels > n_levels || n_levels > 16) return -1;
    uh_fusem::View v;
    for (int i = 0; i < 12; i++) v.T[i] = pose16[i];
    uh_fusem::camera_center(pose16, v.cc);
    v.fx = cam4[0]; v.fy = cam4[1]; v.cx = cam4[2]; v.cy = cam4[3];
    v.min_x = (float)bounds4[0]; v.min_y = (float)bounds4[1]; v.max_x = (float)bounds4[2]; v.max_y = (float)bounds4[3];
    v.log_scale = std::log(predict_sf[1]);
    v.predict_levels = predict_levels;
    v.th = th == 0 ? 2.5f : th; v.widen = widen;
    float sc[16] = {0};
    for (int i = 0; i < n_levels; i++) sc[i] = scale[i];
    const uh_fusem::HostTree t{static_cast<const uh_fusem::HostNode*>(nodes24), n_nodes, leaf_idx, box4, xy, octave, kp_desc, n_kpts};
    const uh_fusem::HostPoints p{n, pos3d, normal, min_dist, max_dist, desc};
    uh_fusem::search_host(v, sc, t, p, skip, max_desc_dist, best_kp, best_dist, status);
    return 0;
}

}  // extern "C"

#ifdef FUSE_HOST_MAIN
// g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -DFUSE_HOST_MAIN fuse_host.cpp -o fuse_host && ./fuse_host
// A hand-made tree (root with two leaves of three keypoints each), four points: found, behind the camera, too far, skipped.
#include <cstdio>
int main() {
    const uh_fusem::HostNode nodes[3] = {{110.f, 200.f, 1, 2, 0, 0, 0}, {0, 0, -1, -1, 0, 3, 0}, {0, 0, -1, -1, 3, 3, 0}};
    const uint32_t leaf[6] = {0, 1, 2, 3, 4, 5};
    const double box[4] = {100, 210, 100, 110};
    const float xy[12] = {100, 100, 105, 102, 110, 104, 200, 100, 205, 105, 210, 110};
    const int32_t oct[6] = {0, 1, 2, 0, 1, 2};
    uint8_t kd[6 * 32];
    for (int i = 0; i < 6 * 32; i++) kd[i] = (uint8_t)(i * 37 + (i >> 5));
    const float scale[4] = {1.f, 1.2f, 1.44f, 1.728f}, cam[4] = {500, 500, 160, 120};
    const int32_t bounds[4] = {0, 0, 320, 240};
    const float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float z = 4.f;
    const float pos[12] = {(105 - 160) / 500.f * z, (102 - 120) / 500.f * z, z, 0, 0, -1, 0, 0, 40, (205 - 160) / 500.f * z, (105 - 120) / 500.f * z, z};
    float nrm[12];
    for (int i = 0; i < 4; i++) {
        const float* p = pos + 3 * i;
        const float l = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        for (int c = 0; c < 3; c++) nrm[3 * i + c] = -p[c] / l;
    }
    const float mind[4] = {2, 2, 2, 2}, maxd[4] = {5, 5, 5, 5};
    uint8_t desc[4 * 32];
    for (int i = 0; i < 4; i++) for (int b = 0; b < 32; b++) desc[32 * i + b] = kd[32 * (i == 3 ? 4 : 1) + b];
    const uint8_t skip[4] = {0, 0, 0, 1};
    int32_t bk[4]; float bd[4]; uint8_t st[4];
    if (fu_host_search(nodes, 3, leaf, box, xy, oct, kd, 6, scale, 4, cam, bounds, pose, scale, 4, 4, pos, nrm, mind, maxd, desc, skip, 0.f, 1.4f, 60.f, bk, bd, st)) return 1;
    for (int i = 0; i < 4; i++) printf("%d %d %g\n", st[i], bk[i], bd[i]);
    return (st[0] == 0 && bk[0] == 1 && bd[0] == 0.f && st[1] == 2 && st[2] == 3 && st[3] == 1) ? 0 : 1;
}
#endif
