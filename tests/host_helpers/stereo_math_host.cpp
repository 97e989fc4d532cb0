// Host build of csrc/stereo_math.hpp with a main of its own: reads scenes dumped by tests/test_stereo_host.py, computes depth and match of
// every left keypoint (and the RGB-D gather) with the shared header, writes them back.  The test compares them with the numpy oracle bit for
// bit; built with -fsanitize=address,undefined the same program is the sanitizer run of this arithmetic (no GPU, no Python):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all stereo_math_host.cpp -o stereo_math_host
//   ./stereo_math_host scenes.bin results.bin
// File format (little endian): int32 n_scenes, then per scene
//   int32 kind (0 stereo, 1 rgbd), rows, cols, n_left, n_right; float bl, fx, mdd
//   stereo: L (rows*cols u8), R, left keypoints (n_left * 28 bytes), left descriptors (n_left * 32), right keypoints, right descriptors
//   rgbd:   D (rows*cols u16), keypoints (n_left * 28); mdd holds the depth scale
// Output per scene: n_left floats (depth), n_left int32 (match; rgbd: zeros).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ucoslam-cv3_amd/csrc/stereo_math.hpp"

struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };
static_assert(sizeof(KeyPoint) == 28, "cv::KeyPoint");

template <typename T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s scenes.bin results.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    const int n_scenes = take<int32_t>(in, 1)[0];
    for (int s = 0; s < n_scenes; s++) {
        const std::vector<int32_t> hd = take<int32_t>(in, 5);
        const std::vector<float> pf = take<float>(in, 3);
        const int kind = hd[0], rows = hd[1], cols = hd[2], nl = hd[3], nr = hd[4];
        std::vector<float> depth(nl, 0.f);
        std::vector<int32_t> match(nl, 0);
        if (kind == 1) {
            const std::vector<uint16_t> D = take<uint16_t>(in, (size_t)rows * cols);
            const std::vector<KeyPoint> k = take<KeyPoint>(in, nl);
            for (int i = 0; i < nl; i++) depth[i] = stm::rgbd_depth(D.data(), cols, cols, rows, k[i].x, k[i].y, pf[2]);
        } else {
            const std::vector<uint8_t> L = take<uint8_t>(in, (size_t)rows * cols), R = take<uint8_t>(in, (size_t)rows * cols);
            const std::vector<KeyPoint> lk = take<KeyPoint>(in, nl);
            const std::vector<uint8_t> ld = take<uint8_t>(in, (size_t)nl * 32);
            const std::vector<KeyPoint> rk = take<KeyPoint>(in, nr);
            const std::vector<uint8_t> rd = take<uint8_t>(in, (size_t)nr * 32);
            std::vector<std::vector<int>> bucket(rows);
            for (int j = 0; j < nr; j++) { const int r = stm::right_row(rk[j].y, rows); if (r >= 0) bucket[r].push_back(j); }
            const float blfx = pf[0] * pf[1];
            for (int i = 0; i < nl; i++) {
                uint64_t key = stm::kNoKey;
                const int r = stm::left_row(lk[i].y, rows);
                if (r >= 0) {
                    uint32_t a[8];
                    memcpy(a, ld.data() + (size_t)i * 32, 32);
                    for (int j : bucket[r]) {
                        if (!stm::candidate_ok(rk[j].x, rk[j].octave, lk[i].x, lk[i].octave)) continue;
                        uint32_t b[8];
                        memcpy(b, rd.data() + (size_t)j * 32, 32);
                        const int d = stm::hamming256(a, b);
                        if (stm::distance_ok(d, pf[2])) key = std::min(key, stm::match_key(d, j));
                    }
                }
                const int j = key == stm::kNoKey ? -1 : (int)(uint32_t)key;
                match[i] = j;
                if (j >= 0) depth[i] = stm::refine_serial(L.data(), cols, R.data(), cols, cols, rows, lk[i].x, lk[i].y, rk[j].x, rk[j].y, blfx);
            }
        }
        if (nl) {
            fwrite(depth.data(), 4, nl, out);
            fwrite(match.data(), 4, nl, out);
        }
    }
    fclose(in);
    fclose(out);
    return 0;
}
