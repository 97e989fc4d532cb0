// Stereo / RGB-D frames: per-keypoint depth on the device — FrameExtractor::processStereo / process_rgbd
// (src/utils/frameextractor.cpp from :1419) behind the extractor.  The arithmetic is stereo_math.hpp (shared with the host form);
// this file holds the lane mappings, the launches and the C entry points on caller-supplied data.
//
//   st_bucket_kernel   one workgroup: CSR index of the right keypoints by rounded row (counters in LDS, block scan, fill)
//   st_match_kernel    8 lanes per left keypoint walk its row's candidates; minimum of (distance, j) keys
//   st_refine_kernel   16 lanes per match: one SAD offset per lane, first-minimum walk, parabola, depth
//   st_rgbd_kernel     one lane per keypoint: the depth image gather
//
// A row's fill order comes from LDS atomics and is not fixed; nothing downstream depends on it, because the match takes the minimum
// of (distance, j) keys, which is the reference's "first smallest in ascending j".
#include "stereo.hpp"
#include "stereo_math.hpp"
#include <algorithm>
#include <vector>

namespace {

constexpr int kBucketThreads = 1024;
constexpr int kMatchLanes = 8;
constexpr int kRefineLanes = 16;

__device__ __forceinline__ int dev_count(int n, const int* d_n) {
    if (!d_n) return n;
    const int v = *d_n;
    return v < 0 ? 0 : (v < n ? v : n);
}

__global__ __launch_bounds__(kBucketThreads) void st_bucket_kernel(const uh_keypoint* __restrict__ r_kps, int n_right, const int* __restrict__ d_n_right,
                                                                   int rows, int* __restrict__ row_ptr, int* __restrict__ row_idx) {
    extern __shared__ int st_lds[];
    int* cnt = st_lds;                 // [rows]: counters, then fill cursors
    int* part = st_lds + rows;         // [kBucketThreads]: the threads' chunk sums
    const int tid = threadIdx.x;
    const int n = dev_count(n_right, d_n_right);
    for (int r = tid; r < rows; r += kBucketThreads) cnt[r] = 0;
    __syncthreads();
    for (int j = tid; j < n; j += kBucketThreads) {
        const int r = stm::right_row(r_kps[j].y, rows);
        if (r >= 0) atomicAdd(&cnt[r], 1);
    }
    __syncthreads();
    const int chunk = (rows + kBucketThreads - 1) / kBucketThreads;
    const int rb = min(tid * chunk, rows), re = min(rb + chunk, rows);
    int sum = 0;
    for (int r = rb; r < re; r++) sum += cnt[r];
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kBucketThreads; off <<= 1) {   // inclusive scan of the chunk sums
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int r = rb; r < re; r++) {
        const int c = cnt[r];
        row_ptr[r] = run;
        cnt[r] = run;
        run += c;
    }
    if (tid == kBucketThreads - 1) row_ptr[rows] = part[tid];
    __syncthreads();
    for (int j = tid; j < n; j += kBucketThreads) {
        const int r = stm::right_row(r_kps[j].y, rows);
        if (r >= 0) row_idx[atomicAdd(&cnt[r], 1)] = j;   // (< row_ptr[rows] <= n)
    }
}

__global__ __launch_bounds__(256) void st_match_kernel(const uh::StereoLaunch a) {
    const int g = (int)((blockIdx.x * 256u + threadIdx.x) / kMatchLanes), sub = threadIdx.x & (kMatchLanes - 1);
    const int n = dev_count(a.n_left, a.d_n_left);
    uint64_t key = stm::kNoKey;
    if (g < n) {
        const float lux = a.l_xy[(size_t)g * a.l_xy_stride], luy = a.l_xy[(size_t)g * a.l_xy_stride + 1];
        const int loct = a.l_oct[(size_t)g * a.l_oct_stride];
        const int r = stm::left_row(luy, a.rows);
        if (r >= 0) {
            const int kb = a.row_ptr[r], ke = a.row_ptr[r + 1];
            if (kb + sub < ke) {
                const uint4* ld = reinterpret_cast<const uint4*>(a.l_desc + (size_t)g * 32);
                const uint4 l0 = ld[0], l1 = ld[1];
                const uint32_t lw[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
                for (int k = kb + sub; k < ke; k += kMatchLanes) {
                    const int j = a.row_idx[k];
                    const uh_keypoint& rk = a.r_kps[j];
                    if (!stm::candidate_ok(rk.x, rk.octave, lux, loct)) continue;
                    const uint4* rd = reinterpret_cast<const uint4*>(a.r_desc + (size_t)j * 32);
                    const uint4 r0 = rd[0], r1 = rd[1];
                    const uint32_t rw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
                    const int d = stm::hamming256(lw, rw);
                    if (stm::distance_ok(d, a.max_desc_dist)) {
                        const uint64_t kk = stm::match_key(d, j);
                        key = kk < key ? kk : key;
                    }
                }
            }
        }
    }
    for (int m = kMatchLanes / 2; m >= 1; m >>= 1) {   // (every lane of the wave gets here)
        const uint64_t other = __shfl_xor((unsigned long long)key, m, kMatchLanes);
        key = other < key ? other : key;
    }
    if (g < n && sub == 0) a.match[g] = key == stm::kNoKey ? -1 : (int)(uint32_t)key;
}

__global__ __launch_bounds__(256) void st_refine_kernel(const uh::StereoLaunch a) {
    const int g = (int)((blockIdx.x * 256u + threadIdx.x) / kRefineLanes), o = threadIdx.x & (kRefineLanes - 1);
    const int n = dev_count(a.n_left, a.d_n_left);
    const int n_right = dev_count(a.n_right, a.d_n_right);
    bool valid = false;
    float lux = 0.f, rpx = 0.f;
    int lx = 0, ly = 0, rx = 0, ry = 0, lo = 0, hi = -1;
    if (g < n) {
        const int j = a.match[g];
        if (j >= 0 && j < n_right) {
            lux = a.l_xy[(size_t)g * a.l_xy_stride];
            const float luy = a.l_xy[(size_t)g * a.l_xy_stride + 1];
            rpx = a.r_kps[j].x;
            const float rpy = a.r_kps[j].y;
            lx = stm::round_away(lux); ly = stm::round_away(luy);
            rx = stm::round_away(rpx); ry = stm::round_away(rpy);
            valid = stm::centre_ok(lx, a.cols) && stm::centre_ok(ly, a.rows) && stm::centre_ok(rx, a.cols) && stm::centre_ok(ry, a.rows);
            if (valid) stm::offset_range(rx, a.cols, lo, hi);
        }
    }
    int cost = 0;
    const int off = o - stm::kMaxOff;
    if (valid && off >= lo && off <= hi) cost = stm::sad6(a.left, a.left_stride, lx, ly, a.right, a.right_stride, rx + off, ry);
    int best = 0, b = -1;
#pragma unroll
    for (int k = 0; k < stm::kNumOff; k++) {   // (every lane of the wave takes part in the shuffles)
        const int ck = __shfl(cost, k, kRefineLanes);
        if (k - stm::kMaxOff >= lo && k - stm::kMaxOff <= hi) stm::take_min(ck, k, best, b);
    }
    const int c0 = __shfl(cost, b < 1 ? 0 : b - 1, kRefineLanes);
    const int c2 = __shfl(cost, b + 1 > stm::kNumOff - 1 ? stm::kNumOff - 1 : (b < 0 ? 0 : b + 1), kRefineLanes);
    if (g < n && o == 0) {
        float dep = 0.f;
        if (valid && b > lo + stm::kMaxOff && b < hi + stm::kMaxOff) dep = stm::depth_from_costs(c0, best, c2, b, rpx, lux, a.blfx);
        a.depth[g] = dep;
    }
}

__global__ __launch_bounds__(256) void st_rgbd_kernel(const uh_keypoint* __restrict__ kps, int n_cap, const int* __restrict__ d_n, const uint16_t* __restrict__ D,
                                                      size_t stride_px, int cols, int rows, float scale, float* __restrict__ depth) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dev_count(n_cap, d_n)) return;
    depth[i] = stm::rgbd_depth(D, stride_px, cols, rows, kps[i].x, kps[i].y, scale);
}

int check_stereo_args(const char* who, const uh_stereo_args* a, const void* depth_out) {
    UH_REQUIRE(a, "%s: NULL arguments", who);
    UH_REQUIRE(a->cols >= 1 && a->rows >= 1 && a->cols <= (1 << 20) && a->rows <= uh::kStereoMaxRows, "%s: image %d x %d outside [1, %d] x [1, %d]", who,
               a->cols, a->rows, 1 << 20, uh::kStereoMaxRows);
    UH_REQUIRE(a->right_cols == a->cols && a->right_rows == a->rows, "%s: left image %d x %d but right image %d x %d", who, a->cols, a->rows,
               a->right_cols, a->right_rows);
    UH_REQUIRE(a->left && a->right && a->left_stride >= (size_t)a->cols && a->right_stride >= (size_t)a->cols, "%s: NULL image or stride < cols", who);
    UH_REQUIRE(a->n_left >= 0 && a->n_right >= 0 && a->n_left <= (1 << 24) && a->n_right <= (1 << 24), "%s: keypoint counts %d / %d", who, a->n_left, a->n_right);
    UH_REQUIRE(a->n_left == 0 || (a->left_und_kpts && a->left_desc && depth_out), "%s: NULL left keypoints / descriptors / depth", who);
    UH_REQUIRE(a->n_right == 0 || (a->right_kpts && a->right_desc), "%s: NULL right keypoints / descriptors", who);
    UH_REQUIRE(a->bl > 0.f, "%s: baseline bl = %g must be > 0", who, (double)a->bl);
    return UH_OK;
}

}  // namespace

namespace uh {

int stereo_launch(uh_ctx* ctx, const StereoLaunch& a) {
    UH_REQUIRE(a.rows >= 1 && a.rows <= kStereoMaxRows && a.cols >= 1, "stereo: image %d x %d (at most %d rows)", a.cols, a.rows, kStereoMaxRows);
    UH_REQUIRE(a.n_left >= 0 && a.n_right >= 0, "stereo: negative keypoint count");
    UH_REQUIRE(((reinterpret_cast<uintptr_t>(a.l_desc) | reinterpret_cast<uintptr_t>(a.r_desc)) & 15) == 0, "stereo: descriptors must be 16-byte aligned");
    if (a.n_left == 0) return UH_OK;
    UH_LAUNCH(ctx, st_bucket_kernel, dim3(1), dim3(kBucketThreads), (size_t)(a.rows + kBucketThreads) * sizeof(int), a.r_kps, a.n_right, a.d_n_right, a.rows,
              a.row_ptr, a.row_idx);
    UH_LAUNCH(ctx, st_match_kernel, dim3(uh_div_up(a.n_left, 256 / kMatchLanes)), dim3(256), 0, a);
    UH_LAUNCH(ctx, st_refine_kernel, dim3(uh_div_up(a.n_left, 256 / kRefineLanes)), dim3(256), 0, a);
    UH_HIP_CHECK(hipGetLastError());
    return UH_OK;
}

int rgbd_launch(uh_ctx* ctx, const uh_keypoint* kps, int n, const int* d_n, const uint16_t* depth_img, size_t stride_px, int cols, int rows, float scale,
                float* depth) {
    if (n <= 0) return UH_OK;
    UH_LAUNCH(ctx, st_rgbd_kernel, dim3(uh_div_up(n, 256)), dim3(256), 0, kps, n, d_n, depth_img, stride_px, cols, rows, scale, depth);
    UH_HIP_CHECK(hipGetLastError());
    return UH_OK;
}

}  // namespace uh

extern "C" {

int uh_stereo_depth_dev(uh_ctx* ctx, const uh_stereo_args* a, float* d_depth, int32_t* d_match) {
    UH_REQUIRE(ctx, "uh_stereo_depth_dev: NULL context");
    int rc = check_stereo_args("uh_stereo_depth_dev", a, d_depth);
    if (rc) return rc;
    if (a->n_left == 0) return UH_OK;
    UH_HIP_CHECK(hipSetDevice(ctx->device));
    uh::Layout lay;
    const size_t o_ptr = lay.take<int>((size_t)a->rows + 1), o_idx = lay.take<int>(std::max(a->n_right, 1)), o_match = lay.take<int>(a->n_left);
    if ((rc = ctx->stereo_ws.reserve(lay.off))) return rc;
    char* ws = ctx->stereo_ws.as<char>();
    uh::StereoLaunch s{};
    s.left = a->left; s.left_stride = a->left_stride; s.right = a->right; s.right_stride = a->right_stride; s.cols = a->cols; s.rows = a->rows;
    s.l_xy = &a->left_und_kpts->x; s.l_xy_stride = sizeof(uh_keypoint) / 4; s.l_oct = &a->left_und_kpts->octave; s.l_oct_stride = sizeof(uh_keypoint) / 4;
    s.l_desc = a->left_desc; s.n_left = a->n_left; s.r_kps = a->right_kpts; s.r_desc = a->right_desc; s.n_right = a->n_right;
    s.blfx = a->bl * a->fx; s.max_desc_dist = a->max_desc_dist;
    s.depth = d_depth; s.match = d_match ? d_match : reinterpret_cast<int*>(ws + o_match);
    s.row_ptr = reinterpret_cast<int*>(ws + o_ptr); s.row_idx = reinterpret_cast<int*>(ws + o_idx);
    return uh::stereo_launch(ctx, s);
}

int uh_stereo_depth(uh_ctx* ctx, const uh_stereo_args* a, float* depth_out, int32_t* match_out) {
    UH_REQUIRE(ctx, "uh_stereo_depth: NULL context");
    int rc = check_stereo_args("uh_stereo_depth", a, depth_out);
    if (rc) return rc;
    if (a->n_left == 0) return UH_OK;
    UH_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t img = (size_t)a->cols * a->rows;
    uh::Layout lay;
    const size_t o_l = lay.take<uint8_t>(img), o_r = lay.take<uint8_t>(img), o_lk = lay.take<uh_keypoint>(a->n_left), o_ld = lay.take<uint8_t>((size_t)a->n_left * 32),
                 o_rk = lay.take<uh_keypoint>(std::max(a->n_right, 1)), o_rd = lay.take<uint8_t>((size_t)std::max(a->n_right, 1) * 32),
                 o_ptr = lay.take<int>((size_t)a->rows + 1), o_idx = lay.take<int>(std::max(a->n_right, 1)), o_match = lay.take<int>(a->n_left),
                 o_depth = lay.take<float>(a->n_left);
    if ((rc = ctx->stereo_ws.reserve(lay.off))) return rc;
    char* ws = ctx->stereo_ws.as<char>();
    UH_HIP_CHECK(hipMemcpy2DAsync(ws + o_l, a->cols, a->left, a->left_stride, a->cols, a->rows, hipMemcpyHostToDevice, st));
    UH_HIP_CHECK(hipMemcpy2DAsync(ws + o_r, a->cols, a->right, a->right_stride, a->cols, a->rows, hipMemcpyHostToDevice, st));
    UH_HIP_CHECK(hipMemcpyAsync(ws + o_lk, a->left_und_kpts, (size_t)a->n_left * sizeof(uh_keypoint), hipMemcpyHostToDevice, st));
    UH_HIP_CHECK(hipMemcpyAsync(ws + o_ld, a->left_desc, (size_t)a->n_left * 32, hipMemcpyHostToDevice, st));
    if (a->n_right > 0) {
        UH_HIP_CHECK(hipMemcpyAsync(ws + o_rk, a->right_kpts, (size_t)a->n_right * sizeof(uh_keypoint), hipMemcpyHostToDevice, st));
        UH_HIP_CHECK(hipMemcpyAsync(ws + o_rd, a->right_desc, (size_t)a->n_right * 32, hipMemcpyHostToDevice, st));
    }
    const uh_keypoint* lk = reinterpret_cast<const uh_keypoint*>(ws + o_lk);
    uh::StereoLaunch s{};
    s.left = reinterpret_cast<const uint8_t*>(ws + o_l); s.left_stride = a->cols; s.right = reinterpret_cast<const uint8_t*>(ws + o_r); s.right_stride = a->cols;
    s.cols = a->cols; s.rows = a->rows;
    s.l_xy = &lk->x; s.l_xy_stride = sizeof(uh_keypoint) / 4; s.l_oct = &lk->octave; s.l_oct_stride = sizeof(uh_keypoint) / 4;
    s.l_desc = reinterpret_cast<const uint8_t*>(ws + o_ld); s.n_left = a->n_left;
    s.r_kps = reinterpret_cast<const uh_keypoint*>(ws + o_rk); s.r_desc = reinterpret_cast<const uint8_t*>(ws + o_rd); s.n_right = a->n_right;
    s.blfx = a->bl * a->fx; s.max_desc_dist = a->max_desc_dist;
    s.depth = reinterpret_cast<float*>(ws + o_depth); s.match = reinterpret_cast<int*>(ws + o_match);
    s.row_ptr = reinterpret_cast<int*>(ws + o_ptr); s.row_idx = reinterpret_cast<int*>(ws + o_idx);
    if ((rc = uh::stereo_launch(ctx, s))) return rc;
    UH_HIP_CHECK(hipMemcpyAsync(depth_out, s.depth, (size_t)a->n_left * 4, hipMemcpyDeviceToHost, st));
    if (match_out) UH_HIP_CHECK(hipMemcpyAsync(match_out, s.match, (size_t)a->n_left * 4, hipMemcpyDeviceToHost, st));
    UH_HIP_CHECK(hipStreamSynchronize(st));
    return UH_OK;
}

int uh_stereo_depth_host(const uh_stereo_args* a, float* depth_out, int32_t* match_out) {
    int rc = check_stereo_args("uh_stereo_depth_host", a, depth_out);
    if (rc) return rc;
    const int rows = a->rows, nr = a->n_right;
    std::vector<int> row_ptr((size_t)rows + 1, 0), row_idx((size_t)std::max(nr, 1));
    for (int j = 0; j < nr; j++) { const int r = stm::right_row(a->right_kpts[j].y, rows); if (r >= 0) row_ptr[(size_t)r + 1]++; }
    for (int r = 0; r < rows; r++) row_ptr[(size_t)r + 1] += row_ptr[r];
    {
        std::vector<int> cur(row_ptr.begin(), row_ptr.end() - 1);
        for (int j = 0; j < nr; j++) { const int r = stm::right_row(a->right_kpts[j].y, rows); if (r >= 0) row_idx[(size_t)cur[r]++] = j; }
    }
    const float blfx = a->bl * a->fx;
    for (int i = 0; i < a->n_left; i++) {
        const uh_keypoint& lk = a->left_und_kpts[i];
        uint64_t key = stm::kNoKey;
        const int r = stm::left_row(lk.y, rows);
        if (r >= 0) {
            uint32_t lw[8];
            std::memcpy(lw, a->left_desc + (size_t)i * 32, 32);
            for (int k = row_ptr[r]; k < row_ptr[(size_t)r + 1]; k++) {
                const int j = row_idx[k];
                const uh_keypoint& rk = a->right_kpts[j];
                if (!stm::candidate_ok(rk.x, rk.octave, lk.x, lk.octave)) continue;
                uint32_t rw[8];
                std::memcpy(rw, a->right_desc + (size_t)j * 32, 32);
                const int d = stm::hamming256(lw, rw);
                if (stm::distance_ok(d, a->max_desc_dist)) key = std::min(key, stm::match_key(d, j));
            }
        }
        const int j = key == stm::kNoKey ? -1 : (int)(uint32_t)key;
        if (match_out) match_out[i] = j;
        depth_out[i] = j < 0 ? 0.f
                             : stm::refine_serial(a->left, a->left_stride, a->right, a->right_stride, a->cols, rows, lk.x, lk.y, a->right_kpts[j].x,
                                                  a->right_kpts[j].y, blfx);
    }
    return UH_OK;
}

static int check_rgbd_args(const char* who, const uh_keypoint* kpts, int32_t n, const uint16_t* D, int32_t cols, int32_t rows, size_t stride, const float* out) {
    UH_REQUIRE(n >= 0 && n <= (1 << 24) && (n == 0 || (kpts && out)), "%s: %d keypoints / NULL buffer", who, n);
    UH_REQUIRE(D && cols >= 1 && rows >= 1 && cols <= (1 << 20) && rows <= (1 << 20), "%s: NULL depth image or bad size %d x %d", who, cols, rows);
    UH_REQUIRE(stride >= (size_t)cols * 2 && (stride & 1) == 0, "%s: depth stride %zu (bytes) below the row or odd", who, stride);
    return UH_OK;
}

int uh_rgbd_depth_host(const uh_keypoint* kpts, int32_t n, const uint16_t* D, int32_t cols, int32_t rows, size_t stride, float scale, float* out) {
    int rc = check_rgbd_args("uh_rgbd_depth_host", kpts, n, D, cols, rows, stride, out);
    if (rc) return rc;
    for (int i = 0; i < n; i++) out[i] = stm::rgbd_depth(D, stride / 2, cols, rows, kpts[i].x, kpts[i].y, scale);
    return UH_OK;
}

int uh_rgbd_depth(uh_ctx* ctx, const uh_keypoint* kpts, int32_t n, const uint16_t* D, int32_t cols, int32_t rows, size_t stride, float scale, float* out) {
    UH_REQUIRE(ctx, "uh_rgbd_depth: NULL context");
    int rc = check_rgbd_args("uh_rgbd_depth", kpts, n, D, cols, rows, stride, out);
    if (rc) return rc;
    if (n == 0) return UH_OK;
    UH_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uh::Layout lay;
    const size_t o_img = lay.take<uint16_t>((size_t)cols * rows), o_k = lay.take<uh_keypoint>(n), o_d = lay.take<float>(n);
    if ((rc = ctx->stereo_ws.reserve(lay.off))) return rc;
    char* ws = ctx->stereo_ws.as<char>();
    UH_HIP_CHECK(hipMemcpy2DAsync(ws + o_img, (size_t)cols * 2, D, stride, (size_t)cols * 2, rows, hipMemcpyHostToDevice, st));
    UH_HIP_CHECK(hipMemcpyAsync(ws + o_k, kpts, (size_t)n * sizeof(uh_keypoint), hipMemcpyHostToDevice, st));
    if ((rc = uh::rgbd_launch(ctx, reinterpret_cast<const uh_keypoint*>(ws + o_k), n, nullptr, reinterpret_cast<const uint16_t*>(ws + o_img), cols, cols, rows, scale,
                              reinterpret_cast<float*>(ws + o_d))))
        return rc;
    UH_HIP_CHECK(hipMemcpyAsync(out, ws + o_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    UH_HIP_CHECK(hipStreamSynchronize(st));
    return UH_OK;
}

}  // extern "C"
