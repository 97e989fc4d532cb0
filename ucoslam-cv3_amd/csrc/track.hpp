// uh_track_pose: the tracker's pose estimation for one frame as ONE host call — what System does between FrameExtractor::process and the
// keyframe decision (src/utils/system.cpp, raw line numbers of the statement starts, read after preprocessing):
//   :6559-6565   projection search against the previous frame                                 (uh_projmatch_match_prev)
//   :6595-6646   with MORE than min_inliers matches: PnPSolver::solvePnp over them            (uh_pnp_solve; pnpsolver.cpp:116-409, look-ups :199-232)
//                (fewer: the reference's FrameMatcher fallback :6664-6780 is the caller's; here it finds nothing, nInliers = 0)
//   :6813-6877   MORE than min_inliers inliers: keep the refined pose and EVERY first match, mark their points seen (:6842), search the
//                local map in a 4 px disc; else predicted pose, projDistThr, no first matches
//   :6897        Map::matchFrameToMapPoints without the points seen this frame (map.cpp:657-668)   (uh_projmatch_match)
//   :6913-6954   the first matches + the new ones, filter_ambiguous_query over the union, per-match look-ups, PnPSolver::solvePnp (uh_pnp_solve)
// Called one after the other through the C ABI the four operators cost four host round trips (launch latency + completion word + unpacking +
// the host's look-ups in between: ~55 of the frame's ~430 us were no kernel's).  Here the host stages both candidate sets, enqueues
// SEVEN launches on the context stream and waits once; what the host did between the calls runs on the device:
//   projmatch_kernel<prev>  ->  track_select_kernel (matches in item order, filter_ambiguous_query, look-ups for the solve)
//   -> pnp_solve_kernel (match count from device memory; its last thread also takes the decision: pose / radius of the map search)
//   -> projmatch_kernel<map> (pose and radius read from device memory)  ->  track_select_kernel (the seen points' hits dropped, its own
//   filter, the union with every first match when tracked, filter, look-ups)  ->  pnp_solve_kernel  ->  track_publish_kernel (everything the
//   sequence of calls returns).
// The look-ups gather from HBM only: the searches leave every candidate's position and its {id, map row, weight} record there again
// (PmPoints::pos_out / aux_out: one more 16-byte read per candidate inside launches that wait on such reads anyway; gathering from pinned
// memory in the select launches was one host-link request per match — 31 us for the second one — and staging the tables there 5 us).
// Same results as the four calls, bit for bit (tests/test_track.py, tests/test_cpp_host.py), and as the CPU oracle of system.cpp's control
// flow (oracle/track_oracle.cpp, tests/test_track_oracle_gpu.py): the same kernels do the searching and the solving; the list logic is
// integer work (stable minimum per keypoint = uh_filter_ambiguous, matcher.hip keep_best_per_key).
// This file is included at the end of projmatch.hip (it uses that unit's internals).
#pragma once

namespace uh {
int pnp_enqueue_dev(uh_pnp* p, const float* d_pose, const float* d_intr4, int n_cap, const int* d_n, const PnpMatches& m, const uh_pnp_markers* d_mk, float* d_pose_out,
                    unsigned char* d_bad_out, int* d_result5, const PnpDecide* dec);
int pnp_reserve(uh_pnp* p, int n_cap, bool stereo);
uh_ctx* pnp_ctx(uh_pnp* p);
}

namespace {

constexpr int kTrkThreads = 1024;
struct TrkElem { int query; unsigned id; float dist; int src; };   // src: bit 30 = candidate of the map search, low bits = its index in its candidate set

// header of the device block (ints)
enum : int { kTrkN1 = 0, kTrkN2 = 1, kTrkNA = 2, kTrkTracked = 3, kTrkRes1 = 4 /* 5 ints */, kTrkRes2 = 9 /* 5 ints */, kTrkHdrInts = 16 };

struct TrkSelect {
    // the search whose results become a list (candidate order)
    int nB; const int* bk; const float* bd; const uint4* aux; int map_kind;   // aux: {id, map row, weight} per candidate (HBM, left by the search)
    // second form only: the list carried over from the first search (all of it enters the union when the frame counts as tracked)
    const uh_dmatch* carry; const int* carry_src; int carry_cap;
    // one byte per map row: 1 = the point was matched by the first search of a tracked frame (lastFIdxSeen, system.cpp:6842); the first
    // form clears it, the second sets it from the carried list and drops those rows' hits before its filter (map.cpp:657-668)
    unsigned char* seen; int n_map_rows;
    int* hdr;                       // counts in / out (see the enum)
    int fresh_n_slot, final_n_slot; // hdr slots of the fresh list's and the final list's length (equal in the first form)
    uh_dmatch* fresh_out; int* fresh_src;   // the search's own matches (after filter_ambiguous_query)
    uh_dmatch* final_out;                   // second form: the union after its filter (NULL in the first form)
    int* final_src;                         // scratch: source of each element of the final list
    // look-ups for the solve over the final list
    const float4* pos_prev; const float4* pos_map;   // HBM: the candidates' positions as the searches left them
    const uint4* aux_prev; const uint4* aux_map; int prefer_map_row;
    const float4* kp_xyo; const float* inv_sigma_lv; int n_levels;
    float* p3d; float* kp; float* isg; float* wgt;
    int n_kpts;
    TrkElem* scratch_a; TrkElem* scratch_b;
    long long* clk;   // UH_TRK_CLK: 8 wall-clock stamps (10 ns) of thread 0
    // uh_track_pose_stereo: the frame's per-keypoint depth (dep_src: pinned, copied once into dep_kp in HBM by the first launch; NULL in the
    // second) and the per-match depth of the solve (dep)
    const float* dep_src; float* dep_kp; float* dep;
};

// Exclusive prefix over the workgroup's per-thread counts; returns the thread's offset and (total) the sum.  Two barriers.
__device__ __forceinline__ int trk_block_offset(int count, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = uh_kd::wave_incl_scan(count);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kTrkThreads / 64; w++) { const int v = s_wave[w]; base += w < wave ? v : 0; tot += v; }
    __syncthreads();
    total = tot;
    return base + inc - count;
}

constexpr int kTrkItems = 4;   // consecutive list positions per thread and pass: lists of up to 4096 elements take ONE scan (two barriers of sixteen waves) per step

// uh_filter_ambiguous(list, n, by query) on the device: the first strict minimum of the distance per keypoint stays, in list order
// (matcher.hip keep_best_per_key).  in / out may not alias.  Returns the new length (every thread).
__device__ int trk_filter(const TrkElem* in, int n, TrkElem* out, unsigned long long* s_best, int n_kpts, int* s_wave) {
    for (int k = threadIdx.x; k < n_kpts; k += kTrkThreads) s_best[k] = ~0ull;
    __syncthreads();
    for (int pos = threadIdx.x; pos < n; pos += kTrkThreads) {
        const TrkElem e = in[pos];
        atomicMin(&s_best[e.query], ((unsigned long long)__float_as_uint(e.dist) << 32) | (unsigned)pos);   // distances are >= 0: their bit patterns order like the values
    }
    __syncthreads();
    int kept = 0;
    for (int p0 = 0; p0 < n; p0 += kTrkThreads * kTrkItems) {
        TrkElem e[kTrkItems];
        int keep[kTrkItems], cnt = 0;
#pragma unroll
        for (int u = 0; u < kTrkItems; u++) {
            const int pos = p0 + (int)threadIdx.x * kTrkItems + u;
            keep[u] = 0;
            if (pos < n) { e[u] = in[pos]; keep[u] = (unsigned)(s_best[e[u].query] & 0xffffffffull) == (unsigned)pos ? 1 : 0; }
            cnt += keep[u];
        }
        int tot;
        int o = kept + trk_block_offset(cnt, s_wave, tot);
#pragma unroll
        for (int u = 0; u < kTrkItems; u++) if (keep[u]) out[o++] = e[u];
        kept += tot;
    }
    __syncthreads();
    return kept;
}

// LDS_LISTS: the two working lists live in dynamic LDS (cap elements each) instead of the HBM scratch (round trips through L2 between the steps)
template <bool LDS_LISTS>
__global__ __launch_bounds__(kTrkThreads) void track_select_kernel(TrkSelect a, int cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    __shared__ unsigned long long s_best[4096];
    __shared__ int s_wave[kTrkThreads / 64];
    __shared__ float s_isl[16];
    if (threadIdx.x < 16) s_isl[threadIdx.x] = (int)threadIdx.x < a.n_levels ? a.inv_sigma_lv[threadIdx.x] : 0.f;   // (pinned memory: read once, not once per match)
    TrkElem* const LA = LDS_LISTS ? reinterpret_cast<TrkElem*>(s_dyn) : a.scratch_a;
    TrkElem* const LB = LDS_LISTS ? reinterpret_cast<TrkElem*>(s_dyn) + cap : a.scratch_b;
    const int tid = threadIdx.x;
#define UH_TRK_STAMP(j) do { if (a.clk && tid == 0) a.clk[j] = wall_clock64(); } while (0)
    UH_TRK_STAMP(0);
    if (a.dep_src)   // (read by this launch's look-ups after the barriers below, and by the second select launch)
        for (int k = tid; k < a.n_kpts; k += kTrkThreads) a.dep_kp[k] = a.dep_src[k];
    if (!a.carry)     // (first form: the seen marks of the previous call go; the second launch reads them only after this one ended)
        for (int k = tid; k < a.n_map_rows; k += kTrkThreads) a.seen[k] = 0;
    const int tracked = a.carry ? a.hdr[kTrkTracked] : 0;
    const int nc = tracked ? min(a.hdr[kTrkN1], a.carry_cap) : 0;
    if (a.carry) {    // ---- tracked: every point of the first search is seen this frame (system.cpp:6842)
        for (int p = tid; p < nc; p += kTrkThreads) {
            const int row = (int)a.aux_prev[a.carry_src[p] & 0x3fffffff].y;
            if (row >= 0 && row < a.n_map_rows) a.seen[row] = 1;
        }
        __syncthreads();
    }
    UH_TRK_STAMP(1);
    // ---- the search's hits in candidate order (second form: without the seen points, whose search map.cpp:657-668 skips)
    int nF = 0;
    for (int p0 = 0; p0 < a.nB; p0 += kTrkThreads * kTrkItems) {
        int kpi[kTrkItems], cnt = 0;
        unsigned id[kTrkItems];
        float dist[kTrkItems];
#pragma unroll
        for (int u = 0; u < kTrkItems; u++) {
            const int i = p0 + tid * kTrkItems + u;
            kpi[u] = -1; id[u] = 0; dist[u] = 0.f;
            if (i < a.nB && !(a.carry && a.seen[i])) { kpi[u] = a.bk[i]; id[u] = a.aux[i].x; dist[u] = a.bd[i]; }
            cnt += kpi[u] >= 0 ? 1 : 0;
        }
        int tot;
        int o = nF + trk_block_offset(cnt, s_wave, tot);
#pragma unroll
        for (int u = 0; u < kTrkItems; u++) if (kpi[u] >= 0) LA[o++] = TrkElem{kpi[u], id[u], dist[u], (a.map_kind << 30) | (p0 + tid * kTrkItems + u)};
        nF += tot;
    }
    __syncthreads();
    UH_TRK_STAMP(2);
    // ---- filter_ambiguous_query of the search's own list (uh_projmatch_match / _match_prev end with it)
    const int n_fresh = trk_filter(LA, nF, LB, s_best, a.n_kpts, s_wave);
    UH_TRK_STAMP(3);
    for (int p = tid; p < n_fresh; p += kTrkThreads) {
        const TrkElem e = LB[p];
        a.fresh_out[p] = uh_dmatch{e.query, (int)e.id, -1, e.dist};
        a.fresh_src[p] = e.src;
    }
    const TrkElem* fin = LB;
    int n_fin = n_fresh;
    UH_TRK_STAMP(4);
    if (a.carry) {
        // ---- the union (system.cpp:6913): every match of the first search when the frame counts as tracked (the first solve only flagged
        // its outliers, pnpsolver.cpp:385-400), then the new matches; filter again
        for (int p = tid; p < nc; p += kTrkThreads) { const uh_dmatch m = a.carry[p]; LA[p] = TrkElem{m.queryIdx, (unsigned)m.trainIdx, m.distance, a.carry_src[p]}; }
        for (int p = tid; p < n_fresh; p += kTrkThreads) LA[nc + p] = LB[p];
        __syncthreads();
        const int nU = nc + n_fresh;
        // (LB is free again: its content lives in LA now)
        n_fin = trk_filter(LA, nU, LB, s_best, a.n_kpts, s_wave);
        for (int p = tid; p < n_fin; p += kTrkThreads) { const TrkElem e = LB[p]; a.final_out[p] = uh_dmatch{e.query, (int)e.id, -1, e.dist}; }
    }
    UH_TRK_STAMP(5);
    // ---- the solver's per-match look-ups (pnpsolver.cpp:199-232): the point's coordinates and weight, the keypoint, 1 / scaleFactor of its octave
    for (int p = tid; p < n_fin; p += kTrkThreads) {
        const TrkElem e = fin[p];
        const int is_map = (e.src >> 30) & 1, idx = e.src & 0x3fffffff;
        const uint4 ax = is_map ? a.aux_map[idx] : a.aux_prev[idx];
        const int row = a.prefer_map_row ? (int)ax.y : -1;   // (first solve: the candidate's own position)
        const float4 pos = row >= 0 ? a.pos_map[row] : a.pos_prev[idx];
        a.p3d[3 * p] = pos.x; a.p3d[3 * p + 1] = pos.y; a.p3d[3 * p + 2] = pos.z;
        a.wgt[p] = __uint_as_float(ax.z);   // (both solves: map_weight of the point's row, else prev_weight[i] or 1 — match_enqueue's record)
        if (a.dep) a.dep[p] = a.dep_kp[e.query];
        const float4 k = a.kp_xyo[e.query];
        a.kp[2 * p] = k.x; a.kp[2 * p + 1] = k.y;
        const int oct = (int)(__float_as_uint(k.z) & 15u);
        a.isg[p] = s_isl[oct < a.n_levels ? oct : 0];
        if (a.final_src) a.final_src[p] = e.src;
    }
    if (tid == 0) { a.hdr[a.fresh_n_slot] = n_fresh; a.hdr[a.final_n_slot] = n_fin; }
    UH_TRK_STAMP(6);
#undef UH_TRK_STAMP
}

struct TrkPublish {
    const int* hdr; const float* pose1; const float* pose2;
    const uh_dmatch* m1; const unsigned char* bad1; const uh_dmatch* m2; const uh_dmatch* ma; const unsigned char* bad2;
    int cap1, cap2, capa;
    // pinned twins
    int* h_hdr; float* h_pose1; float* h_pose2; uh_dmatch* h_m1; unsigned char* h_bad1; uh_dmatch* h_m2; uh_dmatch* h_ma; unsigned char* h_bad2;
    unsigned long long* host_done; unsigned long long word;
};

__global__ __launch_bounds__(kTrkThreads) void track_publish_kernel(TrkPublish p) {
    const int tid = threadIdx.x;
    const int n1 = min(p.hdr[kTrkN1], p.cap1), n2 = min(p.hdr[kTrkN2], p.cap2), na = min(p.hdr[kTrkNA], p.capa);
    if (tid < kTrkHdrInts) p.h_hdr[tid] = p.hdr[tid];
    if (tid < 16) { p.h_pose1[tid] = p.pose1[tid]; p.h_pose2[tid] = p.pose2[tid]; }
    const uint4* s; uint4* d;
    s = reinterpret_cast<const uint4*>(p.m1); d = reinterpret_cast<uint4*>(p.h_m1);
    for (int i = tid; i < n1; i += kTrkThreads) d[i] = s[i];
    s = reinterpret_cast<const uint4*>(p.m2); d = reinterpret_cast<uint4*>(p.h_m2);
    for (int i = tid; i < n2; i += kTrkThreads) d[i] = s[i];
    s = reinterpret_cast<const uint4*>(p.ma); d = reinterpret_cast<uint4*>(p.h_ma);
    for (int i = tid; i < na; i += kTrkThreads) d[i] = s[i];
    for (int i = tid; i < n1; i += kTrkThreads) p.h_bad1[i] = p.bad1[i];
    for (int i = tid; i < na; i += kTrkThreads) p.h_bad2[i] = p.bad2[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // every thread: its stores into pinned memory before the word
    __syncthreads();
    if (tid == 0) __hip_atomic_store(p.host_done, p.word, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

struct uh_track_state {
    uh::DevBuf d;          // header | poses | PmDyn | lists | solver arrays | scratch (TrkLayout)
    uh::MappedBuf h_par;   // pinned, read by the launches in place: [completion word | pose0 | intr | inv sigma per level | depth per keypoint | markers]
    uh::MappedBuf h_out;   // pinned: the results
    unsigned long long seq = 0;
    bool attr_set = false;
    uh::DevBuf d_clk;      // UH_TRK_CLK (measurement)
};

uh_projmatch::~uh_projmatch() { delete track; if (reloc && reloc_free) reloc_free(reloc); }

namespace {

// One call's list capacities and the byte offsets of uh_track_state's blocks (uh::Layout, 256-byte regions).  The device block begins with
// the results, laid out as the pinned result block, which is that prefix; the parameter block has 64-byte regions behind the completion word.
struct TrkLayout {
    int cap1, cap2, capa, capn;   // the first search's list, the second's, the union; capn: a filtered list holds one match per keypoint at most
    size_t hdr, pose1, pose2, m1, bad1, m2, ma, bada, out_bytes;
    size_t pose_map, dyn, src1, src2, srca, p3d, kp, isg, wgt, sa, sb, pos_prev, pos_map, aux_prev, aux_map, dep_kp, dep, seen, d_bytes;
    size_t par_pose0, par_intr, par_isl, par_dep, par_mkp, par_mks, par_mkc, par_bytes;
};

TrkLayout trk_layout(int np, int nm, int nk, bool stereo, int n_mk) {
    TrkLayout L;
    L.cap1 = std::max(np, 1); L.cap2 = std::max(nm, 1); L.capa = std::max(np + nm, 1); L.capn = std::min(L.capa, std::max(nk, 1));
    const size_t c1 = L.cap1, c2 = L.cap2, ca = L.capa;
    uh::Layout d;
    L.hdr = d.take<int>(kTrkHdrInts); L.pose1 = d.take<float>(16); L.pose2 = d.take<float>(16);
    L.m1 = d.take<uh_dmatch>(c1); L.bad1 = d.take<unsigned char>(c1); L.m2 = d.take<uh_dmatch>(c2); L.ma = d.take<uh_dmatch>(ca); L.bada = d.take<unsigned char>(ca);
    L.out_bytes = d.off;
    L.pose_map = d.take<float>(16); L.dyn = d.take<PmDyn>(1); L.src1 = d.take<int>(c1); L.src2 = d.take<int>(c2); L.srca = d.take<int>(ca);
    L.p3d = d.take<float>(3 * ca); L.kp = d.take<float>(2 * ca); L.isg = d.take<float>(ca); L.wgt = d.take<float>(ca); L.sa = d.take<TrkElem>(ca); L.sb = d.take<TrkElem>(ca);
    L.pos_prev = d.take<float4>(c1); L.pos_map = d.take<float4>(c2); L.aux_prev = d.take<uint4>(c1); L.aux_map = d.take<uint4>(c2);
    L.dep_kp = d.take<float>(stereo ? std::max(nk, 1) : 0); L.dep = d.take<float>(stereo ? ca : 0); L.seen = d.take<unsigned char>(c2);
    L.d_bytes = d.take<char>(0);
    uh::Layout p{64};
    L.par_pose0 = p.take<float>(16, 64); L.par_intr = p.take<float>(4, 64); L.par_isl = p.take<float>(16, 64); L.par_dep = p.take<float>(stereo ? nk : 0, 64);
    L.par_mkp = p.take<float>(16 * (size_t)n_mk, 64); L.par_mks = p.take<float>((size_t)n_mk, 64); L.par_mkc = p.take<float>(8 * (size_t)n_mk, 64);   // (uh_track_pose_markers)
    L.par_bytes = p.off;
    return L;
}

// a block's base + offset, as whatever pointer it is assigned to
struct TrkAt { char* p; template <typename T> operator T*() const { return reinterpret_cast<T*>(p); } };

// Every check of uh_track_pose (sx == NULL), uh_track_pose_stereo and uh_track_pose_markers (mk != NULL), before anything is staged
int track_validate(const uh_projmatch* h, uh_pnp* pnp, const uh_track_args* a, const uh_track_stereo* sx, const uh_pnp_markers* mk, const uh_track_result* r) {
    UH_REQUIRE(h && pnp && a && r, "uh_track_pose: NULL argument");
    if (mk) {
        UH_REQUIRE(mk->n >= 0 && mk->n <= UH_PNP_MAX_MARKERS, "uh_track_pose_markers: %d markers outside [0, %d]", mk->n, UH_PNP_MAX_MARKERS);
        if (mk->n > 0) UH_REQUIRE(mk->pose_g2m && mk->size && mk->und_corners, "uh_track_pose_markers: NULL marker arrays");
        for (int i = 0; i < mk->n; i++) UH_REQUIRE(std::isfinite(mk->size[i]) && mk->size[i] > 0.f, "uh_track_pose_markers: marker %d has size %g", i, (double)mk->size[i]);
    }
    UH_REQUIRE(h->have_frame && h->dev, "uh_track_pose: needs a device-resident frame (uh_orb_extract_frame_dev + uh_projmatch_set_frame_dev)");
    UH_REQUIRE(a->pose0 && a->intr4 && a->prev && a->map && a->inv_sigma_levels, "uh_track_pose: NULL input");
    UH_REQUIRE(a->n_levels >= 1 && a->n_levels <= 16, "uh_track_pose: %d levels", a->n_levels);
    const int np = a->prev->n, nm = a->map->n, nk = h->n_kpts;
    UH_REQUIRE(np >= 0 && nm >= 0, "uh_track_pose: negative candidate count");
    UH_REQUIRE(nk <= 4096, "uh_track_pose: %d keypoints exceed the list filter's 4096", nk);
    UH_REQUIRE(a->prev_max_repj_dist > 0 && a->map_radius_tracked > 0 && a->map_radius_lost > 0, "uh_track_pose: search radii must be > 0");
    if (np) UH_REQUIRE(a->prev->ids && a->prev->pos3d && a->prev->octave && a->prev->desc, "uh_track_pose: previous-frame arrays missing");
    if (nm) UH_REQUIRE(a->map->ids && a->map->pos3d && a->map->normal && a->map->min_dist && a->map->max_dist && a->map->desc, "uh_track_pose: map point arrays missing");
    for (int i = 0; i < np; i++)
        UH_REQUIRE(a->prev->octave[i] >= 0 && a->prev->octave[i] < h->n_levels, "uh_track_pose: octave %d of item %d outside [0,%d)", a->prev->octave[i], i, h->n_levels);
    if (a->prev_map_row)   // (a row indexes map_weight on the host and the map search's positions on the device)
        for (int i = 0; i < np; i++)
            UH_REQUIRE(a->prev_map_row[i] >= -1 && a->prev_map_row[i] < nm, "%s: prev_map_row %d of item %d outside [-1,%d)", sx ? "uh_track_pose_stereo" : "uh_track_pose",
                       a->prev_map_row[i], i, nm);
    const bool any_depth = sx && sx->depth && std::any_of(sx->depth, sx->depth + nk, [](float d) { return !(d <= 0.f); });
    UH_REQUIRE(!any_depth || sx->bl > 0.f, "uh_track_pose_stereo: stereo keypoints need a baseline > 0 (bl = %g)", (double)sx->bl);
    UH_REQUIRE(r->matches_prev && r->bad_prev && r->matches_map && r->matches_all && r->bad_all, "uh_track_pose: output buffers missing");
    UH_REQUIRE(h->ctx == uh::pnp_ctx(pnp), "uh_track_pose: matcher and solver belong to different contexts");
    return UH_OK;
}

// A return between the first launch and the completion wait: the launches in flight still read the pinned blocks and slots the next call
// rewrites — wait for them, and have both slots' status words cleared again.  A failed wait does not synchronise (a hung launch would
// block the host for good): it only clears the words.
struct TrkInFlight {
    uh_projmatch* h;
    bool sync = true, done = false;
    ~TrkInFlight() { if (!done) { if (sync) (void)hipStreamSynchronize(h->ctx->stream); h->slot[0].ovf_zeroed = h->slot[1].ovf_zeroed = false; } }
};

// the select launch: its working lists in LDS while two lists of capa elements fit beside the per-keypoint table
int select_launch(uh_projmatch* h, const TrkSelect& s, int capa) {
    const size_t lds = 2 * sizeof(TrkElem) * (size_t)capa;
    const bool in_lds = lds <= 120 * 1024;
    if (in_lds && !h->track->attr_set) {
        UH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(track_select_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024));
        h->track->attr_set = true;
    }
    if (in_lds) UH_LAUNCH(h->ctx, track_select_kernel<true>, dim3(1), dim3(kTrkThreads), lds, s, capa);
    else UH_LAUNCH(h->ctx, track_select_kernel<false>, dim3(1), dim3(kTrkThreads), 0, s, capa);
    return UH_OK;
}

// uh_track_pose (sx == NULL), uh_track_pose_stereo and uh_track_pose_markers (mk: the markers of both solves, or NULL)
int track_pose(uh_projmatch* h, uh_pnp* pnp, const uh_track_args* a, const uh_track_stereo* sx, const uh_pnp_markers* mk, uh_track_result* r) {
    int rc;
    if ((rc = track_validate(h, pnp, a, sx, mk, r))) return rc;
    const int n_mk = mk ? mk->n : 0;
    UH_HIP_CHECK(hipSetDevice(h->ctx->device));
    if (!h->track) h->track = new uh_track_state();
    uh_track_state& T = *h->track;
    const int np = a->prev->n, nm = a->map->n, nk = h->n_kpts;
    const bool stereo = sx && sx->depth;
    const TrkLayout L = trk_layout(np, nm, nk, stereo, n_mk);
    static const bool trk_clk = getenv("UH_TRK_CLK") != nullptr;
    // ---- every buffer of the call before its first launch (a buffer that grows is freed, which synchronises the device)
    if ((rc = T.d.reserve(L.d_bytes)) || (rc = T.h_par.reserve(L.par_bytes)) || (rc = T.h_out.reserve(L.out_bytes))) return rc;
    if ((np && (rc = match_reserve(h, 0, np))) || (nm && (rc = match_reserve(h, 1, nm)))) return rc;
    if ((rc = uh::pnp_reserve(pnp, L.capn, stereo)) || (trk_clk && (rc = T.d_clk.reserve(16 * 8)))) return rc;
    auto at = [D = T.d.as<char>()](size_t o) { return TrkAt{D + o}; };
    auto par = [dp = T.h_par.dev<char>()](size_t o) { return TrkAt{dp + o}; };
    auto out = [dout = T.h_out.dev<char>()](size_t o) { return TrkAt{dout + o}; };
    // ---- the pinned parameters (the previous call's launches are complete: its results were awaited, or its failure drained the stream)
    char* hp = T.h_par.host<char>();
    std::memcpy(hp + L.par_pose0, a->pose0, 64);
    std::memcpy(hp + L.par_intr, a->intr4, 16);
    std::memcpy(hp + L.par_isl, a->inv_sigma_levels, 4 * (size_t)a->n_levels);
    if (stereo && nk) std::memcpy(hp + L.par_dep, sx->depth, 4 * (size_t)nk);
    if (n_mk) {   // (both solves read the markers in place, as they read the intrinsics)
        std::memcpy(hp + L.par_mkp, mk->pose_g2m, 64 * (size_t)n_mk);
        std::memcpy(hp + L.par_mks, mk->size, 4 * (size_t)n_mk);
        std::memcpy(hp + L.par_mkc, mk->und_corners, 32 * (size_t)n_mk);
    }
    std::atomic_thread_fence(std::memory_order_release);   // (every header field the publish reads is written by one of the launches below)
    int* hdr = at(L.hdr);
    // the select launch behind search k (0: the previous frame's items, 1: the local map's points; the second also forms the union)
    auto select_args = [&](int k, const PmPending& pd) {
        TrkSelect s{};
        s.nB = k ? nm : np; s.bk = pd.d_best_kp; s.bd = pd.d_best_dist; s.aux = at(k ? L.aux_map : L.aux_prev); s.map_kind = k;
        if (k) { s.carry = at(L.m1); s.carry_src = at(L.src1); s.carry_cap = L.cap1; }
        s.seen = at(L.seen); s.n_map_rows = nm;
        s.hdr = hdr; s.fresh_n_slot = k ? kTrkN2 : kTrkN1; s.final_n_slot = k ? kTrkNA : kTrkN1;
        s.fresh_out = at(k ? L.m2 : L.m1); s.fresh_src = at(k ? L.src2 : L.src1);
        if (k) { s.final_out = at(L.ma); s.final_src = at(L.srca); }
        s.pos_prev = at(L.pos_prev); s.pos_map = at(L.pos_map); s.aux_prev = at(L.aux_prev); s.aux_map = at(L.aux_map);
        s.prefer_map_row = k;   // (first solve: the candidate's own position)
        s.kp_xyo = h->dev->kd_in(); s.inv_sigma_lv = par(L.par_isl); s.n_levels = a->n_levels;
        s.p3d = at(L.p3d); s.kp = at(L.kp); s.isg = at(L.isg); s.wgt = at(L.wgt);
        s.n_kpts = nk; s.scratch_a = at(L.sa); s.scratch_b = at(L.sb);
        if (trk_clk) s.clk = T.d_clk.as<long long>() + 8 * k;
        if (stereo) { s.dep_kp = at(L.dep_kp); s.dep = at(L.dep); }
        if (stereo && !k) s.dep_src = par(L.par_dep);   // (the first select launch leaves the frame's depths in dep_kp)
        return s;
    };
    // what both solves share: the markers (read in place) and the baseline; the match arrays are those their select launch filled
    const uh_pnp_markers d_mk{n_mk, par(L.par_mkp), par(L.par_mks), par(L.par_mkc)};
    auto matches_of = [bl = stereo ? sx->bl : 0.f](const TrkSelect& s) { return uh::PnpMatches{s.p3d, s.kp, s.isg, s.wgt, s.dep, bl}; };
    TrkInFlight in_flight{h};
    // ---- 1: the search against the previous frame (slot 0), its list and look-ups, the first solve
    PmPending pd1, pd2;
    if (np) {
        const PmTrack t{a->prev_map_row, a->map_weight, sx ? sx->prev_weight : nullptr, at(L.pos_prev), at(L.aux_prev)};
        if ((rc = match_enqueue(h, 0, a->pose0, nullptr, nullptr, a->prev, a->prev_min_desc_dist, a->prev_max_repj_dist, &pd1, &t))) return rc;
    }
    // (the map candidates are staged now, while the device works on the first search: slot 1 has its own pinned block)
    const TrkSelect s1 = select_args(0, pd1);
    if ((rc = select_launch(h, s1, L.capa))) return rc;
    // (the decision — refined pose + small disc or predicted pose + wide radius — rides on the solve's last thread)
    static_assert(sizeof(PmDyn) == 17 * 4, "PmDyn is what pnp_decide writes");
    const uh::PnpDecide dec{a->min_inliers, a->map_radius_tracked, a->map_radius_lost, at(L.dyn), at(L.pose_map), hdr + kTrkTracked};
    if ((rc = uh::pnp_enqueue_dev(pnp, par(L.par_pose0), par(L.par_intr), std::min(L.cap1, L.capn), hdr + kTrkN1, matches_of(s1), &d_mk, at(L.pose1), at(L.bad1), hdr + kTrkRes1, &dec)))
        return rc;
    // ---- 2: the search of the local map at the decided pose / radius (slot 1), the union, the second solve
    if (nm) {
        const PmTrack t{nullptr, a->map_weight, nullptr, at(L.pos_map), at(L.aux_map)};
        if ((rc = match_enqueue(h, 1, nullptr, at(L.dyn), a->map, nullptr, a->map_min_desc_dist, a->map_radius_tracked, &pd2, &t))) return rc;
    }
    const TrkSelect s2 = select_args(1, pd2);
    if ((rc = select_launch(h, s2, L.capa))) return rc;
    if ((rc = uh::pnp_enqueue_dev(pnp, at(L.pose_map), par(L.par_intr), L.capn, hdr + kTrkNA, matches_of(s2), &d_mk, at(L.pose2), at(L.bada), hdr + kTrkRes2, nullptr))) return rc;
    // ---- 3: everything back in one block
    const TrkPublish pb{hdr, at(L.pose1), at(L.pose2), at(L.m1), at(L.bad1), at(L.m2), at(L.ma), at(L.bada), L.cap1, L.cap2, L.capa,   // (the pinned twins at the same offsets)
                        out(L.hdr), out(L.pose1), out(L.pose2), out(L.m1), out(L.bad1), out(L.m2), out(L.ma), out(L.bada), T.h_par.dev<unsigned long long>(), ++T.seq};
    UH_LAUNCH(h->ctx, track_publish_kernel, dim3(1), dim3(kTrkThreads), 0, pb);
    UH_HIP_CHECK(hipGetLastError());
    if ((rc = uh::wait_host_word(reinterpret_cast<volatile unsigned long long*>(hp), pb.word, h->ctx->stream, "uh_track_pose"))) { in_flight.sync = false; return rc; }
    in_flight.done = true;
    h->upload_pending = false;
    if (trk_clk) {
        long long c[16];
        UH_HIP_CHECK(hipMemcpy(c, T.d_clk.p, sizeof(c), hipMemcpyDeviceToHost));
        for (int k = 0; k < 2; k++) {
            const long long* q = c + 8 * k;
            fprintf(stderr, "track_select %d [us]: stage %.2f  candidates %.2f  filter %.2f  outputs %.2f  union+filter %.2f  look-ups %.2f  total %.2f\n", k + 1, (q[1] - q[0]) * 0.01, (q[2] - q[1]) * 0.01,
                    (q[3] - q[2]) * 0.01, (q[4] - q[3]) * 0.01, (q[5] - q[4]) * 0.01, (q[6] - q[5]) * 0.01, (q[6] - q[0]) * 0.01);
        }
    }
    // (both searches posted their own words and walk-overflow flags on the way: the stream is in order, they are long since visible)
    for (int sl = 0; sl < 2; sl++)
        UH_REQUIRE(!(sl ? nm : np) || !*reinterpret_cast<const int*>(h->slot[sl].h_out.host<char>() + 8), "uh_track_pose: kd-tree walk stack overflow");
    const char* ho = T.h_out.host<char>();
    const int* hh = reinterpret_cast<const int*>(ho + L.hdr);
    const int n1 = hh[kTrkN1], n2 = hh[kTrkN2], na = hh[kTrkNA];
    UH_REQUIRE(n1 <= r->cap_prev && n2 <= r->cap_map && na <= r->cap_all, "uh_track_pose: %d / %d / %d matches do not fit the output buffers (%d / %d / %d)", n1, n2, na, r->cap_prev, r->cap_map, r->cap_all);
    r->n_prev = n1; r->n_map = n2; r->n_all = na; r->tracked = hh[kTrkTracked];
    r->inliers1 = hh[kTrkRes1]; r->inliers2 = hh[kTrkRes2];
    for (int i = 0; i < 4; i++) { r->iters1[i] = hh[kTrkRes1 + 1 + i]; r->iters2[i] = hh[kTrkRes2 + 1 + i]; }
    std::memcpy(r->pose1, ho + L.pose1, 64); std::memcpy(r->pose2, ho + L.pose2, 64);
    if (n1) { std::memcpy(r->matches_prev, ho + L.m1, 16 * (size_t)n1); std::memcpy(r->bad_prev, ho + L.bad1, (size_t)n1); }
    if (n2) std::memcpy(r->matches_map, ho + L.m2, 16 * (size_t)n2);
    if (na) { std::memcpy(r->matches_all, ho + L.ma, 16 * (size_t)na); std::memcpy(r->bad_all, ho + L.bada, (size_t)na); }
    return UH_OK;
}

}  // namespace

extern "C" {

int uh_track_pose(uh_projmatch* h, uh_pnp* pnp, const uh_track_args* a, uh_track_result* r) { return track_pose(h, pnp, a, nullptr, nullptr, r); }

int uh_track_pose_stereo(uh_projmatch* h, uh_pnp* pnp, const uh_track_args* a, const uh_track_stereo* stereo, uh_track_result* r) {
    UH_REQUIRE(stereo, "uh_track_pose_stereo: NULL stereo argument");
    return track_pose(h, pnp, a, stereo, nullptr, r);
}

int uh_track_pose_markers(uh_projmatch* h, uh_pnp* pnp, const uh_track_args* a, const uh_track_stereo* stereo, const uh_pnp_markers* markers, uh_track_result* r) {
    return track_pose(h, pnp, a, stereo, markers, r);
}

}  // extern "C"
