// uh_relocalize_pose: System::relocalize's pose search (src/utils/system.cpp ~4950-5500) for ALL candidate keyframes of one lost frame as ONE
// host call.  Through the C ABI operator by operator (ucoslam-cv3_amd/relocalize.py::relocalize_pose, examples/relocalize.cpp) the chain is one
// batched uh_pnp_ransac and then, per surviving candidate, a uh_projmatch_match, an id -> row table on the host and a uh_pnp_solve, each with
// its own upload, wait and download: up to 17 host round trips for eight candidates that do not depend on each other.  Here the host
// stages every candidate once, enqueues EIGHT launches on the context stream whatever the number of candidates, and waits once:
//   reloc_gather_kernel     the RANSAC problems' keypoints from the device-resident frame (kp[j] = und_kpts[query_idx[j]])
//   pr_hypothesis_kernel, pr_select_kernel   uh_pnp_ransac's two launches, without its download and wait (pnp_ransac_stage / _launch)
//   reloc_gate_kernel       per candidate: the count after RANSAC (n_inliers when ok, else all matches), the gate, the search's pose and
//                           camCenter (PmDyn, skip = stopped)
//   projmatch_batch_kernel  Map::matchFrameToMapPoints of every live candidate over its own point list: blockIdx.y = candidate, the body of
//                           projmatch_kernel; positions and {id, row, weight} records stay in HBM for the look-ups
//   reloc_select_kernel     one workgroup per candidate: the hits in point order, filter_ambiguous_query (trk_filter), the match list, the
//                           solver's arrays, the gate on the list's length (the solve's match count: 0 = stopped)
//   pnp_solve_batch_kernel  one workgroup per candidate, the body of pnp_solve_kernel; arguments from a table, match count from device memory
//   reloc_publish_kernel    n_good per candidate and its gate, the ordered arg-max (strict >: the first wins), everything the call returns
//                           into the pinned result block, one completion word
// Same results as the chain of single calls, bit for bit (tests/test_relocalize_onecall.py): the same device code searches and solves; the
// list logic is integer work with ordered prefix sums (no atomics whose order could show).
// This file is included at the end of projmatch.hip, behind track.hpp (it uses both units' internals).
#pragma once

namespace uh {
int pnp_ransac_stage(const char* fn, uh_pnp* p, const float* intr4, int n_problems, const uh_ransac_problem* problems, uh_ransac_result* results, bool kp_on_device,
                     RansacStaged* sg);
int pnp_ransac_launch(uh_pnp* p);
void pnp_ransac_host_pose(const float* rt6, float* pose16);
size_t pnp_batch_table_bytes(int count);
int pnp_enqueue_batch(uh_pnp* p, const float* d_intr4, int count, const PnpBatchItem* items, void* h_table, const void* d_table);
}

namespace {

enum : int { kRelNMap = 0, kRelNSolve = 1, kRelStage = 2, kRelAfter = 3, kRelInts = 4 };   // per candidate, device ints

// One candidate as the launches see it (pinned parameter block, read in place)
struct RelCand {
    int n, pass0, live, m_off;      // matches; n >= min_matches_ransac; index among RANSAC's device problems or -1 (n < 4); first match in the concatenated arrays
    int np, cap, pad0, pad1;        // points; capacity of its lists = min(np, keypoints)
    float host_rt6[6], host_pose[16];   // live < 0: the result of a RANSAC problem below four matches (uh_pnp_ransac: ok = 0, rt6_in, no launch)
    const int* bk; const float* bd; const float4* pos; const uint4* aux;   // the search's results and what it left for the look-ups (HBM)
    TrkElem* sa; TrkElem* sb;
    uh_dmatch* m; float* p3d; float* kp; float* isg; float* wgt; unsigned char* bad;
    float* pose_in; float* pose_out; int* res5;
    uh_dmatch* h_m; unsigned char* h_bad; int* h_inl;   // pinned twins
};

// What the publish launch writes per candidate (pinned)
struct RelOut { int stage, ok, n_inliers, best_iter, n_map, solve_inliers, n_good, pad; int iters[4]; float rt6[6]; float pose_ransac[16]; float pose_solve[16]; int pad2[14]; };
static_assert(sizeof(RelOut) == 256, "result record");
struct RelHead { int best, n_matches, overflow, pad; float pose[16]; };

__global__ __launch_bounds__(256) void reloc_gather_kernel(const int* __restrict__ qidx, int n, const float4* __restrict__ kp_xyo, float* __restrict__ kp) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const float4 k = kp_xyo[qidx[j]];   // (the host checked 0 <= qidx < keypoints)
    kp[2 * j] = k.x; kp[2 * j + 1] = k.y;
}

struct RelGate { int n_cand, min_after; float radius; const RelCand* cand; const uh::RansacOut* rout; PmDyn* dyn; int* st; };

__global__ __launch_bounds__(64) void reloc_gate_kernel(RelGate g) {
    const int c = threadIdx.x;
    if (c >= g.n_cand) return;
    const RelCand& q = g.cand[c];
    int* st = g.st + kRelInts * c;
    PmDyn* d = g.dyn + c;
    int stage = UH_RELOC_FEW_MATCHES, skip = 1, after = 0;
    if (q.pass0) {
        const int ok = q.live >= 0 ? g.rout[q.live].ok : 0, n_inl = q.live >= 0 ? g.rout[q.live].n_inliers : 0;
        const float* T = q.live >= 0 ? g.rout[q.live].pose : q.host_pose;
        after = ok ? n_inl : q.n;   // the reference gates on the list's size, which a failed solvePnPRansac leaves untouched
        stage = UH_RELOC_FEW_AFTER_RANSAC;
        if (after >= g.min_after) { stage = UH_RELOC_FEW_MAP; skip = 0; }
        for (int i = 0; i < 12; i++) d->ps.T[i] = T[i];
        // camCenter = pose_f2g.inv() * (0,0,0), se3transform.h:89-113 — the float expressions of match_enqueue
        const float m0 = T[0], m1 = T[4], m2 = T[8], m4 = T[1], m5 = T[5], m6 = T[9], m8 = T[2], m9 = T[6], m10 = T[10];
        const float m3 = -(T[3] * m0 + T[7] * m1 + T[11] * m2), m7 = -(T[3] * m4 + T[7] * m5 + T[11] * m6), m11 = -(T[3] * m8 + T[7] * m9 + T[11] * m10);
        d->ps.cc[0] = m0 * 0.f + m1 * 0.f + m2 * 0.f + m3;
        d->ps.cc[1] = m4 * 0.f + m5 * 0.f + m6 * 0.f + m7;
        d->ps.cc[2] = m8 * 0.f + m9 * 0.f + m10 * 0.f + m11;
        d->radius = g.radius;
        for (int i = 0; i < 16; i++) q.pose_in[i] = T[i];
    }
    d->skip = skip;
    st[kRelStage] = stage; st[kRelAfter] = after;
}

struct RelSelect { const RelCand* cand; const PmDyn* dyn; int* st; int min_map; const float4* kp_xyo; const float* inv_sigma_lv; int n_levels, n_kpts; };

__global__ __launch_bounds__(kTrkThreads) void reloc_select_kernel(RelSelect a) {
    __shared__ unsigned long long s_best[4096];
    __shared__ int s_wave[kTrkThreads / 64];
    __shared__ float s_isl[16];
    const int c = blockIdx.x, tid = threadIdx.x;
    int* st = a.st + kRelInts * c;
    if (a.dyn[c].skip) {   // (uniform) stopped before the search: no list, and the solve's workgroup leaves at once
        if (tid == 0) { st[kRelNMap] = 0; st[kRelNSolve] = 0; }
        return;
    }
    const RelCand q = a.cand[c];   // (pinned memory: read once)
    if (tid < 16) s_isl[tid] = tid < a.n_levels ? a.inv_sigma_lv[tid] : 0.f;
    TrkElem* const LA = q.sa;
    TrkElem* const LB = q.sb;
    // ---- the search's hits in point order
    int nF = 0;
    for (int p0 = 0; p0 < q.np; p0 += kTrkThreads * kTrkItems) {
        int kpi[kTrkItems], cnt = 0;
        unsigned id[kTrkItems];
        float dist[kTrkItems];
#pragma unroll
        for (int u = 0; u < kTrkItems; u++) {
            const int i = p0 + tid * kTrkItems + u;
            kpi[u] = -1; id[u] = 0; dist[u] = 0.f;
            if (i < q.np) { kpi[u] = q.bk[i]; id[u] = q.aux[i].x; dist[u] = q.bd[i]; }
            cnt += kpi[u] >= 0 ? 1 : 0;
        }
        int tot;
        int o = nF + trk_block_offset(cnt, s_wave, tot);
#pragma unroll
        for (int u = 0; u < kTrkItems; u++) if (kpi[u] >= 0) LA[o++] = TrkElem{kpi[u], id[u], dist[u], p0 + tid * kTrkItems + u};
        nF += tot;
    }
    __syncthreads();
    // ---- filter_ambiguous_query (uh_projmatch_match ends with it)
    const int n_map = trk_filter(LA, nF, LB, s_best, a.n_kpts, s_wave);
    // ---- the match list and the solver's per-match look-ups (relocalize.py: the matched row of the candidate's points, the frame's
    // undistorted keypoint, 1 / scaleFactor of its octave, the row's weight)
    for (int p = tid; p < n_map; p += kTrkThreads) {
        const TrkElem e = LB[p];
        q.m[p] = uh_dmatch{e.query, (int)e.id, -1, e.dist};
        const float4 pos = q.pos[e.src];
        q.p3d[3 * p] = pos.x; q.p3d[3 * p + 1] = pos.y; q.p3d[3 * p + 2] = pos.z;
        q.wgt[p] = __uint_as_float(q.aux[e.src].z);
        const float4 k = a.kp_xyo[e.query];
        q.kp[2 * p] = k.x; q.kp[2 * p + 1] = k.y;
        const int oct = (int)(__float_as_uint(k.z) & 15u);
        q.isg[p] = s_isl[oct < a.n_levels ? oct : 0];
    }
    if (tid == 0) {
        const int on = n_map >= a.min_map ? 1 : 0;
        st[kRelNMap] = n_map; st[kRelNSolve] = on ? n_map : 0;
        st[kRelStage] = on ? UH_RELOC_FEW_GOOD : UH_RELOC_FEW_MAP;
    }
}

struct RelPublish {
    int n_cand, min_good;
    const RelCand* cand; const int* st; const uh::RansacOut* rout; const int* d_inliers; int* overflow;
    RelHead* h_head; RelOut* h_out;
    unsigned long long* host_done; unsigned long long word;
};

__global__ __launch_bounds__(kTrkThreads) void reloc_publish_kernel(RelPublish p) {
    __shared__ int s_good[UH_RANSAC_MAX_PROBLEMS], s_stage[UH_RANSAC_MAX_PROBLEMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- n_good per candidate (one wave each, no atomics) and the last gate
    for (int c = wave; c < p.n_cand; c += kTrkThreads / 64) {
        const int* st = p.st + kRelInts * c;
        const int ns = st[kRelNSolve];
        const unsigned char* bad = p.cand[c].bad;
        int good = 0;
        for (int i0 = 0; i0 < ns; i0 += 64) {
            const int i = i0 + lane;
            good += __popcll(__ballot(i < ns && bad[i] == 0));
        }
        int stage = st[kRelStage];
        if (stage == UH_RELOC_FEW_GOOD && good >= p.min_good) stage = UH_RELOC_SOLVED;
        if (lane == 0) { s_good[c] = stage >= UH_RELOC_FEW_GOOD ? good : 0; s_stage[c] = stage; }
    }
    __syncthreads();
    // ---- the winner: the strictly largest n_good among the solved candidates, the first on ties
    if (tid == 0) {
        int best = -1, best_n = 0;
        for (int c = 0; c < p.n_cand; c++)
            if (s_stage[c] == UH_RELOC_SOLVED && s_good[c] > best_n) { best = c; best_n = s_good[c]; }
        p.h_head->best = best; p.h_head->n_matches = best_n; p.h_head->pad = 0;
        p.h_head->overflow = __hip_atomic_load(p.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p.overflow, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (for the next call)
        for (int i = 0; i < 16; i++) p.h_head->pose[i] = best >= 0 ? p.cand[best].pose_out[i] : 0.f;
    }
    // ---- per candidate: what its stages left, neutral values for those it never reached
    for (int c = 0; c < p.n_cand; c++) {
        const RelCand q = p.cand[c];
        const int* st = p.st + kRelInts * c;
        const int stage = s_stage[c];
        const bool ran = stage >= UH_RELOC_FEW_AFTER_RANSAC, searched = stage >= UH_RELOC_FEW_MAP, solved = stage >= UH_RELOC_FEW_GOOD;
        const uh::RansacOut* ro = (ran && q.live >= 0) ? p.rout + q.live : nullptr;
        RelOut& o = p.h_out[c];
        const int n_inl = ro ? ro->n_inliers : 0, n_map = searched ? st[kRelNMap] : 0;
        if (tid == 0) {
            o.stage = stage; o.ok = ro ? ro->ok : 0; o.n_inliers = n_inl; o.best_iter = ro ? ro->best_iter : -1;
            o.n_map = n_map; o.solve_inliers = solved ? q.res5[0] : 0; o.n_good = s_good[c]; o.pad = 0;
        }
        if (tid < 4) o.iters[tid] = solved ? q.res5[1 + tid] : 0;
        if (tid < 6) o.rt6[tid] = ro ? ro->rt6[tid] : (ran ? q.host_rt6[tid] : 0.f);
        if (tid < 16) {
            o.pose_ransac[tid] = ro ? ro->pose[tid] : (ran ? q.host_pose[tid] : 0.f);
            o.pose_solve[tid] = solved ? q.pose_out[tid] : 0.f;
        }
        if (q.h_inl) for (int i = tid; i < n_inl; i += kTrkThreads) q.h_inl[i] = p.d_inliers[q.m_off + i];
        const uint4* s = reinterpret_cast<const uint4*>(q.m);
        uint4* d = reinterpret_cast<uint4*>(q.h_m);
        for (int i = tid; i < n_map; i += kTrkThreads) d[i] = s[i];
        if (solved) for (int i = tid; i < n_map; i += kTrkThreads) q.h_bad[i] = q.bad[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // every thread: its stores into pinned memory before the word
    __syncthreads();
    if (tid == 0) __hip_atomic_store(p.host_done, p.word, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct uh_reloc_state {
    uh::DevBuf d;          // walk status | per-candidate counts | PmDyn | poses | per candidate: search results, lists, solver arrays
    uh::MappedBuf h_par;   // pinned, read by the launches in place: [completion word | intr | inv sigma | candidates | tables | query indices | point records]
    uh::MappedBuf h_out;   // pinned: the results
    unsigned long long seq = 0;
    unsigned status_gen = 0; bool status_zeroed = false;
    bool attr_set = false;
    std::vector<int32_t> samples;   // drawn for the candidates that come without
};
void reloc_free(void* s) { delete static_cast<uh_reloc_state*>(s); }

// A return between the first enqueue and the completion wait: what is in flight still reads the pinned blocks the next call rewrites
struct RelInFlight {
    uh_projmatch* h; uh_reloc_state* T;
    bool sync = true, done = false;
    ~RelInFlight() { if (!done) { if (sync) (void)hipStreamSynchronize(h->ctx->stream); T->status_zeroed = false; } }
};

int reloc_validate(const uh_projmatch* h, uh_pnp* pnp, const uh_reloc_args* a, int n_cand, const uh_reloc_candidate* cands, const uh_reloc_result* r) {
    const char* fn = "uh_relocalize_pose";
    UH_REQUIRE(h && pnp && a && r, "%s: NULL argument", fn);
    UH_REQUIRE(n_cand >= 0 && n_cand <= UH_RANSAC_MAX_PROBLEMS, "%s: %d candidates outside [0, %d]", fn, n_cand, UH_RANSAC_MAX_PROBLEMS);
    UH_REQUIRE(a->intr4 && a->inv_sigma_levels, "%s: NULL input", fn);
    for (int k = 0; k < 4; k++) UH_REQUIRE(std::isfinite(a->intr4[k]), "%s: non-finite intrinsics (intr4[%d] = %g)", fn, k, (double)a->intr4[k]);
    UH_REQUIRE(a->n_levels >= 1 && a->n_levels <= 16, "%s: %d levels", fn, a->n_levels);
    UH_REQUIRE(a->map_radius > 0, "%s: the search radius must be > 0", fn);
    UH_REQUIRE(a->max_iters >= 1 && a->max_iters <= UH_RANSAC_MAX_ITERS, "%s: %d iterations outside [1, %d]", fn, a->max_iters, UH_RANSAC_MAX_ITERS);
    UH_REQUIRE(h->have_frame && h->dev, "%s: needs a device-resident frame (uh_orb_extract_frame_dev / uh_dev_frame_upload + uh_projmatch_set_frame_dev)", fn);
    const int nk = h->n_kpts;
    UH_REQUIRE(nk <= 4096, "%s: %d keypoints exceed the list filter's 4096", fn, nk);
    UH_REQUIRE(h->ctx == uh::pnp_ctx(pnp), "%s: matcher and solver belong to different contexts", fn);
    if (n_cand == 0) return UH_OK;
    UH_REQUIRE(cands && r->steps, "%s: NULL candidate or step array", fn);
    for (int c = 0; c < n_cand; c++) {
        const uh_reloc_candidate& q = cands[c];
        const uh_reloc_step& s = r->steps[c];
        UH_REQUIRE(q.n >= 0 && q.n <= UH_RANSAC_MAX_MATCHES, "%s: candidate %d: %d matches outside [0, %d]", fn, c, q.n, UH_RANSAC_MAX_MATCHES);
        UH_REQUIRE(q.rt6_in && q.points, "%s: candidate %d: NULL rt6_in or point list", fn, c);
        if (q.n > 0) UH_REQUIRE(q.query_idx && q.p3d && q.normal, "%s: candidate %d: NULL match arrays with n = %d", fn, c, q.n);
        for (int j = 0; j < q.n; j++) UH_REQUIRE(q.query_idx[j] >= 0 && q.query_idx[j] < nk, "%s: candidate %d: query_idx %d of match %d outside the frame's %d keypoints", fn, c, q.query_idx[j], j, nk);
        const uh_map_points& mp = *q.points;
        UH_REQUIRE(mp.n >= 0, "%s: candidate %d: negative point count", fn, c);
        if (mp.n) UH_REQUIRE(mp.ids && mp.pos3d && mp.normal && mp.min_dist && mp.max_dist && mp.desc, "%s: candidate %d: point arrays missing", fn, c);
        const int cap = std::min(mp.n, nk);
        UH_REQUIRE(s.cap_map >= cap && (cap == 0 || (s.matches_map && s.bad)), "%s: candidate %d: match buffers of %d entries for up to %d matches", fn, c, s.cap_map, cap);
        UH_REQUIRE(!s.inliers || s.cap_inliers >= q.n, "%s: candidate %d: inlier buffer of %d entries for %d matches", fn, c, s.cap_inliers, q.n);
    }
    return UH_OK;
}

int relocalize_pose(uh_projmatch* h, uh_pnp* pnp, const uh_reloc_args* a, int n_cand, const uh_reloc_candidate* cands, uh_reloc_result* r) {
    const char* fn = "uh_relocalize_pose";
    int rc;
    if ((rc = reloc_validate(h, pnp, a, n_cand, cands, r))) return rc;
    r->best = -1; r->n_matches = 0;
    std::memset(r->pose, 0, sizeof(r->pose));
    if (n_cand == 0) return UH_OK;
    UH_HIP_CHECK(hipSetDevice(h->ctx->device));
    if (!h->reloc) { h->reloc = new uh_reloc_state(); h->reloc_free = reloc_free; }
    uh_reloc_state& T = *static_cast<uh_reloc_state*>(h->reloc);
    const int nk = h->n_kpts, C = n_cand;
    // ---- the RANSAC problems: the candidates that pass the first gate, in order; samples drawn for those that come without
    std::vector<uh_ransac_problem> prob;
    std::vector<int> prob_of(C, -1);
    size_t n_draw = 0;
    for (int c = 0; c < C; c++)
        if (cands[c].n >= a->min_matches_ransac && !cands[c].samples && cands[c].n >= 4) n_draw += 4 * (size_t)a->max_iters;
    T.samples.resize(std::max<size_t>(n_draw, 1));
    n_draw = 0;
    for (int c = 0; c < C; c++) {
        const uh_reloc_candidate& q = cands[c];
        if (q.n < a->min_matches_ransac) continue;
        const int32_t* smp = q.samples;
        if (!smp && q.n >= 4) {
            if ((rc = uh_pnp_ransac_samples(q.n, a->max_iters, T.samples.data() + n_draw))) return rc;
            smp = T.samples.data() + n_draw;
            n_draw += 4 * (size_t)a->max_iters;
        }
        prob_of[c] = (int)prob.size();
        prob.push_back(uh_ransac_problem{q.n, q.p3d, q.normal, nullptr, a->max_iters, smp, q.rt6_in});
    }
    // ---- the blocks' layouts
    struct Off { size_t rec, aux, bk, bd, pos, daux, sa, sb, m, p3d, kp, isg, wgt, bad, h_m, h_bad, h_inl; };
    std::vector<Off> off(C);
    uh::Layout P{64}, D, O{64};
    const size_t p_intr = P.take<float>(4, 64), p_isl = P.take<float>(16, 64), p_cand = P.take<RelCand>(C, 64), p_items = P.take<PmBatchItem>(C, 64);
    const size_t p_pnp = P.take<char>(uh::pnp_batch_table_bytes(C), 64);
    size_t N = 0;   // the RANSAC's device problems' matches, concatenated
    for (int c = 0; c < C; c++) if (prob_of[c] >= 0 && cands[c].n >= 4) N += (size_t)cands[c].n;
    const size_t p_qidx = P.take<int>(std::max<size_t>(N, 1), 64);
    // (the walk status block first: it is zeroed once per allocation and must not move with the number of candidates)
    const size_t d_status = D.take<char>(256), d_st = D.take<int>(kRelInts * (size_t)C), d_dyn = D.take<PmDyn>(C), d_pin = D.take<float>(16 * (size_t)C), d_pout = D.take<float>(16 * (size_t)C),
                 d_res = D.take<int>(8 * (size_t)C);
    const size_t o_head = O.take<RelHead>(1, 64), o_out = O.take<RelOut>(C, 64);
    int np_max = 0;
    size_t np_total = 0;
    for (int c = 0; c < C; c++) {
        const size_t np = (size_t)cands[c].points->n, cap = std::min<size_t>(np, (size_t)nk), n1 = std::max<size_t>(np, 1), c1 = std::max<size_t>(cap, 1);
        np_max = std::max(np_max, (int)np); np_total += np;
        Off& o = off[c];
        o.rec = P.take<uint4>(4 * n1, 64); o.aux = P.take<uint4>(n1, 64);
        o.bk = D.take<int>(n1); o.bd = D.take<float>(n1); o.pos = D.take<float4>(n1); o.daux = D.take<uint4>(n1); o.sa = D.take<TrkElem>(n1); o.sb = D.take<TrkElem>(c1);
        o.m = D.take<uh_dmatch>(c1); o.p3d = D.take<float>(3 * c1); o.kp = D.take<float>(2 * c1); o.isg = D.take<float>(c1); o.wgt = D.take<float>(c1); o.bad = D.take<unsigned char>(c1);
        o.h_m = O.take<uh_dmatch>(c1, 64); o.h_bad = O.take<unsigned char>(c1, 64); o.h_inl = O.take<int>(std::max(cands[c].n, 1), 64);
    }
    const size_t par_bytes = P.take<char>(0, 64), d_bytes = D.take<char>(0), out_bytes = O.take<char>(0, 64);
    // ---- every buffer of the call before its first enqueue (a buffer that grows is freed, which synchronises the device)
    if ((rc = T.d.reserve(d_bytes)) || (rc = T.h_par.reserve(par_bytes)) || (rc = T.h_out.reserve(out_bytes))) return rc;
    char* hp = T.h_par.host<char>();
    char* dp = T.h_par.dev<char>();
    char* dd = T.d.as<char>();
    char* ho = T.h_out.host<char>();
    char* dout = T.h_out.dev<char>();
    // ---- the pinned parameters (the previous call's launches are complete: its results were awaited, or its failure drained the stream)
    std::memcpy(hp + p_intr, a->intr4, 16);
    std::memset(hp + p_isl, 0, 64);
    std::memcpy(hp + p_isl, a->inv_sigma_levels, 4 * (size_t)a->n_levels);
    RelCand* hc = reinterpret_cast<RelCand*>(hp + p_cand);
    PmBatchItem* hi = reinterpret_cast<PmBatchItem*>(hp + p_items);
    std::vector<uh::PnpBatchItem> solves(C);
    int* hq = reinterpret_cast<int*>(hp + p_qidx);
    int live = 0;
    size_t m_off = 0;
    for (int c = 0; c < C; c++) {
        const uh_reloc_candidate& q = cands[c];
        const Off& o = off[c];
        RelCand& k = hc[c];
        k = RelCand{};
        k.n = q.n; k.pass0 = prob_of[c] >= 0 ? 1 : 0; k.live = -1; k.np = q.points->n; k.cap = std::min(k.np, nk);
        if (k.pass0 && q.n >= 4) {
            k.live = live++; k.m_off = (int)m_off;
            std::memcpy(hq + m_off, q.query_idx, 4 * (size_t)q.n);
            m_off += (size_t)q.n;
        } else if (k.pass0) {   // (a gate below four lets such a candidate through: uh_pnp_ransac's answer without a launch)
            std::memcpy(k.host_rt6, q.rt6_in, sizeof(k.host_rt6));
            uh::pnp_ransac_host_pose(k.host_rt6, k.host_pose);
        }
        auto at = [dd](size_t x) { return TrkAt{dd + x}; };
        k.bk = at(o.bk); k.bd = at(o.bd); k.pos = at(o.pos); k.aux = at(o.daux); k.sa = at(o.sa); k.sb = at(o.sb);
        k.m = at(o.m); k.p3d = at(o.p3d); k.kp = at(o.kp); k.isg = at(o.isg); k.wgt = at(o.wgt); k.bad = at(o.bad);
        k.pose_in = at(d_pin + 64 * (size_t)c); k.pose_out = at(d_pout + 64 * (size_t)c); k.res5 = at(d_res + 32 * (size_t)c);
        k.h_m = reinterpret_cast<uh_dmatch*>(dout + o.h_m); k.h_bad = reinterpret_cast<unsigned char*>(dout + o.h_bad);
        k.h_inl = r->steps[c].inliers ? reinterpret_cast<int*>(dout + o.h_inl) : nullptr;
        const PmTrack t{nullptr, q.weight, nullptr, nullptr, nullptr};
        pm_pack(hp + o.rec, hp + o.aux, q.points, nullptr, &t);
        PmPoints& mp = hi[c].mp;
        mp = PmPoints{};
        mp.n = k.np; mp.rec = reinterpret_cast<const uint4*>(dp + o.rec);
        mp.best_kp = at(o.bk); mp.best_dist = at(o.bd); mp.visible = nullptr;
        mp.pos_out = at(o.pos); mp.aux_in = reinterpret_cast<const uint4*>(dp + o.aux); mp.aux_out = at(o.daux);
        hi[c].dyn = reinterpret_cast<const PmDyn*>(dd + d_dyn) + c;
        solves[c] = uh::PnpBatchItem{k.pose_in, k.cap, reinterpret_cast<const int*>(dd + d_st) + kRelInts * c + kRelNSolve, uh::PnpMatches{k.p3d, k.kp, k.isg, k.wgt, nullptr, 0.f},
                                     k.pose_out, k.bad, k.res5};
    }
    std::atomic_thread_fence(std::memory_order_release);
    hipStream_t st = h->ctx->stream;
    RelInFlight in_flight{h, &T};
    if (!T.status_zeroed || T.status_gen != T.d.gen) {   // the walk-overflow word: zero once per allocation, the publish launch clears it after every call
        UH_HIP_CHECK(hipMemsetAsync(dd + d_status, 0, 256, st));
        T.status_zeroed = true; T.status_gen = T.d.gen;
    }
    // ---- 1: RANSAC for every candidate that passes the first gate (its keypoints gathered from the device-resident frame)
    uh::RansacStaged sg{};
    if (!prob.empty()) {
        if ((rc = uh::pnp_ransac_stage(fn, pnp, a->intr4, (int)prob.size(), prob.data(), nullptr, true, &sg))) return rc;
        if (sg.live) {
            UH_LAUNCH(h->ctx, reloc_gather_kernel, dim3(uh_div_up((int)N, 256)), dim3(256), 0, reinterpret_cast<const int*>(dp + p_qidx), (int)N, h->dev->kd_in(), sg.d_kp);
            if ((rc = uh::pnp_ransac_launch(pnp))) return rc;
        }
    }
    // ---- 2: the gate behind RANSAC and the search's pose per candidate
    const RelCand* d_cand = reinterpret_cast<const RelCand*>(dp + p_cand);
    PmDyn* d_dynp = reinterpret_cast<PmDyn*>(dd + d_dyn);
    int* d_stp = reinterpret_cast<int*>(dd + d_st);
    const RelGate g{C, a->min_matches_after_ransac, a->map_radius, d_cand, sg.d_out, d_dynp, d_stp};
    UH_LAUNCH(h->ctx, reloc_gate_kernel, dim3(1), dim3(64), 0, g);
    // ---- 3: the projection search of every live candidate over its own points
    {
        const int n_nodes = h->n_nodes, levels = h->max_depth + 2;
        const int ncu = std::max(h->ctx->num_cus, 64);
        const int gpw = std::min(kGroupsMax, std::max(4, uh_div_up((int)std::min<size_t>(np_total, 1u << 30), ncu)));
        const size_t stack_bytes = (size_t)levels * gpw * 24 + (size_t)kCandCap * gpw * 8 + 64;
        const size_t tree_bytes = (((size_t)n_nodes * sizeof(KdNodeDev) + 15) & ~(size_t)15) + 16 * (size_t)nk;
        const bool no_lds = getenv("UH_PROJMATCH_NO_LDS") != nullptr;
        const bool in_lds = tree_bytes + stack_bytes <= kLdsBudget && !no_lds;
        const size_t lds = stack_bytes + (in_lds ? tree_bytes : 0);
        if (!T.attr_set) {
#define UH_RL_ATTR(A, B) UH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(projmatch_batch_kernel<A, B>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget))
            UH_RL_ATTR(true, true); UH_RL_ATTR(false, true); UH_RL_ATTR(true, false); UH_RL_ATTR(false, false);
#undef UH_RL_ATTR
            T.attr_set = true;
        }
        const dim3 grid(std::max(1, std::min(uh_div_up(np_max, gpw), kPmMaxBlocks)), C);
        const PmBatchItem* d_items = reinterpret_cast<const PmBatchItem*>(dp + p_items);
        int* d_ovf = reinterpret_cast<int*>(dd + d_status);
        const bool lane_stack = levels <= kGroup;
#define UH_RL_LAUNCH(A, B) UH_LAUNCH(h->ctx, (projmatch_batch_kernel<A, B>), grid, dim3(gpw * kGroup), lds, h->fr, d_items, a->map_min_desc_dist, n_nodes, levels, d_ovf)
        if (lane_stack) { if (in_lds) UH_RL_LAUNCH(true, true); else UH_RL_LAUNCH(false, true); }
        else { if (in_lds) UH_RL_LAUNCH(true, false); else UH_RL_LAUNCH(false, false); }
#undef UH_RL_LAUNCH
    }
    // ---- 4: the lists, the look-ups, the gate on the list's length
    const RelSelect sel{d_cand, d_dynp, d_stp, a->min_matches_map, h->dev->kd_in(), reinterpret_cast<const float*>(dp + p_isl), a->n_levels, nk};
    UH_LAUNCH(h->ctx, reloc_select_kernel, dim3(C), dim3(kTrkThreads), 0, sel);
    UH_HIP_CHECK(hipGetLastError());
    // ---- 5: the solves
    if ((rc = uh::pnp_enqueue_batch(pnp, reinterpret_cast<const float*>(dp + p_intr), C, solves.data(), hp + p_pnp, dp + p_pnp))) return rc;
    // ---- 6: n_good, the last gate, the winner, everything back in one block
    const RelPublish pb{C, a->min_good, d_cand, d_stp, sg.d_out, sg.d_inliers, reinterpret_cast<int*>(dd + d_status), reinterpret_cast<RelHead*>(dout + o_head),
                        reinterpret_cast<RelOut*>(dout + o_out), T.h_par.dev<unsigned long long>(), ++T.seq};
    UH_LAUNCH(h->ctx, reloc_publish_kernel, dim3(1), dim3(kTrkThreads), 0, pb);
    UH_HIP_CHECK(hipGetLastError());
    if ((rc = uh::wait_host_word(reinterpret_cast<volatile unsigned long long*>(hp), pb.word, st, fn))) { in_flight.sync = false; return rc; }
    in_flight.done = true;
    h->upload_pending = false;   // (this call ran behind the frame upload on the same stream)
    const RelHead* hd = reinterpret_cast<const RelHead*>(ho + o_head);
    UH_REQUIRE(!hd->overflow, "%s: kd-tree walk stack overflow", fn);
    const RelOut* out = reinterpret_cast<const RelOut*>(ho + o_out);
    for (int c = 0; c < C; c++) {
        const RelOut& o = out[c];
        uh_reloc_step& s = r->steps[c];
        s.stage = o.stage; s.ok = o.ok; s.n_inliers = o.n_inliers; s.best_iter = o.best_iter; s.n_map = o.n_map; s.solve_inliers = o.solve_inliers; s.n_good = o.n_good;
        std::memcpy(s.iters, o.iters, sizeof(s.iters)); std::memcpy(s.rt6, o.rt6, sizeof(s.rt6));
        std::memcpy(s.pose_ransac, o.pose_ransac, sizeof(s.pose_ransac)); std::memcpy(s.pose_solve, o.pose_solve, sizeof(s.pose_solve));
        if (s.inliers && o.n_inliers) std::memcpy(s.inliers, ho + off[c].h_inl, 4 * (size_t)o.n_inliers);
        if (o.n_map) std::memcpy(s.matches_map, ho + off[c].h_m, 16 * (size_t)o.n_map);
        if (o.n_map && o.stage >= UH_RELOC_FEW_GOOD) std::memcpy(s.bad, ho + off[c].h_bad, (size_t)o.n_map);
    }
    r->best = hd->best; r->n_matches = hd->n_matches;
    std::memcpy(r->pose, hd->pose, sizeof(r->pose));
    return UH_OK;
}

}  // namespace

extern "C" int uh_relocalize_pose(uh_projmatch* pm, uh_pnp* pnp, const uh_reloc_args* args, int n_candidates, const uh_reloc_candidate* cands, uh_reloc_result* result) {
    return relocalize_pose(pm, pnp, args, n_candidates, cands, result);
}
