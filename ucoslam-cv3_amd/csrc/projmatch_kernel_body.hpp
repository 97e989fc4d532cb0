// The body of projmatch_kernel<IN_LDS, PREV, LANE_STACK> and of projmatch_batch_kernel<IN_LDS, LANE_STACK> (projmatch.hip), included inside
// both: in scope are f (PmFrame), mp (PmPoints), ps (PmPose), minDescDist, maxRepjDist, n_nodes, levels, overflow, pub (PmPublish), dyn.
// No include guard: the text is included once per kernel.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (dyn) { ps = dyn->ps; maxRepjDist = dyn->radius; }   // (uniform: scalar loads)
    const int lane = threadIdx.x, g = lane / kGroup, gl = lane % kGroup, gw = (lane & 63) / kGroup;   // gw: group within its wave
    const int nthr = (int)blockDim.x, gpw = nthr / kGroup;   // threads and groups of THIS launch's workgroups
    // measurement (UH_PM_CLK): shader-clock stamps of workgroup 0, thread 0 in the status block behind the overflow word
    long long* const clk = (overflow[1] == 0x434c4b && blockIdx.x == 0 && threadIdx.x == 0) ? reinterpret_cast<long long*>(overflow + 4) : nullptr;
    if (clk) clk[0] = __builtin_readcyclecounter();
    const int n = f.n_kpts;
    size_t off = 0;
    KdNodeDev* s_nodes = reinterpret_cast<KdNodeDev*>(smem);
    if (IN_LDS) off += ((size_t)n_nodes * sizeof(KdNodeDev) + 15) & ~(size_t)15;
    float4* s_rec = reinterpret_cast<float4*>(smem + off);
    if (IN_LDS) off += (size_t)n * 16;
    double* st_m = reinterpret_cast<double*>(smem + off) + (size_t)g * levels;
    off += (size_t)levels * gpw * 8;
    double* st_c = reinterpret_cast<double*>(smem + off) + (size_t)g * levels;
    off += (size_t)levels * gpw * 8;
    int* st_rec = reinterpret_cast<int*>(smem + off) + (size_t)g * levels;
    off += (size_t)levels * gpw * 4;
    float* st_d = reinterpret_cast<float*>(smem + off) + (size_t)g * levels;
    off += (size_t)levels * gpw * 4;
    unsigned int* s_cand = reinterpret_cast<unsigned int*>(smem + off) + (size_t)g * kCandCap;
    off += (size_t)kCandCap * gpw * 4;
    int* s_hd = reinterpret_cast<int*>(smem + off) + (size_t)g * kCandCap;
    // The candidate of this wave's FIRST chunk is requested before the frame is staged: it lies in pinned host memory (uh_projmatch_match
    // hands the points over in place), a host-link round trip that used to start only behind the staging's barrier.
    struct Cand { float P0, P1, P2, n0, n1, n2, mind, maxd; int oct; uint64_t q0, q1, q2, q3; };
    auto load_cand = [&](int mc) {
        const uint4* r = mp.rec + 4 * (size_t)mc;
        const uint4 a = r[0], b = r[1], d0 = r[2], d1 = r[3];
        Cand c;
        c.P0 = __uint_as_float(a.x); c.P1 = __uint_as_float(a.y); c.P2 = __uint_as_float(a.z);
        c.oct = (int)a.w; c.n0 = __uint_as_float(a.w); c.n1 = __uint_as_float(b.x); c.n2 = __uint_as_float(b.y);
        c.mind = __uint_as_float(b.z); c.maxd = __uint_as_float(b.w);
        c.q0 = ((uint64_t)d0.y << 32) | d0.x; c.q1 = ((uint64_t)d0.w << 32) | d0.z; c.q2 = ((uint64_t)d1.y << 32) | d1.x; c.q3 = ((uint64_t)d1.w << 32) | d1.z;
        return c;
    };
    const int m_first = (int)blockIdx.x * gpw + g;
    const Cand c_first = load_cand(m_first < mp.n ? m_first : 0);
    if (IN_LDS) {
        // 16-byte loads, eight in flight per lane and round (the node array is 24 n bytes in a 256-byte aligned block: the last chunk may
        // run 8 bytes into its padding, which the LDS area's rounding covers)
        const uint4* gn = reinterpret_cast<const uint4*>(f.nodes);
        uint4* sn = reinterpret_cast<uint4*>(s_nodes);
        constexpr int U = 8;
        const int n16 = (n_nodes * (int)sizeof(KdNodeDev) + 15) / 16;
        for (int i0 = lane; i0 < n16; i0 += U * nthr) {
            uint4 v[U];
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i0 + u * nthr; v[u] = gn[i < n16 ? i : 0]; }
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i0 + u * nthr; if (i < n16) sn[i] = v[u]; }
        }
        for (int i0 = lane; i0 < n; i0 += U * nthr) {
            float4 a[U];
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i0 + u * nthr; a[u] = f.leaf_rec[i < n ? i : 0]; }
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i0 + u * nthr; if (i < n) s_rec[i] = a[u]; }
        }
        __syncthreads();
    }
    if (clk) clk[1] = __builtin_readcyclecounter();
  for (int chunk = blockIdx.x; chunk * gpw < mp.n; chunk += gridDim.x) {
    const int m = chunk * gpw + g;
    const bool live = m < mp.n;
    const int mc = live ? m : 0;
    const Cand cd = chunk == (int)blockIdx.x ? c_first : load_cand(mc);
    // ---- visibility tests and search parameters (identical in the lanes of the group)
    bool vis = false;
    float px = 0, py = 0;
    int predicted = 0;
    double worst = 0;
    if constexpr (PREV) {
        const float P0 = cd.P0, P1 = cd.P1, P2 = cd.P2;
        const float* T = ps.T;
        const float z = P0 * T[8] + P1 * T[9] + P2 * T[10] + T[11];       // Frame::project (frame.h:140-161)
        const float x = P0 * T[0] + P1 * T[1] + P2 * T[2] + T[3];
        const float y = P0 * T[4] + P1 * T[5] + P2 * T[6] + T[7];
        const float iz = (float)(1. / z);
        px = ((f.fx * x) * iz) + f.cx; py = ((f.fy * y) * iz) + f.cy;
        vis = live && !(z < 0) && (px >= f.min_x && py >= f.min_y && px < f.max_x && py < f.max_y);
        predicted = cd.oct;
        if (vis) {
            const double radius = (double)(maxRepjDist * f.scale[predicted]);
            worst = radius * radius;
        }
    } else {
        const float P0 = cd.P0, P1 = cd.P1, P2 = cd.P2;
        float v0 = ps.cc[0] - P0, v1 = ps.cc[1] - P1, v2 = ps.cc[2] - P2;   // getViewCos
        const double s = 1. / sqrt((double)v0 * v0 + (double)v1 * v1 + (double)v2 * v2);
        v0 = (float)(v0 * s); v1 = (float)(v1 * s); v2 = (float)(v2 * s);
        const float viewCos = v0 * cd.n0 + v1 * cd.n1 + v2 * cd.n2;
        const float* T = ps.T;
        const float x = T[0] * P0 + T[1] * P1 + T[2] * P2 + T[3];
        const float y = T[4] * P0 + T[5] * P1 + T[6] * P2 + T[7];
        const float z = T[8] * P0 + T[9] * P1 + T[10] * P2 + T[11];
        const float dist = (float)sqrt((double)x * x + (double)y * y + (double)z * z);
        const float maxd = cd.maxd;
        const float iz = (float)(1. / z);
        px = x * f.fx * iz + f.cx; py = y * f.fy * iz + f.cy;
        vis = live && !(viewCos < 0.5) && !(z < 0) && (0.8f * cd.mind < dist && dist < 1.2f * maxd) &&
              (px > f.min_x && py > f.min_y && px < f.max_x && py < f.max_y);
        if (vis) {
            const int ns = (int)ceilf(logf_cr(maxd / dist) / f.log_scale);
            predicted = ns < 0 ? 0 : (ns >= f.n_levels ? f.n_levels - 1 : ns);
            float radius_scale = f.scale[predicted];
            if (viewCos < 0.98) radius_scale = (float)(radius_scale * 1.6);
            const double radius = (double)(radius_scale * maxRepjDist);
            worst = radius * radius;
        }
    }
    int best_kp = -1;
    float best_d = PREV ? (float)(minDescDist + 0.01) : 3.402823466e+38f, second_d = 3.402823466e+38f;
    const int oct_lo = PREV ? predicted : predicted - 1;
    int bestLevel = 0, bestLevel2 = -1;
    bool ovf = false;
    const uint64_t q0 = cd.q0, q1 = cd.q1, q2 = cd.q2, q3 = cd.q3;
    int ncand = 0;
    // drain: Hamming distances of the listed hits (16 lanes, one hit each per round), then the in-order best / second rule
    auto drain = [&](int cnt) {
        for (int k = gl; k < cnt; k += kGroup) {
            const uint64_t* kd = f.kp_desc + 4 * (size_t)(s_cand[k] >> 4);
            s_hd[k] = __popcll(q0 ^ kd[0]) + __popcll(q1 ^ kd[1]) + __popcll(q2 ^ kd[2]) + __popcll(q3 ^ kd[3]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int k = 0; k < cnt; k++) {
            const float hd = (float)s_hd[k];
            const unsigned int e = s_cand[k];
            const int oc = (int)(e & 15u);
            const bool lt = PREV ? true : hd < minDescDist;
            const bool isbest = lt && hd < best_d, issecond = lt && !isbest && hd < second_d;
            best_d = isbest ? hd : best_d; best_kp = isbest ? (int)(e >> 4) : best_kp; bestLevel = isbest ? oc : bestLevel;
            second_d = issecond ? hd : second_d; bestLevel2 = issecond ? oc : bestLevel2;
        }
        __builtin_amdgcn_wave_barrier();   // the list is rewritten after this
    };
    if (vis && n > 0) {
        // computeInitialDistances (float accumulator)
        double dd0 = 0, dd1 = 0;
        float distsq = 0.f;
        {
            const double ex = px, ey = py;
            if (ex < f.box[0]) { const double d = ex - f.box[0]; dd0 = d * d; distsq += dd0; }
            if (ex > f.box[1]) { const double d = ex - f.box[1]; dd0 = d * d; distsq += dd0; }
            if (ey < f.box[2]) { const double d = ey - f.box[2]; dd1 = d * d; distsq += dd1; }
            if (ey > f.box[3]) { const double d = ey - f.box[3]; dd1 = d * d; distsq += dd1; }
        }
        // Iterative searchExactLevel.  At an internal node everything the recursion does AFTER its best child returns is
        // already known when the node is entered: dst = (float)dists[col] (deeper levels only ever leave dists[col] rounded
        // to float, which the (float) cast hides), hence mindistsq' = mindistsq + cut - dst and whether the other child
        // will be searched at all.  Only nodes whose other child WILL be searched leave a record (most do not); the record
        // is turned into "restore dists[col]" in place when the other child is entered.
        int n_iter = 0, n_leaf = 0;
        // ---- Round 5: the walk of ONE point spread over the lanes of its wave.  This is a RADIUS search (`worst` never changes), and what a
        // node sees — mindistsq and the two dists[] entries — depends on the path from the root only (entering an "other" child sets
        // dists[col] = cut, a best child inherits everything; what a finished subtree leaves behind is the old value rounded to float, which
        // every later use casts to float anyway), so the subtrees can be expanded side by side: lane 0 starts at the root, every lane follows
        // its best-child chain down to a leaf, and whenever the other child must be searched too it is handed to a free lane (all of a level's
        // hand-overs at once: ballot, prefix count, ds_bpermute of the child's state).  A lane's path is its KEY — bit (63 - depth) set
        // where it was the "other" child — and the leaves' depth-first order, which the candidate list must keep (best / second without
        // demotion is order-dependent), is the order of the keys.  ~tree-depth steps of ~60 instructions instead of one ~90-instruction
        // step per visited node; the launch ended with its heaviest point (radius 15 px x scale x 1.6: 60+ visited nodes).
        // More than 64 leaves (or levels): the serial walk below.
        bool walked = false;
        if constexpr (LANE_STACK) {
            int node = gl == 0 ? 0 : -1;      // >= 0: node to expand; -1: free lane; -2: this lane has reached its leaf
            double pm = (double)distsq, pd0 = dd0, pd1 = dd1;
            unsigned long long key = 0;
            int lbeg = 0, lcnt = 0;
            int nl = 1;                       // lanes in use (wave-uniform)
            bool fits = true;
            for (int depth = 0;; ++depth) {
                const bool act = node >= 0;
                if (__ballot(act) == 0) break;
                if (depth >= 64) { fits = false; break; }
                const int nsafe = act ? node : 0;
                const uint2* np = reinterpret_cast<const uint2*>(IN_LDS ? s_nodes + nsafe : f.nodes + nsafe);
                uint2 w0 = np[0], w1 = np[1], w2 = np[2];
                asm volatile("" : "+v"(w0.x), "+v"(w0.y), "+v"(w1.x), "+v"(w1.y), "+v"(w2.x), "+v"(w2.y));
                const float divlow = __uint_as_float(w0.x), divhigh = __uint_as_float(w0.y);
                const int left = (int)w1.x, right = (int)w1.y;
                const int col = (int)(w2.y >> 16);
                const bool isleaf = left < 0;
                if (act && isleaf) { lbeg = (int)w2.x; lcnt = (int)(w2.y & 0xFFFFu); node = -2; }
                const bool inner = act && !isleaf;
                const double val = col == 0 ? px : py;
                const double diff1 = val - divlow, diff2 = val - divhigh;
                const bool go_left = diff1 + diff2 < 0;
                const double cut = go_left ? diff2 * diff2 : diff1 * diff1;
                const float dst = (float)(col == 0 ? pd0 : pd1);
                const double m2 = pm + cut - dst;
                const bool wantB = inner && (m2 * 1.0 <= worst);
                const unsigned long long mb = __ballot(wantB);
                const int cntB = __popcll(mb);
                if (nl + cntB > kGroup) { fits = false; break; }
                if (cntB) {
                    int src = gl, k = 0;      // receiving lane nl + k pulls from the k-th lane that hands a child over
                    for (unsigned long long t = mb; t; t &= t - 1, ++k) { const int b = __builtin_ctzll(t); src = gl == nl + k ? b : src; }
                    const int bnode = go_left ? right : left;
                    const double bd0 = col == 0 ? cut : pd0, bd1 = col == 0 ? pd1 : cut;
                    const unsigned long long bkey = key | (1ull << (63 - depth));
                    const int sa = src << 2;
                    auto pull64 = [&](unsigned long long v) {
                        const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(sa, (int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_ds_bpermute(sa, (int)(unsigned)(v >> 32));
                        return ((unsigned long long)hi << 32) | lo;
                    };
                    const int r_node = __builtin_amdgcn_ds_bpermute(sa, bnode);
                    const double r_m = __longlong_as_double((long long)pull64((unsigned long long)__double_as_longlong(m2)));
                    const double r_d0 = __longlong_as_double((long long)pull64((unsigned long long)__double_as_longlong(bd0)));
                    const double r_d1 = __longlong_as_double((long long)pull64((unsigned long long)__double_as_longlong(bd1)));
                    const unsigned long long r_key = pull64(bkey);
                    if (gl >= nl && gl < nl + cntB) { node = r_node; pm = r_m; pd0 = r_d0; pd1 = r_d1; key = r_key; }
                    nl += cntB;
                }
                if (inner) node = go_left ? left : right;   // the best child: same mindistsq, same dists, same key
                ++n_iter;
            }
            if (fits) {
                walked = true;
                n_leaf = nl;
                // every used lane holds one leaf.  Its slots' place in the depth-first order: the leaf counts of all leaves with a smaller key
                int off = 0, total = 0;
                for (int j = 0; j < nl; j++) {
                    const unsigned long long kj = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key >> 32), j) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, j);
                    const int cj = __builtin_amdgcn_readlane(lcnt, j);
                    off += kj < key ? cj : 0;
                    total += cj;
                }
                for (int s0 = 0; s0 < total; s0 += kGroup) {
                    const int sidx = s0 + gl;
                    int kp = -1;
                    for (int j = 0; j < nl; j++) {
                        const int oj = __builtin_amdgcn_readlane(off, j), cj = __builtin_amdgcn_readlane(lcnt, j), bj = __builtin_amdgcn_readlane(lbeg, j);
                        kp = (sidx >= oj && sidx < oj + cj) ? bj + (sidx - oj) : kp;
                    }
                    bool hit = false;
                    unsigned int id = 0;
                    int oc = 0;
                    if (kp >= 0) {
                        const float4 c = IN_LDS ? s_rec[kp] : f.leaf_rec[kp];
                        const unsigned io = __float_as_uint(c.z);
                        id = io >> 4; oc = (int)(io & 15u);
                        const double dx = px - c.x;
                        double sqd = dx * dx;
                        if (!(sqd > worst)) { const double dy = py - c.y; sqd += dy * dy; }
                        hit = sqd < worst && oc >= oct_lo && oc <= predicted;
                    }
                    const unsigned long long hm = __ballot(hit);
                    if (hit) s_cand[ncand + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hm, 0u))] = (id << 4) | (unsigned int)oc;
                    ncand += __popcll(hm);
                    if (ncand > kCandCap - kGroup) { drain(ncand); ncand = 0; }
                }
            }
        }
        int sp = 0;
        int l_rec = 0; double l_m = 0, l_c = 0; float l_d = 0;   // LANE_STACK: this lane's walk record (lane = stack slot)
        int cur = walked ? -1 : 0;   // node to visit (-1: take the top record; walked: nothing left to do)
        double cur_m = (double)distsq;
        for (;;) {
            if (walked) break;
            ++n_iter;
            if (cur < 0) {
                if (sp == 0) break;
                const int top = __builtin_amdgcn_readfirstlane(sp) - 1;   // (one point per wave: the stack pointer is wave-uniform)
                const int rec = LANE_STACK ? __builtin_amdgcn_readlane(l_rec, top) : st_rec[sp - 1];
                const int col = (rec >> 1) & 1;
                if (rec & 1) {       // the other child's subtree is done: dists[col] = dst
                    const double dstd = (double)(LANE_STACK ? __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(l_d), top)) : st_d[sp - 1]);
                    if (col == 0) dd0 = dstd; else dd1 = dstd;
                    --sp;
                    continue;
                }
                const double cutv = LANE_STACK ? readlane_f64(l_c, top) : st_c[sp - 1];   // enter the other child: dists[col] = cut
                if (col == 0) dd0 = cutv; else dd1 = cutv;
                cur = rec >> 2;
                cur_m = LANE_STACK ? readlane_f64(l_m, top) : st_m[sp - 1];
                if constexpr (LANE_STACK) { if (gl == top) l_rec = rec | 1; }
                else if (gl == 0) st_rec[sp - 1] = rec | 1;
            }
            // the whole 24-byte node in ONE round trip: three 8-byte reads issued together (left as `nd = s_nodes[cur]` the compiler fetched the
            // fields where they are used — left / right, then the planes, then the column, then the leaf range: four to five dependent LDS
            // round trips per tree step, ~500 of its ~650 clocks)
            KdNodeDev nd;
            {
                const uint2* np = reinterpret_cast<const uint2*>(IN_LDS ? s_nodes + cur : f.nodes + cur);
                uint2 w0 = np[0], w1 = np[1], w2 = np[2];
                asm volatile("" : "+v"(w0.x), "+v"(w0.y), "+v"(w1.x), "+v"(w1.y), "+v"(w2.x), "+v"(w2.y));   // (all six words are needed HERE)
                nd.divlow = __uint_as_float(w0.x); nd.divhigh = __uint_as_float(w0.y);
                nd.left = (int)w1.x; nd.right = (int)w1.y; nd.leaf_begin = (int)w2.x;
                nd.leaf_count = (short)(w2.y & 0xFFFFu); nd.col = (short)(w2.y >> 16);
            }
            if (nd.left < 0) {   // leaf: lane i of the group tests keypoint i; hits are appended in leaf order
                ++n_leaf;
                bool hit = false;
                unsigned int id = 0;
                int oc = 0;
                if (gl < nd.leaf_count) {
                    const float4 c = IN_LDS ? s_rec[nd.leaf_begin + gl] : f.leaf_rec[nd.leaf_begin + gl];
                    const unsigned io = __float_as_uint(c.z);
                    id = io >> 4; oc = (int)(io & 15u);
                    const double dx = px - c.x;
                    double sqd = dx * dx;
                    if (!(sqd > worst)) { const double dy = py - c.y; sqd += dy * dy; }
                    hit = sqd < worst && oc >= oct_lo && oc <= predicted;
                }
                // (only lanes gl < leaf_count <= 10 can hit: the group's hit mask fits 32 bits whatever kGroup is)
                const unsigned int gm = (unsigned int)((__ballot(hit) >> (gw * (kGroup & 63))) & (kGroup >= 32 ? 0xFFFFFFFFull : ((1ull << (kGroup & 31)) - 1ull)));
                if (hit) s_cand[ncand + __popc(gm & ((1u << (gl & 31)) - 1u))] = (id << 4) | (unsigned int)oc;
                ncand += __popc(gm);
                if (ncand > kCandCap - kLeafMax) { drain(ncand); ncand = 0; }
                cur = -1;
                continue;
            }
            const double val = nd.col == 0 ? px : py;
            const double diff1 = val - nd.divlow, diff2 = val - nd.divhigh;
            const bool go_left = diff1 + diff2 < 0;
            const double cut = go_left ? diff2 * diff2 : diff1 * diff1;
            const float dst = (float)(nd.col == 0 ? dd0 : dd1);
            const double m2 = cur_m + cut - dst;
            if (m2 * 1.0 <= worst) {
                if (sp + 1 > levels) { ovf = true; break; }
                const int nrec = ((go_left ? nd.right : nd.left) << 2) | ((int)nd.col << 1);
                if constexpr (LANE_STACK) { if (gl == sp) { l_rec = nrec; l_m = m2; l_c = cut; l_d = dst; } }
                else if (gl == 0) { st_rec[sp] = nrec; st_m[sp] = m2; st_c[sp] = cut; st_d[sp] = dst; }
                sp++;
            }
            cur = go_left ? nd.left : nd.right;   // best child, same mindistsq
        }
        if (clk) { clk[6] = n_iter; clk[7] = n_leaf; }
    }
    if (clk) { clk[2] = __builtin_readcyclecounter(); clk[5] = ncand; }
    if (!ovf) drain(ncand);
    if (clk) clk[3] = __builtin_readcyclecounter();
    if (ovf) { if (gl == 0) __hip_atomic_store(overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); best_kp = -1; }
    if constexpr (PREV) { if (best_kp != -1 && !(best_d < 0.7 * second_d)) best_kp = -1; }
    else if (best_kp != -1 && bestLevel2 == bestLevel && best_d > 0.8 * second_d) best_kp = -1;
    if (live && gl == 0) {   // (write-through: the publishing workgroup may sit on another XCD)
        __hip_atomic_store(mp.best_kp + m, best_kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mp.best_dist + m, (PREV && best_kp < 0) ? 3.402823466e+38f : best_d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (mp.visible) __hip_atomic_store(mp.visible + m, (unsigned char)(vis ? 1 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (mp.pos_out) { mp.pos_out[m] = make_float4(cd.P0, cd.P1, cd.P2, 0.f); mp.aux_out[m] = mp.aux_in[m]; }
    }
    if (clk) clk[4] = __builtin_readcyclecounter();
  }
    if (!pub.ticket) return;
    // ---- hand-over: ticket behind this workgroup's acknowledged stores; the last workgroup publishes
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(pub.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    for (unsigned i = threadIdx.x; i < pub.n8; i += 4 * (unsigned)nthr) {   // four words in flight per lane
        unsigned long long v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) if (i + u * nthr < pub.n8) v[u] = __hip_atomic_load(pub.dev_out + i + u * nthr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int u = 0; u < 4; u++) if (i + u * nthr < pub.n8) __hip_atomic_store(pub.host_out + i + u * nthr, v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (threadIdx.x == 0) {
        const int ov = __hip_atomic_load(overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        reinterpret_cast<unsigned*>(pub.host_done)[2] = (unsigned)ov;      // the status word travels in the header, behind the completion word
        __hip_atomic_store(overflow, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pub.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // every thread: its stores into pinned memory before the word
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(pub.host_done, pub.word, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
