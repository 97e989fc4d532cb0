// Host build of csrc/newpoints_math.hpp (the per-match arithmetic of newpoints.hip, one text for device and host): lets a CPU test
// run the kernel's Jacobi with any sweep count against the numpy oracle.  g++ -O2 -ffp-contract=off -shared -fPIC.
#include "../../ucoslam-cv3_amd/csrc/newpoints_math.hpp"

extern "C" {

int np_host_default_sweeps() { return npm::kJacobiSweeps; }

// frame17: fx fy cx cy | T (12) | c1 (3) ... see the packing below; pair: RT (16) intr4 (4) centre (3)
void np_host_triangulate(const float* intr1, const float* T12, const float* c1, float max_chi2, float ratio_factor, const float* sf1, const float* RT,
                         const float* intr2, const float* c2, const float* sf2, int n, const float* pt1, const int* oct1, const float* pt2,
                         const int* oct2, int sweeps, float* cam, float* glob, unsigned char* status) {
    npm::FrameConst F;
    F.fx1 = intr1[0]; F.fy1 = intr1[1]; F.cx1 = intr1[2]; F.cy1 = intr1[3];
    F.invfx1 = 1.f / F.fx1; F.invfy1 = 1.f / F.fy1;
    for (int k = 0; k < 12; k++) F.T[k] = T12[k];
    for (int k = 0; k < 3; k++) F.c1[k] = c1[k];
    F.max_chi2 = max_chi2; F.ratio_factor = ratio_factor;
    npm::PairConst Q;
    npm::make_pair_const(RT, intr2, c2, Q);
    for (int i = 0; i < n; i++) {
        npm::MatchOut o;
        const float s1 = sf1[oct1[i]], s2 = sf2[oct2[i]];
        npm::triangulate_match(F, Q, pt1[2 * i], pt1[2 * i + 1], pt2[2 * i], pt2[2 * i + 1], 1.f / (s1 * s1), 1.f / (s2 * s2), s1, s2, sweeps, o);
        for (int k = 0; k < 3; k++) { cam[3 * i + k] = o.cam[k]; glob[3 * i + k] = o.glob[k]; }
        status[i] = o.status;
    }
}

}
