// Host build of csrc/mapinit_math.hpp for tests/test_mapinit_host.py: the pieces of the arithmetic one at a time, as the device compiles them.
#include "../../ucoslam-cv3_amd/csrc/mapinit_math.hpp"

extern "C" {

// the null vector of an M x 9 float system (M = 16 or 8), in double
void mi_null_vector(const float* A, int M, double* x9) {
    double W[mim::kWsRowsH * 9];
    for (int k = 0; k < 9 * M; k++) W[k] = A[k];
    mim::null_vector9(W, M, 0, 1, x9);
}
void mi_svd3(const float* A, double* U, double* w, double* V) { mim::svd3(A, U, w, V); }
void mi_rank2(const float* Fpre, float* Fn) { mim::rank2(Fpre, Fn); }
void mi_inv3(const float* m, float* o) { mim::inv3(m, o); }
float mi_det3(const float* m) { return mim::det3f(m); }
void mi_normalise(const float* xy, int n, float* mean_scale4, float* T9) {
    mim::Norm N;
    mim::normalise(xy, n, N);
    mean_scale4[0] = N.mx; mean_scale4[1] = N.my; mean_scale4[2] = N.sx; mean_scale4[3] = N.sy;
    for (int k = 0; k < 9; k++) T9[k] = N.T[k];
}
// R (8 x 9) and t (8 x 3) of the candidates of a model matrix; returns their number
int mi_decompose(int model, const float* M, const float* intr4, float* R, float* t) {
    mim::Candidates C;
    float d3[3];
    if (model == mim::kHomography) mim::decompose_h(M, intr4, C, d3);
    else mim::decompose_f(M, intr4, C);
    for (int c = 0; c < C.n; c++) {
        for (int k = 0; k < 9; k++) R[9 * c + k] = C.R[c][k];
        for (int k = 0; k < 3; k++) t[3 * c + k] = C.t[c][k];
    }
    return C.n;
}
// CheckRT's body for one match: state, cosine, point
int mi_check_rt(const float* intr4, const float* R, const float* t, float th2, const float* xy4, float* cosp, float* p3) {
    mim::RtConst Q;
    mim::make_rt_const(intr4, R, t, th2, Q);
    return mim::check_rt(Q, xy4[0], xy4[1], xy4[2], xy4[3], *cosp, p3);
}

// the decision rules of ReconstructF / ReconstructH on given counts and parallaxes: returns ok, writes the winner
int mi_decide(int model, int n_cand, int N, const int* n_good, const float* parallax, float min_parallax, int min_triangulated, int* winner) {
    return mim::decide(model, n_cand, N, n_good, parallax, min_parallax, min_triangulated, *winner) ? 1 : 0;
}

}  // extern "C"
