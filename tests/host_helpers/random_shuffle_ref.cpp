// The sample sequence of PnPSolver::solvePnPRansac drawn by the REAL std::random_shuffle (removed in C++17: build with -std=c++14):
// one index vector, shuffled once per iteration, its first four entries taken.  tests/test_pnp_ransac_host.py compares
// uh_pnp_ransac_samples with this after the same srand.
#include <algorithm>
#include <cstdlib>
#include <vector>

extern "C" int ref_shuffle_samples(unsigned seed, int n, int iters, int* samples_out, int* next_rand) {
    std::srand(seed);
    std::vector<int> indices((size_t)n);
    for (size_t i = 0; i < indices.size(); i++) indices[i] = (int)i;
    for (int it = 0; it < iters; it++) {
        std::random_shuffle(indices.begin(), indices.end());
        for (int j = 0; j < 4; j++) samples_out[4 * it + j] = indices[j];
    }
    *next_rand = std::rand();
    return 0;
}
