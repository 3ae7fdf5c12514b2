// Host statement of "a k-ordered fmaf chain" (include/aqgnn.h, width-generic graph primitives): what aqg_graph_linear is said to
// compute, in single precision with std::fmaf -- one rounding per term, k from 0 upwards, the bias added last.  Test infrastructure:
// built by tests/test_graph_primitives_cpu.py (fmaf_chain()) the way tests/_util.py builds hostcheck.cpp.
#include <cmath>
#include <cstddef>

extern "C" {

// Y[m][n] = fmaf(X[m][K-1], w(K-1, n), ... fmaf(X[m][0], w(0, n), 0) ...) (+ bias[n]);  w(k, n) = W[n][k], or W[k][n] with w_kn.
int fc_linear(int M, int K, int N, const float* X, const float* W, const float* bias, int w_kn, float* Y) {
    if (M < 0 || K < 0 || N < 0) return 1;
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) {
            float acc = 0.f;
            for (int k = 0; k < K; ++k) {
                const float w = w_kn ? W[(size_t)k * N + n] : W[(size_t)n * K + k];
                acc = std::fmaf(X[(size_t)m * K + k], w, acc);
            }
            Y[(size_t)m * N + n] = bias ? acc + bias[n] : acc;
        }
    return 0;
}

}  // extern "C"
