// board_featuriser.hip -- board records -> node features, with or without the board's graph (include/aqgnn.h, aqg_gcn_boards_graph):
// the first launch of every forward and training step that is not the fused 9x9 trunk -- the plain small-board path
// (gcn_boards_plain.hip), GraphPolicyValueNetwork of any shape (gcn_boards_general.hip, gcn_train_general.hip) and the CNN
// (cnn_forward.hip, cnn_train.hip).
//
//   boards_prep_kernel<N, ELL>: one thread per tile: x0 [B*V, 6], the six planes of pv_network_cnn.py:88-114 tile by tile, and
//                               with ELL the wall-cut grid under PyG's gcn_norm as ELL rows of 5
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "gcn_packed.hpp"

namespace aqg {

// ELL = false: the node features only (the CNN's input planes, csrc/cnn_forward.hip); ell_idx / ell_w are not touched
template <int N, bool ELL = true>
__global__ __launch_bounds__(256) void boards_prep_kernel(const void* __restrict__ states, int fmt, int B, float* __restrict__ x0,
                                                          int32_t* __restrict__ ell_idx, float* __restrict__ ell_w) {
    constexpr int V = N * N, S = N - 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * V) return;
    const int b = i / V, t = i % V;
    const QState s = load_state(states, fmt, b);
    const int x = t / N, y = t % N;
    const bool slot_ok = x < S && y < S;
    const int slot = x * S + y;
    float* f = x0 + (size_t)i * 6;
    f[0] = (t == s.ppos) ? 1.f : 0.f;
    f[1] = (float)s.pwl;
    f[2] = (t == s.epos) ? 1.f : 0.f;
    f[3] = (float)s.ewl;
    f[4] = (slot_ok && ((s.hw >> slot) & 1)) ? 1.f : 0.f;
    f[5] = (slot_ok && ((s.vw >> slot) & 1)) ? 1.f : 0.f;
    if constexpr (!ELL) return;
    const int ob = tile_open_bits<N>(s.hw, s.vw, t);
    const float di = dinv_of_bits(ob);
    const int nb[4] = {t - N, t + N, t - 1, t + 1};
    ell_idx[(size_t)i * 5] = i;
    ell_w[(size_t)i * 5] = di * di;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const bool open = (ob >> d) & 1;
        ell_idx[(size_t)i * 5 + 1 + d] = open ? b * V + nb[d] : -1;
        ell_w[(size_t)i * 5 + 1 + d] = open ? di * dinv_of_bits(tile_open_bits<N>(s.hw, s.vw, nb[d])) : 0.f;
    }
}

// The board featuriser alone, for the width-generic graph primitives (gcn_general.hip): x0 [B*V,6] node features and the
// normalised adjacency as ELL rows of 5 (self loop first, then the open neighbours; a closed side has index -1, weight 0).
int launch_gcn_boards_graph(int N, const void* states, int fmt, int B, float* x0, int32_t* ell_idx, float* ell_w, hipStream_t st) {
    if (!board_size_supported(N)) return fail("board_size must be 3, 5, 7 or 9");
    if (B <= 0) return 0;
    const int R = B * N * N;
    const dim3 pg((R + 255) / 256), blk(256);
    return for_board_size(N, [&](auto n) {
        hipLaunchKernelGGL(boards_prep_kernel<decltype(n)::value>, pg, blk, 0, st, states, fmt, B, x0, ell_idx, ell_w);
        return check_launch("boards_prep_kernel");
    });
}

// The featuriser's node features alone: x0 [B*V,6], the six planes of pv_network_cnn.py:88-114 tile by tile (the CNN's input).
int launch_gcn_boards_features(int N, const void* states, int fmt, int B, float* x0, hipStream_t st) {
    if (!board_size_supported(N)) return fail("board_size must be 3, 5, 7 or 9");
    if (B <= 0) return 0;
    const int R = B * N * N;
    const dim3 pg((R + 255) / 256), blk(256);
    return for_board_size(N, [&](auto n) {
        hipLaunchKernelGGL((boards_prep_kernel<decltype(n)::value, false>), pg, blk, 0, st, states, fmt, B, x0, nullptr, nullptr);
        return check_launch("boards_prep_kernel");
    });
}

}  // namespace aqg
