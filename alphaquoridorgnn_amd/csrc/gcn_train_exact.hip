// gcn_train_exact.hip -- train_board_kernel<N>: the exact-f32 form of the fused training step's board launch (option "train_fused" 1;
// every board below 9x9).  The body is gcn_train_exact.hpp's.
#define AQG_TRAIN_TU exact
#include "gcn_train_exact.hpp"

namespace aqg {

// LF = LOSS_PLAIN: the kernel as it has always been, no further argument; any other form takes its value weight as one trailing float
template <int N, int LF = LOSS_PLAIN, class... VW>
__global__ __launch_bounds__(512) void train_board_kernel(const uint8_t* __restrict__ states72, const int64_t* __restrict__ order, int first,
                                                          TrunkParams tp, HeadParams hpm, const float* __restrict__ pi_all,
                                                          const float* __restrict__ z_all, int A, int B, int hrows,
                                                          float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ g_out,
                                                          float* __restrict__ hp, float* __restrict__ hv, float* __restrict__ lg,
                                                          float* __restrict__ pol, float* __restrict__ vp, float* __restrict__ val,
                                                          float* __restrict__ loss, float* __restrict__ dhp, float* __restrict__ dhv,
                                                          float* __restrict__ part_dW3, float* __restrict__ part_dW2,
                                                          float* __restrict__ part_dW1, float* __restrict__ part_db, VW... vw) {
    static_assert(sizeof...(VW) == (LF == LOSS_PLAIN ? 0 : 1), "a value weight with every form but the plain one");
    __shared__ __align__(16) unsigned char smem[F32_BODY_SMEM];
    train_board_f32_body<N, LF>(smem, states72, order, first, tp, hpm, pi_all, z_all, A, B, hrows, h1, h2, g_out, hp, hv, lg, pol, vp, val,
                                loss, dhp, dhv, part_dW3, part_dW2, part_dW1, part_db, vw...);
}

AQG_TRAIN_STAMP_READER(train_stamps_exact)
AQG_TRAIN_DEBUG_SETTER(train_debug_buf_exact)

int launch_train_board_exact(const aqg_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, int first,
                             int B, hipStream_t st, const aqg_loss* lf) {
    TrunkParams tp;
    for (int i = 0; i < 6; ++i) tp.p[i] = t.params[i];
    HeadParams hp;
    for (int i = 0; i < 8; ++i) hp.p[i] = t.params[6 + i];
    float *pdW3 = t.part, *pdW2 = pdW3 + (size_t)B * TH * TH, *pdW1 = pdW2 + (size_t)B * TH * TH, *pdb = pdW1 + (size_t)B * TH * TF;
    return for_board_size(t.board_size, [&](auto n) {
        constexpr int N = decltype(n)::value;
        if (lf && lf->policy_form == 1)
            hipLaunchKernelGGL((train_board_kernel<N, LOSS_CE, float>), dim3(B), dim3(512), 0, st, states72, order, first, tp, hp, pi, z,
                               t.policy_size, B, N * N, t.h1, t.h2, t.g, t.hp, t.hv, t.lg, t.pol, t.vp, t.val, t.loss, t.dhp, t.dhv, pdW3,
                               pdW2, pdW1, pdb, lf->value_weight);
        else if (lf)
            hipLaunchKernelGGL((train_board_kernel<N, LOSS_REF_W, float>), dim3(B), dim3(512), 0, st, states72, order, first, tp, hp, pi, z,
                               t.policy_size, B, N * N, t.h1, t.h2, t.g, t.hp, t.hv, t.lg, t.pol, t.vp, t.val, t.loss, t.dhp, t.dhv, pdW3,
                               pdW2, pdW1, pdb, lf->value_weight);
        else
            hipLaunchKernelGGL(train_board_kernel<N>, dim3(B), dim3(512), 0, st, states72, order, first, tp, hp, pi, z, t.policy_size, B,
                               N * N, t.h1, t.h2, t.g, t.hp, t.hv, t.lg, t.pol, t.vp, t.val, t.loss, t.dhp, t.dhv, pdW3, pdW2, pdW1, pdb);
        return check_launch("training forward/backward kernels");
    });
}

}  // namespace aqg
