// cnn_train.hip -- one optimisation step of the reference's residual CNN (pv_network_cnn.py:20-84, CNNNetwork) as its
// train_network.py:26-107 takes it, on board records (include/aqgnn.h, aqg_cnn_train_step): every BatchNorm2d in train mode.
//
//   prep       train_general_prep_kernel (gcn_train_general.hip): the mean pool's graph pointer (and, with an order, this step's records gathered)
//   forward    featuriser (launch_gcn_boards_features: the six planes of pv_network_cnn.py:88-114 per tile), then per conv l:
//              cnn_im2col_kernel -> col [R, 9 Cin] (column ci * 9 + tap: the module's weight [F, Cin, 3, 3] is the GEMM's [N, K] as
//              PyTorch stores it), gen_linear -> the raw conv output C_l [R, F] (kept), cnn_bn_partial_kernel + cnn_bn_stats_kernel
//              -> the batch mean / inverse std (and the running statistics updated), cnn_bn_apply_kernel -> relu(BN(C_l) (+ residual))
//              (kept); gen_mean_pool, gen_linear x 2 and gen_heads as the inference path
//   loss       train_general_loss_kernel (gcn_train_general.hip): the reference's two loss terms and d loss / d policy, d value
//   heads      gen_heads_backward, gen_linear_grad for the two Linear layers, gen_linear (W [K,N]) for d loss / d pooled
//   trunk      gen_mean_pool_backward (mask = the last block's output > 0), then per conv l = 2 L .. 0: cnn_bn_bwd_partial_kernel +
//              cnn_bn_bwd_reduce_kernel -> dgamma, dbeta, cnn_bn_bwd_dx_kernel -> dC_l; im2col of the conv's input again and
//              gen_linear_grad -> dW_l; gen_linear (W [K,N]) -> dcol and cnn_col2im_kernel -> dX (the 9 taps summed in order, the
//              residual's gradient added, the ReLU mask of the input applied); the stem needs no dX
//   finish     cnn_adam_kernel: torch.optim.Adam over all 3 C + 4 tensors in one launch (the tensor table lives on the device), and
//              the two batch-mean losses
//
// Every channel statistic is a per-board partial over the board's V tiles (f32, tiles in order) merged over the boards in board
// order in f64 -- the forward's (mean, M2) by Chan's update, never E[x^2] - E[x]^2.  No atomics: every sum runs in an order fixed
// by the shape alone, so two runs give bit-identical parameters and running statistics.  No allocation and no host
// synchronisation: the caller owns one workspace of aqg_cnn_train_workspace_floats floats.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"
#include "train_adam.hpp"
#include "train_driver.hpp"

namespace aqg {

namespace {

inline size_t round64(size_t n) { return (n + 63) & ~(size_t)63; }
inline unsigned blocks_of(long long items, int per) { return (unsigned)((items + per - 1) / per); }
inline int conv_cin(int l, int F) { return l == 0 ? 6 : F; }

// col[r][ci * 9 + tap] = X[the tile at offset (tap / 3 - 1, tap % 3 - 1) from tile r][ci], 0 off the board (padding='same')
__global__ __launch_bounds__(256) void cnn_im2col_kernel(int N, int Cin, size_t total, const float* __restrict__ X,
                                                         float* __restrict__ col) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int K9 = 9 * Cin, V = N * N;
    const size_t r = i / K9;
    const int k = (int)(i - r * K9), ci = k / 9, tap = k - 9 * ci;
    const int t = (int)(r % V), y = t / N + tap / 3 - 1, x = t % N + tap % 3 - 1;
    col[i] = (y >= 0 && y < N && x >= 0 && x < N) ? X[(r - t + (size_t)(y * N + x)) * Cin + ci] : 0.f;
}

// out[r][ci] = mask(sum over the 9 taps in order of dcol[the tile r - offset(tap)][ci * 9 + tap] (+ add[r][ci])): the transpose of
// im2col; the result is zeroed where mask[r][ci] <= 0 (the ReLU that produced the conv's input).  out may alias add.
__global__ __launch_bounds__(256) void cnn_col2im_kernel(int N, int Cin, size_t total, const float* __restrict__ dcol, const float* add,
                                                         const float* __restrict__ mask, float* out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int V = N * N;
    const size_t r = i / Cin;
    const int ci = (int)(i - r * Cin), t = (int)(r % V), y0 = t / N, x0 = t % N;
    const size_t rb = r - t;
    float s = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int y = y0 - (tap / 3 - 1), x = x0 - (tap % 3 - 1);
        if (y >= 0 && y < N && x >= 0 && x < N) s += dcol[(rb + (size_t)(y * N + x)) * (9 * Cin) + ci * 9 + tap];
    }
    if (add) s += add[i];
    out[i] = mask[i] > 0.f ? s : 0.f;
}

// per (board b, channel c): the mean of the board's V tiles (summed in order) and M2 = sum (x - mean_b)^2 -> part[b][c], part[B + b][c]
__global__ __launch_bounds__(256) void cnn_bn_partial_kernel(int V, int B, int F, const float* __restrict__ Cr, float* __restrict__ part) {
    const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    if (c >= F) return;
    const float* x = Cr + (size_t)b * V * F + c;
    float s = 0.f;
    for (int r = 0; r < V; ++r) s += x[(size_t)r * F];
    const float m = s / (float)V;
    float m2 = 0.f;
    for (int r = 0; r < V; ++r) { const float d = x[(size_t)r * F] - m; m2 = fmaf(d, d, m2); }
    part[(size_t)b * F + c] = m;
    part[(size_t)(B + b) * F + c] = m2;
}

// per channel: the board partials merged in board order (Chan's update, f64) -> the batch mean and 1 / sqrt(biased var + eps); the
// running statistics become (1 - momentum) old + momentum (mean, unbiased var), as BatchNorm2d's forward in train mode
__global__ __launch_bounds__(256) void cnn_bn_stats_kernel(int V, int B, int F, const float* __restrict__ part, float bn_eps, float momentum,
                                                           float* __restrict__ mean, float* __restrict__ invstd,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= F) return;
    double n = 0.0, mu = 0.0, m2 = 0.0;
    for (int b = 0; b < B; ++b) {
        const double mb = part[(size_t)b * F + c], m2b = part[(size_t)(B + b) * F + c];
        const double nn = n + V, d = mb - mu;
        mu += d * (double)V / nn;
        m2 += m2b + d * d * n * (double)V / nn;
        n = nn;
    }
    mean[c] = (float)mu;
    invstd[c] = (float)(1.0 / sqrt(m2 / n + (double)bn_eps));
    const double mom = momentum;
    running_mean[c] = (float)((1.0 - mom) * (double)running_mean[c] + mom * mu);
    running_var[c] = (float)((1.0 - mom) * (double)running_var[c] + mom * (m2 / (n - 1.0)));
}

// out = relu(gamma (C - mean) invstd + beta (+ res)); out may alias res
__global__ __launch_bounds__(256) void cnn_bn_apply_kernel(int F, size_t total, const float* __restrict__ Cr, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* res, float* out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % F);
    float v = fmaf((Cr[i] - mean[c]) * invstd[c], gamma[c], beta[c]);
    if (res) v += res[i];
    out[i] = fmaxf(v, 0.f);
}

// per (board b, channel c), the tiles in order: sum dy -> part[b][c], sum dy xhat -> part[B + b][c]  (xhat = (C - mean) invstd)
__global__ __launch_bounds__(256) void cnn_bn_bwd_partial_kernel(int V, int B, int F, const float* __restrict__ dy, const float* __restrict__ Cr,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 float* __restrict__ part) {
    const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    if (c >= F) return;
    const size_t o = (size_t)b * V * F + c;
    const float m = mean[c], is = invstd[c];
    float s = 0.f, sx = 0.f;
    for (int r = 0; r < V; ++r) {
        const float g = dy[o + (size_t)r * F];
        s += g;
        sx = fmaf(g, (Cr[o + (size_t)r * F] - m) * is, sx);
    }
    part[(size_t)b * F + c] = s;
    part[(size_t)(B + b) * F + c] = sx;
}

// per channel, the boards in order (f64): dbeta = sum dy, dgamma = sum dy xhat; red[c] = mean dy, red[Fp + c] = mean dy xhat
__global__ __launch_bounds__(256) void cnn_bn_bwd_reduce_kernel(int V, int B, int F, int Fp, const float* __restrict__ part,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                float* __restrict__ red) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= F) return;
    double s = 0.0, sx = 0.0;
    for (int b = 0; b < B; ++b) { s += part[(size_t)b * F + c]; sx += part[(size_t)(B + b) * F + c]; }
    const double n = (double)B * V;
    dbeta[c] = (float)s;
    dgamma[c] = (float)sx;
    red[c] = (float)(s / n);
    red[Fp + c] = (float)(sx / n);
}

// dC = gamma invstd (dy - mean dy - xhat mean(dy xhat))
__global__ __launch_bounds__(256) void cnn_bn_bwd_dx_kernel(int F, int Fp, size_t total, const float* __restrict__ dy,
                                                            const float* __restrict__ Cr, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ red, float* __restrict__ dC) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % F);
    const float is = invstd[c], xhat = (Cr[i] - mean[c]) * is;
    dC[i] = gamma[c] * is * (dy[i] - red[c] - xhat * red[Fp + c]);
}

// The element counts of the tensor order of include/aqgnn.h (aqg_cnn_train): per conv the weight (9 Cin F), gamma (F), beta (F);
// then the heads (A F, A, F, 1).  Element e0 of the concatenation -> (tensor, offset) in closed form.
struct CnnShape { int F, L, A; };

__host__ __device__ inline size_t cnn_param_count(CnnShape s) {
    const size_t F = s.F;
    return 56 * F + (size_t)(2 * s.L) * (9 * F * F + 2 * F) + (size_t)s.A * F + s.A + F + 1;
}

__device__ inline int cnn_tensor_of(CnnShape s, size_t e0, size_t* off) {
    const size_t F = s.F, stem = 56 * F, per = 9 * F * F + 2 * F, convs = stem + (size_t)(2 * s.L) * per;
    if (e0 < convs) {
        int l;
        size_t in, wsz;
        if (e0 < stem) { l = 0; in = e0; wsz = 54 * F; }
        else { const size_t e1 = e0 - stem; l = 1 + (int)(e1 / per); in = e1 - (size_t)(l - 1) * per; wsz = 9 * F * F; }
        if (in < wsz) { *off = in; return 3 * l; }
        if (in < wsz + F) { *off = in - wsz; return 3 * l + 1; }
        *off = in - wsz - F; return 3 * l + 2;
    }
    size_t h = e0 - convs;
    const int hc = 3 * (2 * s.L + 1);
    const size_t AF = (size_t)s.A * F;
    if (h < AF) { *off = h; return hc; }
    h -= AF;
    if (h < (size_t)s.A) { *off = h; return hc + 1; }
    h -= s.A;
    if (h < F) { *off = h; return hc + 2; }
    *off = h - F; return hc + 3;
}

// torch.optim.Adam over every parameter element (train_adam.hpp), the tensor pointers read from the device table
// [params | grads | adam_m | adam_v]; and, in the workgroup after the last element's (when `loss` is set), its loss_means.
struct CnnAdamArgs {
    CnnShape s; int T; unsigned adam_blocks; size_t total;
    float* const* table;
    AdamStep adam;
    int B; LossMeans means;
};

// Two instantiations: <>, the launch as it has always been (the same instructions and registers as before the template), and
// <CnnOptim>, with the optimiser controls of train_adam.hpp as a second argument: every Adam workgroup first adds up the norm's
// partials and derives the clip coefficient -- AFTER the table's pointers are read: hipcc treats a pointer loaded from the table as
// a global one only while nothing that may write memory (the prologue's LDS store and barrier) lies in front of the load.
using CnnOptim = OptimArgs<AQG_CNN_TRAIN_TENSORS>;
template <class... Optim>
__global__ __launch_bounds__(256) void cnn_adam_kernel(CnnAdamArgs a, Optim... op) {
    constexpr bool OPT = sizeof...(Optim) == 1;
    if (blockIdx.x == a.adam_blocks) {
        const LossMeans means = a.means;
        loss_means(means, a.B);
        return;
    }
    const size_t e0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = e0 < a.total;
    if (!OPT && !live) return;                  // (OPT: every thread stays for the prologue's barrier, reading element 0)
    size_t e;
    const int i = cnn_tensor_of(a.s, live ? e0 : 0, &e);
    float* p = a.table[i];
    const float* g = a.table[a.T + i];
    float* m = a.table[2 * a.T + i];
    float* v = a.table[3 * a.T + i];
    float gr = g[e], opar = p[e];
    const float om = m[e], ov = v[e];
    const AdamStep ad = a.adam;                 // (copies, not references into `a`: train_adam.hpp says why)
    if constexpr (OPT) {
        __shared__ float norm_red[4];
        const OptimStep os = (op.s, ...);
        const float coef = optim_prologue(os, norm_red);
        if (!live) return;
        const GradParam gp = optim_apply(coef, (op.wd[i], ...), os.decoupled, ad.lr, gr, opar);
        gr = gp.g; opar = gp.p;
    }
    const AdamMoments n = adam_moments(ad, gr, om, ov);
    m[e] = n.m; v[e] = n.v;
    p[e] = adam_param(ad, opar, n);
}

struct CnnTrainWorkspace {
    uint8_t* states; int32_t* gptr; float* x0; float* conv; float* out; size_t rf;
    float* mean; float* invstd; size_t fp;
    float* bnpart; float* bnred; float* col; float* g[3];
    float* pooled; float* logits; float* vpre; float* policy; float* value; float* loss; float* loss_mean;
    float* dpol; float* dval; float* dlogits; float* dvpre; float* dpooled;
    float* part; size_t part_floats;
};

// the partial tiles of the largest gen_linear_grad of a step with up to B positions (closed-form bounds, monotone in B)
inline size_t part_floats(int N, int F, int L, int A, int B) {
    const long long R = (long long)B * N * N;
    size_t m = 0;
    const size_t c[4] = {gen_linear_grad_workspace_floats_bound(B, A, F), gen_linear_grad_workspace_floats_bound(B, 1, F),
                         gen_linear_grad_workspace_floats_bound(R, F, 54),
                         L > 0 ? gen_linear_grad_workspace_floats_bound(R, F, 9 * F) : 0};
    for (size_t x : c) m = x > m ? x : m;
    return m;
}

// floats of each region, every one rounded up to 64 (256 bytes); every region grows with B, so max_batch's layout serves every
// smaller batch
inline size_t cnn_train_layout(int N, int F, int L, int A, int B, CnnTrainWorkspace* ws, float* base) {
    const size_t R = (size_t)B * N * N, C = 2 * L + 1, RF = round64(R * F), Fp = round64(F);
    const size_t K9 = (size_t)(9 * F > 54 ? 9 * F : 54);
    const size_t sz[23] = {(size_t)B * 18, (size_t)B + 1, R * 6, RF * C, RF * C, Fp * C, Fp * C, (size_t)2 * B * F, 2 * Fp,
                           R * K9, R * F, R * F, R * F,
                           (size_t)B * F, (size_t)B * A, (size_t)B, (size_t)B * A, (size_t)B, (size_t)2 * B, 2,
                           (size_t)B * A, (size_t)B, part_floats(N, F, L, A, B)};
    const size_t sz2[3] = {(size_t)B * A, (size_t)B, (size_t)B * F};      // dlogits, dvpre, dpooled
    size_t off[26], total = 0;
    for (int i = 0; i < 23; ++i) { off[i] = total; total += round64(sz[i]); }
    for (int i = 0; i < 3; ++i) { off[23 + i] = total; total += round64(sz2[i]); }
    if (ws && base) {
        ws->states = reinterpret_cast<uint8_t*>(base + off[0]); ws->gptr = reinterpret_cast<int32_t*>(base + off[1]);
        ws->x0 = base + off[2]; ws->conv = base + off[3]; ws->out = base + off[4]; ws->rf = RF;
        ws->mean = base + off[5]; ws->invstd = base + off[6]; ws->fp = Fp;
        ws->bnpart = base + off[7]; ws->bnred = base + off[8]; ws->col = base + off[9];
        ws->g[0] = base + off[10]; ws->g[1] = base + off[11]; ws->g[2] = base + off[12];
        ws->pooled = base + off[13]; ws->logits = base + off[14]; ws->vpre = base + off[15]; ws->policy = base + off[16];
        ws->value = base + off[17]; ws->loss = base + off[18]; ws->loss_mean = base + off[19]; ws->dpol = base + off[20];
        ws->dval = base + off[21]; ws->part = base + off[22]; ws->part_floats = sz[22];
        ws->dlogits = base + off[23]; ws->dvpre = base + off[24]; ws->dpooled = base + off[25];
    }
    return total;
}

int launch_im2col(int N, int B, int Cin, const float* X, float* col, hipStream_t st) {
    const size_t total = (size_t)B * N * N * 9 * Cin;
    hipLaunchKernelGGL(cnn_im2col_kernel, dim3(blocks_of((long long)total, 256)), dim3(256), 0, st, N, Cin, total, X, col);
    return check_launch("cnn_im2col_kernel");
}

// forward, losses and backward of B positions (rows order[first ..] or first ..): gradients into t.grads, the running statistics
// updated, per-position losses
int forward_backward(const aqg_cnn_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order, int first,
                     int B, const CnnTrainWorkspace& ws, float* policy, float* value, float* loss, hipStream_t st, const aqg_loss* lf) {
    const int N = t.board_size, V = N * N, F = t.num_filters, L = t.num_blocks, A = t.policy_size, C = 2 * L + 1;
    const int R = B * V, Fp = (int)ws.fp;
    const size_t RFn = (size_t)R * F;
    float* const* p = t.params;
    float* const* g = t.grads;
    const unsigned fblk = blocks_of(F, 256), eblk = blocks_of((long long)RFn, 256);
    if (int r = launch_train_general_prep(V, B, states72, order, first, ws.gptr, ws.states, st)) return r;
    const uint8_t* recs = order ? ws.states : states72 + (size_t)first * 72;
    if (int r = launch_gcn_boards_features(N, recs, 0, B, ws.x0, st)) return r;
    // conv l reads in(l) and writes C_l = conv(l), out(l) = relu(BN(C_l) (+ out(l - 2) for the second conv of a block))
    auto conv = [&](int l) { return ws.conv + (size_t)l * ws.rf; };
    auto out = [&](int l) { return ws.out + (size_t)l * ws.rf; };
    auto in = [&](int l) -> const float* { return l == 0 ? ws.x0 : out(l - 1); };
    for (int l = 0; l < C; ++l) {
        const int cin = conv_cin(l, F);
        float* mean = ws.mean + (size_t)l * Fp;
        float* invstd = ws.invstd + (size_t)l * Fp;
        if (int r = launch_im2col(N, B, cin, in(l), ws.col, st)) return r;
        if (int r = launch_gen_linear(R, 9 * cin, F, ws.col, p[3 * l], nullptr, nullptr, 0, conv(l), st)) return r;
        hipLaunchKernelGGL(cnn_bn_partial_kernel, dim3(B, fblk), dim3(256), 0, st, V, B, F, conv(l), ws.bnpart);
        hipLaunchKernelGGL(cnn_bn_stats_kernel, dim3(fblk), dim3(256), 0, st, V, B, F, ws.bnpart, t.bn_eps[l], t.bn_momentum[l], mean,
                           invstd, t.running_mean[l], t.running_var[l]);
        const float* res = (l > 0 && !(l & 1)) ? out(l - 2) : nullptr;
        hipLaunchKernelGGL(cnn_bn_apply_kernel, dim3(eblk), dim3(256), 0, st, F, RFn, conv(l), mean, invstd, p[3 * l + 1], p[3 * l + 2],
                           res, out(l));
        if (int r = check_launch("cnn_bn kernels")) return r;
    }
    // pool and heads (pv_network_cnn.py:68-78)
    const int h = 3 * C;
    if (int r = launch_gen_mean_pool(F, out(C - 1), ws.gptr, B, ws.pooled, st)) return r;
    if (int r = launch_gen_linear(B, F, A, ws.pooled, p[h], p[h + 1], nullptr, 0, ws.logits, st)) return r;
    if (int r = launch_gen_linear(B, F, 1, ws.pooled, p[h + 2], p[h + 3], nullptr, 0, ws.vpre, st)) return r;
    if (int r = launch_gen_heads(B, A, ws.logits, ws.vpre, policy, value, st, nullptr)) return r;
    // losses, the heads' backward and d loss / d pooled
    if (int r = launch_train_losses(B, A, ws.logits, policy, value, pi, z, order, first, lf, loss, ws.dpol, ws.dval, ws.dlogits,
                                    ws.dvpre, st))
        return r;
    float* part = ws.part;
    const size_t pf = ws.part_floats;
    if (int r = launch_gen_linear_grad(B, F, A, ws.dlogits, ws.pooled, nullptr, part, pf, g[h], g[h + 1], st)) return r;
    if (int r = launch_gen_linear_grad(B, F, 1, ws.dvpre, ws.pooled, nullptr, part, pf, g[h + 2], g[h + 3], st)) return r;
    if (int r = launch_gen_linear(B, A, F, ws.dlogits, p[h], nullptr, nullptr, AQG_LIN_W_KN, ws.dpooled, st)) return r;
    if (int r = launch_gen_linear(B, 1, F, ws.dvpre, p[h + 2], nullptr, nullptr, AQG_LIN_W_KN | AQG_LIN_ACCUMULATE, ws.dpooled, st))
        return r;
    // trunk.  dS = d loss / d (the last conv's BN output + residual), i.e. after the ReLU mask of out(C - 1)
    float* dS = ws.g[0];
    float* dT = ws.g[1];
    float* dC = ws.g[2];
    if (int r = launch_gen_mean_pool_backward(R, F, ws.dpooled, ws.gptr, B, out(C - 1), dS, st)) return r;
    for (int l = C - 1; l >= 0; --l) {
        // d loss / d (conv l's BN output): dS for the second conv of a block and the stem, dT for the first conv of a block
        const float* dy = (l & 1) ? dT : dS;
        const int cin = conv_cin(l, F);
        const float* mean = ws.mean + (size_t)l * Fp;
        const float* invstd = ws.invstd + (size_t)l * Fp;
        hipLaunchKernelGGL(cnn_bn_bwd_partial_kernel, dim3(B, fblk), dim3(256), 0, st, V, B, F, dy, conv(l), mean, invstd, ws.bnpart);
        hipLaunchKernelGGL(cnn_bn_bwd_reduce_kernel, dim3(fblk), dim3(256), 0, st, V, B, F, Fp, ws.bnpart, g[3 * l + 1], g[3 * l + 2],
                           ws.bnred);
        hipLaunchKernelGGL(cnn_bn_bwd_dx_kernel, dim3(eblk), dim3(256), 0, st, F, Fp, RFn, dy, conv(l), mean, invstd, p[3 * l + 1],
                           ws.bnred, dC);
        if (int r = check_launch("cnn_bn backward kernels")) return r;
        if (int r = launch_im2col(N, B, cin, in(l), ws.col, st)) return r;
        if (int r = launch_gen_linear_grad(R, 9 * cin, F, dC, ws.col, nullptr, part, pf, g[3 * l], nullptr, st)) return r;
        if (l == 0) break;                         // the stem needs no dX
        if (int r = launch_gen_linear(R, F, 9 * cin, dC, p[3 * l], nullptr, nullptr, AQG_LIN_W_KN, ws.col, st)) return r;
        // conv l's input is out(l - 1): for the second conv of a block the block's first ReLU (-> dT); for the first conv the previous
        // block's (or the stem's) output, which also feeds the residual of conv l + 1 (-> dS, the residual's gradient added)
        const size_t total = RFn;
        if (l & 1)
            hipLaunchKernelGGL(cnn_col2im_kernel, dim3(eblk), dim3(256), 0, st, N, F, total, ws.col, dS, out(l - 1), dS);
        else
            hipLaunchKernelGGL(cnn_col2im_kernel, dim3(eblk), dim3(256), 0, st, N, F, total, ws.col, nullptr, out(l - 1), dT);
        if (int r = check_launch("cnn_col2im_kernel")) return r;
    }
    return 0;
}

int launch_finish(const aqg_cnn_train& t, int B, bool update, int step, const float* loss, float* loss_mean, float* loss_sums,
                  hipStream_t st, const OptimLaunch* ol = nullptr) {
    CnnAdamArgs a{};
    a.s = CnnShape{t.num_filters, t.num_blocks, t.policy_size};
    a.T = 3 * (2 * t.num_blocks + 1) + 4;
    a.total = cnn_param_count(a.s);
    a.table = t.adam_table;
    a.adam = adam_step(t.lr, t.beta1, t.beta2, t.eps, step);
    a.B = B; a.means = LossMeans{loss, loss_mean, loss_sums};
    a.adam_blocks = update ? blocks_of((long long)a.total, 256) : 0u;
    const unsigned grid = a.adam_blocks + (loss && B > 0 ? 1u : 0u);
    if (grid == 0) return 0;
    if (ol && update) {
        CnnOptim op{};
        fill_optim(*ol, a.T, &op.s, op.wd);
        hipLaunchKernelGGL(cnn_adam_kernel<CnnOptim>, dim3(grid), dim3(256), 0, st, a, op);
        return check_launch("cnn_adam_kernel<CnnOptim>");
    }
    hipLaunchKernelGGL(cnn_adam_kernel<>, dim3(grid), dim3(256), 0, st, a);
    return check_launch("cnn_adam_kernel");
}

bool shape_ok(int N, int F, int L, int A) {
    return board_size_supported(N) && F >= 1 && F <= AQG_CNN_MAX_FILTERS && L >= 0 && L <= AQG_CNN_MAX_BLOCKS &&
           A == N * N + 2 * (N - 1) * (N - 1);
}

}  // namespace

// elements of each of the 3 C + 4 tensors, in parameter order (what cnn_tensor_of walks on the device)
void cnn_train_tensor_sizes(const aqg_cnn_train& t, size_t* numel) {
    const size_t F = t.num_filters, A = t.policy_size;
    const int C = 2 * t.num_blocks + 1;
    for (int l = 0; l < C; ++l) { numel[3 * l] = (l == 0 ? 54 : 9 * F) * F; numel[3 * l + 1] = F; numel[3 * l + 2] = F; }
    numel[3 * C] = A * F; numel[3 * C + 1] = A; numel[3 * C + 2] = F; numel[3 * C + 3] = 1;
}

size_t cnn_train_workspace_floats(int N, int F, int L, int A, int max_batch) {
    if (!shape_ok(N, F, L, A) || max_batch < 1) return 0;
    return cnn_train_layout(N, F, L, A, max_batch, nullptr, nullptr);
}

// the host-side checks of both entry points (include/aqgnn.h aqg_cnn_train): shape, tensors, BatchNorm settings, Adam table
int check_cnn_train(const aqg_cnn_train& t, bool adam, const char* what) {
    if (!board_size_supported(t.board_size)) return fail(what, "board_size must be 3, 5, 7 or 9");
    if (t.num_filters < 1 || t.num_filters > AQG_CNN_MAX_FILTERS) return fail(what, "num_filters must be 1..512");
    if (t.num_blocks < 0 || t.num_blocks > AQG_CNN_MAX_BLOCKS) return fail(what, "num_blocks must be 0..40");
    if (!shape_ok(t.board_size, t.num_filters, t.num_blocks, t.policy_size))
        return fail(what, "policy_size must be N*N + 2*(N-1)^2 of the board");
    const int C = 2 * t.num_blocks + 1, T = 3 * C + 4;
    for (int i = 0; i < T; ++i)
        if (!t.params[i] || !t.grads[i]) return fail(what, "null parameter tensor");
    for (int l = 0; l < C; ++l) {
        if (!t.running_mean[l] || !t.running_var[l]) return fail(what, "null running statistics");
        if (!(t.bn_eps[l] > 0.f) || !(t.bn_momentum[l] >= 0.f && t.bn_momentum[l] <= 1.f))
            return fail(what, "bn_eps must be > 0 and bn_momentum in [0, 1]");
    }
    if (adam && !t.adam_table) return fail(what, "adam_table is NULL");
    if (adam && t.step < 1) return fail(what, "step must be >= 1");
    return 0;
}

// the residual CNN as a kind of train_driver.hpp; check_cnn_train, called by capi.hip, has validated t
struct CnnKind {
    using Workspace = CnnTrainWorkspace;
    static constexpr const char *step_name = "aqg_cnn_train_step", *steps_name = "aqg_cnn_train_steps";
    static constexpr const char* workspace_refusal = "workspace too small (aqg_cnn_train_workspace_floats)";
    static constexpr bool empty_batch_mode1_updates = false;    // batch 0: a no-op unless mode is 2
    static constexpr auto forward_backward = aqg::forward_backward;
    static constexpr auto launch_finish = aqg::launch_finish;
    static int validate(const aqg_cnn_train&, const char*) { return 0; }
    static size_t layout(const aqg_cnn_train& t, int B, CnnTrainWorkspace* ws) {
        return cnn_train_layout(t.board_size, t.num_filters, t.num_blocks, t.policy_size, B, ws, ws ? t.workspace : nullptr);
    }
};

int cnn_train_step(const aqg_cnn_train& t, const uint8_t* states72, const float* pi, const float* z, int mode, hipStream_t st,
                   const OptimPlan* plan, const aqg_weight_average* avg, const aqg_loss* lf) {
    return train_driver_step<CnnKind>(t, states72, pi, z, mode, st, plan, avg, lf);
}
int cnn_train_steps(const aqg_cnn_train& t, const uint8_t* states72, const float* pi, const float* z, const int64_t* order,
                    long long positions, float* loss_sums, hipStream_t st, const OptimPlan* plan,
                    const aqg_weight_average* avg, const aqg_loss* lf) {
    return train_driver_steps<CnnKind>(t, states72, pi, z, order, positions, loss_sums, st, plan, avg, lf);
}

}  // namespace aqg
