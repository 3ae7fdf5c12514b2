// cnn_forward.hip -- the reference's residual CNN (pv_network_cnn.py:20-84, CNNNetwork) in eval mode on board records or on
// [B,6,N,N] planes (include/aqgnn.h, aqg_cnn_*): the forward the engine's prior_mode 4 enqueues per simulation.
//
//   featuriser   boards_prep_kernel<N, false> (board_featuriser.hip): x0 [B*V, 6], the six planes of pv_network_cnn.py:88-114 per tile
//                (or, from planes, cnn_planes_kernel: the NCHW input read into the same tile-major rows)
//   2 L + 1 convs  cnn_conv_kernel: relu(conv3x3(x) * scale + shift (+ residual)), one launch per conv, eval-mode BatchNorm2d
//                folded into the per-channel scale / shift at pack time; the last conv writes AdaptiveAvgPool2d(1) instead
//   heads        gen_linear x 2 and gen_heads (gcn_general.hip): Linear -> Softmax, Linear -> Tanh straight off the pool
//
// The conv is an implicit GEMM on the f32-input matrix pipe (v_mfma_f32_16x16x4_f32: exact f32 products, a k-ordered fmaf chain):
// rows = the board's V tiles (padded to 16-row tiles), columns = 64 output channels per workgroup, K = 9 taps x the input channels
// in slabs of 32.  No atomics; every sum runs in an order fixed by the shape alone, and every board is computed by workgroups of its
// own, so a board's outputs are bit-identical at any batch size, position in the batch and `active` mask.
#include "aqg_common.hpp"
#include "../../include/aqgnn.h"
#include "launchers.hpp"

#include <cmath>

namespace aqg {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int KS = 32;                    // input channels per K slab
constexpr int WSLAB = 9 * (KS / 4) * 64 * 4;   // floats of one packed weight slab: [tap 9][k/4 8][n 64][k%4 4]
constexpr int YS = 68;                    // LDS row stride of the epilogue tile: an MFMA result's 4 rows x 16 columns on 64 banks

inline size_t round64(size_t n) { return (n + 63) & ~(size_t)63; }

// ------------------------------------------------------------------------------------------- packed layout
// Per conv l (0 = the stem, then conv_bn1 / conv_bn2 of each residual block): the weights as [nt][ks][9][8][64][4] (nt = 64-column
// tiles of the output channels, ks = 32-channel slabs of the input, zero past Cout / Cin) -- one slab is the contiguous block a
// workgroup copies into LDS as it is -- then scale [Fp] and shift [Fp] (Fp = filters rounded up to 64, zero past it).  Then the
// heads as PyTorch stores them: policy weight [A,F], bias [A], value weight [1,F], bias [1].  Every region starts on 64 floats.
struct CnnLayout {
    size_t conv_w[2 * AQG_CNN_MAX_BLOCKS + 1], scale[2 * AQG_CNN_MAX_BLOCKS + 1], shift[2 * AQG_CNN_MAX_BLOCKS + 1];
    size_t pw, pb, vw, vb, total;
};

__host__ __device__ inline int conv_cin(int l, int F) { return l == 0 ? 6 : F; }
__host__ __device__ inline int slabs_of(int C) { return (C + KS - 1) / KS; }
__host__ __device__ inline int tiles_of(int F) { return (F + 63) / 64; }

inline void cnn_layout(int F, int L, int A, CnnLayout* o) {
    const int nt = tiles_of(F);
    const size_t Fp = (size_t)nt * 64;
    size_t off = 0;
    for (int l = 0; l < 2 * L + 1; ++l) {
        o->conv_w[l] = off; off += (size_t)nt * slabs_of(conv_cin(l, F)) * WSLAB;
        o->scale[l] = off; off += Fp;
        o->shift[l] = off; off += Fp;
    }
    o->pw = off; off += round64((size_t)A * F);
    o->pb = off; off += round64(A);
    o->vw = off; off += round64(F);
    o->vb = off; off += 64;
    o->total = off;
}

// conv weight [Cout][Cin][3][3] -> the packed slabs of this conv (every element written, zeros included)
__global__ __launch_bounds__(256) void cnn_pack_conv_kernel(int Cin, int Cout, int ks, size_t n_out, const float* __restrict__ W,
                                                           float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int e = (int)(i % WSLAB);
    const size_t slab = i / WSLAB;
    const int s = (int)(slab % ks), tile = (int)(slab / ks);
    const int j = e & 3, n = (e >> 2) & 63, kq = (e >> 8) & 7, tap = e >> 11;
    const int k = KS * s + 4 * kq + j, co = 64 * tile + n;
    out[i] = (co < Cout && k < Cin) ? W[((size_t)co * Cin + k) * 9 + tap] : 0.f;
}

// eval-mode BatchNorm2d folded: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale (f64, rounded once)
__global__ __launch_bounds__(256) void cnn_pack_bn_kernel(int F, int Fp, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                         float* __restrict__ scale, float* __restrict__ shift) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Fp) return;
    if (n >= F) { scale[n] = 0.f; shift[n] = 0.f; return; }
    const double sc = (double)gamma[n] / sqrt((double)var[n] + (double)eps);
    scale[n] = (float)sc;
    shift[n] = (float)((double)beta[n] - (double)mean[n] * sc);
}

// [B,6,N,N] planes -> x0 [B*V,6] (the featuriser's layout)
__global__ __launch_bounds__(256) void cnn_planes_kernel(const float* __restrict__ planes, int V, size_t R, float* __restrict__ x0) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * 6) return;
    const size_t r = i / 6;
    const int f = (int)(i % 6);
    const size_t b = r / V;
    const int t = (int)(r % V);
    x0[i] = planes[(b * 6 + f) * V + t];
}

// ------------------------------------------------------------------------------------------- conv 3x3 "same" + BN + residual + ReLU
// One workgroup (4 waves) per (board b, 64 output channels n0 ..).  Per K slab of 32 input channels the board's tiles go into the
// interior of a zero-haloed (N+2)^2 grid in LDS (layout [k/4][grid position][k%4]) and the slab's packed weights ([9][8][64][4])
// are copied in as they are; wave w owns output channels [16 w, 16 w + 16) for all RT row tiles and accumulates the 9 taps, tap by
// tap, 4 channels at a time.  The epilogue goes through LDS so that a wave stores whole 64-channel rows: v = acc * scale + shift,
// + residual (the block's input, read and written in place by the same thread), ReLU.  With `pooled` the rows stay in LDS and
// pooled[b] = (the V rows summed in order) / V.  A board with active[b] != 1 is skipped whole (no loads, no stores).
template <int N, bool VEC>
__global__ __launch_bounds__(256) void cnn_conv_kernel(int Cin, int Cout, const float* __restrict__ X, const float* __restrict__ Wp,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      const float* res, const uint8_t* __restrict__ active, float* H,
                                                      float* __restrict__ pooled) {
    constexpr int V = N * N, P = N + 2, R2 = P * P, RT = (V + 15) / 16, RP = 16 * RT;
    static_assert(RP * YS <= WSLAB, "the epilogue tile must fit over the weight slab");
    __shared__ alignas(16) float ws[WSLAB];
    __shared__ alignas(16) float xs[(KS / 4) * R2 * 4];
    const int b = blockIdx.x, n0 = blockIdx.y * 64;
    if (active && active[b] != 1) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int ks = slabs_of(Cin);
    const size_t r0 = (size_t)b * V;
    for (int i = tid; i < (KS / 4) * R2 * 4; i += 256) xs[i] = 0.f;       // the halo stays zero over every slab
    // grid position of output row 16 t + c (a padding row >= V reads tile 0's window: its results are never stored)
    int base[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int r = 16 * t + c;
        base[t] = r < V ? (r / N + 1) * P + r % N + 1 : P + 1;
    }
    f32x4 acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4* wsrc = reinterpret_cast<const f32x4*>(Wp + (size_t)blockIdx.y * ks * WSLAB);
    for (int s = 0; s < ks; ++s) {
        const int k0 = KS * s;
        __syncthreads();
        for (int i = tid; i < WSLAB / 4; i += 256) reinterpret_cast<f32x4*>(ws)[i] = wsrc[(size_t)s * (WSLAB / 4) + i];
        if constexpr (VEC) {            // Cin % 4 == 0, X 16-byte aligned: a 4-channel group is wholly inside or outside Cin
            for (int idx = tid; idx < V * (KS / 4); idx += 256) {
                const int r = idx / (KS / 4), kq = idx % (KS / 4), k = k0 + 4 * kq;
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (k < Cin) v = *reinterpret_cast<const f32x4*>(X + (r0 + r) * Cin + k);
                *reinterpret_cast<f32x4*>(xs + (kq * R2 + (r / N + 1) * P + r % N + 1) * 4) = v;
            }
        } else {
            for (int idx = tid; idx < V * KS; idx += 256) {
                const int r = idx / KS, k = idx % KS;
                xs[((k >> 2) * R2 + (r / N + 1) * P + r % N + 1) * 4 + (k & 3)] = k0 + k < Cin ? X[(r0 + r) * Cin + k0 + k] : 0.f;
            }
        }
        __syncthreads();
        for (int tap = 0; tap < 9; ++tap) {
            const int off = (tap / 3 - 1) * P + (tap % 3 - 1);
#pragma unroll
            for (int kq = 0; kq < KS / 4; ++kq) {
                const float bw = ws[((tap * (KS / 4) + kq) * 64 + 16 * w + c) * 4 + q];
#pragma unroll
                for (int t = 0; t < RT; ++t) acc[t] = mfma4(xs[(kq * R2 + base[t] + off) * 4 + q], bw, acc[t]);
            }
        }
    }
    __syncthreads();                            // every wave is done with the weight slab: the epilogue tile goes over it
    float* const ys = ws;
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) ys[(16 * t + 4 * q + i) * YS + 16 * w + c] = acc[t][i];   // C/D: row 4 q + i, col c
    __syncthreads();
    const int n = n0 + lane;
    const bool nok = n < Cout;
    const float sc = nok ? scale[n] : 0.f, sh = nok ? shift[n] : 0.f;
    for (int r = w; r < V; r += 4) {
        float v = fmaf(ys[r * YS + lane], sc, sh);
        if (res && nok) v += res[(r0 + r) * Cout + n];
        v = fmaxf(v, 0.f);
        if (pooled) ys[r * YS + lane] = v;
        else if (nok) H[(r0 + r) * Cout + n] = v;
    }
    if (!pooled) return;
    __syncthreads();
    if (w == 0 && nok) {
        float sum = 0.f;
        for (int r = 0; r < V; ++r) sum += ys[r * YS + lane];
        pooled[(size_t)b * Cout + n] = sum / (float)V;
    }
}

template <int N>
int launch_conv_n(int B, int Cin, int Cout, const float* X, const float* Wp, const float* scale, const float* shift, const float* res,
                  const uint8_t* active, float* H, float* pooled, hipStream_t st) {
    const dim3 grid(B, tiles_of(Cout)), blk(256);
    const bool vec = Cin % 4 == 0 && ((uintptr_t)X & 15) == 0;
    if (vec) hipLaunchKernelGGL((cnn_conv_kernel<N, true>), grid, blk, 0, st, Cin, Cout, X, Wp, scale, shift, res, active, H, pooled);
    else hipLaunchKernelGGL((cnn_conv_kernel<N, false>), grid, blk, 0, st, Cin, Cout, X, Wp, scale, shift, res, active, H, pooled);
    return check_launch("cnn_conv_kernel");
}

int launch_conv(int N, int B, int Cin, int Cout, const float* X, const float* Wp, const float* scale, const float* shift, const float* res,
                const uint8_t* active, float* H, float* pooled, hipStream_t st) {
    return for_board_size(N, [&](auto n) { return launch_conv_n<decltype(n)::value>(B, Cin, Cout, X, Wp, scale, shift, res, active, H, pooled, st); });
}

struct CnnWorkspace { float* x0; float* xa; float* xt; float* pooled; float* logits; float* vpre; };

inline size_t cnn_ws_layout(int N, int F, int A, int B, CnnWorkspace* ws, float* base) {
    const size_t R = (size_t)B * N * N;
    const size_t sz[6] = {R * 6, R * F, R * F, (size_t)B * F, (size_t)B * A, (size_t)B};
    size_t off[6], total = 0;
    for (int i = 0; i < 6; ++i) { off[i] = total; total += round64(sz[i]); }
    if (ws && base) {
        ws->x0 = base + off[0]; ws->xa = base + off[1]; ws->xt = base + off[2]; ws->pooled = base + off[3];
        ws->logits = base + off[4]; ws->vpre = base + off[5];
    }
    return total;
}

// the network after the input rows: 2 L + 1 convs, pool, heads
int cnn_trunk_heads(int N, int B, const aqg_cnn_net* net, const uint8_t* active, const CnnWorkspace& ws, float* pooled, float* logits,
                    float* policy, float* value_pre, float* value, hipStream_t st) {
    const int F = net->num_filters, L = net->num_blocks, A = net->policy_size;
    CnnLayout lay;
    cnn_layout(F, L, A, &lay);
    const float* pk = net->packed;
    const int nconv = 2 * L + 1;
    for (int l = 0; l < nconv; ++l) {
        const bool last = l == nconv - 1;
        // stem: x0 -> xa;  block i: xa -> xt (conv_bn1), then xt (+ xa) -> xa (conv_bn2, in place over its residual)
        const float* X = l == 0 ? ws.x0 : (l & 1) ? ws.xa : ws.xt;
        float* H = (l & 1) ? ws.xt : ws.xa;
        const float* res = (l > 0 && !(l & 1)) ? ws.xa : nullptr;
        if (int r = launch_conv(N, B, conv_cin(l, F), F, X, pk + lay.conv_w[l], pk + lay.scale[l], pk + lay.shift[l], res, active,
                                last ? nullptr : H, last ? pooled : nullptr, st))
            return r;
    }
    // heads (pv_network_cnn.py:68-78): one Linear each off the pool over every row (a skipped board's rows are garbage in, garbage
    // out, never read), then softmax / tanh for the active boards only -- an inactive board's policy / value rows are left as they were
    if (int r = launch_gen_linear(B, F, A, pooled, pk + lay.pw, pk + lay.pb, nullptr, 0, logits, st)) return r;
    if (int r = launch_gen_linear(B, F, 1, pooled, pk + lay.vw, pk + lay.vb, nullptr, 0, value_pre, st)) return r;
    return launch_gen_heads(B, A, logits, value_pre, policy, value, st, active);
}

}  // namespace

int check_cnn_net(const aqg_cnn_net* net, int N, const char** why) {
    if (!net) { *why = "null network descriptor"; return -1; }
    if (net->board_size != N) { *why = "the network's board_size is not the call's"; return -1; }
    if (net->num_filters < 1 || net->num_filters > AQG_CNN_MAX_FILTERS) { *why = "num_filters must be 1..512"; return -1; }
    if (net->num_blocks < 0 || net->num_blocks > AQG_CNN_MAX_BLOCKS) { *why = "num_blocks must be 0..40"; return -1; }
    if (net->policy_size < 1 || net->policy_size > 4096) { *why = "policy_size must be 1..4096"; return -1; }
    if (!net->packed) { *why = "packed is NULL (aqg_cnn_pack)"; return -1; }
    return 0;
}

size_t cnn_packed_floats(int F, int L, int A) {
    if (F < 1 || F > AQG_CNN_MAX_FILTERS || L < 0 || L > AQG_CNN_MAX_BLOCKS || A < 1 || A > 4096) return 0;
    CnnLayout lay;
    cnn_layout(F, L, A, &lay);
    return lay.total;
}

int launch_cnn_pack(int F, int L, int A, const float* const* params, const float* eps, float* packed, hipStream_t st) {
    if (!cnn_packed_floats(F, L, A)) return fail("aqg_cnn_pack: num_filters 1..512, num_blocks 0..40, policy_size 1..4096");
    if (!params || !eps || !packed) return fail("aqg_cnn_pack: params, eps and packed are required");
    const int nconv = 2 * L + 1, np = 5 * nconv + 4;
    for (int i = 0; i < np; ++i)
        if (!params[i]) return fail("aqg_cnn_pack: a parameter pointer is NULL");
    CnnLayout lay;
    cnn_layout(F, L, A, &lay);
    const int Fp = 64 * tiles_of(F);
    for (int l = 0; l < nconv; ++l) {
        const float* const* p = params + 5 * l;
        const int ks = slabs_of(conv_cin(l, F));
        const size_t n = (size_t)tiles_of(F) * ks * WSLAB;
        hipLaunchKernelGGL(cnn_pack_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, conv_cin(l, F), F, ks, n, p[0],
                           packed + lay.conv_w[l]);
        hipLaunchKernelGGL(cnn_pack_bn_kernel, dim3((Fp + 255) / 256), dim3(256), 0, st, F, Fp, p[1], p[2], p[3], p[4], eps[l],
                           packed + lay.scale[l], packed + lay.shift[l]);
    }
    const float* const* h = params + 5 * nconv;
    const size_t bytes[4] = {(size_t)A * F * 4, (size_t)A * 4, (size_t)F * 4, 4};
    const size_t dst[4] = {lay.pw, lay.pb, lay.vw, lay.vb};
    for (int i = 0; i < 4; ++i)
        if (hipMemcpyAsync(packed + dst[i], h[i], bytes[i], hipMemcpyDeviceToDevice, st) != hipSuccess) return fail("aqg_cnn_pack: hipMemcpyAsync");
    return check_launch("cnn_pack kernels");
}

size_t cnn_workspace_floats(int N, int F, int A, int B) {
    if (!board_size_supported(N) || F < 1 || F > AQG_CNN_MAX_FILTERS || A < 1 || B <= 0) return 0;
    return cnn_ws_layout(N, F, A, B, nullptr, nullptr);
}

// input: states (planes == nullptr) or [B,6,N,N] planes
static int cnn_forward(const char* what, int N, const void* states, int fmt, const float* planes, int B, const aqg_cnn_net* net,
                       const uint8_t* active, float* workspace, size_t workspace_floats, float* pooled, float* logits, float* policy,
                       float* value_pre, float* value, hipStream_t st) {
    const char* why = "";
    if (!board_size_supported(N)) return fail(what, "board_size must be 3, 5, 7 or 9");
    if (!planes && fmt != 0 && fmt != 1) return fail(what, "state_fmt must be 0 or 1");
    if (B < 0) return fail(what, "negative size");
    if (check_cnn_net(net, N, &why)) return fail(what, why);
    if (B == 0) return 0;
    if (!(planes ? (const void*)planes : states) || !policy) return fail(what, "the input and policy are required");
    const int F = net->num_filters, A = net->policy_size;
    if (!workspace || workspace_floats < cnn_workspace_floats(N, F, A, B)) return fail(what, "workspace too small (aqg_cnn_workspace_floats)");
    CnnWorkspace ws;
    cnn_ws_layout(N, F, A, B, &ws, workspace);
    if (!pooled) pooled = ws.pooled;
    if (!logits) logits = ws.logits;
    if (!value_pre) value_pre = ws.vpre;
    if (planes) {
        const size_t R = (size_t)B * N * N;
        hipLaunchKernelGGL(cnn_planes_kernel, dim3((unsigned)((R * 6 + 255) / 256)), dim3(256), 0, st, planes, N * N, R, ws.x0);
        if (int r = check_launch("cnn_planes_kernel")) return r;
    } else if (int r = launch_gcn_boards_features(N, states, fmt, B, ws.x0, st)) {
        return r;
    }
    return cnn_trunk_heads(N, B, net, active, ws, pooled, logits, policy, value_pre, value, st);
}

int launch_cnn_forward_boards(int N, const void* states, int fmt, int B, const aqg_cnn_net* net, const uint8_t* active, float* workspace,
                              size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre, float* value,
                              hipStream_t st) {
    return cnn_forward("aqg_cnn_forward_boards", N, states, fmt, nullptr, B, net, active, workspace, workspace_floats, pooled, logits,
                       policy, value_pre, value, st);
}

int launch_cnn_forward_planes(int N, const float* planes, int B, const aqg_cnn_net* net, const uint8_t* active, float* workspace,
                              size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre, float* value,
                              hipStream_t st) {
    return cnn_forward("aqg_cnn_forward_planes", N, nullptr, 0, planes, B, net, active, workspace, workspace_floats, pooled, logits,
                       policy, value_pre, value, st);
}

}  // namespace aqg
