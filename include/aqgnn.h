/*
 * include/aqgnn.h -- C ABI of libaqgnn_hip.so (MI355X / gfx950 only).
 *
 * The reference (ApproximateCaesar/AlphaQuoridorGNN) is pure Python and has no FFI layer; its boundary is
 * the Python module surface.  This library is the native layer *beneath* that surface: each
 * entry point is what a ctypes binding inside the reference's own modules would call for the hot path.  The
 * reference interface each one replaces is cited as file:line (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the parameter name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is stream-ordered and
 *     no entry point synchronises, allocates or frees device memory;
 *   - return value 0 = success, negative = error; aqg_last_error() returns a thread-local message;
 *   - `board_size` N in {3,5,7,9}; V = N*N tiles, NW = (N-1)^2 wall slots, A = V + 2*NW actions (209 at 9x9).
 *
 * state72 record (72 bytes) == State.to_array() (game_logic.py:96-100) flattened, plus plies and N:
 *   [0] player pos  [1] player walls left  [2] enemy pos (ENEMY's frame)  [3] enemy walls left
 *   [4..67] walls[64] (0 none / 1 horizontal / 2 vertical; first NW used)  [68..69] plies_played u16 LE
 *   [70] N  [71] 0
 */
#ifndef AQGNN_H
#define AQGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQG_MAX_LEGAL 136 /* >= 5 pawn moves + 128 wall placements */
#define AQG_ABI_VERSION 15

int aqg_abi_version(void);
const char* aqg_last_error(void);
/* tuning knobs: "trunk_variant" 0/1 = exact f32-input MFMA with 1/2 workgroups per CU, 3 = all-MFMA fp16 split trunk
 * (hi*hi + hi*lo + lo*hi: fp32-equivalent products; default = the 8-wave x 2-per-CU form, also selected by 6); "step_fast_depth" = tree depth (0..61) at which
 * the MCTS step hands over from registers to memory (the round-1 step kernel and its option are gone: no symbol, struct or
 * signature changed with them, so AQG_ABI_VERSION stays 15); "trunk_prio" = static wave priorities in the trunk (-1 = by launch size, default); "step_prio" / "heads_prio" 0..3 = wave
 * priority of the MCTS step / heads kernels (defaults 1 / 3); "step_waves" = games per step workgroup (1, 2, 4 or 8; default 8);
 * "step_heads" 0/1 = the heads inside the MCTS step kernel (default 1): with prior_mode 0 on the 9x9 board, the fp16-split kernels (not
 * AQG_GNN_EXACT_F32) and "step_waves" 8, every expanding step launch computes policy and value of its own workgroup's leaves from the
 * pooled rows, a simulation is two launches (step, trunk) instead of three, and policy / value of those leaves are not written to the
 * engine's `policy` / `value` buffers: after a move or search these hold the ROOT's evaluation (simulation 0 keeps its heads launch;
 * root noise reads it there) where the three-launch form leaves the last leaf's.  Bit-identical searches.  0 = three launches per
 * simulation everywhere (A/B runs, tests); part of the captured graphs' key;
 * "legal_beside_trunk" 0/1 (default 1): where "step_heads" applies, the evaluation cache is off and the set has fewer than 1,024 games, an expanding step launch ends on its
 * new leaf (state, flag, legal_count = -1) and the launch behind it carries ceil(num_games / 8) workgroups that search those leaves' legal
 * moves in front of the trunk's board workgroups -- the same search on the same state, beside the trunk instead of in front of it; still
 * two launches per simulation, bit-identical searches; counters[6] counts the leaves searched there; part of the captured graphs' key;
 * "policy_beside_step" 0/1 (default 1; additive to ABI 15): where "legal_beside_trunk" applies and the engine has a `gnn_workspace` (the expansion jobs live there: see the field), the step launches
 * behind an evaluation launch (simulations 2 .. sims - 1 and the move's last expansion) carry a second kind of workgroup, one per eight
 * games behind the step workgroups: it computes the leaves' policy rows, gathers and renormalises them at the legal actions and writes
 * the new child records, while the step workgroup of the same games computes only the value head, backs up and descends -- nothing in
 * a step launch reads the children it creates.  The evaluation launch's search leaves each marked leaf's {node_count, legal count} in
 * its job record, the only per-game input of the policy workgroups that the step workgroups do not overwrite; counters[7] counts the leaves expanded there.  No new launch, stream or
 * graph branch; bit-identical searches; part of the captured graphs' key;
 * "train_fused" = form of the training step
 * (csrc/gcn_train.hip): 2 (default) one workgroup per position with every contraction in fp16 split precision on the 16-bit
 * matrix pipe (9x9 board; a position whose values leave fp16 range is redone in f32 inside the same launch, counted by
 * aqg_gcn_train_fallbacks), 1 one workgroup per position with f32-input MFMA, 3 = 2 with every position sent through the
 * f32 fallback (tests); other values are refused;
 * "trunk_phase_delay" = start offset of the second- / third-resident workgroups in units of 64 cycles, applied to
 * launches of at least "trunk_delay_min_boards" boards; "trunk_grid" = workgroups of a trunk launch (0 = default: min(boards, 512); diagnostics);
 * "use_graph" 0/1 = replay
 * a move's 2*sims+3 (3*sims+2 without "step_heads") launches as one captured hipGraph when the stream is capturable (default 1); "profile_trunk" 0/1/2 = no event pairs / around trunk launches / around MCTS step launches */
int aqg_set_option(const char* name, int value);
/* Measurement aid (bench.py): with option "profile_trunk" = 1 a HIP event pair is recorded around every launch of the
 * dominant kernel (the GCN trunk) on its launch stream; = 2 brackets the MCTS step kernel's launches instead (`boards` then
 * counts games).  This call waits for the last recorded event, accumulates
 * the elapsed times and returns the running totals (HOST pointers; `boards` = sum of launch batch sizes incl.
 * masked-out rows); reset != 0 clears the totals.  It is the only entry point that blocks the host. */
int aqg_profile_collect(double* total_ms_host, long long* launches_host, long long* boards_host, int reset);
/* Test aid: overwrite the LDS of every CU with NaN bit patterns (stream-ordered), so a kernel that reads LDS it
 * has not written fails deterministically instead of depending on what the previous kernel left behind. */
int aqg_debug_poison_lds(void* stream);
/* Diagnostic builds (-DAQG_TRACE) only; a no-op otherwise: every workgroup of the per-simulation kernels appends
 * {kernel id, tag, start, end | blockIdx << 48} (u64 x 4, 100 MHz timestamps) to `buffer` (device memory, first u64 = entry
 * counter, zeroed by the caller, room for `capacity` entries).  tools/trace_overlap.py. */
int aqg_debug_trace(void* buffer, unsigned int capacity);

/* ------------------------------------------------------------------ game rules (game_logic.py) */

/* State.legal_actions()  game_logic.py:103-117 (+ :120-192 pawn moves, :195-357 wall legality incl. the
 * touch-count prefilter :227-307 and the jump-aware BFS :309-348), batched.
 *   mask  [B, A]  u8, 1 = legal (may be NULL)
 *   order [B, AQG_MAX_LEGAL] u8 action ids in the reference's list order (pawn U,D,L,R/jumps, then per slot
 *         H,V interleaved), entries >= count are 0xFF (may be NULL)
 *   count [B] i32 number of legal actions (may be NULL) */
int aqg_legal_actions(int board_size, const uint8_t* states72, int B, uint8_t* mask, uint8_t* order,
                      int32_t* count, void* stream);

/* State.next(action)  game_logic.py:366-391 (incl. rotate_walls :359-364), batched. */
int aqg_state_next(int board_size, const uint8_t* states72, const int32_t* actions, int B, uint8_t* out72,
                   void* stream);

/* is_lose / is_draw  game_logic.py:43-54 : flags[b] = (lose ? 1 : 0) | (draw ? 2 : 0). */
int aqg_state_status(int board_size, const uint8_t* states72, int B, int plies_for_draw, uint8_t* flags,
                     void* stream);

/* ------------------------------------------------------------------ GNN (pv_network_gnn.py) */

/* Packed weights: one float32 device buffer holding the state_dict of GraphPolicyValueNetwork
 * (pv_network_gnn.py:23-51) in kernel order.  Offsets in floats (9x9: F=6, H=128, A=209):
 *   W1  [H][8]   gcn_layers.0.lin.weight [H,F] rows padded to 8     b1 [H]
 *   W2T [H][H]   gcn_layers.1.lin.weight transposed ([k][n])        b2 [H]
 *   W3T [H][H]   gcn_layers.2.lin.weight transposed                 b3 [H]
 *   HW1T[H][H]   hidden layer of both heads, [k][unit]: unit<H/2 policy_head.0, else value_head.0    hb1 [H]
 *   PW2T[H/2][256] policy_head.2.weight transposed ([k][a], a padded to 256)   pb2 [256]
 *   VW2 [H/2]    value_head.2.weight                                vb2 [1] (+3 pad)
 *   WF2, WF3     W2^T / W3^T again in f32 MFMA B-fragment order (exact-f32 trunk variants 0/1)
 *   WH2, WH3     fp16 hi/lo planes of W2^T / W3^T in 16x16x32 MFMA B-fragment order (default trunk)
 *   WH1          fp16 hi/lo of (15/16) gcn_layers.0.lin.weight as A fragments, rows = output features, the split folded into one
 *                32-deep k block (default trunk: layer 1 runs aggregate-first, (A_hat X) W1)
 *   WHH1, WHP2   the heads' matrices as fp16 hi/lo fragments;  TB  bias rows (15/16) b sqrt(deg) per layer and degree;
 *   GUARD [4]    thresholds of the trunk's fp16-range guard on the linear maps' outputs: [0] = (65504 - max |TB of layer 2|) / 2.07
 *                (below it layer 2's aggregate provably stays under 65504), [1] = 65504, [2..3] spare (ABI 8: the last four floats);
 *                both are -1 (no maximum passes: every board is reported) when a trunk weight's fp16 hi half is not finite
 *                (|W| (16/15) >= 65504, inf or NaN), or when a weight matrix that travels as hi/lo planes (gcn_layers.0/1/2,
 *                policy_head.0, value_head.0, policy_head.2; each on its own) is not all zero and has no entry of magnitude 2^-8 or
 *                more: its lo halves are fp16 subnormals and it would be carried to 2^-25 absolute, whatever its own scale
 *                (same layout, same ABI number: only the values of [0] and [1] for such sets changed)
 * aqg_gcn_packed_floats() returns the total; aqg_gcn_pack_weights_host() fills a HOST buffer from the 14
 * state_dict tensors given as HOST float32 pointers in the key order of KEYS in INTEGRATION.md. */
size_t aqg_gcn_packed_floats(int board_size);
int aqg_gcn_pack_weights_host(int board_size, const float* const* tensors_host, float* packed_host);

/* GraphPolicyValueNetwork.forward  pv_network_gnn.py:53-64 on B boards given as state72 records: node
 * features = pv_network_cnn.py:88-114 read as [V,6]; graph = wall-cut 4-neighbour grid;
 * 3 x (GCNConv + ReLU) -> global_mean_pool -> heads.  f32 data and accumulation throughout; the two 128x128
 * contractions and the neighbourhood aggregation run on the matrix cores as an fp16 hi/lo split with f32 accumulation
 * (default, fp32-equivalent) or as exact f32-input MFMA + VALU aggregation (trunk_variant 0/1, same tolerance).
 *   pooled    [B,128]  workspace/out: mean-pooled trunk features
 *   logits    [B,A]    pre-softmax policy (may be NULL)
 *   policy    [B,A]    Softmax output == module output (may be NULL)
 *   value_pre [B]      pre-tanh value (may be NULL)
 *   value     [B]      Tanh output == module output (may be NULL)
 * state_fmt: 0 = state72 records, 1 = 24-byte packed QState (engine-internal).
 * flags: AQG_GNN_EXACT_F32 forces the exact f32-input MFMA trunk and the f32 heads for this call whatever "trunk_variant" says.
 *   The fp16-split kernels hold every weight and activation as two fp16 numbers, hi + lo.  That is fp32-equivalent while the
 *   values stay inside fp16 range (|x| < 65504, saturating instead of overflowing beyond) AND the lo halves stay normal fp16
 *   numbers: a value below 2^-3 has a subnormal lo and is carried to 2^-25 absolute, so a matrix or an activation image whose whole
 *   scale is m is carried to 2^-25 / m of it -- fp32-equivalent at m ~ 1, past the stated tolerance (atol 1e-5, rtol 1e-4) below
 *   m ~ 2^-11.  Both hold for a network of ordinary scale, neither for every network the reference's fp32 serves (a ReLU network
 *   computes the same function with one layer scaled down and the next scaled up).  The packing refuses weight matrices below
 *   2^-8 (GUARD above).  That test looks at the LARGEST entry only: a matrix that is tiny but for one entry of 2^-8 passes it, and
 *   neither such a matrix nor small ACTIVATIONS under weights of ordinary scale have a run-time signal -- a raw caller of the guarded
 *   entry gets none.  (The split training step applies the same kind of test, at 2^-6 per block of 16 output features of a GCN
 *   matrix, with the same blind spot and nothing behind it.)  For the forward pass the host wrapper checks each
 *   weight set once against the exact kernels on calibration boards, at the stated tolerance taken relative to each board's output scale, and sets this flag when they
 *   disagree (pv_network_gnn.GraphPolicyValueNetwork.packed_weights). */
#define AQG_GNN_EXACT_F32 1
/* AQG_GNN_RANGE_PROVEN (with a non-NULL `saturated` word, ignored together with AQG_GNN_EXACT_F32): the caller has PROVEN -- by a
 * bound over ALL inputs whose two walls-in-hand counts are at most AQG_GNN_PROVEN_MAX_WALLS, not by sampling -- that no value the
 * split trunk holds as an fp16 pair can leave fp16 range for this weight set.  The trunk then skips its per-value range tracking
 * (one vector instruction per stored value, 4 % of the kernel) and checks each record's two wall counts against that maximum
 * instead: a record beyond it raises the word exactly as an out-of-range value would.  The bound GraphPolicyValueNetwork uses
 * (pv_network_gnn._range_proven): with R = 0.2 + 4/sqrt(10) = 1.465 >= every row sum of A_hat on a wall-cut grid and x_max =
 * (1, W, 1, W, 1, 1) for W = AQG_GNN_PROVEN_MAX_WALLS,  z_1 = |W_1| x_max,  h_l = R z_l + |b_l|,  z_{l+1} = |W_{l+1}| h_l;  proven
 * iff 2.3 max(z_l, h_l, |W_l|) < 65504 (2.3 covers the kernel's internal scales: planes c sqrt(deg) H <= 2.10 h, linear-map
 * outputs sqrt(deg) Z <= 2.24 z, weights W / c). */
#define AQG_GNN_RANGE_PROVEN 2
#define AQG_GNN_PROVEN_MAX_WALLS 16
int aqg_gcn_forward_boards(int board_size, const void* states, int state_fmt, int B, const float* packed,
                           float* pooled, float* logits, float* policy, float* value_pre, float* value,
                           int flags, void* stream);
/* The same call with the runtime fp16-range guard: `saturated` (device int32, may be NULL) is OR-ed with 1 by any fp16-split
 * kernel of the call that met a value it cannot hold as an fp16 pair -- a linear-map output or a post-ReLU activation beyond
 * 65504 (the activation is clamped there, never inf / NaN), a pooled feature or head hidden unit beyond it -- or could not rule one
 * out (the trunk bounds layer 2's aggregate by its linear map's output: a linear-map output beyond GUARD[0], about 31,600, is reported;
 * a weight set the packing refused -- a matrix outside fp16 range, or below the split's scale on the low side -- has negative GUARD
 * thresholds, and every board of it is reported).  The results of such
 * a call are finite but not the network's: the caller repeats it with AQG_GNN_EXACT_F32 and keeps that flag for the weight set
 * (GraphPolicyValueNetwork.forward_states / predict do; the engine reports the same event in counters[5]).  The word is never
 * cleared by the library.  Exact-f32 calls never set it.  Reference behaviour: fp32 throughout, no cliff (pv_network_gnn.py:53-64). */
int aqg_gcn_forward_boards_guarded(int board_size, const void* states, int state_fmt, int B, const float* packed,
                                   float* pooled, float* logits, float* policy, float* value_pre, float* value,
                                   int flags, int32_t* saturated, void* stream);
/* The same forward for ANY board size 3/5/7/9: 9x9 dispatches to the fused kernels above (workspace unused), the smaller
 * boards of the reference's constants.py:5-20 run on plain kernels (features + ELL adjacency -> linear / gather x3 -> pool
 * -> heads) and need `workspace` of aqg_gcn_boards_any_workspace_floats(board_size, B) floats. */
size_t aqg_gcn_boards_any_workspace_floats(int board_size, int B);
int aqg_gcn_forward_boards_any(int board_size, const void* states, int state_fmt, int B, const float* packed, float* workspace,
                               size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre, float* value,
                               int flags, void* stream);

/* ------------------------------------------------------------------ width-generic graph primitives (ABI 13)
 *
 * The building blocks of GraphPolicyValueNetwork at ANY shape (num_features, hidden_dim, num_gcn_layers, policy_output_size),
 * of the stand-alone GCNConv.forward(x, edge_index) and of global_mean_pool, forward and backward (csrc/gcn_general.hip; the
 * composition is pv_network_gnn.py: forward(x, edge_index, batch) of every shape, the default 6/128/3 included -- ABI 15 removed
 * the four fixed-width entry points aqg_gcn_{forward,backward}_graph* that served that one shape).  Every buffer is f32 and
 * contiguous (row-major); sizes are runtime values.  Every contraction runs on the f32-input MFMA (a k-ordered fmaf chain) and
 * no kernel uses atomics: each sum runs in an order fixed by the sizes, so results are deterministic.  A call with no rows
 * (M, num_nodes or num_graphs 0) launches nothing (aqg_graph_linear_grad writes zero gradients).
 * tests/test_graph_primitives.py checks this contract, one primitive at a time (the fmaf chain bit for bit against std::fmaf).
 *
 * aqg_graph_linear: Y[M,N] = X[M,K] W^T (+ bias[N]) -- nn.Linear / GCNConv.lin; W [N,K] in PyTorch's [out, in] layout straight
 *   from the parameter (flags & AQG_LIN_W_KN: W is [K,N] and Y = X W, the backward's dX = dY W).  bias may be NULL.  Then, in
 *   this order: AQG_LIN_ACCUMULATE adds the result to what Y holds; AQG_LIN_RELU applies max(., 0); a non-NULL mask [M,N]
 *   zeroes every element whose mask entry is not > 0 (the ReLU backward, with the saved post-ReLU activation as the mask).
 * aqg_graph_linear_grad: dW[N,K] = dY[M,N]^T X[M,K] and db[N] = sum over m of dYb[M,N] (dYb NULL = dY; db may be NULL):
 *   per-row-chunk partial tiles, then a fixed-order reduce, in `workspace` of aqg_graph_linear_grad_workspace_floats(M, N, K)
 *   floats.  Overwrites dW and db.
 * aqg_graph_aggregate: out[i][c] = (relu) ((bias ? bias[c] : 0) + sum over e = csr_ptr[i] .. csr_ptr[i+1] of
 *   csr_w[e] Y[csr_src[e]][c]), the entries in CSR order, Y and out [num_nodes, N].  An entry with csr_src < 0 is skipped (the
 *   board featuriser's ELL rows); every other id must lie in [0, num_nodes): nothing here checks it.  With the CSR by
 *   DESTINATION of GraphPolicyValueNetwork._prepare_graph it is GCNConv's propagate + bias; with its CSR by SOURCE (transpose=True),
 *   no bias and no ReLU, it is the backward A_hat^T dP.
 * aqg_graph_mean_pool: pooled[g] = mean of H[graph_ptr[g] .. graph_ptr[g+1]) (global_mean_pool; an empty graph pools to 0).
 * aqg_graph_mean_pool_backward: dH[i] = dpooled[g(i)] / |g(i)|, zeroed where mask [num_nodes, N] (may be NULL) is not > 0.
 *   Every node must lie in some graph: graph_ptr[0] = 0, graph_ptr[num_graphs] = num_nodes.
 * aqg_graph_heads: policy[g] = softmax(logits[g]) over A; value[g] = tanh(value_pre[g]) (value_pre / value may be NULL).
 * aqg_graph_heads_backward: dlogits[g] = policy[g] (dpolicy[g] - <dpolicy[g], policy[g]>), dvalue_pre[g] = dvalue[g] (1 - value[g]^2);
 *   dpolicy / dvalue NULL = zero.
 * aqg_gcn_boards_graph: the board featuriser of the any-size forward alone, for board_size 3/5/7/9: x [B*V, 6] node features
 *   (pv_network_cnn.py:88-114 read as [V,6]) and the normalised wall-cut grid adjacency as ELL rows of 5, ell_idx / ell_w
 *   [B*V, 5] (self loop first, then up / down / left / right; a closed side is index -1, weight 0); node b*V + t is tile t of
 *   board b.  csr_ptr[i] = 5 i over these rows is a CSR aqg_graph_aggregate accepts. */
#define AQG_LIN_RELU 1
#define AQG_LIN_W_KN 2
#define AQG_LIN_ACCUMULATE 4
int aqg_graph_linear(int M, int K, int N, const float* X, const float* W, const float* bias, const float* mask, int flags,
                     float* Y, void* stream);
size_t aqg_graph_linear_grad_workspace_floats(int M, int N, int K);
int aqg_graph_linear_grad(int M, int K, int N, const float* dY, const float* X, const float* dYb, float* workspace,
                          size_t workspace_floats, float* dW, float* db, void* stream);
int aqg_graph_aggregate(int num_nodes, int N, const float* Y, const int32_t* csr_ptr, const int32_t* csr_src, const float* csr_w,
                        const float* bias, int relu, float* out, void* stream);
int aqg_graph_mean_pool(int num_nodes, int N, const float* H, const int32_t* graph_ptr, int num_graphs, float* pooled,
                        void* stream);
int aqg_graph_mean_pool_backward(int num_nodes, int N, const float* dpooled, const int32_t* graph_ptr, int num_graphs,
                                 const float* mask, float* dH, void* stream);
int aqg_graph_heads(int num_graphs, int A, const float* logits, const float* value_pre, float* policy, float* value,
                    void* stream);
int aqg_graph_heads_backward(int num_graphs, int A, const float* policy, const float* dpolicy, const float* value,
                             const float* dvalue, float* dlogits, float* dvalue_pre, void* stream);
int aqg_gcn_boards_graph(int board_size, const uint8_t* states72, int B, float* x, int32_t* ell_idx, float* ell_w, void* stream);

/* ------------------------------------------------------------------ any-shape network on board records (ABI 14)
 *
 * aqg_gcn_general_net: a GraphPolicyValueNetwork of any shape, by reference to its parameters.  num_features must be 6 (the
 *   board featuriser's planes), hidden 2..1024, num_layers 1..AQG_GENERAL_MAX_LAYERS, policy_size 1..4096.  params[0 .. 2 L + 8)
 *   are DEVICE pointers to the contiguous f32 parameters in the order of pv_network_gnn.state_dict_keys(L), PyTorch layouts:
 *   gcn_layers.i.lin.weight [out,in], gcn_layers.i.bias [out] for each layer, then policy_head.0.weight / .bias, policy_head.2.weight
 *   / .bias, value_head.0.weight / .bias, value_head.2.weight / .bias.  The library reads the weights where they are, at every
 *   call: an in-place update of the tensors needs no new descriptor.
 * aqg_gcn_forward_boards_general: the network on B board records (state_fmt 0 = state72, 1 = the engine's 24-byte records) for
 *   board_size 3/5/7/9: the featuriser of aqg_gcn_boards_graph, then per layer ONE fused launch of GCNConv + bias + ReLU
 *   (linear map and 5-point stencil in LDS; the last layer writes the mean pool), then the heads of aqg_graph_linear /
 *   aqg_graph_heads.  Every output equals aqg_gcn_boards_graph followed by aqg_graph_linear / aqg_graph_aggregate (x L),
 *   aqg_graph_mean_pool and the heads bit for bit.  pooled [B,hidden], logits [B,policy_size] and value_pre [B] may be NULL (then
 *   they live in the workspace); policy [B,policy_size] is required, value [B] may be NULL.  active [B] (may be NULL): a board
 *   with active[b] != 1 is skipped -- its policy / value rows are not written, its other rows are unspecified.  `workspace`:
 *   aqg_gcn_boards_general_workspace_floats(board_size, hidden, policy_size, B) floats.  No allocation, no host synchronisation:
 *   the call can be captured into a hipGraph. */
#define AQG_GENERAL_MAX_LAYERS 32
typedef struct aqg_gcn_general_net {
    int32_t num_features, hidden, num_layers, policy_size;
    const float* params[2 * AQG_GENERAL_MAX_LAYERS + 8];
} aqg_gcn_general_net;
size_t aqg_gcn_boards_general_workspace_floats(int board_size, int hidden, int policy_size, int B);
int aqg_gcn_forward_boards_general(int board_size, const void* states, int state_fmt, int B, const aqg_gcn_general_net* net,
                                   const uint8_t* active, float* workspace, size_t workspace_floats, float* pooled, float* logits,
                                   float* policy, float* value_pre, float* value, void* stream);

/* ------------------------------------------------------------------ the reference's residual CNN (additive to ABI 14)
 *
 * CNNNetwork (pv_network_cnn.py:20-84) in eval mode: a 3x3 conv + BatchNorm2d stem, num_blocks residual blocks of two such convs
 * (ReLU, skip connection, ReLU), AdaptiveAvgPool2d(1), then Linear -> Softmax (policy) and Linear -> Tanh (value), all f32
 * (csrc/cnn_forward.hip: one implicit-GEMM launch per conv on the f32-input MFMA, BN folded into a per-channel scale / shift).
 * aqg_cnn_net: the shape (num_filters 1..AQG_CNN_MAX_FILTERS, num_blocks 0..AQG_CNN_MAX_BLOCKS, policy_size 1..4096, 6 input planes)
 *   and the DEVICE buffer aqg_cnn_pack filled (aqg_cnn_packed_floats(num_filters, num_blocks, policy_size) floats).
 * aqg_cnn_pack: folds and reorders the module's parameters on the device.  params_host: HOST array of DEVICE pointers to contiguous
 *   f32 tensors, per conv (the stem, then residual_blocks.i.conv_bn1, .conv_bn2 for each i) {conv.weight [F,Cin,3,3], bn.weight,
 *   bn.bias, bn.running_mean, bn.running_var}, then policy_head.1.weight [A,F], .bias, value_head.1.weight [1,F], .bias;
 *   eps_host[2 num_blocks + 1]: each BatchNorm2d's eps.  Capturable; re-run it after the parameters change.
 * aqg_cnn_forward_boards: the network on B board records (state_fmt 0 = state72, 1 = the engine's 24-byte records; the featuriser
 *   of aqg_gcn_boards_graph, i.e. pv_network_cnn.py:88-114); aqg_cnn_forward_planes: the same from [B,6,N,N] f32 planes.
 *   pooled [B,F], logits [B,A] and value_pre [B] may be NULL (then they live in the workspace); policy [B,A] is required, value [B]
 *   may be NULL.  active [B] (may be NULL): a board with active[b] != 1 is skipped -- its policy / value rows are not written.
 *   Every board is computed independently of the others: its outputs are bit-identical at any B, position and mask.  workspace:
 *   aqg_cnn_workspace_floats(board_size, num_filters, policy_size, B) floats.  No allocation, no host synchronisation.
 *   tests/test_cnn_conv_edges.py checks this contract on arbitrary planes (exact integer cases bit for bit at every slab and tile
 *   edge of num_filters, both limits included); tests/test_featuriser.py checks aqg_gcn_boards_graph alone. */
#define AQG_CNN_MAX_FILTERS 512
#define AQG_CNN_MAX_BLOCKS 40
typedef struct aqg_cnn_net {
    int32_t board_size, num_filters, num_blocks, policy_size;
    const float* packed;
} aqg_cnn_net;
size_t aqg_cnn_packed_floats(int num_filters, int num_blocks, int policy_size);
int aqg_cnn_pack(int num_filters, int num_blocks, int policy_size, const float* const* params_host, const float* eps_host, float* packed,
                 void* stream);
size_t aqg_cnn_workspace_floats(int board_size, int num_filters, int policy_size, int B);
int aqg_cnn_forward_boards(int board_size, const void* states, int state_fmt, int B, const aqg_cnn_net* net, const uint8_t* active,
                           float* workspace, size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre,
                           float* value, void* stream);
int aqg_cnn_forward_planes(int board_size, const float* planes, int B, const aqg_cnn_net* net, const uint8_t* active, float* workspace,
                           size_t workspace_floats, float* pooled, float* logits, float* policy, float* value_pre, float* value,
                           void* stream);

/* ------------------------------------------------------------------ batched PV-MCTS self-play (pv_mcts.py, self_play.py) */

/* All engine memory is owned by the caller (the Python host allocates torch tensors); this struct only
 * carries device pointers + sizes.  G concurrent games, one wavefront per game, lock-step simulations. */
typedef struct aqg_engine {
    int32_t board_size, num_walls, plies_for_draw;
    int32_t num_games;        /* G: concurrent game slots */
    int32_t quota;            /* games to play on those slots in all, >= G: a finished slot takes the next game not yet handed out
                                 (self_play.py:81-84 is a plain loop over games).  quota == G: one lock-step generation */
    int32_t sims;             /* PV_EVALUATE_COUNT  pv_mcts.py:18 */
    int32_t node_cap;         /* nodes per game tree >= 1 + sims * AQG_MAX_LEGAL */
    int32_t max_plies;        /* history rows per game slot (>= plies_for_draw) */
    int32_t prior_mode;       /* 0: network policy gathered at legal actions + renormalised (pv_network_cnn.py:129-132)
                                 1: `fake` integer-hash evaluator (tests; oracle/mcts.py FakeModel)
                                 2: external evaluator -- the caller's own model.predict (BaseNetwork.py:36-40) fills policy / value
                                    between aqg_engine_step calls (see below)
                                 3: the any-shape network of `general_net` (below), gathered and renormalised like 0
                                 4: the residual CNN of `cnn_net` (below), gathered and renormalised like 0 */
    int32_t fake_bias;
    int32_t gnn_flags;        /* flags of the GNN forward for prior_mode 0 (AQG_GNN_EXACT_F32 or 0) */
    float c_puct;             /* 1.25  pv_mcts.py:71 */
    float temperature;        /* SP_TEMPERATURE self_play.py:20; 1.0 exact, 0 = argmax.  Finite and >= 0, and when > 0:
                                 log2(sims + keep_visits) / temperature <= 1016 (keep_visits: tree reuse's, else 0), so that every term
                                 n ** (1 / temperature) of boltzman (pv_mcts.py:106-109) is below 2^1016 and the sum of at most
                                 AQG_MAX_LEGAL < 2^8 of them is finite.  Anything else is refused by every entry point that takes
                                 the engine, before a launch (the reference raises for a negative and for a too small one) */
    /* tree pool: [G * node_cap] 32-byte node records, two aligned 16-byte halves (ABI 9): {f64 w, f32 p, u32 action} -- read only of the
     * child a descent chooses -- and {i32 n, u32 first_child|count<<24, f32 q = f32(-w/n), f32 cp = f32(c_puct * p)} -- what PUCT
     * scores every child with (pv_mcts.py:69-78) */
    void* node_rec;
    /* per game, [G] */
    int32_t* node_count; uint8_t* root_state /* [G,24] */; int32_t* path /* [G, sims+2] */; int32_t* path_len;
    uint8_t* leaf_flag /* [G] 1 = this simulation's leaf needs an evaluation, 2 = it was served from the evaluation cache (below), 0 = no leaf (terminal / idle) */; uint8_t* leaf_state /* [G,24] */;
    uint8_t* game_active /* [G] slot is playing */; int32_t* slot_game /* [G] index of the game the slot is playing, -1 = retired */;
    /* per game, [quota] */
    int32_t* game_plies /* rows recorded */; int8_t* game_result /* z of ply 0 */; uint8_t* game_done /* 1 = finished */;
    int32_t* game_slot /* slot that played / plays it, -1 = not started */; int32_t* game_first_move /* index of its first aqg_engine_move */;
    /* evaluation buffers, [G,...] */
    uint8_t* legal_order /* [G,AQG_MAX_LEGAL] */; int32_t* legal_count; float* pooled /* [G,128] */;
    float* policy /* [G,A] */; float* value /* [G] */;
    /* history, per game: [quota, max_plies, ...] */
    uint8_t* hist_state72; uint16_t* hist_visits /* [G,max_plies,A] root child visit counts, dense by action */;
    uint8_t* hist_action /* [G,max_plies] */;
    /* counters [8] i32: 0 active slots, 1 finished games, 2 dead-end aborts, 3 next game index to hand out, 4 moves made
     * (updated once per move), 5 fp16-range guard: set to 1 by a GNN evaluation of this engine that met a value outside fp16 range
     * (see aqg_gcn_forward_boards_guarded; cleared by aqg_engine_reset only), 6 leaves whose legal-move search ran in the evaluation
     * launch beside the trunk instead of in the step launch (option "legal_beside_trunk"; cleared by aqg_engine_reset only), 7 leaves
     * expanded by the policy workgroups of a step launch (option "policy_beside_step"; cleared by aqg_engine_reset only) */
    int32_t* counters;
    /* per-game statistics [G] i32 (summed by the host): network evaluations, simulations that ended on a terminal node */
    int32_t* stat_leaf_evals; int32_t* stat_terminal_sims;
    const float* packed_weights;
    /* boards other than 9x9 with prior_mode 0: workspace of the any-size forward, aqg_gcn_boards_any_workspace_floats(N, G)
     * floats (may be NULL for 9x9 and for prior_mode 1).
     * 9x9 with prior_mode 0: the forward uses none of it; NULL, or at least 2 * num_games words -- a workspace of the size above is
     * larger -- whose first 2 G words are [G, 2] i32 expansion jobs {first_new, cnt} of option "policy_beside_step": what the evaluation
     * launch's legal-move search leaves for the policy workgroups of the step launch behind it ({0, 0} = none; every job is rewritten
     * by each evaluation launch and cleared by the step launch that used it, so the content the caller leaves there does not matter).
     * NULL: the option does not apply. */
    float* gnn_workspace;
    /* Evaluation cache (ABI 10; prior_mode 0, 3 (ABI 14) or 4; eval_cache_keys == NULL: off).  The reference builds a new tree for every move
     * (pv_mcts.py:84) and keeps no transposition table, so a game asks model.predict (pv_mcts.py:47) for the same position again and
     * again: transpositions inside a search, and the sub-tree of the move that was played in the next search.  The network's output and
     * legal_actions() are pure functions of (walls, pawns, walls in hand) -- not of the ply counter -- and the fused kernels compute every
     * board independently of its launch, so a per-slot table keyed by those 20 bytes returns bit-identical priors, values and legal
     * lists: the search, the visit counts and the game records do not change, only the leaf is not sent through the network (nor through
     * the legal-move kernel) again.  Per slot 1 << eval_cache_log2 entries: a 32-byte key record {u64 hw, u64 vw, u32 ppos|pwl<<8|
     * epos<<16|ewl<<24, u32 state (0 empty, 2 filled), i32 legal count, f32 value} + a 704-byte row {f32 priors[AQG_MAX_LEGAL] over
     * legal_actions() in order, renormalised (pv_network_cnn.py:129-132), u8 actions[AQG_MAX_LEGAL]}.  A slot keeps its table over its
     * games (positions stay valid); aqg_engine_reset clears it, and so must the caller when the weights change
     * (aqg_engine_clear_eval_cache).  leaf_flag[g] == 2 marks a leaf that was served from the table; eval_mask[g] == 1 the leaves the
     * network evaluates (the `active` mask of the GNN launches). */
    void* eval_cache_keys; void* eval_cache_rows;
    int32_t* eval_cache_slot /* [G] entry reserved for the pending evaluation, -1 none */; uint8_t* eval_mask /* [G] */;
    int32_t* stat_cache_hits /* [G] */;
    /* optional (both or neither): for sets of more than 512 slots aqg_engine_move hands the leaves that miss the table to the trunk
     * launch of simulation s as a compact list -- eval_list[0 .. eval_count[s]) -- instead of a mask to walk */
    int32_t* eval_list /* [G] */; int32_t* eval_count /* [sims + 1] */;
    int32_t eval_cache_log2;
    /* prior_mode 3 (ABI 14): the network of any shape the engine evaluates itself -- aqg_gcn_forward_boards_general over leaf_state
     * per simulation, masked by leaf_flag (eval_mask with the evaluation cache), into policy / value, with gnn_workspace of
     * aqg_gcn_boards_general_workspace_floats(board_size, hidden, A, G) floats; policy_size must be A.  Held BY VALUE: the captured
     * per-move graphs are keyed by the bytes of this struct, so every weight pointer and the shape are part of the key. */
    aqg_gcn_general_net general_net;
    /* prior_mode 4 (additive to ABI 14): the residual CNN -- aqg_cnn_forward_boards over leaf_state per simulation, masked like
     * prior_mode 3, with gnn_workspace of aqg_cnn_workspace_floats(board_size, num_filters, A, G) floats; policy_size must be A.
     * Held by value like general_net: the captured per-move graphs are keyed by the packed buffer's address and the shape. */
    aqg_cnn_net cnn_net;
    /* Root exploration noise (additive to ABI 15; see "root exploration noise" below).  root_noise_eps 0 = off: no launch, and a
     * struct whose four fields are zero behaves exactly as before.  eps in [0, 1); alpha in (0, 100] when eps > 0.  root_noise: NULL =
     * the counter-based generator keyed by root_noise_seed, else a device table f64 [G, AQG_MAX_LEGAL] of gamma variates that the
     * caller refills before each move.  The four fields are part of the captured graph's key like every other byte of the struct. */
    float root_noise_eps, root_noise_alpha;
    uint64_t root_noise_seed;
    const double* root_noise;
} aqg_engine;

/* Reset all G slots to the initial position (State() game_logic.py:25-40) and mark them active; clears the evaluation cache. */
int aqg_engine_reset(const aqg_engine* e_host, void* stream);
/* Empty the evaluation cache of every slot (after a weight update). */
int aqg_engine_clear_eval_cache(const aqg_engine* e_host, void* stream);
/* One self-play move for every active game == pv_mcts_policy (pv_mcts.py:20-95, `sims` lock-step simulations:
 * select :69-78, terminal/leaf evaluate :33-57, backup) + the body of play() (self_play.py:45-60): record
 * (state, visit counts), sample the action with uniforms[g] exactly like np.random.choice (self_play.py:57),
 * apply next(); finished games get z (self_play.py:22-27,:63-66) and go inactive.
 *   uniforms [G] f64 in [0,1). */
int aqg_engine_move(const aqg_engine* e_host, const double* uniforms, void* stream);
/* The same move in pieces, for an evaluator the library does not own (prior_mode 2; pv_mcts.py:47 calls model.predict on
 * whatever BaseNetwork it is given):
 *     aqg_engine_begin_move
 *     for sim in 0 .. sims-1:  aqg_engine_step(do_expand = sim > 0, do_select = 1)
 *                              -> for every game with leaf_flag[g] == 1 the caller writes policy[g][0 .. legal_count[g]) = PMF over
 *                                 the leaf's legal_actions() IN ORDER (legal_order[g]) and value[g]; leaf_state[g] is the 24-byte leaf
 *     aqg_engine_step(1, 0); aqg_engine_finish_move(uniforms)        (or aqg_engine_root_visits for a search only)
 * Per game exactly the reference's loop, one predict per simulation.  aqg_engine_set_roots installs caller-supplied roots. */
int aqg_engine_begin_move(const aqg_engine* e_host, void* stream);
int aqg_engine_step(const aqg_engine* e_host, int do_expand, int do_select, void* stream);
int aqg_engine_finish_move(const aqg_engine* e_host, const double* uniforms, void* stream);
int aqg_engine_set_roots(const aqg_engine* e_host, const uint8_t* root_states72, void* stream);
/* pv_mcts_policy only, for caller-supplied root states (no history, no transition): after the call
 * node_n of the root's children holds the visit counts; `root_states72` [G,72]. */
int aqg_engine_search(const aqg_engine* e_host, const uint8_t* root_states72, void* stream);
/* Read back the root's children after a search: visits [G,AQG_MAX_LEGAL] i32, actions [G,AQG_MAX_LEGAL] u8, count [G]. */
int aqg_engine_root_visits(const aqg_engine* e_host, int32_t* visits, uint8_t* actions, int32_t* count, void* stream);

/* Matches against an agent the engine does not search for (evaluate_agents.py; additive to ABI 14, csrc/agents.hip).
 * aqg_engine_root_states72: out72 [G,72] = the current position of every slot as a state72 record (the rows of inactive slots hold
 *   whatever position the slot was left in: valid bytes, unspecified content).
 * aqg_engine_apply_actions: the transition half of aqg_engine_move with caller-given actions [G] i32.  For every active slot with
 *   actions[g] >= 0: the history row (state72, the action, a visit row that is zero except 1 at the action), next(), game_plies + 1,
 *   and the lose / draw / z / counters / game_active handling of a searched move (and its slot refill when quota > num_games).
 *   actions[g] < 0 on an active slot is the dead end: the game ends as a draw and counters[2] is incremented.  The action is trusted
 *   to be legal, as State.next trusts it (one that is not an action of the board at all leaves the slot untouched).  A launch of
 *   its own: what aqg_engine_move captures and replays does not change, and the next searched move starts from the new root with
 *   a fresh tree, as every move does. */
int aqg_engine_root_states72(const aqg_engine* e_host, uint8_t* out72, void* stream);
int aqg_engine_apply_actions(const aqg_engine* e_host, const int32_t* actions, void* stream);

/* ------------------------------------------------------------------ root exploration noise (additive to ABI 15)
 *
 * With root_noise_eps > 0 every searched move mixes a Dirichlet sample into the root's priors (the reference has no such step):
 *     p'_i = (1 - eps) * p_i + eps * eta_i,   eta_i = f32(g_i / S),   S = g_0 + ... + g_{cnt-1} in float64,   g_i ~ Gamma(alpha, 1)
 * over the root's legal_actions() in order, all in f32 without contraction: 1 - eps is one subtraction, then two products and one
 * sum, each rounded.  p_i are the priors the step kernel would have taken: for the network evaluators the dense row gathered at the
 * legal actions and divided by its sum unless that is 0 (one f32 division), otherwise the first cnt entries of the row.  One launch
 * per move (csrc/mcts_move.hip, engine_root_noise_kernel), one wavefront per slot, between the evaluation of simulation 0 and the step
 * of simulation 1, inside the captured graph; it acts on the active slots whose pending leaf is the root (path_len 0, leaf_flag 1
 * or 2), writes p' to policy[g][0 .. cnt) and marks the leaf with leaf_flag 2 ("normalised priors in legal order").  No atomics, no
 * allocation, no host synchronisation; S is summed in a fixed order, so two runs give identical bytes.
 * The evaluation cache never sees p': a leaf_flag 2 leaf is not stored, and the slot's reservation (eval_cache_slot) is dropped, so
 * the position -- which later turns up as an inner leaf -- is evaluated and stored with the network's own priors then.
 * If S is 0 or not finite the root keeps its priors untouched; cnt == 0 writes nothing.
 *
 * g_i, table mode (root_noise != NULL): g_i = root_noise[g][i].  An entry that is not > 0 or not finite (NaN included) counts as 0:
 *   that action gets no noise mass; a row without a usable entry leaves the root untouched.
 * g_i, generator mode (root_noise == NULL): with mix, G and f(key, j) = (mix(key + G * (j + 1)) >> 11) * 2^-53 of the baseline
 *   agents' generator above, K(s, b) = mix(s + G * (b + 1)):
 *       root = K(K(root_noise_seed, k), ply)     k = slot_game[g], the GAME's index (the slot in the search-only entry point),
 *                                                ply = the root's plies_played
 *       key_i = K(root, i)                        component i draws from its own sub-stream: u_j = f(key_i, j)
 *   so a game's noise does not depend on num_games, slot refill or launch geometry.  Gamma(alpha, 1) in float64 after Marsaglia and
 *   Tsang, evaluated left to right without contraction: a = alpha + 1 if alpha < 1 else alpha; d = a - 1/3; c = 1 / sqrt(9 d);
 *   attempt t = 0 .. 63:  x = sqrt(-2 log(1 - u_{1+3t})) * cospi(2 u_{2+3t});  v1 = 1 + c x;  rejected if v1 <= 0;  v = v1^3;
 *       accepted if log(1 - u_{3+3t}) < 0.5 x x + d - d v + d log(v), and then g = d v.
 *   After 64 rejected attempts g = d (the value of v = 1; the chance is below 1e-80).  For alpha < 1, g = g * (1 - u_0)^(1/alpha).
 *   Finally g = max(g, DBL_MIN): the power may underflow, and a variate is never 0.  alpha is the f32 field widened to float64.
 *   cospi(y) = cos(pi y) is what the device evaluates (the argument is reduced exactly, before the multiplication by pi).
 *   engine.draw_root_noise(seed, k, ply, count, alpha) is the same function in numpy, with cos(2 pi u) for that factor (the product
 *   2 pi u is rounded first); that and the device's log / sqrt / pow differ from the C library's around 1e-15 relative.
 *
 * aqg_engine_root_noise: the launch on its own, for the external-evaluator loop -- behind the caller's evaluation of simulation 0,
 *   in front of aqg_engine_step(1, 1) -- and for tests.  With root_noise_eps == 0 it returns 0 and launches nothing.
 * aqg_engine_root_priors: priors [G,AQG_MAX_LEGAL] f32 = field p of the root's children (0 past the count), count [G] i32: the
 *   priors the last search built the root from, in the layout of aqg_engine_root_visits. */
int aqg_engine_root_noise(const aqg_engine* e_host, void* stream);
int aqg_engine_root_priors(const aqg_engine* e_host, float* priors, int32_t* count, void* stream);
/* aqg_engine_root_values (additive to ABI 15): value [G] f32 = the search value of every slot's root (node 0) after a search or in
 *   front of a finish-move, from the mover's side: n ? (float)(w / (double)n) : 0.0f -- the expression the finish-move launch stores
 *   into hist_value ("self-play targets" below), f32 of the f64 quotient.  One lane per slot (csrc/mcts_move.hip); a NULL argument is
 *   refused before any launch.  aqg_engine_search is unchanged: a caller asks for the values afterwards, as for the priors. */
int aqg_engine_root_values(const aqg_engine* e_host, float* value, void* stream);

/* ------------------------------------------------------------------ self-play targets (additive to ABI 15; the reference has neither)
 *
 * Two controls of what a self-play game teaches, both off by default and both outside the struct: the end of a move (the finish-move
 * launch of csrc/mcts_move.hip and the slot refill) is not part of the captured per-move graph, so the options travel as arguments of
 * two entry points and reach engine_finish_move_kernel as kernel arguments.  The engine struct, the graph cache and its key do not
 * change.  The two entry points below are the move and the finish-move entry points above with two more arguments, and with
 * (0, NULL) for them they behave bit for bit like those (which pass exactly that).
 *
 * temperature_plies = K > 0: the move of a root whose position has plies_played < K is chosen as always -- by e.temperature and
 *   uniforms[g] -- and a root with plies_played >= K takes the first maximum of the visit counts, the temperature == 0 branch.
 *   plies_played is the position's own ply counter, the one the root noise is keyed by.  Only the choice changes: the recorded
 *   policy target is the visit row at every ply.  uniforms[g] is still the slot's entry on an arg-max ply (it is not read), so a
 *   caller's stream of uniforms stays aligned.  K == 0: every ply by e.temperature.  K < 0 is refused.  No late temperature other
 *   than 0 is offered.
 * hist_value != NULL: f32 [quota, max_plies], indexed like hist_action.  Lane 0 of the slot's wavefront writes the root's search
 *   value from the mover's side, v = f32(w / n) with w the float64 sum and n the count of the root after the move's simulations
 *   (the bits of the root record's q, negated), 0 when n == 0; only if ply < max_plies.  Refused when max_plies == 0.  Rows made by
 *   the apply-actions entry point are not written: in a buffer that starts at zero they read 0. */
int aqg_engine_move_targets(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value, void* stream);
int aqg_engine_finish_move_targets(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                   void* stream);

/* ------------------------------------------------------------------ lambda-return value targets (additive to ABI 15; the reference has none)
 *
 * The TD(lambda) return of a finished game's recorded search values, bootstrapped into the game's outcome: the value that takes the
 * place of q in the blended target above, ring_z = (1 - L) z + L G_t.  One launch (csrc/value_targets.hip) over the arrays the
 * engine already holds, given as plain pointers: hist_value is no field of the struct, and any arrays of this layout will do.
 *
 * A finished game k has T = game_plies[k] recorded rows; q_t = hist_value[k * hp + t] is the search value of ply t from the mover's
 * side, r = game_result[k] the result from the side of ply index 0, and z_t = (float)r at an even t, -(float)r at an odd t (the sign
 * of history_tensors(); a draw's z_t is -0.0f at an odd t).  lambda is an f32 in [0, 1] and a = 1.0f - lambda.  In f32, without
 * contraction:
 *     G_{T-1} = a * q_{T-1} + lambda * z_{T-1}
 *     G_t     = a * q_t     + lambda * (-G_{t+1})        for t = T - 2 .. 0
 * -- two products and one sum per ply, each rounded, in the order of the blend (x = a * q, y = lambda * (..), x + y).  The side to
 * move changes every ply, hence -G_{t+1}.  lambda == 1 gives z_t (exactly for r != 0; a draw's zero may change its sign);
 * lambda == 0 gives q_t as a number (a zero may change its sign).  engine.lambda_values_reference is the same function in numpy,
 * bit for bit.
 *
 * Game k < quota is processed iff game_done[k] != 0 and 1 <= game_plies[k] <= hp; out[k * hp + t] is then written for
 * t < game_plies[k].  No other float of out is touched: not a skipped game's row, not the plies past a game's end.  One wavefront
 * per game, four per workgroup; the row is loaded and stored 64 consecutive floats at a time and the recurrence runs as one
 * wave-uniform chain from the last ply down; no LDS, no atomics, no workgroup barrier.  Any hp >= 1.
 * Refused on the host, before any launch (-1, aqg_last_error): quota < 0, hp < 1, a lambda outside [0, 1] or NaN, a NULL pointer,
 * out (quota * hp floats) overlapping hist_value.  quota == 0 returns 0 without a launch and without looking at the pointers. */
int aqg_lambda_values(int quota, int hp, const int32_t* game_plies, const int8_t* game_result, const uint8_t* game_done,
                      const float* hist_value, float lambda, float* out, void* stream);

/* ------------------------------------------------------------------ tree reuse (additive to ABI 15; the reference has none: pv_mcts.py:81)
 *
 * Opt-in: the next move's search starts from the subtree of the child this move chose instead of from an empty tree.  The option
 * travels as a small struct beside the engine struct, which does not change; the entry points above behave as they always did.
 *
 * The rule.  After a searched move at root R whose chosen child is c (index idx in R's child block), the next move's search starts
 * from c with its subtree as it stands -- every descendant's w, n, q, p, cp, action and child order -- iff
 *     the game goes on (not lost, not drawn, not the dead end),   c is expanded (kids != 0),   c.n <= keep_visits;
 * otherwise from a fresh root, exactly as without the option.  On top of either start the move runs the same `sims` simulations.
 * A node's subtree holds at most n expanded nodes and is at most n deep, so with K = keep_visits the caller sizes
 *     node_cap >= 1 + (K + sims) * AQG_MAX_LEGAL  (and < 2^24),     path [G, K + sims + 2],     K + sims <= 32767
 * (a visit count stays <= K + sims, and the visit row is read out as int16).  The step kernels are handed the struct with `sims`
 * replaced by K + sims -- their path stride -- and are otherwise unchanged; eval_count stays [sims + 1].
 * The new root record takes c's w, n, q and its renamed child range, and action 0xFF, p 0, cp 0 like a fresh root; n == 1 + the sum
 * of its children's n holds for it as for any expanded node.  The recorded visit row is the root's children's n and hist_value the
 * root's w / n, kept visits included.
 *
 * The keep launch (csrc/mcts_reuse.hip, engine_keep_subtrees_kernel; one wavefront per slot, no atomics, behind the finish-move
 * launch and outside the captured graph) re-roots the pool in place and in the old index order: c goes to index 0, then every kept
 * child block follows in ascending order of its old first index with the kept nodes' child ranges renamed, so c's own block lands at
 * index 1.  node_count[g] becomes the number of kept records; records behind it are unspecified.  While it runs it keeps its marks in
 * bits 8..31 of the records' action words, which are zero in every record before and after.  A slot whose tree is not kept, or that
 * is inactive, has its pool and node_count left byte for byte; the marker of an active slot that is not kept is cleared.
 * kept [G] u8, the marker: set by the keep launch only; the begin-move launch leaves a marked slot's pool and node_count alone (it
 * still clears the visit row and the evaluation-cache lists).  The finish-move launch of the _reuse entry points clears it (the root
 * changes); aqg_engine_reset, _set_roots and _apply_actions do not know it: call aqg_engine_reset_reuse behind them.  Slot refill
 * only touches inactive slots, which are never marked.
 * Root noise: a kept root is expanded already, so its noise -- same formula, key (seed, game, ply) and table as above -- is mixed
 * into its children's stored p, and cp = f32(c_puct * p') is rewritten, by one more launch in front of simulation 0's step (only with
 * root_noise_eps > 0).  Those children were never a root's before, so no prior is mixed twice.  A fresh root takes the launch above.
 * A game's kept trees are a function of the game alone: slots, refill order and set count do not change a game's rows.
 *
 * Refused before any launch: keep_visits < 0, keep_visits + sims > 32767, node_cap < 1 + (keep_visits + sims) * AQG_MAX_LEGAL,
 * prior_mode 2 (the external evaluator's loop has no keep step), a NULL buffer.  The per-move hipGraph is keyed by the marker's
 * address and keep_visits as well, so a reuse move and a plain move of one engine never replay each other's graph. */
typedef struct aqg_tree_reuse {
    int32_t keep_visits;            /* K >= 0; 0 = on, never keeps */
    uint8_t* kept;                  /* [G] the marker */
    int32_t* child_index;           /* [G] index of the chosen child in the root's block, -1 = do not keep (finish-move -> keep launch) */
    int32_t* stat_moves_kept;       /* [G] moves that started from a kept subtree ... */
    int32_t* stat_visits_kept;      /* [G] ... and the visits those subtrees held (summed by the host) */
} aqg_tree_reuse;
/* aqg_engine_move_targets / aqg_engine_finish_move_targets with the option: the keep launch follows the finish-move launch. */
int aqg_engine_move_reuse(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                          const aqg_tree_reuse* reuse, void* stream);
int aqg_engine_finish_move_reuse(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                 const aqg_tree_reuse* reuse, void* stream);
/* The keep launch alone on caller-given child indices [G] i32 (device), -1 = do not keep: for tests.  reuse->child_index is not read. */
int aqg_engine_keep_subtrees(const aqg_engine* e_host, const aqg_tree_reuse* reuse, const int32_t* child_index, void* stream);
/* Clear the marker (the statistics are the caller's to clear): behind aqg_engine_reset, aqg_engine_set_roots and aqg_engine_apply_actions. */
int aqg_engine_reset_reuse(const aqg_engine* e_host, const aqg_tree_reuse* reuse, void* stream);

/* ------------------------------------------------------------------ resignation (additive to ABI 15; the reference plays every game out)
 *
 * Opt-in: a self-play game whose mover's search says it is lost ends there, and a fraction of the games is played out regardless so
 * that the caller can count how often a resignation would have been wrong (AlphaGo Zero's calibration).  Like the two options above
 * it travels as a small struct beside the engine struct and reaches engine_finish_move_kernel as kernel arguments: the engine
 * struct, the step kernels, the captured per-move graph and its key do not change, and the entry points above behave as they did.
 *
 * The rule.  After the simulations of a searched move at root R with at least one child, by the mover at ply p = the position's
 * plies_played (== the game's ply counter in self-play from the opening):
 *     v_root = f32(w / n) of R, from the mover's side (the bits hist_value records; 0 when n == 0),
 *     v_best = q of the child at the FIRST maximum of the visit counts = f32(-w_c / n_c), 0 when n_c == 0,
 *     m      = max(v_root, v_best) in f32.
 * The mover resigns iff   p >= min_ply   and   m < -threshold (an f32 comparison)   and   the game is resign-enabled.
 * resign_min [quota, 2] f32: for every game and side (p & 1) the running minimum of m over that side's searched plies with
 *   p >= min_ply, from +inf, kept whether or not the game is enabled -- the only statistic a calibration needs: a side "would have
 *   resigned" at threshold T iff its minimum is < -T.  Written by lane 0 of the wavefront of the slot that plays the game: no atomics.
 * Game k is resign-enabled iff counter_uniform(stream_key(seed, k), 0) >= disable_fraction (float64; the generator of the root
 *   noise, keyed by the GAME index, never by the slot; engine.draw_resign_enabled is the same function in numpy).
 * A resigned game: the ply's history row is written as for any searched move (state, visit row, search value), its hist_action is
 *   0xFF, no transition is applied (root_state stays), game_plies[k] = p + 1, game_result[k] = the first player's value with the
 *   mover as loser (-1 if p is even, else +1), game_done[k] = 1, game_resigned[k] = 1; the slot goes inactive and counters[0] / [1]
 *   move as for a lost game.  Slot refill treats the slot like any finished one; with tree reuse its child_index is -1, so its next
 *   game starts from a fresh tree.  A dead end (no child) and a move that ends the game by rule behave as without the option.
 * z of the rows follows from game_result as always: the resigning row reads -1.
 *
 * Refused before any launch: threshold not in (0, 1], min_ply < 0, disable_fraction not in [0, 1], a NULL buffer, max_plies == 0.
 * threshold == 1 can never trigger (m >= -1): the games are those of the option off, and resign_min is still kept. */
typedef struct aqg_resign {
    float threshold;                /* T in (0, 1]: resign when m < -T */
    int32_t min_ply;                /* >= 0: no resignation and no statistic before this ply */
    double disable_fraction;        /* in [0, 1]: the share of games that never resign (0 = none, 1 = all) */
    uint64_t seed;                  /* of the enabled / disabled draw */
    float* resign_min;              /* [quota, 2] running minimum of m per game and side; +inf = no eligible ply yet */
    uint8_t* game_resigned;         /* [quota] 1 = the game ended by resignation */
} aqg_resign;
/* aqg_engine_move_reuse / aqg_engine_finish_move_reuse with the option; reuse == NULL = tree reuse off (then prior_mode 2 is served
 * by the finish-move form as by aqg_engine_finish_move_targets). */
int aqg_engine_move_resign(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                           const aqg_tree_reuse* reuse, const aqg_resign* resign, void* stream);
int aqg_engine_finish_move_resign(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                  const aqg_tree_reuse* reuse, const aqg_resign* resign, void* stream);
/* resign_min = +inf, game_resigned = 0: behind aqg_engine_reset. */
int aqg_engine_reset_resign(const aqg_engine* e_host, const aqg_resign* resign, void* stream);

/* ------------------------------------------------------------------ baseline agents in batch (agents.py; additive to ABI 14)
 *
 * The reference's random and rollout-MCTS agents (agents.py:14-18, :111-214) for B states at once, one wavefront per state
 * (csrc/agents.hip).  Device pointers, stream-ordered, no allocation, no host synchronisation, no atomics: two runs give identical
 * bytes.  Every device loop ends on an integer cap computed from the arguments; a position without a legal action inside a playout
 * ends that playout as a draw.
 *
 * Random draws.  Every random choice is index = min(count - 1, floor(u * count)) over legal_actions() in the reference's order, for
 * a float64 u in [0, 1).  u comes from one of two sources:
 *   uniforms != NULL: a table [B, uniforms_stride] f64; uniforms[b][i] is the i-th draw of state / game b within the call.  A draw
 *     past the end of a row is 0.0 (never a read out of bounds); the reported draw count tells the caller whether that happened.
 *   uniforms == NULL: the counter-based generator u = f(seed, b, i), stateless -- the result does not depend on launch geometry,
 *     wave scheduling or batch size.  With mix(z) the splitmix64 finaliser
 *         z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
 *     and G = 0x9E3779B97F4A7C15, all in 64-bit wrapping arithmetic:
 *         key = mix(seed + G * (b + 1));   f(seed, b, i) = (mix(key + G * (i + 1)) >> 11) * 2^-53.
 *     agents.draw_uniforms(seed, b, n) is the same function in numpy.
 * The reference draws with Python's random.randint; that stream is not reproduced.
 *
 * aqg_agent_random: actions[b] = legal_actions()[index] for one draw, or -1 (and no draw) where the state has no legal action.
 * aqg_playouts: playout() of agents.py:111-121 from each state: value [B] i32 = -1 / 0 / +1 from the point of view of the mover of
 *   the START state, plies [B] = moves played, draws [B] = draws consumed (one per move), final72 [B,72] = the position the playout
 *   ended in (plies, draws, final72 may be NULL).  A state that is already lost / drawn returns at once with 0 draws.  At most
 *   plies_for_draw - plies_played moves are played.
 * aqg_agent_mcts: mcts_action() of agents.py:130-214 for B roots, games in parallel, the evaluations of a game in order.  The root is
 *   expanded before the first evaluation; a descent takes the first child with n == 0, else the FIRST maximum of UCB1; a childless
 *   node gets a playout and is expanded on the visit that makes its n 10; a terminal node scores -1 (lost) or 0 (drawn) without a
 *   playout; the backup negates the value per ply; the answer is the first most-visited root child.  w is an integer.  UCB1 is
 *   float64, (double)(-w) / n + explore[t][n], with no contraction.  explore [(evaluations + 1)^2] f64 is filled by the HOST:
 *   explore[t * (evaluations + 1) + n] = 2 * (2 * log(t) / n) ** 0.5 for 1 <= n <= t <= evaluations exactly as the reference's
 *   CPython evaluates it (agents.py:196) -- the C library's log and pow(x, 0.5), neither of which the device reproduces bit for
 *   bit (pow(x, 0.5) differs from the correctly rounded sqrt(x) for 53 of the 80,200 pairs up to 400); t is the sum of the
 *   children's visit counts; evaluations <= AQG_AGENT_MCTS_MAX_EVALUATIONS.  Draws of game b are consumed in evaluation order, one per random move inside each playout.
 *   action [B] i32 (-1 = no legal action); visits [B,AQG_MAX_LEGAL] i32, actions [B,AQG_MAX_LEGAL] u8 (0xFF past the count) and
 *   count [B] i32 = the root's children in the layout of aqg_engine_root_visits; draws [B] = draws consumed (the last four may be
 *   NULL).  workspace: aqg_agent_mcts_workspace_bytes(board_size, B, evaluations) bytes hold the trees: a game expands its root and
 *   at most evaluations / 10 other nodes, so 1 + (1 + evaluations / 10) * AQG_MAX_LEGAL nodes of 48 bytes bound it. */
#define AQG_AGENT_MCTS_MAX_EVALUATIONS 2048 /* the explore table is (evaluations + 1)^2 doubles: 32 MiB at the cap */
int aqg_agent_random(int board_size, const uint8_t* states72, int B, const double* uniforms, int uniforms_stride, uint64_t seed,
                     int32_t* actions, void* stream);
int aqg_playouts(int board_size, const uint8_t* states72, int B, int plies_for_draw, const double* uniforms, int uniforms_stride,
                 uint64_t seed, int32_t* value, int32_t* plies, int32_t* draws, uint8_t* final72, void* stream);
size_t aqg_agent_mcts_workspace_bytes(int board_size, int B, int evaluations);
int aqg_agent_mcts(int board_size, const uint8_t* states72, int B, int evaluations, int plies_for_draw, const double* explore,
                   const double* uniforms, int uniforms_stride, uint64_t seed, void* workspace, size_t workspace_bytes,
                   int32_t* action, int32_t* visits, uint8_t* actions, int32_t* count, int32_t* draws, void* stream);

/* Depth-limited alpha-beta (agents.py:22-107) for B states at once (csrc/agents.hip; additive to ABI 15).  Device pointers,
 * stream-ordered, no allocation, no host synchronisation, no atomics, integer arithmetic only: two runs give identical bytes.
 * aqg_agent_shortest_paths: out [B,2] i32 = the plies the mover (out[b][0]) and the other side (out[b][1]) need to reach their goal
 *   rows over legal_actions_pos with the other pawn frozen, -1 = walled in: what aqg_host_shortest_path returns for the record and
 *   for its flipped record.  heuristic_eval is (out[b][1] - out[b][0]) / max_dist_from_goal, one float64 division by the caller.
 * aqg_agent_alpha_beta: action [B] i32 = aqg_host_alpha_beta_action of every record (-1 = no legal action), the FIRST root action
 *   with the maximal depth-limited negamax value.  One wavefront per (state, root action): root child 0 with the full window, the
 *   others in parallel under its value, then the first maximum; scores are compared as the integer numerators over
 *   max_dist_from_goal, which orders them exactly as the host's float64 values.  active: NULL, or [B] u8 (an engine's game_active):
 *   action[b] = 0 where active[b] == 0, without a search.  0 <= max_depth <= AQG_AGENT_AB_MAX_DEPTH, 1 <= max_dist_from_goal.
 *   nodes: NULL, or [B] i64 = the positions visited below the root (0 on a masked slot); it differs from the host's count because
 *   the children of a last-ply node are evaluated 64 at a time and root children 1.. do not see each other's scores.
 *   workspace: aqg_agent_alpha_beta_workspace_bytes(board_size, B, max_depth) bytes (0 = invalid board_size, B or max_depth). */
#define AQG_AGENT_AB_MAX_DEPTH 4
int aqg_agent_shortest_paths(int board_size, const uint8_t* states72, int B, int32_t* out, void* stream);
size_t aqg_agent_alpha_beta_workspace_bytes(int board_size, int B, int max_depth);
int aqg_agent_alpha_beta(int board_size, const uint8_t* states72, int B, const uint8_t* active, int plies_for_draw,
                         int max_dist_from_goal, int max_depth, void* workspace, size_t workspace_bytes, int32_t* action,
                         int64_t* nodes, void* stream);

/* ------------------------------------------------------------------ training step (train_network.py:68-95 on the GNN) */

/* One optimisation step on a batch of positions: forward, the reference's losses (CrossEntropyLoss applied to the
 * already-softmaxed policy with probability targets train_network.py:54,85 + MSELoss on the tanh value :55,86),
 * backward, and torch.optim.Adam's update (:56,:90-92).  f32 data and f32 accumulation; two launches per step: one workgroup per
 * position for forward + backward, one fixed-order reduction + Adam (csrc/gcn_train.hip).  On the 9x9 board (option "train_fused" 2,
 * the default) every contraction runs on the 16-bit matrix pipe in fp16 hi/lo split precision (three fp16 products per f32
 * product, the arithmetic of the inference trunk; a position whose values leave fp16 range is redone by the f32-input MFMA body inside
 * the same launch, aqg_gcn_train_fallbacks counts them); smaller boards and "train_fused" 1 use f32-input MFMA.  mode 0 = gradients only (into grads),
 * 1 = gradients + update, 2 = update only from whatever grads holds -- data-parallel training computes local gradients
 * (mode 0), all-reduces them over RCCL, and applies them (mode 2).  The 14 parameter tensors
 * are the state_dict tensors themselves in their PyTorch layouts and in the key order of KEYS in INTEGRATION.md; grads,
 * adam_m, adam_v have the same shapes.  All memory is the caller's (device pointers); nothing allocates or synchronises.
 * B = batch (the capacity the workspace was sized for is the caller's business), A = policy size. */
typedef struct aqg_train {
    int32_t board_size, batch, policy_size;
    int32_t step;                 /* Adam step count of THIS update, >= 1 */
    float lr, beta1, beta2, eps;  /* 1e-3 * LambdaLR factor (train_network.py:56-66), 0.9, 0.999, 1e-8 */
    float* params[14]; float* grads[14]; float* adam_m[14]; float* adam_v[14];
    /* workspace */
    float* h1; float* h2;         /* [B*96, 128] (96 rows per position on every board size): post-ReLU activations of layers 1, 2 -- node
                                   * rows in the f32 form, this round's parked fp16 hi / lo fragments in the split form */
    float* g;                     /* [B, 128]   pooled features */
    float* hp; float* hv; float* dhp; float* dhv;   /* [B, 64] head hidden layers and gradients */
    float* lg;                    /* [B, A]     d loss / d logits */
    float* pol;                   /* [B, A]     softmax policy (the network output) */
    float* vp; float* val;        /* [B]        d loss / d pre-tanh value; tanh value */
    float* loss;                  /* [B, 2]     per-position policy / value loss terms (their means are the two losses) */
    float* part;                  /* [B * AQG_TRAIN_PART_FLOATS] per-board partial sums of the trunk's weight and bias gradients */
} aqg_train;
#define AQG_TRAIN_PART_FLOATS (2 * 128 * 128 + 128 * 6 + 3 * 128)
int aqg_gcn_train_step(const aqg_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                       int mode, void* stream);
/* A run of consecutive single-process steps (mode 1) with no host work in between -- one epoch of train_network.py:72-95:
 * step i takes positions order[i*batch .. (i+1)*batch) (int64 indices into the resident arrays states72 [n,72],
 * pi_target [n,A], z_target [n]; order = NULL means 0..positions-1; the last batch may be short, as the reference's
 * DataLoader keeps it), t->step is the Adam count of the FIRST step, and every step adds its two batch-mean losses to
 * loss_sums[2] (device, may be NULL) -- the per-epoch sums train_network.py:89-90 prints. */
int aqg_gcn_train_steps(const aqg_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                        const int64_t* order, long long positions, float* loss_sums, void* stream);
/* Positions that the split-precision step ("train_fused" 2) has redone in f32 since the last reset (synchronises the device);
 * -1 on error.  A diagnostic: results do not depend on it. */
long long aqg_gcn_train_fallbacks(int reset);

/* ------------------------------------------------------------------ training step at any shape (additive to ABI 14)
 *
 * The step of aqg_gcn_train_step -- forward, the same two losses, backward, torch.optim.Adam -- for a GraphPolicyValueNetwork of
 * any shape aqg_gcn_general_net accepts (6 input features, hidden 2..1024, 1..AQG_GENERAL_MAX_LAYERS layers, policy_size 1..4096;
 * the default 6/128/3 included), on board records (state72, board_size 3/5/7/9), all f32 (csrc/gcn_train_general.hip).  The
 * forward is aqg_gcn_forward_boards_general's kernels with every layer's output kept: policy and value equal that call's bit for
 * bit.  The backward runs one fused launch per GCN layer (stencil and f32-input MFMA), the width-generic primitives for the heads
 * and the weight gradients, and one multi-tensor Adam launch.  No atomics (two runs give bit-identical parameters), no allocation,
 * no host synchronisation.
 *
 * aqg_train_general: num_features .. policy_size = the network's shape (as in aqg_gcn_general_net); params / grads / adam_m /
 *   adam_v [0 .. 2 L + 8) = device pointers to contiguous f32 tensors indexed like aqg_gcn_general_net.params (grads, adam_m, adam_v
 *   of the same shapes; the parameters are updated in place).  batch = positions of this step, step = the Adam count of THIS update
 *   (>= 1), lr / beta1 / beta2 / eps as torch.optim.Adam.  policy [batch, policy_size], value [batch], loss [batch, 2] (per-position
 *   policy / value loss terms) and loss_mean [2] (their batch means, summed in position order) receive the step's outputs; each may
 *   be NULL (it then lives in the workspace).  workspace: aqg_gcn_train_general_workspace_floats(board_size, hidden, num_layers,
 *   policy_size, max_batch) floats serve every batch up to max_batch.
 * aqg_gcn_train_step_general: mode 0 = gradients only (into grads), 1 = gradients + Adam, 2 = Adam only from whatever grads holds
 *   (data parallel: local gradients, all-reduce, update), as aqg_gcn_train_step.  batch 0: no gradients are formed, and mode 1
 *   still applies Adam from whatever grads holds, as mode 2 does (the CNN's step differs: below).
 * aqg_gcn_train_steps_general: one epoch, every step mode 1, as aqg_gcn_train_steps: step i takes the positions
 *   order[i*batch .. (i+1)*batch) (order NULL = 0 .. positions-1; the last batch may be short), t->step counts up from its entry
 *   value, and each step adds its two batch-mean losses to loss_sums[2] (device, may be NULL). */
typedef struct aqg_train_general {
    int32_t board_size, num_features, hidden, num_layers, policy_size;
    int32_t batch, step;
    float lr, beta1, beta2, eps;
    float* params[2 * AQG_GENERAL_MAX_LAYERS + 8];
    float* grads[2 * AQG_GENERAL_MAX_LAYERS + 8];
    float* adam_m[2 * AQG_GENERAL_MAX_LAYERS + 8];
    float* adam_v[2 * AQG_GENERAL_MAX_LAYERS + 8];
    float* policy; float* value; float* loss; float* loss_mean;
    float* workspace;
    size_t workspace_floats;
} aqg_train_general;
size_t aqg_gcn_train_general_workspace_floats(int board_size, int hidden, int num_layers, int policy_size, int max_batch);
int aqg_gcn_train_step_general(const aqg_train_general* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                               int mode, void* stream);
int aqg_gcn_train_steps_general(const aqg_train_general* t_host, const uint8_t* states72, const float* pi_target,
                                const float* z_target, const int64_t* order, long long positions, float* loss_sums, void* stream);

/* ------------------------------------------------------------------ training the residual CNN (additive to ABI 14)
 *
 * One optimisation step of CNNNetwork (pv_network_cnn.py:20-84) as the reference's train_network.py:26-107 takes it: the module in
 * train mode (every BatchNorm2d normalises with the batch mean and the biased batch variance over B x N x N per channel, and updates
 * running_mean / running_var in place with its momentum and the unbiased variance), CrossEntropyLoss on the already-softmaxed policy
 * + MSELoss on the value, backward, torch.optim.Adam -- on board records (state72, board_size 3/5/7/9), all f32
 * (csrc/cnn_train.hip).  Each 3x3 conv is an im2col GEMM on the f32-input MFMA, forward, dX and dW alike; every channel statistic
 * is a per-board partial merged in board order.  No atomics (two runs give bit-identical parameters and running statistics), no
 * allocation, no host synchronisation.  num_batches_tracked is the caller's to advance.
 *
 * Tensor order (T = 3 C + 4 tensors, C = 2 num_blocks + 1 convs: the stem, then conv_bn1 / conv_bn2 of each block): per conv its
 *   conv.weight [F,Cin,3,3], bn.weight [F], bn.bias [F]; then policy_head.1.weight [A,F], .bias [A], value_head.1.weight [1,F],
 *   .bias [1] -- the order of CNNNetwork.parameters().
 * aqg_cnn_train: the shape; batch = positions of this step; step = the Adam count of THIS update (>= 1); lr / beta1 / beta2 / eps as
 *   torch.optim.Adam; bn_eps / bn_momentum [C] = each BatchNorm2d's eps and momentum.  params / grads [T] = device pointers to
 *   contiguous f32 tensors (updated in place; grads of the same shapes); running_mean / running_var [C] = each BatchNorm2d's
 *   buffers (updated in place by every forward, modes 0 and 1).  adam_table: DEVICE array of 4 T pointers -- params, grads, adam_m,
 *   adam_v, each in tensor order (the same params / grads as above) -- built once by the caller: the single Adam launch reads it
 *   (247 tensors at 40 blocks would not fit in kernel arguments).  policy / value / loss / loss_mean as in struct aqg_train_general: each
 *   may be NULL.  workspace: aqg_cnn_train_workspace_floats(board_size, num_filters, num_blocks, policy_size, max_batch) floats.
 * aqg_cnn_train_step: mode 0 = gradients only, 1 = gradients + Adam, 2 = Adam only, as aqg_gcn_train_step_general; batch 0 = no-op
 *   (modes 0 and 1; mode 2 never reads the batch).
 * aqg_cnn_train_steps: one epoch, every step mode 1, with the order / loss_sums contract of aqg_gcn_train_steps_general. */
#define AQG_CNN_TRAIN_CONVS (2 * AQG_CNN_MAX_BLOCKS + 1)
#define AQG_CNN_TRAIN_TENSORS (3 * AQG_CNN_TRAIN_CONVS + 4)
typedef struct aqg_cnn_train {
    int32_t board_size, num_filters, num_blocks, policy_size;
    int32_t batch, step;
    float lr, beta1, beta2, eps;
    float bn_eps[AQG_CNN_TRAIN_CONVS];
    float bn_momentum[AQG_CNN_TRAIN_CONVS];
    float* params[AQG_CNN_TRAIN_TENSORS];
    float* grads[AQG_CNN_TRAIN_TENSORS];
    float* running_mean[AQG_CNN_TRAIN_CONVS];
    float* running_var[AQG_CNN_TRAIN_CONVS];
    float* const* adam_table;
    float* policy; float* value; float* loss; float* loss_mean;
    float* workspace;
    size_t workspace_floats;
} aqg_cnn_train;
size_t aqg_cnn_train_workspace_floats(int board_size, int num_filters, int num_blocks, int policy_size, int max_batch);
int aqg_cnn_train_step(const aqg_cnn_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                       void* stream);
int aqg_cnn_train_steps(const aqg_cnn_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                        const int64_t* order, long long positions, float* loss_sums, void* stream);

/* ------------------------------------------------------------------ optimiser controls (additive to ABI 15; the reference has none)
 *
 * Weight decay and global-norm gradient clipping for the three training steps above, pinned to torch.  With g the gradient of an
 * element and p its parameter, in this order (csrc/train_adam.hpp):
 *   1. clip, torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2): norm = the L2 norm over every gradient element of every
 *      tensor, coef = min(1, max_norm / (norm + 1e-6)) in f32, g <- coef g.  Nothing clipped: coef is exactly 1.0f.  A non-finite
 *      norm gets NO special treatment (torch's default, error_if_nonfinite=False): a NaN norm makes coef, the moments and the
 *      parameters NaN; an infinite one makes coef 0.  Nothing skips the step.
 *   2. weight decay, one coefficient per tensor (0 = none): decoupled != 0, torch.optim.AdamW: p <- p (1 - lr wd), then the unchanged
 *      Adam update on that p; decoupled == 0, torch.optim.Adam(weight_decay=wd): g <- g + wd p before the moments.
 *   3. the Adam update as before.
 * The norm is computed on the device with no host read and no float atomics (csrc/grad_norm.hip): one launch leaves a partial sum of
 * squares per 8,192 elements, and every workgroup of the step's Adam launch adds the partials up in a fixed order before it updates
 * (no combine launch).  Two runs give identical bits; at most 90 additions lie between any term and the total (relative error of the
 * norm below 5e-6).  The general and CNN steps go from one Adam launch to two launches and leave grads as computed.  The fused
 * 6/128/3 step, whose final launch forms and consumes each gradient element in one thread, goes to four (gradients, partials, clip
 * of the stored gradients in place, update) and leaves the CLIPPED gradient in grads, as clip_grad_norm_ leaves it in .grad; a
 * coefficient of exactly 1 writes nothing.  Decay alone adds no launch.
 *
 * aqg_optim: decoupled; weight_decay = HOST array of num_tensors coefficients in the trainer's tensor order (NULL = no decay;
 *   num_tensors must then equal the trainer's tensor count: 14, 2 L + 8, 3 C + 4); max_grad_norm (0 = no clipping); grad_norm =
 *   device float(s) that receive the UNCLIPPED norm (NULL = not wanted; asking for it alone runs the norm without clipping);
 *   workspace / workspace_floats = device floats for the partials, aqg_optim_workspace_floats(total gradient elements) of them
 *   (only looked at when a norm is taken).
 * aqg_optim_workspace_floats(n): partials for n elements at any 4-byte-aligned base; 0 = n is 0 or above 134,217,725.
 * aqg_grad_norm: out[0] = the L2 norm of x[0 .. n) (device f32, 4-byte aligned, n >= 1); reads nothing outside the buffer.
 * The six _optim entry points take the plain call's struct and arguments plus the controls.  optim == NULL, or a struct with every
 *   control off (no non-zero decay, max_grad_norm 0, grad_norm NULL), IS the plain call: the same launches.  Otherwise
 *   mode 0: gradients as always, never scaled; grad_norm[0], if given, receives their norm;
 *   mode 1: gradients, norm, update;   mode 2: norm of whatever grads holds (the all-reduced gradient under data parallelism), update.
 *   _steps: every step mode 1; step i writes grad_norm[i] (the caller provides one float per step).
 *   Refused on the host before any launch (-1, aqg_last_error), besides all the plain call refuses: a negative or non-finite decay,
 *   a num_tensors that is not the trainer's, a negative or non-finite max_grad_norm, and -- when a norm is taken -- a workspace that is
 *   NULL or too small, or grads[] that are not consecutive views of one flat buffer (grads[i + 1] == grads[i] + numel(i)). */
typedef struct aqg_optim {
    int32_t decoupled;
    int32_t num_tensors;
    const float* weight_decay;
    float max_grad_norm;
    float* grad_norm;
    float* workspace;
    size_t workspace_floats;
} aqg_optim;
size_t aqg_optim_workspace_floats(size_t n);
int aqg_grad_norm(const float* x, size_t n, float* out, float* workspace, size_t workspace_floats, void* stream);
int aqg_gcn_train_step_optim(const aqg_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                             const aqg_optim* optim, void* stream);
int aqg_gcn_train_steps_optim(const aqg_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                              const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim, void* stream);
int aqg_gcn_train_step_general_optim(const aqg_train_general* t_host, const uint8_t* states72, const float* pi_target,
                                     const float* z_target, int mode, const aqg_optim* optim, void* stream);
int aqg_gcn_train_steps_general_optim(const aqg_train_general* t_host, const uint8_t* states72, const float* pi_target,
                                      const float* z_target, const int64_t* order, long long positions, float* loss_sums,
                                      const aqg_optim* optim, void* stream);
int aqg_cnn_train_step_optim(const aqg_cnn_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                             const aqg_optim* optim, void* stream);
int aqg_cnn_train_steps_optim(const aqg_cnn_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                              const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim, void* stream);

/* ------------------------------------------------------------------ weight averaging (additive to ABI 15; the reference has none)
 *
 * An exponential moving average of the parameters, kept beside the three training steps above (csrc/weight_average.hip).  For a
 * decay d (float32, 0 <= d < 1) let w = float32(1.0 - (double)d), formed on the host.  An update of one element of the average e
 * from its source element p is
 *     e' = f32(d * e) + f32(w * p)
 * -- two f32 products and one f32 sum, each rounded, never contracted into a fused multiply-add.  On the CPU that is bit for bit
 * torch.optim.swa_utils.get_ema_avg_fn(float(d)), what AveragedModel applies.  The average starts as a copy of the parameters (the
 * caller makes it): no bias correction, no warm-up.  every = K: inside the steps an update is made behind the Adam update of every
 * step whose 1-based Adam step number (t.step, the number the bias corrections use) is a multiple of K -- the step number alone
 * decides, not where an epoch or a library call ends.
 *
 * One launch serves all tensors: a workgroup owns one chunk of AQG_WEIGHT_AVERAGE_CHUNK floats of one tensor, cut on the 16-byte grid
 * the AVERAGE's base sits in (tensor i with its average `mis` = 0..3 floats behind that grid has ceil((mis + numel) / CHUNK) chunks).
 * Where average and source sit alike on that grid, the words wholly inside the tensor are 16-byte accesses; any other float is taken
 * alone, each access guarded by the range: nothing outside either tensor is touched, and the source is only read.  No atomics.
 *
 * The tensor table is 4 T + 1 int64 words, T = num_tensors:
 *     [0, T) average pointers | [T, 2 T) source pointers | [2 T, 3 T) element counts | [3 T, 4 T] the prefix of the chunk counts
 * (prefix[0] = 0, prefix[T] = total_chunks).  The kernel reads `table`, on the device; the checks below read `host_table`, the same
 * words on the host (the caller keeps the two equal: a check that read the device copy would stop the stream at every call).
 *
 * aqg_weight_average_update: the launch alone, on `stream`.  Refused on the host before any launch (-1, aqg_last_error), the average
 *   untouched: a NULL struct or table (either copy); num_tensors < 1 or > AQG_WEIGHT_AVERAGE_MAX_TENSORS; a NULL or not 4-byte-aligned
 *   tensor; a tensor of fewer than 1 element; a chunk prefix or total_chunks that is not the one stated above, or more than 2^31 - 1
 *   chunks; decay outside [0, 1) or NaN; every < 1; any average range that overlaps any source range or another average range.
 * The six _avg entry points take the _optim call's arguments plus the average.  optim may be NULL: the plain step.  avg == NULL is the
 *   _optim call itself.  Otherwise the call refuses what aqg_weight_average_update refuses, in front of every launch, and enqueues the
 *   averaging launch on the same stream behind the finish / Adam launch of a step of mode 1 or 2 (mode 2: the data-parallel update;
 *   the empty-batch update included) whose step number is a multiple of `every`.  Mode 0 never averages.  No other launch changes. */
#define AQG_WEIGHT_AVERAGE_MAX_TENSORS 1024
#define AQG_WEIGHT_AVERAGE_CHUNK 4096
typedef struct aqg_weight_average {
    const int64_t* table;          /* device */
    const int64_t* host_table;     /* host: the same 4 T + 1 words */
    int32_t num_tensors;
    int32_t every;
    int64_t total_chunks;
    float decay;
} aqg_weight_average;
int aqg_weight_average_update(const aqg_weight_average* avg, void* stream);
int aqg_gcn_train_step_avg(const aqg_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                           const aqg_optim* optim, const aqg_weight_average* avg, void* stream);
int aqg_gcn_train_steps_avg(const aqg_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                            const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                            const aqg_weight_average* avg, void* stream);
int aqg_gcn_train_step_general_avg(const aqg_train_general* t_host, const uint8_t* states72, const float* pi_target,
                                   const float* z_target, int mode, const aqg_optim* optim, const aqg_weight_average* avg, void* stream);
int aqg_gcn_train_steps_general_avg(const aqg_train_general* t_host, const uint8_t* states72, const float* pi_target,
                                    const float* z_target, const int64_t* order, long long positions, float* loss_sums,
                                    const aqg_optim* optim, const aqg_weight_average* avg, void* stream);
int aqg_cnn_train_step_avg(const aqg_cnn_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                           const aqg_optim* optim, const aqg_weight_average* avg, void* stream);
int aqg_cnn_train_steps_avg(const aqg_cnn_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                            const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                            const aqg_weight_average* avg, void* stream);

/* ------------------------------------------------------------------ loss form (additive to ABI 15; the reference has one form)
 *
 * The policy loss of the three training steps above, as an option.  Per position b, with x the policy LOGITS, p = softmax(x) the
 * network's policy, t the target row, T = sum_a t_a (targets are not renormalised), v the tanh value, z its target, B the batch:
 *   policy_form 0, the reference's (train_network.py:54,85: CrossEntropyLoss applied to the ALREADY softmaxed policy):
 *       l_b = -sum_a t_a log_softmax(p)_a,   dlogit = p (.) (dp - p . dp),  dp = (softmax(p) T - t) / B
 *   policy_form 1, the cross-entropy between the target and softmax(x), taken from the logits:
 *       m = max x,  lse = m + ln sum_a exp(x_a - m),  l_b = T lse - sum_a t_a x_a,   dlogit_a = (softmax(x)_a T - t_a) / B
 *     -- loss and gradient of torch.nn.CrossEntropyLoss()(logits, t) with probability targets.  The loss is formed from the logits,
 *     never from ln p: a target entry on an action whose p underflows gives a finite term.  An all-zero target row gives l_b = 0 and
 *     a zero policy gradient.
 *   value term, both forms: (v - z)^2.  value_weight = w (finite, >= 0; 1 = the reference) scales its gradient,
 *       dvpre = w 2 (v - z) / B (1 - v^2),
 *     so that the loss minimised is Lp + w Lv.  Reported terms: loss[2 b] = l_b in the chosen form, loss[2 b + 1] = the UNWEIGHTED
 *     (v - z)^2 (the batch means and loss_sums likewise).
 * Form 1 runs inside the steps: a second instantiation of the fused 6/128/3 board kernels whose wave-0 section has no second
 * exponential round; in the general and CNN steps ONE kernel (policy_value_loss_kernel, csrc/gcn_train_general.hip) in place of the
 * loss launch and the heads' backward launch.  Form 0 with w != 1: the fused step's third instantiation; the general and CNN steps
 * keep their two launches and scale d loss / d value by w in one small launch between them.
 *
 * The six _loss entry points take the _avg call's arguments plus the form.  optim and avg may be NULL as there.  loss == NULL, or
 *   {0, 1.0f}, IS the _avg call: the same launches.  Modes 0 and 1 use the option; mode 2 (update only) does not look at it beyond
 *   the refusals.  Refused on the host before any launch (-1, aqg_last_error), besides all the _avg call refuses: a policy_form
 *   other than 0 or 1, a negative or non-finite value_weight.
 * aqg_policy_value_loss: form 1's kernel alone (policy_form must be 1).  B rows of A = 1 .. 4096 logits; the target row of position
 *   b is row order[first + b] (order NULL: first + b) of pi [.][A] and z [.]; writes loss [B][2], dlogits [B][A], dvpre [B] and
 *   nothing else.  One workgroup per row, sums in a fixed order, no atomics. */
typedef struct aqg_loss {
    int32_t policy_form;
    float value_weight;
} aqg_loss;
int aqg_policy_value_loss(int B, int A, const float* logits, const float* value, const float* pi, const float* z, const int64_t* order,
                          int first, const aqg_loss* loss_form, float* loss, float* dlogits, float* dvpre, void* stream);
int aqg_gcn_train_step_loss(const aqg_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                            const aqg_optim* optim, const aqg_weight_average* avg, const aqg_loss* loss_form, void* stream);
int aqg_gcn_train_steps_loss(const aqg_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                             const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                             const aqg_weight_average* avg, const aqg_loss* loss_form, void* stream);
int aqg_gcn_train_step_general_loss(const aqg_train_general* t_host, const uint8_t* states72, const float* pi_target,
                                    const float* z_target, int mode, const aqg_optim* optim, const aqg_weight_average* avg,
                                    const aqg_loss* loss_form, void* stream);
int aqg_gcn_train_steps_general_loss(const aqg_train_general* t_host, const uint8_t* states72, const float* pi_target,
                                     const float* z_target, const int64_t* order, long long positions, float* loss_sums,
                                     const aqg_optim* optim, const aqg_weight_average* avg, const aqg_loss* loss_form, void* stream);
int aqg_cnn_train_step_loss(const aqg_cnn_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target, int mode,
                            const aqg_optim* optim, const aqg_weight_average* avg, const aqg_loss* loss_form, void* stream);
int aqg_cnn_train_steps_loss(const aqg_cnn_train* t_host, const uint8_t* states72, const float* pi_target, const float* z_target,
                             const int64_t* order, long long positions, float* loss_sums, const aqg_optim* optim,
                             const aqg_weight_average* avg, const aqg_loss* loss_form, void* stream);

/* ------------------------------------------------------------------ training augmentation (additive to ABI 15; the reference has none)
 *
 * Quoridor is symmetric under the left-right mirror of the board: column y -> N - 1 - y in each player's own frame.  The mirror of a
 * state72 record: bytes 0 and 2 (the positions p) become (p / N) * N + (N - 1 - p % N); wall slot i < NW moves to
 * (i / W) * W + (W - 1 - i % W), W = N - 1, with its value; every other byte is copied.  The mirror of an action: a pawn action by the
 * position formula, a horizontal / vertical wall action by the slot formula inside its own block; a policy row is permuted
 * accordingly, out[mirror(a)] = in[a].  z is unchanged.  The map is an involution.  A position byte >= N * N has no image and is
 * copied through; no record byte is used as an address.
 *
 * aqg_augment_gather: the shuffle of an epoch and the flips in one launch (csrc/augment.hip).  Output row i < n is source row
 *   r = order[i] (order == NULL: r = i), mirrored iff the flip of r is set:
 *     flips != NULL: flips[r] != 0 (a u8 table indexed by SOURCE row);
 *     flips == NULL, use_seed != 0: f(K(seed, epoch), r) < 0.5 with K and f of the baseline agents' counter-based generator (below) --
 *       a row's orientation depends on (seed, epoch, source row) alone, never on the shuffle, the batch size or the rank;
 *       train_network.draw_mirror_flips(seed, epoch, rows) is the same function in numpy;
 *     neither: a plain gather.
 *   states72 [rows,72] u8 -> out72 [n,72]; pi [rows,policy_size] f32 -> out_pi [n,policy_size], copied as bit patterns; z [rows] f32 ->
 *   out_z [n].  Each input may be NULL together with its output (a states-only or policy-only mirror).  order entries are source rows
 *   the CALLER has checked against its row count; they are not checked here.  Errors: a board_size outside {3,5,7,9}, a policy_size
 *   that is not the board's A, n < 0, an input without its output or the reverse, an output that overlaps an input.  n == 0 returns 0
 *   without looking at the pointers.  The overlap check assumes of a source only what is certain -- n rows when order is NULL, one
 *   row when it is given, since the source's row count is not an argument -- so it never refuses a legitimate call; the outputs must
 *   lie outside the WHOLE source, and keeping them out of the rows behind that is the caller's part. */
int aqg_augment_gather(int board_size, int policy_size, const uint8_t* states72, const float* pi, const float* z, const int64_t* order,
                       const uint8_t* flips, int use_seed, uint64_t seed, uint64_t epoch, int n, uint8_t* out72, float* out_pi,
                       float* out_z, void* stream);

/* ------------------------------------------------------------------ replay window (additive to ABI 15; the reference trains on one file)
 *
 * A ring of training rows that stays on the device: three arrays of `capacity` rows, ring72 u8 [capacity,72], ring_pi f32 [capacity,A],
 * ring_z f32 [capacity] -- what the trainers' entry points read.  Which slots hold rows, and of which generation, is the host's
 * bookkeeping (replay.py).
 *
 * aqg_replay_append: one launch (csrc/replay.hip) writes source row i, 0 <= i < n, into ring slot (head + i) % capacity.
 *   The 72 record bytes are copied verbatim; no byte is interpreted or used as an address.
 *   Counts form (visits and z_i8 given, pi and z_f32 NULL) -- a generation as the engine leaves it (hist_visits, read as UNSIGNED
 *     16-bit, and the i8 outcomes): tot = the exact integer sum of the row's A counts; ring_pi[j] = f32(f64(v_j) / f64(tot)), and A
 *     zeros when tot == 0; ring_z = (float)z.  Those are the bits of the .history route (v / tot in float64, then
 *     torch.tensor(..., dtype=float32)).  The kernel takes the correctly rounded f32 quotient f32(v_j) / f32(tot), which has the same
 *     bits for every tot < 2^24 (A * 65,535 is below that): an integer quotient this small is neither an f32 midpoint nor within 2^-53
 *     relative of one, so rounding once or twice agrees.  The unit is never built with a fast-math flag.
 *   Rows form (pi and z_f32 given, visits and z_i8 NULL) -- finished rows, e.g. of a .history file: a plain copy into the ring.
 *   Refused on the host, before any launch (-1, aqg_last_error): an unsupported board size, a policy_size that is not the board's A,
 *   n < 0, capacity < 1, head outside 0 .. capacity - 1, n > capacity, neither or both forms (or half of one), states72 or a ring
 *   NULL, a ring (capacity rows) that overlaps a source (n rows).  n == 0 returns 0 without looking at the pointers. */
int aqg_replay_append(int board_size, int policy_size, const uint8_t* states72, const uint16_t* visits, const int8_t* z_i8,
                      const float* pi, const float* z_f32, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                      float* ring_z, void* stream);
/* The counts form with a blended value target (additive to ABI 15): the same kernel under a template switch, same geometry, one
 * launch.  search_value f32 [n] is the search value the engine recorded beside each row (hist_value above); the lanes that write
 * ring_z load it and write
 *     ring_z = keep * (float)z + blend * v,   keep = 1.0f - blend
 * in f32 without contraction: one subtraction, two products and one sum, each rounded (replay.blend_targets is the same in numpy).
 * blend 0 writes the bits of the plain append for every finite v; blend 1 writes 0 * z + v, which is v (a zero may change its
 * sign).  ring72 and ring_pi are written
 * exactly as the plain append writes them.  Refused, besides everything the plain append refuses of the counts form: a blend outside
 * [0, 1] or NaN, search_value NULL (with n > 0), search_value (n values) overlapping a ring. */
int aqg_replay_append_blend(int board_size, int policy_size, const uint8_t* states72, const uint16_t* visits, const int8_t* z_i8,
                            const float* search_value, float blend, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                            float* ring_z, void* stream);

/* ------------------------------------------------------------------ reanalyse (additive to ABI 15; the reference has none)
 *
 * aqg_replay_refresh: one launch (csrc/replay_refresh.hip) overwrites the targets of chosen ring slots with fresh search results.
 * Source row i, 0 <= i < n, is a searched root as aqg_engine_root_visits writes it: visits [n,AQG_MAX_LEGAL] i32 and actions
 * [n,AQG_MAX_LEGAL] u8 in legal_actions() order, count [n] i32 their number.  With c = count[i] and tot = the integer sum of
 * visits[i][0 .. c):
 *   - c <= 0, c > AQG_MAX_LEGAL, tot <= 0 or slots[i] outside [0, capacity): the row is skipped and the ring is not touched for it;
 *   - otherwise the WHOLE policy row of slot slots[i] is written once: f32(visits[i][j]) / f32(tot) at actions[i][j] for j < c, 0.0f
 *     everywhere else.  The quotient is the correctly rounded f32 division of aqg_replay_append, with the bits of
 *     f32(f64(v) / f64(tot)) for tot < 2^24; counts are >= 0 and their total below 2^24 (the caller's part: the engine's simulation
 *     cap sees to it), and the unit is never built with a fast-math flag.  An action byte >= policy_size inside the count is dropped;
 *     the ids of one row are distinct, as a legal list's are (of a repeated id one quotient is kept).  No input byte is used as an
 *     address unguarded.
 *   - with search_value (f32 [n], aqg_engine_root_values) and blend != 0:
 *         ring_z[slot] = keep * ring_z[slot] + blend * search_value[i],   keep = 1.0f - blend
 *     in f32 without contraction -- two products and one sum, each rounded, as aqg_replay_append_blend's.  The blend acts on the value
 *     the ring holds NOW, which may already be a blend (of an append with a blend, or of an earlier refresh): refreshing a row k times
 *     leaves keep^k of its first value target.  search_value NULL or blend 0: ring_z is neither read nor written (and may be NULL).
 * slots [n] i64 are distinct (the caller's part, replay.ReplayWindow.refresh_counts checks it); the ring's record bytes are not an
 * argument and are never touched.  No atomics; every output row is stored once, lane-contiguous.
 * Refused on the host, before any launch (-1, aqg_last_error): an unsupported board size, a policy_size that is not the board's A,
 * n < 0, capacity < 1, a blend outside [0, 1] or NaN, a blend != 0 without search_value, and with n > 0: visits, actions, count,
 * slots or ring_pi NULL, ring_z NULL with a blend, a ring (capacity rows) that overlaps a source (n rows) or the other ring.
 * n == 0 returns 0 without looking at the pointers.  replay.refresh_reference is the same in numpy. */
int aqg_replay_refresh(int board_size, int policy_size, const int32_t* visits, const uint8_t* actions, const int32_t* count,
                       const float* search_value, float blend, const int64_t* slots, int n, int capacity, float* ring_pi,
                       float* ring_z, void* stream);

/* ------------------------------------------------------------------ completed-Q policy targets (additive to ABI 15; the reference has none)
 *
 * The improved policy of "Policy improvement by planning with Gumbel" (Danihelka et al., ICLR 2022, section 4 and appendix D),
 *     pi' = softmax(log p + sigma(completedQ)),
 * as a policy target besides the normalised visit counts: a policy improvement at any simulation count, non-zero on unvisited
 * actions, smooth in the values, and a function of the root's child block alone -- the step kernels, the captured per-move graph and
 * the engine struct are untouched.
 *
 * The definition.  For a root (node 0 of a slot's pool) with cnt children i = 0 .. cnt-1 in legal_actions() order, read as their
 * records hold them: p_i f32 (the priors the root was built from: the mixed ones with root noise on), n_i i32, q_i f32 = f32(-w_i / n_i)
 * from the root mover's side (0 while n_i == 0), w_i f64, and the root's own w.  All arithmetic is float64 without contraction;
 * values are rounded to f32 only where stated.
 *   1. Nsum = sum n_i, nmax = max(0, max n_i): integers.
 *   2. vhat = root.w + sum_i w_i -- the root's own network value: a backup adds each simulation's value to a child and its negation to
 *      the root, and simulation 0 adds vhat to the root alone, so the identity is exact up to f64 rounding.
 *   3. With V = {i : n_i > 0}, PV = sum_{i in V} p_i and QV = sum_{i in V} p_i q_i:
 *          vmix = (vhat + Nsum * (QV / PV)) / (1 + Nsum)   if PV > 0,   else vmix = vhat.
 *   4. c_i = q_i if n_i > 0, else vmix.
 *   5. sigma_i = ((c_visit + nmax) * c_scale) * ((c_i + 1) / 2): the values lie in [-1, 1] and the fixed affine map to [0, 1] is the
 *      paper's setting (no min-max rescaling).
 *   6. x_i = log(p_i) + sigma_i for p_i > 0; an entry with p_i <= 0 or NaN is excluded and gets pi'_i = 0.  m = max x_i,
 *      e_i = exp(x_i - m), pi'_i = f32(e_i / sum e).  f32(vmix) is returned too.
 *   7. A root with cnt == 0 or without a p_i > 0 gets an all-zero row (its vmix is still the one above: vhat for cnt == 0).  A root
 *      with cnt > AQG_MAX_LEGAL, or whose child range leaves the pool (first + cnt > node_cap: checked before it is used as an
 *      address), gets the zero row: count 0, actions 0xFF, vmix 0.  Rows are zero past cnt.
 * The sums and maxima are wave reductions and log / exp are the device library's, so the outputs are not the bits of another
 * evaluation order: every f64 intermediate is good to far better than 2^-40 relative, so an f32 output differs from
 * engine.improved_policy_reference (the same in numpy) at most by landing on the other side of a rounding boundary -- one f32 ulp,
 * plus for vmix the absolute floor (cnt + 1) * (Nsum + 1) * 2^-53 of the cancellation in vhat.
 *
 * aqg_engine_root_improved_policy: one launch (csrc/mcts_improve.hip), one wavefront per slot, no LDS, no atomics.  policy
 *   [G,AQG_MAX_LEGAL] f32, actions [G,AQG_MAX_LEGAL] u8 and count [G] i32 in the layout of aqg_engine_root_visits (0 and 0xFF past the
 *   count), vmix [G] f32.  Valid after a search and in front of a finish-move, on every evaluator and with tree reuse (a kept root
 *   satisfies the same identity).  The paper's board-game constants are c_visit = 50, c_scale = 1.  Refused before the launch: a NULL
 *   argument, c_visit or c_scale negative or not finite.
 * aqg_replay_refresh_policy: aqg_replay_refresh with finished f32 policy entries for the source -- policy [n,AQG_MAX_LEGAL] f32 as the
 *   entry above writes it -- copied VERBATIM to their action ids over a zero row: no total, no division, so the launch is bit for bit
 *   replay.refresh_policy_reference.  Geometry, staging, fences, the slot and action guards, the refusals and the blend are
 *   aqg_replay_refresh's.  A row is written iff 1 <= count <= AQG_MAX_LEGAL, the slot is inside the ring, every entry j < count is
 *   finite and >= 0 and at least one is > 0 -- pure predicates, wave-uniform by ballot: no sum is involved, so the decision does not
 *   depend on an order.  (An entry whose action byte is >= policy_size is dropped but counts in these predicates.) */
int aqg_engine_root_improved_policy(const aqg_engine* e_host, double c_visit, double c_scale, float* policy, uint8_t* actions,
                                    int32_t* count, float* vmix, void* stream);
int aqg_replay_refresh_policy(int board_size, int policy_size, const float* policy, const uint8_t* actions, const int32_t* count,
                              const float* search_value, float blend, const int64_t* slots, int n, int capacity, float* ring_pi,
                              float* ring_z, void* stream);

/* ------------------------------------------------------------------ recording completed-Q targets during self-play (additive to ABI 15)
 *
 * The same target for the rows a generation itself produces: an f32 history beside hist_visits, written move by move.  Off by
 * default; with the option off every call launches what it launched before.  The engine struct, the step kernels and the captured
 * per-move graph (and its cache key) are untouched: the option is a struct beside the engine's, like tree reuse and resignation,
 * and one launch outside the graph.
 *
 * The row.  hist_policy f32 [quota, max_plies, A], indexed like hist_visits: row (k, ply) is the improved policy pi' of the section
 * above (steps 1 .. 7, with this struct's c_visit and c_scale) of the root the move at ply `ply` of game k was searched from,
 * scattered DENSE by action id -- pi'_i at action_i for i < cnt, 0.0f everywhere else.  An action byte >= A is dropped; a root
 * without children, or one that fails step 7's guard, gives the zero row.  With root noise on, the root's stored priors are the
 * mixed ones and the row is softmax(log p_mixed + sigma); the noise is not taken out again.
 *
 * The launch (csrc/mcts_record.hip, engine_record_improved_policy_kernel): one wavefront per slot, four per workgroup, the
 * arithmetic of aqg_engine_root_improved_policy in the same device function (csrc/mcts_improve_row.hpp) -- so a recorded row is that read-out scattered, bit for
 * bit.  It acts on a slot g with game_active[g] set, k = slot_game[g] inside [0, quota) and ply = game_plies[k] inside [0, max_plies):
 * the indices the finish-move launch uses for hist_visits.  The whole row is written, every address once, 64 consecutive floats per
 * store, staged through LDS per wavefront; no other byte of hist_policy is touched.  Rows of aqg_engine_apply_actions are never
 * written: in a zeroed buffer they read 0, like hist_value's.
 *
 * aqg_engine_move_policy / aqg_engine_finish_move_policy: aqg_engine_move_resign / aqg_engine_finish_move_resign with the option as
 *   one more argument; here reuse, resign and policy may each be NULL (= that option off).  The record launch goes behind the last
 *   step of the move's search and in front of the finish-move launch, on the same stream: the move is still chosen from the visit
 *   counts, hist_visits is still written, and no game changes.
 * aqg_engine_record_improved_policy: the launch alone.
 * Refused before any launch, behind everything the move refuses: hist_policy NULL, max_plies == 0, c_visit or c_scale negative or
 * not finite. */
typedef struct aqg_policy_record {
    double c_visit;      /* finite, >= 0 */
    double c_scale;      /* finite, >= 0 */
    float* hist_policy;  /* [quota, max_plies, A] */
} aqg_policy_record;
int aqg_engine_move_policy(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                           const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy, void* stream);
int aqg_engine_finish_move_policy(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                  const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy, void* stream);
int aqg_engine_record_improved_policy(const aqg_engine* e_host, const aqg_policy_record* policy, void* stream);
/* aqg_replay_append_policy: the hand-over of such rows to the ring -- aqg_replay_append's kernel and geometry, one launch, with the
 *   policy of the rows form (pi f32 [n,A], copied verbatim) and the outcome of the counts form (z_i8): ring_z = (float)z, or with
 *   search_value != NULL aqg_replay_append_blend's uncontracted keep * (float)z + blend * v.  The 72 record bytes are copied verbatim.
 *   Refused: everything aqg_replay_append refuses, pi or z_i8 NULL (with n > 0), a blend outside [0, 1] or NaN, a blend != 0 without
 *   search_value, search_value overlapping a ring.  replay.append_reference(policy=) is the same in numpy. */
int aqg_replay_append_policy(int board_size, int policy_size, const uint8_t* states72, const float* pi, const int8_t* z_i8,
                             const float* search_value, float blend, int n, int capacity, int head, uint8_t* ring72, float* ring_pi,
                             float* ring_z, void* stream);

/* ------------------------------------------------------------------ position merge (additive to ABI 15; the reference has none)
 *
 * Rows of (states72, pi, z) that hold the same position merged into one row with the mean targets (csrc/replay_merge.hip;
 * replay.merge_positions drives the three entry points, replay.merge_reference states them in numpy).  The KEY BYTES of a record are
 * bytes 0..67 and 70: two rows hold the same position iff their key bytes are equal; bytes 68-69 (the ply counter) and 71 (spare)
 * never matter.  perm, index and starts hold rows and places the CALLER has checked; they are not checked here.  Every entry refuses
 * on the host, before any launch (-1, aqg_last_error), and returns 0 for n == 0 without looking at a pointer.  Of a gathered source
 * the overlap checks assume one row, as aqg_augment_gather does.
 *
 * aqg_replay_position_keys: keys[i] = the 64-bit hash of the key bytes of row index[i] (index == NULL: row i), 0 <= i < n:
 *   h = sum over the key bytes k of (b_k + 1) * (splitmix64(k) | 1) mod 2^64, keys[i] = splitmix64(h) (replay.position_keys).  A single
 *   changed key byte always changes the key.  The hash only groups rows for the sort; nothing is merged on it.
 *   Refused: n < 0, states72 or keys NULL, keys overlapping states72 or index.
 * aqg_replay_run_heads: heads[i] = 1 iff i == 0 or the key bytes of row perm[i] differ from those of row perm[i - 1], else 0 -- a full
 *   compare, so two positions with one hash split a run and never merge.  Refused: n < 0, a NULL array, heads overlapping a source.
 * aqg_replay_merge_runs: output row o < u is the run of rows perm[starts[o]], ..., perm[starts[o + 1] - 1] (starts[u] = n; starts is
 *   increasing from 0): out72 = the run's FIRST row's 72 bytes verbatim, count = its length L, out_pi / out_z = the mean of its policy
 *   rows / values in f32.  L == 1 is a bit-for-bit copy.  Summation order, a function of L and the order within the run alone: chunks of
 *   64 rows, each summed left to right from its first row; the chunk sums summed left to right; then the correctly rounded division by
 *   (float)L.  A term passes through at most min(L, 64) - 1 + ceil(L / 64) - 1 additions.  No atomics.  Chunks of runs longer than 64
 *   rows are summed by a launch of their own in front (into `workspace`), so that a run of thousands of rows is read by many wavefronts.
 *   workspace: aqg_replay_merge_workspace_floats(board_size, n, u) floats -- 0 when n - u < 64 (no run can be longer than one chunk;
 *   workspace may then be NULL), else 2 * ceil(n / 64) * (A + 1).
 *   Refused: an unsupported board size, a policy_size that is not the board's A, n < 0, u < 0, u > n, u == 0 with n > 0, a NULL array,
 *   a workspace that is needed and NULL or too small, an output (u rows; the workspace) that overlaps a source or another output. */
int aqg_replay_position_keys(const uint8_t* states72, const int64_t* index, int n, int64_t* keys, void* stream);
int aqg_replay_run_heads(const uint8_t* states72, const int64_t* perm, int n, uint8_t* heads, void* stream);
size_t aqg_replay_merge_workspace_floats(int board_size, int n, int u);
int aqg_replay_merge_runs(int board_size, int policy_size, const uint8_t* states72, const float* pi, const float* z, const int64_t* perm,
                          const int64_t* starts, int n, int u, uint8_t* out72, float* out_pi, float* out_z, int32_t* count,
                          float* workspace, size_t workspace_floats, void* stream);

/* ------------------------------------------------------------------ policy surprise weighting (additive to ABI 15; the reference has none)
 *
 * Which rows an update trains on, drawn by how far the network is from each row's policy target (csrc/replay_surprise.hip;
 * replay.surprise_index drives the two entry points, replay.surprise_reference and replay.surprise_counts_reference state them in
 * numpy).  For the m rows an update trains on (index[0..m), or rows 0..m-1 of the arrays), t a row's f32 policy target [A] and p the
 * f32 softmaxed policy the network the update STARTS from gives for the row's record:
 *
 * 1. Surprise, in float64, no operation contracted:  KL = sum over {a : t_a > 0} of t_a * (ln t_a - ln max(p_a, 2^-126)).
 *    Summation order: lane l of 64 adds its own entries a = l, l + 64, ... in ascending order to +0.0 (an entry with t_a <= 0 adds
 *    nothing), then the xor-shuffle wave reduction 32, 16, ..., 1 (v_l += v_{l xor off}).  k = f32(min(max(KL, 0), 88)); the upper
 *    clamp never acts on a row whose target sums to 1 (KL <= 126 ln 2 = 87.34) and keeps q below 2^27 whatever a row holds.
 *    k = 0 for a row with a non-finite entry in t or p, a negative target entry (-0.0 is not one), no positive target entry, or an
 *    index entry outside the arrays (such a row is not read).  t == p bitwise gives k = 0 exactly.
 * 2. Integer weight: q = floor(k * 2^20) -- an exact f64 product, q < 2^27.  S = sum q is an exact integer whatever the order; m <=
 *    2^24 (more is refused), so S < 2^51.
 * 3. Expected copies for an update that wants E rows with uniform share U, in float64 in this order:
 *    f = (E * U) / m + ((E * (1 - U)) * q) / S  when S > 0,  f = E / m  when S <= 0.  U = 1, E = c m gives f = c exactly.
 * 4. Copies: count = min(floor(f) + [u < f - floor(f)], C), u = counter_uniform(stream_key(seed, update), r) of the generator above,
 *    r the row's place in the arrays (index[j], or j) -- for a replay window the ring slot -- so a row's draw does not depend on m, on
 *    the chunking or on the rank.  C = the most copies of one row, 1..255.
 * 5. The update's index: the rows in input order, row j count_j times (torch.repeat_interleave; no kernel).
 *
 * aqg_replay_surprise_rows: steps 1 and 2 for one chunk of n rows whose network policy the caller has just computed -- net_policy f32
 *   [n,A], row i of the chunk being training row offset + i: its target is row index[offset + i] of ring_pi f32 [rows,A] (index ==
 *   NULL: row offset + i), its results go to k[offset + i] (f32) and q[offset + i] (i32); index, k and q have m entries.  16 rows per
 *   workgroup, 4 per wavefront, all their loads in flight before the first use; no LDS, no atomics, no scratch.
 *   Refused: an unsupported board size, a policy_size that is not the board's A, m < 0 or m > 2^24, rows < 0, m > rows without an
 *   index, a chunk outside the m rows (offset < 0, n < 0, offset + n > m), a NULL array (with n > 0), an output overlapping a source
 *   (of a gathered ring one row is assumed, as aqg_augment_gather does) or the other output.
 * aqg_replay_surprise_counts: steps 3 and 4, one lane per row: q i32 [m], index i64 [m] or NULL, total = a DEVICE int64 holding S
 *   (the caller's exact integer sum of q; it is read by the kernel, never by the host), count i32 [m].
 *   Refused: m < 0 or m > 2^24, uniform_share outside [0, 1] or NaN, max_copies outside 1..255, expected_rows < 1 (or > 2^40), q,
 *   total or count NULL (with m > 0), count overlapping a source.
 * Both refuse on the host, before any launch (-1, aqg_last_error), and return 0 for an empty launch without looking at a pointer. */
int aqg_replay_surprise_rows(int board_size, int policy_size, const float* net_policy, const float* ring_pi, const int64_t* index,
                             int rows, int m, int offset, int n, float* k, int32_t* q, void* stream);
int aqg_replay_surprise_counts(const int32_t* q, const int64_t* index, const int64_t* total, int m, long long expected_rows,
                               double uniform_share, int max_copies, uint64_t seed, uint64_t update, int32_t* count, void* stream);

/* ------------------------------------------------------------------ row metrics (additive to ABI 15; the reference has no held-out set)
 *
 * What a network scores on rows no update trains on, under one fixed definition (csrc/row_metrics.hip; validation.row_metrics and
 * validation.holdout_split drive the entry points, replay.row_metrics_reference, replay.row_metrics_reduce_reference and
 * replay.holdout_reference state them in numpy).  A row has a policy target t (f32 [A]) and a value target z (f32), the ply
 * ply = rec[68] | rec[69] << 8 of its record, and the network's softmaxed policy p (f32 [A]) and tanh value v (f32) of that record.
 * Everything below is float64 from the f32 inputs, no operation contracted:
 *
 *   ce  = -sum over {a : t_a > 0} of t_a * ln max(p_a, 2^-126)       the true cross-entropy
 *   ent = -sum over {a : t_a > 0} of t_a * ln t_a                    the target's entropy; KL = ce - ent is formed by the caller
 *   lp  = (sum_a t_a) * ln(sum_b exp(p_b)) - sum_a t_a p_a           the trainers' policy loss term (gcn_train_heads.hpp: the
 *                                                                    reference's double softmax), so that the held-out number
 *                                                                    compares with the line the loop prints
 *   se  = (v - z)^2, the difference and the square in float64: exact up to one rounding
 *   hit = 1 iff t[a*] == max_a t, a* the first maximum of p (the least index whose p equals the maximum): tied targets all count
 *   the value sign is counted iff z != 0; it agrees iff (double)v * (double)z > 0
 *   bucket = min(ply / bucket_plies, buckets - 1), 1 <= buckets <= 64, bucket_plies >= 1
 *   A row is REJECTED -- it contributes to no sum and is counted in the extra bucket `buckets` -- if t, p, v or z has a non-finite
 *   entry, t has a negative entry (-0.0 is not one), t has no positive entry, or its index entry is outside the ring (such a row is
 *   not read).
 *
 * Summation order of a row: lane l of 64 adds its own entries a = l, l + 64, ... in ascending order to +0.0 (an entry that adds
 * nothing adds +0.0), then the xor-shuffle wave reduction 32, 16, ..., 1 -- five sums: S_ce = sum t ln max(p, 2^-126) and S_ent = sum
 * t ln t over t > 0, S_t = sum t, S_e = sum exp(p), S_tp = sum t p over all entries; ce = 0 - S_ce, ent = 0 - S_ent, lp = S_t *
 * ln(S_e) - S_tp (a product, then a difference).  The first maximum is the wave maximum of the value, then the least index among the
 * entries that hold it.
 *
 * aqg_replay_row_metrics: one chunk of n rows whose network outputs the caller has just computed -- net_policy f32 [n,A] and net_value
 *   f32 [n], row i of the chunk being row offset + i of the m: its targets and record are row index[offset + i] of ring_pi f32
 *   [rows,A], ring_z f32 [rows] and states72 u8 [rows,72] (index == NULL: row offset + i); vals[offset + i] = {ce, ent, lp, se} (f64
 *   [m,4]; zeros for a rejected row) and tag[offset + i] (i32 [m]) = bucket in bits 0-7 (`buckets` for a rejected row), hit in bit 8,
 *   sign counted in bit 9, sign agrees in bit 10.  The geometry is aqg_replay_surprise_rows': 16 rows per workgroup, 4 per wavefront,
 *   all their loads in flight before the first use; no LDS, no atomics, no scratch.
 *   Refused: an unsupported board size, a policy_size that is not the board's A, m < 0 or m > 2^24, rows < 0, m > rows without an
 *   index, a chunk outside the m rows, buckets outside 1..64, bucket_plies < 1, a NULL array (with n > 0), an output overlapping a
 *   source (of a gathered ring one row is assumed) or the other output.  n == 0 returns 0 without looking at a pointer.
 * aqg_row_metrics_reduce: sums f64 [buckets+1,4] = the sums of vals per bucket, counts i64 [buckets+1,4] = rows, hits, signs counted,
 *   signs agreeing per bucket (exact); row `buckets` of both is the rejected rows' (its sums are zeros).  A fixed-order sum without
 *   atomics, two launches: (1) workgroup (c, b) of 256 lanes takes the 4,096 rows of chunk c; lane l adds the rows l, l + 256, ... in
 *   ascending order whose tag names bucket b to +0.0; wave_xor_sum; the four wave results added in wave order ((w0 + w1) + w2) + w3;
 *   partial[c][b] stored.  (2) one wavefront per bucket adds the chunk partials lane, lane + 64, ... ascending to +0.0, then
 *   wave_xor_sum.  partial: aqg_row_metrics_workspace_doubles(m, buckets) doubles = ceil(m / 4096) * (buckets + 1) * 8 (0 for m == 0 or
 *   an argument out of range).  m == 0 stores zero tables and needs neither vals, tag nor partial.
 *   Refused: m < 0 or m > 2^24, buckets outside 1..64, sums or counts NULL, vals, tag or partial NULL with m > 0, an output
 *   overlapping a source or another output.
 * aqg_replay_holdout_mask: mask[i] (u8) = counter_uniform(stream_key(seed, AQG_HOLDOUT_STREAM), (uint64)keys[i]) < share, one lane per
 *   row; keys i64 [n] from aqg_replay_position_keys, so a position lands on one side under a seed wherever and however often it
 *   occurs.  Refused: n < 0, share outside (0, 1) or NaN, keys or mask NULL (with n > 0), mask overlapping keys.
 * All three refuse on the host, before any launch (-1, aqg_last_error). */
#define AQG_HOLDOUT_STREAM 0x686F6C646F7574ull      /* "holdout": the sub-stream of a seed that splits positions */
int aqg_replay_row_metrics(int board_size, int policy_size, const float* net_policy, const float* net_value, const uint8_t* states72,
                           const float* ring_pi, const float* ring_z, const int64_t* index, int rows, int m, int offset, int n,
                           int bucket_plies, int buckets, double* vals, int32_t* tag, void* stream);
size_t aqg_row_metrics_workspace_doubles(int m, int buckets);
int aqg_row_metrics_reduce(const double* vals, const int32_t* tag, int m, int buckets, double* partial, double* sums, int64_t* counts,
                           void* stream);
int aqg_replay_holdout_mask(const int64_t* keys, int n, uint64_t seed, double share, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------ start positions (additive to ABI 15; the reference starts every game from the opening)
 *
 * Games that start from caller-given records: opening books, paired matches, forks of recorded positions.  Off by default: without
 * a table every call launches what it launched before.  The engine struct, the ABI number, the step kernels, the captured per-move
 * graph and its key do not change: the table is a struct beside the engine's, an argument of the reset and refill launches.
 *
 * The checker (csrc/state_check.hip; one predicate on the rule header, compiled for the device and for the host).  flags[i] == 0:
 * record i may start a game.  Bits:
 *   AQG_CHECK_BOARD        byte 70 is not board_size, or a pawn cell is >= N*N
 *   AQG_CHECK_WALLS        a wall byte > 2 among the first (N-1)^2, or two walls that overlap: two horizontal walls in neighbouring
 *                          slots of one row, or two vertical walls in neighbouring slots of one column (what can_place_wall refuses,
 *                          game_logic.py:199-223)
 *   AQG_CHECK_WALL_COUNT   a walls-left byte > num_walls, or player_left + enemy_left + placed != 2 * num_walls; placed = the wall bytes
 *                          that are 1 or 2 (a byte > 2 is no wall)
 *   AQG_CHECK_SAME_SQUARE  both pawns on one square: ppos == N*N - 1 - epos
 *   AQG_CHECK_OVER         the game is over: is_lose (epos / N == 0), the mover on its own goal row (ppos / N == 0), plies >= plies_for_draw
 *   AQG_CHECK_ODD_PLY      the ply counter is odd.  history z, the resignation side and the match loops take the side from a game's own
 *                          ply index; game_result takes it from the record.  With an even start they agree, so a start must be even.
 *   AQG_CHECK_NO_PATH      a pawn has no path to its goal row through the walls: the fill of the wall-legality search with no candidate
 *                          wall and the other pawn taken off the board.  (With the other pawn as an obstacle, positions of real games
 *                          would be flagged: a wall is legal while both jump-aware paths exist, but a pawn may later step into the
 *                          other's only corridor.  The path through the walls alone is what the rules keep invariant.)
 *                          Evaluated only when BOARD, WALLS and SAME_SQUARE are clear, else 0
 * Bytes past the board's wall slots and byte 71 are not read; nothing outside the record is read; every index formed from a record
 * byte is bounded first; no atomics; every loop is bounded by a constant of N.  Reachability from the opening is NOT a condition.
 *   aqg_states72_check     device: states72 u8 [B,72], flags u8 [B]; one thread per record.  Refused: an unsupported board size, B < 0,
 *                          a NULL array with B > 0, num_walls outside 0..127, plies_for_draw outside 0..65535.
 *   aqg_host_check_state   the same byte for one record in HOST memory; -1 for a NULL record, an unsupported board size or a constant
 *                          outside those ranges.  game_logic.check_state_reference is the statement in numpy.
 *
 * The table.  Game k -- the engine's game index, slot_game -- starts from row index ? index[k] : k % count of states72 u8 [count,72]
 * (device); index i32 [quota] (device) or NULL.  A game's start is a function of its game index alone, never of slot, refill order or
 * set count.  The caller has run the rows through the checker and the index through a range check: the entry points refuse a NULL
 * states72 and count < 1 only, and the kernels start a game whose row number is outside [0, count) from the opening record.
 * engine_reset_kernel / engine_refill_kernel (csrc/mcts_move.hip) take the table under a template switch:
 * store_state(root_state, g, unpack72(row)) replaces the initial_state store and nothing else changes; the plain instantiations are
 * the kernels as they were.  The table is only read.
 * Everything per game keeps counting plies played in THIS game: game_plies and the history rows as always, and with a table the
 * finish-move launch (its GAME_PLY instantiation) compares temperature_plies and resign min_ply with game_plies[k] instead of the
 * record's counter -- from the opening the two are one number.  The root-noise key of a move stays (seed, game, the record's ply
 * counter): it is formed inside the captured graph, which does not change, and it is still unique per game and ply.  The draw rule
 * reads the record's own counter: a start at ply p has plies_for_draw - p plies left and fits the existing history.
 *   aqg_engine_reset_start          aqg_engine_reset with the table (NULL = aqg_engine_reset)
 *   aqg_engine_move_start / aqg_engine_finish_move_start   aqg_engine_move_policy / aqg_engine_finish_move_policy with the table as one
 *                                   more nullable pointer: the refill behind the move starts its games from it
 *   aqg_engine_apply_actions_start  aqg_engine_apply_actions, likewise */
#define AQG_CHECK_BOARD 1
#define AQG_CHECK_WALLS 2
#define AQG_CHECK_WALL_COUNT 4
#define AQG_CHECK_SAME_SQUARE 8
#define AQG_CHECK_OVER 16
#define AQG_CHECK_ODD_PLY 32
#define AQG_CHECK_NO_PATH 64
int aqg_states72_check(int board_size, const uint8_t* states72, int B, int num_walls, int plies_for_draw, uint8_t* flags,
                       void* stream);
int aqg_host_check_state(int board_size, const uint8_t* rec72_host, int num_walls, int plies_for_draw);
typedef struct aqg_start_table {
    const uint8_t* states72;        /* [count, 72] checked records */
    const int32_t* index;           /* [quota] row of every game, or NULL = game k starts from row k % count */
    int32_t count;                  /* >= 1 */
} aqg_start_table;
int aqg_engine_reset_start(const aqg_engine* e_host, const aqg_start_table* start, void* stream);
int aqg_engine_move_start(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                          const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy,
                          const aqg_start_table* start, void* stream);
int aqg_engine_finish_move_start(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                 const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy,
                                 const aqg_start_table* start, void* stream);
int aqg_engine_apply_actions_start(const aqg_engine* e_host, const int32_t* actions, const aqg_start_table* start, void* stream);

/* ------------------------------------------------------------------ Gumbel root search
 * The other half of "Policy improvement by planning with Gumbel" (Danihelka et al., ICLR 2022; the completed-Q target above is the
 * first): the root samples m actions without replacement (Gumbel top-m), spends the simulations on them by sequential halving and
 * plays the survivor with the largest g + logit + sigma(q).  Below the root the search is the reference's PUCT, untouched.  Off (a
 * NULL aqg_gumbel*) every entry point launches what it always launched.  The engine struct and AQG_ABI_VERSION stay.
 * A root has cnt children in legal_actions() order with stored priors p_i; `sims` is the engine's simulation count (>= 2 with the
 * option): simulation 0 evaluates the root, so the root is selected from sims - 1 times.
 * 1. Gumbel logits.  gl_i = f32(scale * g_i + log(p_i)), formed in float64 without contraction and rounded once; gl_i = -inf where
 *    p_i is not > 0 (NaN included).  g_i: table mode (table != NULL) g_i = table[g][i], a non-finite entry reads 0; generator mode
 *    u = f(key, 0) of the counter generator above, e = -log(1 - u), e = DBL_MIN if that is 0, g_i = -log(e), with
 *    key = K(K(K(seed, k), ply), i), k = slot_game[g] (the GAME's index; the slot in the search-only entry point) and ply the root
 *    record's counter -- root noise's keying, so a game's variates do not depend on slot, refill or set count.
 *    m_g = min(considered, number of children with gl_i > -inf).
 * 2. The visit schedule T[m'][0 .. sims - 2], m' = 0 .. considered: the considered visit counts of sequential halving.  m' <= 1:
 *    T[m'][j] = j.  Otherwise L = ceil(log2 m'), visits = [0] * m', k = m'; until sims - 1 entries exist: x = max(1, floor((sims - 1) /
 *    (L * k))); x times: append visits[:k], then add 1 to each of visits[:k]; then k = max(2, k / 2).  Cut to sims - 1 entries.  Built
 *    on the host (gumbel.considered_visits), uploaded once: schedule[m' * (sims - 1) + j].
 * 3. Root selection of simulation s = 1 .. sims - 1.  v = T[m_g][s - 1]; n_i, q_i = the children's visit counts and stored q after
 *    every earlier simulation's backup; nmax = max_i n_i.  In float32, left to right, no contraction:
 *        S_i = gl_i + (n_i > 0 ? ((c_visit + float(nmax)) * c_scale) * ((q_i + 1.0f) * 0.5f) : 0.0f)
 *        S_i = -inf where n_i != v or gl_i is -inf
 *    The chosen child is the first index of the maximum; if nothing equals the maximum, child 0 (as the PUCT arg-max).  c_visit and
 *    c_scale are the f32 values of the policy record's constants, so selection and the recorded target use one transform.
 * 4. The move.  v* = max n_i over the children with gl_i > -inf; the move is the action of the first arg-max of S_i with v = v*.  No
 *    uniform is consumed and `temperature` is not read.
 * Where it lives.  gl_i travels in the `cp` word of the ROOT's children (nothing but root selection reads it); m_g is a per-slot word.
 * A move's launches: step(0, 1), evaluate; step(1, 0) -- the root's expansion and backup, in memory; the root launch
 * (csrc/mcts_gumbel.hip engine_gumbel_root_kernel: one wavefront per slot, writes gl_i and m_g; a count above AQG_MAX_LEGAL or a
 * child range that leaves the pool writes nothing and sets m_g = 0); then per simulation the plain three-launch form with the step
 * kernel's GUMBEL instantiation (csrc/mcts_step.hip: level 0 scores by rule 3, every other level is PUCT) -- two launches more per
 * move than the three-launch PUCT form; step_heads, legal_beside_trunk and policy_beside_step do not apply.  The finish launch
 * (engine_finish_move_gumbel_kernel) is engine_finish_move_kernel's history row with rule 4 in place of the draw.
 * A root that is the pending leaf of a GUMBEL step cannot occur in that order; the kernel then drops the simulation and leaves
 * m_g = -1 for the read-out to show.
 * Refused before any launch, in this order: sims < 2; considered outside 1..64; a non-finite or negative scale; root noise; tree
 * reuse; resignation; temperature_plies > 0; prior_mode 2.  The evaluation cache, the policy record and the start table stay allowed.
 * The struct's contents are part of the hipGraph cache key. */
typedef struct aqg_gumbel {
    const double* table;            /* f64 [G, AQG_MAX_LEGAL] variates of this move's roots, or NULL = the generator */
    uint64_t seed;                  /* the generator's seed */
    double scale;                   /* finite, >= 0; 0 = a deterministic search */
    int32_t considered;             /* M, 1..64 */
    float c_visit, c_scale;         /* the f32 constants of sigma */
    const int32_t* schedule;        /* T, i32 [considered + 1, sims - 1] */
    int32_t* m;                     /* m_g, i32 [G] */
} aqg_gumbel;
/* aqg_engine_move_start / aqg_engine_finish_move_start with the option (uniforms may be NULL: none is read) */
int aqg_engine_move_gumbel(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                           const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy,
                           const aqg_start_table* start, const aqg_gumbel* gumbel, void* stream);
int aqg_engine_finish_move_gumbel(const aqg_engine* e_host, const double* uniforms, int32_t temperature_plies, float* hist_value,
                                  const aqg_tree_reuse* reuse, const aqg_resign* resign, const aqg_policy_record* policy,
                                  const aqg_start_table* start, const aqg_gumbel* gumbel, void* stream);
/* aqg_engine_search with the option (keys by slot) */
int aqg_engine_search_gumbel(const aqg_engine* e_host, const uint8_t* root_states72, const aqg_gumbel* gumbel, void* stream);
/* the root launch alone: gl_i into the expanded roots' children, m_g into the words */
int aqg_engine_gumbel_root(const aqg_engine* e_host, const aqg_gumbel* gumbel, void* stream);
/* the read-out: gl f32 [G, AQG_MAX_LEGAL] (-inf past the count), m i32 [G], the winner's child index by rule 4 i32 [G] (-1 without
 * children).  It changes nothing. */
int aqg_engine_root_gumbel(const aqg_engine* e_host, const aqg_gumbel* gumbel, float* gl, int32_t* m, int32_t* winner, void* stream);

/* ------------------------------------------------------------------ CPU baseline agents (agents.py) -- HOST pointers, host code */

/* The reference's baseline opponents (agents.py:14-214) are CPU code; so are these: the host instantiation of the rule header
 * the kernels compile, exported from the same library.  `rec72_host` = one state72 record in HOST memory.
 *   aqg_host_legal_actions   State.legal_actions() game_logic.py:103-117 -> ordered ids in out136_host[AQG_MAX_LEGAL], returns the count
 *   aqg_host_next            State.next(action) game_logic.py:366-391
 *   aqg_host_shortest_path   shortest_path_bfs agents.py:27-41: plies to the goal row over legal_actions_pos (jumps, frozen enemy), -1 = none
 *   aqg_host_heuristic_eval  heuristic_eval agents.py:22-54: (enemy's path - mover's path) / max_dist_from_goal
 *   aqg_host_alpha_beta_action  alpha_beta_action agents.py:60-108: depth-limited negamax with that heuristic, first best action; -1 = none */
int aqg_host_legal_actions(int board_size, const uint8_t* rec72_host, uint8_t* out136_host);
int aqg_host_next(int board_size, const uint8_t* rec72_host, int action, uint8_t* out72_host);
int aqg_host_shortest_path(int board_size, const uint8_t* rec72_host);
double aqg_host_heuristic_eval(int board_size, const uint8_t* rec72_host, int max_dist_from_goal);
int aqg_host_alpha_beta_action(int board_size, const uint8_t* rec72_host, int plies_for_draw, int max_dist_from_goal, int max_depth);

#ifdef __cplusplus
}
#endif
#endif /* AQGNN_H */
