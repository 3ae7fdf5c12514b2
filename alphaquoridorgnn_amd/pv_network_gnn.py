"""Policy-Value GNN -- drop-in for the reference's pv_network_gnn.py, executed by hand-written gfx950 kernels.

Call surface kept (pv_network_gnn.py:17-80): NUM_FEATURES, HIDDEN_DIM, NUM_GCN_LAYERS, POLICY_OUTPUT_SIZE,
`GraphPolicyValueNetwork(num_features, hidden_dim, num_gcn_layers, policy_output_size)` with submodules
`gcn_layers`, `policy_head`, `value_head`, `forward(x, edge_index, batch) -> (policy, value)`, `create_network()`.
state_dict keys follow PyG's GCNConv (`gcn_layers.i.lin.weight [out,in]`, `gcn_layers.i.bias [out]`).

Added (absent from the reference): `forward_states(states72)` -- the fused board-graph path the
self-play engine uses -- and `GNNNetwork`, the BaseNetwork-style wrapper (BaseNetwork.py:9-54) giving
`predict / prep_for_inference / preprocess_input / name`.

Any shape: the reference's GraphPolicyValueNetwork takes any (num_features, hidden_dim, num_gcn_layers, policy_output_size).
`forward(x, edge_index, batch)` of every shape (within SHAPE_LIMITS) runs the width-generic graph primitives of
csrc/gcn_general.hip, which also serve `GCNConv.forward(x, edge_index)` and `global_mean_pool(x, batch)` -- PyG's calls, on any
layer -- forward and backward.  On board records the default 6/128/3 network (`fused`) runs the fused kernels.

All arithmetic runs in libaqgnn_hip.so (fp32 data; fp16-split or f32-input MFMA, see csrc/gcn_trunk_split.hip and
csrc/gcn_trunk_exact.hip); there is no torch/CPU forward in this file.
"""
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .constants import BOARD_SIZE, PV_NETWORK_PATH, num_actions
from . import game_logic

NUM_FEATURES = 6      # pv_network_gnn.py:17
HIDDEN_DIM = 128      # :18
NUM_GCN_LAYERS = 3    # :19
POLICY_OUTPUT_SIZE = num_actions(BOARD_SIZE)  # :20

# inclusive bounds of the shapes the width-generic kernels take (GraphPolicyValueNetwork raises ValueError outside them)
SHAPE_LIMITS = {"num_features": (1, 1024), "hidden_dim": (2, 1024), "num_gcn_layers": (1, 32), "policy_output_size": (1, 4096)}

STATE_DICT_KEYS = [
    "gcn_layers.0.lin.weight", "gcn_layers.0.bias", "gcn_layers.1.lin.weight", "gcn_layers.1.bias",
    "gcn_layers.2.lin.weight", "gcn_layers.2.bias", "policy_head.0.weight", "policy_head.0.bias",
    "policy_head.2.weight", "policy_head.2.bias", "value_head.0.weight", "value_head.0.bias",
    "value_head.2.weight", "value_head.2.bias",
]


def state_dict_keys(num_gcn_layers):
    """The parameter names of a network with `num_gcn_layers` GCN layers, in the order of the HIP entry points
    (STATE_DICT_KEYS for the default 3)."""
    keys = []
    for i in range(num_gcn_layers):
        keys += [f"gcn_layers.{i}.lin.weight", f"gcn_layers.{i}.bias"]
    return keys + STATE_DICT_KEYS[6:]


class GCNConv(nn.Module):
    """PyG's GCNConv with its naming and initialisation (lin: Glorot-uniform, no bias; bias: zeros).  On board records a
    default 6/128/3 network fuses the layer arithmetic into its network-level kernels; forward(x, edge_index) runs the layer
    alone on the width-generic kernels (any in / out width)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        a = math.sqrt(6.0 / (in_channels + out_channels))
        with torch.no_grad():
            self.lin.weight.uniform_(-a, a)

    def forward(self, x, edge_index):
        """PyG's GCNConv.forward with its defaults: A_hat (x W^T) + b, no ReLU.  x [n, in_channels] floating point,
        edge_index [2, E] integer ids in [0, n); gcn_norm and validation as GraphPolicyValueNetwork._prepare_graph (one
        device-to-host read).  Returns f32 [n, out_channels]; differentiable with respect to x, lin.weight and bias."""
        dev = _lib.require_gpu(x.device)
        W, b = self.lin.weight, self.bias
        if x.dim() == 2 and x.shape[1] == self.in_channels:
            batch = torch.zeros((x.shape[0],), dtype=torch.int64, device=dev)
        else:
            batch = torch.zeros((0,), dtype=torch.int64, device=dev)      # (_prepare_graph names the shape error of x)
        record = torch.is_grad_enabled() and (x.requires_grad or W.requires_grad or b.requires_grad)
        tensors = GraphPolicyValueNetwork._prepare_graph(x, edge_index, batch, transpose=record, num_features=self.in_channels)
        xf = x.to(torch.float32).contiguous()
        if record:
            return _GCNConvFunction.apply(tensors, dev, xf, W, b)
        return _gcn_conv(_lib.load(), dev, xf, tensors[:3], _param(W, dev), _param(b, dev))


class GraphPolicyValueNetwork(nn.Module):
    def __init__(self, num_features=NUM_FEATURES, hidden_dim=HIDDEN_DIM, num_gcn_layers=NUM_GCN_LAYERS,
                 policy_output_size=POLICY_OUTPUT_SIZE, board_size=BOARD_SIZE):
        super().__init__()
        for name, v in (("num_features", num_features), ("hidden_dim", hidden_dim), ("num_gcn_layers", num_gcn_layers),
                        ("policy_output_size", policy_output_size)):
            lo, hi = SHAPE_LIMITS[name]
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an integer in [{lo}, {hi}] (the limit of the HIP kernels), got {v!r}")
        num_features, hidden_dim, num_gcn_layers, policy_output_size = (int(num_features), int(hidden_dim), int(num_gcn_layers),
                                                                        int(policy_output_size))
        # the default shape has the fused board kernels (packed weights, forward_states, engine 'gnn' evaluator, GNNTrainer)
        self.fused = (num_features, hidden_dim, num_gcn_layers) == (NUM_FEATURES, HIDDEN_DIM, NUM_GCN_LAYERS)
        self.state_dict_keys = state_dict_keys(num_gcn_layers)
        self.num_features = num_features
        self.hidden_dim = hidden_dim
        self.num_gcn_layers = num_gcn_layers
        self.policy_output_size = policy_output_size
        self.board_size = board_size

        self.gcn_layers = nn.ModuleList()
        self.gcn_layers.append(GCNConv(num_features, hidden_dim))
        for _ in range(num_gcn_layers - 1):
            self.gcn_layers.append(GCNConv(hidden_dim, hidden_dim))
        self.policy_head = nn.Sequential(nn.Linear(hidden_dim, hidden_dim // 2), nn.ReLU(),
                                         nn.Linear(hidden_dim // 2, policy_output_size), nn.Softmax(dim=1))
        self.value_head = nn.Sequential(nn.Linear(hidden_dim, hidden_dim // 2), nn.ReLU(),
                                        nn.Linear(hidden_dim // 2, 1), nn.Tanh())
        self._packed = None
        self._packed_key = None
        self._gnn_flags = 0
        self._sat_words = {}          # device -> int32 [1]: the runtime fp16-range guard's word (aqg_gcn_forward_boards_guarded)

    # ---------------------------------------------------------------- weight packing
    def packed_weights(self, device):
        """float32 device buffer in the kernel layout (include/aqgnn.h); rebuilt when a parameter changes.  Every rebuild
        also re-runs the fp16-range check of this weight set (`gnn_flags`).  Default 6/128/3 shape only."""
        self._require_fused("packed_weights (the fused kernels' weight layout)")
        sd = self.state_dict()
        key = (str(device),) + tuple((sd[k].data_ptr(), sd[k]._version) for k in STATE_DICT_KEYS)
        if self._packed is None or key != self._packed_key:
            lib = _lib.load()
            host = [sd[k].detach().to("cpu", torch.float32).contiguous() for k in STATE_DICT_KEYS]
            arr = (ctypes.c_void_p * 14)(*[ctypes.c_void_p(t.data_ptr()) for t in host])
            out = torch.empty(lib.aqg_gcn_packed_floats(self.board_size), dtype=torch.float32)
            _lib.check(lib.aqg_gcn_pack_weights_host(self.board_size, arr, ctypes.c_void_p(out.data_ptr())),
                       "aqg_gcn_pack_weights_host")
            self._packed = out.to(device)
            self._packed_key = key
            for w in self._sat_words.values():
                w.zero_()
            self._gnn_flags = self._calibrate(self._packed, device)
            if self._gnn_flags == 0 and self._range_proven(host):
                self._gnn_flags = _lib.GNN_RANGE_PROVEN
        return self._packed

    def _range_proven(self, host):
        """A static bound over ALL inputs (any board graph, any record with at most GNN_PROVEN_MAX_WALLS walls in hand per player) on
        every value the split trunk holds as an fp16 pair (include/aqgnn.h, AQG_GNN_RANGE_PROVEN).  GCNConv is
        P = A_hat (H W^T) + b with A_hat >= 0 and H >= 0 after the ReLU.  A row of A_hat sums to
        1/d_n + sum_{k ~ n} 1/sqrt(d_n d_k) <= 1/d_n + (d_n - 1)/sqrt(2 d_n) <= R = 0.2 + 4/sqrt(10) = 1.465  (closed degrees d <= 5 on
        the grid, and a neighbour of n has d_k >= 2: itself and n), so  |Z_l| <= |W_l| h_{l-1} =: z_l  and  |P_l|, H_l <= R z_l + |b_l|
        =: h_l,  with h_0 = the feature maxima.  The kernel's own images are these times its internal scales: planes
        CQ sqrt(d) H <= 2.10 h, linear-map outputs sqrt(d) Z <= 2.24 z, weights W / CQ <= 1.07 |W|: proven iff
        2.3 max(z_l, h_l, |W_l|) < 65504.  True for the weights, not for a sample of boards: when it holds, the kernels' per-value
        range tracking is redundant and is switched off (the records' wall counts are still checked, on the scalar unit)."""
        if self.board_size != 9:
            return False
        if not all(bool(torch.isfinite(t).all()) for t in host[:6]):
            return False                                  # (Python's max() below would skip a NaN)
        W1, b1, W2, b2, W3, b3 = (t.double().abs() for t in host[:6])
        R = 0.2 + 4.0 / 10.0 ** 0.5
        wmax = float(_lib.GNN_PROVEN_MAX_WALLS)
        h = torch.tensor([1.0, wmax, 1.0, wmax, 1.0, 1.0], dtype=torch.float64)     # pv_network_cnn.py:88-114: one-hot, count, one-hot, count, bit, bit
        worst = 0.0
        for W, b in ((W1, b1), (W2, b2), (W3, b3)):
            z = W @ h
            h = R * z + b
            worst = max(worst, float(z.max()), float(h.max()), float(W.max()))
        return bool(np.isfinite(worst)) and 2.3 * worst < 65504.0

    def _require_fused(self, what):
        if not self.fused:
            raise ValueError(
                f"{what} exists for the default {NUM_FEATURES}/{HIDDEN_DIM}/{NUM_GCN_LAYERS} network only; this one is "
                f"{self.num_features}/{self.hidden_dim}/{self.num_gcn_layers}: train it with train_network.GeneralTrainer (6 input features) "
                "or autograd (forward(x, edge_index, batch), loss.backward() and a torch optimiser) instead of GNNTrainer, and search "
                "with evaluator='general' (the engine's any-shape "
                "evaluator) or evaluator='external' (its predict) instead of the engine's 'gnn' evaluator")

    def invalidate_packed(self):
        """Call after the parameters were changed behind torch's back (train_network.GNNTrainer updates them in place from
        a HIP kernel, which does not bump the tensors' version counters)."""
        self._packed = None
        self._packed_key = None

    def gnn_flags(self, device):
        """Flags every GNN forward of this weight set must carry: 0; _lib.GNN_RANGE_PROVEN when a static bound shows that
        nothing can leave fp16 range (_range_proven: the split kernels then skip their per-value range tracking); or
        _lib.GNN_EXACT_F32 when the fp16-split kernels cannot represent its activations -- found on the calibration boards when
        the set is packed (_calibrate), or at run time by the kernels' range guard (mark_saturated)."""
        self.packed_weights(device)
        return self._gnn_flags

    def saturation_word(self, device):
        """The int32 device word the split kernels OR 1 into when they meet a value outside fp16 range (include/aqgnn.h,
        aqg_gcn_forward_boards_guarded); one per device, zero until that happens."""
        key = str(device)
        if key not in self._sat_words:
            self._sat_words[key] = torch.zeros((1,), dtype=torch.int32, device=device)
        return self._sat_words[key]

    def mark_saturated(self, device=None):
        """The range guard fired for this weight set (a forward of this module, or an engine evaluating with it): from now on --
        until the parameters change -- it is served by the exact f32-input kernels, like a set that fails calibration."""
        self._gnn_flags = _lib.GNN_EXACT_F32
        for w in self._sat_words.values():
            w.zero_()

    _calib_boards = {}

    @classmethod
    def _calibration_boards(cls, device):
        """64 synthetic 9x9 boards spanning the feature range (pawns anywhere, 0..10 walls in hand, 0..20 walls on the
        board, not necessarily legal positions: only the network sees them), plus the start position."""
        key = str(device)
        if key not in cls._calib_boards:
            rng = np.random.RandomState(20250117)
            recs = np.zeros((64, 72), dtype=np.uint8)
            for i in range(64):
                recs[i, 0], recs[i, 2] = rng.randint(0, 81, 2)
                recs[i, 1], recs[i, 3] = (10, 10) if i < 8 else rng.randint(0, 11, 2)
                nw = 0 if i == 0 else rng.randint(0, 21)
                recs[i, 4 + rng.choice(64, nw, replace=False)] = rng.randint(1, 3, nw)
                recs[i, 70] = 9
            recs[0, 0] = recs[0, 2] = 76
            cls._calib_boards[key] = torch.from_numpy(recs).to(device)
        return cls._calib_boards[key]

    def _calibrate(self, packed, device):
        """The default trunk / heads hold every activation as TWO fp16 numbers (hi + lo: fp32-equivalent products on the
        16-bit matrix pipe).  That is exact-enough only while activations stay inside fp16 range; beyond it the kernels
        saturate at 65504 instead of overflowing -- finite, but no longer the network -- and, on the low side, only while the
        lo halves are normal fp16 numbers: an operand below 2^-3 is carried to 2^-25 absolute, whatever its own scale.  The
        reference's fp32 has neither limit, so each weight set is checked once: both kernel families run on the calibration
        boards, and if their logits or values disagree beyond the bar stated for the split kernels (atol 1e-5, rtol 1e-4) the
        weight set is served by the exact f32-input MFMA kernels from then on.  The bar is taken per board and relative to the
        board's own output scale, s = the largest |logit| or |value_pre| of the exact kernels between 1 and 10: both families
        accumulate in f32, so on a board whose activations are thousands they differ from EACH OTHER by rounding that grows with
        them (the scaled-weight tests take their bars times max(1, max |logits|) for the same reason); s = 1, the stated bar, for
        outputs of ordinary size, and at s = 10 the bar this check used to apply to every set.  What asks for the scale: the
        weight sets of tests/test_gpu_parity.py::test_gnn_runtime_saturation_signal (set A, gcn_layers.0 column 1 = 200: pooled
        features to 3,600 and logits to 620 on the calibration boards) and of test_step_heads_fused.py's pooled-overflow case must
        pass this check and be caught at run time instead; at the flat 1e-5 / 1e-4 they fail it on f32 rounding alone.  What it
        costs: a board whose largest |logit| is 10 or more -- a confident trained policy -- is still held to the former bar only.
        (A weight matrix that is itself below the split's scale never gets here as a pass: the packing gives it negative guard
        thresholds, and the word fires; one that passes the packing on a single larger entry is caught here,
        tests/test_split_low_side.py::test_calibration_catches_what_the_packing_admits.)"""
        if self.board_size != 9:
            return 0                                      # smaller boards run the plain f32 kernels anyway
        lib = _lib.load()
        boards = self._calibration_boards(device)
        B, A = boards.shape[0], self.policy_output_size
        res = []
        word = torch.zeros((1,), dtype=torch.int32, device=device)
        for flags in (0, _lib.GNN_EXACT_F32):
            pooled = torch.empty((B, HIDDEN_DIM), dtype=torch.float32, device=device)
            logits = torch.empty((B, A), dtype=torch.float32, device=device)
            vpre = torch.empty((B,), dtype=torch.float32, device=device)
            _lib.check(lib.aqg_gcn_forward_boards_guarded(9, _lib.ptr(boards), 0, B, _lib.ptr(packed), _lib.ptr(pooled), _lib.ptr(logits),
                                                          None, _lib.ptr(vpre), None, flags, _lib.ptr(word), _lib.stream_ptr(device)),
                       "calibration forward")
            res.append(torch.cat([logits, vpre.unsqueeze(1)], 1).double())
        split, exact = res
        scale = exact.abs().amax(dim=1, keepdim=True).clamp(1.0, 10.0)
        ok = bool(((split - exact).abs() <= scale * (1e-5 + 1e-4 * exact.abs())).all())    # NaN compares False
        ok = ok and int(word.item()) == 0                                         # the kernels' own range guard, on the same boards
        return 0 if ok else _lib.GNN_EXACT_F32

    # ---------------------------------------------------------------- fused board path
    def forward_states(self, states72, want_logits=False, state_fmt=0, check_saturation=True):
        """states72: uint8 [B,72] device tensor (state_fmt=0) -> (policy [B,A] softmaxed, value [B,1] tanh'ed);
        with want_logits also returns (logits [B,A], value_pre [B]).
        check_saturation: after a forward on the fp16-split kernels the range guard's word is read back (one 4-byte copy, a
        host sync); if a value left fp16 range the weight set is marked (mark_saturated) and the call is repeated on the
        exact f32-input kernels, so the caller always receives the network's outputs -- the reference's fp32 has no cliff
        (pv_network_gnn.py:53-64).  False skips the read-back (the engine has its own counter, counters()['gnn_saturated'])."""
        if not self.fused:
            return self._forward_states_general(states72, want_logits, state_fmt)
        dev = _lib.require_gpu(states72.device)
        lib = _lib.load()
        B = states72.shape[0]
        A = self.policy_output_size
        f32 = dict(dtype=torch.float32, device=dev)
        pooled = torch.empty((B, HIDDEN_DIM), **f32)
        policy = torch.empty((B, A), **f32)
        value = torch.empty((B,), **f32)
        logits = torch.empty((B, A), **f32) if want_logits else None
        vpre = torch.empty((B,), **f32) if want_logits else None
        if self.board_size == 9:
            word = self.saturation_word(dev)
            for attempt in range(2):
                flags = self.gnn_flags(dev)
                _lib.check(lib.aqg_gcn_forward_boards_guarded(self.board_size, _lib.ptr(states72), state_fmt, B,
                                                              _lib.ptr(self.packed_weights(dev)), _lib.ptr(pooled), _lib.ptr(logits),
                                                              _lib.ptr(policy), _lib.ptr(vpre), _lib.ptr(value), flags,
                                                              _lib.ptr(word), _lib.stream_ptr(dev)),
                           "aqg_gcn_forward_boards_guarded")
                if (flags & _lib.GNN_EXACT_F32) or not check_saturation or B == 0 or int(word.item()) == 0:
                    break
                self.mark_saturated(dev)          # outside fp16 range: repeat on the exact kernels, and stay there
        else:   # the reference's smaller boards (constants.py:5-20): plain kernels over a caller-owned workspace
            nws = lib.aqg_gcn_boards_any_workspace_floats(self.board_size, B)
            ws = torch.empty((max(int(nws), 1),), **f32)
            _lib.check(lib.aqg_gcn_forward_boards_any(self.board_size, _lib.ptr(states72), state_fmt, B,
                                                      _lib.ptr(self.packed_weights(dev)), _lib.ptr(ws), nws, _lib.ptr(pooled),
                                                      _lib.ptr(logits), _lib.ptr(policy), _lib.ptr(vpre), _lib.ptr(value), 0,
                                                      _lib.stream_ptr(dev)), "aqg_gcn_forward_boards_any")
        if want_logits:
            return policy, value.unsqueeze(1), logits, vpre
        return policy, value.unsqueeze(1)

    def _forward_states_general(self, states72, want_logits, state_fmt):
        """forward_states of a non-default shape: the board featuriser (aqg_gcn_boards_graph) and the width-generic layers."""
        if self.num_features != 6:
            raise ValueError(f"board records have 6 feature planes; this network takes num_features={self.num_features}: "
                             "use forward(x, edge_index, batch)")
        if state_fmt != 0:
            raise ValueError("a network of non-default shape takes state72 records (state_fmt=0) only")
        dev = _lib.require_gpu(states72.device)
        lib = _lib.load()
        N = self.board_size
        V, B = N * N, states72.shape[0]
        R = B * V
        x = torch.empty((R, 6), dtype=torch.float32, device=dev)
        idx = torch.empty((R * 5,), dtype=torch.int32, device=dev)
        w = torch.empty((R * 5,), dtype=torch.float32, device=dev)
        if B:
            _lib.check(lib.aqg_gcn_boards_graph(N, _lib.ptr(states72.contiguous()), B, _lib.ptr(x), _lib.ptr(idx), _lib.ptr(w),
                                                _lib.stream_ptr(dev)), "aqg_gcn_boards_graph")
        csr = (torch.arange(0, 5 * R + 1, 5, dtype=torch.int32, device=dev), idx, w)     # ELL rows of 5 (closed sides: id -1)
        gptr = torch.arange(0, R + 1, V, dtype=torch.int32, device=dev)
        pf = [_param(p, dev) for _, p in self._ordered_params()]
        policy, value, logits, vpre = _general_forward(lib, dev, self, x, csr, gptr, B, pf)[:4]
        if want_logits:
            return policy, value.unsqueeze(1), logits, vpre
        return policy, value.unsqueeze(1)

    # ---------------------------------------------------------------- generic (x, edge_index, batch) path
    @staticmethod
    def _prepare_graph(x, edge_index, batch, transpose=False, num_features=NUM_FEATURES):
        """Everything forward(x, edge_index, batch) does before its launch, on x's device (CPU or GPU alike):
        validation, PyG's gcn_norm as a CSR by destination, and the graph pointer of the mean pool.

        Raises ValueError unless x is [n, num_features] floating point, edge_index an integer [2, E] tensor with every id in [0, n),
        and batch an integer [n] tensor, non-negative and sorted (PyG's Batch convention; unsorted batches are not
        supported).  The id and batch checks share ONE device-to-host read, made before any tensor is indexed with the ids.

        gcn_norm with GCNConv's defaults: every edge has weight 1; add_remaining_self_loops drops every existing i -> i edge
        and appends exactly one self loop per node; repeated non-loop edges each count.  deg[i] = number of edges INTO i
        (flow source_to_target, the self loop included, so deg >= 1), w_e = deg[src]^-1/2 * deg[dst]^-1/2.
        Returns (ptr int32 [n+1], src int32 [E_nonloop+n], w float32 [E_nonloop+n], gptr int32 [G+1], G): the edges into
        node i are ptr[i] .. ptr[i+1] (its incoming edges in input order, then its self loop), graph g holds the nodes
        gptr[g] .. gptr[g+1] and G = batch.max() + 1 (a graph id without nodes pools to 0, as in PyG).
        transpose=True (the recording forward of autograd) appends the same entries as a CSR by SOURCE, (tptr int32 [n+1],
        tdst int32, tw float32): the entries leaving node j are tptr[j] .. tptr[j+1], in their order above (a stable sort),
        built on the device without another host read."""
        def integral(t):
            return not (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool)
        if x.dim() != 2 or x.shape[1] != num_features or not x.is_floating_point():
            raise ValueError(f"x must be a floating-point [num_nodes, {num_features}] tensor, got {x.dtype} {tuple(x.shape)}")
        n = x.shape[0]
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or not integral(edge_index):
            raise ValueError(f"edge_index must be an integer [2, E] tensor, got {edge_index.dtype} {tuple(edge_index.shape)}")
        if batch.dim() != 1 or batch.shape[0] != n or not integral(batch):
            raise ValueError(f"batch must be an integer [num_nodes] = [{n}] tensor, got {batch.dtype} {tuple(batch.shape)}")
        dev = x.device
        ei = edge_index.to(dev).long()
        src, dst = ei[0], ei[1]
        batch = batch.to(dev).long()
        E = src.shape[0]
        loop = src == dst
        # one device-to-host read for every data-dependent check and size
        stats = [(~loop).sum()]
        if E:
            stats += [ei.amin(), ei.amax()]
        if n:
            stats += [batch[0], batch[-1], (batch[1:] < batch[:-1]).sum()]
        stats = torch.stack(stats).tolist()
        E_nonloop = stats[0]
        if E and (stats[1] < 0 or stats[2] >= n):
            raise ValueError(f"edge_index holds node ids outside [0, {n}) (min {stats[1]}, max {stats[2]})")
        if n and stats[-1]:
            raise ValueError("batch must be sorted (PyG Batch convention; unsorted batches are not supported)")
        if n and stats[-3] < 0:
            raise ValueError(f"batch ids must be non-negative (min {stats[-3]})")
        G = stats[-2] + 1 if n else 0
        # add_remaining_self_loops + CSR in one stable sort: existing loops get the key n (sorted past every node and cut
        # off), one loop per node is appended after the input edges
        nodes = torch.arange(n, device=dev)
        src = torch.cat([src, nodes])
        dst = torch.cat([torch.where(loop, n, dst), nodes])
        order = torch.argsort(dst, stable=True)[:E_nonloop + n]
        src, dst = src[order], dst[order]
        ptr = torch.searchsorted(dst, torch.arange(n + 1, device=dev)).to(torch.int32)
        dis = (ptr[1:] - ptr[:-1]).to(torch.float32).pow(-0.5)
        w = dis[src] * dis[dst]
        gptr = torch.searchsorted(batch, torch.arange(G + 1, device=dev)).to(torch.int32)
        if not transpose:
            return ptr, src.to(torch.int32).contiguous(), w.contiguous(), gptr, G
        torder = torch.argsort(src, stable=True)
        tptr = torch.searchsorted(src[torder], torch.arange(n + 1, device=dev)).to(torch.int32)
        return (ptr, src.to(torch.int32).contiguous(), w.contiguous(), gptr, G,
                tptr, dst[torder].to(torch.int32).contiguous(), w[torder].contiguous())

    def forward(self, x, edge_index, batch):
        """pv_network_gnn.py:53-64 with PyG's GCNConv / global_mean_pool semantics (_prepare_graph: the self-loop rule and the
        validated inputs).  x [sum V, num_features] floating point, edge_index [2, E] integer ids in [0, sum V), batch [sum V]
        integer, non-negative and sorted (unsorted raises ValueError).  One device-to-host read per call.  Every shape, the
        default 6/128/3 included, runs the width-generic kernels (csrc/gcn_general.hip) on the module's own parameters.

        Autograd: in train mode, with grad enabled and x or any parameter requiring grad, the forward is recorded
        (_GeneralForward): the outputs carry a grad_fn and backward() fills the parameters' .grad (and x.grad) from the same
        HIP primitives.  Its values are bit-identical to the plain forward's.  Otherwise (eval mode, no_grad,
        inference_mode) the outputs carry no graph."""
        dev = _lib.require_gpu(x.device)
        params = [p for _, p in self._ordered_params()]
        record = self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        tensors = self._prepare_graph(x, edge_index, batch, transpose=record, num_features=self.num_features)
        xf = x.to(torch.float32).contiguous()            # outside the Function: torch routes x's gradient through the cast
        if record:
            policy, value, logits, vpre = _GeneralForward.apply(self, tensors, dev, xf, *params)
        else:
            pf = [_param(p, dev) for p in params]
            policy, value, logits, vpre = _general_forward(_lib.load(), dev, self, xf, tensors[:3], tensors[3], tensors[4], pf)[:4]
        self.last_logits, self.last_value_pre = logits, vpre
        return policy, value.unsqueeze(1)

    def predict_batch(self, states72):
        """Batched predict: device uint8 [B,72] -> (policy [B,A] over ALL actions, value [B])."""
        policy, value = self.forward_states(states72)
        return policy, value[:, 0]

    def predict(self, state, device=None):
        """pv_network_cnn.py:117-137: PMF over state.legal_actions() (in that order) as float32 numpy + python float."""
        dev = _lib.require_gpu()
        rec = torch.from_numpy(state.record() if hasattr(state, "record") else
                               game_logic.pack_state72(state.player, state.enemy, state.walls, state.plies_played, state.N)
                               ).to(dev).unsqueeze(0)
        with torch.inference_mode():
            policy, value = self.forward_states(rec)
            _, order, count = game_logic.legal_actions_batch(rec, self.board_size, want_mask=False)
            n = int(count.item())
            pol = policy[0][order[0, :n].long()]
            s = torch.sum(pol)
            pol = pol / (s if s else 1)
        return pol.cpu().numpy(), value.item()

    def _ordered_params(self):
        sd = dict(self.named_parameters())
        return [(k, sd[k]) for k in self.state_dict_keys]

    # ---------------------------------------------------------------- any-shape descriptor (engine prior_mode 3)
    def general_net(self, device):
        """The ctypes descriptor of this network for aqg_gcn_forward_boards_general and the engine's evaluator='general'
        (include/aqgnn.h aqg_gcn_general_net): its shape and device pointers to the module's OWN parameters, so an in-place
        optimiser update is seen by the next launch without a repack.  Every parameter must be a contiguous float32 tensor on
        `device`; works for any shape with 6 input features, the default 6/128/3 included."""
        if self.num_features != 6:
            raise ValueError(f"board records have 6 feature planes; this network takes num_features={self.num_features}: "
                             "use forward(x, edge_index, batch)")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        net = _lib.GeneralNetStruct()
        net.num_features, net.hidden, net.num_layers, net.policy_size = (self.num_features, self.hidden_dim, self.num_gcn_layers,
                                                                         self.policy_output_size)
        for i, (k, p) in enumerate(self._ordered_params()):
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous():
                raise ValueError(f"{k} must be a contiguous float32 tensor on {dev} for the engine's 'general' evaluator "
                                 f"(it is {p.dtype} on {p.device}): move the network with .to({str(dev)!r}) first")
            net.params[i] = p.data_ptr()
        return net

    def general_weights_key(self):
        """(data pointer, version counter) of every parameter: changes whenever a parameter is replaced or updated in place."""
        return tuple((p.data_ptr(), p._version) for _, p in self._ordered_params())


# ---------------------------------------------------------------- width-generic graph primitives (csrc/gcn_general.hip)
def _param(p, dev):
    """A parameter as the kernels read it: f32, contiguous, on dev (the parameter itself when it already is)."""
    return p.detach().to(device=dev, dtype=torch.float32).contiguous()


def _empty(shape, dev):
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _linear(lib, dev, X, W, bias=None, relu=False, mask=None, w_kn=False, out=None, accumulate=False):
    """aqg_graph_linear: X [M,K] W^T (+ bias) (ReLU) (masked); W [N,K], or [K,N] with w_kn (X W)."""
    M, K = X.shape
    N = W.shape[1] if w_kn else W.shape[0]
    Y = _empty((M, N), dev) if out is None else out
    flags = (_lib.LIN_RELU if relu else 0) | (_lib.LIN_W_KN if w_kn else 0) | (_lib.LIN_ACCUMULATE if accumulate else 0)
    _lib.check(lib.aqg_graph_linear(M, K, N, _lib.ptr(X), _lib.ptr(W), _lib.ptr(bias), _lib.ptr(mask), flags, _lib.ptr(Y),
                                    _lib.stream_ptr(dev)), "aqg_graph_linear")
    return Y


def _linear_grad(lib, dev, dY, X, dYb=None):
    """aqg_graph_linear_grad: (dW [N,K] = dY^T X, db [N] = column sums of dYb, default dY)."""
    M, N = dY.shape
    K = X.shape[1]
    nws = int(lib.aqg_graph_linear_grad_workspace_floats(M, N, K))
    ws = _empty((nws,), dev) if nws else None
    dW, db = _empty((N, K), dev), _empty((N,), dev)
    _lib.check(lib.aqg_graph_linear_grad(M, K, N, _lib.ptr(dY), _lib.ptr(X), _lib.ptr(dYb), _lib.ptr(ws), nws, _lib.ptr(dW),
                                         _lib.ptr(db), _lib.stream_ptr(dev)), "aqg_graph_linear_grad")
    return dW, db


def _aggregate(lib, dev, Y, csr, bias=None, relu=False):
    """aqg_graph_aggregate over csr = (ptr, src, w): the CSR by destination (propagate) or by source (its backward)."""
    n, N = Y.shape
    out = _empty((n, N), dev)
    ptr, src, w = csr
    _lib.check(lib.aqg_graph_aggregate(n, N, _lib.ptr(Y), _lib.ptr(ptr), _lib.ptr(src), _lib.ptr(w), _lib.ptr(bias), int(relu),
                                       _lib.ptr(out), _lib.stream_ptr(dev)), "aqg_graph_aggregate")
    return out


def _mean_pool(lib, dev, H, gptr, G):
    n, N = H.shape
    pooled = _empty((G, N), dev)
    _lib.check(lib.aqg_graph_mean_pool(n, N, _lib.ptr(H), _lib.ptr(gptr), G, _lib.ptr(pooled), _lib.stream_ptr(dev)),
               "aqg_graph_mean_pool")
    return pooled


def _mean_pool_backward(lib, dev, dpooled, gptr, G, n, mask=None):
    N = dpooled.shape[1]
    dH = _empty((n, N), dev)
    _lib.check(lib.aqg_graph_mean_pool_backward(n, N, _lib.ptr(dpooled), _lib.ptr(gptr), G, _lib.ptr(mask), _lib.ptr(dH),
                                                _lib.stream_ptr(dev)), "aqg_graph_mean_pool_backward")
    return dH


def _gcn_conv(lib, dev, xf, csr, W, b, relu=False):
    """One GCNConv: A_hat (x W^T) + b (ReLU)."""
    return _aggregate(lib, dev, _linear(lib, dev, xf, W), csr, bias=b, relu=relu)


def _general_forward(lib, dev, model, xf, csr, gptr, G, pf):
    """The network on the width-generic primitives: L x (linear, aggregate + bias + ReLU) -> mean pool -> the two heads ->
    softmax / tanh.  Returns (policy [G,A], value [G], logits [G,A], value_pre [G], acts) with acts = (H_0 = x, H_1 .. H_L,
    pooled, policy hidden, value hidden) -- what the backward reads."""
    L, A = model.num_gcn_layers, model.policy_output_size
    hs = [xf]
    for l in range(L):
        hs.append(_gcn_conv(lib, dev, hs[-1], csr, pf[2 * l], pf[2 * l + 1], relu=True))
    pooled = _mean_pool(lib, dev, hs[-1], gptr, G)
    o = 2 * L
    hp = _linear(lib, dev, pooled, pf[o], pf[o + 1], relu=True)
    logits = _linear(lib, dev, hp, pf[o + 2], pf[o + 3])
    hv = _linear(lib, dev, pooled, pf[o + 4], pf[o + 5], relu=True)
    vpre = _linear(lib, dev, hv, pf[o + 6], pf[o + 7]).view(G)
    policy, value = _empty((G, A), dev), _empty((G,), dev)
    _lib.check(lib.aqg_graph_heads(G, A, _lib.ptr(logits), _lib.ptr(vpre), _lib.ptr(policy), _lib.ptr(value), _lib.stream_ptr(dev)),
               "aqg_graph_heads")
    return policy, value, logits, vpre, (hs, pooled, hp, hv)


class _GeneralForward(torch.autograd.Function):
    """forward(x, edge_index, batch) as one autograd node: _general_forward with its activations kept,
    and the backward composed from the same primitives.  Neither direction reads anything back to the host."""

    @staticmethod
    def forward(ctx, model, tensors, dev, xf, *params):
        ptr, src, w, gptr, G, tptr, tdst, tw = tensors
        lib = _lib.load()
        pf = [_param(p, dev) for p in params]
        policy, value, logits, vpre, acts = _general_forward(lib, dev, model, xf, (ptr, src, w), gptr, G, pf)
        ctx.save_for_backward(policy, value, *pf)
        ctx.graph = ((tptr, tdst, tw), gptr, G, dev, model.num_gcn_layers)
        ctx.param_dtypes = [p.dtype for p in params]
        ctx.acts = acts
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(logits, vpre)
        return policy, value, logits, vpre

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dpolicy, dvalue, _dlogits, _dvpre):
        policy, value, *pf = ctx.saved_tensors
        tcsr, gptr, G, dev, L = ctx.graph
        hs, pooled, hp, hv = ctx.acts
        lib = _lib.load()
        n, A = hs[0].shape[0], policy.shape[1]
        grads = [None] * (2 * L + 8)
        dp = dpolicy.to(torch.float32).contiguous() if dpolicy is not None else None
        dv = dvalue.to(torch.float32).contiguous() if dvalue is not None else None
        dlogits, dvpre = _empty((G, A), dev), _empty((G, 1), dev)
        _lib.check(lib.aqg_graph_heads_backward(G, A, _lib.ptr(policy), _lib.ptr(dp), _lib.ptr(value), _lib.ptr(dv),
                                                _lib.ptr(dlogits), _lib.ptr(dvpre), _lib.stream_ptr(dev)), "aqg_graph_heads_backward")
        o = 2 * L
        grads[o + 2], grads[o + 3] = _linear_grad(lib, dev, dlogits, hp)               # policy_head.2
        grads[o + 6], grads[o + 7] = _linear_grad(lib, dev, dvpre, hv)                 # value_head.2
        dhp = _linear(lib, dev, dlogits, pf[o + 2], mask=hp, w_kn=True)
        dhv = _linear(lib, dev, dvpre, pf[o + 6], mask=hv, w_kn=True)
        grads[o], grads[o + 1] = _linear_grad(lib, dev, dhp, pooled)                   # policy_head.0
        grads[o + 4], grads[o + 5] = _linear_grad(lib, dev, dhv, pooled)               # value_head.0
        dpooled = _linear(lib, dev, dhp, pf[o], w_kn=True)
        _linear(lib, dev, dhv, pf[o + 4], w_kn=True, out=dpooled, accumulate=True)
        dP = _mean_pool_backward(lib, dev, dpooled, gptr, G, n, mask=hs[L])
        dx = None
        for l in range(L, 0, -1):                 # P_l = A_hat (H_{l-1} W_l^T) + b_l, H_l = relu(P_l)
            dZ = _aggregate(lib, dev, dP, tcsr)
            grads[2 * l - 2], grads[2 * l - 1] = _linear_grad(lib, dev, dZ, hs[l - 1], dYb=dP)
            if l > 1:
                dP = _linear(lib, dev, dZ, pf[2 * l - 2], mask=hs[l - 1], w_kn=True)
            elif ctx.needs_input_grad[3]:
                dx = _linear(lib, dev, dZ, pf[0], w_kn=True)
        out = [g.view(pf[i].shape) if ctx.needs_input_grad[4 + i] else None for i, g in enumerate(grads)]
        out = [o.to(ctx.param_dtypes[i]) if o is not None else None for i, o in enumerate(out)]
        return (None, None, None, dx, *out)


class _GCNConvFunction(torch.autograd.Function):
    """GCNConv.forward as one autograd node: out = A_hat Z + b with Z = x W^T;  dZ = A_hat^T dout, dW = dZ^T x,
    db = sum_i dout[i], dx = dZ W."""

    @staticmethod
    def forward(ctx, tensors, dev, xf, W, b):
        ptr, src, w, _gptr, _G, tptr, tdst, tw = tensors
        Wf, bf = _param(W, dev), _param(b, dev)
        out = _gcn_conv(_lib.load(), dev, xf, (ptr, src, w), Wf, bf)
        ctx.save_for_backward(xf, Wf)
        ctx.graph = ((tptr, tdst, tw), dev)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        xf, Wf = ctx.saved_tensors
        tcsr, dev = ctx.graph
        lib = _lib.load()
        dout = dout.to(torch.float32).contiguous()
        dZ = _aggregate(lib, dev, dout, tcsr)
        dW, db = _linear_grad(lib, dev, dZ, xf, dYb=dout)
        dx = _linear(lib, dev, dZ, Wf, w_kn=True) if ctx.needs_input_grad[2] else None
        return (None, None, dx, dW if ctx.needs_input_grad[3] else None, db if ctx.needs_input_grad[4] else None)


class _MeanPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gptr, G, dev, xf):
        ctx.graph = (gptr, G, dev, xf.shape[0])
        return _mean_pool(_lib.load(), dev, xf, gptr, G)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dpooled):
        gptr, G, dev, n = ctx.graph
        dH = _mean_pool_backward(_lib.load(), dev, dpooled.to(torch.float32).contiguous(), gptr, G, n)
        return None, None, None, dH


def global_mean_pool(x, batch, size=None):
    """PyG's global_mean_pool on the pool kernel: x [n, F] floating point, batch [n] integer graph ids, non-negative and
    sorted (PyG's Batch convention; None = one graph), size = number of graphs (default batch.max() + 1).  Returns f32
    [size, F]; a graph id without nodes pools to 0.  Differentiable with respect to x.  At most one device-to-host read."""
    dev = _lib.require_gpu(x.device)
    if x.dim() != 2 or not x.is_floating_point():
        raise ValueError(f"x must be a floating-point [num_nodes, F] tensor, got {x.dtype} {tuple(x.shape)}")
    n = x.shape[0]
    if batch is None:
        batch = torch.zeros((n,), dtype=torch.int64, device=dev)
        size = 1 if size is None else size
    if batch.dim() != 1 or batch.shape[0] != n or batch.is_floating_point() or batch.is_complex() or batch.dtype == torch.bool:
        raise ValueError(f"batch must be an integer [num_nodes] = [{n}] tensor, got {batch.dtype} {tuple(batch.shape)}")
    batch = batch.to(dev).long()
    if n:
        first, last, unsorted = torch.stack([batch[0], batch[-1], (batch[1:] < batch[:-1]).sum()]).tolist()
        if unsorted:
            raise ValueError("batch must be sorted (PyG Batch convention; unsorted batches are not supported)")
        if first < 0:
            raise ValueError(f"batch ids must be non-negative (min {first})")
    G = (last + 1 if n else 0) if size is None else int(size)
    if G < 0 or (n and last >= G):
        raise ValueError(f"size {G} does not cover the batch ids (max {last if n else None})")
    gptr = torch.searchsorted(batch, torch.arange(G + 1, device=dev)).to(torch.int32)
    xf = x.to(torch.float32).contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        return _MeanPoolFunction.apply(gptr, G, dev, xf)
    return _mean_pool(_lib.load(), dev, xf, gptr, G)


class GNNNetwork(GraphPolicyValueNetwork):
    """BaseNetwork-style wrapper (BaseNetwork.py:9-54; reference implementation of the contract:
    pv_network_cnn.py:50-140) around the GNN.  `optimised_model` of the reference (TensorRT) has no counterpart:
    the HIP kernels are the inference path."""

    def __init__(self):
        super().__init__(NUM_FEATURES, HIDDEN_DIM, NUM_GCN_LAYERS, POLICY_OUTPUT_SIZE)
        self._name = "GNN"

    @property
    def name(self):
        return self._name

    def prep_for_inference(self, model_path):
        """BaseNetwork.py:21-32 minus the TensorRT compile."""
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.load_state_dict(torch.load(model_path, map_location=device, weights_only=True))
        self.eval()
        self.to(device)
        if device.type == "cuda":
            self.packed_weights(device)

    def preprocess_input(self, game_state_arrays):
        """List of State.to_array() triples -> uint8 [n,72] state records (the input the GNN kernels accept)."""
        return pack_states(game_state_arrays, self.board_size)

    def train_model(self, data_loader, optimizer, loss_fn, device='cpu', num_epochs=10):
        pass  # stub in the reference as well (pv_network_cnn.py:139-140); training is SURVEY 8(f1), a later row


def pack_states(game_state_arrays, board_size=BOARD_SIZE):
    """List of State.to_array() triples -> uint8 [n,72] state records, for a network of any shape.  plies_played is not part of
    to_array() and is not a network input; it is stored as 0."""
    out = np.zeros((len(game_state_arrays), 72), dtype=np.uint8)
    for i, (player, enemy, walls) in enumerate(game_state_arrays):
        out[i] = game_logic.pack_state72(player, enemy, walls, 0, board_size)
    return out


def create_network(hidden_dim=None, num_gcn_layers=None):
    """pv_network_gnn.py:68-80 (path taken from constants.PV_NETWORK_PATH like pv_network_cnn.py:144-155).  hidden_dim /
    num_gcn_layers (default HIDDEN_DIM / NUM_GCN_LAYERS) shape the network written when no best.pth exists yet."""
    model_path = PV_NETWORK_PATH + 'best.pth'
    if os.path.exists(model_path):
        return
    model = GraphPolicyValueNetwork(NUM_FEATURES, HIDDEN_DIM if hidden_dim is None else hidden_dim,
                                    NUM_GCN_LAYERS if num_gcn_layers is None else num_gcn_layers, POLICY_OUTPUT_SIZE)
    os.makedirs(PV_NETWORK_PATH, exist_ok=True)
    torch.save(model.state_dict(), model_path)


def shape_of_state_dict(sd):
    """(num_features, hidden_dim, num_gcn_layers, policy_output_size) of a GraphPolicyValueNetwork state_dict."""
    L = 0
    while f"gcn_layers.{L}.lin.weight" in sd:
        L += 1
    if L == 0 or "policy_head.2.weight" not in sd:
        raise ValueError("not a GraphPolicyValueNetwork state_dict (no gcn_layers.0.lin.weight / policy_head.2.weight)")
    hidden, features = (int(n) for n in sd["gcn_layers.0.lin.weight"].shape)
    return features, hidden, L, int(sd["policy_head.2.weight"].shape[0])


def load_network(path, device=None):
    """The network a .pth file holds, whatever its shape: GNNNetwork for the default 6/128/3 (the fused kernels), otherwise a
    GraphPolicyValueNetwork of the shape the state_dict implies -- or, for the reference's CNN state_dict, a CNNNetwork of its
    shape (pv_network_cnn.py).  Loaded onto `device` (default: the current GPU, else the CPU) in eval mode."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    sd = torch.load(path, map_location=device, weights_only=True)
    from . import pv_network_cnn
    if pv_network_cnn.is_cnn_state_dict(sd):
        model = pv_network_cnn.CNNNetwork(*pv_network_cnn.shape_of_state_dict(sd))
        model.load_state_dict(sd)
        return model.to(device).eval()
    shape = shape_of_state_dict(sd)
    if shape == (NUM_FEATURES, HIDDEN_DIM, NUM_GCN_LAYERS, POLICY_OUTPUT_SIZE):
        model = GNNNetwork()
    else:
        model = GraphPolicyValueNetwork(*shape)
    model.load_state_dict(sd)
    return model.to(device).eval()


if __name__ == '__main__':
    create_network()
