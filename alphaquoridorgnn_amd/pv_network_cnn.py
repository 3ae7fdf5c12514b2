"""Policy-Value CNN -- drop-in for the reference's pv_network_cnn.py, its inference executed by hand-written gfx950 kernels.

Call surface kept (pv_network_cnn.py:11-155): NUM_FILTERS, NUM_RESIDUAL_BLOCKS, INPUT_SHAPE, POLICY_OUTPUT_SIZE, `ConvBN`,
`ResidualBlock`, `CNNNetwork` with submodules `conv`, `residual_blocks`, `global_avg_pool`, `policy_head`, `value_head` (so a
`best.pth` the reference wrote loads unchanged), the BaseNetwork contract (`name`, `preprocess_input`, `predict`,
`prep_for_inference` without TensorRT, `train_model` a stub as in the reference) and `create_network()`.

Added: the shape as arguments, `CNNNetwork(num_filters, num_residual_blocks, board_size)`; `forward_states(states)` on board
records; `packed_weights(device)` / `cnn_net(device)`, the descriptor of the engine's evaluator='cnn' (include/aqgnn.h aqg_cnn_net).

`forward(x)` on a [B,6,N,N] GPU tensor, in eval mode, with autograd not recording, runs csrc/cnn_forward.hip (eval-mode BatchNorm
folded at pack time, one implicit-GEMM launch per conv on the f32-input MFMA).  Otherwise -- training-mode BatchNorm, a CPU
tensor, a recording autograd -- it runs the stock nn modules: the reference's own arithmetic.  Training on HIP: train_network.CNNTrainer.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import game_logic
from .constants import BOARD_SIZE, num_actions as policy_size_of

NUM_FILTERS = 128          # pv_network_cnn.py:14
NUM_RESIDUAL_BLOCKS = 16   # :15
INPUT_SHAPE = (6, BOARD_SIZE, BOARD_SIZE)                           # :16
POLICY_OUTPUT_SIZE = policy_size_of(BOARD_SIZE)                    # :17
CNN_NETWORK_PATH = f"models/CNN/{BOARD_SIZE}x{BOARD_SIZE}/"        # the reference's PV_NETWORK_PATH with PV_NETWORK_NAME = 'CNN'

# inclusive bounds of the shapes the HIP kernels take (CNNNetwork raises ValueError outside them)
SHAPE_LIMITS = {"num_filters": (1, 512), "num_residual_blocks": (0, 40), "policy_output_size": (1, 4096)}
BOARD_SIZES = (3, 5, 7, 9)


# Convolutional layer with batch normalization (pv_network_cnn.py:21-31)
class ConvBN(nn.Module):
    def __init__(self, num_channels, num_filters):
        super().__init__()
        self.conv = nn.Conv2d(num_channels, num_filters, kernel_size=3, padding='same', bias=False)
        self.bn = nn.BatchNorm2d(num_filters)

    def forward(self, x):
        return self.bn(self.conv(x))


# Residual block (pv_network_cnn.py:35-46)
class ResidualBlock(nn.Module):
    def __init__(self, num_filters):
        super().__init__()
        self.conv_bn1 = ConvBN(num_filters, num_filters)
        self.conv_bn2 = ConvBN(num_filters, num_filters)

    def forward(self, x):
        residual = x
        x = F.relu(self.conv_bn1(x))
        x = self.conv_bn2(x)
        x = x + residual
        return F.relu(x)


class CNNNetwork(nn.Module):
    """pv_network_cnn.py:50-140 at any shape within SHAPE_LIMITS (6 input planes, board_size 3/5/7/9)."""

    def __init__(self, num_filters=NUM_FILTERS, num_residual_blocks=NUM_RESIDUAL_BLOCKS, board_size=BOARD_SIZE):
        super().__init__()
        if board_size not in BOARD_SIZES or isinstance(board_size, bool):
            raise ValueError(f"board_size must be one of {BOARD_SIZES}, got {board_size!r}")
        policy_output_size = policy_size_of(board_size)
        for name, v in (("num_filters", num_filters), ("num_residual_blocks", num_residual_blocks),
                        ("policy_output_size", policy_output_size)):
            lo, hi = SHAPE_LIMITS[name]
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an integer in [{lo}, {hi}] (the limit of the HIP kernels), got {v!r}")
        self._name = 'CNN'
        self.num_filters = int(num_filters)
        self.num_residual_blocks = int(num_residual_blocks)
        self.board_size = int(board_size)
        self.policy_output_size = policy_output_size
        self.optimised_model = None            # BaseNetwork.py:13 (TensorRT's compiled copy): the HIP kernels are the inference path

        self.conv = ConvBN(INPUT_SHAPE[0], self.num_filters)
        self.residual_blocks = nn.Sequential(*[ResidualBlock(self.num_filters) for _ in range(self.num_residual_blocks)])
        self.global_avg_pool = nn.AdaptiveAvgPool2d(1)
        self.policy_head = nn.Sequential(nn.Flatten(), nn.Linear(self.num_filters, policy_output_size), nn.Softmax(dim=1))
        self.value_head = nn.Sequential(nn.Flatten(), nn.Linear(self.num_filters, 1), nn.Tanh())
        self._packed = None
        self._packed_key = None

    @property
    def name(self):
        return self._name

    # ---------------------------------------------------------------- forward
    def forward(self, x):
        """x [B,6,N,N] -> (policy [B,A] softmaxed, value [B,1] tanh'ed).  HIP kernels for a GPU tensor in eval mode with autograd
        not recording; the stock modules otherwise (pv_network_cnn.py:77-84)."""
        if x.is_cuda and not self.training and not torch.is_grad_enabled():
            return self._forward_planes(x)
        return self._forward_stock(x)

    def _forward_stock(self, x):
        x = F.relu(self.conv(x))
        x = self.residual_blocks(x)
        x = self.global_avg_pool(x)
        return self.policy_head(x), self.value_head(x)

    def _outputs(self, B, dev, want_logits):
        f32 = dict(dtype=torch.float32, device=dev)
        A = self.policy_output_size
        nws = int(_lib.load().aqg_cnn_workspace_floats(self.board_size, self.num_filters, A, max(B, 1)))
        return dict(ws=torch.empty((max(nws, 1),), **f32), nws=nws, pooled=torch.empty((B, self.num_filters), **f32),
                    policy=torch.empty((B, A), **f32), value=torch.empty((B,), **f32),
                    logits=torch.empty((B, A), **f32) if want_logits else None, vpre=torch.empty((B,), **f32) if want_logits else None)

    def _finish(self, o, want_logits, want_pooled):
        out = (o["policy"], o["value"].unsqueeze(1))
        if want_logits:
            out = out + (o["logits"], o["vpre"])
        if want_pooled:
            out = out + (o["pooled"],)
        return out

    def _forward_planes(self, x, want_logits=False, want_pooled=False):
        N = self.board_size
        if x.dim() != 4 or tuple(x.shape[1:]) != (6, N, N):
            raise ValueError(f"the HIP forward takes [B, 6, {N}, {N}] planes, got {tuple(x.shape)}")
        dev = _lib.require_gpu(x.device)
        lib = _lib.load()
        x = x.to(torch.float32).contiguous()
        B = x.shape[0]
        o = self._outputs(B, dev, want_logits)
        net = self.cnn_net(dev)
        _lib.check(lib.aqg_cnn_forward_planes(N, _lib.ptr(x), B, ctypes.byref(net), None, _lib.ptr(o["ws"]), o["nws"],
                                              _lib.ptr(o["pooled"]), _lib.ptr(o["logits"]), _lib.ptr(o["policy"]), _lib.ptr(o["vpre"]),
                                              _lib.ptr(o["value"]), _lib.stream_ptr(dev)), "aqg_cnn_forward_planes")
        return self._finish(o, want_logits, want_pooled)

    def forward_states(self, states, want_logits=False, want_pooled=False, active=None):
        """states: uint8 device tensor of state72 rows [B,72] or of the engine's 24-byte records [B,24] -> (policy [B,A], value
        [B,1]) (+ (logits [B,A], value_pre [B]) with want_logits, + pooled [B,F] with want_pooled).  active (uint8 [B], optional):
        rows with active != 1 are skipped and their outputs left as they were (here: uninitialised)."""
        states = torch.as_tensor(states)
        if states.dim() != 2 or states.shape[1] not in (72, 24) or states.dtype != torch.uint8:
            raise ValueError("forward_states takes uint8 state72 rows [B,72] or engine records [B,24]")
        dev = _lib.require_gpu(states.device if states.is_cuda else None)
        lib = _lib.load()
        states = states.to(dev).contiguous()
        B = states.shape[0]
        fmt = 0 if states.shape[1] == 72 else 1
        o = self._outputs(B, dev, want_logits)
        net = self.cnn_net(dev)
        act = None if active is None else torch.as_tensor(active, dtype=torch.uint8).to(dev).contiguous()
        _lib.check(lib.aqg_cnn_forward_boards(self.board_size, _lib.ptr(states), fmt, B, ctypes.byref(net), _lib.ptr(act),
                                              _lib.ptr(o["ws"]), o["nws"], _lib.ptr(o["pooled"]), _lib.ptr(o["logits"]),
                                              _lib.ptr(o["policy"]), _lib.ptr(o["vpre"]), _lib.ptr(o["value"]), _lib.stream_ptr(dev)),
                   "aqg_cnn_forward_boards")
        return self._finish(o, want_logits, want_pooled)

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

    def preprocess_input(self, game_state_arrays):
        """pv_network_cnn.py:88-114: list of State.to_array() triples -> float32 [n, 6, N, N] planes."""
        N = self.board_size
        out = np.zeros((len(game_state_arrays), 6, N, N), dtype=np.float32)
        for i, (player, enemy, walls) in enumerate(game_state_arrays):
            out[i, 0, player[0] // N, player[0] % N] = 1       # player pawn
            out[i, 1, :, :] = player[1]                        # player walls in hand
            out[i, 2, enemy[0] // N, enemy[0] % N] = 1         # enemy pawn (in the enemy's own frame, as the reference)
            out[i, 3, :, :] = enemy[1]                         # enemy walls in hand
            for wall_index, wall in enumerate(walls):
                if wall != 0:
                    row, col = divmod(N * (wall_index // (N - 1)) + (wall_index % (N - 1)), N)
                    if wall == 1:
                        out[i, 4, row, col] = 1                # horizontal
                    elif wall == 2:
                        out[i, 5, row, col] = 1                # vertical
        return out

    def prep_for_inference(self, model_path):
        """BaseNetwork.py:21-32 minus the TensorRT compile."""
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.load_state_dict(torch.load(model_path, map_location=device, weights_only=True))
        self.eval()
        self.to(device)
        if device.type == "cuda":
            self.packed_weights(device)

    def train_model(self, data_loader, optimizer, loss_fn, device='cpu', num_epochs=10):
        pass  # a stub in the reference as well (pv_network_cnn.py:139-140)

    # ---------------------------------------------------------------- packed weights (aqg_cnn_pack)
    def _convs(self):
        return [self.conv] + [cb for blk in self.residual_blocks for cb in (blk.conv_bn1, blk.conv_bn2)]

    def _pack_tensors(self):
        ts = []
        for cb in self._convs():
            ts += [cb.conv.weight, cb.bn.weight, cb.bn.bias, cb.bn.running_mean, cb.bn.running_var]
        return ts + [self.policy_head[1].weight, self.policy_head[1].bias, self.value_head[1].weight, self.value_head[1].bias]

    def weights_key(self):
        """(data pointer, version counter) of every tensor the pack reads, and every BatchNorm's eps: changes whenever one of them
        is replaced or updated in place."""
        return tuple((t.data_ptr(), t._version) for t in self._pack_tensors()) + tuple(float(cb.bn.eps) for cb in self._convs())

    def packed_weights(self, device):
        """float32 device buffer of aqg_cnn_pack (eval-mode BatchNorm folded, weights in the kernel layout); the SAME tensor while no
        parameter or running statistic has changed, a new one after any change."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (str(dev),) + self.weights_key()
        if self._packed is None or key != self._packed_key:
            lib = _lib.load()
            F_, L, A = self.num_filters, self.num_residual_blocks, self.policy_output_size
            n = int(lib.aqg_cnn_packed_floats(F_, L, A))
            if n == 0:
                _lib.check(-1, "aqg_cnn_packed_floats (shape outside the kernels' limits)")
            out = torch.empty((n,), dtype=torch.float32, device=dev)
            src = [t.detach().to(dev, torch.float32).contiguous() for t in self._pack_tensors()]
            ptrs = (ctypes.c_void_p * len(src))(*[t.data_ptr() for t in src])
            eps = (ctypes.c_float * (2 * L + 1))(*[float(cb.bn.eps) for cb in self._convs()])
            _lib.check(lib.aqg_cnn_pack(F_, L, A, ptrs, eps, _lib.ptr(out), _lib.stream_ptr(dev)), "aqg_cnn_pack")
            self._packed = out
            self._packed_key = key
        return self._packed

    def invalidate_packed(self):
        self._packed = None
        self._packed_key = None

    def cnn_net(self, device):
        """The ctypes descriptor of this network for aqg_cnn_forward_boards and the engine's evaluator='cnn' (include/aqgnn.h
        aqg_cnn_net): its shape and the packed buffer of packed_weights(device)."""
        net = _lib.CnnNetStruct()
        net.board_size, net.num_filters, net.num_blocks, net.policy_size = (self.board_size, self.num_filters, self.num_residual_blocks,
                                                                            self.policy_output_size)
        net.packed = self.packed_weights(device).data_ptr()
        return net


def state_dict_keys(num_residual_blocks=NUM_RESIDUAL_BLOCKS):
    """The state_dict keys of a CNNNetwork (the reference's: 202 for 16 blocks)."""
    def conv_bn(p):
        return [p + "conv.weight"] + [p + "bn." + k for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    keys = conv_bn("conv.")
    for i in range(num_residual_blocks):
        keys += conv_bn(f"residual_blocks.{i}.conv_bn1.") + conv_bn(f"residual_blocks.{i}.conv_bn2.")
    return keys + ["policy_head.1.weight", "policy_head.1.bias", "value_head.1.weight", "value_head.1.bias"]


def is_cnn_state_dict(sd):
    return "conv.conv.weight" in sd and "policy_head.1.weight" in sd


def shape_of_state_dict(sd):
    """(num_filters, num_residual_blocks, board_size) of a CNNNetwork state_dict."""
    if not is_cnn_state_dict(sd):
        raise ValueError("not a CNNNetwork state_dict (no conv.conv.weight / policy_head.1.weight)")
    L = 0
    while f"residual_blocks.{L}.conv_bn1.conv.weight" in sd:
        L += 1
    filters = int(sd["conv.conv.weight"].shape[0])
    A = int(sd["policy_head.1.weight"].shape[0])
    sizes = [n for n in BOARD_SIZES if policy_size_of(n) == A]
    if not sizes:
        raise ValueError(f"a policy head of {A} actions matches no board size of {BOARD_SIZES}")
    return filters, L, sizes[0]


def load_network(path, device=None):
    """The CNNNetwork a .pth file holds, of the shape its state_dict implies, on `device` (default: the current GPU, else the CPU)
    in eval mode."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    sd = torch.load(path, map_location=device, weights_only=True)
    model = CNNNetwork(*shape_of_state_dict(sd))
    model.load_state_dict(sd)
    return model.to(device).eval()


def create_network():
    """pv_network_cnn.py:144-155: writes models/CNN/{N}x{N}/best.pth unless it exists."""
    model_path = CNN_NETWORK_PATH + 'best.pth'
    if os.path.exists(model_path):
        return
    model = CNNNetwork()
    os.makedirs(CNN_NETWORK_PATH, exist_ok=True)
    torch.save(model.state_dict(), model_path)


if __name__ == '__main__':
    create_network()
