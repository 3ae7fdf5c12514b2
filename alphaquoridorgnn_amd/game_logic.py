"""Quoridor game logic -- drop-in for the reference's game_logic.py, backed by the HIP library.

`State` keeps the reference's constructor, public mutable attributes and method names
(game_logic.py:15-54, :96-117, :195-196, :359-395).  The cheap bookkeeping (next, is_done, to_array ...) is
host Python like the reference; everything that walks the board -- legal_actions(), legal_actions_pos(),
legal_actions_wall() -- runs the gfx950 kernel (aqg_legal_actions) on a batch of one.  Batched callers
should use `legal_actions_batch` / `next_batch` / `status_batch` on device tensors of state72 records.
"""
import numpy as np
import torch

from . import _lib
from .constants import BOARD_SIZE, NUM_WALLS, NUM_PLIES_FOR_DRAW, num_actions  # noqa: F401

MOVEMENT_DIRECTIONS = [(-1, 0), (1, 0), (0, -1), (0, 1)]  # U, D, L, R (game_logic.py:11)
STATE72 = 72
MAX_LEGAL = _lib.MAX_LEGAL


# ------------------------------------------------------------------ batched device API
def legal_actions_batch(states72, board_size=BOARD_SIZE, want_mask=True):
    """states72: uint8 [B,72] device tensor -> (mask u8 [B,A] or None, order u8 [B,136], count i32 [B])."""
    dev = _lib.require_gpu(states72.device)
    lib = _lib.load()
    B = states72.shape[0]
    A = num_actions(board_size)
    mask = torch.empty((B, A), dtype=torch.uint8, device=dev) if want_mask else None
    order = torch.empty((B, MAX_LEGAL), dtype=torch.uint8, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.check(lib.aqg_legal_actions(board_size, _lib.ptr(states72), B, _lib.ptr(mask), _lib.ptr(order), _lib.ptr(count),
                                     _lib.stream_ptr(dev)), "aqg_legal_actions")
    return mask, order, count


def next_batch(states72, actions, board_size=BOARD_SIZE):
    dev = _lib.require_gpu(states72.device)
    out = torch.empty_like(states72)
    actions = actions.to(device=dev, dtype=torch.int32).contiguous()
    _lib.check(_lib.load().aqg_state_next(board_size, _lib.ptr(states72), _lib.ptr(actions), states72.shape[0],
                                          _lib.ptr(out), _lib.stream_ptr(dev)), "aqg_state_next")
    return out


def status_batch(states72, board_size=BOARD_SIZE, plies_for_draw=NUM_PLIES_FOR_DRAW):
    """flags u8 [B]: bit0 = is_lose, bit1 = is_draw."""
    dev = _lib.require_gpu(states72.device)
    out = torch.empty((states72.shape[0],), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().aqg_state_status(board_size, _lib.ptr(states72), states72.shape[0], plies_for_draw,
                                            _lib.ptr(out), _lib.stream_ptr(dev)), "aqg_state_status")
    return out


# ------------------------------------------------------------------ may a record start a game?  (include/aqgnn.h, "start positions")
def _check_constants(board_size, num_walls, plies_for_draw):
    from .constants import board_params
    walls, draw = board_params(board_size)
    return int(walls if num_walls is None else num_walls), int(draw if plies_for_draw is None else plies_for_draw)


def check_states_batch(states72, board_size=BOARD_SIZE, num_walls=None, plies_for_draw=None):
    """flags u8 [B] of states72 (uint8 [B,72] device tensor): 0 = the record may start a game, else the AQG_CHECK_* bits
    (_lib.CHECK_BOARD ... _lib.CHECK_NO_PATH).  num_walls / plies_for_draw: the board's own unless given."""
    dev = _lib.require_gpu(states72.device)
    if states72.dtype != torch.uint8 or states72.dim() != 2 or states72.shape[1] != STATE72:
        raise ValueError("states72 must be a uint8 [B,72] device tensor")
    walls, draw = _check_constants(board_size, num_walls, plies_for_draw)
    states72 = states72.contiguous()
    out = torch.empty((states72.shape[0],), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().aqg_states72_check(board_size, _lib.ptr(states72), states72.shape[0], walls, draw, _lib.ptr(out),
                                              _lib.stream_ptr(dev)), "aqg_states72_check")
    return out


def check_state_host(rec72, board_size=BOARD_SIZE, num_walls=None, plies_for_draw=None):
    """The checker's byte for one record in host memory, by the host build of the kernel's own predicate (aqg_host_check_state)."""
    import ctypes
    walls, draw = _check_constants(board_size, num_walls, plies_for_draw)
    rec = np.ascontiguousarray(rec72, dtype=np.uint8).reshape(STATE72)
    flags = _lib.load().aqg_host_check_state(board_size, rec.ctypes.data_as(ctypes.c_void_p), walls, draw)
    if flags < 0:
        raise ValueError(f"aqg_host_check_state refuses board_size {board_size}, num_walls {walls}, plies_for_draw {draw}")
    return flags


def _reaches_row(N, walls, start, obstacle, goal_row):
    """Can a pawn on `start` reach row `goal_row` while the other pawn stands on `obstacle` (None = no other pawn: the walls alone)?
    Breadth-first over the pawn moves of game_logic.py:120-192 (steps, straight jumps, side jumps), in plain Python."""
    S = N - 1

    def wall(sx, sy, kind):
        return 0 <= sx < S and 0 <= sy < S and walls[sx * S + sy] == kind

    def is_open(t, d):          # d: 0 up, 1 down, 2 left, 3 right
        x, y = divmod(t, N)
        if d == 0:
            return x > 0 and not (wall(x - 1, y, 1) or wall(x - 1, y - 1, 1))
        if d == 1:
            return x < N - 1 and not (wall(x, y, 1) or wall(x, y - 1, 1))
        if d == 2:
            return y > 0 and not (wall(x, y - 1, 2) or wall(x - 1, y - 1, 2))
        return y < N - 1 and not (wall(x, y, 2) or wall(x - 1, y, 2))

    step = (-N, N, -1, 1)
    seen, queue = {start}, [start]
    while queue:
        t = queue.pop(0)
        if t // N == goal_row:
            return True
        nxt = []
        for d in range(4):
            if not is_open(t, d):
                continue
            n = t + step[d]
            if n != obstacle:
                nxt.append(n)
            elif is_open(n, d):
                nxt.append(n + step[d])
            else:
                nxt += [n + step[s] for s in ((2, 3) if d < 2 else (0, 1)) if is_open(n, s)]
        for n in nxt:
            if n not in seen:
                seen.add(n)
                queue.append(n)
    return False


def check_state_reference(rec72, board_size=BOARD_SIZE, num_walls=None, plies_for_draw=None):
    """The checker, stated in plain Python/numpy (include/aqgnn.h, "start positions"): the byte aqg_states72_check and
    aqg_host_check_state give for this record."""
    N = int(board_size)
    num_walls, draw = _check_constants(N, num_walls, plies_for_draw)
    rec = np.asarray(rec72, dtype=np.uint8).reshape(STATE72)
    V, S = N * N, N - 1
    ppos, pleft, epos, eleft = (int(x) for x in rec[:4])
    walls = [int(x) for x in rec[4:4 + S * S]]
    plies = int(rec[68]) | (int(rec[69]) << 8)
    flags = 0
    if int(rec[70]) != N or ppos >= V or epos >= V:
        flags |= _lib.CHECK_BOARD
    overlap = any(walls[i] == 1 and walls[i + 1] == 1 for i in range(S * S - 1) if i % S != S - 1) or \
        any(walls[i] == 2 and walls[i + S] == 2 for i in range(S * S - S))
    if any(w > 2 for w in walls) or overlap:
        flags |= _lib.CHECK_WALLS
    placed = sum(1 for w in walls if w in (1, 2))
    if pleft > num_walls or eleft > num_walls or pleft + eleft + placed != 2 * num_walls:
        flags |= _lib.CHECK_WALL_COUNT
    if ppos == V - 1 - epos:
        flags |= _lib.CHECK_SAME_SQUARE
    if epos // N == 0 or ppos // N == 0 or plies >= draw:
        flags |= _lib.CHECK_OVER
    if plies % 2:
        flags |= _lib.CHECK_ODD_PLY
    if not flags & (_lib.CHECK_BOARD | _lib.CHECK_WALLS | _lib.CHECK_SAME_SQUARE):
        other = V - 1 - epos
        # through the walls alone: a pawn standing in the other's only corridor is a position of real games, not a bad record
        if not (_reaches_row(N, walls, ppos, None, 0) and _reaches_row(N, walls, other, None, N - 1)):
            flags |= _lib.CHECK_NO_PATH
    return flags


# ------------------------------------------------------------------ the left-right mirror (include/aqgnn.h, "training augmentation")
def _mirror_cells(cells, width):
    """Cell i of a grid of lines of `width` cells, mirrored inside its line."""
    return cells - cells % width + (width - 1 - cells % width)


def mirror_actions(actions, board_size=BOARD_SIZE):
    """The mirror images of an integer array of actions (column y -> N - 1 - y): a pawn action by its tile, a horizontal / vertical
    wall action by its slot inside its own block.  An involution; int64 of the same shape."""
    N = int(board_size)
    if N % 2 == 0 or not 3 <= N <= 9:
        raise ValueError("board_size must be 3, 5, 7 or 9")
    a = np.asarray(actions, dtype=np.int64)
    V, W = N * N, N - 1
    NW = W * W
    if a.size and (a.min() < 0 or a.max() >= V + 2 * NW):
        raise ValueError(f"an action is outside 0..{V + 2 * NW - 1}, the actions of a {N}x{N} board")
    block = np.where(a < V, 0, np.where(a < V + NW, V, V + NW))
    return block + np.where(a < V, _mirror_cells(a, N), _mirror_cells(a - block, W))


def mirror_action(a, board_size=BOARD_SIZE):
    return int(mirror_actions(int(a), board_size))


def mirror_record(rec72):
    """The mirror of a state72 record (uint8 [72], or [B,72] of one board size), in numpy; N is read from byte 70.  A position byte
    that is no tile of the board is copied through, as the kernel does."""
    rec = np.asarray(rec72, dtype=np.uint8)
    if rec.shape[-1] != STATE72 or rec.ndim not in (1, 2):
        raise ValueError("mirror_record takes state72 records: uint8 [72] or [B,72]")
    out = rec.copy()
    if rec.size == 0:
        return out
    N = int(rec.reshape(-1, STATE72)[0, 70])
    if N % 2 == 0 or not 3 <= N <= 9 or (rec[..., 70] != N).any():
        raise ValueError("byte 70 of every record must hold the same board size 3, 5, 7 or 9")
    for k in (0, 2):
        p = rec[..., k].astype(np.int64)
        out[..., k] = np.where(p < N * N, _mirror_cells(p, N), p).astype(np.uint8)
    nw = (N - 1) ** 2
    out[..., 4:4 + nw] = rec[..., 4 + _mirror_cells(np.arange(nw), N - 1)]
    return out


_ONES = {}


def _mirror_launch(states72, pi, board_size):
    x = states72 if states72 is not None else pi
    dev = _lib.require_gpu(x.device)
    A = num_actions(board_size)
    if states72 is not None and (states72.dtype != torch.uint8 or states72.dim() != 2 or states72.shape[1] != STATE72):
        raise ValueError("states72 must be a uint8 [B,72] device tensor")
    if pi is not None and (pi.dtype != torch.float32 or pi.dim() != 2 or pi.shape[1] != A):
        raise ValueError(f"pi must be a float32 [B,{A}] device tensor on a {board_size}x{board_size} board")
    x = x.contiguous()
    out = torch.empty_like(x)
    B = x.shape[0]
    flips = _ONES.get(dev)                      # "every row": one table per device, grown when a larger batch comes
    if flips is None or flips.shape[0] < B:
        flips = _ONES[dev] = torch.ones((max(B, 1024),), dtype=torch.uint8, device=dev)
    s, p = (x, None) if states72 is not None else (None, x)
    _lib.check(_lib.load().aqg_augment_gather(board_size, A, _lib.ptr(s), _lib.ptr(p), None, None, _lib.ptr(flips), 0, 0, 0, B,
                                              _lib.ptr(out if s is not None else None), _lib.ptr(out if p is not None else None),
                                              None, _lib.stream_ptr(dev)), "aqg_augment_gather")
    return out


def mirror_batch(states72, board_size=BOARD_SIZE):
    """states72: uint8 [B,72] device tensor -> the mirrored records, on the device (aqg_augment_gather, every row flipped)."""
    return _mirror_launch(states72, None, board_size)


def mirror_policy_batch(pi, board_size=BOARD_SIZE):
    """pi: float32 [B,A] device tensor -> the rows permuted by the mirror, out[b, mirror(a)] = pi[b, a], on the device."""
    return _mirror_launch(None, pi, board_size)


def pack_state72(player, enemy, walls, plies_played, board_size):
    r = np.zeros(STATE72, dtype=np.uint8)
    r[0], r[1] = int(player[0]), int(player[1])
    r[2], r[3] = int(enemy[0]), int(enemy[1])
    w = np.asarray(walls, dtype=np.uint8)
    r[4:4 + len(w)] = w
    r[68] = plies_played & 0xFF
    r[69] = (plies_played >> 8) & 0xFF
    r[70] = board_size
    return r


# ------------------------------------------------------------------ reference-shaped single state
class State:
    """
    :param walls: 1 by (N-1)^2 int list from the current player's perspective; 0 none, 1 horizontal, 2 vertical,
        slot i = 2x2 block with top-left tile (i // (N-1), i % (N-1)).
    :param player: [position, walls left], position in the player's own frame.
    :param enemy: [position, walls left], position in the ENEMY's own frame.
    :param plies_played: plies played so far.
    """

    def __init__(self, board_size=BOARD_SIZE, num_walls=NUM_WALLS, player=None, enemy=None, walls=None, plies_played=0):
        self.N = board_size
        N = self.N
        if N % 2 == 0:
            raise ValueError('The board size must be an odd number.')
        self.player = player if player is not None else [0] * 2
        self.enemy = enemy if enemy is not None else [0] * 2
        self.walls = walls if walls is not None else [0] * ((N - 1) ** 2)
        self.plies_played = plies_played
        if player is None or enemy is None:
            init_pos = N * (N - 1) + N // 2
            self.player[0] = init_pos
            self.player[1] = num_walls
            self.enemy[0] = init_pos
            self.enemy[1] = num_walls

    # -- cheap host-side bookkeeping (game_logic.py:43-54, :96-100, :359-395)
    def is_lose(self):
        return self.enemy[0] // self.N == 0

    def is_draw(self):
        from . import constants
        draw = NUM_PLIES_FOR_DRAW if self.N == BOARD_SIZE else constants.board_params(self.N)[1]
        return self.plies_played >= draw

    def is_done(self):
        return self.is_lose() or self.is_draw()

    def to_array(self):
        return [list(self.player), list(self.enemy), list(self.walls)]

    def is_first_player(self):
        return self.plies_played % 2 == 0

    def rotate_walls(self):
        self.walls = list(self.walls)[::-1]

    @classmethod
    def from_record(cls, rec):
        """State of a state72 record (the layout in include/aqgnn.h)."""
        N = int(rec[70])
        nw = (N - 1) ** 2
        return cls(board_size=N, player=[int(rec[0]), int(rec[1])], enemy=[int(rec[2]), int(rec[3])],
                   walls=[int(x) for x in rec[4:4 + nw]], plies_played=int(rec[68]) | (int(rec[69]) << 8))

    def mirror(self):
        """The left-right mirror of this state (mirror_record): a symmetry of the rules."""
        return State.from_record(mirror_record(self.record()))

    def next(self, action):
        """game_logic.py:366-391 -- move the pawn or set the wall, turn the board by 180 degrees, swap the players -- by the rule
        header the kernels compile, in its host instantiation (aqg_host_next): one transition code for device and host."""
        import ctypes
        rec, out = self.record(), np.empty(STATE72, dtype=np.uint8)
        if _lib.load().aqg_host_next(self.N, rec.ctypes.data_as(ctypes.c_void_p), int(action), out.ctypes.data_as(ctypes.c_void_p)) != 0:
            raise ValueError(f"action {action} is not an action of a {self.N}x{self.N} board")
        return State.from_record(out)

    # -- board-walking queries: HIP kernel, batch of one
    def record(self):
        return pack_state72(self.player, self.enemy, self.walls, self.plies_played, self.N)

    def _device_record(self, rec=None):
        dev = _lib.require_gpu()
        return torch.from_numpy(self.record() if rec is None else rec).to(dev).unsqueeze(0)

    def legal_actions(self):
        """Ordered like the reference: pawn moves (U,D,L,R / jumps), then per wall slot H, V (game_logic.py:103-117)."""
        _, order, count = legal_actions_batch(self._device_record(), self.N, want_mask=False)
        n = int(count.item())
        return [int(a) for a in order[0, :n].cpu().numpy()]

    def legal_actions_pos(self, pos):
        """Pawn destinations from `pos` (game_logic.py:120-192): the pawn-move prefix of the legal list of the
        same position with the mover placed on `pos`."""
        rec = self.record()
        rec[0] = int(pos)
        rec[1] = 0          # no walls left -> the list is the pawn moves only
        _, order, count = legal_actions_batch(self._device_record(rec), self.N, want_mask=False)
        n = int(count.item())
        return [int(a) for a in order[0, :n].cpu().numpy()]

    def legal_actions_wall(self, pos):
        """Legal wall placements at slot `pos` (game_logic.py:195-357)."""
        rec = self.record()
        if rec[1] == 0:
            rec[1] = 1      # legality of a slot does not depend on the wall count (:113 gates the loop only)
        mask, _, _ = legal_actions_batch(self._device_record(rec), self.N, want_mask=True)
        N = self.N
        m = mask[0].cpu().numpy()
        out = []
        if m[N * N + pos]:
            out.append(N * N + pos)
        if m[N * N + (N - 1) ** 2 + pos]:
            out.append(N * N + (N - 1) ** 2 + pos)
        return out

    def __str__(self):
        """Compact ASCII render (the reference's :398-456 debug print is out of scope; this is our own)."""
        N = self.N
        me, en = self.player[0], N * N - 1 - self.enemy[0]
        if not self.is_first_player():
            pass
        rows = []
        for x in range(N):
            rows.append(" ".join("P" if x * N + y == me else ("E" if x * N + y == en else ".") for y in range(N)))
        walls = [f"{'H' if w == 1 else 'V'}{i}" for i, w in enumerate(self.walls) if w]
        return "\n".join(rows) + f"\nwalls: {' '.join(walls) or '-'}  left: {self.player[1]}/{self.enemy[1]}  ply {self.plies_played}"
