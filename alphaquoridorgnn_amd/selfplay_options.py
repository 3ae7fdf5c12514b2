"""The self-play options of the engine -- root noise, the target options, tree reuse, resignation -- on the host: their validation
as the library does it, the seeds an engine derives when it is given none, and the one refusal of the paths that play no self-play."""
import numpy as np

from . import _lib
from .constants import num_actions
from .counter_rng import GOLDEN, MASK64, mix64

ROOT_NOISE_ATTEMPTS = 64      # cap of the gamma sampler's rejection loop (csrc/mcts_move.hip ROOT_NOISE_ATTEMPTS)


def default_root_noise_alpha(board_size):
    """The usual "10 / typical number of legal moves" rule, with the board's action count N^2 + 2 (N - 1)^2 for the moves."""
    return 10.0 / num_actions(board_size)


def check_root_noise(eps, alpha):
    """Validate the root-noise options as the library does, on the f32 values its struct holds: eps in [0, 1); alpha in (0, 100]
    when eps > 0.  Returns them as floats (alpha 0.0 when the noise is off)."""
    eps = float(np.float32(eps))
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"root_noise_eps must be in [0, 1) as a float32, not {eps}")
    if eps == 0.0:
        return 0.0, 0.0
    alpha = float(np.float32(alpha))
    if not 0.0 < alpha <= 100.0:
        raise ValueError(f"root_noise_alpha must be in (0, 100] as a float32, not {alpha}")
    return eps, alpha


POLICY_TARGETS = ("visits", "completed_q")      # how a reanalyse pass forms a row's policy target (reanalyse.reanalyse)


def check_completed_q(c_visit=50.0, c_scale=1.0):
    """Validate the constants of the completed-Q transform (include/aqgnn.h, "completed-Q policy targets") as the library does, on the
    float64 values it is given: both finite and >= 0.  Returns them as floats."""
    out = []
    for name, x in (("c_visit", c_visit), ("c_scale", c_scale)):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a finite number >= 0, not {x!r}")
        x = float(x)
        if not (x >= 0.0 and x != float("inf")):                # NaN fails the first
            raise ValueError(f"{name} must be a finite number >= 0, not {x!r}")
        out.append(x)
    return tuple(out)


def check_policy_target(policy_target="visits", c_visit=50.0, c_scale=1.0):
    """Validate the policy-target options of a reanalyse pass: 'visits' (normalised visit counts) or 'completed_q' (the improved policy
    of the completed-Q transform; 'completed-q' is accepted, as the command line spells it).  Returns (policy_target, c_visit, c_scale)."""
    name = policy_target.replace("-", "_") if isinstance(policy_target, str) else policy_target
    if name not in POLICY_TARGETS:
        raise ValueError(f"policy_target must be one of {POLICY_TARGETS}, not {policy_target!r}")
    return (name,) + check_completed_q(c_visit, c_scale)


def check_policy_record(policy_target="visits", policy_c_visit=50.0, policy_c_scale=1.0, record_history=True):
    """Validate the recorded policy target of a self-play engine (include/aqgnn.h, "recording completed-Q targets during self-play"):
    check_policy_target's names and constants; 'completed_q' needs the history its rows are a column of.  Returns (policy_target,
    c_visit, c_scale)."""
    name, c_visit, c_scale = check_policy_target(policy_target, policy_c_visit, policy_c_scale)
    if name == "completed_q" and not record_history:
        raise ValueError("policy_target='completed_q' needs record_history: the recorded rows are a column of the history")
    return name, c_visit, c_scale


def check_target_options(temperature_plies, record_search_value=False, record_history=True):
    """Validate the self-play target options (include/aqgnn.h, "self-play targets"): temperature_plies an integer >= 0 (0 = off);
    record_search_value needs the history it is a column of.  Returns (temperature_plies, record_search_value)."""
    if isinstance(temperature_plies, bool) or int(temperature_plies) != temperature_plies or not 0 <= int(temperature_plies) < 2 ** 31:
        raise ValueError(f"temperature_plies must be an integer >= 0, not {temperature_plies!r}")
    if record_search_value and not record_history:
        raise ValueError("record_search_value needs record_history: the search value is a column of the history")
    return int(temperature_plies), bool(record_search_value)


def check_temperature(temperature, sims, keep_visits=None):
    """Validate the sampling temperature as the library does (include/aqgnn.h, `temperature`), on the f32 value its struct holds:
    finite and >= 0 (0 = the first maximum); when > 0, log2(sims + keep_visits) / temperature <= 1016, so that every term
    n ** (1 / temperature) of boltzman is below 2**1016 and the sum of at most MAX_LEGAL < 2**8 of them is finite.  The reference raises
    for a negative one (ZeroDivisionError for 0 ** negative) and for a too small one (OverflowError); the kernel would form inf / inf
    and play child 0 without a word.
    keep_visits: check_tree_reuse's (None = tree reuse off).  Returns the temperature as a float."""
    if isinstance(temperature, (bool, str)) or not isinstance(temperature, (int, float, np.integer, np.floating)):
        raise ValueError(f"temperature must be a finite number >= 0, not {temperature!r}")
    with np.errstate(over="ignore"):
        t = float(np.float32(temperature))
    if not (t >= 0.0 and t != float("inf")):                     # NaN fails the first
        raise ValueError(f"temperature must be a finite number >= 0 as a float32, not {temperature!r}")
    visits = int(sims) + int(keep_visits or 0)
    if t > 0.0 and visits > 0 and not np.log2(float(visits)) / t <= 1016.0:
        raise ValueError(f"temperature {temperature!r} is too small for {visits} visits: log2(sims + keep_visits) / temperature must be "
                         f"<= 1016 (n ** (1 / temperature) overflows)")
    return t


def check_value_lambda(lam):
    """Validate the lambda of the lambda-return value targets as the library does (include/aqgnn.h, "lambda-return value targets"), on
    the f32 value the kernel is given: a number in [0, 1], not NaN (ValueError otherwise).  Returns it as a float."""
    if isinstance(lam, (bool, str)) or not isinstance(lam, (int, float, np.integer, np.floating)):
        raise ValueError(f"value_lambda must be a number in [0, 1], not {lam!r}")
    value = float(np.float32(lam))
    if not 0.0 <= value <= 1.0:                                  # NaN fails both
        raise ValueError(f"value_lambda must be in [0, 1] as a float32, not {lam!r}")
    return value


def check_tree_reuse(tree_reuse, tree_reuse_visits, sims, evaluator="gnn"):
    """Validate the tree-reuse options as the library does (include/aqgnn.h, "tree reuse").  Returns keep_visits, or None when the
    option is off.  tree_reuse_visits None = `sims`; 0 is legal: on, never keeps."""
    if not tree_reuse:
        if tree_reuse_visits is not None:
            raise ValueError("tree_reuse_visits needs tree_reuse=True")
        return None
    if evaluator == "external":
        raise ValueError("tree_reuse is not offered with evaluator='external': its host loop has no keep step")
    keep = sims if tree_reuse_visits is None else tree_reuse_visits
    if isinstance(keep, bool) or int(keep) != keep or int(keep) < 0:
        raise ValueError(f"tree_reuse_visits must be an integer >= 0, not {tree_reuse_visits!r}")
    keep = int(keep)
    if keep + int(sims) > 32767:
        raise ValueError("tree_reuse_visits + sims must be <= 32767: the visit row is read out as int16")
    if 1 + (keep + int(sims)) * _lib.MAX_LEGAL >= 1 << 24:
        raise ValueError("tree_reuse_visits + sims is too large: the tree pool must stay below 2**24 records")
    return keep


def check_resign(resign_threshold, resign_min_ply=0, resign_disable_fraction=0.1, record_history=True):
    """Validate the resignation options as the library does (include/aqgnn.h, "resignation"), on the values its struct holds.
    Returns (threshold, min_ply, disable_fraction), or None when the option is off (resign_threshold None).  A threshold of 1.0 is
    legal: on, never resigns -- the statistics are still kept."""
    if resign_threshold is None:
        return None
    if isinstance(resign_threshold, (bool, str)):
        raise ValueError(f"resign_threshold must be a number in (0, 1], not {resign_threshold!r}")
    thr = float(np.float32(resign_threshold))
    if not 0.0 < thr <= 1.0:
        raise ValueError(f"resign_threshold must be in (0, 1] as a float32, not {resign_threshold!r}")
    if isinstance(resign_min_ply, bool) or int(resign_min_ply) != resign_min_ply or not 0 <= int(resign_min_ply) < 2 ** 31:
        raise ValueError(f"resign_min_ply must be an integer >= 0, not {resign_min_ply!r}")
    frac = float(resign_disable_fraction)
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"resign_disable_fraction must be in [0, 1], not {resign_disable_fraction!r}")
    if not record_history:
        raise ValueError("resignation needs record_history: a resigned game ends in a history row")
    return thr, int(resign_min_ply), frac


def check_gumbel(gumbel_considered=0, gumbel_scale=1.0, sims=2, root_noise_eps=0.0, tree_reuse=False, resign_threshold=None,
                 temperature_plies=0, evaluator="gnn"):
    """Validate the Gumbel root search as the library does (include/aqgnn.h, "Gumbel root search"), in the library's order: sims >= 2;
    gumbel_considered in 1..64; gumbel_scale finite and >= 0; then not with root noise, tree reuse, resignation, temperature_plies > 0
    or evaluator='external'.  Returns (considered, scale), or None when the option is off (gumbel_considered 0)."""
    if isinstance(gumbel_considered, bool) or not isinstance(gumbel_considered, (int, np.integer)):
        raise ValueError(f"gumbel_considered must be an integer in 0..64 (0 = off), not {gumbel_considered!r}")
    considered = int(gumbel_considered)
    if considered == 0:
        return None
    if int(sims) < 2:
        raise ValueError("gumbel_considered needs sims >= 2: simulation 0 evaluates the root, the root is selected from sims - 1 times")
    if not 1 <= considered <= 64:
        raise ValueError(f"gumbel_considered must be in 1..64 (0 = off), not {gumbel_considered!r}")
    if isinstance(gumbel_scale, (bool, str)) or not isinstance(gumbel_scale, (int, float, np.integer, np.floating)):
        raise ValueError(f"gumbel_scale must be a finite number >= 0, not {gumbel_scale!r}")
    scale = float(gumbel_scale)
    if not (scale >= 0.0 and scale != float("inf")):             # NaN fails the first
        raise ValueError(f"gumbel_scale must be a finite number >= 0, not {gumbel_scale!r}")
    if root_noise_eps:
        raise ValueError("gumbel_considered is not offered with root noise: the Gumbel variates are the root's exploration")
    if tree_reuse:
        raise ValueError("gumbel_considered is not offered with tree_reuse: a kept root's children hold no Gumbel logits")
    if resign_threshold is not None:
        raise ValueError("gumbel_considered is not offered with resignation")
    if temperature_plies:
        raise ValueError("gumbel_considered is not offered with temperature_plies: the move is the survivor, no temperature is read")
    if evaluator == "external":
        raise ValueError("gumbel_considered is not offered with evaluator='external': its host loop has no root launch")
    return considered, scale


def default_gumbel_seed(seed):
    """The Gumbel seed of an engine that was given none: `seed` through the mixer (see default_root_noise_seed)."""
    return mix64((int(seed) & MASK64) ^ 0x47554D42454C5F5F)


def default_root_noise_seed(seed):
    """The noise seed of an engine that was given none: `seed` through the mixer.  NOT a linear map: the generator's stream of game
    k is keyed by mix(noise_seed + GOLDEN * (k + 1)), so noise seeds that differ by a multiple of GOLDEN -- what any affine map of
    consecutive engine seeds onto them risks -- would hand game k of one engine the stream of another game of the next."""
    return mix64((int(seed) & MASK64) ^ 0x524F4F544E4F4953)


def default_resign_seed(seed):
    """The resignation seed of an engine that was given none: `seed` through the mixer (see default_root_noise_seed)."""
    return mix64((int(seed) & MASK64) ^ 0x52455349474E4544)


def set_noise_seeds(seed, root_noise_seed, sizes, quotas):
    """The noise seeds of MultiSetSelfPlay's sets (slots `sizes`, games `quotas`).  The sets' games are numbered through -- set i's
    game k is game first_i + k of the whole engine -- and the numbering rides in the seed: the stream of game k under
    base + GOLDEN * first is the stream of game first + k under base.  Every set has a seed of its own and no two games share one."""
    base = default_root_noise_seed(seed) if root_noise_seed is None else int(root_noise_seed) & MASK64
    firsts = [sum(max(q, g) for q, g in zip(quotas[:i], sizes[:i])) for i in range(len(sizes))]
    return [(base + GOLDEN * f) & MASK64 for f in firsts]


# ------------------------------------------------------------------ start positions (include/aqgnn.h, "start positions")
def _start_rows(start_states):
    """The table as a uint8 [S, 72] numpy array or torch tensor, S >= 1 (ValueError otherwise)."""
    import torch
    rows = start_states if isinstance(start_states, torch.Tensor) else np.asarray(start_states)
    if str(rows.dtype) not in ("uint8", "torch.uint8") or len(rows.shape) != 2 or rows.shape[1] != 72 or rows.shape[0] < 1:
        raise ValueError("start_states must be a uint8 [S, 72] tensor or array of state72 records, S >= 1")
    return rows


def check_start_index(start_index, rows, quota):
    """start_index as an int32 numpy array [quota] with every entry in [0, rows) (ValueError otherwise); None stays None."""
    if start_index is None:
        return None
    import torch
    index = start_index.cpu().numpy() if isinstance(start_index, torch.Tensor) else np.asarray(start_index)
    if index.ndim != 1 or index.dtype.kind not in "iu":
        raise ValueError("start_index must be a one-dimensional integer array")
    if index.shape[0] != quota:
        raise ValueError(f"start_index has {index.shape[0]} entries for {quota} games: one row number per game of the quota")
    bad = np.flatnonzero((index < 0) | (index >= rows))
    if bad.size:
        raise ValueError(f"start_index[{int(bad[0])}] = {int(index[bad[0]])} is outside the {rows} rows of start_states")
    return index.astype(np.int32)


def check_start_table(start_states, start_index, board_size, quota, device):
    """None without a table, else (rows u8 [S,72], index i32 [quota] or None) on `device`, checked: the rows by the device checker
    (one device-to-host read), the index for length and range.  ValueError names the first bad row and its flags."""
    import torch
    if start_states is None:
        if start_index is not None:
            raise ValueError("start_index needs start_states")
        return None
    rows = _start_rows(start_states)
    index = check_start_index(start_index, rows.shape[0], quota)
    from .game_logic import check_states_batch
    if not isinstance(rows, torch.Tensor):
        rows = torch.from_numpy(np.array(rows, dtype=np.uint8))       # (a copy: the caller's array may be read-only)
    rows = rows.to(device).contiguous().clone()                        # the engine's own copy
    flags = check_states_batch(rows, board_size).cpu().numpy()
    bad = np.flatnonzero(flags)
    if bad.size:
        raise ValueError(f"start_states row {int(bad[0])} cannot start a game: checker flags {int(flags[bad[0]])} "
                         f"({bad.size} of {rows.shape[0]} rows are flagged; game_logic.check_state_reference names the bits)")
    return rows, None if index is None else torch.from_numpy(index).to(device)


def set_start_indices(start_states, start_index, set_quotas):
    """The start indices of MultiSetSelfPlay's sets (games `set_quotas`): the sets' games are numbered through in history_tensors()'
    order, and set i is handed the slice of its block -- of the caller's index, or of the default k % S written out."""
    if start_states is None:
        if start_index is not None:
            raise ValueError("start_index needs start_states")
        return [None] * len(set_quotas)
    rows = _start_rows(start_states).shape[0]
    total = int(sum(set_quotas))
    index = check_start_index(start_index, rows, total)
    if index is None:
        index = (np.arange(total) % rows).astype(np.int32)
    firsts = np.concatenate([[0], np.cumsum(set_quotas)]).astype(int)
    return [index[firsts[i]:firsts[i + 1]] for i in range(len(set_quotas))]


# Matches, evaluation paths and single searches add no noise (they measure strength), search from a fresh tree every move (two
# alternating searchers would need a two-ply descent into per-model trees) and play every game to its rule end.
_NOISE, _REUSE, _RESIGN = "never adds root exploration noise", "never keeps a subtree between moves", "never resigns a game"
_GUMBEL = "never samples its root's actions (the Gumbel root search)"
SELF_PLAY_ONLY = {"root_noise_eps": _NOISE, "root_noise_alpha": _NOISE, "root_noise_seed": _NOISE,
                  "tree_reuse": _REUSE, "tree_reuse_visits": _REUSE,
                  "resign_threshold": _RESIGN, "resign_min_ply": _RESIGN, "resign_disable_fraction": _RESIGN, "resign_seed": _RESIGN,
                  "gumbel_considered": _GUMBEL, "gumbel_scale": _GUMBEL, "gumbel_seed": _GUMBEL}


def refuse_self_play_options(what, **options):
    """`what` is no self-play: a self-play option that is given (not None -- False and 0.0 are given) is a mistake, not something
    to drop silently.  The groups are refused in the table's order, each with its own sentence."""
    for sentence in dict.fromkeys(SELF_PLAY_ONLY.values()):
        bad = sorted(k for k, v in options.items() if v is not None and SELF_PLAY_ONLY[k] == sentence)
        if bad:
            raise ValueError(f"{what} {sentence}: {', '.join(bad)} is a self-play option")
