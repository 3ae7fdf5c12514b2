"""Shared by the start-position tests (tests/test_start_positions_cpu.py, tests/test_state_check.py, tests/test_start_positions.py):
crafted records for the checker, start tables, and host statements of what an engine with a table does.  No torch.

crafted_records(N): (name, record, flags) -- the flags are stated here by hand, from the bit table of include/aqgnn.h ("start
positions"); the numpy statement game_logic.check_state_reference is held to them on the CPU, and the kernel to the statement.
refill_reference(G, Q, end_sets, rows, index): tests/_move_cycle.refill_reference with the record every refilled slot must hold.
play_from(...): oracle.mcts.play restated from a given state, on pv_mcts_policy, choice_index and first_player_value."""
import numpy as np

from tests import _move_cycle as MC

BOARD, WALLS, WALL_COUNT, SAME_SQUARE, OVER, ODD_PLY, NO_PATH = 1, 2, 4, 8, 16, 32, 64


def params(N):
    from oracle import quoridor as oq
    return oq.BOARDS[N]          # (walls per side, plies_for_draw)


def set_plies(rec, plies):
    rec[68], rec[69] = plies & 0xFF, plies >> 8
    return rec


def fenced_record(N):
    """The mover shut into the bottom row: horizontal walls over columns 0 .. N-2 of the row above it, a vertical wall beside the
    last column.  S / 2 + 1 walls, none overlapping, the accounting right."""
    from oracle import quoridor as oq
    rec = oq.init_record(N)
    S, walls = N - 1, params(N)[0]
    for sy in range(0, S, 2):
        rec[4 + (N - 2) * S + sy] = 1
    rec[4 + (N - 2) * S + S - 1] = 2
    placed = S // 2 + 1
    left = 2 * walls - placed
    rec[1], rec[3] = min(left, walls), left - min(left, walls)
    return rec


def crafted_records(N):
    """Each bit alone, pairs of bits, pawn cells of 255 and wall bytes of 255, and clean records beside the edges of each rule."""
    from oracle import quoridor as oq
    V, S = N * N, N - 1
    walls, draw = params(N)
    opening = oq.init_record(N)
    centre = (V - 1) // 2
    out = []

    def add(name, flags, **bytes_):
        rec = bytes_.pop("base", opening).copy()
        for k, v in bytes_.items():
            rec[int(k[1:])] = v
        out.append((name, rec, flags))
        return rec

    add("opening", 0)
    add("spare_bytes_ignored", 0, b71=0xFF, **({f"b{4 + S * S}": 0xFF} if S * S < 64 else {}))
    # --- bit 1
    add("byte70", BOARD, b70=N + 2)
    add("ppos_255", BOARD, b0=255)
    add("epos_255", BOARD, b2=255)
    add("ppos_V", BOARD, b0=V)
    # --- bit 2 (a byte above 2 is no wall: the accounting holds)
    add("wall_255_first", WALLS, b4=255)
    add("wall_3_last", WALLS, **{f"b{4 + S * S - 1}": 3})
    two = dict(b1=walls - 1, b3=walls - 1)
    add("h_beside_h", WALLS, b4=1, b5=1, **two)
    add("v_above_v", WALLS, b4=2, **{f"b{4 + S}": 2}, **two)
    rec = add("h_row_end_and_next_row_start", 0, **{f"b{4 + S - 1}": 1, f"b{4 + S}": 1}, **two)
    assert rec[4 + S - 1] == 1 and rec[4 + S] == 1
    if N > 3:                                                      # (on 3x3 these two shut the enemy in)
        add("h_beside_v", 0, b4=1, b5=2, **two)
    # --- bit 4
    add("walls_left_above", WALL_COUNT, b1=walls + 1)
    add("walls_left_short", WALL_COUNT, b1=walls - 1)
    add("placed_not_counted", WALL_COUNT, b4=1)
    # --- bit 8
    add("same_square", SAME_SQUARE, b0=centre, b2=centre)
    # --- bit 16
    add("enemy_on_goal", OVER, b2=0)
    add("mover_on_goal", OVER, b0=0)
    set_plies(add("drawn", OVER), draw)
    set_plies(add("two_before_draw", 0), draw - 2)
    # --- bit 32
    set_plies(add("odd_ply", ODD_PLY), 1)
    set_plies(add("ply_258_high_byte", OVER), 258)
    # --- bit 64
    fenced = fenced_record(N)
    add("fenced", NO_PATH, base=fenced)
    if N == 3:      # a position of a real game: the enemy pawn stands in the mover's only corridor, the walls alone leave a path
        rec = set_plies(add("pawn_in_corridor", 0, b0=8, b1=0, b2=6, b3=0, b5=2, b6=1), 8)
        assert rec[4:8].tolist() == [0, 2, 1, 0]
    # --- pairs
    set_plies(add("ppos_255+odd", BOARD | ODD_PLY, b0=255), 3)
    add("ppos_255+enemy_on_goal", BOARD | OVER, b0=255, b2=0)
    add("wall_255+walls_left", WALLS | WALL_COUNT, b4=255, b1=walls + 1)
    add("wall_255+same_square", WALLS | SAME_SQUARE, b5=255, b0=centre, b2=centre)
    set_plies(add("walls_left+drawn", WALL_COUNT | OVER, b3=walls + 1), draw)
    set_plies(add("same_square+odd", SAME_SQUARE | ODD_PLY, b0=centre, b2=centre), 1)
    add("same_square+over", SAME_SQUARE | OVER, b0=N // 2, b2=V - 1 - N // 2)
    set_plies(add("over+odd", OVER | ODD_PLY, b2=N - 1), draw + 1)
    set_plies(add("fenced+odd", NO_PATH | ODD_PLY, base=fenced), 5)
    add("fenced+walls_left", NO_PATH | WALL_COUNT, base=fenced, b1=int(fenced[1]) + 1)
    add("byte70+wall_255", BOARD | WALLS, b70=0, b4=255)
    return [(name, rec, flags) for name, rec, flags in out]


def garbage_records(N, n, seed):
    """Records of random bytes, and crafted records with a few random bytes thrown in: what the checker is there to meet."""
    rng = np.random.RandomState(seed)
    recs = rng.randint(0, 256, (n, 72)).astype(np.uint8)
    crafted = [r for _, r, _ in crafted_records(N)]
    for i in range(n // 2):
        rec = crafted[i % len(crafted)].copy()
        at = rng.randint(0, 72, 3)
        rec[at] = rng.randint(0, 256, 3)
        recs[i] = rec
    recs[n // 4:n // 2, 70] = N
    return recs


def walk_positions(N, games, seed):
    """Every position of `games` seeded random walks from the opening to the end, the ended one left out: records in walk order."""
    from oracle import quoridor as oq
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(games):
        state = oq.State(N=N)
        while not state.is_done():
            out.append(state.rec.copy())
            legal = state.legal_actions()
            state = state.next(int(legal[rng.randint(len(legal))]))
    return np.stack(out)


def start_rows(N, plies, count, seed):
    """`count` distinct records `plies` plies deep (even), none of them over: seeded walks from the opening."""
    from oracle import quoridor as oq
    assert plies % 2 == 0
    rng = np.random.RandomState(seed)
    rows, seen = [], set()
    for _ in range(10000):
        if len(rows) == count:
            break
        state = oq.State(N=N)
        for _ in range(plies):
            legal = state.legal_actions()
            state = state.next(int(legal[rng.randint(len(legal))]))
            if state.is_done():
                break
        if not state.is_done() and state.plies_played == plies and state.rec.tobytes() not in seen:
            seen.add(state.rec.tobytes())
            rows.append(state.rec.copy())
    assert len(rows) == count
    return np.stack(rows)


def row_of_game(k, rows, index):
    return int(index[k]) if index is not None else k % len(rows)


def refill_reference(G, Q, end_sets, rows, index=None):
    """tests/_move_cycle.refill_reference, each snapshot with `start72`: for every slot that was refilled in that move the record its
    new game starts from -- row index[k], or k % S, of the table for game k -- and None elsewhere."""
    snaps = MC.refill_reference(G, Q, end_sets)
    for snap in snaps:
        snap["start72"] = [rows[row_of_game(int(snap["slot_game"][s]), rows, index)] if snap["refilled"][s] else None for s in range(G)]
    return snaps


def visit_counts(scores, total):
    """The integer visit counts behind pv_mcts_policy's T = 1 scores n / sum(n), sum(n) = total."""
    x = np.asarray(scores, dtype=np.float64) * total
    n = np.rint(x)
    assert np.abs(x - n).max() < 1e-6 and int(n.sum()) == total
    return n.astype(np.int64)


def play_from(model, rec, sims, uniforms, temperature=1.0, temperature_plies=0):
    """oracle.mcts.play (self_play.py:40-68) from the state of `rec` instead of the opening: per ply pv_mcts_policy at T = 1 for the
    recorded visit counts, the move by choice_index over the scores at `temperature` (the first maximum at T = 0, or from the
    game's ply temperature_plies on), z from first_player_value.  `uniforms`: one per ply of THIS game.  Returns dict(states [P,72],
    visits i16 [P,A], actions [P], z i8 [P], result, plies)."""
    from oracle import mcts as om, quoridor as oq
    state = oq.State(rec)
    N = state.N
    A = N * N + 2 * (N - 1) ** 2
    states, visits, actions = [], [], []
    while not state.is_done():
        ply = len(states)
        scores = om.pv_mcts_policy(model, state, 1.0, sims)
        legal = state.legal_actions()
        n = visit_counts(scores, sims - 1)
        row = np.zeros(A, dtype=np.int16)
        row[legal] = n
        late = temperature_plies > 0 and ply >= temperature_plies
        if temperature == 0 or late:
            idx = int(np.argmax(n))
        else:
            assert temperature == 1.0
            idx = om.choice_index(scores, float(uniforms[ply]))
        states.append(state.rec.copy())
        visits.append(row)
        actions.append(int(legal[idx]))
        state = state.next(legal[idx])
    result = om.first_player_value(state)
    z = np.asarray([result * (1 if i % 2 == 0 else -1) for i in range(len(states))], dtype=np.int8)
    return dict(states=np.stack(states), visits=np.stack(visits), actions=np.asarray(actions), z=z, result=result, plies=len(states),
                last=state.rec.copy())


def match_points_from(models, rec, first, sims):
    """One game of a paired match at T = 0 from `rec` (even ply): side `first` moves first, the mover's own model searches from a
    fresh tree (oracle.mcts.evaluate_play from a given state).  Returns side 0's points."""
    from oracle import mcts as om, quoridor as oq
    state = oq.State(rec)
    ply = 0
    while not state.is_done():
        model = models[first if ply % 2 == 0 else 1 - first]
        scores = om.pv_mcts_policy(model, state, 0, sims)
        legal = state.legal_actions()
        state = state.next(legal[int(np.argmax(scores))])
        ply += 1
    # the first mover of THIS game is the side to move at `rec`, an even-ply record: first_player_point is its point
    point = om.first_player_point(state)
    return point if first == 0 else 1.0 - point
