"""Held-out validation (csrc/row_metrics.hip; the definition is in include/aqgnn.h, "row metrics"): what a network scores on rows no
update trains on, per ply bucket, and the split of rows by position that keeps such rows apart.

  row_metrics(model, states72, pi, z, index)     the per-bucket table of a network on rows: true cross-entropy, target entropy, their
                                                 difference (KL), the trainers' policy loss, value MSE, top-1 and value-sign agreement
  holdout_split(states72, index, share, seed)    (train_index, holdout_index): a position falls on one side under a seed wherever and
                                                 however often it occurs
  python -m alphaquoridorgnn_amd.validation NET.pth FILE.history [...]      the table of a saved network on the rows of the files

replay_reference.row_metrics_reference, row_metrics_reduce_reference and holdout_reference are the launches in numpy; rows in host
memory (a ReplayWindow on the CPU) go through them."""
import numpy as np
import torch

from . import _lib
from .constants import BOARD_SIZE, check_board_size, num_actions
from .replay_merge import check_gpu_rows
from .replay_reference import (ROW_METRICS_MAX_ROWS, check_holdout_options, check_row_metrics_options, holdout_split_reference,
                               row_metrics_reduce_reference, row_metrics_reference)

COLUMNS = ("ce", "ent", "lp", "se")                 # of sums
COUNTS = ("rows", "hits", "signs", "agree")         # of counts


class Metrics:
    """The result of row_metrics: sums float64 [buckets+1,4] = per bucket the sums of {ce, ent, lp, se}, counts int64 [buckets+1,4] =
    per bucket {rows, hits, signs counted, signs agreeing} (numpy arrays; row `buckets` holds the rejected rows, with zero sums), and
    the totals over the accepted rows: policy_ce, target_entropy, kl = policy_ce - target_entropy, policy_loss (the mean of lp: the
    trainers' policy loss), value_mse, top1, value_sign (of the rows with z != 0).  A total over no row is nan."""

    def __init__(self, sums, counts, bucket_plies, buckets):
        self.sums, self.counts = np.asarray(sums, dtype=np.float64), np.asarray(counts, dtype=np.int64)
        self.bucket_plies, self.buckets = int(bucket_plies), int(buckets)
        if self.sums.shape != (self.buckets + 1, 4) or self.counts.shape != (self.buckets + 1, 4):
            raise ValueError("Metrics: sums and counts are [buckets + 1, 4] tables")
        self.rejected = int(self.counts[self.buckets, 0])
        self.rows = int(self.counts[:self.buckets, 0].sum())
        total = [float(x) for x in self.sums[:self.buckets].sum(axis=0)]
        hits, signs, agree = (int(x) for x in self.counts[:self.buckets, 1:].sum(axis=0))
        self.policy_ce, self.target_entropy, self.policy_loss, self.value_mse = (_ratio(x, self.rows) for x in total)
        self.kl = self.policy_ce - self.target_entropy
        self.top1, self.value_sign = _ratio(hits, self.rows), _ratio(agree, signs)

    def bucket(self, b):
        """The totals of bucket b alone, as a dict (the keys of totals() and `rows`)."""
        rows, hits, signs, agree = (int(x) for x in self.counts[b])
        ce, ent, lp, se = (_ratio(float(x), rows) for x in self.sums[b])
        return dict(rows=rows, policy_ce=ce, target_entropy=ent, kl=ce - ent, policy_loss=lp, value_mse=se, top1=_ratio(hits, rows),
                    value_sign=_ratio(agree, signs))

    def totals(self):
        return dict(rows=self.rows, rejected=self.rejected, policy_ce=self.policy_ce, target_entropy=self.target_entropy, kl=self.kl,
                    policy_loss=self.policy_loss, value_mse=self.value_mse, top1=self.top1, value_sign=self.value_sign)

    def as_dict(self):
        """Everything, as plain Python values (what the loop's log holds)."""
        return dict(totals=self.totals(), bucket_plies=self.bucket_plies, buckets=self.buckets, sums=self.sums.tolist(),
                    counts=self.counts.tolist())

    def table(self):
        """The per-bucket lines: one per bucket that holds a row, then the totals, then the rejected rows when there are any."""
        head = f"{'plies':>11} {'rows':>8} {'CE':>8} {'H(t)':>8} {'KL':>8} {'P loss':>8} {'V MSE':>8} {'top-1':>6} {'sign':>6}"
        lines = [head]
        for b in range(self.buckets):
            if self.counts[b, 0] == 0:
                continue
            lo = b * self.bucket_plies
            span = f"{lo}+" if b == self.buckets - 1 else f"{lo}-{lo + self.bucket_plies - 1}"
            lines.append(_table_line(span, self.bucket(b)))
        lines.append(_table_line("all", self.totals()))
        if self.rejected:
            lines.append(f"{'rejected':>11} {self.rejected:>8}")
        return "\n".join(lines)


def _ratio(x, n):
    return float(x) / n if n else float("nan")


def _table_line(name, d):
    return (f"{name:>11} {d['rows']:>8} {d['policy_ce']:>8.4f} {d['target_entropy']:>8.4f} {d['kl']:>8.4f} {d['policy_loss']:>8.4f} "
            f"{d['value_mse']:>8.4f} {d['top1']:>6.3f} {d['value_sign']:>6.3f}")


def _checked_index(what, index, dev):
    if index is None:
        return None
    if index.dtype != torch.int64 or index.dim() != 1 or index.device != dev:
        raise ValueError(f"{what}: index must be an int64 [m] tensor on the rows' device")
    return index.contiguous()


def row_metrics(model, states72, pi, z, index=None, *, bucket_plies=8, buckets=16, chunk_rows=16384):
    """The metrics of `model` on the rows index[0..m) (int64, on the tensors' device; None: all rows) of states72 uint8 [rows,72], pi
    float32 [rows,A] and z float32 [rows]: a Metrics object.

    On the GPU: model.forward_states runs over the records in chunks of at most chunk_rows rows, in eval mode (BatchNorm uses its
    running statistics: that is the network that plays), without autograd, with its fp16-range guard, and the module's mode is left
    as it was; one aqg_replay_row_metrics launch per chunk, one aqg_row_metrics_reduce, and one device-to-host read of its own
    (besides the forward's guard): the two small tables.  Rows in host memory take the same steps through the numpy statements, with
    the model's forward_states fed host tensors."""
    bucket_plies, buckets = check_row_metrics_options(bucket_plies, buckets)
    if int(chunk_rows) < 1:
        raise ValueError("row_metrics: chunk_rows must be >= 1")
    board_size, A = int(model.board_size), int(model.policy_output_size)
    check_board_size(board_size, "row_metrics")
    if A != num_actions(board_size):            # a policy head that is not the board's
        raise ValueError("row_metrics: unsupported board_size (odd 3..9)")
    rows = int(states72.shape[0]) if states72.dim() == 2 else -1
    dev = states72.device
    specs = ((states72, "states72", torch.uint8, (rows, 72)), (pi, "pi", torch.float32, (rows, A)), (z, "z", torch.float32, (rows,)))
    if dev.type == "cpu":
        for x, name, dtype, shape in specs:
            if x.dtype != dtype or tuple(x.shape) != shape or x.device != dev:
                raise ValueError(f"row_metrics: {name} must be a {dtype} {list(shape)} tensor in host memory ({board_size}x{board_size} board)")
    else:
        check_gpu_rows("row_metrics", board_size, specs)
    states72, pi, z = states72.contiguous(), pi.contiguous(), z.contiguous()
    index = _checked_index("row_metrics", index, dev)
    m = rows if index is None else int(index.numel())
    if m > ROW_METRICS_MAX_ROWS:
        raise ValueError(f"row_metrics: {m} rows; 2^24 at most")
    chunk = int(chunk_rows)
    was_training = bool(getattr(model, "training", False))

    def outputs(off, n):
        records = states72[off:off + n] if index is None else states72.index_select(0, index[off:off + n])
        out = model.forward_states(records.contiguous())
        return out[0].contiguous(), out[1].reshape(n).contiguous()

    if dev.type == "cpu":
        model.eval()
        try:
            with torch.no_grad():
                parts = [outputs(off, min(chunk, m - off)) for off in range(0, m, chunk)]
        finally:
            model.train(was_training)
        net_policy = np.concatenate([x.numpy() for x, _ in parts]) if parts else np.zeros((0, A), np.float32)
        net_value = np.concatenate([y.numpy() for _, y in parts]) if parts else np.zeros((0,), np.float32)
        vals, tag = row_metrics_reference(states72.numpy(), pi.numpy(), z.numpy(), net_policy.astype(np.float32, copy=False),
                                          net_value.astype(np.float32, copy=False), None if index is None else index.numpy(),
                                          bucket_plies, buckets)
        return Metrics(*row_metrics_reduce_reference(vals, tag, buckets), bucket_plies, buckets)
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        vals = torch.empty((m, 4), dtype=torch.float64, device=dev)
        tag = torch.empty((m,), dtype=torch.int32, device=dev)
        tables = torch.empty((2, buckets + 1, 4), dtype=torch.int64, device=dev)       # sums (as 8-byte words) and counts: one read
        model.eval()
        try:
            with torch.no_grad():
                for off in range(0, m, chunk):
                    n = min(chunk, m - off)
                    net_policy, net_value = outputs(off, n)
                    _lib.check(lib.aqg_replay_row_metrics(board_size, A, _lib.ptr(net_policy), _lib.ptr(net_value), _lib.ptr(states72),
                                                          _lib.ptr(pi), _lib.ptr(z), _lib.ptr(index), rows, m, off, n, bucket_plies,
                                                          buckets, _lib.ptr(vals), _lib.ptr(tag), st), "aqg_replay_row_metrics")
        finally:
            model.train(was_training)
        words = int(lib.aqg_row_metrics_workspace_doubles(m, buckets))
        partial = torch.empty((words,), dtype=torch.float64, device=dev) if words else None
        _lib.check(lib.aqg_row_metrics_reduce(_lib.ptr(vals if m else None), _lib.ptr(tag if m else None), m, buckets, _lib.ptr(partial),
                                              _lib.ptr(tables[0]), _lib.ptr(tables[1]), st), "aqg_row_metrics_reduce")
        host = tables.cpu().numpy()                                     # the one read
    return Metrics(host[0].view(np.float64), host[1], bucket_plies, buckets)


def holdout_split(states72, index=None, share=0.1, seed=0, board_size=BOARD_SIZE):
    """(train_index, holdout_index) of the rows index[0..n) (int64, on the rows' device; None: all rows) of states72 uint8 [rows,72]:
    both int64 on the rows' device and in input order.  A row is held out iff counter_uniform(stream_key(seed, HOLDOUT_STREAM), its
    position key) < share -- a function of (seed, the record's key bytes) alone, so a position lands on one side in every update and
    every generation, merged or not, whatever its ply bytes hold.  On the GPU: aqg_replay_position_keys, aqg_replay_holdout_mask and
    two nonzeros; rows in host memory: the numpy statements."""
    check_board_size(board_size, "holdout_split")
    share, seed, _ = check_holdout_options(share, seed)
    if states72.dtype != torch.uint8 or states72.dim() != 2 or states72.shape[1] != 72:
        raise ValueError("holdout_split: states72 must be a uint8 [rows,72] tensor")
    dev = states72.device
    index = _checked_index("holdout_split", index, dev)
    rows = int(states72.shape[0])
    if dev.type == "cpu":
        if index is not None and index.numel() and (int(index.min()) < 0 or int(index.max()) >= rows):
            raise ValueError("holdout_split: index names a row the arrays do not have")
        train, held = holdout_split_reference(states72.numpy(), None if index is None else index.numpy(), share, seed)
        return torch.from_numpy(train), torch.from_numpy(held)
    _lib.require_gpu(dev)
    states72 = states72.contiguous()
    n = rows if index is None else int(index.numel())
    base = torch.arange(n, dtype=torch.int64, device=dev) if index is None else index
    if n == 0:
        return base.clone(), base.clone()
    if index is not None:
        lo, hi = torch.stack((index.min(), index.max())).tolist()
        if lo < 0 or hi >= rows:
            raise ValueError("holdout_split: index names a row the arrays do not have")
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        mask = torch.empty((n,), dtype=torch.uint8, device=dev)
        _lib.check(lib.aqg_replay_position_keys(_lib.ptr(states72), _lib.ptr(index), n, _lib.ptr(keys), st), "aqg_replay_position_keys")
        _lib.check(lib.aqg_replay_holdout_mask(_lib.ptr(keys), n, seed, share, _lib.ptr(mask), st), "aqg_replay_holdout_mask")
        return base[(mask == 0).nonzero().squeeze(1)], base[mask.nonzero().squeeze(1)]


def history_rows(paths, board_size, device):
    """The rows of .history files, in the order given, as (states72 uint8 [n,72], pi float32 [n,A], z float32 [n]) on `device`,
    converted as the trainers convert a file.  Every record carries ply 0."""
    import pickle
    from .pv_network_gnn import pack_states
    history = []
    for path in paths:
        with open(path, mode="rb") as f:
            history += list(pickle.load(f))
    A = num_actions(board_size)
    s, p, v = zip(*history) if history else ((), (), ())
    return (torch.from_numpy(pack_states(s, board_size)).to(device),
            torch.tensor(np.array(p, dtype=np.float64).reshape(len(history), A), dtype=torch.float32, device=device),
            torch.tensor(np.array(v, dtype=np.float64).reshape(len(history)), dtype=torch.float32, device=device))


def main(argv=None):
    """python -m alphaquoridorgnn_amd.validation NET.pth FILE.history [...]: the table of a saved network -- a GNN of any shape or the
    residual CNN -- on the rows of the files.  No training run is needed: it is how one measures an old checkpoint on new games.
    (Rows read from .history files carry ply 0: they all land in bucket 0.)"""
    import argparse
    from . import distributed as aqd
    from .pv_network_cnn import is_cnn_state_dict, load_network as load_cnn
    from .pv_network_gnn import load_network
    ap = argparse.ArgumentParser(prog="python -m alphaquoridorgnn_amd.validation", description=main.__doc__)
    ap.add_argument("network")
    ap.add_argument("history", nargs="+")
    ap.add_argument("--bucket-plies", type=int, default=8)
    ap.add_argument("--buckets", type=int, default=16)
    ap.add_argument("--chunk-rows", type=int, default=16384)
    args = ap.parse_args(argv)
    try:
        check_row_metrics_options(args.bucket_plies, args.buckets)
    except ValueError as err:
        ap.error(str(err))
    dev = aqd.device()
    cnn = is_cnn_state_dict(torch.load(args.network, map_location="cpu", weights_only=True))
    model = (load_cnn if cnn else load_network)(args.network, dev)
    states72, pi, z = history_rows(args.history, model.board_size, dev)
    result = row_metrics(model, states72, pi, z, bucket_plies=args.bucket_plies, buckets=args.buckets, chunk_rows=args.chunk_rows)
    print(f"{args.network}: {int(states72.shape[0])} rows of {len(args.history)} file(s)")
    print(result.table())
    return result


if __name__ == "__main__":
    main()
