#!/usr/bin/env python3
"""Generate tests/golden/cnn_{9x9,5x5}.npz by IMPORTING the reference's own CNNNetwork (read-only, /root/reference).

Generation-time tooling only, like tools/gen_golden.py (whose stub recipe it uses): runs where the reference exists, never on the
GPU box.  It builds the reference's CNNNetwork at a small shape (16 filters x 2 residual blocks), gives every BatchNorm non-trivial
running statistics, gamma and beta, and records on 40 positions of random legal play (reference rules) its fp32 eval-mode
policy and value.  The file is data only: the parameters by state_dict key, the positions as state72 records, the outputs.

Usage:  python tools/gen_golden_cnn.py --board 9
        python tools/gen_golden_cnn.py --board 5
"""
import argparse
import os
import sys

sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

FILTERS, BLOCKS, STATES = 16, 2, 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9, choices=(5, 9))
    ap.add_argument("--out", default=os.path.join(gen_golden.REPO, "tests", "golden"))
    args = ap.parse_args()
    out_dir = os.path.abspath(args.out)
    game_logic, _, _, cnn = gen_golden.import_reference(args.board)
    import torch

    torch.manual_seed(1234 + args.board)
    cnn.NUM_FILTERS, cnn.NUM_RESIDUAL_BLOCKS = FILTERS, BLOCKS      # the reference's constructor reads these module constants
    model = cnn.CNNNetwork()
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                n = mod.num_features
                mod.weight.copy_(torch.empty(n).uniform_(0.5, 1.5))
                mod.bias.copy_(torch.empty(n).uniform_(-0.2, 0.2))
                mod.running_mean.copy_(torch.empty(n).uniform_(-0.3, 0.3))
                mod.running_var.copy_(torch.empty(n).uniform_(0.5, 2.0))
                mod.num_batches_tracked.fill_(7)
    model.eval()

    rng = np.random.RandomState(args.board)
    states = []
    s = game_logic.State()
    while len(states) < STATES:
        states.append(s)
        la = list(s.legal_actions())
        s = s.next(la[rng.randint(len(la))])
        if s.is_done():
            s = game_logic.State()
    x = torch.from_numpy(model.preprocess_input([st.to_array() for st in states]))
    with torch.no_grad():
        policy, value = model(x)
    fixture = {"param." + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    fixture.update(states=np.stack([gen_golden.rec_of(st) for st in states]), policy=policy.numpy().astype(np.float32),
                   value=value.numpy()[:, 0].astype(np.float32), shape=np.asarray([FILTERS, BLOCKS, args.board], dtype=np.int64))
    path = os.path.join(out_dir, f"cnn_{args.board}x{args.board}.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
