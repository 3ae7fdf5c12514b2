#!/usr/bin/env python3
"""Generate tests/golden/cnn_train_5x5.npz by IMPORTING the reference's own CNNNetwork (read-only, /root/reference).

Generation-time tooling only, like tools/gen_golden_cnn.py (gen_golden's stub recipe): runs where the reference exists, never on the
GPU box.  It builds the reference's CNNNetwork at 16 filters x 2 residual blocks on 5x5, gives every BatchNorm non-trivial running
statistics, gamma and beta, and takes ONE step of its train_network.py:84-92 in fp32 on 40 positions of random legal play with
random targets: the module in train mode, CrossEntropyLoss on the softmaxed policy + MSELoss on the value, backward,
torch.optim.Adam(lr=0.001).  Recorded, data only: the parameters and buffers before the step (by state_dict key), the positions as
state72 records, the targets, both losses, every parameter's .grad, the running statistics after the forward and the parameters
after the Adam step.

Usage:  python tools/gen_golden_cnn_train.py
"""
import argparse
import os
import sys

sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

FILTERS, BLOCKS, STATES, BOARD = 16, 2, 40, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(gen_golden.REPO, "tests", "golden"))
    args = ap.parse_args()
    out_dir = os.path.abspath(args.out)
    game_logic, _, _, cnn = gen_golden.import_reference(BOARD)
    import torch

    torch.manual_seed(4321)
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
                mod.num_batches_tracked.fill_(3)
    fixture = {"param." + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}

    rng = np.random.RandomState(11)
    states = []
    s = game_logic.State()
    while len(states) < STATES:
        states.append(s)
        la = list(s.legal_actions())
        s = s.next(la[rng.randint(len(la))])
        if s.is_done():
            s = game_logic.State()
    A = BOARD ** 2 + 2 * (BOARD - 1) ** 2
    pi = rng.rand(STATES, A) * (rng.rand(STATES, A) < 0.2)
    pi[:, 0] += 1e-3
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    z = rng.choice([-1.0, 0.0, 1.0], STATES).astype(np.float32)

    # train_network.py:84-92 on one batch
    model.train()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.001)
    x = torch.from_numpy(model.preprocess_input([st.to_array() for st in states]))
    optimizer.zero_grad()
    policy, value = model(x)
    policy_loss = torch.nn.CrossEntropyLoss()(policy, torch.from_numpy(pi))
    value_loss = torch.nn.MSELoss()(value.squeeze(), torch.from_numpy(z))
    (policy_loss + value_loss).backward()
    fixture.update({"grad." + k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()})
    fixture.update({"stats." + k: v.detach().numpy().copy() for k, v in model.state_dict().items()
                    if k.endswith(("running_mean", "running_var", "num_batches_tracked"))})
    optimizer.step()
    fixture.update({"after." + k: p.detach().numpy().copy() for k, p in model.named_parameters()})
    fixture.update(states=np.stack([gen_golden.rec_of(st) for st in states]), pi=pi, z=z,
                   policy=policy.detach().numpy().astype(np.float32), value=value.detach().numpy()[:, 0].astype(np.float32),
                   losses=np.asarray([policy_loss.item(), value_loss.item()], dtype=np.float32),
                   shape=np.asarray([FILTERS, BLOCKS, BOARD], dtype=np.int64))
    path = os.path.join(out_dir, f"cnn_train_{BOARD}x{BOARD}.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
