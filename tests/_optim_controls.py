"""What the optimiser-control tests share (test_optim_controls_cpu.py, test_optim_controls.py): the torch side -- a shadow of the
parameters under torch.optim.Adam / AdamW and clip_grad_norm_ on the CPU --, the project's Adam bar, and the visibility guard that
keeps a passing comparison from being blind to the option under test.  No GPU, no library call."""
import numpy as np
import torch

LR = 2e-2                     # the three-step comparisons' learning rate (see assert_visible for why not 1e-3) ...
LRS = (1e-4, LR, LR)          # ... of steps 2 and 3; step 1 takes a small one (see assert_visible)
CLIP_FACTORS = (0.9, 0.1, 0.5)          # max_grad_norm of step i = CLIP_FACTORS[i] x that step's unclipped norm
DECAY = 1.0                   # the decay coefficient of the three-step comparisons (see assert_visible)
BAR_WELL = 1e-5               # the Adam bar of test_adam_steps_vs_torch on elements with |g| >= 1e-3 max|g| ...
BAR_ANY = 0.25                # ... and, x lr, on every element
VISIBLE = 100 * BAR_WELL


def assert_adam_bar(got, ref, grads, lr, what):
    """The project's Adam bar (test_train_general.test_adam_steps_vs_torch): per tensor, |got - ref| <= 0.25 lr everywhere and
    <= 1e-5 where |g| >= 1e-3 max|g|."""
    for i, (a, b, g) in enumerate(zip(got, ref, grads)):
        a, b, g = (np.asarray(x, dtype=np.float64) for x in (a, b, g))
        d = np.abs(a - b)
        assert d.max() <= BAR_ANY * lr, (what, i, d.max())
        well = np.abs(g) >= 1e-3 * np.abs(g).max()
        if well.any():
            assert d[well].max() <= BAR_WELL, (what, i, d[well].max())


def shadow_run(params, grads_per_step, lrs, weight_decay=0.0, decoupled=True, mask=None, max_norms=None, betas=(0.9, 0.999),
               eps=1e-8):
    """torch on the CPU: `params` (arrays) under Adam (coupled decay, or none) or AdamW (decoupled) with the decay on the tensors of
    `mask`, fed grads_per_step[i] (unclipped) at lrs[i], clipped first by clip_grad_norm_(max_norms[i]) when given.  Returns the
    parameters after every step, [steps][tensors] float32 arrays."""
    shadow = [torch.nn.Parameter(torch.tensor(np.asarray(p, dtype=np.float32))) for p in params]
    mask = [False] * len(shadow) if mask is None else mask
    groups = [dict(params=[s for s, d in zip(shadow, mask) if d], weight_decay=float(weight_decay)),
              dict(params=[s for s, d in zip(shadow, mask) if not d], weight_decay=0.0)]
    groups = [g for g in groups if g["params"]]
    kind = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = kind(groups, lr=lrs[0], betas=betas, eps=eps)
    out = []
    for i, grads in enumerate(grads_per_step):
        for g in opt.param_groups:
            g["lr"] = lrs[i]
        for s, gr in zip(shadow, grads):
            s.grad = torch.tensor(np.asarray(gr, dtype=np.float32))
        if max_norms is not None and max_norms[i] is not None:
            torch.nn.utils.clip_grad_norm_(shadow, float(max_norms[i]), norm_type=2)
        opt.step()
        out.append([s.detach().numpy().copy() for s in shadow])
    return out


def assert_visible(with_option, without, params, what):
    """The guard, on the torch side alone: the shadow with the option and the shadow without differ by more than 100 x the bar on at
    least half of every weight matrix (tensor of two or more dimensions).  The bar meant is the one that binds on those elements,
    1e-5 (nearly every element of a weight matrix has |g| >= 1e-3 max|g|): 1e-3.  Every effect of an option on an Adam path scales
    with lr.  Clipping at 0.9 / 0.1 / 0.5 of the norm changes the path by about 0.4 lr for a steady gradient (step 1 is
    scale-invariant; steps 2 and 3 take 0.75 and 0.81 of a full step).  Coupled decay changes an element whose g and p agree in
    sign only by making its gradient steadier, about 0.1 lr per step at 60 % batch noise.  So lr = 1e-3 could show neither, and the
    comparisons run at LR = 2e-2.  DECAY = 1 moves a decoupled weight by 2 lr DECAY |p| = 0.04 |p|, above 1e-3 for |p| > 0.025.

    The first step runs at 1e-4 (LRS).  Adam's first step moves every element by lr sign(g) whatever the clip, so its rate adds
    nothing to what the guard sees; but at 2e-2 it moves each pre-activation of a 128-wide layer by up to 128 x 2e-2 x |input|,
    after which the network's gradient is another one (its norm falls a hundredfold, half its ReLU units die) and the path no
    longer depends on the clip levels, which show only while consecutive gradients are comparable.  At 1e-4 the second step sees
    nearly the first one's gradient, the clip's 0.25 lr of step 2 is there in full, and whatever step 2 does to the network,
    step 3 adds 0.2 lr of the same sign from the moments alone."""
    for i, (a, b, p) in enumerate(zip(with_option, without, params)):
        if np.asarray(p).ndim < 2:
            continue
        far = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) > VISIBLE
        assert far.mean() >= 0.5, (what, i, far.mean())


def global_norm64(grads):
    return float(np.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in grads)))
