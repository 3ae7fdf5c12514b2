"""The numpy statements of the parameter update and of the loss forms: what the tests hold the HIP optimiser steps, the weight
average and the losses to, and the one check of the average's controls and of the loss controls.  numpy only -- no torch, no
library -- so a test or a tool may import it without either."""
import numpy as np

LEARNING_RATE = 0.001   # train_network.py:56


def clip_coefficient(norm, max_norm):
    """The factor torch.nn.utils.clip_grad_norm_(params, max_norm) multiplies every gradient by, in float32 as the kernels take it:
    min(1, max_norm / (norm + 1e-6)) -- exactly 1.0 when nothing is clipped; a NaN norm gives NaN (torch.clamp's minimum)."""
    c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def adam_reference(p, g, m, v, step, lr=LEARNING_RATE, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, coef=1.0):
    """One update of one tensor as the finish kernels take it (csrc/train_adam.hpp), in numpy float32: clip (g <- coef g), weight
    decay (decoupled, torch.optim.AdamW: p <- p (1 - lr wd); coupled, torch.optim.Adam(weight_decay=): g <- g + wd p), then
    torch.optim.Adam's update with the bias corrections of `step` (1-based) computed in float64.  Returns (p, m, v), new arrays."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    lr, b1, b2, eps, wd = f(lr), f(betas[0]), f(betas[1]), f(eps), f(weight_decay)
    g = f(coef) * g
    if wd != 0:
        if decoupled:
            p = p * (f(1) - lr * wd)
        else:
            g = g + wd * p
    bc1 = f(1.0 - float(b1) ** step)
    bc2_sqrt = f(np.sqrt(1.0 - float(b2) ** step))
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * g * g
    denom = np.sqrt(v) / bc2_sqrt + eps
    return p - (lr / bc1) * (m / denom), m, v


def weight_average_reference(avg, src, decay):
    """One update of the weight average (include/aqgnn.h "weight averaging") in numpy float32: with d = float32(decay) and
    w = float32(1.0 - float(d)), e' = f32(d * e) + f32(w * p) -- two rounded products and one rounded sum, bit for bit
    torch.optim.swa_utils.get_ema_avg_fn(float(d)) on CPU tensors.  Returns a new array."""
    f = np.float32
    d = f(decay)
    w = f(1.0 - float(d))
    return d * np.asarray(avg, dtype=f) + w * np.asarray(src, dtype=f)


def weight_average_due(step, every):
    """Whether the average is updated behind the Adam update of 1-based step `step`: at the multiples of `every`, wherever an epoch
    or a library call ends."""
    return int(step) % int(every) == 0


def check_average_controls(decay, every):
    """(decay as the float32 the kernel takes, every as int), refused as the library refuses them."""
    try:
        d = np.float32(decay)
    except (TypeError, ValueError):
        raise ValueError("the weight average's decay is a number in [0, 1)") from None
    if not (d >= 0 and d < 1):                               # a NaN fails both; a decay that rounds to 1.0f is refused too
        raise ValueError(f"the weight average's decay must be in [0, 1) as a float32 (got {decay!r})")
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError(f"the weight average's every must be an integer >= 1 (got {every!r})")
    return float(d), int(every)


_checked_average_controls = check_average_controls          # the name it had in train_network


POLICY_LOSS_FORMS = {"reference": 0, "cross_entropy": 1}    # aqg_loss.policy_form (include/aqgnn.h "loss form")


def check_loss_controls(policy_loss, value_loss_weight):
    """(policy_form as the int the library takes, value weight as float), refused in the library's words."""
    form = policy_loss if isinstance(policy_loss, (int, np.integer)) and not isinstance(policy_loss, bool) \
        else POLICY_LOSS_FORMS.get(policy_loss, -1)
    if form not in (0, 1):
        raise ValueError(f"policy_form must be 0 (reference) or 1 (cross-entropy): policy_loss is 'reference' or 'cross_entropy' "
                         f"(got {policy_loss!r})")
    try:
        w = float(np.float32(value_loss_weight))
    except (TypeError, ValueError):
        raise ValueError("value_weight must be finite and >= 0") from None
    if not (w >= 0 and np.isfinite(w)):
        raise ValueError(f"value_weight must be finite and >= 0 (got {value_loss_weight!r})")
    return int(form), w


def loss_reference(logits, value, pi, z, policy_form=1, value_weight=1.0):
    """Both loss terms of a batch and their gradients at the logits and at the pre-tanh value (include/aqgnn.h "loss form"), in
    numpy float64.  logits [B, A], value [B] (the tanh output), pi [B, A] (targets, not renormalised), z [B].
    Returns (loss [B, 2], dlogits [B, A], dvpre [B]): loss[b] = (l_b in the chosen form, the unweighted (v - z)^2); the gradients
    are those of mean_b l_b + value_weight mean_b (v - z)^2.
      policy_form 1: m = max x, lse = m + ln sum exp(x - m), l_b = T lse - sum_a t_a x_a (summed as t_a (lse - x_a)),
                     dlogit = (softmax(x) T - t) / B  -- torch.nn.CrossEntropyLoss()(logits, t) with probability targets
      policy_form 0: the reference's, the same expression on p = softmax(x) in place of x, then back through the softmax."""
    x = np.asarray(logits, dtype=np.float64)
    v = np.asarray(value, dtype=np.float64)
    t = np.asarray(pi, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    B = x.shape[0]
    T = t.sum(axis=1, keepdims=True)

    def lse_of(y):
        m = y.max(axis=1, keepdims=True)
        e = np.exp(y - m)
        s = e.sum(axis=1, keepdims=True)
        return m + np.log(s), e / s

    lse, p = lse_of(x)
    if policy_form == 1:
        lp = (t * (lse - x)).sum(axis=1)
        dlogits = (p * T - t) / B
    elif policy_form == 0:
        lse2, p2 = lse_of(p)
        lp = (t * (lse2 - p)).sum(axis=1)
        dp = (p2 * T - t) / B
        dlogits = p * (dp - (dp * p).sum(axis=1, keepdims=True))
    else:
        raise ValueError("policy_form must be 0 (reference) or 1 (cross-entropy)")
    dv = v - z
    loss = np.stack([lp, dv * dv], axis=1)
    dvpre = float(value_weight) * 2.0 * dv / B * (1.0 - v * v)
    return loss, dlogits, dvpre
