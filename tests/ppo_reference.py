"""fp64 twin of one PPO minibatch update (csrc/ppo.hpp, include/upkie_hip.h): SB3's loss on an MLP actor-critic, its
gradient by hand-written backpropagation (numpy), clip_grad_norm_ and Adam. For tests/test_ppo*.py; the CPU tests check
it against torch autograd of the literal SB3 expression."""

import math

import numpy as np

from tests import mlp_reference as R

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
DEFAULTS = dict(clip_range=0.2, clip_range_vf=None, normalize_advantage=True, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, lr=3e-4,
                beta1=0.9, beta2=0.999, eps=1e-5)


def _act(shape, z):
    return np.tanh(z) if int(shape.activation) == 0 else np.maximum(z, 0.0)


def _dact(shape, h):
    return 1.0 - h * h if int(shape.activation) == 0 else (h > 0.0).astype(np.float64)


def _forward(shape, layers, x):
    hs = [x]
    for i, (W, b) in enumerate(layers):
        z = hs[-1] @ W.T + b
        hs.append(_act(shape, z) if i < len(layers) - 1 else z)
    return hs  # input, hidden outputs, head output


def _backward(shape, layers, hs, dout):
    """(dW, db) per layer, for d loss / d head output = dout [B, out]."""
    grads = [None] * len(layers)
    dz = dout
    for i in range(len(layers) - 1, -1, -1):
        W, _ = layers[i]
        grads[i] = (dz.T @ hs[i], dz.sum(axis=0))
        if i:
            dz = (dz @ W) * _dact(shape, hs[i])
    return grads


def surrogate_grad(adv, ratio, clip_range):
    """d/d ratio of sum(min(adv ratio, adv clamp(ratio, 1 - c, 1 + c))) as torch autograd forms it: torch.minimum
    splits a tie half / half, clamp passes its bounds."""
    lo, hi = 1.0 - clip_range, 1.0 + clip_range
    a1, a2 = adv * ratio, adv * np.clip(ratio, lo, hi)
    w1 = np.where(a1 < a2, 1.0, np.where(a1 == a2, 0.5, 0.0))
    passes = ((ratio >= lo) & (ratio <= hi)).astype(np.float64)
    return w1 * adv + (1.0 - w1) * adv * passes


def minibatch(shape, sources, obs, actions, old_values, old_log_prob, advantages, returns, obs_normalized=False, **cfg):
    """Loss statistics and the gradient of one minibatch: (stats [7] as in STAT_NAMES with the norm of the gradient, the
    gradient as a list over the trainable sources -- log_std, then (weight, bias) per layer of the actor and of the
    critic, each shaped as the source)."""
    c = dict(DEFAULTS, **cfg)
    _, _, _, _, log_std, actor, critic = R.split_sources(shape, sources)
    x = np.asarray(obs, dtype=np.float64).reshape(len(obs), -1)
    if not obs_normalized:
        x = R.normalize(shape, sources, x)
    B = len(x)
    adv = np.asarray(advantages, dtype=np.float64)
    if c["normalize_advantage"] and B > 1:
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    act = np.asarray(actions, dtype=np.float64).reshape(B, -1)
    old_lp, old_v, ret = (np.asarray(v, dtype=np.float64) for v in (old_log_prob, old_values, returns))

    ha = _forward(shape, actor, x)
    mu = ha[-1]
    sigma2 = np.exp(2.0 * log_std)
    d = act - mu
    lp = np.sum(-(d * d) / (2.0 * sigma2) - log_std - HALF_LOG_2PI, axis=1)
    ratio = np.exp(lp - old_lp)
    lo, hi = 1.0 - c["clip_range"], 1.0 + c["clip_range"]
    policy_loss = -np.mean(np.minimum(adv * ratio, adv * np.clip(ratio, lo, hi)))
    g_lp = -surrogate_grad(adv, ratio, c["clip_range"]) * ratio / B
    d_mu = g_lp[:, None] * d / sigma2
    d_log_std = np.sum(g_lp[:, None] * (d * d / sigma2 - 1.0), axis=0) - c["ent_coef"]

    hc = _forward(shape, critic, x)
    v = hc[-1][:, 0]
    if c["clip_range_vf"] is None:
        vp, vpass = v, np.ones(B)
    else:
        cv = c["clip_range_vf"]
        vp = old_v + np.clip(v - old_v, -cv, cv)
        vpass = ((v - old_v >= -cv) & (v - old_v <= cv)).astype(np.float64)
    value_loss = np.mean((ret - vp) ** 2)
    d_v = c["vf_coef"] * 2.0 * (vp - ret) / B * vpass
    entropy_loss = -np.sum(0.5 + HALF_LOG_2PI + log_std)
    loss = policy_loss + c["ent_coef"] * entropy_loss + c["vf_coef"] * value_loss

    grads = [d_log_std]
    for W_b in _backward(shape, actor, ha, d_mu) + _backward(shape, critic, hc, d_v[:, None]):
        grads += list(W_b)
    norm = math.sqrt(sum(float(np.sum(g * g)) for g in grads))
    approx_kl = np.mean((ratio - 1.0) - (lp - old_lp))
    clip_fraction = np.mean(np.abs(ratio - 1.0) > c["clip_range"])
    stats = np.array([policy_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction, norm])
    return stats, grads, ratio


# ---------------------------------------------------------------- the launch geometry (ppo_plan, csrc/ppo.hpp)
LDS_BUDGET = 65280  # dynamic LDS of the gradient launch while one tile's stage fits
MAX_GRID = 512
PARTIAL_CAP_BYTES = 48 << 20
HEADER_BYTES, STATS, FOLD_THREADS = 256, 4, 256


def plan(shape):
    """The gradient launch's geometry for a shape: the LDS stage of one 16-sample tile per tower in floats (the input,
    every hidden layer's padded output tiles, the head's dZ -- one row of 16 for a dot head -- and the actor's log_std
    terms), the waves per block `nw`, the grid cap and the trainable words."""
    lay = R._layout(shape)
    in_tiles = (int(shape.obs_dim) + 15) // 16
    act_tiles = (int(shape.act_dim) + 15) // 16

    def stage(layers, actor):
        floats = 256 * in_tiles
        for kind, _, _, _, out_t in layers:
            floats += 16 if kind == "dot" else 256 * out_t
        return floats + (256 * act_tiles if actor else 0)

    stages = (stage(lay["actor"], True), stage(lay["critic"], False))
    tile_floats = max(stages)
    nw = min(4, max(1, LDS_BUDGET // (4 * tile_floats)))
    train_words = lay["words"] - lay["log_std"]
    return {"stage_floats": stages, "tile_floats": tile_floats, "nw": nw, "lds_bytes": 4 * nw * tile_floats, "train_off": lay["log_std"],
            "train_words": train_words, "grid_cap": min(MAX_GRID, max(1, PARTIAL_CAP_BYTES // (4 * train_words))),
            "fold_blocks": (train_words + FOLD_THREADS - 1) // FOLD_THREADS}


def chunks(p, n):
    """Chunks of `nw` tiles a minibatch of n samples has; a block takes chunks b, b + grid, ..."""
    return ((n + 15) // 16 + p["nw"] - 1) // p["nw"]


def grid(p, n):
    return min(chunks(p, n), p["grid_cap"])


def workspace_bytes(p, n):
    """upkie_ppo_workspace_bytes: the header, one partial gradient and STATS fp64 loss sums per block, the folded gradient
    and the fold's fp64 partial squares."""
    g = grid(p, n)
    return HEADER_BYTES + 4 * g * p["train_words"] + 8 * g * STATS + 4 * p["train_words"] + 8 * p["fold_blocks"]


def trainable(shape, sources):
    """The trainable sources (log_std, then weight and bias per layer, actor then critic), fp64, shaped."""
    _, _, _, _, log_std, actor, critic = R.split_sources(shape, sources)
    out = [log_std]
    for W, b in actor + critic:
        out += [W, b]
    return out


def adam_step(params, grads, m, v, t, max_grad_norm=0.5, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5):
    """clip_grad_norm_ then one torch.optim.Adam step: (params, m, v, t) after it."""
    norm = math.sqrt(sum(float(np.sum(g * g)) for g in grads))
    coef = min(1.0, max_grad_norm / (norm + 1e-6))
    t = t + 1
    out_p, out_m, out_v = [], [], []
    for p, g, mm, vv in zip(params, grads, m, v):
        g = g * coef
        mm = beta1 * mm + (1.0 - beta1) * g
        vv = beta2 * vv + (1.0 - beta2) * g * g
        out_p.append(p - (lr / (1.0 - beta1**t)) * mm / (np.sqrt(vv) / math.sqrt(1.0 - beta2**t) + eps))
        out_m.append(mm)
        out_v.append(vv)
    return out_p, out_m, out_v, t
