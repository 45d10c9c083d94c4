"""fp64 twin of one minibatch of the mirrored PPO update (csrc/ppo.hpp MIR = true; include/upkie_hip.h, "PPO update with
mirror symmetry"), built from tests/ppo_reference.py's `_forward` and `_backward`: the advantages are normalised over the
B originals, then the 2 B positions (originals, then their mirrored partners) go through the towers, the partners'
surrogate and value terms weighted by `augment`, plus the mirror loss on the actor's means. tests/test_symmetry.py holds
it to torch autograd in fp64. `mutation` breaks it in one line, for the host test that shows that the GPU tests' inputs
tell each break from the feature. Also the builders the tests share: random signed involutions and a rollout whose
original AND mirrored ratios stay clear of the clip bounds."""

import math

import numpy as np

from tests import asymmetric_reference as AR
from tests import mlp_reference as R
from tests import mlp_shapes as S
from tests import ppo_reference as PR
from upkie_amd.symmetry import MirrorSymmetry

STAT_NAMES = ("policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "grad_norm", "mirror_loss")
MUTATIONS = ("actions_not_mirrored", "permutation_without_signs", "target_without_action_mirror", "target_not_detached",
             "normalise_before_mirror", "mirror_loss_over_2ba", "kl_over_n")
LOG_STD = 0.5  # of the GPU tests' inputs: with the helpers' -0.5 a mirrored |log ratio| reaches 36 on the 64-action row


def _towers(shape, sources):
    """(log_std, actor layers, critic layers, normalise(actor rows), normalise(critic rows)) of a symmetric or an
    asymmetric policy."""
    if int(getattr(shape, "critic_obs_dim", 0)) == 0:
        _, _, _, _, log_std, actor, critic = R.split_sources(shape, sources)
        norm = lambda x: R.normalize(shape, sources, x)  # noqa: E731
        return log_std, actor, critic, norm, norm
    (sa, srca), (sc, srcc) = AR.views(shape, sources)
    log_std, actor = R.split_sources(sa, srca)[4:6]
    critic = R.split_sources(sc, srcc)[6]
    return log_std, actor, critic, (lambda x: R.normalize(sa, srca, x)), (lambda x: R.normalize(sc, srcc, x))


def _plain(sym):
    """`sym` with every sign +1 (the "permutation without signs" mistake)."""
    one = lambda s: None if s is None else np.ones_like(s)  # noqa: E731
    return MirrorSymmetry(sym.obs_index, one(sym.obs_sign), sym.act_index, one(sym.act_sign), sym.critic_index, one(sym.critic_sign))


def minibatch(shape, sources, sym, obs, actions, old_values, old_log_prob, advantages, returns, critic_obs=None, obs_normalized=False,
              augment=True, mirror_coef=0.0, mutation=None, details=None, **cfg):
    """(stats [8] as in STAT_NAMES, the gradient as a list over the trainable sources -- log_std, then (weight, bias) per
    layer of the actor and of the critic --, the ratios of the originals [B], those of the mirrored partners [B])."""
    assert mutation is None or mutation in MUTATIONS
    c = dict(PR.DEFAULTS, **cfg)
    log_std, actor, critic, norm_a, norm_c = _towers(shape, sources)
    asym = critic_obs is not None
    if mutation == "permutation_without_signs":
        sym = _plain(sym)
    B = len(obs)
    A = int(shape.act_dim)

    def rows(raw, mirror, normalise):
        """The 2 B input rows of a tower: the stored rows and their mirrors, each then treated as a stored row."""
        x = np.asarray(raw, dtype=np.float64).reshape(B, -1)
        if obs_normalized:
            return np.concatenate([x, mirror(x)])
        if mutation == "normalise_before_mirror":
            return np.concatenate([normalise(x), mirror(normalise(x))])
        return np.concatenate([normalise(x), normalise(mirror(x))])

    xa = rows(obs, sym.mirror_obs, norm_a)
    xc = rows(critic_obs, sym.mirror_critic_obs, norm_c) if asym else xa
    adv = np.asarray(advantages, dtype=np.float64)
    if c["normalize_advantage"] and B > 1:
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)  # (over the originals)
    act = np.asarray(actions, dtype=np.float64).reshape(B, A)
    act = np.concatenate([act, act if mutation == "actions_not_mirrored" else sym.mirror_action(act)])
    two = lambda v: np.tile(np.asarray(v, dtype=np.float64), 2)  # noqa: E731
    adv, old_lp, old_v, ret = two(adv), two(old_log_prob), two(old_values), two(returns)
    live = np.concatenate([np.ones(B, dtype=bool), np.full(B, bool(augment))])  # (the positions whose PPO terms count)
    n = int(live.sum())

    ha = PR._forward(shape, actor, xa)
    mu = ha[-1]
    sigma2 = np.exp(2.0 * log_std)
    d = act - mu
    lp = np.sum(-(d * d) / (2.0 * sigma2) - log_std - PR.HALF_LOG_2PI, axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        ratio = np.exp(lp - old_lp)
        lo, hi = 1.0 - c["clip_range"], 1.0 + c["clip_range"]
        surrogate = np.minimum(adv * ratio, adv * np.clip(ratio, lo, hi))
        g_lp = np.where(live, -PR.surrogate_grad(adv, ratio, c["clip_range"]) * ratio / n, 0.0)
    policy_loss = -np.sum(surrogate[live]) / n
    d_mu = g_lp[:, None] * d / sigma2
    log_std_terms = g_lp[:, None] * (d * d / sigma2 - 1.0)
    d_log_std = np.sum(log_std_terms, axis=0) - c["ent_coef"]

    # the mirror loss: the partner's mean against the mirrored mean of the original, which is a constant
    target = mu[:B] if mutation == "target_without_action_mirror" else sym.mirror_action(mu[:B])
    e = mu[B:] - target
    denominator = (2 if mutation == "mirror_loss_over_2ba" else 1) * B * A
    mirror_loss = np.sum(e * e) / denominator
    d_e = mirror_coef * 2.0 * e / denominator
    d_mu[B:] += d_e
    if mutation == "target_not_detached":  # (d target[a] / d mu[index[a]] = sign[a]; M_a is an involution)
        d_mu[:B] -= sym.mirror_action(d_e)

    hc = PR._forward(shape, critic, xc)
    v = hc[-1][:, 0]
    if c["clip_range_vf"] is None:
        vp, vpass = v, np.ones(2 * B)
    else:
        cv = c["clip_range_vf"]
        vp = old_v + np.clip(v - old_v, -cv, cv)
        vpass = ((v - old_v >= -cv) & (v - old_v <= cv)).astype(np.float64)
    value_loss = np.sum(((ret - vp) ** 2)[live]) / n
    d_v = np.where(live, c["vf_coef"] * 2.0 * (vp - ret) / n * vpass, 0.0)
    if details is not None:  # (the condition numbers of the two gradient tensors that are plain sums of signed terms over the positions)
        details["value_bias_condition"] = float(np.sum(np.abs(d_v)) / max(abs(np.sum(d_v)), 1e-300))
        details["log_std_condition"] = float(np.linalg.norm(np.sum(np.abs(log_std_terms), axis=0)) / max(np.linalg.norm(d_log_std), 1e-300))
    entropy_loss = -np.sum(0.5 + PR.HALF_LOG_2PI + log_std)
    loss = policy_loss + c["ent_coef"] * entropy_loss + c["vf_coef"] * value_loss + mirror_coef * mirror_loss

    grads = [d_log_std]
    for W_b in PR._backward(shape, actor, ha, d_mu) + PR._backward(shape, critic, hc, d_v[:, None]):
        grads += list(W_b)
    norm = math.sqrt(sum(float(np.sum(g * g)) for g in grads))
    over = live if mutation == "kl_over_n" else np.concatenate([np.ones(B, dtype=bool), np.zeros(B, dtype=bool)])
    approx_kl = np.mean(((ratio - 1.0) - (lp - old_lp))[over])
    clip_fraction = np.mean((np.abs(ratio - 1.0) > c["clip_range"])[over])
    stats = np.array([policy_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction, norm, mirror_loss])
    return stats, grads, ratio[:B], ratio[B:]


# ---------------------------------------------------------------- the builders the host and the GPU tests share
def signed_involution(n, rng):
    """(index, sign) of a random signed involution of n words: about half the words swapped in pairs, about a third of
    the orbits flipped, at least one flip (and, from two words on, one swap)."""
    index, sign = np.arange(n), np.ones(n)
    order = rng.permutation(n)
    pairs = max(1, n // 4) if n >= 2 else 0
    for a, b in order[: 2 * pairs].reshape(pairs, 2):
        index[a], index[b] = b, a
    for k in range(n):
        if index[k] >= k and rng.random() < 0.35:
            sign[k] = sign[index[k]] = -1.0
    if (sign > 0).all():
        k = int(order[-1])
        sign[k] = sign[index[k]] = -1.0
    return index, sign


def row_mirror(row, seed=0, critic_dim=0, **kw):
    """The builder's `MirrorSymmetry` of a row of tests/mlp_shapes.MATRIX (and, with `critic_dim`, of a critic row)."""
    rng = np.random.default_rng(77 + seed + 10 * row.seed)
    obs, act = signed_involution(row.obs_dim, rng), signed_involution(row.act_dim, rng)
    critic = signed_involution(critic_dim, rng) if critic_dim else (None, None)
    return MirrorSymmetry(*obs, *act, *critic, **kw)


def identity_mirror(row, **kw):
    return MirrorSymmetry.signs(np.ones(row.obs_dim), np.ones(row.act_dim), **kw)


def row_sources(index, row):
    """The fp64 sources of MATRIX row `index` as the GPU tests build its policy: log_std = LOG_STD."""
    return S.row_sources(row, *S.row_modules(row), S.row_normalize(index), log_std=LOG_STD)


def _nudge(data, lp, lp_m):
    """The shared old log-probs of `data` moved until neither the original's ratio (log-prob `lp`) nor the mirrored
    partner's (`lp_m`) lies within 1e-3 of a clip bound."""
    total = lp.size
    old = data["log_probs"].reshape(total).copy()
    for _ in range(100):
        near = np.zeros(total, dtype=bool)
        for mine in (lp, lp_m):
            ratio = np.exp(mine - old.astype(np.float64))
            near |= (np.abs(ratio - 0.8) < 1.5e-3) | (np.abs(ratio - 1.2) < 1.5e-3)
        if not near.any():
            break
        old[near] += np.float32(0.01)
    else:
        raise AssertionError("the old log-probs could not be nudged clear of the clip bounds")
    data["log_probs"] = old.reshape(data["log_probs"].shape)
    return data


def row_rollout(row, shape, sources, sym, seed=0):
    """`mlp_shapes.row_rollout` (T x N samples, float32) with the shared old log-probs nudged until neither the original's
    nor the mirrored partner's ratio lies within 1e-3 of a clip bound."""
    data = S.row_rollout(row, shape, sources, seed=seed)
    total, D, A = S.T * row.N, row.obs_dim, row.act_dim
    obs, act = data["observations"].reshape(total, D).astype(np.float64), data["actions"].reshape(total, A).astype(np.float64)
    log_std = np.asarray(sources[4], dtype=np.float64)
    _, mean, _ = R.forward(shape, sources, obs)
    _, mean_m, _ = R.forward(shape, sources, sym.mirror_obs(obs))
    return _nudge(data, R.log_prob(act, mean, log_std), R.log_prob(sym.mirror_action(act), mean_m, log_std))


def asymmetric_row_rollout(row, shape, sources, sym, seed=0):
    """`asymmetric_shapes.row_rollout` of a row of its ROWS, nudged likewise (the actor alone decides the ratios)."""
    from tests import asymmetric_shapes as AS

    data = AS.row_rollout(row, shape, sources, seed=seed)
    total, D, A = S.T * row.N, row.obs_dim, row.act_dim
    obs, act = data["observations"].reshape(total, D).astype(np.float64), data["actions"].reshape(total, A).astype(np.float64)
    rows = data["critic_observations"].reshape(total, -1).astype(np.float64)
    log_std = np.asarray(sources[AR.N_FIXED], dtype=np.float64)
    _, mean, _, _ = AR.forward(shape, sources, obs, rows)
    _, mean_m, _, _ = AR.forward(shape, sources, sym.mirror_obs(obs), rows)
    return _nudge(data, R.log_prob(act, mean, log_std), R.log_prob(sym.mirror_action(act), mean_m, log_std))


# The critic's head bias gradient is the plain sum of the positions' signed value errors, zero-mean by construction of the
# rollouts, and log_std's (A words; ONE on a row with one action) that of the positions' signed (d^2 / sigma^2 - 1) terms:
# now and then a mirror makes one cancel (seed 0 on the 1001-5-[40,24]-3 row: the bias to 1/340 of the sum of magnitudes, 170
# times under the other rows'). An fp32 sum carries about its unit roundoff (6e-8) times the condition number sum|x| / |sum x|
# as relative error, so a relative bound of 1e-5 can be asked of it only while that number stays under about 100.
MAX_CONDITION = 100.0


def conditioned_inputs(row, shape, sources, rollout=row_rollout, critic_dim=0, samples=None, **kw):
    """(mirror, rollout data) of a row: the builder's first seed whose inputs keep the condition numbers of
    the critic's head bias gradient and of log_std's under MAX_CONDITION on the first `samples` samples (None: all), augmented. tests/test_symmetry.py
    asserts the condition on what this returns."""
    for seed in range(10):
        sym = row_mirror(row, seed=seed, critic_dim=critic_dim, **kw)
        data = rollout(row, shape, sources, sym)
        if condition(shape, sources, sym, data, samples) <= MAX_CONDITION:
            return sym, data
    raise AssertionError("no mirror of ten keeps the critic's head bias gradient well conditioned")


def condition(shape, sources, sym, data, samples=None):
    total = data["observations"].shape[0] * data["observations"].shape[1]
    B = total if samples is None else samples
    args = [data[k].reshape(total, *data[k].shape[2:])[:B] for k in ("observations", "actions", "values", "log_probs", "advantages", "returns")]
    rows = data["critic_observations"].reshape(total, -1)[:B] if "critic_observations" in data else None
    details = {}
    minibatch(shape, sources, sym, *args, critic_obs=rows, augment=True, mirror_coef=0.5, details=details, ent_coef=0.01, clip_range_vf=0.2)
    return max(details["value_bias_condition"], details["log_std_condition"])
