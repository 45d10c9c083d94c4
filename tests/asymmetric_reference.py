"""fp64 twins of the asymmetric actor-critic (a critic that reads a row of its own: csrc/policy_mlp.hpp, csrc/ppo.hpp,
csrc/privileged_obs.hpp), COMPOSED from the symmetric twins rather than derived again:

* `views` -- an asymmetric policy as two symmetric ones: the actor with a zero critic on the actor's observation, and
  the critic with a zero actor on the critic's row. tests/mlp_reference.py and tests/ppo_reference.py run on each.
* `forward` -- `mlp_reference.forward` once per tower, on each tower's own input and statistics.
* `minibatch` -- no term of PPO's loss couples the towers before the norm clip, so d_log_std and the actor's (W, b) are
  `ppo_reference.minibatch`'s on (actor, obs), the critic's those of a second call on (critic, critic_obs); policy_loss,
  approx_kl and clip_fraction come from the first call, value_loss from the second; loss and ||g|| are recombined.
* `layout` -- the packed layout of an asymmetric shape (held to `upkie_mlp_packed_words` and `pack_index` by
  tests/test_asymmetric_critic.py).
* `PrivilegedTwin` -- the privileged row and its terminal form, restated in numpy; `mutation` breaks it in one line,
  for the CPU test that shows the GPU test's inputs tell each break from the feature.
"""

import math

import numpy as np

from tests import mlp_reference as R
from tests import ppo_reference as PR
from upkie_amd import abi

N_FIXED = 6  # obs_mean, obs_std, action_low, action_high, critic_obs_mean, critic_obs_std; then log_std


def _symmetric(shape, obs_dim, actor_widths, critic_widths):
    s = abi.UpkieMlpShape()
    s.obs_dim, s.act_dim, s.activation = int(obs_dim), int(shape.act_dim), int(shape.activation)
    s.actor_layers, s.critic_layers = len(actor_widths), len(critic_widths)
    for dst, widths in ((s.actor_widths, actor_widths), (s.critic_widths, critic_widths)):
        for i, w in enumerate(widths):
            dst[i] = int(w)
    s.normalize, s.clip_obs = int(shape.normalize), float(shape.clip_obs)
    return s


def _zero_tower(n_in, n_out):
    """(weight, bias) per layer of a one-unit tower that outputs zero: the tower a view does not look at."""
    return [np.zeros((1, n_in)), np.zeros(1), np.zeros((n_out, 1)), np.zeros(n_out)]


def views(shape, sources):
    """((actor shape, actor sources), (critic shape, critic sources)): two symmetric policies in `mlp_reference`'s source
    order, from the sources of an asymmetric one (`MlpActorCritic.sources()` order)."""
    D, A, Dc = int(shape.obs_dim), int(shape.act_dim), int(shape.critic_obs_dim)
    assert Dc > 0, "views() is for asymmetric shapes"
    src = [np.asarray(s, dtype=np.float64) for s in sources]
    mean, std, low, high, cmean, cstd, log_std = src[:N_FIXED + 1]
    na = 2 * (int(shape.actor_layers) + 1)
    actor, critic = src[N_FIXED + 1:N_FIXED + 1 + na], src[N_FIXED + 1 + na:]
    assert len(critic) == 2 * (int(shape.critic_layers) + 1)
    aw, cw = list(shape.actor_widths[: shape.actor_layers]), list(shape.critic_widths[: shape.critic_layers])
    actor_view = (_symmetric(shape, D, aw, [1]), [mean, std, low, high, log_std] + actor + _zero_tower(D, 1))
    critic_view = (_symmetric(shape, Dc, [1], cw), [cmean, cstd, low, high, log_std] + _zero_tower(Dc, A) + critic)
    return actor_view, critic_view


def forward(shape, sources, obs, critic_obs):
    """(normalised obs, mean [N, A], normalised critic obs, value [N]) in fp64."""
    (sa, srca), (sc, srcc) = views(shape, sources)
    x, mean, _ = R.forward(sa, srca, obs)
    xc, _, value = R.forward(sc, srcc, critic_obs)
    return x, mean, xc, value


def minibatch(shape, sources, obs, critic_obs, actions, old_values, old_log_prob, advantages, returns, obs_normalized=False, **cfg):
    """(stats [7], gradient as a list over the trainable sources -- log_std, then (weight, bias) per layer of the actor and
    of the critic --, ratio) of one minibatch of an asymmetric policy."""
    c = dict(PR.DEFAULTS, **cfg)
    (sa, srca), (sc, srcc) = views(shape, sources)
    rest = (actions, old_values, old_log_prob, advantages, returns)
    stats_a, grads_a, ratio = PR.minibatch(sa, srca, obs, *rest, obs_normalized=obs_normalized, **cfg)
    stats_c, grads_c, _ = PR.minibatch(sc, srcc, critic_obs, *rest, obs_normalized=obs_normalized, **cfg)
    na = 2 * (int(shape.actor_layers) + 1)
    grads = grads_a[: 1 + na] + grads_c[1 + 4:]  # (each call's other tower is the four tensors of a zero tower)
    policy_loss, value_loss, entropy_loss = stats_a[0], stats_c[1], stats_a[2]
    loss = policy_loss + c["ent_coef"] * entropy_loss + c["vf_coef"] * value_loss
    norm = math.sqrt(sum(float(np.sum(g * g)) for g in grads))
    return np.array([policy_loss, value_loss, entropy_loss, loss, stats_a[4], stats_a[5], norm]), grads, ratio


def trainable(shape, sources):
    """The trainable sources (log_std, then weight and bias per layer, actor then critic), fp64, shaped."""
    (sa, srca), (sc, srcc) = views(shape, sources)
    na = 2 * (int(shape.actor_layers) + 1)
    return PR.trainable(sa, srca)[: 1 + na] + PR.trainable(sc, srcc)[1 + 4:]


# ---------------------------------------------------------------- the packed layout (mlp_layout, csrc/policy_mlp.hpp)
def layout(shape):
    """Offsets of the packed buffer of an asymmetric shape: `mlp_reference._layout` with the critic's statistics block
    between action_high and log_std, the width class also over critic_obs_dim, and the critic's first layer on
    tiles(critic_obs_dim) input tiles."""
    tiles = lambda w: (int(w) + 15) // 16  # noqa: E731
    D, A, Dc = int(shape.obs_dim), int(shape.act_dim), int(shape.critic_obs_dim)
    widths = [D, A, Dc] + list(shape.actor_widths[: shape.actor_layers]) + list(shape.critic_widths[: shape.critic_layers])
    W = next(c for c in (16, 32, 64, 128, 256) if max(widths) <= c)
    pair = 2 if W >= 32 else 1
    lay, off = {"W": W, "pair": pair}, 0
    dp, dcp, at = (D + 3) // 4 * 4, (Dc + 3) // 4 * 4, 16 * tiles(A)
    blocks = [("mean", dp), ("std", dp), ("low", at), ("high", at)] + ([("critic_mean", dcp), ("critic_std", dcp)] if Dc else []) + [("log_std", at)]
    for name, n in blocks:
        lay[name] = off
        off += n

    def tower(n_in, layers, widths, outputs):
        nonlocal off
        out, in_t = [], tiles(n_in)
        for w in list(widths[:layers]) + [outputs]:
            if w == 1 and len(out) == layers:
                out.append(("dot", off, off + 16 * in_t, in_t, 0))
                off += 16 * in_t + 4
            else:
                out_t = (tiles(w) + pair - 1) // pair * pair
                out.append(("mfma", off, off + out_t * in_t * 256, in_t, out_t))
                off += out_t * in_t * 256 + out_t * 16
                in_t = tiles(w)
        return out

    lay["actor"] = tower(D, shape.actor_layers, shape.actor_widths, A)
    lay["critic"] = tower(Dc or D, shape.critic_layers, shape.critic_widths, 1)
    lay["words"] = off
    return lay


def plan(shape):
    """`ppo_reference.plan` for an asymmetric shape: each tower's stage starts with its own input's tiles."""
    lay = layout(shape)
    act_tiles = (int(shape.act_dim) + 15) // 16

    def stage(layers, in_dim, actor):
        floats = 256 * ((int(in_dim) + 15) // 16)
        for kind, _, _, _, out_t in layers:
            floats += 16 if kind == "dot" else 256 * out_t
        return floats + (256 * act_tiles if actor else 0)

    stages = (stage(lay["actor"], shape.obs_dim, True), stage(lay["critic"], shape.critic_obs_dim or shape.obs_dim, False))
    tile_floats = max(stages)
    nw = min(4, max(1, PR.LDS_BUDGET // (4 * tile_floats)))
    train_words = lay["words"] - lay["log_std"]
    return {"stage_floats": stages, "tile_floats": tile_floats, "nw": nw, "lds_bytes": 4 * nw * tile_floats, "train_off": lay["log_std"],
            "train_words": train_words, "grid_cap": min(PR.MAX_GRID, max(1, PR.PARTIAL_CAP_BYTES // (4 * train_words))),
            "fold_blocks": (train_words + PR.FOLD_THREADS - 1) // PR.FOLD_THREADS}


# ---------------------------------------------------------------- the privileged row (csrc/privileged_obs.hpp)
MUTATIONS = ("new_tail_in_terminal_row", "force_before_events_step", "final_obs_ignored")
# two more, which only a masked reset or an `include` out of the default order can show
LAYOUT_MUTATIONS = MUTATIONS + ("mask_ignored_on_reset", "default_order_starts")
SEGMENTS = ("observation", "command", "push_force", "link_scale")


class PrivilegedTwin:
    """The privileged stage in numpy. ``include``: the segments in order, each of "observation" (D words of next_obs),
    "command" (A words), "push_force" (3 words of force[:, n]) and "link_scale" (link_scale[links, n]). `step` is one
    call after ``events.step``; where the episode ended the terminal row is final_obs (next_obs where there is none) with
    the OLD row's other words around it; without end flags no episode ended. `reset` writes the rows of the envs with
    ``mask`` set (None: all) and leaves the terminal rows alone. ``mutation``: one of `LAYOUT_MUTATIONS`, a one-line
    break of these rules ("default_order_starts": the segments land where the default order would put them)."""

    def __init__(self, num_envs, obs_dim, act_dim, links, include=("observation", "command", "push_force", "link_scale"), mutation=None):
        assert mutation is None or mutation in LAYOUT_MUTATIONS
        self.N, self.D, self.A, self.links, self.include, self.mutation = num_envs, obs_dim, act_dim, list(links), tuple(include), mutation
        counts = {"observation": obs_dim, "command": act_dim, "push_force": 3, "link_scale": len(self.links)}
        self.order = tuple(k for k in SEGMENTS if k in self.include) if mutation == "default_order_starts" else self.include
        self.counts = [counts[k] for k in self.order]
        self.dim = sum(self.counts)
        self.observation = np.zeros((num_envs, self.dim), dtype=np.float32)
        self.final_observation = np.zeros((num_envs, self.dim), dtype=np.float32)
        self._force_before = np.zeros((3, num_envs), dtype=np.float32)

    def _row(self, obs, command, force, link_scale):
        parts = {"observation": lambda: obs[:, : self.D], "command": lambda: command[:, : self.A], "push_force": lambda: force[:3].T,
                 "link_scale": lambda: link_scale[self.links].T}
        return np.concatenate([np.asarray(parts[k](), dtype=np.float32).reshape(self.N, -1) for k in self.order], axis=1)

    def _obs_columns(self):
        cols = np.zeros(self.dim, dtype=bool)
        if "observation" in self.order:
            k = self.order.index("observation")
            start = sum(self.counts[:k])
            cols[start:start + self.D] = True
        return cols

    def reset(self, obs, command, force, link_scale, mask=None):
        new = self._row(obs, command, force, link_scale)
        take = np.ones(self.N, dtype=bool) if mask is None or self.mutation == "mask_ignored_on_reset" else np.asarray(mask) != 0
        self.observation = np.where(take[:, None], new, self.observation)
        self._force_before = np.array(force[:3], dtype=np.float32)
        return self.observation

    def step(self, next_obs, final_obs, command, force, link_scale, terminated=None, truncated=None):
        """``force`` / ``link_scale``: the events' buffers AFTER ``events.step`` of this env step. ``final_obs`` None:
        ``next_obs`` stands in; an end flag None: all zero."""
        final_obs = next_obs if final_obs is None else final_obs
        terminated = np.zeros(self.N, dtype=np.uint8) if terminated is None else terminated
        truncated = np.zeros(self.N, dtype=np.uint8) if truncated is None else truncated
        used = self._force_before if self.mutation == "force_before_events_step" else force
        self._force_before = np.array(force[:3], dtype=np.float32)
        new = self._row(next_obs, command, used, link_scale)
        done = (np.asarray(terminated) != 0) | (np.asarray(truncated) != 0)
        terminal = (new if self.mutation == "new_tail_in_terminal_row" else self.observation).copy()
        last = next_obs if self.mutation == "final_obs_ignored" else final_obs
        terminal[:, self._obs_columns()] = self._row(last, command, used, link_scale)[:, self._obs_columns()]
        self.final_observation = np.where(done[:, None], terminal, new)
        self.observation = new
        return self.observation
