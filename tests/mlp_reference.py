"""Host twins of the MLP actor-critic launch (csrc/policy_mlp.hpp), for tests/test_mlp_policy*.py:

* `forward` -- the network in fp64 (numpy) from the source tensors (`MlpActorCritic.sources()` order);
* `log_prob` -- SB3's DiagGaussianDistribution.log_prob summed over the action dimensions, fp64;
* `philox_normal` -- the documented draw (include/upkie_hip.h): z of action a of env n at call c, on
  `oracle.oracle.philox` (the fp64 oracle's Philox4x32-10);
* `emulate_packed` -- the kernel's lane arithmetic (MFMA fragment maps, k order, dot heads) on a packed buffer, in
  fp64: checks the packing against `forward` without a GPU.
"""

import math

import numpy as np

from oracle import oracle as O

STREAM_POLICY = 4
TWO_PI_F32 = np.float32(6.283185307179586)


def split_sources(shape, sources):
    """(mean, std, low, high, log_std, actor [(W, b)], critic [(W, b)]) as fp64 arrays, from the flattened sources."""
    src = [np.asarray(s, dtype=np.float64).reshape(-1) for s in sources]
    mean, std, low, high, log_std = src[:5]
    rest = src[5:]
    D, A = int(shape.obs_dim), int(shape.act_dim)

    def tower(rest, layers, widths, outputs):
        out, n_in = [], D
        for w in list(widths[:layers]) + [outputs]:
            W, b = rest[0].reshape(int(w), n_in), rest[1]
            out.append((W, b))
            rest, n_in = rest[2:], int(w)
        return out, rest

    actor, rest = tower(rest, int(shape.actor_layers), shape.actor_widths, A)
    critic = []
    if shape.critic_layers > 0:
        critic, rest = tower(rest, int(shape.critic_layers), shape.critic_widths, 1)
    assert not rest
    return mean, std, low, high, log_std, actor, critic


def _act(shape, x):
    return np.tanh(x) if int(shape.activation) == 0 else np.maximum(x, 0.0)


def normalize(shape, sources, obs):
    mean, std = split_sources(shape, sources)[:2]
    x = np.asarray(obs, dtype=np.float64).reshape(len(obs), -1)
    if shape.normalize:
        x = np.clip((x - mean) / std, -float(shape.clip_obs), float(shape.clip_obs))
    return x


def forward(shape, sources, obs):
    """(normalised obs, mean [N, A], value [N] or None) in fp64."""
    _, _, _, _, _, actor, critic = split_sources(shape, sources)
    x = normalize(shape, sources, obs)

    def run(layers):
        h = x
        for i, (W, b) in enumerate(layers):
            h = h @ W.T + b
            if i < len(layers) - 1:
                h = _act(shape, h)
        return h

    return x, run(actor), (run(critic)[:, 0] if critic else None)


def log_prob(action, mean, log_std):
    """sum_a -(action - mean)^2 / (2 sigma^2) - log sigma - log(2 pi) / 2, fp64."""
    action, mean, log_std = (np.asarray(v, dtype=np.float64) for v in (action, mean, log_std))
    sigma = np.exp(log_std)
    return np.sum(-((action - mean) ** 2) / (2.0 * sigma**2) - log_std - 0.5 * math.log(2.0 * math.pi), axis=-1)


def philox_normal(env: int, call: int, a: int, seed: int) -> float:
    """z of action a of env `env` at call `call` (the fp32 uniforms and angle as the kernel forms them, the rest fp64)."""
    r = O.philox([env & 0xFFFFFFFF, call & 0xFFFFFFFF, 0, (STREAM_POLICY << 24) | (a >> 2)], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    p, i = (a & 3) >> 1, a & 1
    u1 = np.float32((r[2 * p] >> 8) + 1) * np.float32(1.0 / 16777216.0)  # (0, 1]
    u2 = np.float32(r[2 * p + 1] >> 8) * np.float32(1.0 / 16777216.0)
    angle = float(np.float32(TWO_PI_F32 * u2))
    radius = math.sqrt(-2.0 * math.log(float(u1)))
    return radius * (math.cos(angle) if i == 0 else math.sin(angle))


def philox_normals(n_envs: int, act_dim: int, call, seed: int) -> np.ndarray:
    """[n_envs, act_dim] draws; `call`: one counter for all envs or one per env."""
    calls = np.broadcast_to(np.asarray(call, dtype=np.int64), (n_envs,))
    return np.array([[philox_normal(e, int(calls[e]), a, seed) for a in range(act_dim)] for e in range(n_envs)])


# ---------------------------------------------------------------- the kernel's lane arithmetic on a packed buffer
def _layout(shape):
    """Offsets of the packed buffer, as mlp_layout() (csrc/policy_mlp.hpp) computes them."""
    tiles = lambda w: (int(w) + 15) // 16  # noqa: E731
    widths = [shape.obs_dim, shape.act_dim] + list(shape.actor_widths[: shape.actor_layers]) + list(shape.critic_widths[: shape.critic_layers])
    W = next(c for c in (16, 32, 64, 128, 256) if max(widths) <= c)
    pair = 2 if W >= 32 else 1
    off = 0
    lay = {"W": W, "pair": pair}
    dp =(shape.obs_dim + 3) // 4 * 4
    for name, n in (("mean", dp), ("std", dp), ("low", 16 * tiles(shape.act_dim)), ("high", 16 * tiles(shape.act_dim)), ("log_std", 16 * tiles(shape.act_dim))):
        lay[name] = off
        off += n

    def tower(layers, widths, outputs):
        nonlocal off
        out, in_t = [], tiles(shape.obs_dim)
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

    lay["actor"] = tower(shape.actor_layers, shape.actor_widths, shape.act_dim)
    if shape.critic_layers:
        lay["critic"] = tower(shape.critic_layers, shape.critic_widths, 1)
    lay["words"] = off
    return lay


def emulate_packed(shape, packed, obs):
    """(mean [N, A], value [N] or None) computed from the PACKED buffer the way the kernel reads it, in fp64:
    v_mfma_f32_16x16x4_f32 lane maps (A[i][k] in lane i + 16k, B[k][j] in lane j + 16k, D row 4(l >> 4) + r and
    column l & 15 in register r of lane l), the first layer's natural k order, the later layers' accumulator order."""
    lay = _layout(shape)
    pk = np.asarray(packed, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64).reshape(len(obs), -1)
    N, D, A = len(obs), int(shape.obs_dim), int(shape.act_dim)
    lane = np.arange(64)
    q, col = lane >> 4, lane & 15
    means, values = np.zeros((N, A)), np.zeros(N)
    for e0 in range(0, N, 16):
        env = e0 + col
        ok = env < N
        x = {}  # (t, s) -> [64] B registers of the first layer
        for t in range((D + 15) // 16):
            for s in range(4):
                k = 16 * t + 4 * s + q
                v = np.where(ok & (k < D), obs[np.minimum(env, N - 1), np.minimum(k, D - 1)], 0.0)
                if shape.normalize:
                    m, sd = pk[lay["mean"] + np.minimum(k, D - 1)], pk[lay["std"] + np.minimum(k, D - 1)]
                    v = np.where(ok & (k < D), np.clip((v - m) / sd, -shape.clip_obs, shape.clip_obs), 0.0)
                x[(t, s)] = v

        def run(tower):
            regs = None  # (t, r) -> [64] accumulator registers
            for li, (kind, w_off, b_off, in_t, out_t) in enumerate(tower):
                last = li == len(tower) - 1
                if kind == "dot":
                    part = np.zeros(64)
                    for t in range(in_t):
                        for i in range(4):
                            part += pk[w_off + 16 * t + 4 * q + i] * regs[(t, i)]
                    total = sum(part[col + 16 * g] for g in range(4)) + pk[b_off]
                    return {(0, 0): total}
                new = {}
                for o in range(out_t):
                    acc = np.array([[pk[b_off + 16 * o + row] for _ in range(16)] for row in range(16)])  # [row][col]
                    for t in range(in_t):
                        for s in range(4):
                            if li == 0 and 16 * t + 4 * s >= D:
                                continue
                            a_reg = pk[w_off + ((o * in_t + t) * 64 + lane) * 4 + s]
                            b_reg = x[(t, s)] if li == 0 else regs[(t, s)]
                            Am = a_reg.reshape(4, 16).T  # A[i][k] = lane i + 16k
                            Bm = b_reg.reshape(4, 16)  # B[k][j] = lane j + 16k
                            acc = acc + Am @ Bm
                    for r in range(4):
                        v = acc[4 * q + r, col]
                        new[(o, r)] = v if last else _act(shape, v)
                regs = new
            return regs

        out = run(lay["actor"])
        for a in range(A):
            if lay["actor"][-1][0] == "dot":
                m = out[(0, 0)][:16]
            else:
                m = out[(a // 16, a % 4)][16 * ((a % 16) // 4) : 16 * ((a % 16) // 4) + 16]
            means[e0 : e0 + 16, a][: min(16, N - e0)] = m[: min(16, N - e0)]
        if "critic" in lay:
            values[e0 : e0 + 16] = run(lay["critic"])[(0, 0)][: min(16, N - e0)]
    return means, (values if "critic" in lay else None)
