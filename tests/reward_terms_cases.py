"""The scripted cases tests/test_reward_terms.py (CPU: the twin alone) and tests/test_reward_terms_gpu.py (the device)
share: the sizes, a term table per size, six steps of inputs with scripted episode ends, and the error / bound ratio.

Sizes, the smallest at which the kernel's mapping can go wrong: N covers a partial wavefront, the wavefront edge and the
block edge; (D, A, K) covers the 16-byte row load (D = 4), a row of fewer than 4 words, read word by word (D = 3), tap
gathers (D > 4; at D = 256 word 255 is tapped) and the caps (16 terms, 8 taps, 64 actions). Every table's
term 0 is ``|0.8 o[0] - 0.6 a[0] + 0.15 rate[0] + 0.5 sin(o[D - 1])|`` so that every mutation of the twin has something
to change in every table; the other terms cycle through the sources, the functions and the shapes.

Ranges: observations and actions in [-1, 1], dt = 0.3 (so |rate| <= 6.7 and 1 / dt is no float32), coefficients in
[-0.5, 0.5], at most 8 taps: |x| <= 27, and the exp shapes' scales are at least 4, so |x / s| < 8 and exp stays far
from underflow (`Twin.max_exp_argument`, asserted on the CPU)."""

import numpy as np

from tests.reward_terms_reference import F32, Twin
from upkie_amd import rewards as R

N_VALUES = (1, 63, 64, 65, 257)
SIZES = ((4, 1, 1), (4, 1, 16), (6, 2, 5), (30, 6, 16), (256, 64, 16), (3, 2, 3))
DT = 0.3
CLIP = (-0.75, 0.6)
STEPS = 6
_SHAPES = ("identity", "abs", "square", "exp_abs", "exp_square", "deadband")
_FNS = (None, "sin", "cos")


def terms_for(D, A, K):
    """The table of size (D, A, K): a list of (name, Term)."""
    rng = np.random.default_rng(1000 * D + 10 * A + K)
    terms = [("t0", R.Term(-1.0, "abs", taps=[R.obs(0, 0.8), R.act(0, -0.6), R.act_rate(0, 0.15), R.obs(D - 1, 0.5, fn="sin")]))]
    for k in range(1, K):
        taps = []
        for j in range(1 + (3 * k) % 8):
            coef = float(rng.uniform(0.1, 0.5) * rng.choice([-1.0, 1.0]))
            fn = _FNS[(k + 2 * j) % 3]
            which = (k + j) % 5
            if which == 0:
                taps.append(R.obs(int(rng.integers(D)), coef, fn=fn))
            elif which == 1:
                taps.append(R.act(int(rng.integers(A)), coef, fn=fn))
            elif which == 2:
                taps.append(R.act_rate(int(rng.integers(A)), coef, fn=fn))
            elif which == 3:
                taps.append(R.one(coef, fn=fn))
            else:
                taps.append(R.terminated(coef, fn=fn))
        shape = _SHAPES[k % 6]
        scale = {"exp_abs": 4.0 + 0.1 * k, "exp_square": 4.0 + 0.3 * k, "deadband": 0.25}.get(shape)
        weight = float(rng.uniform(0.3, 1.5) * rng.choice([-1.0, 1.0]))
        terms.append((f"t{k}", R.Term(weight, shape, scale=scale, taps=taps)))
    return terms


def inputs(N, D, A, seed=0):
    """Six steps: next_obs, final_obs [6, N, D], action [6, N, A] float32, terminated, truncated [6, N] uint8. Nobody ends
    in step 0; env 0 terminates in step 1; the last env truncates in step 2; every env ends in step 3 (even envs
    terminate, odd ones truncate); env N // 2 is both terminated and truncated in step 4; nobody ends in step 5.
    `final_obs` differs from `next_obs` in every word."""
    rng = np.random.default_rng(seed + 7 * N + D)
    next_obs = rng.uniform(-1.0, 1.0, (STEPS, N, D)).astype(F32)
    shift = rng.uniform(0.2, 0.5, (STEPS, N, D)) * rng.choice([-1.0, 1.0], (STEPS, N, D))
    final_obs = np.clip(next_obs + shift, -1.0, 1.0).astype(F32)
    final_obs = np.where(final_obs == next_obs, -next_obs, final_obs).astype(F32)
    action = rng.uniform(-1.0, 1.0, (STEPS, N, A)).astype(F32)
    terminated, truncated = np.zeros((STEPS, N), dtype=np.uint8), np.zeros((STEPS, N), dtype=np.uint8)
    terminated[1, 0] = 1
    truncated[2, N - 1] = 1
    terminated[3, 0::2] = 1
    truncated[3, 1::2] = 1
    terminated[4, N // 2] = truncated[4, N // 2] = 1
    return next_obs, final_obs, action, terminated, truncated


def worst_ratio(twin: Twin, data, device_values, device_prev=None):
    """The worst |device v - twin v| / bound over the six steps, terms and envs. ``device_values[t]`` [K, N]: the term
    values a device (or another twin) produced in step t. With ``device_prev[t]`` (the device's `prev_action` before step
    t) the twin computes every step from the device's own state; without, it runs on from its own (a mutated twin)."""
    next_obs, final_obs, action, terminated, truncated = data
    worst = 0.0
    for t in range(STEPS):
        prev = None if device_prev is None else device_prev[t]
        v, bound = twin.values(next_obs[t], action[t], terminated[t], truncated[t], final_obs[t], prev_action=prev)
        worst = max(worst, float(np.max(np.abs(np.asarray(device_values[t], dtype=np.float64) - v) / bound)))
        twin.advance(v, action[t], terminated[t], truncated[t])
    return worst


def twin_values(N, D, A, K, mutation=None, clip=CLIP):
    """([v of step t], the twin after the six steps) of a twin run on the scripted inputs."""
    twin = Twin(N, D, A, DT, terms_for(D, A, K), clip=clip, mutation=mutation)
    data = inputs(N, D, A)
    values = []
    for t in range(STEPS):
        values.append(twin.step(data[0][t], data[2][t], data[3][t], data[4][t], data[1][t])[1])
    return values, twin
