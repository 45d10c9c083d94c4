"""The shapes the agent pipeline's three launches (csrc/agent_pipeline.hpp: shape_action, observe, reset) are tested at, and
the builders the tests share: the plan of a row as the header computes it, its batch sizes, its settings and its scripted
inputs, all plain numpy under seeds of the row.

`MATRIX` holds the shapes of tests/test_agent_pipeline_gpu.py as rows plus the rows that reach the wavefront geometries those
leave out; tests/test_agent_pipeline_matrix.py asserts that the table covers what it claims,
tests/test_agent_pipeline_matrix_gpu.py runs every row at every batch size on the device."""

import functools
from collections import namedtuple

import numpy as np

from tests import agent_pipeline_reference as P

DEV = "cuda:0"
F32 = np.float32
EPS = 2.0 ** -24
WAVE_WORDS, THREADS = 256, 256  # PIPELINE_WAVE_WORDS, PIPELINE_THREADS
WAVES = THREADS // 64  # wavefronts of a block

Row = namedtuple("Row", "K D A in_obs why")

# (stack K, obs_dim D, act_dim A, action_in_observation), then what the row is there for
MATRIX = [
    Row(1, 1, 6, False, "every word slot is another env; A > S: one lane zeroes six prev_command words"),
    Row(3, 1, 2, False, "one dead slot at lane 63, r = 3"),
    Row(1, 4, 1, True, "tests/test_agent_pipeline_gpu.py's; K = 1: no shift"),
    Row(8, 4, 1, True, "tests/test_agent_pipeline_gpu.py's; envs straddle the stride of 64"),
    Row(4, 6, 3, True, "tests/test_agent_pipeline_gpu.py's arithmetic shape"),
    Row(4, 13, 3, True, "an env is exactly one r; 63 live lanes in shape_action"),
    Row(5, 8, 5, True, "one word past a stride; action-noise block 1"),
    Row(2, 57, 7, True, "the shift's source is the same lane one r later"),
    Row(3, 36, 7, True, "one env per wave, nearly half of the slots idle"),
    Row(4, 36, 6, True, "tests/test_agent_pipeline_gpu.py's; 168 words"),
    Row(3, 79, 6, True, "tests/test_agent_pipeline_gpu.py's; 255 of the 256 words"),
    Row(2, 64, 64, True, "the cap; A = 64: action blocks 0-15, one env per shape_action wave, no idle lane"),
    Row(256, 1, 1, False, "shift by one word: every load's source belongs to another lane or another r"),
    Row(1, 256, 33, False, "observation blocks 0-63, terminal blocks 64-127; 31 idle lanes per shape_action wave"),
]
EXISTING = [(1, 4, 1), (8, 4, 1), (4, 36, 6), (3, 79, 6), (4, 6, 3)]  # the (K, D, A) of tests/test_agent_pipeline_gpu.py


def row_id(row):
    return f"K{row.K}-D{row.D}-A{row.A}-{'cmd' if row.in_obs else 'nocmd'}"


IDS = [row_id(r) for r in MATRIX]


def plan(row):
    """The header's `pipeline_sizes` in Python: F, S, group, group_act, used (tests/test_agent_pipeline_matrix.py holds it
    to the header's own)."""
    F = row.D + (row.A if row.in_obs else 0)
    S = row.K * F
    assert 1 <= row.A <= 64 and 1 <= S <= WAVE_WORDS
    group = WAVE_WORDS // S
    return {"F": F, "S": S, "group": group, "group_act": 64 // row.A, "used": group * S}


def blocks(num_envs, group):
    """`pipeline_blocks`: the grid of a launch whose wavefronts serve `group` envs each."""
    waves = -(-num_envs // group)
    return -(-waves // WAVES)


def batch_sizes(row):
    """1; a whole number of observe blocks; one env more (a last block whose only live wave holds one env); an odd N of at
    least two blocks of both kernels; where they exist, one env fewer than an observe wave holds and one more than a
    shape_action wave holds."""
    p = plan(row)
    g, ga = p["group"], p["group_act"]
    odd = max(WAVES * g, WAVES * ga) + 1
    odd += 1 - odd % 2
    sizes = {1, WAVES * g, WAVES * g + 1, odd, ga + 1}
    if g > 1:
        sizes.add(g - 1)
    return sorted(sizes)


CASES = [(row, n) for row in MATRIX for n in batch_sizes(row)]
CASE_IDS = [f"{row_id(row)}-N{n}" for row, n in CASES]


def steps_of(row):
    """Two ends in a row, K - 1 steps that fill the stack, the masked reset, K steps in which a frame travels through the
    whole stack, and one more end on that full stack; eight at least (`stage_steps`)."""
    return max(2 * row.K + 3, 8)


def reset_after(row):
    """The masked reset follows this step: the stack of env 0 then holds K frames of one episode, so that the reset
    launch itself zeroes a full stack at every geometry."""
    return row.K + 1


def stage_steps(row):
    """Steps of the runs with every stage on: through the masked reset and a step behind it, eight at least (the sixth
    drives the integrator into its bounds)."""
    return max(8, row.K + 3)


# ---------------------------------------------------------------- settings
def _pattern(values, n):
    return [values[i % len(values)] for i in range(n)]


def bounds_of(row):
    return _pattern([-1.0, -3.0, -0.25], row.A), _pattern([1.0, 2.0, 0.5], row.A)


def sigmas_of(row):
    """Per-column sigmas, some 0; the last action's and the last column's are not (they alone reach the last block of
    A = 33 and sit in the largest block of every row)."""
    sig_a, sig_o = _pattern([0.05, 0.0, 0.3], row.A), _pattern([0.01, 0.0, 0.1, 0.02, 0.5, 0.003], row.D)
    sig_a[-1], sig_o[-1] = sig_a[-1] or 0.25, sig_o[-1] or 0.125
    return sig_a, sig_o


def seed_of(row):
    return ((7 + row.K) << 32) | (12345 + 1000 * row.D + row.A)


def settings(row, stages):
    """(low, high, dt, keyword arguments) of `AgentPipeline` and of the twins: `stages` False is data movement alone."""
    kw = dict(stack=row.K, action_in_observation=row.in_obs)
    if not stages:
        return [-1.0] * row.A, [1.0] * row.A, 0.005, kw
    low, high = bounds_of(row)
    sig_a, sig_o = sigmas_of(row)
    kw.update(integrate_action=True, action_noise=sig_a, action_lag=0.03, observation_noise=sig_o, seed=seed_of(row))
    return low, high, 0.01, kw


def twin(row, num_envs, stages, **more):
    low, high, dt, kw = settings(row, stages)
    return P.BatchTwin(num_envs, row.D, low, high, dt, **kw, **more)


# ---------------------------------------------------------------- scripted inputs
Script = namedtuple("Script", "first actions next_obs final_obs terminated truncated mask again steps reset_after")


@functools.lru_cache(maxsize=None)
def _script(row, stages):
    """The inputs of a row at its largest N; a smaller batch reads the first rows, so that an env sees the same inputs
    at every batch size. The masks are random (about a fifth of the envs end per step) but for what the matrix demands of
    them at every N (tests/test_agent_pipeline_matrix.py): nobody ends in step 0; env 0 ends in step 1 (terminated
    alone) and in step 2 (truncated alone), survives until the masked reset behind step K + 1 finds its stack full, survives
    the K steps after that and ends in the last step (both flags) on a full stack; env 1 survives step 1 and ends in step 2
    (both); the masked reset takes env 0 and leaves env 1."""
    N, T = max(batch_sizes(row)), steps_of(row)
    rng = np.random.default_rng([row.K, row.D, row.A, int(row.in_obs), int(stages)])
    low, high = (np.asarray(b, dtype=np.float64) for b in settings(row, stages)[:2])
    m = np.maximum(np.maximum(np.abs(low), np.abs(high)), 1.0)
    scale = np.where(np.arange(T) % 6 == 5, 100.0, 1.0)[:, None, None] if stages else 1.0  # (every sixth step drives the integrator into its bounds)
    actions = (rng.uniform(-1, 1, size=(T, N, row.A)) * m * scale).astype(F32)
    normal = lambda *size: rng.normal(size=size).astype(F32)  # noqa: E731
    first, again, next_obs, final_obs = normal(N, row.D), normal(N, row.D), normal(T, N, row.D), normal(T, N, row.D)
    terminated, truncated = rng.uniform(size=(T, N)) < 0.1, rng.uniform(size=(T, N)) < 0.1
    mask = rng.uniform(size=N) < 0.4
    terminated[0], truncated[0] = False, False
    terminated[:, 0], truncated[:, 0] = False, False
    terminated[1, 0] = truncated[2, 0] = terminated[T - 1, 0] = truncated[T - 1, 0] = True
    mask[0] = True
    if N > 1:
        terminated[1, 1] = truncated[1, 1] = False
        terminated[2, 1] = truncated[2, 1] = True
        mask[1] = False
    for a in (first, actions, next_obs, final_obs, terminated, truncated, mask, again):
        a.setflags(write=False)
    return Script(first, actions, next_obs, final_obs, terminated, truncated, mask, again, T, reset_after(row))


def script(row, num_envs, stages=False):
    """The scripted run of a row for its first `num_envs` envs: `first` [N, D] (the unmasked reset), per step `actions`
    [T, N, A], `next_obs`, `final_obs` [T, N, D], `terminated`, `truncated` [T, N]; `mask` [N] and `again` [N, D]: the masked
    reset behind step `reset_after`. Read-only views."""
    s = _script(row, bool(stages))
    n = int(num_envs)
    assert n <= s.first.shape[0]
    return Script(s.first[:n], s.actions[:, :n], s.next_obs[:, :n], s.final_obs[:, :n], s.terminated[:, :n], s.truncated[:, :n], s.mask[:n],
                  s.again[:n], s.steps, s.reset_after)


# ---------------------------------------------------------------- the twin's run of a script, computed once per row
Trace = namedtuple("Trace", "reset command observation final prev_command after_reset prev_after_reset calls")


def run_twin(tw, s, with_final=True, masks="both"):
    """`tw` over the script `s`: what every step leaves. `masks`: which of the two flags the device is given ("both",
    "terminated", "truncated" or "none"); an env ends when a flag that is given is set."""
    out = {k: [] for k in ("command", "observation", "final", "prev_command")}
    reset = tw.reset(s.first).copy()
    after_reset = prev_after = None
    for t in range(s.steps):
        done = done_of(s, t, masks)
        out["command"].append(tw.shape_action(s.actions[t]).copy())
        out["observation"].append(tw.observe(s.next_obs[t], done, s.final_obs[t] if with_final else None).copy())
        out["final"].append(tw.final.reshape(tw.N, -1).copy())
        out["prev_command"].append(tw.prev_command.copy())
        if t == s.reset_after:
            after_reset, prev_after = tw.reset(s.again, s.mask).copy(), tw.prev_command.copy()
    return Trace(reset, *(np.stack(out[k]) for k in ("command", "observation", "final", "prev_command")), after_reset, prev_after, tw.calls.copy())


def done_of(s, t, masks="both"):
    zero = np.zeros_like(s.terminated[t])
    return (s.terminated[t] if masks in ("both", "terminated") else zero) | (s.truncated[t] if masks in ("both", "truncated") else zero)


@functools.lru_cache(maxsize=1)  # (the cases of a row follow one another; the K = 256 row's trace is a quarter of a GiB)
def data_movement_trace(row, with_final=True, masks="both"):
    """The noise-free twin's run at the row's largest N. Noise off, an env's run does not depend on the batch: a smaller
    batch compares with the first rows."""
    n = max(batch_sizes(row))
    trace = run_twin(twin(row, n, stages=False), script(row, n), with_final, masks)
    for a in trace:
        a.setflags(write=False)
    return trace


# ---------------------------------------------------------------- the bounds of the arithmetic (tests/test_agent_pipeline_gpu.py derives them)
def command_bound(row, z):
    """Per command word [N, A]: each stage is at most three float32 roundings of values bounded by m = max(|low|, |high|, 1),
    plus the draw's bound (1e-6 + 2e-7 |z|, the policy's) times sigma (the clip is 1-Lipschitz)."""
    low, high = (np.asarray(b) for b in bounds_of(row))
    m = np.maximum(np.maximum(np.abs(low), np.abs(high)), 1.0)
    return 4 * EPS * m + np.asarray(sigmas_of(row)[0]) * (1e-6 + 2e-7 * np.abs(z))


def observation_bound(row, exact, z):
    """Per noised observation column [N, D]: one fma, rounded once on the device and once in the twin's store, of a value v,
    plus the draw's bound times sigma."""
    return 2 * EPS * np.maximum(np.abs(exact), 1.0) + np.asarray(sigmas_of(row)[1]) * (1e-6 + 2e-7 * np.abs(z))


# ---------------------------------------------------------------- device helpers (torch is imported by the GPU tests only)
def _dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.array(a, order="C"), dtype=dtype).to(DEV)  # (a copy: the scripts are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def counters(pipe):
    """`calls` as uint32 values."""
    return _np(pipe.calls).astype(np.int64) & 0xFFFFFFFF


def pipeline(row, num_envs, stages):
    from upkie_amd.pipeline import AgentPipeline

    low, high, dt, kw = settings(row, stages)
    return AgentPipeline(num_envs, row.D, low, high, dt, device=DEV, **kw)
