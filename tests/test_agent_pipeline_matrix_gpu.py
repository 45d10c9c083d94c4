"""Every row of tests/agent_pipeline_shapes.py at every batch size on the MI355X, against the batched numpy twin
(tests/agent_pipeline_reference.py): data movement bit for bit, every stage one step at a time from the device's own state
under the bounds of tests/test_agent_pipeline_gpu.py (the terminal frame included), an env's run against the same env in
another batch, guard words around every buffer the launches write, the counter's wrap, graph replay and poisoned words.
tests/test_agent_pipeline_matrix.py shows without a GPU that the table covers the geometry and that these checks are sharp."""

import numpy as np
import pytest
import torch

from tests import agent_pipeline_shapes as S
from tests.agent_pipeline_shapes import _dev, _np

pytestmark = pytest.mark.gpu
ROWS = pytest.mark.parametrize("row", S.MATRIX, ids=S.IDS)
CASES = pytest.mark.parametrize("row, n", S.CASES, ids=S.CASE_IDS)
STATE = ("observation", "final_observation", "command", "prev_command", "calls")


def _row(K, D, A):
    return next(r for r in S.MATRIX if (r.K, r.D, r.A) == (K, D, A))


class Inputs:
    """A script on the device."""

    def __init__(self, s):
        self.s = s
        self.first, self.again, self.mask = _dev(s.first), _dev(s.again), _dev(s.mask)
        self.actions, self.next_obs, self.final_obs = _dev(s.actions), _dev(s.next_obs), _dev(s.final_obs)
        self.terminated, self.truncated = _dev(s.terminated), _dev(s.truncated.astype(np.uint8))  # (bool and bytes: both are taken)

    def step(self, pipe, t, with_final=True, masks="both"):
        """shape_action and observe of step t; `masks` names the flags the device is given."""
        cmd = pipe.shape_action(self.actions[t])
        obs = pipe.observe(self.next_obs[t], self.terminated[t] if masks in ("both", "terminated") else None,
                           self.truncated[t] if masks in ("both", "truncated") else None, final_obs=self.final_obs[t] if with_final else None)
        return cmd, obs


def _state(pipe):
    return [getattr(pipe, k).clone() for k in STATE]


# ---------------------------------------------------------------- data movement
VARIANTS = [(row, n, True, "both") for row, n in S.CASES]
for _shape in ((8, 4, 1), (256, 1, 1), (1, 1, 6), (5, 8, 5)):
    _r = _row(*_shape)
    _n = S.batch_sizes(_r)[-1]
    VARIANTS += [(_r, _n, True, "terminated"), (_r, _n, True, "truncated"), (_r, _n, True, "none"), (_r, _n, False, "both")]


@pytest.mark.parametrize("row, n, with_final, masks", VARIANTS, ids=[f"{S.row_id(r)}-N{n}-{'final' if f else 'nofinal'}-{m}" for r, n, f, m in VARIANTS])
def test_data_movement_is_bit_exact(row, n, with_final, masks):
    """No noise, no lag, no integration, 2 K + 3 steps (eight at least) behind an unmasked reset, with a masked reset on the way: after every
    step `observation`, `final_observation`, `command` and `prev_command` are the twin's bits (rows of `final_observation`
    of envs that did not end keep what they held), and the counters do not move. `masks` other than "both": the launch is
    given terminated=None, truncated=None or both; nofinal: final_obs=None."""
    want = S.data_movement_trace(row, with_final, masks)
    s = S.script(row, n)
    inputs, pipe = Inputs(s), S.pipeline(row, n, stages=False)
    assert pipe.stacked_dim == S.plan(row)["S"]
    assert np.array_equal(_np(pipe.reset(inputs.first)), want.reset[:n])
    for t in range(s.steps):
        cmd, obs = inputs.step(pipe, t, with_final, masks)
        assert obs.data_ptr() == pipe.observation.data_ptr() and cmd.data_ptr() == pipe.command.data_ptr()
        assert np.array_equal(_np(cmd), want.command[t, :n]) and np.array_equal(_np(cmd), s.actions[t]), t
        assert np.array_equal(_np(obs), want.observation[t, :n]), t
        assert np.array_equal(_np(pipe.final_observation), want.final[t, :n]), t
        assert np.array_equal(_np(pipe.prev_command), want.prev_command[t, :n]), t
        if t == s.reset_after:  # (env 0 holds K frames of one episode: the reset launch zeroes a full stack)
            assert np.array_equal(_np(pipe.reset(inputs.again, inputs.mask)), want.after_reset[:n])
            assert np.array_equal(_np(pipe.prev_command), want.prev_after_reset[:n])
    assert not pipe.calls.any(), "no noise: the counters do not move"


# ---------------------------------------------------------------- every stage, one step at a time
def _within(got, exact, bound, where):
    err = np.abs(got.astype(np.float64) - exact)
    assert (err <= bound).all(), (where, float((err / bound).max()), np.argwhere(err > bound)[:4].tolist())
    return float((err / bound).max()) if err.size else 0.0


@CASES
def test_every_stage_one_step_at_a_time_from_the_devices_own_state(row, n):
    """integrate_action, action_noise, action_lag and observation_noise on, sigmas per column (some 0). Every launch starts
    from the DEVICE's prev_command, stack and counters, so errors do not accumulate; the bounds are
    tests/test_agent_pipeline_gpu.py's (`S.command_bound`, `S.observation_bound`). What is copied is copied bit for bit: the
    moved frames, the command beside a frame, the zeros of a restart. For an env that ended, `final_observation` is the
    old stack moved, then `final_obs` noised from the blocks 64 + (d >> 2) under the same bound, then the command; the other
    rows keep what they held. Every noisy call advances the counter of every env it draws for, by one."""
    K, D, A = row.K, row.D, row.A
    s = S.script(row, n, stages=True)
    inputs, pipe, tw = Inputs(s), S.pipeline(row, n, stages=True), S.twin(row, n, stages=True)
    worst = {"command": 0.0, "observation": 0.0, "terminal": 0.0}
    stack = lambda t: _np(t).reshape(n, K, -1)  # noqa: E731

    def restart(mask, obs, before, calls, prev_before, where):
        got, exact, z = stack(pipe.observation), *tw.frame_exact(obs, calls)
        assert not got[mask, :-1].any() and not got[mask, -1, D:].any() and not _np(pipe.prev_command)[mask].any(), where
        assert np.array_equal(got[~mask], before[~mask]) and np.array_equal(_np(pipe.prev_command)[~mask], prev_before[~mask]), where
        worst["observation"] = max(worst["observation"], _within(got[mask, -1, :D], exact[mask], S.observation_bound(row, exact, z)[mask], where))
        assert np.array_equal(S.counters(pipe), (calls + mask) & 0xFFFFFFFF), where

    zero = np.zeros((n, K, pipe.frame_dim), dtype=S.F32)
    pipe.reset(inputs.first)
    restart(np.ones(n, dtype=bool), s.first, zero, np.zeros(n, dtype=np.int64), np.zeros((n, A), dtype=S.F32), "reset")
    kept = zero.copy()
    for t in range(S.stage_steps(row)):
        prev, calls = _np(pipe.prev_command).copy(), S.counters(pipe)
        cmd = _np(pipe.shape_action(inputs.actions[t])).copy()
        exact, z = tw.shape_action_exact(s.actions[t], prev=prev, calls=calls)
        worst["command"] = max(worst["command"], _within(cmd, exact, S.command_bound(row, z), ("command", t)))
        assert np.array_equal(_np(pipe.prev_command), cmd)
        assert np.array_equal(S.counters(pipe), (calls + 1) & 0xFFFFFFFF)
        before, calls = stack(pipe.observation).copy(), S.counters(pipe)
        done = S.done_of(s, t)
        obs = stack(pipe.observe(inputs.next_obs[t], inputs.terminated[t], inputs.truncated[t], final_obs=inputs.final_obs[t]))
        assert not obs[done, :-1].any() and not obs[done, -1, D:].any() and not _np(pipe.prev_command)[done].any(), t
        assert np.array_equal(obs[~done, :-1], before[~done, 1:]) and np.array_equal(obs[~done, -1, D:], cmd[~done][:, : pipe.frame_dim - D]), t
        assert np.array_equal(_np(pipe.prev_command)[~done], cmd[~done]), t
        exact, z = tw.frame_exact(s.next_obs[t], calls)
        worst["observation"] = max(worst["observation"], _within(obs[:, -1, :D], exact, S.observation_bound(row, exact, z), ("frame", t)))
        final = stack(pipe.final_observation)
        assert np.array_equal(final[~done], kept[~done]), "rows of envs that did not end keep what they held"
        assert np.array_equal(final[done, :-1], before[done, 1:]) and np.array_equal(final[done, -1, D:], cmd[done][:, : pipe.frame_dim - D]), t
        exact, z_terminal = tw.frame_exact(s.final_obs[t], calls, terminal=True)  # (draws of its own: tests/test_agent_pipeline_matrix.py)
        worst["terminal"] = max(worst["terminal"], _within(final[done, -1, :D], exact[done], S.observation_bound(row, exact, z_terminal)[done], ("terminal", t)))
        kept = final.copy()
        assert np.array_equal(S.counters(pipe), (calls + 1) & 0xFFFFFFFF), "ended envs draw as the others do"
        if t == s.reset_after:
            before, prev, calls = stack(pipe.observation).copy(), _np(pipe.prev_command).copy(), S.counters(pipe)
            pipe.reset(inputs.again, inputs.mask)
            restart(s.mask, s.again, before, calls, prev, "masked reset")
    print(f"matrix {S.row_id(row)} N {n}: worst error / bound: command {worst['command']:.3f}, observation {worst['observation']:.3f}, "
          f"terminal {worst['terminal']:.3f}")


# ---------------------------------------------------------------- an env's run does not depend on the batch
def _run(row, n, steps):
    """Every stage on, over the script: the state after the reset, every step and the masked reset (host arrays)."""
    inputs, pipe = Inputs(S.script(row, n, stages=True)), S.pipeline(row, n, stages=True)
    pipe.reset(inputs.first)
    out = [[_np(x) for x in _state(pipe)]]
    for t in range(steps):
        inputs.step(pipe, t)
        out.append([_np(x) for x in _state(pipe)])
        if t == inputs.s.reset_after:
            pipe.reset(inputs.again, inputs.mask)
            out.append([_np(x) for x in _state(pipe)])
    return out


@ROWS
def test_an_envs_run_does_not_depend_on_the_batch_and_repeats(row):
    """Device against device, noise on: the envs two batch sizes share hold the same bits in `command`, `observation`,
    `final_observation`, `prev_command` and `calls` after every launch pair, whichever wavefront, slot and block they fall
    into; the same run from the same state gives the same bits."""
    ns = S.batch_sizes(row)
    large = ns[-1]
    steps = S.stage_steps(row)
    whole = _run(row, large, steps)
    for a, b in zip(whole, _run(row, large, steps)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "a repeated run"
    for small in ns[:-1]:
        for i, (a, b) in enumerate(zip(_run(row, small, steps), whole)):
            for name, x, y in zip(STATE, a, b):
                assert np.array_equal(x, y[:small]), (small, i, name)


# ---------------------------------------------------------------- nothing outside the buffers is written
GUARD, PATTERN = 64, 0x5A5A5A5A  # guard words on either side of a buffer (the views stay 256-byte aligned, as the allocator's)


@CASES
def test_nothing_outside_the_buffers_is_written(row, n):
    """The five tensors the launches write are views into larger buffers with guard words before and after; after both
    resets and K + 3 steps (eight at least) with every stage on, the views hold what an ordinary pipeline holds and the guards their pattern."""
    inputs = Inputs(S.script(row, n, stages=True))
    plain, pipe = S.pipeline(row, n, stages=True), S.pipeline(row, n, stages=True)
    whole = {}
    for name in STATE:
        t = getattr(pipe, name)
        buf = torch.full((t.numel() + 2 * GUARD,), PATTERN, dtype=torch.int32, device=S.DEV)
        view = buf[GUARD:GUARD + t.numel()].view(t.dtype).view(t.shape)
        view.zero_()
        assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * GUARD
        setattr(pipe, name, view)
        whole[name] = buf
    for p in (plain, pipe):
        p.reset(inputs.first)
        for t in range(S.stage_steps(row)):
            inputs.step(p, t)
            if t == inputs.s.reset_after:
                p.reset(inputs.again, inputs.mask)
    torch.cuda.synchronize()
    for name, buf in whole.items():
        assert torch.equal(getattr(pipe, name), getattr(plain, name)), name
        guards = torch.cat([buf[:GUARD], buf[-GUARD:]])
        assert bool((guards == PATTERN).all()), (name, "a guard word changed")
        assert getattr(pipe, name).data_ptr() == buf.data_ptr() + 4 * GUARD


# ---------------------------------------------------------------- the counter wraps
@pytest.mark.parametrize("row", [_row(5, 8, 5), _row(1, 1, 6), _row(1, 256, 33)], ids=S.row_id)
def test_the_counter_wraps_to_zero_and_draws_as_the_twin_at_the_last_call(row):
    n = S.batch_sizes(row)[-1]
    s = S.script(row, n, stages=True)
    inputs, pipe, tw = Inputs(s), S.pipeline(row, n, stages=True), S.twin(row, n, stages=True)
    pipe.reset(inputs.first)
    inputs.step(pipe, 0)
    last = np.arange(n) % 3 != 1  # (env 0, a whole wave's worth of others, not all)
    for launch in ("shape_action", "observe"):
        calls = np.where(last, 0xFFFFFFFF, S.counters(pipe))
        pipe.calls.copy_(_dev(calls.astype(np.uint32).view(np.int32)))
        if launch == "shape_action":
            prev = _np(pipe.prev_command).copy()
            cmd = _np(pipe.shape_action(inputs.actions[1]))
            exact, z = tw.shape_action_exact(s.actions[1], prev=prev, calls=calls)
            _within(cmd, exact, S.command_bound(row, z), launch)
        else:
            obs = _np(pipe.observe(inputs.next_obs[1], None, None)).reshape(n, row.K, -1)
            exact, z = tw.frame_exact(s.next_obs[1], calls)
            _within(obs[:, -1, :row.D], exact, S.observation_bound(row, exact, z), launch)
        assert np.array_equal(S.counters(pipe), np.where(last, 0, calls + 1)), launch


# ---------------------------------------------------------------- graph replay
@pytest.mark.parametrize("row", [_row(256, 1, 1), _row(2, 64, 64)], ids=S.row_id)
def test_a_graphed_loop_of_both_launches_replays_the_eager_bits(row):
    """One stream, no parallel branch: `unroll` steps of shape_action + observe over scripted device-resident inputs, every
    stage on, replayed twice, against the same launches issued eagerly; `calls` is part of what is compared."""
    from upkie_amd.graphs import GraphedLoop

    n, unroll, replays = S.batch_sizes(row)[-1], 4, 2
    inputs = Inputs(S.script(row, n, stages=True))
    assert inputs.s.steps > unroll
    results = []
    for graphed in (False, True):
        pipe = S.pipeline(row, n, stages=True)
        pipe.reset(inputs.first)
        at = [0]

        def step():
            inputs.step(pipe, at[0])
            at[0] = at[0] % unroll + 1  # 0 (the warm-up, executed), then 1 .. unroll, again and again

        if graphed:
            loop = GraphedLoop(step, unroll=unroll, warmup=1, device=pipe.device)
            for _ in range(replays):
                loop.replay()
        else:
            for _ in range(1 + unroll * replays):
                step()
        torch.cuda.synchronize()
        results.append(_state(pipe))
    for name, a, b in zip(STATE, *results):
        assert torch.equal(a, b), name
    assert int(results[0][4].min()) == 1 + 2 * (1 + unroll * replays), "one draw per env at reset, two per step"


# ---------------------------------------------------------------- poisoned words
@pytest.mark.parametrize("row", [_row(2, 64, 64), _row(1, 1, 6)], ids=S.row_id)
def test_a_poisoned_action_word_gives_the_neutral_command_and_touches_no_neighbour(row):
    """Two pipelines in the same state, every stage on: one is given NaN, +inf and -inf in three action words, the other 0
    there. The poisoned words give command 0 and keep prev_command; every other word of both launches, and the counters,
    are the same bits."""
    n, A = S.batch_sizes(row)[-1], row.A
    inputs = Inputs(S.script(row, n, stages=True))
    pipes = [S.pipeline(row, n, stages=True) for _ in range(2)]
    for p in pipes:
        p.reset(inputs.first)
        inputs.step(p, 0, masks="none")
    before = pipes[0].prev_command.clone()
    assert torch.equal(before, pipes[1].prev_command) and bool(before.any())
    where = [(0, 2, float("nan")), (1, 0, float("inf")), (n - 1, A - 1, float("-inf"))]
    clean = inputs.actions[1].clone()
    for e, a, _ in where:
        clean[e, a] = 0.0
    poisoned = clean.clone()
    for e, a, v in where:
        poisoned[e, a] = v
    cmd, ref = pipes[0].shape_action(poisoned), pipes[1].shape_action(clean)
    hit = torch.zeros(n, A, dtype=torch.bool, device=S.DEV)
    for e, a, _ in where:
        hit[e, a] = True
    assert bool((cmd[hit] == 0).all()) and torch.equal(pipes[0].prev_command[hit], before[hit])
    assert torch.equal(cmd[~hit], ref[~hit]) and torch.equal(pipes[0].prev_command[~hit], pipes[1].prev_command[~hit])
    assert torch.equal(pipes[0].calls, pipes[1].calls)
    assert bool(torch.isfinite(cmd).all()) and bool(torch.isfinite(pipes[0].prev_command).all())
