"""Stable-Baselines3's ``evaluate_policy`` and ``EvalCallback`` for a batch of envs, on the device.

SB3 says how good a policy is by running it (deterministically) in an evaluation env until ``n_eval_episodes`` episodes
have ended, env ``i`` giving ``(n_eval_episodes + i) // n_envs`` of them, and reporting the mean and the standard
deviation of their returns. As a Python loop around ``env.step`` that is a variable-length gather of the finished envs,
i.e. a host synchronisation on every step. `EpisodeTally` is that bookkeeping as one launch per step
(``upkie_eval_step``, csrc/eval_episodes.hpp; include/upkie_hip.h states the arithmetic) with all of its state on the
device, `evaluate_policy` the loop around it, captured in a hipGraph and read once per ``chunk`` steps, and
`EvalCallback` the callback of `upkie_amd.ppo.Ppo.learn` that adds ``eval/*`` records and keeps the best model."""

import math
from typing import Callable, Optional

import torch

from . import lib
from .agent_step import AgentStep
from .exceptions import UpkieRuntimeError
from .launch import check, device_tensor, end_flags, launcher, ptr

SUMMARY_NAMES = ("mean_reward", "var_reward", "mean_ep_length", "var_ep_length", "min_reward", "max_reward", "time_limit_frac")


class EpisodeTally:
    """The bookkeeping of SB3's ``evaluate_policy`` for ``num_envs`` envs and up to ``capacity`` episodes.

    ``reset(n_eval_episodes)`` starts an evaluation of E = ``n_eval_episodes`` <= ``capacity`` episodes: env ``i`` is
    to give ``target[i] = (E + i) // num_envs`` of them (with ``num_envs > E`` only the last E envs count, as in SB3).
    ``step(reward, terminated, truncated)`` adds the step's raw reward to the running return (fp64, summed in step
    order) and one to the length of every env below its quota; the envs with ``terminated | truncated`` finish their
    episode, which is appended to the records in increasing env index, so the list is step-major and env-minor: the
    order SB3's loop appends in. An env at its quota is left alone, so steps taken after the last record change
    nothing. The step that fills the list writes `summary`. ``remaining()`` is the number of records still missing
    (one device-to-host read); ``result()`` the finished evaluation.

    Differences from SB3: the mean is ``(r_0 + r_1 + ...) / E`` summed sequentially in fp64 and the variance a second
    sequential pass, not numpy's pairwise sums, so they may differ from ``np.mean`` / ``np.std`` of the same records in
    the last bits; the lengths' mean is exact. ``time_limit_frac`` (the share of episodes ended by the time limit and
    not by termination), ``min_reward`` / ``max_reward`` and ``episode_envs`` are additions; there is no
    ``is_success`` and no ``callback`` per step.

    All state is allocated at construction; a step allocates nothing and has no host argument that changes between
    steps, so it can be captured in a hipGraph (`GraphedLoop`); E is such an argument: a captured step serves the E it
    was captured with. Device only: there is no CPU fallback."""

    def __init__(self, num_envs: int, capacity: int, device="cuda:0"):
        self.num_envs, self.capacity = int(num_envs), int(capacity)
        if self.num_envs < 1:
            raise ValueError("num_envs must be positive")
        if self.capacity < 1:
            raise ValueError("capacity must be positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise UpkieRuntimeError("EpisodeTally runs on the HIP device only (there is no CPU fallback): give device='cuda:0'")
        self._lib = lib.load()
        lib.require(self._lib, "upkie_eval_step", "(the evaluation tally)")
        nbytes = int(self._lib.upkie_eval_workspace_bytes(self.num_envs))
        check(nbytes)
        self._launcher = launcher(self.device)
        N, K, dev = self.num_envs, self.capacity, self.device
        self.ep_return = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ep_length = torch.zeros(N, dtype=torch.int32, device=dev)
        self.count = torch.zeros(N, dtype=torch.int32, device=dev)
        self.target = torch.zeros(N, dtype=torch.int32, device=dev)
        self.rec_return = torch.zeros(K, dtype=torch.float64, device=dev)
        self.rec_length = torch.zeros(K, dtype=torch.int32, device=dev)
        self.rec_env = torch.zeros(K, dtype=torch.int32, device=dev)
        self.rec_truncated = torch.zeros(K, dtype=torch.uint8, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)  # filled, steps
        self.summary = torch.zeros(len(SUMMARY_NAMES), dtype=torch.float64, device=dev)
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # (its ticket starts, and stays, at zero)
        self.n_eval_episodes = 0  # (no evaluation begun: `step` refuses)

    def reset(self, n_eval_episodes: int) -> None:
        """Begin an evaluation of ``n_eval_episodes`` episodes: accumulators, counts, `counters` and `summary` to zero,
        the quotas rewritten. The records of an earlier evaluation are not cleared: only the first ``filled`` count."""
        E = int(n_eval_episodes)
        if not 1 <= E <= self.capacity:
            raise ValueError(f"n_eval_episodes must be in 1-{self.capacity} (the capacity), got {E}")
        self._launcher(self._lib.upkie_eval_reset, self.num_envs, self.capacity, E, self.ep_return.data_ptr(), self.ep_length.data_ptr(),
                       self.count.data_ptr(), self.target.data_ptr(), self.counters.data_ptr(), self.summary.data_ptr())
        self.n_eval_episodes = E

    def step(self, reward: torch.Tensor, terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None) -> None:
        """One env step: ``reward`` [N] float32 (the raw reward), ``terminated`` / ``truncated`` [N] bool or uint8
        (None: none ended)."""
        if self.n_eval_episodes < 1:
            raise UpkieRuntimeError("EpisodeTally.step before reset(n_eval_episodes)")
        reward = device_tensor(reward, "reward", self.device, (self.num_envs,))
        terminated, truncated = end_flags(terminated, truncated, self.device, self.num_envs)
        self._launcher(self._lib.upkie_eval_step, self.num_envs, self.capacity, self.n_eval_episodes, reward.data_ptr(), ptr(terminated),
                       ptr(truncated), self.ep_return.data_ptr(), self.ep_length.data_ptr(), self.count.data_ptr(), self.target.data_ptr(),
                       self.rec_return.data_ptr(), self.rec_length.data_ptr(), self.rec_env.data_ptr(), self.rec_truncated.data_ptr(),
                       self.counters.data_ptr(), self.summary.data_ptr(), self.workspace.data_ptr())

    # ---- host reads (each synchronises with the device)
    def remaining(self) -> int:
        """Records still missing (one device-to-host read); 0: the evaluation is complete and `summary` is written."""
        return self.n_eval_episodes - int(self.counters[0])

    @property
    def steps(self) -> int:
        """Steps the evaluation took so far: those that began with a record missing."""
        return int(self.counters[1])

    def result(self) -> dict:
        """The finished evaluation: ``mean_reward``, ``std_reward``, ``mean_ep_length``, ``std_ep_length``,
        ``min_reward``, ``max_reward``, ``time_limit_frac`` (floats; the standard deviations are the square roots,
        taken here, of the device's population variances) and the lists ``episode_rewards``, ``episode_lengths``,
        ``episode_envs`` in record order. Raises while records are missing."""
        E = self.n_eval_episodes
        missing = self.remaining()
        if E < 1 or missing:
            raise UpkieRuntimeError(f"the evaluation is not complete: {E - missing} of {E} episodes have finished")
        s = dict(zip(SUMMARY_NAMES, self.summary.cpu().tolist()))
        return {"mean_reward": s["mean_reward"], "std_reward": math.sqrt(s["var_reward"]), "mean_ep_length": s["mean_ep_length"],
                "std_ep_length": math.sqrt(s["var_ep_length"]), "min_reward": s["min_reward"], "max_reward": s["max_reward"],
                "time_limit_frac": s["time_limit_frac"], "episode_rewards": self.rec_return[:E].cpu().tolist(),
                "episode_lengths": self.rec_length[:E].cpu().tolist(), "episode_envs": self.rec_env[:E].cpu().tolist()}


class PolicyEvaluator:
    """The objects of one evaluation setup, kept across evaluations: the `EpisodeTally`, the action buffer and the
    captured loop (what `EvalCallback` owns; `evaluate_policy` builds one per call). See `evaluate_policy` for the
    arguments and the order of a step."""

    def __init__(self, policy, env, capacity: int, deterministic: bool = True, pipeline=None, reward=None, reward_fn: Optional[Callable] = None,
                 chunk: int = 32, graph: bool = True, events=None, targets=None):
        mode = getattr(env, "autoreset_mode", None)
        if mode != "same_step":
            raise ValueError(f"evaluation needs an env with autoreset_mode='same_step' (SB3's VecEnv semantics, and the terminal observation "
                             f"the reward terms read), this one has {mode!r}")
        self._agent = AgentStep(env, policy, pipeline, reward, reward_fn, noun="evaluation", events=events, targets=targets)  # (checks the sizes)
        self.events, self.targets = events, targets
        if int(chunk) < 1:
            raise ValueError("chunk must be positive")
        self.policy, self.env, self.pipeline, self.reward, self.reward_fn = policy, env, pipeline, reward, reward_fn
        self.deterministic, self.chunk, self.graph = bool(deterministic), int(chunk), bool(graph)
        self.device = env.device
        N, A = int(env.num_envs), int(policy.shape.act_dim)
        self.tally = EpisodeTally(N, capacity, device=self.device)
        self._action = torch.empty(N, A, dtype=torch.float32, device=self.device)
        self._loop, self._captured_for = None, None

    def begin(self, n_eval_episodes: int, seed: Optional[int] = None) -> None:
        """Start an evaluation over: the pipeline's noise counters zeroed, the env reset (``reset(seed=seed)``) and the
        pipeline's stack restarted, the events restarted (`AgentStep.reset`), the reward's running episodes forgotten, the
        tally reset for ``n_eval_episodes``."""
        if self.pipeline is not None:
            self.pipeline.calls.zero_()  # (its noise starts over, so that two evaluations from one seed draw the same)
        self._agent.reset(seed)
        if self.reward is not None:
            self.reward.reset()
        self.tally.reset(n_eval_episodes)

    def step(self, record: bool = True) -> None:
        """One evaluation step (`evaluate_policy` lists its stages); ``record=False`` leaves the tally's launch out (what
        tools/bench_evaluation.py times the tally against)."""
        pol, agent = self.policy, self._agent
        if self.deterministic:
            pol.mean_action(agent.observation, self._action)
        else:
            pol.act(agent.observation, out={"env_action": self._action})
        _, reward, terminated, truncated, _, _ = agent.apply(self._action)
        agent.observe()
        if record:
            self.tally.step(reward, terminated, truncated)  # the raw reward

    def run(self, n_eval_episodes: int, seed: Optional[int] = None, max_steps: Optional[int] = None) -> dict:
        """One evaluation; `EpisodeTally.result`'s dict."""
        E, N = int(n_eval_episodes), self.tally.num_envs
        if not 1 <= E <= self.tally.capacity:
            raise ValueError(f"n_eval_episodes must be in 1-{self.tally.capacity}, got {E}")
        if max_steps is None:
            limit = getattr(self.env, "max_episode_steps", None)
            if limit is None:
                raise ValueError("evaluation needs a bound on its length: an env with max_episode_steps, or max_steps")
            max_steps = -(-E // N) * int(limit)  # (the largest quota times the longest episode)
        max_steps = int(max_steps)
        if max_steps < 1:
            raise ValueError("max_steps must be positive")
        if self.graph and self._captured_for != E:
            from .graphs import GraphedLoop

            self.begin(E, seed)  # (capture runs ONE real warm-up step, as GraphedLoop does; `begin` below starts over)
            self._loop = GraphedLoop(self.step, unroll=self.chunk, warmup=1, device=self.device)
            self._captured_for = E
        self.begin(E, seed)
        steps, missing = 0, E
        while missing and steps < max_steps:
            n = min(self.chunk, max_steps - steps)
            if self.graph and n == self.chunk:
                self._loop.replay()
            else:  # (eager, and the last steps of a max_steps that is no multiple of the chunk: never more than max_steps)
                for _ in range(n):
                    self.step()
            steps += n
            missing = self.tally.remaining()
        if missing:
            raise UpkieRuntimeError(f"evaluation: {E - missing} of {E} episodes finished within max_steps = {max_steps} steps")
        return self.tally.result()


def evaluate_policy(policy, env, n_eval_episodes: int = 10, deterministic: bool = True, pipeline=None, reward=None,
                    reward_fn: Optional[Callable] = None, seed: Optional[int] = None, max_steps: Optional[int] = None, chunk: int = 32,
                    graph: bool = True, return_episode_rewards: bool = False, events=None, targets=None):
    """SB3's ``evaluate_policy`` on the device: run ``policy`` (an `upkie_amd.policies.MlpActorCritic`) in ``env`` until
    ``n_eval_episodes`` episodes have ended, env ``i`` giving ``(n_eval_episodes + i) // num_envs`` of them, and return
    ``(mean_reward, std_reward)``, or ``(episode_rewards, episode_lengths)`` with ``return_episode_rewards``.

    One evaluation step is: 1. the policy's action from the observation it reads (the env's, or the ``pipeline``'s
    stack): `MlpActorCritic.mean_action`, which serves any batch size and touches nothing of the policy; 2. to 5. the
    two halves of `upkie_amd.agent_step.AgentStep`, back to back: ``pipeline.shape_action``, ``env.step``, the reward
    (``reward``, ``reward_fn`` or the env's own; always raw, never normalised), ``pipeline.observe``; 6.
    `EpisodeTally.step`. The policy normalises observations with its own packed statistics,
    which `RunningNormalizer.attach` keeps live: the evaluation env needs no normaliser and is always in sync with
    training (SB3's ``sync_envs_normalization``). ``pipeline`` and ``reward`` are the evaluation's own instances (sized
    for ``env``), reset when it begins; so is ``events`` (a `upkie_amd.events.EpisodeEvents` built on ``env``: the
    evaluation under random pushes and per-episode inertias), stepped after the reward, and ``targets`` (a
    `upkie_amd.targets.TaskTargets` built on ``env``, with the ranges to evaluate at: a goal-conditioned policy reads its
    rows), stepped right after the env and reset with it.

    ``env`` is reset (``reset(seed=seed)``) first. The loop runs ``chunk`` steps per graph replay (``graph=False``:
    eagerly) and reads `EpisodeTally.remaining` once per chunk; the steps after the last record change nothing, every
    env being at its quota. It takes at most ``max_steps`` steps (default: the largest quota times
    ``env.max_episode_steps``; without either, ``ValueError``) and raises `UpkieRuntimeError` when the quota is not met
    by then. Capturing the loop runs one real warm-up step, after which everything is reset again: graphed and eager
    evaluations from one seed give the same bits. ``env`` must have ``autoreset_mode="same_step"``.

    With ``deterministic=False`` the action is sampled with ``policy.act``: that needs ``env.num_envs`` to be the
    policy's batch size and ADVANCES the policy's per-env noise counters (the warm-up step included), so a training
    run that shares the policy does not continue as it would have."""
    runner = PolicyEvaluator(policy, env, int(n_eval_episodes), deterministic, pipeline, reward, reward_fn, chunk, graph, events, targets)
    result = runner.run(n_eval_episodes, seed, max_steps)
    if return_episode_rewards:
        return result["episode_rewards"], result["episode_lengths"]
    return result["mean_reward"], result["std_reward"]


class EvalCallback:
    """SB3's ``EvalCallback`` for ``Ppo.learn(callback=...)``: every ``eval_freq`` vec-env steps (``num_timesteps /
    n_envs``, as SB3 counts calls) -- at the end of the first iteration at or after each multiple -- the model's policy
    is evaluated deterministically for ``n_eval_episodes`` episodes in ``eval_env`` (any number of envs;
    ``autoreset_mode="same_step"``), reset with the same ``seed`` every time so that successive evaluations are
    comparable. ``eval/mean_reward``, ``eval/mean_ep_length`` and ``eval/time_limit_frac`` are added to that iteration's
    record; off the log interval (``record`` None) a record with these and ``time/total_timesteps``,
    ``time/iterations`` is appended to ``model.records``. `best_mean_reward`, `last_mean_reward` and `evaluations`
    (``timesteps``, ``results``, ``ep_lengths``: the content of SB3's ``evaluations.npz``, in memory) are kept, and
    ``model.save(best_model_save_path)`` is called on a new best. The callback returns None: it never stops training.

    The tally and the captured loop are built by the first evaluation and reused. Evaluation reads the policy's packed
    weights and writes nothing the training run reads (`MlpActorCritic.mean_action`, its own env, tally, ``pipeline``
    and ``reward`` instances, and ``events``, a `upkie_amd.events.EpisodeEvents` built on ``eval_env``, to evaluate
    under pushes and per-episode inertias, and ``targets``, a `upkie_amd.targets.TaskTargets` built on ``eval_env``): a run with this callback trains bit for bit as one without."""

    def __init__(self, eval_env, n_eval_episodes: int = 5, eval_freq: int = 10000, best_model_save_path=None, pipeline=None, reward=None,
                 seed: int = 0, reward_fn: Optional[Callable] = None, max_steps: Optional[int] = None, chunk: int = 32, graph: bool = True,
                 events=None, targets=None):
        self.eval_env, self.n_eval_episodes, self.eval_freq = eval_env, int(n_eval_episodes), int(eval_freq)
        if self.n_eval_episodes < 1 or self.eval_freq < 1:
            raise ValueError("n_eval_episodes and eval_freq must be positive")
        self.best_model_save_path, self.pipeline, self.reward, self.reward_fn = best_model_save_path, pipeline, reward, reward_fn
        self.events = events  # (the evaluation env's own `EpisodeEvents`)
        self.targets = targets  # (the evaluation env's own `TaskTargets`, at the ranges to evaluate at)
        self.seed, self.max_steps, self.chunk, self.graph = seed, max_steps, int(chunk), bool(graph)
        self.best_mean_reward, self.last_mean_reward = -math.inf, None
        self.evaluations = {"timesteps": [], "results": [], "ep_lengths": []}
        self._next, self._iteration = self.eval_freq, 0
        self._runner = None

    def evaluate(self, model) -> dict:
        """One evaluation of ``model.policy`` (`EpisodeTally.result`'s dict)."""
        if self._runner is None or self._runner.policy is not model.policy:
            self._runner = PolicyEvaluator(model.policy, self.eval_env, self.n_eval_episodes, True, self.pipeline, self.reward, self.reward_fn,
                                           self.chunk, self.graph, self.events, self.targets)
        return self._runner.run(self.n_eval_episodes, self.seed, self.max_steps)

    def __call__(self, model, record) -> None:
        vec_steps = int(model.num_timesteps) // int(model.n_envs)
        if int(model.iterations) <= self._iteration:  # (learn(reset_num_timesteps=True) started the count again)
            self._next = self.eval_freq
        self._iteration = int(model.iterations)
        if vec_steps < self._next:
            return None
        self._next = (vec_steps // self.eval_freq + 1) * self.eval_freq
        result = self.evaluate(model)
        mean = float(result["mean_reward"])
        self.last_mean_reward = mean
        self.evaluations["timesteps"].append(int(model.num_timesteps))
        self.evaluations["results"].append(list(result["episode_rewards"]))
        self.evaluations["ep_lengths"].append(list(result["episode_lengths"]))
        if record is None:
            record = {"time/total_timesteps": model.num_timesteps, "time/iterations": model.iterations}
            model.records.append(record)
        record.update({"eval/mean_reward": mean, "eval/mean_ep_length": float(result["mean_ep_length"]),
                       "eval/time_limit_frac": float(result["time_limit_frac"])})
        if mean > self.best_mean_reward:
            self.best_mean_reward = mean
            if self.best_model_save_path is not None:
                model.save(self.best_model_save_path)
        return None
