"""What the training drivers share (`upkie_amd.ppo.Ppo`, `upkie_amd.distill.Distillation`): the counters and `learn` of
Stable-Baselines3's ``OnPolicyAlgorithm``, the rollout's slots and its `GraphedLoop`, the captured update, and the file
of `save` / `load`. A driver adds its stages (`_setup`), its rollout step (`_rollout_step`), its update (`train`) and what
its record and its file hold beyond the common part."""

from typing import Callable, Optional

import torch


class OnPolicyDriver:
    """A driver sets ``env``, ``policy``, ``n_envs``, ``n_steps``, ``graph``, ``gamma``, ``pipeline``, ``targets`` and its
    `upkie_amd.agent_step.AgentStep` (``_agent``) in its constructor, and in `_setup` ``device``, ``trainer``,
    ``episodes``, ``normalizer`` and its stages; tests fill the same members by hand."""

    # where a stage's `state_tensors` go under "tensors" in the file: stage -> (prefix, the names that differ from the stage's own)
    _FILE_NAMES = {}

    def __init__(self):
        self.num_timesteps, self.iterations, self.total_timesteps, self.progress_remaining = 0, 0, 0, 1.0
        self.records = []
        self._loop = self._update_graph = None

    def _observation_normalizer(self, policy, **kw):
        """The `RunningNormalizer` of the observations ``policy`` reads, attached to it: the env's columns, or with a
        pipeline (SB3: VecNormalize over VecFrameStack, so the stack's columns) or targets (D + G) the policy's."""
        from .normalize import RunningNormalizer

        if self.pipeline is None and self.targets is None:
            normalizer = RunningNormalizer.for_env(self.env, gamma=self.gamma, **kw)
        else:
            normalizer = RunningNormalizer(self.n_envs, int(policy.shape.obs_dim), gamma=self.gamma, device=self.device, **kw)
        normalizer.attach(policy)
        return normalizer

    # ---- the rollout: ``n_steps`` slots, filled in turn
    def _begin_rollouts(self) -> None:
        """The last act of `_setup`: the first slot, and with ``graph`` the captured loop of ``n_steps`` rollout steps."""
        self._slot = self.n_steps - 1 if self.graph else 0  # (the capture's warm-up step takes the last slot)
        if self.graph:
            from .graphs import GraphedLoop

            self._loop = GraphedLoop(self._rollout_step, unroll=self.n_steps, warmup=1, device=self.device)

    def _advance_slot(self) -> None:
        self._slot = (self._slot + 1) % self.n_steps

    def collect_rollouts(self) -> None:
        """``n_steps`` steps of every env (SB3's ``collect_rollouts``): one graph replay, or the steps one by one."""
        if self._loop is not None:
            self._loop.replay()
        else:
            for _ in range(self.n_steps):
                self._rollout_step()
        self.num_timesteps += self.n_steps * self.n_envs

    # ---- the update as a graph
    def _replay_update(self, update: Callable, kept) -> None:
        """Replay ``update()``, captured by the first call: one warm-up run off the capture first, after which the
        ``kept`` tensors are put back, so that the first replay is the first update."""
        if self._update_graph is None:
            state = [t.clone() for t in kept]
            update()
            torch.cuda.synchronize(self.device)
            self._update_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._update_graph):
                update()
            for dst, src in zip(kept, state):
                dst.copy_(src)
        self._update_graph.replay()

    # ---- learn
    def _after_rollout(self) -> None:
        """After the rollout and the counters, before `train`: the schedules at ``progress_remaining``."""

    def _rollout_record(self) -> dict:
        """The part of a record every driver logs; `_record`, the driver's, is the whole of it."""
        return {"rollout/ep_rew_mean": self.episodes.ep_rew_mean(), "rollout/ep_len_mean": self.episodes.ep_len_mean(),
                "time/total_timesteps": self.num_timesteps, "time/iterations": self.iterations}

    def learn(self, total_timesteps: int, callback: Optional[Callable] = None, log_interval: int = 1, reset_num_timesteps: bool = True):
        """Train for ``total_timesteps`` env steps (whole iterations of ``n_steps * n_envs``, as SB3). With
        ``reset_num_timesteps=False`` training continues: ``total_timesteps`` more steps, ``progress_remaining`` over
        the sum, as SB3's ``_setup_learn``. Every iteration ``callback(self, record)`` is called, ``record`` None off the
        ``log_interval``; a callback that returns False ends training. Returns self."""
        self._setup()
        if reset_num_timesteps:
            self.num_timesteps, self.iterations = 0, 0
            self.total_timesteps = int(total_timesteps)
        else:
            self.total_timesteps = int(total_timesteps) + self.num_timesteps
        while self.num_timesteps < self.total_timesteps:
            self.collect_rollouts()
            self.iterations += 1
            self.progress_remaining = 1.0 - float(self.num_timesteps) / float(self.total_timesteps)
            self._after_rollout()
            self.train()
            record = None
            if log_interval and self.iterations % int(log_interval) == 0:
                record = self._record()
                self.records.append(record)
            if callback is not None and callback(self, record) is False:
                break
        return self

    # ---- saving and loading
    def _env_tensors(self):
        named = dict(self.env.state_tensors())
        named.setdefault("observation", self._agent.raw_observation)  # (an env without a persistent buffer: the one its latest step handed out)
        return {k: v for k, v in named.items() if isinstance(v, torch.Tensor)}

    def _own_tensors(self) -> dict:
        """The driver's own tensors in the file (no stage holds them)."""
        return {}

    def _state_tensors(self):
        named = self._own_tensors()
        named.update({f"env.{k}": v for k, v in self._env_tensors().items()})
        for stage, (prefix, renamed) in self._FILE_NAMES.items():
            if getattr(self, stage) is not None:
                named.update({renamed.get(k, prefix + k): v for k, v in getattr(self, stage).state_tensors().items()})
        return {k: v for k, v in named.items() if v is not None}

    def _save_own(self, sd: dict) -> None:
        """Add the driver's keys to the file's dictionary."""

    def save(self, path) -> None:
        """``torch.save`` of the training state (tensors and numbers only): everything the next iteration reads."""
        self._setup()
        torch.cuda.synchronize(self.device)
        sd = {"tensors": {k: v.cpu() for k, v in self._state_tensors().items()}, "generator": self.trainer.generator.get_state().cpu(),
              "normalizer": self.normalizer.state_dict() if self.normalizer is not None else None,
              "counters": {"num_timesteps": self.num_timesteps, "iterations": self.iterations, "total_timesteps": self.total_timesteps,
                           "progress_remaining": self.progress_remaining, "policy_seed": int(self.policy.seed)},
              "sizes": {"n_envs": self.n_envs, "n_steps": self.n_steps}}
        self._save_own(sd)
        torch.save(sd, path)

    def _before_restore(self) -> None:
        """Between `_setup` (and the policy's reseed) and the copy of the file's tensors."""

    def _restore_own(self, sd: dict) -> None:
        """What `_save_own` wrote, after the common part."""

    @classmethod
    def _load(cls, path, *args, **kwargs):
        """``cls(*args, **kwargs)`` on fresh objects of the saved sizes, continuing the saved run."""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        model = cls(*args, **kwargs)
        if sd["sizes"] != {"n_envs": model.n_envs, "n_steps": model.n_steps}:
            raise ValueError(f"the file holds a run of {sd['sizes']}, this one is {model.n_envs} envs x {model.n_steps} steps")
        model._setup()
        c = sd["counters"]
        model.policy.reseed(c["policy_seed"])
        model._before_restore()
        for name, dst in model._state_tensors().items():
            if name not in sd["tensors"]:
                raise ValueError(f"the file has no {name}: it was saved from another kind of env, policy or stage")
            dst.copy_(sd["tensors"][name])
        model.trainer.generator.set_state(sd["generator"])
        if model.normalizer is not None:
            model.normalizer.load_state_dict(sd["normalizer"])
        model.num_timesteps, model.iterations, model.total_timesteps = c["num_timesteps"], c["iterations"], c["total_timesteps"]
        model.progress_remaining = c["progress_remaining"]
        model._restore_own(sd)
        model.trainer.sync_modules()
        return model
