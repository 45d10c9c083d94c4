"""The step between a policy's action and the next observation, shared by `upkie_amd.ppo.Ppo` and
`upkie_amd.evaluation.PolicyEvaluator`.

The caller takes the policy's action from `observation` (the env's, or the ``pipeline``'s stack of frames); then

1. `apply`: ``pipeline.shape_action`` (the env receives the shaped command, else the action itself); ``env.step``; the
   reward: ``reward_fn(next_obs, info)``, or ``reward``, a `upkie_amd.rewards.RewardTerms` stepped on the RAW next
   observation, the APPLIED action and ``info["final_obs"]`` (one launch), or by default the env's own. Always raw,
   never normalised: what a Monitor and an evaluation count. With ``targets`` (a `upkie_amd.targets.TaskTargets`: a
   per-env goal appended to the observation) ``targets.step`` runs right after ``env.step``, and from there on the raw
   observation IS ``targets.observation`` and the final one ``targets.final_observation``, D + G words wide: the reward
   terms are stepped on the final rows alone (the step's outcome under the target the policy was given, in every env),
   ``reward_fn`` receives the same rows.
2. the caller's stages that read the raw reward before the stack moves (`Ppo`: the episode statistics);
   Last, ``events.step(terminated, truncated)`` (a `upkie_amd.events.EpisodeEvents`: random pushes, per-episode
   inertias), so that what it decides after step k acts during step k + 1.
3. `observe`: ``pipeline.observe`` on the raw next observation and ``info["final_obs"]``; it returns what a normaliser
   and a time-limit bootstrap read: the stack and its terminal form, or without a pipeline the env's two.

Nothing here allocates per step, so a caller's step can be captured in a hipGraph as before."""

from typing import Callable, Optional


class AgentStep:
    def __init__(self, env, policy, pipeline=None, reward=None, reward_fn: Optional[Callable] = None, noun: str = "rollout",
                 events=None, targets=None):
        """Checks the stages' sizes against each other once; ``noun`` names the caller in the messages."""
        if reward is not None and reward_fn is not None:
            raise ValueError("give reward (a RewardTerms) or reward_fn (a callable), not both")
        if targets is not None:
            N, D = int(env.num_envs), int(policy.shape.obs_dim)
            if int(targets.num_envs) != N:
                raise ValueError(f"the targets serve {targets.num_envs} envs, the {noun} has {N}")
            raw = pipeline.obs_dim if pipeline is not None else D
            if raw != targets.dim:
                raise ValueError(f"the {'pipeline' if pipeline is not None else 'policy'} reads {raw} raw observation words, the env's "
                                 f"{targets.obs_dim} and the {targets.num_targets} targets make {targets.dim}")
        if reward is not None or pipeline is not None:
            N, D, A = int(env.num_envs), int(policy.shape.obs_dim), int(policy.shape.act_dim)
            raw = pipeline.obs_dim if pipeline is not None else D
            if reward is not None and (reward.num_envs != N or reward.act_dim != A or reward.obs_dim != raw):
                raise ValueError(f"the reward serves {reward.num_envs} envs, {reward.obs_dim} observation words and {reward.act_dim} actions, the "
                                 f"{noun} has {N}, {raw} (raw) and {A}")
            if pipeline is not None and D != pipeline.stacked_dim:
                raise ValueError(f"the policy reads {D} observation words, the pipeline stacks {pipeline.stack} frames of "
                                 f"{pipeline.frame_dim} = {pipeline.stacked_dim}")
            if pipeline is not None and (A != pipeline.act_dim or N != pipeline.num_envs):
                raise ValueError(f"the pipeline serves {pipeline.num_envs} envs and {pipeline.act_dim} actions, the env has {N} and the policy {A}")
        if events is not None and int(events.num_envs) != int(env.num_envs):
            raise ValueError(f"the events serve {events.num_envs} envs, the {noun} has {int(env.num_envs)}")
        self.env, self.pipeline, self.reward, self.reward_fn, self.events, self.targets = env, pipeline, reward, reward_fn, events, targets
        self.raw_observation = None  # the env's latest observation (an env without a persistent buffer hands out a new one per step)
        self._stepped = None  # what the latest `apply` returned

    def reset(self, seed: Optional[int] = None):
        """``env.reset``, then ``targets.reset`` on the first observation (the first targets, the first row), then the
        pipeline's stack restarted on the first row, then ``events.reset``."""
        reset = self.env.reset(seed=seed) if seed is not None else self.env.reset()
        obs = getattr(self.env, "observation", None)
        if obs is None:
            obs = reset[0] if isinstance(reset, tuple) else reset
        if self.targets is not None:
            obs = self.targets.reset(obs)
        self.raw_observation = obs
        if self.pipeline is not None:
            self.pipeline.reset(obs)
        if self.events is not None:
            self.events.reset()

    @property
    def observation(self):
        """The observation the policy reads: the env's, or with a pipeline the stack of frames it keeps."""
        return self.raw_observation if self.pipeline is None else self.pipeline.observation

    def apply(self, env_action):
        """The first half; returns ``(next_obs, reward, terminated, truncated, final_obs, info)``."""
        action = env_action if self.pipeline is None else self.pipeline.shape_action(env_action)  # (what the env receives)
        stepped = self.env.step(action)
        next_obs, reward, terminated, truncated = stepped[:4]
        info = stepped[4] if len(stepped) > 4 else {}
        self.raw_observation = next_obs
        final_obs = info.get("final_obs") if hasattr(info, "get") else None
        if self.targets is not None:  # (the rows with the targets: the final one is written for every env)
            next_obs = self.targets.step(next_obs, terminated, truncated, final_obs=final_obs)
            final_obs = self.targets.final_observation
            self.raw_observation = next_obs
            if self.reward_fn is not None:
                reward = self.reward_fn(final_obs, info)
            elif self.reward is not None:
                reward = self.reward.step(final_obs, action, terminated, truncated, final_obs=None)
        elif self.reward_fn is not None:
            reward = self.reward_fn(next_obs, info)
        elif self.reward is not None:
            reward = self.reward.step(next_obs, action, terminated, truncated, final_obs=final_obs)
        if self.events is not None:
            self.events.step(terminated, truncated)
        self._stepped = stepped = (next_obs, reward, terminated, truncated, final_obs, info)
        return stepped

    def observe(self):
        """The second half; returns ``(observation, final observation)`` as the policy reads them."""
        (next_obs, _, terminated, truncated, final_obs, _), pipe = self._stepped, self.pipeline
        if pipe is None:
            return next_obs, final_obs
        pipe.observe(next_obs, terminated, truncated, final_obs=final_obs)
        return pipe.observation, pipe.final_observation
