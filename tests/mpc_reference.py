"""The fp64 twin of the balancer's two entry points (upkie_amd/csrc/mpc.hpp through `upkie_mpc_step` and
`upkie_mpc_step_env`): a thin wrapper over the checker's `oracle_mpc_step` that adds what `step_env` adds -- the target is
column 0 of an [B][2] action, an env whose `done` word is not 0 gets `MPCBalancer.reset()` instead of a solve (both
workspace columns and its commanded velocity become 0), a target that is not finite counts as 0 -- and leaves every other
env exactly as `oracle_mpc_step` leaves it.

`mutation`: the twin wrong in one named way a kernel could be wrong (tests/test_mpc_matrix_gpu.py shows that the comparison
that guards each of them notices):
  drop_last_index    horizon index N - 1 is treated as padding: its warm start is neither read nor written
  ignore_done        a `done` row is solved like any other
  no_velocity_clamp  the commanded velocity is not held to +-max_ground_velocity
  ignore_fallen      a fallen robot that still touches the ground integrates the first input like an upright one
  target_stride_1    env e reads word e of the action, not word 2 e
"""

import ctypes as C

import numpy as np

from oracle import oracle as O

MUTATIONS = ("drop_last_index", "ignore_done", "no_velocity_clamp", "ignore_fallen", "target_stride_1")
HUGE = 1.0e300  # (a threshold nothing reaches; finite, so that the checker's comparisons stay ordinary)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Twin:
    """`workspace` [2 N][B], `commanded_velocity` [B] and `first_input` [B] in fp64, as `BatchedMpc` holds them."""

    def __init__(self, config, mutation=None):
        assert mutation is None or mutation in MUTATIONS, mutation
        self.mutation = mutation
        self.config = type(config).from_buffer_copy(config)
        if mutation == "no_velocity_clamp":
            self.config.max_ground_velocity = HUGE
        if mutation == "ignore_fallen":
            self.config.fall_pitch = HUGE
        self.N, self.B = int(config.nb_timesteps), int(config.num_envs)
        self.workspace = np.zeros((2 * self.N, self.B))
        self.commanded_velocity = np.zeros(self.B)
        self.first_input = np.zeros(self.B)

    def reset(self, mask=None):
        hit = np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask) != 0
        self.workspace[:, hit] = 0.0
        self.commanded_velocity[hit] = 0.0

    def _drop_last(self):
        if self.mutation == "drop_last_index":
            self.workspace[self.N - 1] = self.workspace[2 * self.N - 1] = 0.0

    def step(self, x0, target_velocity, contact, dt):
        """`upkie_mpc_step`: returns (commanded velocity, first input), views of the twin's own arrays."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        target = np.array(target_velocity, dtype=np.float64)
        target[~(np.abs(target) < 3.0e38)] = 0.0  # the non-finite guard of the kernels
        contact = np.ascontiguousarray(contact, dtype=np.uint8)
        assert x0.shape == (self.B, 4) and target.shape == (self.B,) and contact.shape == (self.B,)
        self._drop_last()
        O.lib().oracle_mpc_step(C.byref(self.config), _p(self.workspace), _p(x0), _p(target), _p(contact), C.c_double(dt),
                                _p(self.commanded_velocity), _p(self.first_input))
        self._drop_last()
        return self.commanded_velocity, self.first_input

    def step_env(self, x0, act, contact, done, dt):
        """`upkie_mpc_step_env`: `act` [B][2], `done` [B] or None. Returns the commanded velocity."""
        act = np.asarray(act)
        assert act.shape == (self.B, 2)
        target = act.reshape(-1)[:self.B] if self.mutation == "target_stride_1" else act[:, 0]
        self.step(x0, target, contact, dt)
        if done is not None and self.mutation != "ignore_done":
            self.reset(np.asarray(done) != 0)  # (-0.0 is 0: not done)
        return self.commanded_velocity
