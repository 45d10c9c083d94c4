"""Host twin of the reward terms (csrc/reward_terms.hpp; include/upkie_hip.h states the arithmetic), for
tests/test_reward_terms*.py: the whole batch at once in numpy, fp64 for the arithmetic, float32 for what the library
stores as float32 (the table's coefficients, weights, scales, 1 / dt and clamp; `prev_action`). Besides every term's
exact value it carries a bound on what the float32 kernel may differ from it (`Twin.values`), derived operation by
operation, and it can be wrong on purpose (``mutation``), which is how the tests show that they would notice.

The bound. u = 2^-24 is float32's unit roundoff, so one rounding of a value t computed from inputs that are off by at
most P costs ``rnd(t, P) = P (1 + u) + u |t| + 2^-149``. The device's sinf / cosf are held to the OpenCL full-profile
ceiling of 4 ulp and expf to 3 ulp; one ulp of a float32 z is at most 2^-23 |z| = 2 u |z|. sin and cos are
1-Lipschitz; |exp(-(q + d)) - exp(-q)| <= exp(-q) expm1(|d|); |x|, max(., 0) and the clamp are 1-Lipschitz;
|(x + d)^2 - x^2| <= |d| (2 |x| + |d|)."""

import numpy as np

from upkie_amd import abi
from upkie_amd.rewards import SHAPES, Term  # noqa: F401

F32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149
SIN_COS_ULP, EXP_ULP = 4.0, 3.0
MUTATIONS = ("next_obs_on_ended", "prev_action_kept", "swapped_tap_sources", "clamp_before_sums")


def rnd(t, P):
    """The bound after one float32 rounding of a value whose exact twin is t and whose inputs carried P."""
    return P * (1.0 + U) + U * np.abs(t) + TINY


def f32(v) -> float:
    return float(F32(v))


class Twin:
    """``terms``: a list of (name, `Term`) pairs (or a mapping). State as the library's: ``prev_action`` [A, N] float32,
    ``term_sum`` / ``term_last`` [K, N] fp64, ``finished`` [N] int32."""

    def __init__(self, num_envs, obs_dim, act_dim, dt, terms, clip=None, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.N, self.D, self.A, self.mutation = int(num_envs), int(obs_dim), int(act_dim), mutation
        self.terms = [t for _, t in (terms.items() if hasattr(terms, "items") else terms)]
        self.K = len(self.terms)
        self.inv_dt = f32(1.0 / float(dt))
        self.clip = (-np.inf, np.inf) if clip is None else (f32(clip[0]), f32(clip[1]))
        self.prev_action = np.zeros((self.A, self.N), dtype=F32)
        self.term_sum = np.zeros((self.K, self.N))
        self.term_last = np.zeros((self.K, self.N))
        self.finished = np.zeros(self.N, dtype=np.int32)
        self.max_exp_argument = 0.0  # the largest |x / s| (or its square's root) an exp shape has seen

    def _taps(self, term):
        taps = [(t.source, t.index) for t in term.taps]
        if self.mutation == "swapped_tap_sources" and len(taps) > 1 and taps[0][0] != taps[1][0]:
            limit = lambda src: self.D if src == abi.REWARD_OBS else self.A  # noqa: E731
            if taps[0][1] < limit(taps[1][0]) and taps[1][1] < limit(taps[0][0]):
                taps[0], taps[1] = (taps[1][0], taps[0][1]), (taps[0][0], taps[1][1])
        return taps

    def values(self, next_obs, action, terminated=None, truncated=None, final_obs=None, prev_action=None):
        """(v [K, N] fp64: every term's exact value; bound [K, N]: what a correct float32 kernel may differ by) from
        ``prev_action`` (default: the state)."""
        N = self.N
        term = np.zeros(N, dtype=bool) if terminated is None else np.asarray(terminated).astype(bool)
        ended = term | (np.zeros(N, dtype=bool) if truncated is None else np.asarray(truncated).astype(bool))
        o = np.asarray(next_obs, dtype=F32).astype(np.float64)
        if final_obs is not None and self.mutation != "next_obs_on_ended":
            o = np.where(ended[:, None], np.asarray(final_obs, dtype=F32).astype(np.float64), o)
        a = np.asarray(action, dtype=F32).astype(np.float64)
        p = (self.prev_action if prev_action is None else np.asarray(prev_action, dtype=F32)).astype(np.float64)
        v, bound = np.zeros((self.K, N)), np.zeros((self.K, N))
        with np.errstate(all="ignore"):
            for k, t in enumerate(self.terms):
                x, Ex = np.zeros(N), np.zeros(N)
                for (source, index), tap in zip(self._taps(t), t.taps):
                    Es = np.zeros(N)
                    if source == abi.REWARD_OBS:
                        s = o[:, index]
                    elif source == abi.REWARD_ACTION:
                        s = a[:, index]
                    elif source == abi.REWARD_ACTION_RATE:
                        d = a[:, index] - p[index]
                        s = d * self.inv_dt
                        Es = rnd(s, rnd(d, 0.0) * abs(self.inv_dt))
                    elif source == abi.REWARD_ONE:
                        s = np.ones(N)
                    else:
                        s = term.astype(np.float64)
                    if tap.fn != abi.REWARD_FN_ID:
                        s = np.sin(s) if tap.fn == abi.REWARD_FN_SIN else np.cos(s)
                        Es = Es + SIN_COS_ULP * 2.0 * U * (np.abs(s) + Es) + TINY
                    c = f32(tap.coef)
                    x = c * s + x
                    Ex = rnd(x, abs(c) * Es + Ex)
                w = f32(t.weight)
                scale = f32(t.scale) if t.scale is not None else 1.0
                shape = SHAPES[t.shape]
                if shape == abi.REWARD_IDENTITY:
                    y, Ey = x, Ex
                elif shape == abi.REWARD_ABS:
                    y, Ey = np.abs(x), Ex
                elif shape == abi.REWARD_SQUARE:
                    y = x * x
                    Ey = rnd(y, Ex * (2.0 * np.abs(x) + Ex))
                elif shape == abi.REWARD_EXP_ABS:
                    q = np.abs(x) / scale
                    Eq = rnd(q, Ex / scale)
                    y = np.exp(-q)
                    Ey = y * np.expm1(Eq) + EXP_ULP * 2.0 * U * y * np.exp(Eq) + TINY
                    self.max_exp_argument = max(self.max_exp_argument, float(np.nanmax(q)))
                elif shape == abi.REWARD_EXP_SQUARE:
                    q = x / scale
                    Eq = rnd(q, Ex / scale)
                    r = q * q
                    Er = rnd(r, Eq * (2.0 * np.abs(q) + Eq))
                    y = np.exp(-r)
                    Ey = y * np.expm1(Er) + EXP_ULP * 2.0 * U * y * np.exp(Er) + TINY
                    self.max_exp_argument = max(self.max_exp_argument, float(np.nanmax(np.abs(q))))
                else:
                    d = np.abs(x) - scale
                    y = np.where(d < 0.0, 0.0, d)
                    Ey = rnd(d, Ex)
                v[k] = w * y
                bound[k] = rnd(v[k], abs(w) * Ey)
                if self.mutation == "clamp_before_sums":
                    v[k] = np.where(v[k] < self.clip[0], self.clip[0], np.where(v[k] > self.clip[1], self.clip[1], v[k]))
        return v, bound

    @staticmethod
    def reward_bound(v, bound):
        """The bound on the float32 sum of the terms in order (one rounding per term of the sum), before the clamp
        (which is 1-Lipschitz)."""
        r, E = np.zeros(v.shape[1]), np.zeros(v.shape[1])
        for k in range(v.shape[0]):
            r = r + v[k]
            E = rnd(r, E + bound[k])
        return E

    def clamp(self, r):
        lo, hi = self.clip
        return np.where(r < lo, lo, np.where(r > hi, hi, r))  # (a NaN passes)

    def advance(self, v, action, terminated=None, truncated=None):
        """The state update of one step, given every term's value ``v`` [K, N] (the twin's own, or the float32 ones a
        device produced): `term_sum` in fp64 in step order, the episode ends, `prev_action`."""
        N = self.N
        ended = (np.zeros(N, dtype=bool) if terminated is None else np.asarray(terminated).astype(bool)) | (
            np.zeros(N, dtype=bool) if truncated is None else np.asarray(truncated).astype(bool))
        total = self.term_sum + np.asarray(v, dtype=np.float64)
        self.term_last = np.where(ended[None, :], total, self.term_last)
        self.term_sum = np.where(ended[None, :], 0.0, total)
        self.finished = self.finished + ended.astype(np.int32)
        a = np.asarray(action, dtype=F32).T.copy()
        if self.mutation != "prev_action_kept":
            a[:, ended] = 0
        self.prev_action = a

    def step(self, next_obs, action, terminated=None, truncated=None, final_obs=None):
        """One step from the twin's own state: (reward [N] fp64 after the clamp, v [K, N], bound [K, N])."""
        v, bound = self.values(next_obs, action, terminated, truncated, final_obs)
        total = np.zeros(self.N)
        for k in range(self.K):  # (in term order)
            total = total + v[k]
        reward = self.clamp(total)
        self.advance(v, action, terminated, truncated)
        return reward, v, bound

    def reset(self, mask=None):
        mask = np.ones(self.N, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
        self.term_sum[:, mask] = 0.0
        self.prev_action[:, mask] = 0


def float32_reward(v32, clip=None):
    """The library's float32 reward from its own float32 term values ``v32`` [K, N]: the sum in term order, one
    rounding per addition, then the clamp. Bit for bit."""
    v32 = np.asarray(v32, dtype=F32)
    r = np.zeros(v32.shape[1], dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(v32.shape[0]):
            r = (r + v32[k]).astype(F32)
    if clip is not None:
        lo, hi = F32(clip[0]), F32(clip[1])
        r = np.where(r < lo, lo, np.where(r > hi, hi, r)).astype(F32)
    return r
