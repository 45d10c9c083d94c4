"""fp64 twin of the episode events (csrc/episode_events.hpp; include/upkie_hip.h, "Episode events"): the five steps of a
call per env, the link factors ``1 + uniform(-v, v, u)`` as oracle/upkie_oracle.c writes them and `fuse_links` of
csrc/host_setup.hpp restated in fp64 from the model's link tables, in the oracle's order of operations. Philox4x32-10 is
restated in numpy over whole batches (tests/test_episode_events.py holds it to the oracle's exported rounds). Plain
numpy, no device; `gpu_cases` are the inputs tests/test_episode_events_gpu.py drives the kernel with."""

import numpy as np

from upkie_amd import abi

STREAM_INERTIA, STREAM_PUSH, STREAM_EVENTS = 2, 3, 6
TWO_PI = 6.283185307179586  # (the constant of the kernels and of the oracle)
MUTATIONS = ("done_keeps_remaining", "countdown_after_decision", "redraw_before_increment")


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The rounds on arrays of uint32 words (any broadcastable shapes); returns the four output words."""
    u32, u64 = np.uint32, np.uint64
    c0, c1, c2, c3 = (np.asarray(c, dtype=u64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1, mask = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF, u64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = u64(0xD2511F53) * c0, u64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> u64(32)) ^ c1 ^ u64(k0), p1 & mask, (p0 >> u64(32)) ^ c3 ^ u64(k1), p0 & mask
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c.astype(u32) for c in (c0, c1, c2, c3)]


def link_tables(model: abi.UpkieModel):
    """(count, body, randomized, mass, com, inertia) as `randomize_inertias` sees the links: one per body when the model
    names none (convert_links, csrc/host_setup.hpp)."""
    n = int(model.num_links)
    if n > 0:
        return (n, [int(model.link_body[l]) for l in range(n)], [model.link_randomized[l] != 0 for l in range(n)],
                [float(model.link_mass[l]) for l in range(n)], [[float(x) for x in model.link_com[l]] for l in range(n)],
                [[float(x) for x in model.link_inertia[l]] for l in range(n)])
    return (abi.NB, list(range(abi.NB)), [True] * abi.NB, [float(model.mass[b]) for b in range(abi.NB)],
            [[float(x) for x in model.com[b]] for b in range(abi.NB)], [[float(x) for x in model.inertia[b]] for b in range(abi.NB)])


def fuse_links(tables, f):
    """`fuse_links` for a batch: ``f`` [MAX_LINKS, n] link factors -> records [NB * INERTIAL_WORDS, n]."""
    count, body, _, mass, com, inertia = tables
    n = f.shape[1]
    records = np.zeros((abi.NB * abi.INERTIAL_WORDS, n))
    for b in range(abi.NB):
        m, mc = np.zeros(n), [np.zeros(n) for _ in range(3)]
        for l in range(count):
            if body[l] != b:
                continue
            ml = f[l] * mass[l]
            m = m + ml
            for d in range(3):
                mc[d] = mc[d] + ml * com[l][d]
        c = [mc[d] / m for d in range(3)]
        I = [np.zeros(n) for _ in range(6)]
        for l in range(count):
            if body[l] != b:
                continue
            ml = f[l] * mass[l]
            d = [com[l][k] - c[k] for k in range(3)]
            I[0] = I[0] + (f[l] * inertia[l][0] + ml * (d[1] * d[1] + d[2] * d[2]))
            I[1] = I[1] + (f[l] * inertia[l][1] + ml * (d[0] * d[0] + d[2] * d[2]))
            I[2] = I[2] + (f[l] * inertia[l][2] + ml * (d[0] * d[0] + d[1] * d[1]))
            I[3] = I[3] + (f[l] * inertia[l][3] - ml * d[0] * d[1])
            I[4] = I[4] + (f[l] * inertia[l][4] - ml * d[0] * d[2])
            I[5] = I[5] + (f[l] * inertia[l][5] - ml * d[1] * d[2])
        r = abi.INERTIAL_WORDS * b
        records[r] = m
        for k in range(3):
            records[r + 1 + k] = c[k]
        for k in range(6):
            records[r + 4 + k] = I[k]
    return records


class Twin:
    """The stage for ``num_envs`` envs with global ids ``env_id_offset + n`` under the sim's ``seed``. ``mutation``: one of
    `MUTATIONS`, a one-line bug the GPU test's inputs have to tell from the stage."""

    def __init__(self, model: abi.UpkieModel, num_envs: int, seed: int = 0, env_id_offset: int = 0, push_prob: float = 0.0,
                 push_norm=(0.0, 20.0), push_steps=(1, 1), inertia_variation: float = 0.0, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.N, self.mutation = int(num_envs), mutation
        self.tables = link_tables(model)
        self.key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        ids = (int(env_id_offset) + np.arange(self.N, dtype=np.uint64)) & np.uint64(0xFFFFFFFFFFFFFFFF)
        self.env_lo, self.env_hi = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ids >> np.uint64(32)).astype(np.uint32)
        self.threshold = int(np.floor(float(push_prob) * 2.0 ** 24 + 0.5))  # llround
        self.norm_min, self.norm_max = float(push_norm[0]), float(push_norm[1])
        self.steps_min, self.steps_max = int(push_steps[0]), int(push_steps[1])
        self.variation = float(inertia_variation)
        N = self.N
        self.calls, self.pushes, self.episodes = (np.zeros(N, dtype=np.uint32) for _ in range(3))
        self.remaining = np.zeros(N, dtype=np.int32)
        self.force = np.zeros((3, N))
        self.body_inertials = self.link_scale = None
        if self.variation > 0.0:
            self.body_inertials = np.zeros((abi.NB * abi.INERTIAL_WORDS, N))
            self.link_scale = np.ones((abi.MAX_LINKS, N))
        self.reset()

    def _block(self, envs, word2, stream, block=0):
        return philox4x32_10(self.env_lo[envs], self.env_hi[envs], word2, np.uint32((stream << 24) | block), *self.key)

    def link_factors(self, envs, episode):
        """[MAX_LINKS, len(envs)] factors of (env, episode): blocks 0 .. MAX_LINKS / 4 - 1 of the inertia stream."""
        count, _, randomized = self.tables[:3]
        f = np.ones((abi.MAX_LINKS, len(envs)))
        for blk in range(abi.MAX_LINKS // 4):
            r = self._block(envs, episode, STREAM_INERTIA, blk)
            for i in range(4):
                l = 4 * blk + i
                if l < count and randomized[l]:
                    u = (r[i] >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)
                    f[l] = 1.0 + (-self.variation + (self.variation - -self.variation) * u)
        return f

    def _redraw(self, envs, episode):
        f = self.link_factors(envs, episode)
        self.link_scale[:, envs] = f
        self.body_inertials[:, envs] = fuse_links(self.tables, f)

    def push(self, envs, k):
        """[3, len(envs)]: push number ``k`` (array or scalar) of the envs."""
        r = self._block(envs, k, STREAM_PUSH)
        u0, u1 = ((r[i] >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0) for i in (0, 1))
        norm, phi = self.norm_min + (self.norm_max - self.norm_min) * u0, TWO_PI * u1
        return np.stack([norm * np.cos(phi), norm * np.sin(phi), np.zeros(len(envs))])

    def reset(self, mask=None):
        envs = np.arange(self.N) if mask is None else np.flatnonzero(np.asarray(mask))
        for a in (self.calls, self.remaining, self.pushes, self.episodes):
            a[envs] = 0
        self.force[:, envs] = 0.0
        if self.variation > 0.0 and len(envs):
            self._redraw(envs, np.uint32(0))

    def step(self, terminated=None, truncated=None):
        """One call; returns what happened per env, as boolean arrays: ``start``, ``hold`` (force left as it is),
        ``zero`` (a free step without a start), ``cut`` (a held push ended by the episode's end), ``redrawn``."""
        N, every = self.N, np.arange(self.N)
        done = np.zeros(N, dtype=bool)
        for flag in (terminated, truncated):
            if flag is not None:
                done |= np.asarray(flag).astype(bool)
        r = self._block(every, self.calls, STREAM_EVENTS)  # 1. every env, every call
        self.calls += np.uint32(1)
        cut = done & (self.remaining > 1)  # (a force that the countdown alone would still have held)
        ended = np.flatnonzero(done)  # 2.
        if self.mutation == "redraw_before_increment" and self.variation > 0.0 and len(ended):
            self._redraw(ended, self.episodes[ended])
        self.episodes[ended] += np.uint32(1)
        if self.mutation != "done_keeps_remaining":
            self.remaining[ended] = 0
        if self.mutation != "redraw_before_increment" and self.variation > 0.0 and len(ended):
            self._redraw(ended, self.episodes[ended])
        if self.mutation != "countdown_after_decision":
            self.remaining[self.remaining > 0] -= 1  # 3.
        free = self.remaining == 0  # 4.
        start = free & ((r[0] >> np.uint32(8)).astype(np.int64) < self.threshold)  # (an integer compare; threshold 2^24: always)
        zero = free & ~start
        envs = np.flatnonzero(start)
        if len(envs):
            self.force[:, envs] = self.push(envs, self.pushes[envs])
            self.pushes[envs] += np.uint32(1)
            span = self.steps_max - self.steps_min + 1
            self.remaining[envs] = self.steps_min + ((r[3][envs] >> np.uint32(8)) % np.uint32(span)).astype(np.int32)
        self.force[:, zero] = 0.0
        if self.mutation == "countdown_after_decision":
            self.remaining[self.remaining > 0] -= 1
        return {"start": start, "hold": ~free, "zero": zero, "cut": cut, "redrawn": done.copy()}  # 5. hold: nothing written

    def snapshot(self):
        named = {"calls": self.calls, "remaining": self.remaining, "pushes": self.pushes, "episodes": self.episodes, "force": self.force,
                 "body_inertials": self.body_inertials, "link_scale": self.link_scale}
        return {k: v.copy() for k, v in named.items() if v is not None}


# ---- the inputs of the kernel-against-twin test (tests/test_episode_events_gpu.py), stated once for both test files
GPU_SETTINGS = dict(push_prob=0.25, push_norm=(5.0, 20.0), push_steps=(1, 3), inertia_variation=0.3)
GPU_SEED, GPU_CALLS = 11, 40
GPU_SIZES = tuple((n, 1000) for n in (1, 63, 64, 65, 257)) + ((64, 2 ** 32 - 16),)  # (num_envs, env_id_offset); the last: a carry into the high id word


def gpu_flags(num_envs: int, env_id_offset: int):
    """(terminated, truncated), each [GPU_CALLS, num_envs] uint8: an episode ends with probability 0.1 per env and call,
    by either flag."""
    rng = np.random.default_rng([num_envs, env_id_offset % 2 ** 32, 5])
    done = rng.random((GPU_CALLS, num_envs)) < 0.1
    by_limit = rng.random((GPU_CALLS, num_envs)) < 0.5
    return (done & ~by_limit).astype(np.uint8), (done & by_limit).astype(np.uint8)
