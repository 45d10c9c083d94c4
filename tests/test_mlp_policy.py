"""The MLP actor-critic policy (upkie_amd.policies.MlpActorCritic, csrc/policy_mlp.hpp) without a GPU: argument
checks, SB3 state-dict parsing, the weight packing (round trip, layout size, and the kernel's lane arithmetic emulated
on the packed buffer), the C struct against its ctypes mirror, the exported symbols, and the host twins the GPU tests
compare against (tests/test_mlp_policy_gpu.py)."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import mlp_reference as R
from tests.mlp_shapes import MATRIX
from tests.mlp_shapes import tower as _tower
from upkie_amd import abi, lib
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.policies import MlpActorCritic, MlpPolicy, mlp_shape, pack_index, sb3_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (obs_dim, actor widths, act_dim, critic widths, activation): the GPU tests' shapes and some edges
SHAPES = [
    (4, [64, 64], 1, [64, 64], "tanh"),
    (6, [64, 64], 2, [64, 64], "relu"),
    (30, [256, 256, 128], 36, [256, 256, 128], "tanh"),
    (3, [16], 2, [16], "relu"),
    (5, [7, 33, 20, 1], 17, [], "tanh"),
    (17, [48], 64, [3, 256, 5, 9], "relu"),
]
# and every row of the GPU shape matrix (tests/mlp_shapes.py) that is not above already
for _row in MATRIX:
    if (_row.obs_dim, _row.actor, _row.act_dim, _row.critic, _row.activation) not in SHAPES:
        SHAPES.append((_row.obs_dim, _row.actor, _row.act_dim, _row.critic, _row.activation))
SHAPE_IDS = [f"{s[0]}-{s[1]}-{s[2]}-{s[4]}" if s in SHAPES[:6] else f"{s[0]}-{s[1]}-{s[2]}-{s[3]}-{s[4]}".replace(" ", "") for s in SHAPES]


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


def _sources(shape, seed=0, normalize=False):
    """Random source vectors in `MlpActorCritic.sources()` order (flattened) for a shape."""
    rng = np.random.default_rng(seed)
    D, A = shape.obs_dim, shape.act_dim
    out = [rng.normal(size=D), np.sqrt(rng.uniform(0.5, 2.0, size=D)), -rng.uniform(0.5, 1.0, size=A), rng.uniform(0.5, 1.0, size=A),
           rng.normal(scale=0.3, size=A)]

    def tower(widths, d_out):
        n = D
        for w in list(widths) + [d_out]:
            out.extend([rng.normal(scale=1.0 / math.sqrt(n), size=w * n), rng.normal(scale=0.1, size=w)])
            n = w

    tower(list(shape.actor_widths[: shape.actor_layers]), A)
    if shape.critic_layers:
        tower(list(shape.critic_widths[: shape.critic_layers]), 1)
    return [o.astype(np.float32) for o in out]


def _shape(D, aw, A, cw, act, normalize=False):
    dims = lambda widths, out: [(w, n) for w, n in zip(list(widths) + [out], [D] + list(widths))]  # noqa: E731
    return mlp_shape(dims(aw, A), dims(cw, 1) if cw else [], act, normalize)


def test_shape_and_argument_checks():
    s = _shape(4, [64, 64], 1, [64, 64], "tanh")
    assert (s.obs_dim, s.act_dim, s.actor_layers, list(s.actor_widths), s.critic_layers) == (4, 1, 2, [64, 64, 0, 0], 2)
    with pytest.raises(ValueError, match="activation"):
        _shape(4, [8], 1, [], "gelu")
    with pytest.raises(ValueError, match="hidden layers"):
        _shape(4, [8] * 5, 1, [], "tanh")
    with pytest.raises(ValueError, match="hidden layers"):
        mlp_shape([(1, 4)], [], "tanh")  # a head and nothing else
    with pytest.raises(ValueError, match="widths"):
        _shape(4, [300], 1, [], "tanh")
    with pytest.raises(ValueError, match="act_dim"):
        _shape(4, [8], 65, [], "tanh")
    with pytest.raises(ValueError, match="obs_dim"):
        _shape(257, [8], 1, [], "tanh")
    with pytest.raises(ValueError, match="takes 5 inputs"):
        mlp_shape([(8, 4), (1, 5)], [], "tanh")
    with pytest.raises(ValueError, match="1 value"):
        mlp_shape([(8, 4), (1, 8)], [(8, 4), (2, 8)], "tanh")
    with pytest.raises(ValueError, match="Tanh or ReLU"):
        MlpActorCritic.from_modules(nn.Sequential(nn.Linear(4, 8), nn.Sigmoid(), nn.Linear(8, 1)), None, torch.zeros(1), -1, 1)
    with pytest.raises(ValueError, match="one activation"):
        MlpActorCritic.from_modules(nn.Sequential(nn.Linear(4, 8), nn.Tanh(), nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 1)), None,
                                    torch.zeros(1), -1, 1)
    # host tensors: refused, there is no CPU fallback
    with pytest.raises(UpkieRuntimeError, match="HIP device only"):
        MlpActorCritic.from_modules(_tower(4, [8], 1, "tanh"), _tower(4, [8], 1, "tanh"), torch.zeros(1), -1.0, 1.0)
    with pytest.raises(UpkieRuntimeError, match="HIP device only"):
        MlpPolicy.from_modules(_tower(4, [8], 1, "relu"), -1.0, 1.0)


def test_sb3_state_dict_loads_the_same_network():
    torch.manual_seed(0)
    actor_head = nn.Linear(64, 2)
    policy_net = nn.Sequential(nn.Linear(6, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh())
    value_net = nn.Sequential(nn.Linear(6, 32), nn.Tanh(), nn.Linear(32, 32), nn.Tanh())
    sd = {}
    for prefix, mod in (("mlp_extractor.policy_net.", policy_net), ("mlp_extractor.value_net.", value_net)):
        for k, v in mod.state_dict().items():
            sd[prefix + k] = v
    for k, v in actor_head.state_dict().items():
        sd["action_net." + k] = v
    value_head = nn.Linear(32, 1)
    for k, v in value_head.state_dict().items():
        sd["value_net." + k] = v
    sd["log_std"] = torch.full((2,), -0.5)
    aw, ab, cw, cb, log_std = sb3_parameters(sd)
    actor = nn.Sequential(*policy_net, actor_head)
    critic = nn.Sequential(*value_net, value_head)
    for got, mod in ((list(zip(aw, ab)), actor), (list(zip(cw, cb)), critic)):
        want = [(m.weight, m.bias) for m in mod if isinstance(m, nn.Linear)]
        assert len(got) == len(want)
        for (w, b), (w2, b2) in zip(got, want):
            assert torch.equal(w, w2) and torch.equal(b, b2)
    assert torch.equal(log_std, sd["log_std"])
    s = mlp_shape([tuple(w.shape) for w in aw], [tuple(w.shape) for w in cw], "tanh")
    assert (s.obs_dim, s.act_dim, s.actor_layers, list(s.actor_widths)[:2], s.critic_layers, list(s.critic_widths)[:2]) == (6, 2, 2, [64, 64], 2, [32, 32])
    x = torch.randn(5, 6)
    ref = R.forward(s, [np.zeros(6), np.ones(6), -np.ones(2), np.ones(2), log_std] + [t.detach().numpy() for p in zip(aw + cw, ab + cb) for t in p], x.numpy())
    with torch.no_grad():
        assert np.allclose(ref[1], actor(x).double().numpy(), atol=1e-5)
        assert np.allclose(ref[2], critic(x)[:, 0].double().numpy(), atol=1e-5)
    with pytest.raises(ValueError, match="shared"):
        sb3_parameters(dict(sd, **{"mlp_extractor.shared_net.0.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="log_std"):
        sb3_parameters({k: v for k, v in sd.items() if k != "log_std"})


@pytest.mark.parametrize("spec", SHAPES, ids=SHAPE_IDS)
def test_pack_unpack_round_trip_and_layout_size(spec, library):
    shape = _shape(*spec)
    sources = _sources(shape)
    index = pack_index(shape, [s.size for s in sources])
    assert index.size == library.upkie_mlp_packed_words(C.byref(shape)) == R._layout(shape)["words"]
    assert index.size % 4 == 0
    flat = np.concatenate(sources + [np.zeros(1, np.float32)])
    packed = flat[index]
    used = index[index < flat.size - 1]
    assert np.array_equal(np.sort(used), np.arange(flat.size - 1)), "every source word packed exactly once"
    back = np.zeros_like(flat)
    back[index] = packed
    assert back[:-1].tobytes() == flat[:-1].tobytes()  # bit for bit


@pytest.mark.parametrize("spec", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("normalize", [False, True])
def test_kernel_lane_arithmetic_on_the_packed_buffer_is_the_network(spec, normalize):
    """The packing read through the kernel's MFMA fragment maps (emulated in fp64) computes the network."""
    shape = _shape(*spec, normalize=normalize)
    sources = _sources(shape, seed=1)
    index = pack_index(shape, [s.size for s in sources])
    packed = np.concatenate(sources + [np.zeros(1, np.float32)])[index]
    obs = np.random.default_rng(2).normal(size=(21, shape.obs_dim))  # (21: a partial second tile of 16 envs)
    x, mean, value = R.forward(shape, sources, obs)
    emu_mean, emu_value = R.emulate_packed(shape, packed, obs)
    assert np.allclose(emu_mean, mean, atol=1e-9, rtol=1e-9)
    if value is None:
        assert emu_value is None
    else:
        assert np.allclose(emu_value, value, atol=1e-9, rtol=1e-9)


def test_shape_struct_matches_ctypes():
    probe = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "upkie_hip.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\n", sizeof(UpkieMlpShape), offsetof(UpkieMlpShape, obs_dim),
             offsetof(UpkieMlpShape, act_dim), offsetof(UpkieMlpShape, activation), offsetof(UpkieMlpShape, actor_layers),
             offsetof(UpkieMlpShape, actor_widths), offsetof(UpkieMlpShape, critic_layers), offsetof(UpkieMlpShape, critic_widths),
             offsetof(UpkieMlpShape, normalize), offsetof(UpkieMlpShape, clip_obs), UPKIE_MLP_MAX_LAYERS, UPKIE_MLP_TANH, UPKIE_MLP_RELU,
             UPKIE_STRUCT_MLP_SHAPE);
      return 0;
    }
    """
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    S = abi.UpkieMlpShape
    want = [C.sizeof(S)] + [getattr(S, f).offset for f in ("obs_dim", "act_dim", "activation", "actor_layers", "actor_widths", "critic_layers",
                                                           "critic_widths", "normalize", "clip_obs")]
    assert got == want + [abi.MLP_MAX_LAYERS, abi.MLP_TANH, abi.MLP_RELU, [k for k, v in abi.STRUCT_IDS.items() if v is S][0]]


def test_library_exports_the_policy_and_checks_shapes_without_a_gpu(library):
    for name in ("upkie_mlp_packed_words", "upkie_mlp_actor_critic"):
        assert name in lib.EXPORTED_SYMBOLS and getattr(library, name) is not None
    assert library.upkie_hip_struct_bytes(9) == C.sizeof(abi.UpkieMlpShape)
    bad = _shape(4, [64], 1, [], "tanh")
    bad.actor_widths[0] = 0
    assert library.upkie_mlp_packed_words(C.byref(bad)) < 0
    assert b"out of range" in library.upkie_sim_last_error(None)
    good = _shape(4, [64], 1, [], "tanh")
    out = (C.c_float * 4)()
    status = library.upkie_mlp_actor_critic(0, C.byref(good), out, out, None, 0, 1, None, None, out, None, None, None, None)
    assert status == abi.ERR_INVALID_ARGUMENT
    status = library.upkie_mlp_actor_critic(16, C.byref(good), out, out, None, 0, 0, None, None, out, None, None, None, None)
    assert status == abi.ERR_INVALID_ARGUMENT and b"counters" in library.upkie_sim_last_error(None)  # sampling without counters
    status = library.upkie_mlp_actor_critic(16, C.byref(good), out, out, None, 0, 1, None, None, None, None, out, None, None)
    assert status == abi.ERR_INVALID_ARGUMENT and b"critic" in library.upkie_sim_last_error(None)  # a value without a critic


def test_a_library_built_before_the_mlp_policy_still_loads():
    """A build of the library from before the MLP policy (an A/B build loaded through UPKIE_HIP_LIBRARY) answers -1 for
    UpkieMlpShape and lacks its entry points: the struct check accepts it. A build that exports the entry points must
    report the struct's size."""
    sizes = {which: C.sizeof(cls) for which, cls in abi.STRUCT_IDS.items()}
    cases = "".join(f"    case {w}: return {n};\n" for w, n in sizes.items() if w not in abi.OPTIONAL_STRUCTS)
    stub = "#include <stdint.h>\nint64_t upkie_hip_struct_bytes(int which) {\n  switch (which) {\n" + cases + "    default: return -1;\n  }\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        for exports_entry in (False, True):
            src, so = os.path.join(tmp, f"stub{int(exports_entry)}.c"), os.path.join(tmp, f"libstub{int(exports_entry)}.so")
            with open(src, "w") as f:
                f.write(stub + ("int upkie_mlp_actor_critic(void) { return -1; }\n" if exports_entry else ""))
            subprocess.run(["gcc", "-shared", "-fPIC", src, "-o", so], check=True)
            older = C.CDLL(so)
            if exports_entry:
                with pytest.raises(UpkieRuntimeError, match="UpkieMlpShape"):
                    lib._check_struct_sizes(older)
            else:
                lib._check_struct_sizes(older)  # accepted


def test_fp64_reference_log_prob_is_torch_normal():
    rng = np.random.default_rng(3)
    mean, log_std = rng.normal(size=(50, 6)), rng.normal(scale=0.5, size=6)
    action = mean + np.exp(log_std) * rng.normal(size=(50, 6))
    want = torch.distributions.Normal(torch.as_tensor(mean), torch.as_tensor(np.exp(log_std))).log_prob(torch.as_tensor(action)).sum(-1)
    assert np.allclose(R.log_prob(action, mean, log_std), want.numpy(), atol=1e-12, rtol=1e-12)


def test_philox_twin_is_well_defined():
    # Philox4x32-10 known-answer vector (Salmon et al. 2011, Random123 kat_vectors): counter 0, key 0
    assert R.O.philox([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    z = R.philox_normals(8, 6, 0, seed=7)
    assert np.all(np.isfinite(z)) and np.array_equal(z, R.philox_normals(8, 6, 0, seed=7))
    assert not np.array_equal(z, R.philox_normals(8, 6, 1, seed=7))  # another call: other draws
    assert not np.array_equal(z, R.philox_normals(8, 6, 0, seed=8))
    assert len(np.unique(z)) == z.size
    # actions 4b..4b+3 share block b: two Box-Muller pairs of one radius each
    r01 = np.hypot(z[:, 0], z[:, 1])
    r23 = np.hypot(z[:, 2], z[:, 3])
    assert not np.allclose(r01, r23)
    # u1 = 0 cannot occur: the smallest u1 is 2^-24, a finite radius
    assert math.isfinite(math.sqrt(-2.0 * math.log(1.0 / 16777216.0)))
    # moments over many draws
    many = R.philox_normals(2000, 4, 3, seed=11).reshape(-1)
    assert abs(many.mean()) < 5 / math.sqrt(many.size) and abs(many.var() - 1.0) < 5 * math.sqrt(2.0 / many.size)
