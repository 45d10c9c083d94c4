"""The reward terms without a device: the host twin against a plain per-env loop, the host-side validation (Python and
``upkie_reward_terms_params``), the symbols, the example's term list, and that the scripted cases of
tests/reward_terms_cases.py are sharp: every mutation of the twin moves a term value by more than twice the bound the
GPU test allows the device (so, whatever the device's rounding, a mutated twin's ratio there is above 1), and the exp
shapes stay far from underflow."""

import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from tests import reward_terms_cases as CASES
from tests.reward_terms_reference import MUTATIONS, Twin, float32_reward
from upkie_amd import abi, lib
from upkie_amd import rewards as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("upkie_reward_terms_params", "upkie_reward_terms_step", "upkie_reward_terms_reset")


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


# ---------------------------------------------------------------- the twin against a plain loop
def _loop_values(D, A, dt, terms, next_obs, action, terminated, truncated, final_obs, prev):
    """Section 1 of the header, one env and one tap at a time with `math`."""
    inv_dt = float(np.float32(1.0 / dt))
    N = next_obs.shape[0]
    out = np.zeros((len(terms), N))
    for e in range(N):
        ended = bool(terminated[e]) or bool(truncated[e])
        o = final_obs[e] if ended else next_obs[e]
        for k, (_, term) in enumerate(terms):
            x = 0.0
            for tap in term.taps:
                if tap.source == abi.REWARD_OBS:
                    s = float(o[tap.index])
                elif tap.source == abi.REWARD_ACTION:
                    s = float(action[e][tap.index])
                elif tap.source == abi.REWARD_ACTION_RATE:
                    s = (float(action[e][tap.index]) - float(prev[tap.index][e])) * inv_dt
                elif tap.source == abi.REWARD_ONE:
                    s = 1.0
                else:
                    s = 1.0 if terminated[e] else 0.0
                s = math.sin(s) if tap.fn == abi.REWARD_FN_SIN else math.cos(s) if tap.fn == abi.REWARD_FN_COS else s
                x = float(np.float32(tap.coef)) * s + x
            scale = None if term.scale is None else float(np.float32(term.scale))
            y = {"identity": lambda: x, "abs": lambda: abs(x), "square": lambda: x * x, "exp_abs": lambda: math.exp(-abs(x) / scale),
                 "exp_square": lambda: math.exp(-((x / scale) ** 2)), "deadband": lambda: max(abs(x) - scale, 0.0)}[term.shape]()
            out[k, e] = float(np.float32(term.weight)) * y
    return out


@pytest.mark.parametrize("size", CASES.SIZES)
def test_twin_matches_a_plain_loop(size):
    D, A, K = size
    N = 5
    terms = CASES.terms_for(D, A, K)
    next_obs, final_obs, action, terminated, truncated = CASES.inputs(N, D, A)
    twin = Twin(N, D, A, CASES.DT, terms, clip=CASES.CLIP)
    sums, last, finished = np.zeros((K, N)), np.zeros((K, N)), np.zeros(N, dtype=np.int32)
    for t in range(CASES.STEPS):
        prev = twin.prev_action.copy()
        expected = _loop_values(D, A, CASES.DT, terms, next_obs[t], action[t], terminated[t], truncated[t], final_obs[t], prev)
        reward, v, bound = twin.step(next_obs[t], action[t], terminated[t], truncated[t], final_obs[t])
        np.testing.assert_allclose(v, expected, rtol=1e-13, atol=1e-15)
        assert np.all(bound > 0) and np.all(bound < 1e-2)
        total = np.zeros(N)
        for k in range(K):
            total = total + v[k]
        np.testing.assert_array_equal(reward, np.clip(total, np.float32(CASES.CLIP[0]), np.float32(CASES.CLIP[1])))
        ended = (terminated[t] | truncated[t]).astype(bool)
        for e in range(N):
            for k in range(K):
                sums[k, e] += v[k, e]
                if ended[e]:
                    last[k, e], sums[k, e] = sums[k, e], 0.0
            finished[e] += int(ended[e])
        np.testing.assert_array_equal(twin.term_sum, sums)
        np.testing.assert_array_equal(twin.term_last, last)
        np.testing.assert_array_equal(twin.finished, finished)
        np.testing.assert_array_equal(twin.prev_action, np.where(ended[None, :], np.float32(0), action[t].T))
    mask = np.arange(N) % 2 == 0
    before = twin.term_sum.copy(), twin.prev_action.copy(), twin.term_last.copy()
    twin.reset(mask)
    assert not twin.term_sum[:, mask].any() and not twin.prev_action[:, mask].any()
    np.testing.assert_array_equal(twin.term_sum[:, ~mask], before[0][:, ~mask])
    np.testing.assert_array_equal(twin.prev_action[:, ~mask], before[1][:, ~mask])
    np.testing.assert_array_equal(twin.term_last, before[2])


def test_float32_reward_rounds_every_addition():
    v = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], dtype=np.float32)
    assert float32_reward(v)[0] == np.float32(1.0)  # (each half-ulp addend is rounded away; an exact sum would be 1 + 2^-23)
    assert float32_reward(np.array([[2.0], [-5.0]], dtype=np.float32), clip=(-0.5, 0.5))[0] == np.float32(-0.5)
    assert np.isnan(float32_reward(np.array([[np.nan]], dtype=np.float32), clip=(-0.5, 0.5))[0])


# ---------------------------------------------------------------- the scripted cases are sharp
@pytest.mark.parametrize("size", CASES.SIZES)
@pytest.mark.parametrize("N", (1, 65))
def test_every_mutation_moves_a_term_beyond_twice_the_bound(N, size):
    D, A, K = size
    data = CASES.inputs(N, D, A)
    true_values, twin = CASES.twin_values(N, D, A, K)
    assert twin.max_exp_argument <= 8.0, twin.max_exp_argument
    assert CASES.worst_ratio(Twin(N, D, A, CASES.DT, CASES.terms_for(D, A, K), clip=CASES.CLIP), data, true_values) == 0.0
    for mutation in MUTATIONS:
        mutated = Twin(N, D, A, CASES.DT, CASES.terms_for(D, A, K), clip=CASES.CLIP, mutation=mutation)
        ratio = CASES.worst_ratio(mutated, data, true_values)
        print(f"N {N} (D, A, K) {size} {mutation}: worst |v - mutated v| / bound {ratio:.3g}")
        assert ratio > 2.0, (mutation, ratio)


def test_the_scripted_tables_cover_every_shape_function_and_source():
    for D, A, K in CASES.SIZES:
        terms = CASES.terms_for(D, A, K)
        assert len(terms) == K and any(t.source == abi.REWARD_OBS and t.index == D - 1 for _, term in terms for t in term.taps)
    terms = CASES.terms_for(256, 64, 16)
    assert {term.shape for _, term in terms} == set(R.SHAPES)
    assert {t.fn for _, term in terms for t in term.taps} == {0, 1, 2}
    assert {t.source for _, term in terms for t in term.taps} == {0, 1, 2, 3, 4}
    assert max(len(term.taps) for _, term in terms) == abi.REWARD_MAX_TAPS
    for N in CASES.N_VALUES:
        next_obs, final_obs, _, terminated, truncated = CASES.inputs(N, 4, 1)
        assert np.all(next_obs != final_obs)
        ended = terminated | truncated
        assert [int(ended[t].sum()) for t in range(6)] == [0, 1, 1, N, 1, 0]
        assert terminated[1, 0] and truncated[2, N - 1] and terminated[4, N // 2] and truncated[4, N // 2]


# ---------------------------------------------------------------- validation
def test_python_validation_messages():
    ok = {"a": R.Term(1.0, taps=[R.obs(0)])}
    assert len(R.pack_terms(4, 1, 0.005, ok)) == abi.REWARD_PARAMS_BYTES
    cases = [
        (dict(obs_dim=0), "obs_dim must be in 1-256"),
        (dict(obs_dim=257), "obs_dim must be in 1-256"),
        (dict(act_dim=65), "act_dim must be in 1-64"),
        (dict(dt=0.0), "dt must be positive"),
        (dict(terms={}), "1-16 terms"),
        (dict(terms={f"t{k}": R.Term(1.0, taps=[R.one()]) for k in range(17)}), "1-16 terms"),
        (dict(terms={"a": R.Term(1.0, taps=[])}), "1-8 taps"),
        (dict(terms={"a": R.Term(1.0, taps=[R.one()] * 9)}), "1-8 taps"),
        (dict(terms={"a": R.Term(1.0, taps=[R.obs(4)])}), r"obs\(4\) is beyond the observation's 4 words"),
        (dict(terms={"a": R.Term(1.0, taps=[R.act(1)])}), "action word 1 is beyond the action's 1 words"),
        (dict(terms={"a": R.Term(1.0, taps=[R.act_rate(-1)])}), "beyond the action's"),
        (dict(terms={"a": R.Term(1.0, "exp_abs", taps=[R.obs(0)])}), "needs a positive, finite scale"),
        (dict(terms={"a": R.Term(1.0, "deadband", scale=0.0, taps=[R.obs(0)])}), "needs a positive, finite scale"),
        (dict(terms={"a": R.Term(1.0, "exp_square", scale=-1.0, taps=[R.obs(0)])}), "needs a positive, finite scale"),
        (dict(terms={"a": R.Term(float("nan"), taps=[R.obs(0)])}), "weight must be finite"),
        (dict(terms={"a": R.Term(float("inf"), taps=[R.obs(0)])}), "weight must be finite"),
        (dict(terms={"a": R.Term(1.0, taps=[R.obs(0, float("inf"))])}), "coefficients must be finite"),
        (dict(terms={"a": R.Term(1.0, "cube", taps=[R.obs(0)])}), "shape must be one of"),
        (dict(terms=[("a", R.Term(1.0, taps=[R.one()])), ("a", R.Term(2.0, taps=[R.one()]))]), "duplicate term name 'a'"),
        (dict(clip=(1.0, -1.0)), "clip needs low <= high"),
    ]
    for change, message in cases:
        kw = dict(obs_dim=4, act_dim=1, dt=0.005, terms=ok, clip=None)
        kw.update(change)
        with pytest.raises(ValueError, match=message):
            R.pack_terms(**kw)
    with pytest.raises(ValueError, match="fn is None, 'sin' or 'cos'"):
        R.obs(0, fn="tan")
    with pytest.raises(ValueError, match="num_envs must be positive"):
        R.RewardTerms(0, 4, 1, 0.005, ok)


def test_host_tensors_and_a_host_device_are_refused():
    from upkie_amd.exceptions import UpkieRuntimeError

    with pytest.raises(UpkieRuntimeError, match="no CPU fallback"):
        R.RewardTerms(8, 4, 1, 0.005, {"a": R.Term(1.0, taps=[R.obs(0)])}, device="cpu")


def test_a_build_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    from upkie_amd.exceptions import UpkieRuntimeError

    class Old:
        pass

    monkeypatch.setattr(lib, "load", lambda: Old())
    with pytest.raises(UpkieRuntimeError, match="rebuild"):
        R.RewardTerms(8, 4, 1, 0.005, {"a": R.Term(1.0, taps=[R.obs(0)])}, device="cuda:0")


def test_symbols_are_declared_listed_and_exported(library):
    with open(os.path.join(ROOT, "include", "upkie_hip.h")) as f:
        declared = set(re.findall(r"\b(upkie_[a-z_]+)\s*\(", f.read()))
    for name in SYMBOLS:
        assert name in declared and name in lib.EXPORTED_SYMBOLS
        assert getattr(library, name) is not None
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(name in text for name in SYMBOLS)
    with open(os.path.join(ROOT, "include", "upkie_hip.h")) as f:
        text = f.read()
    for prefix, names in (("UPKIE_REWARD_", ("OBS", "ACTION", "ACTION_RATE", "ONE", "TERMINATED", "IDENTITY", "ABS", "SQUARE", "EXP_ABS", "EXP_SQUARE",
                                               "DEADBAND", "FN_ID", "FN_SIN", "FN_COS")),):
        for name in names:
            value = int(re.search(rf"\b{prefix}{name} = (\d+)", text).group(1))
            assert value == getattr(abi, f"REWARD_{name}"), name
    for name in ("MAX_TERMS", "MAX_TAPS", "PARAMS_BYTES"):
        assert int(re.search(rf"#define UPKIE_REWARD_{name} (\d+)", text).group(1)) == getattr(abi, f"REWARD_{name}")


def _params(library, D=4, A=1, dt=0.005, shapes=(0,), weights=(1.0,), scales=(1.0,), counts=(1,), sources=(0,), indices=(0,), fns=(0,),
            coefs=(1.0,), low=-math.inf, high=math.inf, out=None):
    ints = lambda v: (C.c_int32 * len(v))(*v)  # noqa: E731
    floats = lambda v: (C.c_float * len(v))(*v)  # noqa: E731
    status = library.upkie_reward_terms_params(D, A, len(shapes), dt, ints(shapes), floats(weights), floats(scales), ints(counts), ints(sources),
                                               ints(indices), ints(fns), floats(coefs), low, high, out)
    return int(status), (library.upkie_sim_last_error(None) or b"").decode()


def test_params_accepts_and_refuses_on_the_host(library):
    out = C.create_string_buffer(abi.REWARD_PARAMS_BYTES)
    assert _params(library)[0] == abi.REWARD_PARAMS_BYTES  # (params NULL: check only)
    assert _params(library, dt=0.25, shapes=(3, 0), weights=(2.0, -1.0), scales=(0.5, 0.0), counts=(2, 1), sources=(0, 2, 4), indices=(3, 0, 9),
                   fns=(1, 0, 2), coefs=(0.5, -0.25, 1.0), low=-1.0, high=2.0, out=out)[0] == abi.REWARD_PARAMS_BYTES
    words = np.frombuffer(out.raw, dtype=np.int32)
    floats = np.frombuffer(out.raw, dtype=np.float32)
    assert list(words[1:4]) == [2, 4, 1] and list(floats[4:7]) == [4.0, -1.0, 2.0]  # K, D, A; 1 / dt, the clamp
    term0, term1 = 8, 8 + 36
    assert list(words[term0:term0 + 2]) == [3, 2] and list(floats[term0 + 2:term0 + 4]) == [2.0, 0.5]
    assert list(words[term0 + 4:term0 + 7]) == [0, 3, 1] and floats[term0 + 7] == 0.5
    assert list(words[term0 + 8:term0 + 11]) == [2, 0, 0] and floats[term0 + 11] == -0.25
    assert list(words[term1:term1 + 2]) == [0, 1] and list(words[term1 + 4:term1 + 7]) == [4, 0, 2]  # (the index of a flag tap is ignored)
    refused = [
        (dict(D=0), "obs_dim must be in 1-256"),
        (dict(A=65), "act_dim in 1-64"),
        (dict(shapes=(), weights=(), scales=(), counts=()), "num_terms in 1-16"),
        (dict(dt=0.0), "dt must be positive"),
        (dict(dt=float("nan")), "dt must be positive"),
        (dict(shapes=(6,)), "unknown shape"),
        (dict(counts=(0,)), "1-8 taps"),
        (dict(counts=(9,)), "1-8 taps"),
        (dict(weights=(float("inf"),)), "weight must be finite"),
        (dict(shapes=(3,), scales=(0.0,)), "positive, finite scale"),
        (dict(shapes=(5,), scales=(float("nan"),)), "positive, finite scale"),
        (dict(sources=(5,)), "unknown tap source"),
        (dict(fns=(3,)), "unknown tap function"),
        (dict(coefs=(float("nan"),)), "coefficients must be finite"),
        (dict(indices=(4,)), "tap index 4 is beyond the observation's 4 words"),
        (dict(sources=(1,), indices=(1,)), "beyond the action's 1 words"),
        (dict(sources=(2,), indices=(-1,)), "beyond the action's 1 words"),
        (dict(low=1.0, high=0.0), "clip_low <= clip_high"),
        (dict(low=float("nan")), "clip_low <= clip_high"),
    ]
    for change, message in refused:
        status, error = _params(library, **change)
        assert status == abi.ERR_INVALID_ARGUMENT and message in error, (change, error)


def test_step_and_reset_check_their_arguments_before_the_device(library):
    """Wrong arguments are reported as such on a machine without a GPU too."""
    # N, D, A, K, params, next_obs, action, terminated, truncated, final_obs, prev_action, term_sum, term_last, finished, reward, stream
    args = [8, 4, 1, 1, 1, 1, 1, None, None, None, 1, 1, 1, 1, 1, None]  # (non-null dummies: refused before anything is read)
    for (at, value), message in (((0, 0), "num_envs must be positive"), ((1, 257), "obs_dim must be in 1-256"), ((3, 17), "num_terms in 1-16"),
                                 ((4, None), "null argument"), ((14, None), "null argument")):
        bad = list(args)
        bad[at] = value
        assert library.upkie_reward_terms_step(*bad) == abi.ERR_INVALID_ARGUMENT
        assert message in library.upkie_sim_last_error(None).decode()
    assert library.upkie_reward_terms_reset(8, 65, 1, None, 1, 1, None) == abi.ERR_INVALID_ARGUMENT
    assert library.upkie_reward_terms_reset(8, 1, 1, None, None, 1, None) == abi.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the example
def test_the_examples_terms_reproduce_its_former_reward():
    """examples/ppo_learn_reward_terms.py's alive, upright and in_place terms are ppo_learn_pipeline.py's ``1 - |pitch| -
    |position| / 4`` on envs that did not end, to fp64 rounding; its two new terms are the rate and the fall penalty."""
    spec = importlib.util.spec_from_file_location("ppo_learn_reward_terms", os.path.join(ROOT, "examples", "ppo_learn_reward_terms.py"))
    import sys

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))
    terms = module.terms()
    assert list(terms) == ["alive", "upright", "in_place", "action_rate", "fall"]
    N = 64
    rng = np.random.default_rng(0)
    obs = rng.uniform(-1.0, 1.0, (N, 4)).astype(np.float32)
    action = rng.uniform(-1.0, 1.0, (N, 1)).astype(np.float32)
    twin = Twin(N, 4, 1, 1.0 / 200.0, terms)
    twin.prev_action[:] = action.T
    v, _ = twin.values(obs, action, np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8), final_obs=obs + 1)
    former = 1.0 - np.abs(obs[:, 0].astype(np.float64)) - 0.25 * np.abs(obs[:, 1].astype(np.float64))
    np.testing.assert_allclose(v[0] + v[1] + v[2], former, rtol=0, atol=4 * np.finfo(np.float64).eps)
    assert not v[3].any() and not v[4].any()  # (a constant command, nobody fell)
    fallen = np.zeros(N, dtype=np.uint8)
    fallen[3] = 1
    moved = (action + np.float32(0.01)).astype(np.float32)
    v, _ = twin.values(obs, moved, fallen, None, final_obs=obs)
    assert v[4][3] == -10.0 and not np.delete(v[4], 3).any()
    np.testing.assert_allclose(v[3], float(np.float32(-0.01)) * ((moved.astype(np.float64) - action.astype(np.float64))[:, 0] * 200.0) ** 2, rtol=1e-12)
    R.pack_terms(4, 1, 1.0 / 200.0, terms)
