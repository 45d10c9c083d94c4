"""Which step kernel a step call launches (upkie_amd/csrc/step_dispatch.hpp::select_step_instance), without a GPU: the
selector, through tests/host_harness.hip, against a restatement of its rules over the whole grid of facts, and the
instantiations the simulator's unit references (its undefined launch stubs) against the instances the selector can
produce: what can be chosen, what is referenced and what step_instances.hpp declares are the same 140 kernels."""

import ctypes as C
import itertools
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_device_arithmetic_on_host import harness  # noqa: F401  (the fixture that builds the harness)
from upkie_amd import abi, lib

RESET, PENDULUM, AGENT, GYROPOD, SERVOS, BASE_VELOCITY, ROLLOUT = range(7)  # (step_kernels.hpp, StepMode)
MODES = (RESET, PENDULUM, AGENT, GYROPOD, SERVOS, BASE_VELOCITY, ROLLOUT)
NUM_ENVS = (64, 8192, 8193, 16384, 16385, 32768, 32769, 131071, 131072)
AUTORESET_DISABLED, AUTORESET_NEXT_STEP = 0, 1
FACTS = ("mode", "num_envs", "lanes_per_env", "spine", "manifold", "ext_on_leg_links", "randomized", "always_rand", "default_scalars",
         "final_obs_set", "autoreset_mode", "done_pass", "packed")
FIELDS = ("family", "rand", "waves", "spine", "bullet", "default_scalars", "in_place", "done_pass_follows", "refused")
BOTH = (0, 1)
GRID = list(itertools.product(MODES, NUM_ENVS, (0, 1, 2, 8), BOTH, BOTH, BOTH, BOTH, BOTH, BOTH, BOTH,
                              (AUTORESET_DISABLED, AUTORESET_NEXT_STEP), BOTH, (0, 1, 2)))


def expected(mode, num_envs, forced, spine, manifold, ext_on_leg_links, randomized, always_rand, default_scalars, final_obs_set,
             autoreset_mode, done_pass, packed):
    """The rules, as the project states them; the fields a family does not have stay at 1 wave / False."""
    eight_ok = not spine and num_envs * abi.STATE_WORDS * 4 < 2**32 and not ext_on_leg_links
    if forced in (1, 2, 8):
        if forced == 8 and not eight_ok:
            lanes = 1 if manifold else 2
        elif forced == 2 and manifold:
            lanes = 1
        else:
            lanes = forced
    elif num_envs <= 16384 and eight_ok:
        lanes = 8
    elif manifold:
        lanes = 1
    else:
        lanes = 2 if num_envs <= 32768 else 1
    if mode == SERVOS and lanes == 8 and forced != 8 and num_envs > 8192:
        lanes = 1 if manifold else 2
    same_step = (mode in (PENDULUM, GYROPOD, SERVOS) and not done_pass and packed != 1 and final_obs_set
                 and autoreset_mode == AUTORESET_DISABLED)
    in_kernel = same_step and lanes == 8
    k = dict(family=lanes, rand=randomized or (always_rand and lanes != 8), waves=1, spine=False, bullet=False, default_scalars=False,
             in_place=False, done_pass_follows=same_step and not in_kernel, refused=False)
    if lanes == 8:
        k.update(bullet=manifold, in_place=in_kernel, default_scalars=not manifold and default_scalars and mode in (PENDULUM, AGENT, ROLLOUT, GYROPOD))
    elif lanes == 2:
        k.update(spine=spine)
    elif mode == ROLLOUT:
        k.update(refused=True)
    elif manifold:
        k.update(bullet=True)
    else:
        k.update(waves=2 if num_envs >= 131072 else 1, spine=spine)
    return tuple(int(k[name]) for name in FIELDS)


@pytest.fixture(scope="module")
def chosen(harness):  # noqa: F811
    """What the selector answers over GRID, [len(GRID)][len(FIELDS)]."""
    facts = np.ascontiguousarray(GRID, dtype=np.int32)
    assert facts.shape == (len(GRID), len(FACTS))
    out = np.full((len(GRID), len(FIELDS)), -1, dtype=np.int32)
    harness.harness_select_step_instances.restype = None
    harness.harness_select_step_instances(C.c_int(len(GRID)), facts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def instances(rows):
    """The distinct kernels among (facts, result) rows, named as the demangled launch stubs are."""
    names = set()
    flag = ("false", "true")
    for facts, k in rows:
        family, rand, waves, spine, bullet, default_scalars, in_place, _, refused = (int(v) for v in k)
        if refused:
            continue
        mode = facts[0]
        if family == 8:
            names.add(f"step_kernel_octet<{mode}, {flag[rand]}, {flag[default_scalars]}, {flag[in_place]}, {flag[bullet]}>")
        elif family == 2:
            names.add(f"step_kernel_pair<{mode}, {flag[rand]}, {flag[spine]}>")
        else:
            names.add(f"step_kernel<{mode}, {flag[rand]}, {waves}, {flag[spine]}, {flag[bullet]}>")
    return names


def test_selector_is_the_stated_rules_over_the_whole_grid(chosen):
    wrong = [(dict(zip(FACTS, facts)), dict(zip(FIELDS, got.tolist())), dict(zip(FIELDS, expected(*facts))))
             for facts, got in zip(GRID, chosen) if tuple(got.tolist()) != expected(*facts)]
    assert not wrong, f"{len(wrong)} of {len(GRID)} choices differ, the first (facts, selector, rules): {wrong[0]}"


def test_referenced_kernels_are_the_instances_the_selector_can_choose(chosen, tmp_path):
    if shutil.which("hipcc") is None or shutil.which("nm") is None:
        pytest.skip("hipcc or nm not available")
    obj = str(tmp_path / "upkie_hip.o")
    subprocess.run(["hipcc"] + lib.HIPCC_FLAGS + ["-c", lib.SIM_ABI_SOURCE, "-o", obj], check=True, capture_output=True)
    symbols = subprocess.run(["nm", "-uC", obj], check=True, capture_output=True, text=True).stdout
    referenced = re.findall(r"__device_stub__(step_kernel\w*<[^>]*>)", symbols)
    assert len(referenced) == len(set(referenced)) == 140
    defined = subprocess.run(["nm", "-C", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    assert not re.findall(r"::(?:__device_stub__)?step_kernel\w*<", defined), "the simulator's unit compiles no step kernel of its own"
    can_be_chosen = instances(zip(GRID, chosen))
    assert can_be_chosen == set(referenced)
    # ... and step_instances.hpp declares them by the same rules (the restatement's instances, for the record of what differs)
    assert instances((facts, expected(*facts)) for facts in GRID) == set(referenced)
