"""`upkie_amd.launch`: the one way into the HIP library. Without a GPU: a recording stand-in for the library function,
and `torch.cuda.current_device`, `torch.cuda.device`, `torch.cuda.current_stream` and the raw-stream getter replaced."""

import ctypes as C
import types

import pytest
import torch

from upkie_amd import abi, launch, lib
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.launch import device_tensor, launcher, ptr
from upkie_amd.sim import BatchedSim

RAW, OBJECT = 0x7000, 0x9000  # stream handles: what the raw getter / a `Stream` object's `cuda_stream` give for device 0


class Recorder:
    """Stands for a library function: records its arguments and the device current while it runs."""

    def __init__(self, cuda, status=0, error=None):
        self.cuda, self.status, self.error, self.calls = cuda, status, error, []

    def __call__(self, *args):
        self.calls.append((args, self.cuda.current))
        if self.error is not None:
            raise self.error
        return self.status


class FakeCuda:
    """`torch.cuda` as far as the launcher uses it: which device is current, the context manager that changes it, and
    the two ways to the current stream, each counting its uses."""

    def __init__(self, monkeypatch, current=0, raw=True):
        self.current, self.entered, self.left, self.streams_built, self.raw_calls = current, 0, 0, 0, 0
        fake = self

        class device:
            def __init__(self, dev):
                self.index = torch.device(dev).index

            def __enter__(self):
                fake.entered += 1
                self.previous, fake.current = fake.current, self.index

            def __exit__(self, *exc):
                fake.left += 1
                fake.current = self.previous
                return False

        def current_stream(dev):
            fake.streams_built += 1
            return types.SimpleNamespace(cuda_stream=OBJECT + torch.device(dev).index)

        def raw_stream(index):
            fake.raw_calls += 1
            return RAW + index

        monkeypatch.setattr(torch.cuda, "current_device", lambda: fake.current)
        monkeypatch.setattr(torch.cuda, "device", device)
        monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
        monkeypatch.setattr(launch, "_raw_stream", raw_stream if raw else None)


def test_ptr_is_a_plain_address_or_none():
    t = torch.zeros(3)
    assert ptr(t) == t.data_ptr() and type(ptr(t)) is int and ptr(None) is None


def test_device_tensor_passes_none_when_not_required_and_refuses_host_tensors():
    """What a host-only run reaches of `device_tensor` (the checks of a device tensor: tests/test_launch_gpu.py)."""
    dev = torch.device("cuda:0")
    assert device_tensor(None, "mask", dev, (8,), (torch.bool, torch.uint8), required=False) is None
    with pytest.raises(ValueError, match="^reward is required$"):
        device_tensor(None, "reward", dev, (8,))
    for host in (torch.zeros(8), [0.0] * 8):
        with pytest.raises(UpkieRuntimeError, match=r"^reward must be a device tensor \(there is no CPU fallback\)$"):
            device_tensor(host, "reward", dev, (8,), required=False)


def test_require_names_the_symbol_and_the_hint():
    library = types.SimpleNamespace(upkie_episodes_step=object())
    assert lib.require(library, "upkie_episodes_step") is None
    with pytest.raises(UpkieRuntimeError, match="^this build of libupkie_hip.so has no upkie_vecnorm_merge: rebuild it$"):
        lib.require(library, "upkie_vecnorm_merge")
    with pytest.raises(UpkieRuntimeError, match="^this build of libupkie_hip.so has no upkie_vecnorm_merge: rebuild it for a process group$"):
        lib.require(library, "upkie_vecnorm_merge", "for a process group")


def test_handle_first_stream_last_arguments_untouched(monkeypatch):
    cuda = FakeCuda(monkeypatch)
    fn, ref = Recorder(cuda), C.byref(C.c_int(3))
    launcher("cuda:0", "handle", lambda h: b"")(fn, 7, None, 2.5, ref)
    assert fn.calls == [(("handle", 7, None, 2.5, ref, RAW), 0)]
    launcher("cuda:0")(fn, 7, None)  # a handle-free entry point
    assert fn.calls[1] == ((7, None, RAW), 0)
    launcher("cuda:0", None, lambda h: b"")(fn)  # a handle family keeps its slot, whatever the handle
    assert fn.calls[2] == ((None, RAW), 0)


def test_fast_path_enters_no_context_and_builds_no_stream(monkeypatch):
    cuda = FakeCuda(monkeypatch, current=1)
    fn = Recorder(cuda)
    launcher("cuda:1")(fn, 5)
    assert fn.calls == [((5, RAW + 1), 1)]
    assert (cuda.entered, cuda.left, cuda.streams_built, cuda.raw_calls) == (0, 0, 0, 1)


def test_device_not_current_enters_and_leaves_the_context_once(monkeypatch):
    cuda = FakeCuda(monkeypatch, current=0)
    fn = Recorder(cuda)
    launcher("cuda:1")(fn, 5)
    assert fn.calls == [((5, OBJECT + 1), 1)]  # (the call ran with device 1 current, on device 1's stream)
    assert (cuda.entered, cuda.left, cuda.current) == (1, 1, 0)
    boom = Recorder(cuda, error=RuntimeError("from the library function"))
    with pytest.raises(RuntimeError, match="from the library function"):
        launcher("cuda:1")(boom)
    assert (cuda.entered, cuda.left, cuda.current) == (2, 2, 0)


def test_without_a_raw_stream_getter_the_stream_object_supplies_the_handle(monkeypatch):
    cuda = FakeCuda(monkeypatch, current=0, raw=False)
    fn = Recorder(cuda)
    launcher("cuda:0", "handle", lambda h: b"")(fn, 5)
    assert fn.calls == [(("handle", 5, OBJECT), 0)]
    assert (cuda.entered, cuda.left, cuda.streams_built) == (1, 1, 1)


def test_a_device_without_an_index_is_the_one_current_at_construction(monkeypatch):
    cuda = FakeCuda(monkeypatch, current=2)
    go = launcher("cuda")
    assert go.index == 2 and go.device == torch.device("cuda", 2)
    fn = Recorder(cuda)
    go(fn)
    assert fn.calls == [((RAW + 2,), 2)] and cuda.entered == 0
    cuda.current = 0  # another device has become current: the call still runs on device 2, on device 2's stream
    go(fn)
    assert fn.calls[1] == ((OBJECT + 2,), 2) and (cuda.entered, cuda.left, cuda.current) == (1, 1, 0)


@pytest.mark.parametrize("family", ["sim", "mpc", "observers", None])
def test_negative_status_raises_with_the_launchers_own_last_error(monkeypatch, family):
    cuda = FakeCuda(monkeypatch)
    asked = []

    def last_error_of(name):
        def last_error(handle):
            asked.append((name, handle))
            return f"{name} says no".encode()

        return last_error

    # (the handle-free entry points report through upkie_sim_last_error(NULL) of the loaded library)
    monkeypatch.setattr(lib, "load", lambda: types.SimpleNamespace(upkie_sim_last_error=last_error_of("handle-free")))
    go = launcher("cuda:0") if family is None else launcher("cuda:0", "handle", last_error_of(family))
    name, handle = ("handle-free", None) if family is None else (family, "handle")
    assert go(Recorder(cuda, status=0), 1) is None and go(Recorder(cuda, status=3), 1) is None and asked == []
    with pytest.raises(lib.UpkieHipError, match=f"upkie_hip status -1: {name} says no") as info:
        go(Recorder(cuda, status=-1), 1)
    assert info.value.status == -1 and asked == [(name, handle)]
    with pytest.raises(lib.UpkieHipError, match=f"status -2: {name} says no") as info:
        go.check(-2)  # (a status that came from no launch: a setter, a creator)
    assert info.value.status == -2
    go.check(0)
    if family is None:
        with pytest.raises(lib.UpkieHipError, match="status -5: handle-free says no"):
            launch.check(-5)
        launch.check(64)  # (a size)
    else:
        go.release()  # the handle is destroyed: the library gets NULL in its place
        fn = Recorder(cuda, status=-1)
        with pytest.raises(lib.UpkieHipError):
            go(fn, 1)
        assert fn.calls[0][0] == (None, 1, RAW) and asked[-1] == (family, None)


# ---- the per-step closures of BatchedSim: the launcher's call with the constant addresses fixed
ARGTYPES = {name: argtypes for name, _, argtypes, _ in lib._ABI}
ACT, OBS, REW, TERM, TRUNC = 101, 102, 103, 104, 105  # late arguments, told apart from any address


def _bare_sim(monkeypatch):
    """A `BatchedSim` without a device: host tensors for the buffers, recorders for the library's step functions."""
    cuda = FakeCuda(monkeypatch)
    sim = BatchedSim.__new__(BatchedSim)
    sim.num_envs, sim.device, sim._handle = 2, torch.device("cpu"), "handle"
    sim._lib = types.SimpleNamespace(**{name: Recorder(cuda) for name in ARGTYPES if name.startswith("upkie_sim_step_")})
    sim._launch = launcher("cuda:0", sim._handle, lambda h: b"")
    sim.state, sim.reward = torch.zeros((abi.STATE_WORDS, 2)), torch.zeros(2)
    sim.terminated, sim.truncated = torch.zeros(2, dtype=torch.uint8), torch.zeros(2, dtype=torch.uint8)
    sim.obs4, sim.obs6, sim.obs_servos = torch.zeros((2, 4)), torch.zeros((2, 6)), None
    return sim


def _only_call(sim, name):
    fn = getattr(sim._lib, name)
    assert len(fn.calls) == 1 and all(not other.calls for key, other in vars(sim._lib).items() if key != name)
    args = fn.calls[0][0]
    assert len(args) == len(ARGTYPES[name]) and args[0] == "handle" and args[-1] == RAW
    return args[1:-1]


@pytest.mark.parametrize("kind", ["pendulum", "gyropod", "servos", "pendulum_agent"])
def test_stepper_passes_the_action_address_in_the_library_functions_order(monkeypatch, kind):
    sim = _bare_sim(monkeypatch)
    step = sim.stepper(kind)
    obs = {"pendulum": sim.obs4, "gyropod": sim.obs6, "servos": sim.obs_servos, "pendulum_agent": sim.obs4}[kind]
    assert obs is not None and (kind != "servos" or obs.shape == (2, 6, 5))  # (allocated by the first need of it)
    outputs = (obs.data_ptr(), sim.reward.data_ptr(), sim.terminated.data_ptr(), sim.truncated.data_ptr())
    if kind == "pendulum_agent":
        assert step() is None
        assert _only_call(sim, "upkie_sim_step_pendulum_agent") == (sim.state.data_ptr(),) + outputs
    else:
        assert step(ACT) is None
        assert _only_call(sim, f"upkie_sim_step_{kind}") == (sim.state.data_ptr(), ACT) + outputs
    with pytest.raises(KeyError):
        sim.stepper("base_velocity")


@pytest.mark.parametrize("kind", ["pendulum", "gyropod", "servos", "servos_policy", "base_velocity"])
def test_step_into_fn_passes_the_output_addresses_in_the_library_functions_order(monkeypatch, kind):
    sim = _bare_sim(monkeypatch)
    state = sim.state.data_ptr()
    if kind == "servos_policy":
        policy = abi.UpkieServoPolicy()
        step = sim.step_into_fn(kind, policy=policy)
        assert step(ACT, OBS, REW, TERM, TRUNC) is None
        got = _only_call(sim, "upkie_sim_step_servos_policy")
        assert C.addressof(got[1]._obj) == C.addressof(policy)
        # (the caller's action address is ignored: the policy writes the handle's own action buffer)
        assert (got[0],) + got[2:] == (state, sim._policy_act.data_ptr(), OBS, REW, TERM, TRUNC) and sim._policy_act.shape == (2, 6, 6)
    elif kind == "base_velocity":
        mpc = types.SimpleNamespace(_handle="mpc handle", workspace=torch.zeros((8, 2)), commanded_velocity=torch.zeros(2))
        x0, contact = torch.zeros((2, 4)), torch.zeros(2, dtype=torch.uint8)
        step = sim.step_into_fn(kind, mpc=mpc, mpc_x0=x0, mpc_contact=contact)
        assert step(ACT, OBS, REW, TERM, TRUNC) is None
        assert _only_call(sim, "upkie_sim_step_base_velocity_mpc") == (
            "mpc handle", state, mpc.workspace.data_ptr(), ACT, mpc.commanded_velocity.data_ptr(), OBS, x0.data_ptr(), contact.data_ptr(),
            REW, TERM, TRUNC)
    else:
        step = sim.step_into_fn(kind)
        assert step(ACT, OBS, REW, TERM, TRUNC) is None
        assert _only_call(sim, f"upkie_sim_step_{kind}") == (state, ACT, OBS, REW, TERM, TRUNC)
    with pytest.raises(ValueError, match="unknown env kind"):
        sim.step_into_fn("pendulum_agent")


def test_scratch_buffers_are_allocated_once_under_their_attribute_names(monkeypatch):
    sim = _bare_sim(monkeypatch)
    assert sim.obs_servos is None and getattr(sim, "obs3", None) is None  # (what the vector envs read before the first use)
    obs3 = sim._scratch("obs3", (3,))
    assert obs3 is sim.obs3 and obs3.shape == (2, 3) and obs3.dtype is torch.float32 and sim._scratch("obs3", (3,)) is obs3
    assert sim._scratch("obs4", (4,)) is sim.obs4
