"""`upkie_amd.launch` on the real runtime: every handle family and the handle-free entry points launch on torch's
CURRENT stream, i.e. the raw-stream getter gives what the `Stream` object's ``cuda_stream`` gives (tests/test_launch.py
cannot pin that without a device)."""

import pytest
import torch

from upkie_amd import abi, lib

B = 64  # one wavefront: the smallest launch these entry points have


@pytest.mark.gpu
def test_every_family_launches_on_torchs_current_stream(monkeypatch):
    from upkie_amd.episodes import EpisodeStatistics
    from upkie_amd.mpc import BatchedMpc
    from upkie_amd.observers import BatchedObservers
    from upkie_amd.policies import LinearPolicy
    from upkie_amd.sim import BatchedSim

    library = lib.load()
    streams = {}

    def record(name):
        real = getattr(library, name)

        def fn(*args):
            streams[name] = args[-1]
            return real(*args)

        monkeypatch.setattr(library, name, fn)

    sim = BatchedSim(abi.default_sim_config(B, seed=0))
    mpc = BatchedMpc(abi.default_mpc_config(B, 16))
    observers = BatchedObservers(abi.default_observer_config(B, 1e-3))
    policy = LinearPolicy([10.0, 1.0, 0.0, 0.1], clip=0.99)
    episodes = EpisodeStatistics(B)
    act = torch.zeros(B, dtype=torch.float32, device=sim.device)
    calls = {
        "upkie_sim_step_pendulum": lambda: sim.step_pendulum(act),
        "upkie_sim_reset": lambda: sim.reset(),  # (a method that used to hand-roll its launch)
        "upkie_mpc_reset": lambda: mpc.reset(),
        "upkie_observers_reset": lambda: observers.reset(),
        "upkie_linear_policy": lambda: policy(sim.obs4),
        "upkie_episodes_reset": lambda: episodes.reset(),
    }
    for name in calls:
        record(name)

    def launched_on():
        streams.clear()
        for call in calls.values():
            call()
        assert set(streams) == set(calls)
        return {name: int(stream or 0) for name, stream in streams.items()}

    default = torch.cuda.current_stream(sim.device)
    assert launched_on() == {name: default.cuda_stream for name in calls}
    side = torch.cuda.Stream(sim.device)
    assert side.cuda_stream != default.cuda_stream
    side.wait_stream(default)
    with torch.cuda.stream(side):
        assert launched_on() == {name: side.cuda_stream for name in calls}
    default.wait_stream(side)
    assert launched_on() == {name: default.cuda_stream for name in calls}
    torch.cuda.synchronize(sim.device)
    for handle in (sim, mpc, observers):
        handle.close()


@pytest.mark.gpu
def test_device_tensor_checks_device_dtype_size_and_layout():
    from upkie_amd.launch import device_tensor

    dev = torch.device("cuda", torch.cuda.current_device())
    good = torch.zeros(8, device=dev)
    assert device_tensor(good, "reward", dev, (8,)) is good and device_tensor(good, "obs", dev, (2, 4)) is good  # (the element count, not the shape)
    flags = torch.zeros(8, dtype=torch.uint8, device=dev)
    assert device_tensor(flags, "mask", dev, (8,), (torch.bool, torch.uint8), required=False) is flags
    wrong = {"dtype": torch.zeros(8, dtype=torch.float64, device=dev), "size": torch.zeros(9, device=dev),
             "layout": torch.zeros(8, 2, device=dev)[:, 0], "flag dtype": good}
    for what, t in wrong.items():
        dtypes = (torch.bool, torch.uint8) if what == "flag dtype" else (torch.float32,)
        with pytest.raises(ValueError, match="reward must be a contiguous") as info:
            device_tensor(t, "reward", dev, (8,), dtypes)
        assert str(info.value) == f"reward must be a contiguous [8] tensor of {' or '.join(map(str, dtypes))} on {dev}", what
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="reward must be a contiguous"):
            device_tensor(good, "reward", torch.device("cuda", (dev.index + 1) % torch.cuda.device_count()), (8,))
    with pytest.raises(ValueError, match="reward must be a contiguous"):
        device_tensor(good, "reward", torch.device("cpu"), (8,))  # (a stage on another device than the tensor)
