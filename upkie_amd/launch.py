"""The one way into the HIP library: "make the device current, fetch torch's current stream, call, check the
status", stated once. Every module of the package that launches a kernel holds the `launcher` of its device (and
handle) and calls the library through it; `ptr` is how a tensor becomes an argument."""

from typing import Optional

import torch

from . import lib
from .exceptions import UpkieRuntimeError

# the raw handle of torch's current stream on a device without building a torch.cuda.Stream object per call
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def ptr(t: Optional[torch.Tensor]):
    # (a plain integer: ctypes turns it into the c_void_p the argtypes ask for, without an object per argument)
    return t.data_ptr() if t is not None else None


def device_tensor(t, what: str, device, shape, dtypes=(torch.float32,), required: bool = True):
    """`t` as an argument of a launch: a contiguous tensor of ``shape``'s element count and one of ``dtypes`` on
    ``device``, returned as it is; None passes when not ``required``. ``what`` names it in the messages."""
    if t is None:
        if required:
            raise ValueError(f"{what} is required")
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise UpkieRuntimeError(f"{what} must be a device tensor (there is no CPU fallback)")
    n = 1
    for s in shape:
        n *= s
    if t.device != device or t.dtype not in dtypes or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"{what} must be a contiguous {list(shape)} tensor of {' or '.join(map(str, dtypes))} on {device}")
    return t


def end_flags(terminated, truncated, device, num_envs: int):
    """``(terminated, truncated)`` of an env step as arguments of a launch: each [num_envs] bool or uint8, or None."""
    flags = (torch.bool, torch.uint8)
    return (device_tensor(terminated, "terminated", device, (num_envs,), flags, required=False),
            device_tensor(truncated, "truncated", device, (num_envs,), flags, required=False))


def check(status: int, last_error=None, handle=None) -> None:
    """Raise `UpkieHipError` on a negative status, also of a call that is no launch (a setter, a creator, a size), with
    the message of ``last_error(handle)``: a handle family's ``upkie_*_last_error``, or ``upkie_sim_last_error(NULL)``
    for the handle-free entry points."""
    if status >= 0:
        return
    msg = (last_error or lib.load().upkie_sim_last_error)(handle)
    raise lib.UpkieHipError(status, msg.decode() if msg else "")


def launcher(device, handle=None, last_error=None):
    """The way into the library for one device: returns ``launch``, and ``launch(fn, *args)`` runs ``fn(*args, stream)``
    with torch's current stream on that device and raises `UpkieHipError` on a negative status. Given ``last_error``
    (the ``upkie_*_last_error`` of a handle family: sim, mpc, observers) it is bound to ``handle``: it runs
    ``fn(handle, *args, stream)`` and reads the message from that handle. Without, the entry points are the handle-free
    ones, whose message is ``upkie_sim_last_error(NULL)``. ``launch.check(status)`` is `check` with the same message
    source, for calls that are no launch; ``launch.release()`` forgets a destroyed handle: later calls hand the library
    NULL, which it refuses. ``launch.device`` and ``launch.index`` say where it launches.

    A Python-level RL loop pays this once or more per `env.step()`: no device context manager when the device is
    already current, no stream object (11.3 -> 7.9 us of CPU per step, profiles/r02_vec_env_python_loop.txt). It is a
    closure over its few constants, so that the call reads cells and no attributes. `BatchedSim.step_into_fn` and the
    agent's `stepper` are this call with its constant arguments fixed by ``functools.partial`` or a lambda; a lambda
    costs `env.step()` one more frame, so the action-taking `stepper` alone keeps the fast path written out, with
    ``launch.index`` and ``launch.raw_stream``. A device given without an index
    ("cuda") is the one current at construction, from then on."""
    device = torch.device(device)
    index = device.index
    if index is None and device.type == "cuda":
        index = torch.cuda.current_device()
        device = torch.device("cuda", index)
    head = [] if last_error is None else [handle]
    current_device, raw_stream = torch.cuda.current_device, _raw_stream

    def launch(fn, *args) -> None:
        if raw_stream is not None and current_device() == index:
            status = fn(*head, *args, raw_stream(index))
        else:
            with torch.cuda.device(device):
                status = fn(*head, *args, torch.cuda.current_stream(device).cuda_stream)
        if status < 0:
            check(status, last_error, *head)

    def release() -> None:
        head[0] = None

    launch.check = lambda status: check(status, last_error, *head)
    launch.release, launch.device, launch.index, launch.raw_stream = release, device, index, raw_stream
    return launch
