"""`PpoTrainer.update`'s launch plan without a GPU: the sequence of (entry point, arguments) it hands the launcher, and
the slot exchanges between them, for one rank and for a process group, plain and controlled. The trainer is built with
``__new__``: a recording launcher, a library whose attributes are their own names, recording `SlotExchange` doubles
of two ranks and small host tensors for the buffers. Ten samples in minibatches of four: sizes 4, 4 and 2, so that
``start``, ``size`` and ``world * size`` all vary. Pointers are compared by the NAME of the tensor they came from
(views by their index; an epoch's ``adv_stats[e]`` begins where ``adv_stats[e, 0]`` does, and ``scalars`` is the
first two words of ``control``: one address each)."""

import contextlib
import ctypes as C
import types

import pytest
import torch

from upkie_amd import abi
from upkie_amd.ppo import PpoTrainer

EPOCHS, TOTAL, BATCH, D, A = 2, 10, 4, 4, 1
SAMPLES = ("observations", "actions", "values", "log_probs", "advantages", "returns")  # the six arrays every minibatch launch reads

ONE_RANK_PLAIN = [
    ("upkie_ppo_advantage_stats", 10, 4, "perm[0]", "advantages", 1, "adv_stats[0,0]"),
    ("upkie_ppo_minibatch_update", "shape", "cfg", 10, 0, 4, 4, "perm[0]", *SAMPLES, "adv_stats[0,0]", "packed", "m", "v", "control", "workspace", "stats[0,0]"),
    ("upkie_ppo_minibatch_update", "shape", "cfg", 10, 4, 4, 4, "perm[0]", *SAMPLES, "adv_stats[0,1]", "packed", "m", "v", "control", "workspace", "stats[0,1]"),
    ("upkie_ppo_minibatch_update", "shape", "cfg", 10, 8, 2, 4, "perm[0]", *SAMPLES, "adv_stats[0,2]", "packed", "m", "v", "control", "workspace", "stats[0,2]"),
    ("upkie_ppo_advantage_stats", 10, 4, "perm[1]", "advantages", 1, "adv_stats[1,0]"),
    ("upkie_ppo_minibatch_update", "shape", "cfg", 10, 0, 4, 4, "perm[1]", *SAMPLES, "adv_stats[1,0]", "packed", "m", "v", "control", "workspace", "stats[1,0]"),
    ("upkie_ppo_minibatch_update", "shape", "cfg", 10, 4, 4, 4, "perm[1]", *SAMPLES, "adv_stats[1,1]", "packed", "m", "v", "control", "workspace", "stats[1,1]"),
    ("upkie_ppo_minibatch_update", "shape", "cfg", 10, 8, 2, 4, "perm[1]", *SAMPLES, "adv_stats[1,2]", "packed", "m", "v", "control", "workspace", "stats[1,2]"),
]

ONE_RANK_CONTROLLED = [
    ("upkie_ppo_update_begin", "control"),
    ("upkie_ppo_advantage_stats", 10, 4, "perm[0]", "advantages", 1, "adv_stats[0,0]"),
    ("upkie_ppo_minibatch_update_controlled", "shape", "cfg", 10, 0, 4, 4, "perm[0]", *SAMPLES, "adv_stats[0,0]", "packed", "m", "v", "control", "workspace", "stats[0,0]"),
    ("upkie_ppo_minibatch_update_controlled", "shape", "cfg", 10, 4, 4, 4, "perm[0]", *SAMPLES, "adv_stats[0,1]", "packed", "m", "v", "control", "workspace", "stats[0,1]"),
    ("upkie_ppo_minibatch_update_controlled", "shape", "cfg", 10, 8, 2, 4, "perm[0]", *SAMPLES, "adv_stats[0,2]", "packed", "m", "v", "control", "workspace", "stats[0,2]"),
    ("upkie_ppo_advantage_stats", 10, 4, "perm[1]", "advantages", 1, "adv_stats[1,0]"),
    ("upkie_ppo_minibatch_update_controlled", "shape", "cfg", 10, 0, 4, 4, "perm[1]", *SAMPLES, "adv_stats[1,0]", "packed", "m", "v", "control", "workspace", "stats[1,0]"),
    ("upkie_ppo_minibatch_update_controlled", "shape", "cfg", 10, 4, 4, 4, "perm[1]", *SAMPLES, "adv_stats[1,1]", "packed", "m", "v", "control", "workspace", "stats[1,1]"),
    ("upkie_ppo_minibatch_update_controlled", "shape", "cfg", 10, 8, 2, 4, "perm[1]", *SAMPLES, "adv_stats[1,2]", "packed", "m", "v", "control", "workspace", "stats[1,2]"),
]

GROUP_PLAIN = [
    ("upkie_ppo_advantage_partials", 10, 4, "perm[0]", "advantages", 0, None, 2, "adv.mine"),
    ("exchange", "adv"),
    ("upkie_ppo_advantage_partials", 10, 4, "perm[0]", "advantages", 1, "adv.slots", 2, "adv.mine"),
    ("exchange", "adv"),
    ("upkie_ppo_advantage_finish", 10, 4, 1, "adv.slots", 2, "adv_stats[0,0]"),
    ("upkie_ppo_minibatch_gradient", "shape", "cfg", 10, 0, 4, 8, 4, "perm[0]", *SAMPLES, "adv_stats[0,0]", "packed", "workspace", "grad.mine"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply", "shape", "cfg", 8, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[0,0]"),
    ("upkie_ppo_minibatch_gradient", "shape", "cfg", 10, 4, 4, 8, 4, "perm[0]", *SAMPLES, "adv_stats[0,1]", "packed", "workspace", "grad.mine"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply", "shape", "cfg", 8, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[0,1]"),
    ("upkie_ppo_minibatch_gradient", "shape", "cfg", 10, 8, 2, 4, 4, "perm[0]", *SAMPLES, "adv_stats[0,2]", "packed", "workspace", "grad.mine"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply", "shape", "cfg", 4, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[0,2]"),
    ("upkie_ppo_advantage_partials", 10, 4, "perm[1]", "advantages", 0, None, 2, "adv.mine"),
    ("exchange", "adv"),
    ("upkie_ppo_advantage_partials", 10, 4, "perm[1]", "advantages", 1, "adv.slots", 2, "adv.mine"),
    ("exchange", "adv"),
    ("upkie_ppo_advantage_finish", 10, 4, 1, "adv.slots", 2, "adv_stats[1,0]"),
    ("upkie_ppo_minibatch_gradient", "shape", "cfg", 10, 0, 4, 8, 4, "perm[1]", *SAMPLES, "adv_stats[1,0]", "packed", "workspace", "grad.mine"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply", "shape", "cfg", 8, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[1,0]"),
    ("upkie_ppo_minibatch_gradient", "shape", "cfg", 10, 4, 4, 8, 4, "perm[1]", *SAMPLES, "adv_stats[1,1]", "packed", "workspace", "grad.mine"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply", "shape", "cfg", 8, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[1,1]"),
    ("upkie_ppo_minibatch_gradient", "shape", "cfg", 10, 8, 2, 4, 4, "perm[1]", *SAMPLES, "adv_stats[1,2]", "packed", "workspace", "grad.mine"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply", "shape", "cfg", 4, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[1,2]"),
]

GROUP_CONTROLLED = [
    ("upkie_ppo_update_begin", "control"),
    ("upkie_ppo_advantage_partials", 10, 4, "perm[0]", "advantages", 0, None, 2, "adv.mine"),
    ("exchange", "adv"),
    ("upkie_ppo_advantage_partials", 10, 4, "perm[0]", "advantages", 1, "adv.slots", 2, "adv.mine"),
    ("exchange", "adv"),
    ("upkie_ppo_advantage_finish", 10, 4, 1, "adv.slots", 2, "adv_stats[0,0]"),
    ("upkie_ppo_minibatch_gradient_controlled", "shape", "cfg", 10, 0, 4, 8, 4, "perm[0]", *SAMPLES, "adv_stats[0,0]", "packed", "workspace", "grad.mine", "control"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply_controlled", "shape", "cfg", 0, 8, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[0,0]"),
    ("upkie_ppo_minibatch_gradient_controlled", "shape", "cfg", 10, 4, 4, 8, 4, "perm[0]", *SAMPLES, "adv_stats[0,1]", "packed", "workspace", "grad.mine", "control"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply_controlled", "shape", "cfg", 4, 8, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[0,1]"),
    ("upkie_ppo_minibatch_gradient_controlled", "shape", "cfg", 10, 8, 2, 4, 4, "perm[0]", *SAMPLES, "adv_stats[0,2]", "packed", "workspace", "grad.mine", "control"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply_controlled", "shape", "cfg", 8, 4, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[0,2]"),
    ("upkie_ppo_advantage_partials", 10, 4, "perm[1]", "advantages", 0, None, 2, "adv.mine"),
    ("exchange", "adv"),
    ("upkie_ppo_advantage_partials", 10, 4, "perm[1]", "advantages", 1, "adv.slots", 2, "adv.mine"),
    ("exchange", "adv"),
    ("upkie_ppo_advantage_finish", 10, 4, 1, "adv.slots", 2, "adv_stats[1,0]"),
    ("upkie_ppo_minibatch_gradient_controlled", "shape", "cfg", 10, 0, 4, 8, 4, "perm[1]", *SAMPLES, "adv_stats[1,0]", "packed", "workspace", "grad.mine", "control"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply_controlled", "shape", "cfg", 0, 8, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[1,0]"),
    ("upkie_ppo_minibatch_gradient_controlled", "shape", "cfg", 10, 4, 4, 8, 4, "perm[1]", *SAMPLES, "adv_stats[1,1]", "packed", "workspace", "grad.mine", "control"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply_controlled", "shape", "cfg", 4, 8, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[1,1]"),
    ("upkie_ppo_minibatch_gradient_controlled", "shape", "cfg", 10, 8, 2, 4, 4, "perm[1]", *SAMPLES, "adv_stats[1,2]", "packed", "workspace", "grad.mine", "control"),
    ("exchange", "grad"),
    ("upkie_ppo_minibatch_apply_controlled", "shape", "cfg", 8, 4, 4, "grad.slots", 2, "packed", "m", "v", "control", "workspace", "stats[1,2]"),
]


class _Names:
    """A library whose every attribute is its own name."""

    def __getattr__(self, name):
        return name


class _Exchange:
    def __init__(self, name, words, log):
        self.name, self.world, self.log = name, 2, log
        self.mine, self.slots = torch.zeros(words), torch.zeros(2, words)

    def exchange(self):
        self.log.append(("exchange", self.name))


def _trainer(monkeypatch, group, controlled):
    """(trainer, buffer, log, entered): `log` is what `update` launched and exchanged, `entered` the device blocks."""
    log, entered, names = [], [], {}
    tr = PpoTrainer.__new__(PpoTrainer)
    shape, config = abi.UpkieMlpShape(), abi.UpkiePpoConfig()
    shape.obs_dim, shape.act_dim = D, A
    names[C.addressof(shape)], names[C.addressof(config)] = "shape", "cfg"
    f32 = dict(dtype=torch.float32)
    buffer = types.SimpleNamespace(device=torch.device("cpu"), buffer_size=TOTAL // 2, n_envs=2, observations=torch.zeros(TOTAL // 2, 2, D, **f32),
                                   actions=torch.zeros(TOTAL // 2, 2, A, **f32), values=torch.zeros(TOTAL // 2, 2, **f32),
                                   log_probs=torch.zeros(TOTAL // 2, 2, **f32), advantages=torch.zeros(TOTAL // 2, 2, **f32),
                                   returns=torch.zeros(TOTAL // 2, 2, **f32))
    tr.policy = types.SimpleNamespace(shape=shape, packed=torch.zeros(64), _normalizer=None)
    tr.config, tr.device, tr.obs_normalized, tr.normalize_advantage, tr.controlled = config, torch.device("cpu"), False, True, controlled
    tr.n_epochs, tr.batch_size, tr._mb, tr.n_minibatches, tr._total = EPOCHS, BATCH, BATCH, 3, TOTAL
    tr.m, tr.v, tr.workspace = torch.zeros(64), torch.zeros(64), torch.zeros(32, dtype=torch.uint8)
    tr.control = torch.zeros(abi.PPO_CTRL_WORDS, dtype=torch.float64)
    tr.scalars = tr.control[:2]
    tr.perm = torch.zeros((EPOCHS, TOTAL), dtype=torch.int32)
    tr.adv_stats, tr.stats = torch.zeros((EPOCHS, 3, 2), dtype=torch.float64), torch.zeros((EPOCHS, 3, 7), **f32)
    tr.advantages, tr.returns = torch.zeros(TOTAL, **f32), torch.zeros(TOTAL, **f32)
    tr._buffer = PpoTrainer._addresses(buffer)
    tr.process_group = "a group" if group else None
    tr._grad_exchange = _Exchange("grad", 16, log) if group else None
    tr._adv_exchange = _Exchange("adv", 8, log) if group else None
    for name in ("m", "v", "control", "workspace", "advantages", "returns"):  # (the trainer's advantages and returns, not the buffer's)
        names[getattr(tr, name).data_ptr()] = name
    for name in ("observations", "actions", "values", "log_probs"):
        names[getattr(buffer, name).data_ptr()] = name
    names[tr.policy.packed.data_ptr()] = "packed"
    for e in range(EPOCHS):
        names[tr.perm[e].data_ptr()] = f"perm[{e}]"
        for j in range(3):
            names[tr.adv_stats[e, j].data_ptr()], names[tr.stats[e, j].data_ptr()] = f"adv_stats[{e},{j}]", f"stats[{e},{j}]"
    for ex in (tr._grad_exchange, tr._adv_exchange):
        if ex is not None:
            names[ex.mine.data_ptr()], names[ex.slots.data_ptr()] = f"{ex.name}.mine", f"{ex.name}.slots"
    assert len(set(names.values())) == len(names)

    def name_of(arg):
        if arg is None or isinstance(arg, int) and arg not in names:
            assert arg is None or arg < 4096, "an address of no known tensor"
            return arg
        return names[arg if isinstance(arg, int) else C.addressof(arg._obj)]

    tr._lib = _Names()
    tr._launcher = lambda fn, *args: log.append((fn,) + tuple(name_of(a) for a in args))
    tr.sync_modules = lambda: log.append(("sync_modules",))

    @contextlib.contextmanager
    def device(dev):
        entered.append(dev)
        yield

    monkeypatch.setattr(torch.cuda, "device", device)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return tr, buffer, log, entered


@pytest.mark.parametrize("group,controlled,expected", [(False, False, ONE_RANK_PLAIN), (False, True, ONE_RANK_CONTROLLED),
                                                       (True, False, GROUP_PLAIN), (True, True, GROUP_CONTROLLED)])
def test_update_issues_exactly_these_launches_and_exchanges(monkeypatch, group, controlled, expected):
    tr, buffer, log, entered = _trainer(monkeypatch, group, controlled)
    assert tr.update(buffer, sync=False) is tr.stats
    assert log == expected
    assert entered == [torch.device("cpu")], "one device block around the whole update"
    del log[:]
    tr.update(buffer)
    assert log == expected + [("sync_modules",)]


def test_update_with_a_process_group_refuses_a_capture(monkeypatch):
    tr, buffer, log, _ = _trainer(monkeypatch, True, False)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(Exception, match="cannot be captured in a graph"):
        tr.update(buffer)
    assert log == []
    tr, buffer, log, _ = _trainer(monkeypatch, False, False)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    tr.update(buffer, sync=False)  # (one rank: capturable)
    assert log == ONE_RANK_PLAIN
