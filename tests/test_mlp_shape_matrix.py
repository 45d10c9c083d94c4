"""The shape matrix of tests/mlp_shapes.py without a GPU: the table covers what tests/test_mlp_shape_matrix_gpu.py claims
to run (every kernel instantiation, every gradient block geometry, both grid regimes, the partial tiles, the second load
chunk), the Python twin of ppo_plan agrees with the library, and every row is sharp: dropping the last input unit or the
last output unit of any layer moves the outputs and the gradient by at least 100 times the tolerance the GPU test
applies. (The packing of every row is run by tests/test_mlp_policy.py, whose SHAPES hold the matrix.)"""

import ctypes as C

import numpy as np
import pytest

from tests import mlp_reference as MR
from tests import mlp_shapes as S
from tests import ppo_reference as R
from upkie_amd import lib

SHARPNESS = 100.0  # a dropped unit moves a checked quantity by at least this many tolerances
ROWS = list(enumerate(S.MATRIX))
IDS = [S.row_id(r) for r in S.MATRIX]
GRAD_CFG = dict(ent_coef=0.01, clip_range_vf=0.2, max_grad_norm=1e9)  # the GPU gradient test's


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


def _plans():
    return [R.plan(S.shape_of(r)) for r in S.MATRIX]


def test_matrix_keeps_the_symmetric_cases_and_has_unique_rows():
    for row, case in zip(S.MATRIX, S.CASES + [S.WIDEST]):
        assert (row.N, row.obs_dim, row.actor, row.act_dim, row.activation) == tuple(case) and row.critic == row.actor
    assert len(set(IDS)) == len(IDS)
    assert max(r.N for r in S.MATRIX) == 4096
    assert all(r.critic for r in S.MATRIX), "a shape with no critic tower is out of scope"


def test_every_instantiation_is_in_the_table(library):
    pairs = set()
    for row in S.MATRIX:
        shape = S.shape_of(row)
        assert library.upkie_mlp_packed_words(C.byref(shape)) == MR._layout(shape)["words"], row
        pairs.add((S.width_class(shape), row.activation))
    assert pairs == {(w, a) for w in (16, 32, 64, 128, 256) for a in ("tanh", "relu")}


@pytest.mark.parametrize("row", S.MATRIX, ids=IDS)
def test_plan_twin_is_the_librarys_workspace(row, library):
    """The workspace depends on the grid, hence on nw and the cap: minibatches whose tile counts every nw divides
    differently, the row's own minibatch, and one past every cap."""
    shape = S.shape_of(row)
    p = R.plan(shape)
    for mb in (1, 16 * 12, 16 * 12 + 1, 16 * 60, S.T * row.N, 1 << 20):
        assert library.upkie_ppo_workspace_bytes(C.byref(shape), mb) == R.workspace_bytes(p, mb), (mb, p)
    grids = {nw: R.grid(dict(p, nw=nw), 16 * 12) for nw in (1, 2, 3, 4)}
    assert len(set(grids.values())) == 4, "at 12 tiles the workspace tells the four nw apart"
    assert p["lds_bytes"] <= 4 * 16 * (256 + 4 * 256 + 64 + 64)


def test_block_geometries_and_grid_regimes():
    plans = _plans()
    assert {p["nw"] for p in plans} == {1, 2, 3, 4}
    over = [r for r, p in zip(S.MATRIX, plans) if R.chunks(p, S.T * r.N) > p["grid_cap"]]
    under = [r for r, p in zip(S.MATRIX, plans) if R.chunks(p, S.T * r.N) < p["grid_cap"]]
    assert over, "a row whose blocks add a later chunk to their own partial gradient"
    assert under, "a row with fewer chunks than the grid cap"
    # launch A takes the larger tower's stage: the table has rows where that is the actor's, and where it is the critic's
    assert any(p["stage_floats"][0] > p["stage_floats"][1] for p in plans) and any(p["stage_floats"][1] > p["stage_floats"][0] for p in plans)


def test_partial_tiles():
    ns = [r.N for r in S.MATRIX]
    assert any(n < 16 for n in ns) and any(n % 16 == 0 for n in ns) and any(n > 16 and n % 16 for n in ns)
    assert any((S.T * n) % 16 for n in ns), "a gradient minibatch with a partial last tile"


def test_what_decides_the_width_class():
    cls = lambda *ws: next(c for c in (16, 32, 64, 128, 256) if max(ws) <= c)  # noqa: E731 (of parts of a shape: the whole is width_class)
    by = {"critic": 0, "obs_dim": 0, "act_dim": 0}
    for row in S.MATRIX:
        W = S.width_class(S.shape_of(row))
        parts = {"critic": cls(*row.critic), "obs_dim": cls(row.obs_dim), "act_dim": cls(row.act_dim), "actor": cls(*row.actor)}
        assert W == max(parts.values())
        top = [k for k, v in parts.items() if v == W]
        if len(top) == 1 and top[0] in by:
            by[top[0]] += 1
    assert all(by.values()), by


def test_second_load_chunk_and_partly_filled_action_tile():
    assert any(MR._layout(S.shape_of(r))["actor"][0][3] > 8 for r in S.MATRIX if r.N != S.WIDEST[0] or r.obs_dim != S.WIDEST[1]), \
        "a row besides the widest whose first layer has more than CH = 8 input tiles"
    assert any(r.obs_dim > 128 and r.obs_dim % 16 for r in S.MATRIX), "a second chunk whose last tile is partly filled"
    assert any(17 <= r.act_dim <= 31 for r in S.MATRIX)
    assert any(r.act_dim == 64 for r in S.MATRIX) and any(r.act_dim == 16 for r in S.MATRIX)


# ---------------------------------------------------------------- sharpness
def _tensor_index(row, tower, layer):
    """Index of the weight of `layer` of a tower in the sources; its bias follows."""
    return 5 + 2 * layer + (2 * (len(row.actor) + 1) if tower == "critic" else 0)


def _grad_index(row, tower, layer):
    return _tensor_index(row, tower, layer) - 4  # (the gradient list starts at log_std)


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("index,row", ROWS, ids=IDS)
def test_every_layers_last_units_are_seen(index, row):
    """Per tower and layer: zero the weight column of the last input unit; separately, the weight row and bias of the
    last output unit. The tower's output (on the policy test's observations) moves by >= 100 bounds on some sample, and
    the gradient of the layer's tensors (on the gradient test's rollout) by >= 100 bounds. So does the part of the
    unchanged gradient that belongs to the unit: a kernel that dropped it would be that far off."""
    normalize = S.row_normalize(index)
    shape = S.shape_of(row, normalize)
    actor, critic = S.row_modules(row)
    src = S.row_sources(row, actor, critic, normalize)
    bound = S.bounds(row)
    obs = S.row_observations(row, scale=2.0 if normalize else 1.0).double().numpy()
    _, mean0, value0 = MR.forward(shape, src, obs)
    data = S.row_rollout(row, shape, src)
    flat = lambda k, *tail: data[k].astype(np.float64).reshape(S.T * row.N, *tail)  # noqa: E731
    args = (flat("observations", row.obs_dim), flat("actions", row.act_dim), flat("values"), flat("log_probs"), flat("advantages"), flat("returns"))
    _, grads0, _ = R.minibatch(shape, src, *args, **GRAD_CFG)
    for tower, widths, out in (("actor", row.actor, row.act_dim), ("critic", row.critic, 1)):
        for layer in range(len(widths) + 1):
            k = _tensor_index(row, tower, layer)
            gW, gb = grads0[_grad_index(row, tower, layer)], grads0[_grad_index(row, tower, layer) + 1]
            where = (tower, layer)
            # the unit's own share of the gradient
            assert np.linalg.norm(gW[:, -1]) >= SHARPNESS * bound["grad"] * np.linalg.norm(gW), where
            assert np.linalg.norm(gW[-1, :]) >= SHARPNESS * bound["grad"] * np.linalg.norm(gW), where
            assert abs(gb[-1]) >= SHARPNESS * bound["grad"] * np.linalg.norm(gb), where
            for change in ("input", "output"):
                changed = [np.array(s, dtype=np.float64, copy=True) for s in src]
                if change == "input":
                    changed[k][:, -1] = 0.0
                else:
                    changed[k][-1, :] = 0.0
                    changed[k + 1][-1] = 0.0
                _, mean, value = MR.forward(shape, changed, obs)
                moved = np.abs(mean - mean0).max() if tower == "actor" else np.abs(value - value0).max()
                assert moved >= SHARPNESS * bound["mean" if tower == "actor" else "value"], (where, change, moved)
                _, grads, _ = R.minibatch(shape, changed, *args, **GRAD_CFG)
                concerned = [0] if change == "input" else [0, 1]
                for j in concerned:
                    g0, g = grads0[_grad_index(row, tower, layer) + j], grads[_grad_index(row, tower, layer) + j]
                    assert _rel(g, g0) >= SHARPNESS * bound["grad"], (where, change, j, _rel(g, g0))
