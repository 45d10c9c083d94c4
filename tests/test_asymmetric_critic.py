"""The asymmetric actor-critic without a device: the packed layout and the gradient launch's plan against their twins,
symmetric shapes pinned to what they were, `pack_index` round trips, every refusal, that the matrix of
tests/asymmetric_shapes.py reaches every instantiation, block geometry, grid regime and input-tile edge (and needs each of
its later rows for that), and that the inputs of tests/test_asymmetric_critic_gpu.py tell the feature from its likely
bugs (the critic fed the actor's observation; the privileged stage's one-line mistakes, at every layout of its table)."""

import ctypes as C
import types

import numpy as np
import pytest

from tests import asymmetric_reference as AR
from tests import asymmetric_shapes as AS
from tests import mlp_reference as R
from tests import mlp_shapes as S
from tests import ppo_reference as PR
from upkie_amd import abi, lib
from upkie_amd.policies import asymmetric_shape, mlp_shape, pack_index

ROWS = [pytest.param(i, r, id=AS.row_id(r)) for i, r in enumerate(AS.ROWS)]


@pytest.fixture(scope="module")
def library():
    return lib.load()


def _error(library):
    return library.upkie_sim_last_error(None).decode()


# ---------------------------------------------------------------- layout
@pytest.mark.parametrize("index,row", ROWS)
def test_the_layout_twin_is_the_librarys(library, index, row):
    shape = AS.shape_of(row, AS.row_normalize(index))
    assert int(shape.critic_obs_dim) == row.critic_obs_dim
    lay, plan = AR.layout(shape), AR.plan(shape)
    assert int(library.upkie_mlp_packed_words(C.byref(shape))) == lay["words"]
    for n in (1, 16 * plan["nw"] + 1, AS.T * row.N, 131072):
        assert int(library.upkie_ppo_workspace_bytes(C.byref(shape), n)) == PR.workspace_bytes(plan, n), n
    dcp = (row.critic_obs_dim + 3) // 4 * 4
    assert lay["critic_std"] == lay["critic_mean"] + dcp and lay["log_std"] == lay["critic_std"] + dcp, "mean, std directly after it, then log_std"
    from upkie_amd.ppo import trainable_offset

    assert trainable_offset(shape) == lay["log_std"]


@pytest.mark.parametrize("row", S.MATRIX, ids=[S.row_id(r) for r in S.MATRIX])
def test_a_symmetric_shape_keeps_its_sizes(library, row):
    """critic_obs_dim = 0: the packed words and the workspace bytes are the symmetric twins', which predate the field."""
    shape = S.shape_of(row)
    assert int(shape.critic_obs_dim) == 0
    lay, plan = R._layout(shape), PR.plan(shape)
    assert int(library.upkie_mlp_packed_words(C.byref(shape))) == lay["words"]
    assert AR.layout(shape)["words"] == lay["words"] and AR.plan(shape) == plan
    for n in (1, S.T * row.N, 131072):
        assert int(library.upkie_ppo_workspace_bytes(C.byref(shape), n)) == PR.workspace_bytes(plan, n), n


def test_the_struct_grew_at_its_end(library):
    assert abi.UpkieMlpShape.critic_obs_dim.offset == abi.UpkieMlpShape.clip_obs.offset + 4
    assert C.sizeof(abi.UpkieMlpShape) == abi.UpkieMlpShape.critic_obs_dim.offset + 4 == int(library.upkie_hip_struct_bytes(9))
    for name in ("upkie_mlp_actor_critic_asym", "upkie_ppo_minibatch_update_asym", "upkie_ppo_minibatch_gradient_asym", "upkie_privileged_observation"):
        assert name in lib.EXPORTED_SYMBOLS and hasattr(library, name)


@pytest.mark.parametrize("index,row", ROWS)
def test_pack_index_round_trip(index, row):
    """Pack, then unpack, returns the sources; and the statistics sit where the layout twin says."""
    normalize = AS.row_normalize(index)
    shape = AS.shape_of(row, normalize)
    sources = AS.row_sources(row, *AS.row_modules(row), normalize=True)
    sizes = [s.size for s in sources]
    index_map = pack_index(shape, sizes)
    lay = AR.layout(shape)
    assert index_map.size == lay["words"]
    flat = np.concatenate([s.reshape(-1) for s in sources] + [np.zeros(1)])
    packed = flat[index_map]
    back = np.zeros(flat.size)
    back[index_map] = packed
    back[-1] = 0.0
    for k, (got, want) in enumerate(zip(np.split(back[:-1], np.cumsum(sizes)[:-1]), sources)):
        assert np.array_equal(got, want.reshape(-1)), k
    Dc = row.critic_obs_dim
    assert np.array_equal(packed[lay["critic_mean"]: lay["critic_mean"] + Dc], sources[4])
    assert np.array_equal(packed[lay["critic_std"]: lay["critic_std"] + Dc], sources[5])
    assert np.array_equal(packed[lay["log_std"]: lay["log_std"] + row.act_dim], sources[6])
    # the critic's first layer in the first-layer order of its own width: word (o, t, lane, s) = W[16 o + (lane & 15)][16 t + 4 s + (lane >> 4)]
    kind, w_off, _, in_t, _ = lay["critic"][0]
    Wc = sources[AR.N_FIXED + 1 + 2 * (len(row.actor) + 1)]
    assert kind == "mfma" and in_t == (Dc + 15) // 16 and Wc.shape == (row.critic[0], Dc)
    for o, t, lane, s in ((0, 0, 0, 0), (0, in_t - 1, 17, 1), (0, in_t - 1, 63, 3), (0, 0, 5, 2)):
        unit, k = 16 * o + (lane & 15), 16 * t + 4 * s + (lane >> 4)
        want = Wc[unit, k] if unit < Wc.shape[0] and k < Dc else 0.0
        assert packed[w_off + ((o * in_t + t) * 64 + lane) * 4 + s] == want, (o, t, lane, s)


# ---------------------------------------------------------------- what the matrix covers
NEW_ROWS = range(6, len(AS.ROWS))


def _geometry(row):
    """What decides the code a row runs: the plan twin's launch geometry of its T N minibatch and the layout twin's tiles."""
    shape = AS.shape_of(row)
    lay, plan = AR.layout(shape), AR.plan(shape)
    cls = lambda *ws: next(c for c in (16, 32, 64, 128, 256) if max(ws) <= c)  # noqa: E731
    rest = cls(row.obs_dim, row.act_dim, row.critic_obs_dim, *row.actor)
    return {"W": lay["W"], "nw": plan["nw"], "chunks": PR.chunks(plan, AS.T * row.N), "grid_cap": plan["grid_cap"], "lds_bytes": plan["lds_bytes"],
            "actor_tiles": lay["actor"][0][3], "critic_tiles": lay["critic"][0][3], "W_by_critic_layers_alone": cls(*row.critic) > rest}


def _uncovered(rows):
    """The claims of the matrix that `rows` leave open (none, for the whole table)."""
    geo = [_geometry(r) for r in rows]
    both = list(zip(rows, geo))
    tiles = {g["critic_tiles"] for g in geo}
    claims = {
        "the ten (W, activation) instantiations": {(g["W"], r.activation) for r, g in both} == {(w, a) for w in (16, 32, 64, 128, 256) for a in ("tanh", "relu")},
        "gradient blocks of 1, 2, 3 and 4 waves": {g["nw"] for g in geo} == {1, 2, 3, 4},
        "a row above the grid cap: a block restages, then stages the next chunk's actor rows and adds to its partial": any(g["chunks"] > g["grid_cap"] for g in geo),
        "a row below the grid cap": any(g["chunks"] < g["grid_cap"] for g in geo),
        "a stage above the default dynamic-LDS limit": any(g["lds_bytes"] > PR.LDS_BUDGET for g in geo),
        "critic input tiles of 1, 2, more than 8, and 16": {1, 2, 16} <= tiles and any(8 < t < 16 for t in tiles),
        "a Dc that is a multiple of 16 and one that is no multiple of 4": any(r.critic_obs_dim % 16 == 0 for r in rows) and any(r.critic_obs_dim % 4 for r in rows),
        "more actor input tiles than critic's, and the reverse": any(g["actor_tiles"] > g["critic_tiles"] for g in geo) and any(g["actor_tiles"] < g["critic_tiles"] for g in geo),
        "sixteen actor input tiles over one critic tile, the largest stale overlap": any(g["actor_tiles"] == 16 and g["critic_tiles"] == 1 for g in geo),
        "a width class set by a critic hidden layer alone": any(g["W_by_critic_layers_alone"] for g in geo),
        "N = 1, and a T N that is no multiple of 16": any(r.N == 1 for r in rows) and any((AS.T * r.N) % 16 for r in rows),
    }
    return [name for name, held in claims.items() if not held]


def test_the_matrix_covers_every_geometry_and_no_new_row_is_spare():
    """The table reaches every instantiation, block geometry, grid regime and input-tile edge of the kernels the critic's
    own row goes through -- and each row appended for that is needed: without it some claim is open."""
    assert _uncovered(AS.ROWS) == []
    assert len({AS.row_id(r) for r in AS.ROWS}) == len(AS.ROWS) and max(r.N for r in AS.ROWS) <= 1001
    for index in NEW_ROWS:
        rest = [r for k, r in enumerate(AS.ROWS) if k != index]
        assert _uncovered(rest), f"row {index} ({AS.row_id(AS.ROWS[index])}) adds nothing the others do not cover"
    widest = _geometry(AS.ROWS[11])
    assert widest["lds_bytes"] == 90112 and widest["nw"] == 1 and widest["actor_tiles"] == widest["critic_tiles"] == 16 and AS.T * AS.ROWS[11].N == 200


def test_the_degenerate_rows_reach_a_short_block_and_the_grid_cap():
    """The bit-for-bit test runs its rows with Dc = D: also then one of them has fewer than four waves per block, and one
    has more chunks than blocks (its full update is where the asymmetric Adam and fold are compared)."""
    assert AS.DEGENERATE[:2] == (4, 5)
    geo = [_geometry(AS.ROWS[i]._replace(critic_obs_dim=AS.ROWS[i].obs_dim)) for i in AS.DEGENERATE]
    assert any(g["nw"] < 4 for g in geo) and any(g["chunks"] > g["grid_cap"] for g in geo), geo
    # the update's minibatches are N + 7 samples and the rest: the row above the cap stays above it in both
    row = AS.ROWS[10]
    plan = AR.plan(AS.shape_of(row._replace(critic_obs_dim=row.obs_dim)))
    assert all(PR.chunks(plan, n) > plan["grid_cap"] for n in (row.N + 7, AS.T * row.N - (row.N + 7)))


# ---------------------------------------------------------------- refusals
def test_mlp_shape_takes_a_critic_of_another_width():
    shape = mlp_shape(S.dims(4, [16], 1), S.dims(9, [16], 1), "tanh")
    assert int(shape.critic_obs_dim) == 9 and int(shape.obs_dim) == 4
    assert int(mlp_shape(S.dims(4, [16], 1), S.dims(4, [16], 1), "tanh").critic_obs_dim) == 0
    assert int(asymmetric_shape(mlp_shape(S.dims(4, [16], 1), S.dims(4, [16], 1), "tanh")).critic_obs_dim) == 4
    with pytest.raises(ValueError, match="1-256"):
        mlp_shape(S.dims(4, [16], 1), S.dims(257, [16], 1), "tanh")
    with pytest.raises(ValueError, match="needs a critic"):
        asymmetric_shape(mlp_shape(S.dims(4, [16], 1), [], "tanh"))


def test_shapes_out_of_range_are_refused(library):
    shape = AS.shape_of(AS.ROWS[0])
    for bad, layers in ((-1, 1), (257, 1), (5, 0)):
        s = abi.UpkieMlpShape.from_buffer_copy(shape)
        s.critic_obs_dim, s.critic_layers = bad, layers
        assert int(library.upkie_mlp_packed_words(C.byref(s))) == abi.ERR_INVALID_ARGUMENT
        assert "critic_obs_dim" in _error(library)
        assert int(library.upkie_ppo_workspace_bytes(C.byref(s), 64)) == abi.ERR_INVALID_ARGUMENT


def test_the_old_entry_points_refuse_an_asymmetric_shape(library):
    """Before any device use, with a message that names both widths and the entry point that takes the critic's rows."""
    shape, cfg = AS.shape_of(AS.ROWS[0]), abi.UpkiePpoConfig()
    head = (C.byref(shape), C.byref(cfg))
    one = 1  # (any non-null pointer: the refusal comes first)
    calls = [
        (library.upkie_mlp_actor_critic, (4, C.byref(shape), one, one, None, 0, 1) + (None,) * 7, "upkie_mlp_actor_critic_asym"),
        (library.upkie_ppo_minibatch_update, head + (8, 0, 8, 8) + (one,) * 15, "upkie_ppo_minibatch_update_asym"),
        (library.upkie_ppo_minibatch_update_controlled, head + (8, 0, 8, 8) + (8,) * 15, "upkie_ppo_minibatch_update_asym"),
        (library.upkie_ppo_minibatch_gradient, head + (8, 0, 8, 8, 8) + (8,) * 12, "upkie_ppo_minibatch_gradient_asym"),
        (library.upkie_ppo_minibatch_gradient_controlled, head + (8, 0, 8, 8, 8) + (8,) * 13, "upkie_ppo_minibatch_gradient_asym"),
    ]
    for fn, args, other in calls:
        assert fn(*args) == abi.ERR_INVALID_ARGUMENT, fn.__name__
        message = _error(library)
        assert "critic_obs_dim 5" in message and "obs_dim 3" in message and other in message, message
    assert library.upkie_ppo_minibatch_update_asym(*head, 8, 0, 8, 8, one, one, None, *((one,) * 14)) == abi.ERR_INVALID_ARGUMENT
    assert "critic_obs" in _error(library)
    assert library.upkie_mlp_actor_critic_asym(4, C.byref(shape), one, one, None, None, 0, 1, None, None, None, None, None, one, None,
                                               None) == abi.ERR_INVALID_ARGUMENT
    assert "critic_obs" in _error(library)


def test_the_privileged_entry_point_checks_its_segments(library):
    def call(kinds, counts, obs_dim=4, act_dim=2, sources=(8, 8, 8, 8, 8, 8), reset=0, final=8):
        k, c = (C.c_int32 * len(kinds))(*kinds), (C.c_int32 * len(counts))(*counts)
        next_obs, final_obs, command, force, scale, links = sources
        return library.upkie_privileged_observation(16, obs_dim, act_dim, len(kinds), k, c, next_obs, final_obs, command, force, scale, links, None,
                                                    None, reset, 8, final, None)

    no_device = abi.ERR_NO_DEVICE if library.upkie_hip_device_count() <= 0 else None
    for kinds, counts in (([], []), ([9], [1]), ([0], [5]), ([1], [3]), ([2], [4]), ([3], [25]), ([0, 3, 3], [4, 24, 24]), ([0] * 9, [1] * 9)):
        assert call(kinds, counts) == abi.ERR_INVALID_ARGUMENT, (kinds, counts)
        assert "privileged" in _error(library)
    assert call([0, 2], [4, 3], sources=(8, 8, 8, None, 8, 8)) == abi.ERR_INVALID_ARGUMENT and "segment 1" in _error(library)
    assert call([3], [2], sources=(8, 8, 8, 8, 8, None)) == abi.ERR_INVALID_ARGUMENT
    assert call([0], [4], final=None) == abi.ERR_INVALID_ARGUMENT and "final_observation" in _error(library)
    if no_device is not None:
        assert call([0, 1, 2, 3], [4, 2, 3, 4]) == no_device


def test_ppo_names_both_sizes_on_every_mismatch():
    from upkie_amd.ppo import Ppo

    env = types.SimpleNamespace(num_envs=4)
    sym = types.SimpleNamespace(shape=types.SimpleNamespace(obs_dim=40, act_dim=1), asymmetric=False, critic_obs_dim=40)
    asym = types.SimpleNamespace(shape=types.SimpleNamespace(obs_dim=40, act_dim=1), asymmetric=True, critic_obs_dim=12)
    rows = lambda dim, n=4: types.SimpleNamespace(dim=dim, num_envs=n)  # noqa: E731
    with pytest.raises(ValueError, match="asymmetric.*reads 12 words.*actor 40"):
        Ppo(env, asym)
    with pytest.raises(ValueError, match="critic_observation has 12 words.*symmetric.*40-word"):
        Ppo(env, sym, critic_observation=rows(12))
    with pytest.raises(ValueError, match="critic_observation has 9 words.*takes 12"):
        Ppo(env, asym, critic_observation=rows(9))
    with pytest.raises(ValueError, match="serves 8 envs.*has 4"):
        Ppo(env, asym, critic_observation=rows(12, 8))
    assert Ppo(env, asym, critic_observation=rows(12)).critic_observation.dim == 12


# ---------------------------------------------------------------- the inputs tell the bugs from the feature
@pytest.mark.parametrize("index,row", ROWS)
def test_the_critics_row_is_told_from_the_actors(index, row):
    """With the twin, on the GPU tests' inputs: the value of the critic fed `obs` (truncated or zero-padded to Dc) differs
    from the value of the critic fed `critic_obs` by more than 100 x the value bound on at least 90 % of the samples, and
    the critic's first-layer gradient by more than 100 x its Frobenius bound. A kernel that read the wrong pointer, width,
    statistics or stage rows cannot pass tests/test_asymmetric_critic_gpu.py on these rows."""
    normalize = AS.row_normalize(index)
    shape = AS.shape_of(row, normalize)
    sources = AS.row_sources(row, *AS.row_modules(row), normalize)
    obs, cobs = (t.double().numpy() * (2.0 if normalize else 1.0) for t in AS.row_observations(row, scale=1.0))
    wrong = AS.obs_as_critic_rows(row, obs)
    _, _, _, value = AR.forward(shape, sources, obs, cobs)
    _, _, _, value_wrong = AR.forward(shape, sources, obs, wrong)
    told = np.abs(value - value_wrong) > 100 * AS.BOUNDS["value"]
    assert told.mean() >= 0.9, told.mean()

    data = AS.row_rollout(row, shape, sources)
    total = AS.T * row.N
    flat = lambda k, *tail: data[k].astype(np.float64).reshape(total, *tail)  # noqa: E731
    args = (flat("actions", row.act_dim), flat("values"), flat("log_probs"), flat("advantages"), flat("returns"))
    kw = dict(ent_coef=0.01, clip_range_vf=0.2, max_grad_norm=1e9)
    o, c = flat("observations", row.obs_dim), flat("critic_observations", row.critic_obs_dim)
    _, grads, _ = AR.minibatch(shape, sources, o, c, *args, **kw)
    _, grads_wrong, _ = AR.minibatch(shape, sources, o, AS.obs_as_critic_rows(row, o), *args, **kw)
    first = 1 + 2 * (len(row.actor) + 1)  # the critic's first-layer weight
    assert grads[first].shape == (row.critic[0], row.critic_obs_dim)
    rel = np.linalg.norm(grads[first] - grads_wrong[first]) / np.linalg.norm(grads[first])
    assert rel > 100 * AS.BOUNDS["grad"], rel
    for k in range(first):  # the actor's half does not see the critic's rows at all
        assert np.array_equal(grads[k], grads_wrong[k]), k


def test_the_recombined_gradient_is_the_symmetric_twins_when_the_rows_coincide():
    """Dc = D and critic_obs = obs with equal statistics: the composed twin is `ppo_reference.minibatch`, term for term."""
    row = AS.ROWS[4]
    sym = mlp_shape(S.dims(row.obs_dim, row.actor, row.act_dim), S.dims(row.obs_dim, row.critic, 1), row.activation, True, 3.0)
    shape = asymmetric_shape(sym)
    src = AS.row_sources(row, *AS.row_modules(row), normalize=True)
    src[4], src[5] = src[0], src[1]
    sym_src = src[:4] + src[6:]
    data = AS.row_rollout(row, shape, src)
    total = AS.T * row.N
    flat = lambda k, *tail: data[k].astype(np.float64).reshape(total, *tail)  # noqa: E731
    args = (flat("actions", row.act_dim), flat("values"), flat("log_probs"), flat("advantages"), flat("returns"))
    o = flat("observations", row.obs_dim)
    stats, grads, ratio = AR.minibatch(shape, src, o, o, *args, ent_coef=0.01, clip_range_vf=0.2)
    want_stats, want_grads, want_ratio = PR.minibatch(sym, sym_src, o, *args, ent_coef=0.01, clip_range_vf=0.2)
    np.testing.assert_allclose(stats, want_stats, rtol=1e-13, atol=0.0)
    assert np.array_equal(ratio, want_ratio) and len(grads) == len(want_grads)
    for g, w in zip(grads, want_grads):
        assert np.array_equal(g, w)


# ---------------------------------------------------------------- the privileged stage's twin
@pytest.mark.parametrize("num_envs", AS.PRIVILEGED_SIZES)
def test_each_one_line_mistake_of_the_privileged_stage_shows(num_envs):
    """On the inputs the GPU test feeds the kernel, each of the three mutations changes some output of some call."""
    calls = AS.privileged_calls(num_envs)
    assert sum(int((c["terminated"] | c["truncated"]).sum()) for c in calls) >= 1, "some episode ends"
    good = AS.run_privileged_twin(num_envs, calls)
    D, A = AS.PRIVILEGED_D, AS.PRIVILEGED_A
    assert good[1][0].shape == (num_envs, D + A + 3 + len(AS.PRIVILEGED_LINKS))
    for mutation in AR.MUTATIONS:
        assert _shows(AS.DEFAULT_LAYOUT, num_envs, calls, good, mutation), mutation
    # and the rule itself: where the episode ended the terminal row is final_obs, then the previous row's tail
    for k in range(1, len(calls)):
        c, (row, final), (before, _) = calls[k], good[k], good[k - 1]
        done = (c["terminated"] | c["truncated"]) != 0
        assert np.array_equal(final[done, :D], c["final_obs"][done]) and np.array_equal(final[done, D:], before[done, D:])
        assert np.array_equal(final[~done], row[~done]) and np.array_equal(row[:, :D], c["next_obs"])
        assert np.array_equal(row[:, D + A: D + A + 3], c["force"].T) and np.array_equal(row[:, D + A + 3:], c["link_scale"][list(AS.PRIVILEGED_LINKS)].T)


def _shows(layout, num_envs, calls, good, mutation):
    bad = AS.run_privileged_twin(num_envs, calls, mutation, layout)
    return any(not np.array_equal(g[0], b[0]) or not np.array_equal(g[1], b[1]) for g, b in zip(good[1:], bad[1:]))


def _applies(layout, mutation):
    """Whether a layout has the segment a mutation breaks."""
    include = layout.include
    return {"new_tail_in_terminal_row": include != ("observation",), "force_before_events_step": "push_force" in include,
            "final_obs_ignored": "observation" in include, "mask_ignored_on_reset": True,
            "default_order_starts": include != tuple(k for k in AS.SEGMENTS if k in include)}[mutation]


def test_the_layout_table_holds_what_the_kernel_serves():
    by_name = {lay.name: lay for lay in AS.PRIVILEGED_LAYOUTS}
    assert len(by_name) == len(AS.PRIVILEGED_LAYOUTS) and AS.PRIVILEGED_LAYOUTS[0] is AS.DEFAULT_LAYOUT
    assert (AS.DEFAULT_LAYOUT.include, AS.DEFAULT_LAYOUT.sizes, AS.DEFAULT_LAYOUT.calls) == (AS.SEGMENTS, (1, 65, 1000), 40)
    assert by_name["reversed"].include == ("link_scale", "push_force", "command", "observation")
    assert by_name["observation-256"].include == ("observation",) and AS.layout_dim(by_name["observation-256"]) == 256
    assert by_name["force-alone"].include == ("push_force",)
    staged = lambda lay: sum({"push_force": 3, "link_scale": len(lay.links)}.get(k, 0) for k in lay.include)  # noqa: E731
    assert staged(by_name["27-columns"]) == 27 and staged(AS.DEFAULT_LAYOUT) == 7 and staged(by_name["observation-256"]) == 0
    assert -(-27 * 64 // 256) == 7 and -(-7 * 64 // 256) == 2, "passes of the 256-thread staging loop over 64 envs per column"
    full = by_name["256-words"]
    assert AS.layout_dim(full) == 256 and set(full.include) == set(AS.SEGMENTS)
    for name in ("reversed", "27-columns"):
        assert by_name[name].sizes == (1, 63, 64, 65, 129, 1000)
    assert all(lay.sizes == (1, 65, 1000) for lay in AS.PRIVILEGED_LAYOUTS if lay.name not in ("reversed", "27-columns"))
    assert all(AS.layout_dim(lay) <= 256 and lay.A <= 64 and max(lay.links, default=0) < AS.PRIVILEGED_MAX_LINKS for lay in AS.PRIVILEGED_LAYOUTS)
    for op in ("step", "step_no_final", "step_no_flags", "reset_mixed", "reset_zero", "reset_all"):
        assert op in AS.SCRIPT
    # every mutation has a new layout to show on, and the order mutation more than one
    for mutation in AR.LAYOUT_MUTATIONS:
        assert sum(_applies(lay, mutation) for lay in AS.NEW_LAYOUTS) >= 2, mutation


LAYOUT_CASES, LAYOUT_IDS = AS.layout_cases()


@pytest.mark.parametrize("layout,num_envs", LAYOUT_CASES, ids=LAYOUT_IDS)
def test_each_one_line_mistake_shows_on_every_layout(layout, num_envs):
    """On the inputs the GPU test feeds the kernel at a new layout and size: episodes of both kinds end, every mutation
    whose segment the layout has changes some output of some call, and the twin keeps the rules call by call."""
    N, D = num_envs, layout.D
    calls = AS.layout_calls(layout, N)
    assert len(calls) == 1 + layout.calls and [c["op"] for c in calls[1:]] == list(AS.SCRIPT)
    terminated, truncated = (sum(int(c[k].sum()) for c in calls) for k in ("terminated", "truncated"))
    assert terminated + truncated >= 1 and (N == 1 or (terminated >= 1 and truncated >= 1)), (terminated, truncated)
    ended_without_final = sum(int((c["terminated"] | c["truncated"]).sum()) for c in calls[1:] if c["op"] == "step_no_final")
    assert N == 1 or ended_without_final >= 1, "an episode ends in a step that has no final_obs"
    good = AS.run_privileged_twin(N, calls, layout=layout)
    assert good[1][0].shape == (N, AS.layout_dim(layout))
    for mutation in AR.LAYOUT_MUTATIONS:
        if _applies(layout, mutation):
            assert _shows(layout, N, calls, good, mutation), mutation

    # the rules, stated over the row's columns without the twin's own row builder
    counts = {"observation": D, "command": layout.A, "push_force": 3, "link_scale": len(layout.links)}
    at, cols = 0, {}
    for name in layout.include:
        cols[name] = slice(at, at + counts[name])
        at += counts[name]
    obs_cols = np.zeros(at, dtype=bool)
    if "observation" in cols:
        obs_cols[cols["observation"]] = True

    def new_row(c):
        parts = {"observation": c["next_obs"], "command": c["command"], "push_force": c["force"].T, "link_scale": c["link_scale"][list(layout.links)].T}
        return np.concatenate([parts[name] for name in layout.include], axis=1)

    assert np.array_equal(good[0][0], new_row(calls[0]))
    final_before = np.zeros((N, at), dtype=np.float32)
    for k in range(1, len(calls)):
        c, (row, final), (before, _) = calls[k], good[k], good[k - 1]
        op = c["op"]
        if op.startswith("reset"):
            take = np.ones(N, dtype=bool) if c["mask"] is None else c["mask"] != 0
            assert (op == "reset_mixed") <= (N == 1 or 0 < take.sum() < N) and (op != "reset_zero" or not take.any())
            assert np.array_equal(row[take], new_row(c)[take]) and np.array_equal(row[~take], before[~take]), (k, op)
            assert np.array_equal(final, final_before), "a reset leaves the terminal rows alone"
        else:
            done = ((c["terminated"] | c["truncated"]) != 0) & (op != "step_no_flags")
            last = c["next_obs"] if op == "step_no_final" else c["final_obs"]
            assert np.array_equal(row, new_row(c)), (k, op)
            assert np.array_equal(final[~done], row[~done])
            assert np.array_equal(final[done][:, ~obs_cols], before[done][:, ~obs_cols])
            if "observation" in cols:
                assert np.array_equal(final[done][:, obs_cols], last[done])
            assert op != "step_no_flags" or np.array_equal(final, row)
        final_before = final
