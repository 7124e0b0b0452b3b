"""The twin critic over a TWO-branch extractor as a generated chain class (visfly_amd/_jit.py: NB = 2 with PASS = 1), without a GPU: the
shape rules, the generated source, which class an MlpPolicy with the layout picks, and the C entry point that carries the third input
pointer.  The kernels themselves: tests/test_two_branch_critic_gpu.py."""
import pytest

CRITICS = ["critic_gate", "critic_nav"]


@pytest.mark.parametrize("name", CRITICS)
def test_two_branch_critic_shapes_are_generated_classes(name):
    from visfly_amd import _jit
    dims, ext, pi, vf, heads, pas = _jit.PREBUILD_CRITIC[name]
    sh = _jit.shape_of(dims, ext, pi, vf, heads, pas)
    assert sh is not None and not _jit.is_builtin(sh) and sh[-1] == (1, 1)
    assert len(sh[0]) == 2 and len(sh[1]) == 2, "two observation branches"
    assert sh == _jit.prebuild_shape(name)
    src = _jit.source(sh)
    assert "static constexpr int NB = 2;" in src and "static constexpr int PASS = 1;" in src
    assert "static constexpr int HM = 1, HV = 1;" in src
    assert "(+) action, heads 1/1" in _jit.name_of(sh) and _jit._slug(sh).endswith("_h11")
    # a class of its own: neither the actor's over the same extractor nor the one-branch critic's
    actor = _jit.shape_of({k: v for k, v in dims.items() if k != "action"}, ext, pi, vf, (4, 4))
    assert actor is not None and _jit.path_of(actor) != _jit.path_of(sh)
    one = _jit.shape_of({"state": dims["state"], "action": 4}, {"state": ext["state"]}, pi, vf, heads, pas)
    assert one is not None and len(one[0]) == 1 and _jit.path_of(one) != _jit.path_of(sh)


def test_the_gate_column_is_branch_one_with_kin_8():
    from visfly_amd import _jit
    sh = _jit.prebuild_shape("critic_gate")
    assert sh[0] == (16, 8) and sh[1] == ((2, 1), (1,)) and sh[2] == sh[3] == (1,)
    assert "static constexpr int KIN[2] = {16, 8};" in _jit.source(sh)
    assert _jit.prebuild_shape("critic_nav")[:4] == ((16, 8), ((2, 2), (1,)), (2,), (2,))


def test_what_stays_off_the_chain_classes():
    """features (+) action are the K of the trunks' first layers: four input tiles at most, the pass-through tile among them"""
    from visfly_amd import _jit
    dims = {"state": 13, "target": 3, "action": 4}
    crit = dict(head_dims=(1, 1), passthrough=("action",))
    # the trainers' default two-branch extractor: 64 + 64 + 4 = 132 columns
    assert _jit.shape_of(dims, {"state": [128, 64], "target": [128, 64]}, [64, 64], [64, 64], **crit) is None
    # 96 + 32 + 4 = 132 as well; 64 + 32 + 4 = 100 and 96 + 4 fit
    assert _jit.shape_of(dims, {"state": [96], "target": [32]}, [64], [64], **crit) is None
    assert _jit.shape_of(dims, {"state": [64], "target": [32]}, [64], [64], **crit) is not None
    assert _jit.shape_of({"state": 13, "action": 4}, {"state": [128]}, [64], [64], **crit) is None
    assert _jit.shape_of({"state": 13, "action": 4}, {"state": [96]}, [64], [64], **crit) is not None
    # 6 pass-through columns, two pass-through inputs, three branches
    ext = {"state": [64, 64], "target": [32]}
    assert _jit.shape_of({**dims, "action": 6}, ext, [64], [64], **crit) is None
    assert _jit.shape_of({**dims, "extra": 2}, ext, [64], [64], head_dims=(1, 1), passthrough=("action", "extra")) is None
    assert _jit.shape_of({**dims, "gate": 1}, {**ext, "gate": [32]}, [64], [64], **crit) is None
    # a critic needs its pass-through input, an actor must not have one
    assert _jit.shape_of(dims, ext, [64], [64], head_dims=(1, 1)) is None
    assert _jit.shape_of(dims, ext, [64], [64], head_dims=(4, 4), passthrough=("action",)) is None


@pytest.mark.parametrize("name", CRITICS)
def test_policy_with_the_layout_picks_the_class(name):
    from visfly_amd import _jit
    from visfly_amd.ppo import MlpPolicy
    dims, ext, pi, vf, heads, pas = _jit.PREBUILD_CRITIC[name]
    pol = MlpPolicy(dims, ext, pi, vf, "cpu", seed=1, ortho_init=False, head_dims=heads, passthrough=pas, log_std_param=False)
    assert pol.chain_shape == _jit.prebuild_shape(name)
    assert not pol.wide and pol._plan is not None and pol.chain_jit is False      # (nothing is compiled for a CPU policy)
    assert pol.obs_keys == list(ext) + ["action"]
    # the frozen identity layer sits between the extractor layers and the trunks; the trunks read features (+) action
    n_ext = sum(len(v) for v in ext.values())
    assert pol.layers[n_ext].frozen and pol.layers[n_ext].src == "obs:action"
    feat = sum(v[-1] for v in ext.values())
    assert pol.layers[n_ext].dc == feat and pol.layers[n_ext + 1].K == feat + 4


def test_default_two_branch_critic_keeps_its_layer_by_layer_path():
    from visfly_amd.ppo import MlpPolicy
    dims = {"state": 13, "target": 3, "action": 4}
    pol = MlpPolicy(dims, {"state": [128, 64], "target": [128, 64]}, [64, 64], [64, 64], "cpu", seed=1, ortho_init=False, head_dims=(1, 1),
                    passthrough=("action",), log_std_param=False)
    assert pol.wide and pol._plan is None and pol.chain_shape is None
    assert pol.twin_q_update(None, None, None, 1) is False


def test_entry_point_with_the_third_input_is_exported():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from visfly_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "vf_twin_q_update_in3") and hasattr(L, "vf_twin_q_update")
    res3, args3 = _lib.SIGNATURES["vf_twin_q_update_in3"]
    res2, args2 = _lib.SIGNATURES["vf_twin_q_update"]
    assert res3 is res2 is C.c_int and len(args3) == len(args2) + 1 == 13
    assert L.vf_twin_q_update_in3.argtypes is not None and len(L.vf_twin_q_update_in3.argtypes) == 13
    assert L.vf_abi_version() == _lib.ABI_VERSION == 11
    # argument checks come before any device work
    assert L.vf_twin_q_update_in3(*([None] * 10), 0, 0, None) == -1 and b"vf_twin_q_update" in L.vf_last_error()      # VF_EINVAL


def test_prebuild_lists_the_two_critics():
    """__graft_entry__.build() compiles them with the other pre-built shapes"""
    import os
    from visfly_amd import _jit
    for name in CRITICS:
        assert name in _jit.PREBUILD_CRITIC
        path = _jit.path_of(_jit.prebuild_shape(name))
        assert os.path.dirname(path) == _jit.JIT_DIR and "_h11_" in os.path.basename(path)
