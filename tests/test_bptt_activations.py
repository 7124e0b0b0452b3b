"""BPTT actors with Tanh / ELU / LeakyReLU trunks, the part that needs no GPU: the activations are part of a generated chain class's
shape, cache key and source (visfly_amd/_jit.py), the BPTT plugin of the Tanh actor is on the pre-build list and cross-compiles for gfx950,
and the trainers' constructors / archives name the activations (tests/test_bptt_activations_gpu.py runs them)."""
import os

import pytest

SAC_HOVER = ({"state": 13}, {"state": [64, 64, 32]}, [32], [32])
CFG = ("bptt", 0, 1, 0, True)        # hover kind, bodyrate, Euler, ctrl_delay


def test_activations_are_part_of_the_shape_the_cache_key_and_the_source():
    from visfly_amd import _jit
    relu = _jit.shape_of(*SAC_HOVER, head_dims=(4, 4))
    sh = _jit.shape_of(*SAC_HOVER, head_dims=(4, 4), acts=(2, 1))
    assert sh[-1] == ("act", 2, 1) and sh[:-1] == relu and not _jit.is_builtin(sh)
    assert _jit.shape_of(*SAC_HOVER, head_dims=(4, 4), acts=(1, 1)) == relu
    # every (trunk, extractor) pair is a class of its own, for the chain plugin and for the BPTT plugin
    keys = {_jit._key(_jit.shape_of(*SAC_HOVER, head_dims=(4, 4), acts=a), CFG) for a in ((1, 1), (2, 1), (1, 2), (3, 1), (4, 1), (2, 2))}
    assert len(keys) == 6
    assert _jit.path_of(sh, CFG) != _jit.path_of(relu, CFG) and "_a21_bptt0101_" in _jit.path_of(sh, CFG)
    assert _jit.path_of(sh) != _jit.path_of(relu)
    src = _jit.bptt_source(sh, CFG[1:])
    assert "static constexpr int ACT = 2, EACT = 1;" in src and "static constexpr int HM = 4, HV = 4;" in src
    assert "VF_CHAIN_PLUGIN_BPTT_DEFINE(Net, NetPi, 0, 1, 0, true," in src and "act tanh/relu" in src
    assert "static constexpr int ACT = 1, EACT = 1;" in _jit.bptt_source(relu, CFG[1:])
    assert "static constexpr int ACT = 3, EACT = 4;" in _jit.bptt_source(_jit.shape_of(*SAC_HOVER, head_dims=(4, 4), acts=(3, 4)), CFG[1:])


def test_the_tanh_actor_is_on_the_prebuild_lists():
    from visfly_amd import _jit
    names = [n for n, cfg in _jit.PREBUILD_BPTT if ("bptt",) + cfg == CFG and n in _jit.PREBUILD_ACT and _jit.PREBUILD_ACT[n][5] == (2, 1)]
    assert "sac_hover_tanh" in names
    v = _jit.PREBUILD_ACT["sac_hover_tanh"]
    assert v[:5] == _jit.PREBUILD_SAC["sac_hover"] and _jit.prebuild_shape("sac_hover_tanh") == _jit.shape_of(*SAC_HOVER, head_dims=(4, 4), acts=(2, 1))
    # every BPTT entry names a shape one of the lists holds; the entries whose name is PREBUILD_ACT's carry that list's activations
    for n, _cfg in _jit.PREBUILD_BPTT:
        sh = _jit.prebuild_shape(n)
        assert sh is not None and (_jit._acts(sh) != (1, 1)) == (n in _jit.PREBUILD_ACT), n
    assert _jit.prebuild_shape("sac_hover") == _jit.shape_of(*_jit.PREBUILD_SAC["sac_hover"])


def test_the_tanh_bptt_plugin_compiles_for_gfx950_and_registers():
    """hipcc cross-compiles both persistent launches of the Tanh actor without a GPU (cached: __graft_entry__.build() made it)"""
    from visfly_amd import _jit, _lib
    lib = _lib.lib()
    sh = _jit.prebuild_shape("sac_hover_tanh")
    for path in (_jit.build(sh), _jit.build(sh, rollout=CFG)):
        assert os.path.exists(path) and os.path.dirname(path) == _jit.JIT_DIR
        _lib.check(lib.vf_chain_plugin_load(path.encode()))
    names = [lib.vf_chain_plugin_name(i) for i in range(lib.vf_chain_plugin_count())]
    assert _jit.name_of(sh).encode() in names
    assert any(n.startswith(_jit.name_of(sh).encode()) and b"BPTT horizon kind 0 act 1 int 0 delay 1" in n for n in names)


def test_only_shac_refuses_an_activation():
    """the translation of policy_kwargs (no device needed): BPTT takes the four activations of ppo.activation_kind for trunks and extractor,
    SHAC's check still raises and says who refuses"""
    from visfly_amd import checkpoint
    from visfly_amd.bptt import BPTT
    from visfly_amd.shac import SHAC
    for name, kind in (("ReLU", 1), ("Tanh", 2), ("ELU", 3), ("LeakyReLU", 4), ("leaky_relu", 4)):
        pk = checkpoint.policy_kwargs_from_reference(dict(activation_fn=name, features_extractor_kwargs=dict(activation_fn=name)), ["state"])
        assert BPTT._activations(BPTT.__new__(BPTT), pk) == (kind, kind)
        if kind != 1:
            with pytest.raises(NotImplementedError, match="SHAC"):
                SHAC._activations(SHAC.__new__(SHAC), pk)
    assert SHAC._activations(SHAC.__new__(SHAC), dict(activation=1, extractor_activation="relu")) == (1, 1)
    with pytest.raises(NotImplementedError):
        BPTT._activations(BPTT.__new__(BPTT), dict(activation="gelu"))
    # native MlpPolicy arguments (an archive's policy_spec) pass through the translation: `activation` wins, `activation_fn` is honoured
    assert BPTT._activations(BPTT.__new__(BPTT), dict(extractor={}, activation="tanh", activation_fn="relu")) == (2, 1)
    assert BPTT._activations(BPTT.__new__(BPTT), dict(extractor={}, activation_fn="elu", extractor_activation="tanh")) == (3, 2)


def test_archive_activation_check():
    from types import SimpleNamespace
    from visfly_amd import checkpoint
    tanh, relu = SimpleNamespace(act=2, ext_act=1), SimpleNamespace(act=1, ext_act=1)
    assert checkpoint.activation_spec(tanh) == dict(activation="tanh", extractor_activation="relu")
    assert checkpoint.activation_spec(relu) == dict(activation="relu", extractor_activation="relu")
    checkpoint.check_activations(tanh, checkpoint.activation_spec(tanh))
    checkpoint.check_activations(relu, {})           # an archive without the fields is a ReLU network
    checkpoint.check_activations(relu, None)
    for pol, spec in ((relu, checkpoint.activation_spec(tanh)), (tanh, {}), (tanh, dict(activation="tanh", extractor_activation="tanh"))):
        with pytest.raises(ValueError, match="activations"):
            checkpoint.check_activations(pol, spec)
