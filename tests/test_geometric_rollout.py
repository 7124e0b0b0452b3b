"""The persistent PPO roll-out and evaluation launches for the velocity / position action types (the geometric SO(3) controller), the part
that needs no GPU: the library holds built-in instances for all four action types in the roll-out and evaluation kernels and none in the
BPTT kernels, the generated classes' plugins for these action types are on the pre-build lists and cross-compile for gfx950, the ABI is
unchanged, and BPTT / SHAC refuse such an env in their constructors (tests/test_geometric_rollout_gpu.py runs the launches)."""
import os
import re

import pytest

VELOCITY, POSITION = 2, 3           # VF_ACT_* (include/visfly_amd.h)
GEOMETRIC_ROLLOUT = [("one_layer_extractor", (0, VELOCITY, 0, True)), ("one_layer_extractor", (1, POSITION, 0, True))]
GEOMETRIC_EVAL = [("tanh_nav", (1, POSITION, 0, True))]


def _instances(kernel):
    """{(rows per wave, env kind, action type, integrator, motor lag)} of the instances of `kernel` libvisfly_amd.so holds, read from the
    mangled names: k<Net, ROWS, KIND, ACT, INTEG, CTRL_DELAY> ends in ..Li<ROWS>ELi<K>ELi<A>ELi<I>ELb<D>EEEv"""
    from visfly_amd import _lib
    with open(_lib.LIB, "rb") as f:
        blob = f.read()
    pat = re.compile(rb"%s\w*?Li(16|32)ELi(\d)ELi(\d)ELi(\d)ELb([01])EEEv" % kernel)
    return {tuple(int(x) for x in m.groups()) for m in pat.finditer(blob)}


def test_the_library_has_roll_out_and_evaluation_instances_for_all_four_action_types():
    for kernel in (b"k_ppo_rollout", b"k_eval_rollout"):
        inst = _instances(kernel)
        assert {a for _, _, a, _, _ in inst} == {0, 1, VELOCITY, POSITION}, kernel
        # every (rows, kind, integrator, motor lag) the bodyrate action type has, the two geometric ones have as well
        for act in (VELOCITY, POSITION):
            assert {(r, k, i, d) for r, k, a, i, d in inst if a == act} == {(r, k, i, d) for r, k, a, i, d in inst if a == 1}, (kernel, act)
        assert {r for r, *_ in inst} == {16, 32} and {i for _, _, _, i, _ in inst} == {0, 1}


def test_the_bptt_kernels_have_no_geometric_instance():
    """the adjoint covers thrust and bodyrate: the horizon launches' dispatchers do not ask with_env_config for the other two"""
    from visfly_amd import _lib
    with open(_lib.LIB, "rb") as f:
        blob = f.read()
    for kernel in (b"k_bptt_rollout", b"k_bptt_reverse"):
        names = set(re.findall(rb"_ZN2vf\d+%s\w+" % kernel, blob))
        assert names, kernel
        # <.., KIND, ACT, INTEG, CTRL_DELAY[, ..]>: no name carries the action types 2 / 3 in front of an integrator and a bool
        acts = {int(m.group(1)) for n in names for m in re.finditer(rb"Li[0-3]ELi(\d)ELi[01]ELb[01]E", n)}
        assert acts and acts <= {0, 1}, (kernel, acts)


def test_abi_is_unchanged():
    from visfly_amd import _lib
    assert _lib.lib().vf_abi_version() == 11


@pytest.mark.parametrize("kind", ["rollout", "eval"])
def test_geometric_plugins_are_prebuilt_for_gfx950_and_register(kind):
    """cached: __graft_entry__.build() made the entries of the pre-build lists"""
    from visfly_amd import _jit, _lib
    lib = _lib.lib()
    entries, listed = (GEOMETRIC_ROLLOUT, _jit.PREBUILD_ROLLOUT) if kind == "rollout" else (GEOMETRIC_EVAL, _jit.PREBUILD_EVAL)
    for name, cfg in entries:
        assert (name, cfg) in listed
        sh = _jit.prebuild_shape(name)
        key = cfg if kind == "rollout" else ("eval",) + cfg
        path = _jit.path_of(sh, key)
        assert os.path.exists(path) and os.path.dirname(path) == _jit.JIT_DIR, path
        with open(path, "rb") as f:
            assert b"gfx950" in f.read()
        _lib.check(lib.vf_chain_plugin_load(path.encode()))
        what = b"roll-out" if kind == "rollout" else b"evaluation"
        want = b"%s kind %d act %d int %d delay %d" % (what, cfg[0], cfg[1], cfg[2], int(cfg[3]))
        names = [lib.vf_chain_plugin_name(i) for i in range(lib.vf_chain_plugin_count())]
        assert any(n.startswith(_jit.name_of(sh).encode()) and want in n for n in names), (want, names)
    # every geometric entry of either list is one of the above (a new one gets its test case here)
    assert sorted(e for e in listed if e[1][1] in (VELOCITY, POSITION)) == sorted(entries)


@pytest.mark.parametrize("act", [VELOCITY, POSITION])
def test_generated_sources_name_the_action_type(act):
    from visfly_amd import _jit
    sh = _jit.prebuild_shape("one_layer_extractor")
    src = _jit.rollout_source(sh, (0, act, 0, True))
    assert f"VF_CHAIN_PLUGIN_ROLLOUT_DEFINE(Net, 0, {act}, 0, true," in src and f"roll-out kind 0 act {act} int 0 delay 1" in src
    src = _jit.eval_source(sh, (1, act, 1, False))
    assert f"VF_CHAIN_PLUGIN_EVAL_DEFINE(Net, 1, {act}, 1, false," in src and f"evaluation kind 1 act {act} int 1 delay 0" in src
    # one cache file per action type
    assert len({_jit.path_of(sh, (0, a, 0, True)) for a in range(4)}) == 4 and len({_jit.path_of(sh, ("eval", 0, a, 0, True)) for a in range(4)}) == 4


class _Env:
    """as much of an env as the constructors look at before they refuse"""
    def __init__(self, action_type):
        from types import SimpleNamespace
        from visfly_amd.constants import ACTION_TYPES
        self.envs = SimpleNamespace(dynamics=SimpleNamespace(constants={"action_type": ACTION_TYPES[action_type]}))


@pytest.mark.parametrize("action_type", ["velocity", "position"])
def test_bptt_and_shac_refuse_the_geometric_action_types_in_the_constructor(action_type):
    from visfly_amd.bptt import BPTT
    from visfly_amd.shac import SHAC
    for cls in (BPTT, SHAC):
        with pytest.raises(NotImplementedError, match=f'{cls.__name__} over action_type="{action_type}"') as e:
            cls(_Env(action_type))
        assert "autograd raises" in str(e.value) and "PPO" in str(e.value)


@pytest.mark.parametrize("action_type", ["thrust", "bodyrate"])
def test_the_refusal_is_for_the_geometric_action_types_only(action_type):
    """thrust / bodyrate pass the check: the constructor goes on (and fails on the stand-in env's missing members, not with the refusal)"""
    from visfly_amd.bptt import BPTT
    with pytest.raises(AttributeError):
        BPTT(_Env(action_type))
