"""Actor-critic policies whose actor and critic do not share a feature extractor (utils/policies/policies.py:117-175,210-215: the
reference's ``share_features_extractor=False`` and its ``pi_features_extractor_class`` / ``vf_features_extractor_class``), on the host side:
the translation of both reference forms and of what the reference's own asserts refuse, the layer table and ``flat`` layout MlpPolicy
builds, the archive names and shapes, forward values and the parameter gradient against fixtures read off the reference's own policy
(tests/golden/sep_keys.json, sep_extractor.npz: tools/gen_sep_golden.py), the chain-kernel shape / generated source, and that a policy
without the argument is what it was."""
import json
import os
import types

import numpy as np
import pytest
import torch

from _gradcheck import assert_blocks

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIMS = {"state": 13, "target": 3}
ST = {"state": [64, 32], "target": [32]}
# the two forms of the fixture: MlpPolicy arguments (extractor, pi, vf, vf_extractor, activation)
FORMS = {"sym": (ST, [32], [32], ST, "tanh"), "asym": ({"state": [64]}, [32, 32], [64], ST, "relu")}


def ref_net_arch(e):
    return dict(net_arch={k: dict(layer=list(v)) for k, v in e.items()}, activation_fn="relu")


def reference_kwargs(form):
    if form == "sym":
        return dict(features_extractor_class="StateTargetExtractor", features_extractor_kwargs=ref_net_arch(ST),
                    share_features_extractor=False, net_arch=dict(pi=[32], vf=[32]), activation_fn="tanh")
    return dict(features_extractor_class=None, pi_features_extractor_class="StateExtractor",
                pi_features_extractor_kwargs=ref_net_arch({"state": [64]}), vf_features_extractor_class="StateTargetExtractor",
                vf_features_extractor_kwargs=ref_net_arch(ST), share_features_extractor=False, net_arch=dict(pi=[32, 32], vf=[64]),
                activation_fn="relu")


def policy(form, seed=1, device="cpu"):
    from visfly_amd.ppo import MlpPolicy
    ext, pi, vf, vext, act = FORMS[form]
    dims = {k: DIMS[k] for k in dict.fromkeys(list(ext) + list(vext))}
    return MlpPolicy(dims, ext, pi, vf, device, seed=seed, activation=act, vf_extractor=vext, log_std_init=-0.5)


@pytest.mark.parametrize("form", list(FORMS))
def test_both_reference_forms_translate(form):
    from visfly_amd import checkpoint
    from visfly_amd.ppo import ACTIVATIONS
    ext, pi, vf, vext, act = FORMS[form]
    pk = checkpoint.policy_kwargs_from_reference(reference_kwargs(form), ["state", "target"])
    assert pk["extractor"] == ext and pk["vf_extractor"] == vext and (pk["pi"], pk["vf"]) == (pi, vf)
    assert pk["activation"] == ACTIVATIONS[act] and pk["extractor_activation"] == pk["vf_extractor_activation"] == ACTIVATIONS["relu"]
    assert checkpoint.extractor_keys(reference_kwargs(form), ["state", "target"]) == ("state", "target")
    assert checkpoint.extractor_keys(pk, ["state", "target"]) == ("state", "target")
    # each side's own activation_fn
    kw = reference_kwargs(form)
    kw["vf_features_extractor_kwargs" if form == "asym" else "features_extractor_kwargs"]["activation_fn"] = "elu"
    pk = checkpoint.policy_kwargs_from_reference(kw, ["state", "target"])
    assert pk["vf_extractor_activation"] == ACTIVATIONS["elu"]
    assert pk["extractor_activation"] == (ACTIVATIONS["relu"] if form == "asym" else ACTIVATIONS["elu"])
    # class objects are read by name
    if form == "asym":
        kw = reference_kwargs(form)
        kw["pi_features_extractor_class"] = type("StateExtractor", (), {})
        kw["vf_features_extractor_class"] = type("StateTargetExtractor", (), {})
        assert checkpoint.policy_kwargs_from_reference(kw, ["state", "target"])["vf_extractor"] == vext
    # the shared network keeps translating to what it did
    shared = dict(reference_kwargs("sym"), share_features_extractor=True)
    assert "vf_extractor" not in checkpoint.policy_kwargs_from_reference(shared, ["state", "target"])


def test_what_the_reference_refuses_is_a_value_error():
    from visfly_amd import checkpoint
    tr = lambda **kw: checkpoint.policy_kwargs_from_reference(kw, ["state", "target"])
    a = reference_kwargs("asym")
    with pytest.raises(ValueError, match="policies.py:133"):        # features_extractor_class=None without both side classes
        tr(**{k: v for k, v in a.items() if k != "vf_features_extractor_class"})
    with pytest.raises(ValueError, match="policies.py:133"):
        tr(features_extractor_class=None)
    with pytest.raises(ValueError, match="policies.py:138"):        # side classes next to features_extractor_class
        tr(**dict(a, features_extractor_class="StateExtractor"))
    with pytest.raises(ValueError, match="policies.py:136"):        # side classes with share_features_extractor=True (its default)
        tr(**dict(a, share_features_extractor=True))
    with pytest.raises(ValueError, match="policies.py:136"):
        tr(**{k: v for k, v in a.items() if k != "share_features_extractor"})
    with pytest.raises(ValueError, match="needs observation keys"):
        checkpoint.policy_kwargs_from_reference(a, ["state"])


@pytest.mark.parametrize("flag", ["bn", "ln"])
@pytest.mark.parametrize("side", ["pi", "vf"])
@pytest.mark.parametrize("form", list(FORMS))
def test_norm_layers_on_either_side_are_not_implemented(form, side, flag):
    from visfly_amd import checkpoint
    kw = reference_kwargs(form)
    if form == "sym":        # one class, instantiated twice: the flag is on both sides
        kw["features_extractor_kwargs"]["net_arch"]["state"][flag] = True
    else:
        kw[f"{side}_features_extractor_kwargs"]["net_arch"]["state"][flag] = True
    with pytest.raises(NotImplementedError, match="batch norm" if flag == "bn" else "layer norm"):
        checkpoint.policy_kwargs_from_reference(kw, ["state", "target"])


def test_layer_table_and_flat_layout():
    gold = json.load(open(os.path.join(GOLD, "sep_keys.json")))
    for form in FORMS:
        ext, pi, vf, vext, act = FORMS[form]
        pol = policy(form)
        assert pol.n_params == gold[form]["n_params"], form
        sides = [(ly.side, ly.ext) for ly in pol.layers]
        n_pe, n_ve = sum(len(v) for v in ext.values()), sum(len(v) for v in vext.values())
        assert sides == [("pi", True)] * n_pe + [("vf", True)] * n_ve + [("pi", False)] * (len(pi) + 1) + [("vf", False)] * (len(vf) + 1)
        offs = [ly.w_off for ly in pol.layers]
        assert offs == sorted(offs) and offs[0] == 0 and pol.log_std_off == pol.n_params - 4 == pol.n_total - 4
        assert pol.obs_keys == ["state", "target"] and pol.spec["vf_extractor"] == vext and "vf_extractor_activation" not in pol.spec
        # the pi side keeps the names of a shared network, the vf side has its own; no buffer is read by both trunks
        assert {ly.dst for ly in pol.layers if ly.side == "pi" and ly.ext} <= {"feat", "x:state:0"}
        assert {ly.dst for ly in pol.layers if ly.side == "vf" and ly.ext} == {"vfeat", "vx:state:0"}
        first = {t: next(ly for ly in pol.layers if ly.dst == t + ":0") for t in ("pi", "vf")}
        assert (first["pi"].src, first["pi"].K) == ("feat", pol.widths["feat"]) and (first["vf"].src, first["vf"].K) == ("vfeat", pol.widths["vfeat"])
        assert pol.widths["vfeat"] == 64 and pol.widths["feat"] == 64
        assert pol.bucket_split() == first["pi"].w_off and pol._plan is not None
    other = policy("asym")
    from visfly_amd.ppo import MlpPolicy
    diff = MlpPolicy(DIMS, {"state": [64]}, [32, 32], [64], "cpu", vf_extractor=ST, extractor_activation="relu", vf_extractor_activation="elu")
    assert diff.spec["vf_extractor_activation"] == "elu" and [ly.relu for ly in diff.layers if ly.side == "vf" and ly.ext] == [3, 3, 3]
    assert [ly.relu for ly in other.layers if ly.side == "vf" and ly.ext] == [1, 1, 1]
    # a vf side that reads a key the pi side does not: appended to the inputs
    assert MlpPolicy(DIMS, {"target": [32]}, [32], [32], "cpu", vf_extractor={"state": [32]}).obs_keys == ["target", "state"]


def test_combinations_that_are_not_implemented_say_so():
    from visfly_amd.ppo import MlpPolicy
    mk = lambda **kw: MlpPolicy({**DIMS, "action": 4}, {"state": [64]}, [32], [32], "cpu", vf_extractor={"state": [64]}, **kw)
    with pytest.raises(NotImplementedError, match="passthrough"):
        mk(passthrough=("action",), head_dims=(1, 1), log_std_param=False)
    with pytest.raises(NotImplementedError, match=r"head_dims \(4, 4\)"):
        mk(head_dims=(4, 4), log_std_param=False)
    with pytest.raises(NotImplementedError, match="log_std_param=False"):
        mk(log_std_param=False)
    with pytest.raises(NotImplementedError, match="layer_norm"):
        mk(layer_norm=dict(pi=True))
    mk(layer_norm=dict(pi=False, vf=False))          # all flags false: no LayerNorm


@pytest.mark.parametrize("form", list(FORMS))
def test_archive_names_and_shapes_equal_the_reference(form):
    from visfly_amd import checkpoint
    gold = json.load(open(os.path.join(GOLD, "sep_keys.json")))[form]
    sd = checkpoint.policy_state_dict(policy(form))
    assert {k: list(v.shape) for k, v in sd.items()} == gold["shapes"], sorted(set(sd) ^ set(gold["shapes"]))
    for k, first in gold["alias"].items():      # SB3 registers the pi side's module under both names (share_features_extractor=False)
        assert torch.equal(sd[k], sd[first])
    assert all(k.startswith("features_extractor.") for k in gold["unused"])


def load_fixture(form, device="cpu"):
    """the policy of `form` with the fixture's parameters, loaded by their reference names -> (policy, fixture arrays of that form)"""
    from visfly_amd import checkpoint
    z = np.load(os.path.join(GOLD, "sep_extractor.npz"))
    fx = {k[len(form) + 1:]: z[k] for k in z.files if k.startswith(form + ":")}
    pol = policy(form, seed=5, device=device)
    sd = {k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param:")}
    assert checkpoint.load_policy_state_dict(pol, sd, strict=True) == []
    return pol, fx


def squashed_log_prob(mean, log_std, actions):
    """SB3 SquashedDiagGaussianDistribution.log_prob(actions) with gaussian_actions=None, in the precision of its arguments"""
    eps = torch.finfo(actions.dtype).eps
    g = torch.atanh(actions.clamp(-1 + eps, 1 - eps))
    lp = torch.distributions.Normal(mean, log_std.exp().expand_as(mean)).log_prob(g).sum(dim=1)
    return lp - torch.log(1 - actions ** 2 + 1e-6).sum(dim=1)


@pytest.mark.parametrize("form", list(FORMS))
def test_fixture_parameters_reproduce_the_reference_and_its_gradient(form):
    from visfly_amd import checkpoint
    pol, fx = load_fixture(form)
    assert bool(fx["entropy_is_none"])        # (the squashed Gaussian has no analytical entropy: nothing to compare)
    back = checkpoint.policy_state_dict(pol)
    gold = json.load(open(os.path.join(GOLD, "sep_keys.json")))[form]
    for k in back:
        if k not in gold["unused"]:
            assert torch.equal(back[k], torch.from_numpy(fx["param:" + k])), k
    net = pol.to_torch().double()
    obs = {"state": torch.from_numpy(fx["obs_state"]).double(), "target": torch.from_numpy(fx["obs_target"]).double()}
    mean, value = net({k: obs[k] for k in pol.obs_keys})
    lp = squashed_log_prob(mean, net.log_std, torch.from_numpy(fx["actions"]).double())
    for name, got, want, w32 in (("values", value.reshape(-1), fx["values64"], fx["values32"]), ("log_prob", lp, fx["log_prob64"], fx["log_prob32"])):
        own = np.abs(w32.astype(np.float64) - want).max()
        err = np.abs(got.detach().numpy() - want).max()
        print(f"{form} {name}: |to_torch().double() - fp64| {err:.3e}, the fixture's own |fp32 - fp64| {own:.3e}")
        assert own > 0 and err <= 4 * own, (name, err, own)
    # the parameter gradient of sum(values c1) + sum(log_prob c2), block by block against the reference's fp64 autograd
    ((value.reshape(-1) * torch.from_numpy(fx["c1"])).sum() + (lp * torch.from_numpy(fx["c2"])).sum()).backward()
    got = torch.zeros(pol.n_params, dtype=torch.float64)
    for ly, m in zip(pol.layers, net.lin):
        got[ly.w_off:ly.w_off + ly.K * ly.No], got[ly.b_off:ly.b_off + ly.No] = m.weight.grad.reshape(-1), m.bias.grad
    got[pol.log_std_off:] = net.log_std.grad
    want = torch.zeros(pol.n_params, dtype=torch.float64)
    n = 0
    for ly, prefixes in checkpoint._names(pol):
        p = next(p for p in prefixes if "grad64:" + p + ".weight" in fx)
        want[ly.w_off:ly.w_off + ly.K * ly.No] = torch.from_numpy(fx["grad64:" + p + ".weight"]).reshape(-1)
        want[ly.b_off:ly.b_off + ly.No] = torch.from_numpy(fx["grad64:" + p + ".bias"])
        n += ly.K * ly.No + ly.No
    assert n + 4 == pol.n_params == sum(v.size for k, v in fx.items() if k.startswith("grad64:"))
    assert torch.allclose(got[pol.log_std_off:], torch.from_numpy(fx["grad64:log_std"]), rtol=1e-9, atol=1e-12)
    # (the same network in the same precision: the fp32 yardstick of assert_blocks is the reference itself -- the bound is BLOCK_TOL)
    assert_blocks(pol, got, types.SimpleNamespace(grad=want, grad32=want), f"{form}: to_torch().double() vs the reference's fp64 autograd")


def test_chain_shape_source_and_cache_path():
    from visfly_amd import _jit
    ext, pi, vf, vext, _ = FORMS["asym"]
    shared = _jit.shape_of(DIMS, ST, pi, vf)
    assert _jit.shape_of(DIMS, ST, pi, vf, vf_extractor=None) == shared        # without the argument: exactly what it was
    sh = _jit.shape_of(DIMS, ext, pi, vf, vf_extractor=vext)
    assert sh == ((16,), ((2,),), (1, 1), (2,), ("sep", (16, 8), ((2, 1), (1,)), (0, 1), 1)) == policy("asym").chain_shape
    assert sh == _jit.prebuild_shape("sep_asym") and not _jit.is_builtin(sh)
    sym = _jit.shape_of(DIMS, ST, [32], [32], acts=(2, 1), vf_extractor=ST)
    assert sym == policy("sym").chain_shape == _jit.prebuild_shape("sep_nav_tanh") and sym[4] == ("act", 2, 1)
    # a symmetric network is not the shared network of the same sizes: its own name, slug and cache file
    same = _jit.shape_of(DIMS, ST, [32], [32], acts=(2, 1))
    assert _jit.name_of(sym) != _jit.name_of(same) and _jit.path_of(sym) != _jit.path_of(same) and "_sep" in _jit.path_of(sym)
    assert _jit.path_of(sh) != _jit.path_of(_jit.shape_of(DIMS, ext, pi, vf, vf_extractor={"state": [64, 32], "target": [64]}))
    assert not _jit.is_builtin(_jit.shape_of(DIMS, {"state": [128, 64], "target": [128, 64]}, [64, 64], [64, 64],
                                             vf_extractor={"state": [128, 64], "target": [128, 64]}))
    src = _jit.source(sh)
    assert src.count("static constexpr bool VF = false;") == 2 and "struct SpecA" in src and "struct SpecB" in src
    assert '#include "vf_mlp_chain_sep.hpp"' in src and "VF_CHAIN_PLUGIN_SEP_DEFINE(NetA, NetB" in src
    assert "using NetA = vf::SepNet<SpecA, 0, 0, 4, 9, 0, -1, 1>;" in src and "using NetB = vf::SepNet<SpecB, 1, 1, 7, 9, 0, 1, 2>;" in src
    assert "static constexpr int PW[4] = {1, 1, 0, 0};" in src and "static constexpr int PW[4] = {2, 0, 0, 0};" in src
    # each side by today's rules; at most two inputs in all
    assert _jit.shape_of(DIMS, ext, pi, vf, vf_extractor={"state": [48]}) is None
    assert _jit.shape_of(DIMS, {"state": [160]}, pi, vf, vf_extractor=vext) is None
    assert _jit.shape_of({**DIMS, "gate": 1}, {"state": [64], "gate": [32]}, pi, vf, vf_extractor=vext) is None
    assert _jit.shape_of(DIMS, ext, pi, vf, head_dims=(4, 4), vf_extractor=vext) is None
    # no persistent launches for these networks
    assert _jit.ensure_rollout(sh, (1, 1, 0, True)) is False and _jit.ensure_eval(sh, (1, 1, 0, True)) is False
    assert _jit.ensure_bptt(sh, (1, 1, 0, True)) is False


def test_plugin_compiles_for_gfx950_and_loads():
    """hipcc cross-compiles the separate-extractor plugin without a GPU (cached by the build); the registry takes it"""
    from visfly_amd import _jit, _lib
    lib = _lib.lib()
    sh = _jit.prebuild_shape("sep_asym")
    path = _jit.build(sh)
    assert os.path.exists(path)
    _lib.check(lib.vf_chain_plugin_load(path.encode()))
    assert _jit.name_of(sh).encode() in [lib.vf_chain_plugin_name(i) for i in range(lib.vf_chain_plugin_count())]


def test_a_policy_without_the_argument_is_unchanged():
    from visfly_amd import _jit
    from visfly_amd.ppo import MlpPolicy
    a = MlpPolicy(DIMS, ST, [32], [32], "cpu", seed=3, activation="tanh")
    b = MlpPolicy(DIMS, ST, [32], [32], "cpu", seed=3, activation="tanh", vf_extractor=None, vf_extractor_activation=None)
    assert a.spec == b.spec == dict(extractor=ST, pi=[32], vf=[32], activation="tanh", extractor_activation="relu")
    assert a.n_params == b.n_params == 13 * 64 + 64 + 64 * 32 + 32 + 3 * 32 + 32 + 2 * (64 * 32 + 32) + 32 * 4 + 4 + 32 + 1 + 4
    assert a.chain_shape == b.chain_shape == _jit.shape_of(DIMS, ST, [32], [32], acts=(2, 1)) == ((16, 8), ((2, 1), (1,)), (1,), (1,), ("act", 2, 1))
    assert torch.equal(a.flat, b.flat) and not a.sep and all(ly.side is None for ly in a.layers)
    assert [(ly.src, ly.dst, ly.w_off) for ly in a.layers] == [(ly.src, ly.dst, ly.w_off) for ly in b.layers]
    assert [ly.dst for ly in a.layers if ly.ext] == ["x:state:0", "feat", "feat"] and a.obs_keys == ["state", "target"]


def test_archive_and_trainer_must_agree_about_the_separate_extractor():
    from visfly_amd import checkpoint
    from visfly_amd.ppo import MlpPolicy
    sep = policy("sym")
    shared = MlpPolicy(DIMS, ST, [32], [32], "cpu", activation="tanh")
    with pytest.raises(ValueError, match="vf_extractor"):
        checkpoint.check_separate_extractors(shared, sep.spec)
    with pytest.raises(ValueError, match="vf_extractor"):
        checkpoint.check_separate_extractors(sep, shared.spec)
    with pytest.raises(ValueError, match="vf_extractor"):
        checkpoint.check_separate_extractors(sep, dict(sep.spec, vf_extractor={"state": [64, 32], "target": [64]}))
    checkpoint.check_separate_extractors(sep, dict(sep.spec))
    checkpoint.check_separate_extractors(shared, dict(shared.spec))
    checkpoint.check_separate_extractors(shared, None)
    # a state_dict of the shared network lacks the vf side's tensors: nothing is copied
    before = sep.flat.clone()
    sd = {k: v for k, v in checkpoint.policy_state_dict(shared).items() if not k.startswith("vf_features_extractor")}
    with pytest.raises(KeyError, match="vf_features_extractor"):
        checkpoint.load_policy_state_dict(sep, sd)
    assert torch.equal(sep.flat, before)


class _Env:
    """what a trainer's constructor reads of an env before it builds its policy"""
    device, num_envs, _is_initial = torch.device("cpu"), 4, True
    tensor_output = requires_grad = False

    def get_observation(self):
        return {"state": torch.zeros(4, 13), "target": torch.zeros(4, 3)}

    def set_requires_grad(self, on, horizon=None):
        self.requires_grad = on


# BPTT's own actor (policy=None) takes the actor-critic policy's kwargs: both forms reach it.  The td policies (BPTT with a policy name,
# SHAC) read share_features_extractor as THEIR flag (the critic runs the actor's extractor), so only the side classes are a request
@pytest.mark.parametrize("trainer,policy_name,form", [("BPTT", None, "sym"), ("BPTT", None, "asym"), ("BPTT", "MlpPolicy", "asym"),
                                                      ("SHAC", None, "asym")])
def test_bptt_and_shac_say_that_they_do_not_run_such_networks(trainer, policy_name, form):
    from visfly_amd import bptt, shac
    cls = {"BPTT": bptt.BPTT, "SHAC": shac.SHAC}[trainer]
    with pytest.raises(NotImplementedError, match=trainer + ".*(separate|pi_features_extractor_class)"):
        cls(_Env(), policy=policy_name, policy_kwargs=reference_kwargs(form))
