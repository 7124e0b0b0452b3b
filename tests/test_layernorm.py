"""LayerNorm in the extractor and trunk MLPs (create_mlp's ``ln``), the parts that need no GPU: the plain restatements the GPU tests
check the kernels against (tests/_ln_ref.py) and what their comparators can tell apart, the translation of the reference's
``ln`` / ``pi_ln`` / ``vf_ln`` flags, MlpPolicy's parameter layout with and without ``layer_norm``, and the checkpoint names, shapes
and optimiser order against fixtures read off the reference's own modules (tools/gen_ln_golden.py)."""
import json
import os

import numpy as np
import pytest
import torch

import _ln_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TORCH_ACT = {0: torch.nn.Identity, 1: torch.nn.ReLU, 2: torch.nn.Tanh, 3: torch.nn.ELU, 4: torch.nn.LeakyReLU}
# (M, W) of the host runs of the comparators: the GPU test's input generator at a few of its shapes, and its variance rows
HOST_SHAPES = [(65, 4), (63, 33), (64, 48), (65, 64), (257, 200), (3, 512)]


# ---------------------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_restatements_equal_fp64_autograd_of_torch_layernorm(kind):
    W, M = 48, 37
    inp = R.ln_inputs(M, W, kind)
    z = torch.from_numpy(inp["z"]).double().requires_grad_(True)
    net = torch.nn.Sequential(torch.nn.LayerNorm(W, eps=1e-3), TORCH_ACT[kind]()).double()
    with torch.no_grad():
        net[0].weight.copy_(torch.from_numpy(inp["gamma"]).double())
        net[0].bias.copy_(torch.from_numpy(inp["beta"]).double())
    y = net(z)
    (y * torch.from_numpy(inp["dy"]).double()).sum().backward()
    f = R.ln_fwd(inp["z"], inp["gamma"], inp["beta"], kind, R.F64, 1e-3)
    assert np.allclose(f["y"], y.detach().numpy(), rtol=1e-12, atol=1e-13)
    # the backward restatement from ITS OWN forward's saved arrays, all in fp64
    b = R.ln_bwd(inp["dy"], f["y"], f["xhat"], f["rstd"], inp["gamma"], kind, R.F64)
    assert np.allclose(b["dz"], z.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(b["dgamma"], net[0].weight.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(b["dbeta"], net[0].bias.grad.numpy(), rtol=1e-10, atol=1e-12)


def _got(d):
    return {k: R.padded(v) for k, v in d.items()}


@pytest.mark.parametrize("M,W", HOST_SHAPES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_fp32_restatement_passes_every_comparator(M, W, kind):
    for vr in ((False, True) if M >= 3 else (False,)):
        inp = R.ln_inputs(M, W, kind, variance_rows=vr)
        R.check_fwd(_got(R.fwd_refs(inp)[0]), inp)
        R.check_bwd(_got(R.bwd_refs(inp)[0]), inp)
        R.check_bwd(_got(R.bwd_refs(inp, init=5.0)[0]), inp, init=5.0)


def test_a_written_pad_is_caught():
    inp = R.ln_inputs(5, 8, 2)
    got = _got(R.fwd_refs(inp)[0])
    got["y"][-R.PAD] = 0.0
    with pytest.raises(AssertionError, match="pad"):
        R.check_fwd(got, inp)


def _fwd_mutant(inp, which):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    z, gamma, beta, kind = t(inp["z"]), t(inp["gamma"]), t(inp["beta"]), inp["kind"]
    W = z.shape[1]
    eps = float(np.float32(1e-5 if which == "eps" else R.EPS))
    mean = z.sum(dim=1, keepdim=True) / W
    if which == "one_pass":
        var = (z * z).sum(dim=1, keepdim=True) / W - mean * mean
    elif which == "unbiased":
        var = ((z - mean) ** 2).sum(dim=1, keepdim=True) / (W - 1)
    else:
        var = ((z - mean) ** 2).sum(dim=1, keepdim=True) / W
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mean) * rstd
    return {"y": R.act_fwd(gamma * xhat + beta, kind).numpy(), "xhat": xhat.numpy(), "rstd": rstd.view(-1).numpy()}


def _bwd_mutant(inp, which):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    dy, y, xhat, rstd, gamma, kind = t(inp["dy"]), t(inp["y"]), t(inp["xhat"]), t(inp["rstd"]).view(-1, 1), t(inp["gamma"]), inp["kind"]
    g = R.act_mul(dy, y, kind) if kind else dy
    W = dy.shape[1]
    h = g if which == "no_gamma" else g * gamma
    m1 = h.sum(dim=1, keepdim=True) / W
    m2 = (h * xhat).sum(dim=1, keepdim=True) / W
    dz = rstd * (h - m1 - (0.0 if which == "no_m2" else xhat * m2))
    dgamma = g.sum(dim=0) if which == "dgamma_no_xhat" else (g * xhat).sum(dim=0)
    return {"dz": dz.numpy(), "dgamma": dgamma.numpy(), "dbeta": g.sum(dim=0).numpy()}


@pytest.mark.parametrize("which", ["one_pass", "unbiased", "eps"])
def test_forward_mutants_fail_a_comparator(which):
    """over the GPU test's inputs (its variance rows among them), per activation kind: no mutant passes them all"""
    for kind in R.KINDS:
        failed = 0
        for M, W in HOST_SHAPES:
            for vr in ((False, True) if M >= 3 else (False,)):
                inp = R.ln_inputs(M, W, kind, variance_rows=vr)
                with np.errstate(all="ignore"):
                    got = _got(_fwd_mutant(inp, which))
                try:
                    R.check_fwd(got, inp)
                except AssertionError:
                    failed += 1
        assert failed > 0, (which, kind)
    # the row of 1000 + N(0, 1) is what the one-pass variance is caught by even where the other rows let it through
    inp = R.ln_inputs(65, 64, 2, variance_rows=True)
    if which == "one_pass":
        with pytest.raises(AssertionError):
            with np.errstate(all="ignore"):
                R.check_fwd(_got(_fwd_mutant(inp, which)), inp)


@pytest.mark.parametrize("which", ["no_gamma", "no_m2", "dgamma_no_xhat"])
def test_backward_mutants_fail_a_comparator(which):
    for kind in R.KINDS:
        for M, W in HOST_SHAPES:
            inp = R.ln_inputs(M, W, kind)
            with pytest.raises(AssertionError):
                R.check_bwd(_got(_bwd_mutant(inp, which)), inp)


# ---------------------------------------------------------------------------------------------------------------------------
# translation of the reference's policy_kwargs
# ---------------------------------------------------------------------------------------------------------------------------
def _pk(state_ln=None, target_ln=None, pi_ln=None, vf_ln=None, **extra):
    arch = {"state": {"layer": [128, 64]}, "target": {"layer": [96, 32]}}
    if state_ln is not None:
        arch["state"]["ln"] = state_ln
    if target_ln is not None:
        arch["target"]["ln"] = target_ln
    na = dict(pi=[64, 48], vf=[64, 64])
    if pi_ln is not None:
        na["pi_ln"] = pi_ln
    if vf_ln is not None:
        na["vf_ln"] = vf_ln
    na.update(extra)
    return dict(features_extractor_class="StateTargetExtractor", features_extractor_kwargs=dict(net_arch=arch), net_arch=na)


def test_translation_of_ln_flags():
    from visfly_amd.checkpoint import policy_kwargs_from_reference as tr
    keys = ["state", "target"]
    out = tr(_pk(state_ln=True, pi_ln=True, vf_ln=True), keys)
    assert out["layer_norm"] == dict(extractor={"state": True, "target": False}, pi=True, vf=True)
    # create_mlp tests the flag's truthiness once for the whole MLP: a non-empty list normalises every layer, whatever it holds
    out = tr(_pk(state_ln=[True, False], target_ln=[False], pi_ln=[True, False], vf_ln=[]), keys)
    assert out["layer_norm"] == dict(extractor={"state": True, "target": True}, pi=True, vf=False)
    out = tr(_pk(vf_ln=True), keys)
    assert out["layer_norm"] == dict(extractor={"state": False, "target": False}, pi=False, vf=True)
    for pk in (_pk(), _pk(state_ln=False, target_ln=False, pi_ln=False, vf_ln=False), _pk(state_ln=[], pi_ln=[], vf_ln=0)):
        assert "layer_norm" not in tr(pk, keys)
    assert tr(_pk(state_ln=True), keys)["extractor"] == {"state": [128, 64], "target": [96, 32]}


def test_bn_flags_still_raise():
    from visfly_amd.checkpoint import policy_kwargs_from_reference as tr
    keys = ["state", "target"]
    for pk in (_pk(pi_bn=True), _pk(vf_bn=True), _pk(pi_bn=[True], pi_ln=True)):
        with pytest.raises(NotImplementedError):
            tr(pk, keys)
    pk = _pk(state_ln=True)
    pk["features_extractor_kwargs"]["net_arch"]["state"]["bn"] = True        # in create_mlp bn wins over ln
    with pytest.raises(NotImplementedError):
        tr(pk, keys)


# ---------------------------------------------------------------------------------------------------------------------------
# MlpPolicy: parameter layout
# ---------------------------------------------------------------------------------------------------------------------------
DIMS = {"state": 13, "target": 3}
EXT = {"state": [128, 64], "target": [96, 32]}
PI, VF = [64, 48], [64, 64]


def _closed_form():
    """[(K, No)] in schedule order: extractor branches, policy trunk + action head, value trunk + value head"""
    shapes = []
    for k, hidden in EXT.items():
        K = DIMS[k]
        for h in hidden:
            shapes.append((K, h))
            K = h
    feat = sum(v[-1] for v in EXT.values())
    for hidden, head in ((PI, 4), (VF, 1)):
        K = feat
        for h in hidden + [head]:
            shapes.append((K, h))
            K = h
    return shapes


def test_policy_without_layer_norm_is_unchanged():
    from visfly_amd.ppo import MlpPolicy
    shapes = _closed_form()
    for kw in ({}, dict(layer_norm=None), dict(layer_norm=dict(extractor={"state": False}, pi=False, vf=False))):
        pol = MlpPolicy(DIMS, EXT, PI, VF, "cpu", seed=3, **kw)
        off = 0
        assert len(pol.layers) == len(shapes)
        for ly, (K, No) in zip(pol.layers, shapes):
            assert (ly.K, ly.No, ly.w_off, ly.b_off) == (K, No, off, off + K * No) and not ly.ln
            off += K * No + No
        assert pol.log_std_off == off == sum(K * No + No for K, No in shapes) and pol.n_params == off + 4
        assert pol.spec == dict(extractor=EXT, pi=PI, vf=VF)
        assert not pol.ln and pol._plan is not None
    a = MlpPolicy(DIMS, EXT, PI, VF, "cpu", seed=3)
    b = MlpPolicy(DIMS, EXT, PI, VF, "cpu", seed=3, layer_norm=dict(pi=False))
    assert torch.equal(a.flat, b.flat)


def test_policy_with_layer_norm_layout():
    from visfly_amd.ppo import MlpPolicy
    shapes = _closed_form()
    normed = [True, True, False, False, True, True, False, False, False, False]      # state branch, policy trunk; heads never
    pol = MlpPolicy(DIMS, EXT, PI, VF, "cpu", seed=3, layer_norm=dict(extractor={"state": True}, pi=True), activation="tanh")
    off = 0
    for ly, (K, No), ln in zip(pol.layers, shapes, normed):
        assert (ly.K, ly.No, ly.w_off, ly.b_off, ly.ln) == (K, No, off, off + K * No, ln), ly.dst
        off += K * No + No
        if ln:
            assert (ly.g_off, ly.be_off) == (off, off + No)
            assert bool((pol.flat[ly.g_off:ly.g_off + No] == 1).all()) and bool((pol.flat[ly.be_off:ly.be_off + No] == 0).all())
            off += 2 * No
    assert pol.log_std_off == off and pol.n_params == off + 4 and pol.grad.numel() == pol.n_params
    assert pol.ln and pol._plan is None and pol.chain_shape is None
    assert pol.pack_map() == (None, None)
    assert pol.spec["layer_norm"] == dict(extractor={"state": True, "target": False}, pi=True, vf=False)
    # the Linear weights are what the same seed gives without LayerNorm: the norm draws nothing from the generator
    plain = MlpPolicy(DIMS, EXT, PI, VF, "cpu", seed=3, activation="tanh")
    for a, b in zip(pol.layers, plain.layers):
        assert torch.equal(pol.weight(a), plain.weight(b)) and torch.equal(pol.bias(a), plain.bias(b))
    with pytest.raises(ValueError):
        MlpPolicy(DIMS, EXT, PI, VF, "cpu", layer_norm=dict(extractor={"gate": True}))
    with pytest.raises(ValueError):
        MlpPolicy(DIMS, EXT, PI, VF, "cpu", layer_norm=dict(qf=True))


# ---------------------------------------------------------------------------------------------------------------------------
# fixtures read off the reference's modules
# ---------------------------------------------------------------------------------------------------------------------------
def _fixture_policy():
    from visfly_amd.ppo import MlpPolicy
    return MlpPolicy(DIMS, EXT, PI, VF, "cpu", seed=1, layer_norm=dict(extractor={"state": True}, pi=True), activation="tanh")


def test_state_dict_names_and_shapes_match_the_reference():
    from visfly_amd import checkpoint
    gold = json.load(open(os.path.join(GOLD, "ln_keys.json")))
    assert gold.pop("features_dim") == 96
    sd = checkpoint.policy_state_dict(_fixture_policy())
    for k, shape in gold.items():
        assert k in sd, k
        assert list(sd[k].shape) == shape, (k, list(sd[k].shape), shape)
    ours = {k for k in sd if k.startswith(("features_extractor.", "mlp_extractor.policy_net."))}
    assert ours == set(gold), sorted(ours ^ set(gold))
    # the value trunk is not normalised: Linear 2 i
    assert {"mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.2.weight"} <= set(sd) and "mlp_extractor.value_net.1.weight" not in sd
    # SB3's aliases of a shared extractor carry the LayerNorm too
    assert torch.equal(sd["pi_features_extractor.state_extractor.1.weight"], sd["features_extractor.state_extractor.1.weight"])


def test_fixture_parameters_reproduce_the_reference_output():
    from visfly_amd import checkpoint
    z = np.load(os.path.join(GOLD, "ln_create_mlp.npz"))
    pol = _fixture_policy()
    sd = checkpoint.policy_state_dict(pol)
    n = 0
    for k in z.files:
        if k.startswith("param:"):
            t = torch.from_numpy(z[k])
            for alias in ("", "pi_", "vf_"):
                name = alias + k[6:] if k[6:].startswith("features_extractor") else k[6:]
                assert name in sd and sd[name].shape == t.shape, name
                sd[name] = t
            n += 1
    assert n == 20
    checkpoint.load_policy_state_dict(pol, sd, strict=True)
    back = checkpoint.policy_state_dict(pol)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    ly = pol.layers[0]
    assert torch.equal(pol.ln_weight(ly), torch.from_numpy(z["param:features_extractor.state_extractor.1.weight"]))
    assert not bool((pol.ln_weight(ly) == 1).all())
    net = pol.to_torch()
    with torch.no_grad():
        net({"state": torch.from_numpy(z["obs_state"]), "target": torch.from_numpy(z["obs_target"])})
    for name, got in (("features", net.acts["feat"]), ("latent_pi", net.acts["pi:1"])):
        w32, w64 = z[name + "32"].astype(np.float64), z[name + "64"]
        own = np.abs(w32 - w64).max()
        err = np.abs(got.double().numpy() - w64).max()
        print(f"{name}: |to_torch - fp64| {err:.3e}, the fixture's own |fp32 - fp64| {own:.3e}")
        assert own > 0 and err <= 4 * own, (name, err, own)


def test_param_order_follows_registration_order():
    from visfly_amd import checkpoint
    pol = _fixture_policy()
    order = checkpoint._param_order(pol)
    assert order[0] == (pol.log_std_off, (4,))
    by = {ly.dst + ":" + str(ly.dc): ly for ly in pol.layers}
    s0, s1, t0, t1 = by["x:state:0:0"], by["feat:0"], by["x:target:0:0"], by["feat:64"]
    p0, p1, v0, v1, mean, value = by["pi:0:0"], by["pi:1:0"], by["vf:0:0"], by["vf:1:0"], by["mean:0"], by["value:0"]
    lin = lambda ly: [(ly.w_off, (ly.No, ly.K)), (ly.b_off, (ly.No,))]
    norm = lambda ly: [(ly.g_off, (ly.No,)), (ly.be_off, (ly.No,))]
    want = (lin(s0) + norm(s0) + lin(s1) + norm(s1) + lin(t0) + lin(t1) + lin(p0) + norm(p0) + lin(p1) + norm(p1)
            + lin(v0) + lin(v1) + lin(mean) + lin(value))
    assert order[1:] == want
    # every trainable parameter exactly once
    cover = np.zeros(pol.n_params, np.int32)
    for off, shape in order:
        cover[off:off + int(np.prod(shape))] += 1
    assert (cover == 1).all()


def test_archive_layer_norm_must_match_the_policy():
    from visfly_amd import checkpoint
    pol = _fixture_policy()
    checkpoint.check_layer_norm(pol, dict(pol.spec))
    from visfly_amd.ppo import MlpPolicy
    plain = MlpPolicy(DIMS, EXT, PI, VF, "cpu", seed=1, activation="tanh")
    checkpoint.check_layer_norm(plain, dict(plain.spec))
    with pytest.raises(ValueError, match="layer_norm"):
        checkpoint.check_layer_norm(plain, dict(pol.spec))
    with pytest.raises(ValueError, match="layer_norm"):
        checkpoint.check_layer_norm(pol, dict(plain.spec))
    # a state_dict without the LayerNorm tensors cannot be loaded into a normalised policy, nor the reverse
    with pytest.raises(KeyError):
        checkpoint.load_policy_state_dict(pol, checkpoint.policy_state_dict(plain))
    with pytest.raises(KeyError):
        checkpoint.load_policy_state_dict(plain, checkpoint.policy_state_dict(pol))
