"""StateGateExtractor (utils/policies/extractors.py:752-761: StateExtractor plus an MLP over the racing envs' "gate" index) on the host side:
the translation of the reference's policy_kwargs, the layer table MlpPolicy builds for the two branches, and the archive names and shapes
against fixtures read off the reference's own module (tests/golden/gate_keys.json, gate_extractor.npz: tools/gen_gate_golden.py)."""
import json
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIMS = {"state": 16, "gate": 1}
EXT = {"state": [64, 32], "gate": [32]}
PI = VF = [32]


class StateGateExtractor:        # stands for the reference's class object: only its name is read
    pass


def reference_kwargs(cls="StateGateExtractor", **gate_flags):
    return dict(features_extractor_class=cls,
                features_extractor_kwargs=dict(net_arch=dict(state=dict(layer=[64, 32]), gate=dict(layer=[32], **gate_flags))),
                net_arch=dict(pi=[32], vf=[32]), activation_fn="relu")


@pytest.mark.parametrize("cls", ["StateGateExtractor", StateGateExtractor], ids=["string", "class"])
def test_translation_names_the_gate_branch(cls):
    from visfly_amd import checkpoint
    pk = checkpoint.policy_kwargs_from_reference(reference_kwargs(cls), ["state", "gate"])
    assert pk["extractor"] == EXT and list(pk["extractor"]) == ["state", "gate"]
    assert (pk["pi"], pk["vf"]) == (PI, VF) and "layer_norm" not in pk
    assert checkpoint._EXTRACTORS["StateGateExtractor"] == ("state", "gate")
    assert checkpoint.extractor_keys(reference_kwargs(cls), ["state", "gate"]) == ("state", "gate")


def test_gate_flags_behave_like_the_other_branches():
    from visfly_amd import checkpoint
    pk = checkpoint.policy_kwargs_from_reference(reference_kwargs(ln=True), ["state", "gate"])
    assert pk["layer_norm"] == dict(extractor={"state": False, "gate": True}, pi=False, vf=False)
    with pytest.raises(NotImplementedError, match="batch norm"):
        checkpoint.policy_kwargs_from_reference(reference_kwargs(bn=True), ["state", "gate"])


def test_an_env_without_gate_is_refused():
    from visfly_amd import checkpoint
    with pytest.raises(ValueError, match="needs observation keys"):
        checkpoint.policy_kwargs_from_reference(reference_kwargs(), ["state"])


def test_the_other_extractors_keep_their_keys():
    from visfly_amd import checkpoint
    assert checkpoint.extractor_keys(None, ["state", "gate"]) == ("state",)
    assert checkpoint.extractor_keys({}, ["state", "target"]) == ("state", "target")
    assert checkpoint.extractor_keys(dict(features_extractor_class="StateExtractor"), ["state", "target"]) == ("state",)
    assert checkpoint.extractor_keys(dict(extractor={"state": [64], "gate": [32]}), ["state", "gate"]) == ("state", "gate")


def test_trainers_keep_gate_only_when_the_extractor_reads_it():
    from visfly_amd.ppo import policy_rows, trainer_obs_keys
    obs = {"state": torch.zeros(3, 13), "gate": torch.tensor([2, 0, 3], dtype=torch.int32), "depth": torch.zeros(3, 1)}
    assert trainer_obs_keys(obs, None) == ["state"]
    assert trainer_obs_keys(obs, dict(features_extractor_class="StateExtractor")) == ["state"]
    assert trainer_obs_keys(obs, reference_kwargs()) == ["state", "gate"]
    assert trainer_obs_keys({"state": obs["state"], "target": torch.zeros(3, 3)}, None) == ["state", "target"]
    assert trainer_obs_keys({"state": obs["state"]}, reference_kwargs()) == ["state"]        # (the translation then raises: no "gate")
    rows = policy_rows(obs, ["state", "gate"])
    assert rows["gate"].dtype == torch.float32 and rows["gate"].shape == (3, 1) and rows["gate"].reshape(-1).tolist() == [2.0, 0.0, 3.0]
    assert rows["state"] is not None and rows["state"].data_ptr() == obs["state"].data_ptr()
    col = policy_rows({"gate": obs["gate"].reshape(3, 1)}, ["gate"])["gate"]                   # RacingEnv2's (N, 1)
    assert torch.equal(col, rows["gate"])


def _policy(seed=1):
    from visfly_amd.ppo import MlpPolicy
    return MlpPolicy(DIMS, EXT, PI, VF, "cpu", seed=seed)


def test_layer_table_of_the_two_branches():
    pol = _policy()
    first = [ly for ly in pol.layers if ly.first]
    assert [(ly.src, ly.K, ly.No) for ly in first] == [("obs:state", 16, 64), ("obs:gate", 1, 32)]
    into_feat = [(ly.src, ly.dc, ly.No) for ly in pol.layers if ly.dst == "feat"]
    assert into_feat == [("x:state:0", 0, 32), ("obs:gate", 32, 32)]
    assert pol.widths["feat"] == 64 and pol.obs_keys == ["state", "gate"] and pol.obs_dims == DIMS
    assert pol.spec["extractor"] == EXT
    from visfly_amd import _jit
    assert pol.chain_shape == ((16, 8), ((2, 1), (1,)), (1,), (1,)) == _jit.prebuild_shape("gate_pi")


def test_state_dict_names_and_shapes_match_the_reference():
    from visfly_amd import checkpoint
    gold = json.load(open(os.path.join(GOLD, "gate_keys.json")))
    assert gold.pop("features_dim") == 64
    sd = checkpoint.policy_state_dict(_policy())
    ours = {k: list(v.shape) for k, v in sd.items() if k.startswith("features_extractor.")}
    assert ours == gold, sorted(set(ours) ^ set(gold))
    for k in gold:       # SB3's aliases of a shared extractor carry the branch too
        for alias in ("pi_", "vf_"):
            assert torch.equal(sd[alias + k], sd[k]), alias + k


def test_fixture_parameters_round_trip_and_reproduce_the_reference_output():
    from visfly_amd import checkpoint
    z = np.load(os.path.join(GOLD, "gate_extractor.npz"))
    pol = _policy()
    sd = checkpoint.policy_state_dict(pol)
    n = 0
    for k in z.files:
        if k.startswith("param:"):
            t = torch.from_numpy(z[k])
            for alias in ("", "pi_", "vf_"):
                assert alias + k[6:] in sd and sd[alias + k[6:]].shape == t.shape, alias + k[6:]
                sd[alias + k[6:]] = t
            n += 1
    assert n == 6
    checkpoint.load_policy_state_dict(pol, sd, strict=True)
    back = checkpoint.policy_state_dict(pol)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    gate_layer = next(ly for ly in pol.layers if ly.src == "obs:gate")
    assert torch.equal(pol.weight(gate_layer), torch.from_numpy(z["param:features_extractor.gate_extractor.0.weight"]))
    # the torch replica of the layer table on obs.float() against the module's own features
    gate = z["obs_gate"]
    assert gate.dtype == np.int32 and gate.shape == (64, 1) and sorted(set(gate.reshape(-1).tolist())) == [0, 1, 2, 3]
    net = pol.to_torch()
    with torch.no_grad():
        net({"state": torch.from_numpy(z["obs_state"]), "gate": torch.from_numpy(gate).float()})
    w32, w64 = z["features32"].astype(np.float64), z["features64"]
    own = np.abs(w32 - w64).max()
    err = np.abs(net.acts["feat"].double().numpy() - w64).max()
    print(f"features: |to_torch - fp64| {err:.3e}, the fixture's own |fp32 - fp64| {own:.3e}")
    assert own > 0 and err <= 4 * own, (err, own)


def test_archive_and_policy_must_agree_about_the_branch():
    from visfly_amd import checkpoint
    from visfly_amd.ppo import MlpPolicy
    gated = _policy()
    # the same feature width without the branch: every trunk shape agrees, the state branch's last layer does not
    plain = MlpPolicy({"state": 16}, {"state": [64, 64]}, PI, VF, "cpu", seed=1)
    narrow = MlpPolicy({"state": 16}, {"state": [64, 32]}, PI, VF, "cpu", seed=1)
    for other in (plain, narrow):
        before = other.flat.clone()
        with pytest.raises(ValueError, match="shape"):
            checkpoint.load_policy_state_dict(other, checkpoint.policy_state_dict(gated))
        assert torch.equal(other.flat, before), "a refused state_dict must leave the policy as it was"
        # the reverse: the shape ValueError as well (shapes are checked before missing names are reported)
        mine = _policy()
        before = mine.flat.clone()
        with pytest.raises(ValueError, match="shape"):
            checkpoint.load_policy_state_dict(mine, checkpoint.policy_state_dict(other))
        assert torch.equal(mine.flat, before)
    # a state_dict that merely lacks the branch's tensors (every tensor it has fits): the existing KeyError, nothing copied
    sd = {k: v for k, v in checkpoint.policy_state_dict(gated).items() if "gate_extractor" not in k}
    mine = _policy(seed=3)
    before = mine.flat.clone()
    with pytest.raises(KeyError, match="gate_extractor"):
        checkpoint.load_policy_state_dict(mine, sd)
    assert torch.equal(mine.flat, before)


def test_no_gradient_is_planned_for_the_gate_column():
    """the reverse layer table hands out an observation gradient for "state" only; the gate branch's input tile goes to a buffer of the
    policy's own that is not among the returned gradients (a "target" branch keeps its gradient)"""
    from visfly_amd.ppo import MlpPolicy
    M = 8
    pol = _policy()
    dm, dv = torch.zeros(M, 4), torch.zeros(M, 1)
    pol._buffers(M, 0).update({"obs:state": torch.zeros(M, 16), "obs:gate": torch.zeros(M, 1)})       # (what forward() leaves there)
    d, d_in = pol._bwd_desc(pol._buffers(M, 0), M, dm, dv, True)
    assert sorted(d_in) == ["state"] and d_in["state"].shape == (M, 16)
    entries = {(e.K, e.No): e for e in (d.layer[i] for i in range(d.n_layers))}
    gate, state = entries[(1, 32)], entries[(16, 64)]
    assert state.dX == d_in["state"].data_ptr() and gate.need_dx and gate.dX == pol._index_sink(M, 1).data_ptr() != state.dX
    _, none = pol._bwd_desc(pol._buffers(M, 0), M, dm, dv, False)
    assert none == {}
    nav = MlpPolicy({"state": 13, "target": 3}, {"state": [64, 32], "target": [32]}, PI, VF, "cpu", seed=1)
    nav._buffers(M, 0).update({"obs:state": torch.zeros(M, 13), "obs:target": torch.zeros(M, 3)})
    assert sorted(nav._bwd_desc(nav._buffers(M, 0), M, dm, dv, True)[1]) == ["state", "target"]
