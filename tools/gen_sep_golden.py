#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden-vector generator for actor-critic policies with separate pi / vf feature extractors.  Runs ONLY where the
reference is importable.

The reference's ``CustomMultiInputActorCriticPolicy`` (utils/policies/policies.py:117-175,210-215,244-249,296-308) builds such a network
in two forms:

* ``sym``: ``share_features_extractor=False`` next to ``features_extractor_class=StateTargetExtractor`` -- SB3 instantiates the class a
  second time for the critic (``features_extractor`` IS ``pi_features_extractor``);
* ``asym``: ``features_extractor_class=None`` with ``pi_features_extractor_class=StateExtractor`` and
  ``vf_features_extractor_class=StateTargetExtractor`` of another ``net_arch`` -- the actor reads "state", the critic "state" and "target".

Two fixtures, data only, read off the reference's own modules:

* tests/golden/sep_keys.json: per form the ``state_dict`` names and shapes, which names share storage (``alias``), which parameters no
  output depends on (``unused``: the pi-class module SB3 leaves under ``features_extractor`` in the second form) and the number of
  parameters the outputs do depend on (``n_params``).
* tests/golden/sep_extractor.npz: per form the parameters (biases moved off their default draw), 64 observation rows and 64 actions,
  ``evaluate_actions`` -> values / log-prob (the squashed Gaussian has no analytical entropy: the reference returns None, recorded as the
  flag ``entropy_is_none``) in fp32 and from a ``.double()`` copy, and the fp64 parameter gradient of
  ``sum(values c1) + sum(log_prob c2)`` for recorded c1, c2.

The stubs that make the reference's policy package importable without its simulator are oracle/gen_golden.py's own; the SB3 restatement is
oracle/gen_ppo_loop.py's (``_install_ppo_sb3``), imported, not edited.

Usage:  python tools/gen_sep_golden.py [--out DIR]
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gen_golden as GG  # noqa: E402  (stubs, import_envs)
import gen_ppo_loop as GP  # noqa: E402  (_install_ppo_sb3)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402
import torch.nn as nn  # noqa: E402

ROWS = 64
ST = {"net_arch": {"state": {"layer": [64, 32]}, "target": {"layer": [32]}}, "activation_fn": nn.ReLU}
FORMS = {
    # name: (policy kwargs, label)
    "sym": (lambda E: dict(net_arch=dict(pi=[32], vf=[32]), activation_fn=nn.Tanh, features_extractor_class=E.StateTargetExtractor,
                           features_extractor_kwargs=copy.deepcopy(ST), share_features_extractor=False),
            "StateTargetExtractor twice {state: [64, 32], target: [32]}, pi [32], vf [32], Tanh trunks"),
    "asym": (lambda E: dict(net_arch=dict(pi=[32, 32], vf=[64]), activation_fn=nn.ReLU, features_extractor_class=None,
                            pi_features_extractor_class=E.StateExtractor,
                            pi_features_extractor_kwargs={"net_arch": {"state": {"layer": [64]}}, "activation_fn": nn.ReLU},
                            vf_features_extractor_class=E.StateTargetExtractor, vf_features_extractor_kwargs=copy.deepcopy(ST),
                            share_features_extractor=False),
             "pi StateExtractor {state: [64]}, vf StateTargetExtractor {state: [64, 32], target: [32]}, pi [32, 32], vf [64], ReLU trunks"),
}


def gen(out):
    sp = GP._install_ppo_sb3()
    GG.import_envs()
    import VisFly.utils.policies.extractors as E
    import VisFly.utils.policies.policies as RPOL
    obs_space = sp.Dict({"state": sp.Box(-1, 1, (13,)), "target": sp.Box(-1, 1, (3,))})
    act_space = sp.Box(-1, 1, (4,))
    keys, arrays = {}, {}
    for fi, (form, (kw, label)) in enumerate(FORMS.items()):
        th.manual_seed(20270 + fi)
        policy = RPOL.CustomMultiInputActorCriticPolicy(obs_space, act_space, lr_schedule=lambda _: 1e-3, log_std_init=-0.5, **kw(E))
        assert not policy.share_features_extractor and type(policy.action_dist).__name__ == "SquashedDiagGaussianDistribution"
        assert policy.pi_features_extractor is not policy.vf_features_extractor
        with th.no_grad():       # biases away from their zero / small default draw, the mean head off its 0.01 gain
            for m in policy.modules():
                if isinstance(m, nn.Linear):
                    m.bias.add_(0.1 * th.randn_like(m.bias))
            policy.action_net.weight.mul_(30.0)
        sd = policy.state_dict()
        first = {}
        alias = {}
        for k, v in sd.items():
            if v.data_ptr() in first:
                alias[k] = first[v.data_ptr()]
            else:
                first[v.data_ptr()] = k
        rng = np.random.default_rng(77 + fi)
        obs = {"state": th.from_numpy(rng.normal(size=(ROWS, 13)).astype(np.float32)),
               "target": th.from_numpy(rng.normal(size=(ROWS, 3)).astype(np.float32))}
        actions = th.from_numpy(np.tanh(rng.normal(scale=0.8, size=(ROWS, 4))).astype(np.float32))
        c1 = th.from_numpy(rng.normal(size=ROWS)).double()
        c2 = th.from_numpy(rng.normal(size=ROWS)).double()
        with th.no_grad():
            v32, lp32, ent = policy.evaluate_actions(obs, actions)
        p64 = copy.deepcopy(policy).double()
        v64, lp64, ent64 = p64.evaluate_actions({k: v.double() for k, v in obs.items()}, actions.double())
        ((v64.reshape(-1) * c1).sum() + (lp64 * c2).sum()).backward()
        named = dict(p64.named_parameters(remove_duplicate=False))
        unused = sorted(k for k, p in named.items() if p.grad is None)
        n_params = sum(p.numel() for k, p in named.items() if k not in alias and p.grad is not None)
        keys[form] = dict(label=label, shapes={k: list(v.shape) for k, v in sd.items()}, alias=alias, unused=unused, n_params=int(n_params))
        for k, v in sd.items():
            arrays[f"{form}:param:{k}"] = v.detach().numpy().astype(np.float32)
        for k, p in named.items():
            if p.grad is not None and k not in alias:
                arrays[f"{form}:grad64:{k}"] = p.grad.detach().numpy().astype(np.float64)
        arrays.update({f"{form}:obs_state": obs["state"].numpy(), f"{form}:obs_target": obs["target"].numpy(), f"{form}:actions": actions.numpy(),
                       f"{form}:c1": c1.numpy(), f"{form}:c2": c2.numpy(),
                       f"{form}:values32": v32.reshape(-1).numpy(), f"{form}:log_prob32": lp32.numpy(),
                       f"{form}:values64": v64.detach().reshape(-1).numpy(), f"{form}:log_prob64": lp64.detach().numpy(),
                       f"{form}:entropy_is_none": np.asarray(ent is None and ent64 is None), f"{form}:label": np.asarray("reference " + label)})
        print(f"{form}: {len(sd)} tensors ({len(alias)} aliases, {len(unused)} unused), n_params {n_params}; values |32 - 64| "
              f"{float((v32.reshape(-1).double() - v64.detach().reshape(-1)).abs().max()):.3e}, log_prob |32 - 64| "
              f"{float((lp32.double() - lp64.detach()).abs().max()):.3e}")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "sep_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(out, "sep_extractor.npz"), **arrays)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GG.OUT)
    gen(ap.parse_args().out)
