#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden-vector generator for LayerNorm in create_mlp.  Runs ONLY where the reference is importable.

The reference's ``create_mlp`` (utils/policies/extractors.py:376-449) puts ``nn.LayerNorm(width, eps=1e-3)`` between every hidden
``nn.Linear`` and its activation when ``ln`` is truthy.  Two fixtures, data only, read off the reference's own modules:

* tests/golden/ln_keys.json: ``state_dict`` names and shapes of a ``StateTargetExtractor`` whose ``state`` branch is normalised and
  whose ``target`` branch is not, and of ``create_mlp(96, [64, 48], nn.Tanh, ln=True)`` under the name MlpExtractor2 gives it
  (``mlp_extractor.policy_net``, policies.py:34-49) -- the key pattern visfly_amd/checkpoint.py has to write (Linear 3 i, LayerNorm
  3 i + 1 in a normalised MLP, Linear 2 i otherwise).
* tests/golden/ln_create_mlp.npz: the parameters of those modules (LayerNorm weight / bias perturbed away from 1 / 0, so that a
  consumer that ignores them fails), a 64-row observation, and what the modules compute on it: the extractor's features and the
  policy trunk's output on those features, in fp32 and from the ``.double()`` copies of the same modules.

The stubs that make the reference's policy package importable without its simulator are oracle/gen_golden.py's own.

Usage:  python tools/gen_ln_golden.py [--out DIR]
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gen_golden as GG  # noqa: E402  (stubs, import_envs)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402
import torch.nn as nn  # noqa: E402

NET_ARCH = {"state": {"layer": [128, 64], "ln": True}, "target": {"layer": [96, 32]}}
PI = [64, 48]
ROWS = 64


def gen(out):
    GG.import_envs()
    GG._sb3_stubs()
    import VisFly.utils.policies.extractors as E
    sp = sys.modules["gymnasium.spaces"]
    th.manual_seed(20261)
    space = sp.Dict({"state": sp.Box(-1, 1, (13,)), "target": sp.Box(-1, 1, (3,))})
    ext = E.StateTargetExtractor(space, net_arch=copy.deepcopy(NET_ARCH), activation_fn=nn.ReLU)
    pi_net, pi_dim = E.create_mlp(input_dim=96, layer=list(PI), activation_fn=nn.Tanh, ln=True)
    assert int(ext.features_dim) == 96 and pi_dim == PI[-1]
    mods = (("features_extractor", ext), ("mlp_extractor.policy_net", pi_net))
    n_ln = 0
    with th.no_grad():
        for _, mod in mods:
            for m in mod.modules():
                if isinstance(m, nn.LayerNorm):
                    assert m.eps == 1e-3
                    m.weight.add_(0.3 * th.randn_like(m.weight))
                    m.bias.add_(0.2 * th.randn_like(m.bias))
                    n_ln += 1
    assert n_ln == 4, n_ln       # state branch 2, policy trunk 2, target branch none
    keys, params = {}, {}
    for prefix, mod in mods:
        for k, v in mod.state_dict().items():
            keys[f"{prefix}.{k}"] = list(v.shape)
            params["param:" + f"{prefix}.{k}"] = v.detach().numpy().astype(np.float32)
    keys["features_dim"] = int(ext.features_dim)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "ln_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)

    state, target = th.randn(ROWS, 13), th.randn(ROWS, 3)
    state[0] = 0.25                      # a constant observation row
    state[1] = 1000.0 + th.randn(13)     # a row far from zero

    def run(e, p, s, t):
        with th.no_grad():
            feat = th.cat([e.state_extractor(s), e.target_extractor(t)], dim=1)
            return feat, p(feat)
    f32, l32 = run(ext, pi_net, state, target)
    f64, l64 = run(copy.deepcopy(ext).double(), copy.deepcopy(pi_net).double(), state.double(), target.double())
    np.savez_compressed(os.path.join(out, "ln_create_mlp.npz"), obs_state=state.numpy(), obs_target=target.numpy(),
                        features32=f32.numpy(), features64=f64.numpy(), latent_pi32=l32.numpy(), latent_pi64=l64.numpy(),
                        label=np.asarray("reference StateTargetExtractor (state: ln) + create_mlp(96, [64, 48], Tanh, ln=True)"), **params)
    print(f"ln_keys: {len(keys) - 1} tensors; ln_create_mlp: features |32 - 64| {float((f32.double() - f64).abs().max()):.3e}, "
          f"latent_pi |32 - 64| {float((l32.double() - l64).abs().max()):.3e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GG.OUT)
    gen(ap.parse_args().out)
