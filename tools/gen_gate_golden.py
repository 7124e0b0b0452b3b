#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden-vector generator for StateGateExtractor.  Runs ONLY where the reference is importable.

The reference's ``StateGateExtractor`` (utils/policies/extractors.py:752-761) is ``StateExtractor`` plus a second MLP over the
observation's ``"gate"`` entry -- the racing envs' next-gate index, a ``Box(shape=(1,), dtype=int32)`` that SB3's ``preprocess_obs``
turns into one float column -- with the two outputs concatenated.  Two fixtures, data only, read off the reference's own module:

* tests/golden/gate_keys.json: ``state_dict`` names and shapes of the extractor for ``net_arch = {state: [64, 32], gate: [32]}`` under
  the name the policy gives it (``features_extractor``): the key pattern visfly_amd/checkpoint.py has to write for the second branch.
* tests/golden/gate_extractor.npz: its parameters, 64 observation rows (16-wide state rows as RacingEnv2 forms them; the gate column as
  int32 with all four indices present) and the features the module computes on ``obs.float()``, in fp32 and from a ``.double()`` copy.

The stubs that make the reference's policy package importable without its simulator are oracle/gen_golden.py's own.

Usage:  python tools/gen_gate_golden.py [--out DIR]
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

NET_ARCH = {"state": {"layer": [64, 32]}, "gate": {"layer": [32]}}
ROWS, STATE_W, N_GATES = 64, 16, 4


def gen(out):
    GG.import_envs()
    GG._sb3_stubs()
    import VisFly.utils.policies.extractors as E
    sp = sys.modules["gymnasium.spaces"]
    th.manual_seed(20262)
    space = sp.Dict({"state": sp.Box(-np.inf, np.inf, (STATE_W,)), "gate": sp.Box(0, N_GATES, (1,), dtype=np.int32)})
    ext = E.StateGateExtractor(space, net_arch=copy.deepcopy(NET_ARCH), activation_fn=nn.ReLU)
    assert int(ext.features_dim) == 64
    keys, params = {}, {}
    with th.no_grad():       # biases away from nn.Linear's small default draw, so that a consumer that drops one fails
        for m in ext.modules():
            if isinstance(m, nn.Linear):
                m.bias.add_(0.1 * th.randn_like(m.bias))
    for k, v in ext.state_dict().items():
        keys[f"features_extractor.{k}"] = list(v.shape)
        params["param:" + f"features_extractor.{k}"] = v.detach().numpy().astype(np.float32)
    keys["features_dim"] = int(ext.features_dim)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "gate_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)

    state = th.randn(ROWS, STATE_W)
    gate = (th.arange(ROWS) * 7 % N_GATES).to(th.int32).reshape(ROWS, 1)      # every index, in no regular run
    assert sorted(set(gate.reshape(-1).tolist())) == list(range(N_GATES))

    def run(e, s, g):
        with th.no_grad():
            return th.cat([e.state_extractor(s), e.gate_extractor(g)], dim=1)
    f32 = run(ext, state, gate.float())                                       # SB3 preprocess_obs: obs.float() for a Box space
    f64 = run(copy.deepcopy(ext).double(), state.double(), gate.double())
    with th.no_grad():       # the module's own path (extract: the branches in the order it registered them)
        assert th.equal(ext.extract({"state": state, "gate": gate.float()}), f32)
    np.savez_compressed(os.path.join(out, "gate_extractor.npz"), obs_state=state.numpy(), obs_gate=gate.numpy(),
                        features32=f32.numpy(), features64=f64.numpy(),
                        label=np.asarray("reference StateGateExtractor, net_arch {state: [64, 32], gate: [32]}, ReLU"), **params)
    print(f"gate_keys: {len(keys) - 1} tensors; gate_extractor: features |32 - 64| {float((f32.double() - f64).abs().max()):.3e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GG.OUT)
    gen(ap.parse_args().out)
