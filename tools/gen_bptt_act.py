#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden-vector generator for BPTT with a non-ReLU actor.  Runs ONLY where the reference is importable.

tests/golden/bptt_loop_hover_tanh.npz: ONE iteration of the reference's own ``BPTT.learn`` exactly as oracle/gen_shac.py::gen_bptt_loop
records it for tests/golden/bptt_loop_hover.npz (same env, spawn box, seeds, noise feed, network sizes, recorded arrays), with
``policy_kwargs["activation_fn"] = th.nn.Tanh``: MTDPolicy hands it to the Actor's two trunks (td_policies.py:297), the StateExtractor's
MLP keeps its own default ReLU (extractors.py:560).

The recorder is gen_bptt_loop itself; this script only stands between it and the reference's ``BPTT`` constructor and swaps the
activation class in the policy_kwargs it is handed.

Usage:  python tools/gen_bptt_act.py [--activation Tanh] [--name bptt_loop_hover_tanh]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gen_shac as GS  # noqa: E402  (imports gen_golden: stubs, CR-sqrt patch, constants extraction)

import torch.nn as nn  # noqa: E402


def gen(name, activation):
    GS._install_sb3()
    import VisFly.utils.algorithms.BPTT as B
    act = getattr(nn, activation)
    real = B.BPTT
    seen = []

    def with_activation(env, policy, policy_kwargs=None, **kw):
        pk = dict(policy_kwargs or {})
        assert pk.get("activation_fn") is nn.ReLU, pk
        pk["activation_fn"] = act
        algo = real(env, policy, policy_kwargs=pk, **kw)
        actor = algo.policy.actor
        # the trunks carry the activation, the extractor MLP stays ReLU: what the fixture's consumer builds ((trunk, extractor) kinds)
        kinds = lambda mod: {type(m).__name__ for m in mod.modules() if not isinstance(m, (nn.Linear, nn.Sequential))}
        assert kinds(actor.latent_pi) == kinds(actor.log_latent_pi) == {activation}, (kinds(actor.latent_pi), kinds(actor.log_latent_pi))
        assert kinds(actor.features_extractor.state_extractor) <= {"ReLU", "Flatten"}, kinds(actor.features_extractor.state_extractor)
        seen.append(activation)
        return algo
    B.BPTT = with_activation
    try:
        GS.gen_bptt_loop(name=name)
    finally:
        B.BPTT = real
    assert seen == [activation]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--activation", default="Tanh", choices=["Tanh", "ELU", "LeakyReLU"])
    ap.add_argument("--name", default=None)
    a = ap.parse_args()
    gen(a.name or "bptt_loop_hover_" + a.activation.lower(), a.activation)
