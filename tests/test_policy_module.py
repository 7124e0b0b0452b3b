"""visfly_amd/policy.py is the home of MlpPolicy and its helpers: the trainers and checkpoint.py import it, it imports none of them,
and the names that used to live in ppo.py are the same objects when taken from there."""
import os
import subprocess
import sys

import pytest
import torch

import visfly_amd.checkpoint
import visfly_amd.policy
import visfly_amd.ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_taken_from_ppo_are_the_owning_modules_objects():
    for name in ("MlpPolicy", "policy_rows", "activation_kind", "_Linear", "_ptr", "obs_width", "ACTIVATIONS", "_TORCH_ACT", "INDEX_OBS_KEYS"):
        assert getattr(visfly_amd.ppo, name) is getattr(visfly_amd.policy, name), name
    assert visfly_amd.ppo.trainer_obs_keys is visfly_amd.checkpoint.trainer_obs_keys
    assert visfly_amd.policy.MlpPolicy.__module__ == "visfly_amd.policy"
    assert visfly_amd.checkpoint.trainer_obs_keys.__module__ == "visfly_amd.checkpoint"


def test_importing_the_policy_imports_no_trainer_and_no_checkpoint():
    code = ("import sys, visfly_amd.policy\n"
            "print([m for m in ('visfly_amd.ppo', 'visfly_amd.bptt', 'visfly_amd.shac', 'visfly_amd.checkpoint') if m in sys.modules])")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "[]", r.stdout


class _Leaf(Exception):
    pass


def test_weight_grad_slots_reads_the_policy_modules_split_size(monkeypatch):
    """weight_grad_slots splits a horizon above visfly_amd.policy.WGRAD_SPLIT_ROWS, read when it is called: the first descriptor it
    asks for covers the whole horizon under the shipped value and one run of the split under a smaller one.  No launch: the
    descriptor builder is stubbed and ends the call."""
    M, n = 32, 4
    pol = visfly_amd.policy.MlpPolicy({"state": 13}, {"state": [32]}, [32], [32], "cpu")
    pol.reserve_slots(M, n)
    asked = []

    def first_desc(b, rows, *a):
        asked.append(rows)
        raise _Leaf

    monkeypatch.setattr(pol, "_bwd_desc", first_desc)
    d_mean = torch.zeros((n, M, 4))
    assert n * M <= visfly_amd.policy.WGRAD_SPLIT_ROWS
    with pytest.raises(_Leaf):
        pol.weight_grad_slots(M, n, d_mean)
    monkeypatch.setattr(visfly_amd.policy, "WGRAD_SPLIT_ROWS", 2 * M)      # (restored by monkeypatch)
    with pytest.raises(_Leaf):
        pol.weight_grad_slots(M, n, d_mean)
    assert asked == [n * M, 2 * M]
    assert visfly_amd.policy.MlpPolicy.weight_grad_slots.__globals__ is vars(visfly_amd.policy)
