"""The env adjoint under string wind functions, the half that needs no GPU: what the fixtures of tools/gen_wind_golden.py must hold
for the GPU tests (tests/test_wind_adjoint_gpu.py) to mean something, and the two entry points' place in the C ABI."""
import os
import re

import numpy as np
import pytest

from _golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADJOINT = ["bptt_wind_hover", "bptt_wind_hover_resets", "bptt_wind_nav_rk4"]
REL_TOL = 1e-5        # the adjoint tests' bound (tests/test_bptt_gpu.py)


@pytest.mark.parametrize("name", ADJOINT)
def test_fixture_conditions(name):
    """N = 70 (dead lanes behind the last wind row in the last block), the wind of every step stored and non-zero on all three axes;
    where the re-spawns are planted or absent the wind moves the reference's own gradient by at least 50 x the adjoint tolerance, so
    an adjoint that ignores the wind, or takes another step's, cannot pass; the resets fixture re-spawns agents at t != 0 (a new
    wind mid-horizon)"""
    fx = load(name)
    H, N = fx["actions"].shape[:2]
    assert (H, N) == (12, 70) and N % 64 and N % 256
    assert fx["wind"].shape == (H, N, 3) and fx["d_actions_nowind"].shape == fx["d_actions"].shape == (H, N, 4)
    assert "wind_settings" in str(fx["dyn_kw"]) and ("rk4" in str(fx["dyn_kw"])) == (name == "bptt_wind_nav_rk4")
    assert (np.abs(fx["wind"]) > 0).any((0, 1)).all()
    assert not np.array_equal(fx["wind"][0], fx["wind"][-1])          # it changes from step to step
    if name != "bptt_wind_nav_rk4":
        moved = np.abs(fx["d_actions"] - fx["d_actions_nowind"]).max()
        assert moved >= 50 * REL_TOL * np.abs(fx["d_actions"]).max(), moved
    if name == "bptt_wind_hover":
        assert len(fx["ev_step"]) == 0 and not fx["done"].any()
    if name == "bptt_wind_hover_resets":
        assert int(fx["max_episode_steps"]) == 5 and len(fx["ev_step"]) and (fx["ev_fs"][:, 21] != 0).any()


@pytest.mark.parametrize("name", ["bptt_loop_hover_wind", "shac_hover_wind"])
def test_trainer_fixtures_run_under_wind(name):
    fx, base = load(name), load(name[:-5])
    assert "wind_settings" in str(fx["dyn_kw"]) and "wind_settings" not in str(base["dyn_kw"])
    assert np.array_equal(fx["actor_params0"], base["actor_params0"]) and np.array_equal(fx["eps"], base["eps"])
    # the wind moves the actor gradient of the same iteration far beyond the 2e-5 the trainer tests hold
    assert np.abs(fx["actor_grad"] - base["actor_grad"]).max() >= 50 * 2e-5 * np.abs(fx["actor_grad"]).max()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 1 << 20


def test_entry_points_declared_exported_and_mirrored():
    """vf_env_step_bwd_wind (4 arguments) / vf_dyn_step_bwd_wind (8): in the header, in the library, in the ctypes table; the structs
    and VF_ABI_VERSION are untouched; null arguments are refused before any device work"""
    import __graft_entry__ as ge
    ge.build()
    from visfly_amd import _lib
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "visfly_amd.h")).read(), flags=re.S)
    for sym, nargs in (("vf_env_step_bwd_wind", 4), ("vf_dyn_step_bwd_wind", 8)):
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)", src)
        assert m, f"{sym} is not declared"
        assert len(m.group(1).split(",")) == nargs and "wind_Nx4" in m.group(1)
        assert hasattr(L, sym)
        assert len(_lib.SIGNATURES[sym][1]) == nargs
        assert len(_lib.SIGNATURES[sym][1]) == len(_lib.SIGNATURES[sym[:-5]][1]) + 1
    assert L.vf_abi_version() == _lib.ABI_VERSION == 11
    assert L.vf_env_step_bwd_wind(None, None, None, None) == -1            # VF_EINVAL
    assert L.vf_dyn_step_bwd_wind(None, None, None, None, None, None, None, None) == -1            # VF_EINVAL
    assert b"vf_dyn_step_bwd_wind" in L.vf_last_error()
