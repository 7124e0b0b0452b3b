"""TrackEnv without a GPU: the fixtures of tools/gen_track_golden.py against the CPU oracle stepped as HoverEnv toward waypoint 0 plus
the numpy restatement of the 40-column rows, the two entry points' ABI and argument checks, and the host-side rules of the class on a
stub (no device)."""
import types

import numpy as np
import pytest
import torch

import oracle
from _golden import assert_bits_equal, consts_of, decode_actions, load
from _track_ref import track_rows_np, waypoints_np

EINVAL = -1          # VF_EINVAL (include/visfly_amd.h)


def test_fixture_target_is_the_numpy_table():
    fx = load("track_env")
    wp = waypoints_np()
    assert fx["target"].shape == (10, 3)
    assert_bits_equal(fx["target"], wp, "waypoint table")
    assert_bits_equal(wp[0], np.asarray([4, 0, 1], np.float32), "waypoint 0")
    assert_bits_equal(load("track_bptt")["target"], wp, "waypoint table (gradient fixture)")


def test_fixture_conditions():
    fx = load("track_env")
    N = fx["fs_init"].shape[0]
    assert N == 64 and fx["reward"].shape == (96, 64) and int(fx["max_episode_steps"]) == 32
    assert len(fx["ev_step"]) >= 2 * N and int(fx["done"].sum()) == len(fx["ev_step"])
    assert fx["ev_tobs"].shape == (len(fx["ev_step"]), 40) and fx["obs_state_keep"].shape[1:] == (N, 40)
    b = load("track_bptt")
    assert b["done"].shape == (12, 32) and b["Wo"].shape == (12, 32, 40) and int(b["max_episode_steps"]) == 8
    assert b["done"].any(axis=0).all(), "every agent ends an episode inside the horizon"
    assert np.isfinite(b["d_actions"]).all() and np.abs(b["d_actions"]).max() > 0


def test_fixture_stays_close_to_the_unpatched_reference():
    """reward within the 1.4e-7 the README states for the env fixtures, identical done flags"""
    fx = load("track_env")
    assert np.array_equal(fx["done"], fx["raw_done"])
    err = float(np.abs(fx["reward"] - fx["raw_reward"]).max())
    print(f"track_env: |reward - unpatched reference's| max {err:.3e}")
    assert err <= 1.4e-7


def test_oracle_as_hover_toward_waypoint_0_reproduces_the_reference_run():
    """rewards, done flags, kept observation rows and terminal rows of all 96 steps, bit for bit: the step is HoverEnv's with target
    [4, 0, 1], the rows are the numpy restatement of the raw state rows"""
    fx = load("track_env")
    wp = fx["target"]
    acts = decode_actions(fx)
    N = fx["fs_init"].shape[0]
    env = oracle.OracleEnv(consts_of(fx), N, "hover", int(fx["max_episode_steps"]), target=wp[0], success_radius=0.5)
    env.reset_full_state(fx["fs_init"])
    assert_bits_equal(track_rows_np(env.obs_state, wp), fx["obs0_state"], "reset() rows")
    keep = list(fx["keep_steps"])
    terminal = 0
    for k in range(acts.shape[0]):
        raw, reward, done = env.step(acts[k])
        assert_bits_equal(reward, fx["reward"][k], f"reward @ {k}")
        assert np.array_equal(done.astype(np.uint8), fx["done"][k]), f"done @ {k}"
        assert np.array_equal(env.a["step_count"], fx["step_count"][k]), f"step_count @ {k}"
        assert not env.a["success"].any()
        sel = fx["ev_step"] == k
        assert np.array_equal(np.nonzero(done)[0], fx["ev_agent"][sel]), f"reset set @ {k}"
        if sel.any():
            assert_bits_equal(track_rows_np(raw, wp)[fx["ev_agent"][sel]], fx["ev_tobs"][sel], f"terminal rows @ {k}")
            terminal += int(sel.sum())
            env.reset_agents(fx["ev_agent"][sel], fx["ev_fs"][sel])
        if k in keep:
            assert_bits_equal(track_rows_np(env.obs_state, wp), fx["obs_state_keep"][keep.index(k)], f"rows (post-reset) @ {k}")
    assert terminal == len(fx["ev_step"])


def test_gradient_fixture_forward_matches_the_oracle():
    """track_bptt's rewards and done flags from the oracle stepped as hover kind (the adjoint itself is a GPU test)"""
    fx = load("track_bptt")
    N = fx["fs_init"].shape[0]
    env = oracle.OracleEnv(consts_of(fx), N, "hover", int(fx["max_episode_steps"]), target=fx["target"][0])
    env.reset_full_state(fx["fs_init"])
    for t in range(fx["actions"].shape[0]):
        _, reward, done = env.step(fx["actions"][t])
        assert_bits_equal(reward, fx["reward"][t], f"reward @ {t}")
        assert np.array_equal(done.astype(np.uint8), fx["done"][t])
        sel = fx["ev_step"] == t
        if sel.any():
            env.reset_agents(fx["ev_agent"][sel], fx["ev_fs"][sel])


def test_entry_points_declared_exported_signed_abi_11():
    import os
    import __graft_entry__ as ge
    ge.build()
    from visfly_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "visfly_amd.h")).read()
    L = _lib.lib()
    for s in ("vf_track_obs", "vf_track_obs_bwd"):
        assert f"int {s}(" in header and hasattr(L, s) and s in _lib.SIGNATURES
    assert L.vf_abi_version() == _lib.ABI_VERSION == 11


def test_argument_errors_before_any_launch():
    """VF_EINVAL for null pointers, n_points out of range, N < 1, half a terminal pair and a misaligned output: decided on the host, so
    the calls are safe with made-up addresses (and on a machine without a GPU)"""
    import ctypes as C
    from visfly_amd import _lib
    L = _lib.lib()
    wp = (C.c_float * 48)()
    a, b, c, d = 0x10000, 0x20000, 0x30000, 0x40000      # never dereferenced
    bad = [(None, b, None, None, wp, 10, 10.0, 4), (a, None, None, None, wp, 10, 10.0, 4), (a, b, None, None, None, 10, 10.0, 4),
           (a, b, None, None, wp, 0, 10.0, 4), (a, b, None, None, wp, 17, 10.0, 4), (a, b, None, None, wp, 10, 10.0, 0),
           (a, b, None, None, wp, 10, 10.0, -3), (a, b, c, None, wp, 10, 10.0, 4), (a, b, None, d, wp, 10, 10.0, 4),
           (a, b + 4, None, None, wp, 10, 10.0, 4), (a, b, c, d + 8, wp, 10, 10.0, 4), (a, b, None, None, wp, 10, 0.0, 4)]
    for args in bad:
        assert L.vf_track_obs(*args, None) == EINVAL, args
        assert b"vf_track_obs" in L.vf_last_error()
    for args in [(None, b, 10, 10.0, 4), (a, None, 10, 10.0, 4), (a, b, 0, 10.0, 4), (a, b, 17, 10.0, 4), (a, b, 10, 10.0, 0),
                 (a, b, 10, -1.0, 4)]:
        assert L.vf_track_obs_bwd(*args, None) == EINVAL, args
        assert b"vf_track_obs_bwd" in L.vf_last_error()


@pytest.fixture
def stub(monkeypatch):
    """TrackEnv's own constructor over a base constructor that opens no device: what it hands to the base, and the host-side rules"""
    from visfly_amd.envs import TrackEnv, spaces
    from visfly_amd.envs.base import DroneGymEnvsBase
    seen = {}

    def fake_init(self, **kw):
        seen.update(kw)
        self.device = torch.device("cpu")
        self.num_agent = self.num_envs = kw["num_agent_per_scene"] * kw["num_scene"]
        self.envs = types.SimpleNamespace(dynamics=types.SimpleNamespace(t=torch.zeros(self.num_agent), _wind_fn=None))
        self.observation_space = spaces.Dict({"state": spaces.Box(low=-np.inf, high=np.inf, shape=(13,), dtype=np.float32)})
        self._is_initial, self.spawn_mode, self._tape = True, "device", None

    monkeypatch.setattr(DroneGymEnvsBase, "__init__", fake_init)
    monkeypatch.setattr(DroneGymEnvsBase, "__del__", lambda self: None)
    env = TrackEnv(num_agent_per_scene=6, num_scene=1, random_kwargs={"state_generator": {"class": "Uniform", "kwargs": [
        {"position": {"mean": [9., 9., 9.], "half": [1., 1., 1.]}}]}}, target=[7., 7., 7.], max_episode_steps=32)
    return env, seen


def test_stub_constructor_space_and_target(stub):
    env, seen = stub
    assert env.observation_space["state"].shape == (40,)
    assert env.KIND == 0 and seen["target"] == [4.0, 0.0, 1.0] and seen["success_radius"] == 0.5
    box = seen["random_kwargs"]["state_generator"]["kwargs"][0]["position"]          # the caller's spawn and target are ignored
    assert seen["random_kwargs"]["state_generator"]["class"] == "Uniform" and box["mean"] == [2.0, 0.0, 1.0]
    assert np.allclose(box["half"], [.2, .2, .2])
    assert tuple(env.target.shape) == (6, 10, 3)
    assert_bits_equal(env.target[3].numpy(), load("track_env")["target"], "env.target")
    assert (env.next_points_num, env.radius, env.dt, env.success_radius, env.max_sense_radius) == (10, 2, 0.1, 0.5, 10)
    assert env.center.tolist() == [2, 0, 1] and env.radius_spd == 0.2 * torch.pi


def test_stub_update_target(stub):
    env, _ = stub
    before = env.target.clone()
    env.update_target()                      # agents at t == 0: the constructed table
    assert torch.equal(env.target, before)
    env.envs.dynamics.t = torch.tensor([0., 0., 0.02, 0., 0., 0.])
    with pytest.raises(NotImplementedError, match="vf_env_cfg"):
        env.update_target()


def test_stub_refusals_before_any_library_call(stub, monkeypatch):
    """step_n refuses; every persistent path answers False in Python -- the library is not even loaded"""
    env, _ = stub
    from visfly_amd import _lib

    def no_library():
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(_lib.VisflyError, match="TrackEnv"):
        env.step_n(torch.zeros((2, 6, 4)))
    assert env.rollout_policy(None, ["state"], None, None, None, None, None, 0.99, 1.0) is False
    assert env.reverse_policy(None, 4, None, None, None, None, None) is False
    assert env.collect_policy(None, ["state"], None, None, 0, 0, None) is False
    assert env.evaluate_policy_launch(None, ["state"], None, None, None, None) is False
