#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden-vector generator for TrackEnv.  Runs ONLY where the reference is importable.

The reference's TrackEnv (envs/TrackingEnv.py:14-116) is imported through the stubs of oracle/gen_golden.py and run on the CPU under
the CR-sqrt / CR-trig patches, like every env fixture.  Its signatures predate the base class (defect class C-4, as RacingEnv's): the
base calls ``get_observation(predicted_obs=...)`` and ``get_reward(predicted_obs=...)`` and TrackEnv takes neither, so the class below
adds the two parameters and nothing else.

    tests/golden/track_env.npz    oracle/gen_golden.py::gen_env's layout, recorded by gen_env itself (the case is added to the table it
                                  reads and the shim is handed to it in HoverEnv's place): N = 64, 96 steps, max_episode_steps = 32,
                                  ENV_DYN, hover-style actions.  `target` is the (10, 3) waypoint table, `ev_tobs` the 40-column terminal
                                  rows, `raw_reward` / `raw_done` the run of the reference exactly as torch runs it.
    tests/golden/track_bptt.npz   gen_bptt's layout (its loop restated here: gen_bptt weights 13 observation columns), N = 32, H = 12,
                                  max_episode_steps = 8, `Wo` (H, N, 40).

Asserted here and again by tests/test_track_env.py: at least 2 N episode ends in track_env, every agent ends an episode inside the
horizon of track_bptt, the target never moves.

Usage:  python tools/gen_track_golden.py [--only track_env | track_bptt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gen_golden as G  # noqa: E402
from gen_golden import decode_actions, extend_state, extract_consts, f32, import_envs, use_cr_sqrt, use_cr_trig  # noqa: E402,F401

import torch as th  # noqa: E402

HOVER, SCALE = [-1 / 3, 0, 0, 0], 0.5


def track_shim():
    import_envs()
    from VisFly.envs.TrackingEnv import TrackEnv

    class TrackEnvShim(TrackEnv):  # defect C-4: the base passes predicted_obs to both
        def get_observation(self, indices=None, predicted_obs=None):
            return TrackEnv.get_observation(self, indices)

        def get_reward(self, predicted_obs=None):
            return TrackEnv.get_reward(self)

    return TrackEnvShim


def gen_env(name="track_env", N=64, steps=96, max_episode_steps=32, seed=42):
    cls = track_shim()
    G.ENV_CASES[name] = ("hover", dict(max_episode_steps=max_episode_steps), HOVER, SCALE, steps)
    real = G.import_envs
    hover, nav, racing = real()
    G.import_envs = lambda: (cls, nav, racing)
    try:
        G.gen_env(name, N=N, seed=seed)
    finally:
        G.import_envs = real
        del G.ENV_CASES[name]
    z = np.load(os.path.join(G.OUT, name + ".npz"))
    ends = len(z["ev_step"])
    assert z["target"].shape == (10, 3) and z["ev_tobs"].shape == (ends, 40) and z["obs_state_keep"].shape[-1] == 40
    assert ends >= 2 * N, f"{name}: {ends} episode ends, fewer than 2 N"
    assert z["raw_reward"].shape == (steps, N) and np.array_equal(z["raw_done"], z["done"])
    # the target never moves: a fresh env stepped through resets keeps its constructed table
    use_cr_sqrt(True)
    env = cls(num_agent_per_scene=8, num_scene=1, seed=seed, visual=False, dynamics_kwargs=dict(G.ENV_DYN), device="cpu",
              tensor_output=True, max_episode_steps=4)
    t0 = env.target.clone()
    env.reset()
    for _ in range(10):
        env.step(th.tensor([HOVER] * 8, dtype=th.float32))
    assert th.equal(env.target, t0) and np.array_equal(f32(t0[0]).view(np.uint32), z["target"].view(np.uint32))
    print(f"{name}: {ends} episode ends, |reward - unpatched| max {np.abs(z['reward'] - z['raw_reward']).max():.3e}, "
          f"{os.path.getsize(os.path.join(G.OUT, name + '.npz'))} bytes")


def gen_bptt(name="track_bptt", N=32, H=12, max_episode_steps=8, seed=42):
    cls = track_shim()
    dkw = dict(G.ENV_DYN)
    use_cr_sqrt(True)
    env = cls(num_agent_per_scene=N, num_scene=1, seed=seed, visual=False, dynamics_kwargs=dict(dkw), device="cpu", requires_grad=True,
              tensor_output=True, max_episode_steps=max_episode_steps)
    env.tensor_output = True
    consts = extract_consts(env.envs.dynamics)
    rng = np.random.default_rng(seed + 5)
    a0 = decode_actions(rng.integers(-127, 128, size=(H, N, 4), dtype=np.int8), HOVER, 0.3)
    acts = th.tensor(a0, requires_grad=True)
    Wr = th.tensor(rng.normal(size=(H, N)).astype(np.float32))
    Wo = th.tensor((rng.normal(size=(H, N, 40)) * 0.1).astype(np.float32))
    env.reset()
    dyn = env.envs.dynamics
    fs_init = f32(dyn.full_state)
    loss = 0
    dones, rewards, ev_step, ev_agent, ev_fs = [], [], [], [], []
    for t in range(H):
        o, r, d, info = env.step(acts[t])
        loss = loss + (Wr[t] * r).sum() + (Wo[t] * o["state"]).sum()
        dones.append(d.numpy().astype(np.uint8)); rewards.append(f32(r))
        didx = np.nonzero(d.numpy())[0]
        if len(didx):
            fs = f32(dyn.full_state)
            for i in didx:
                ev_step.append(t); ev_agent.append(i); ev_fs.append(fs[i])
    loss.backward()
    g = f32(acts.grad)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    assert np.stack(dones).any(0).all(), f"{name}: an agent ends no episode inside the horizon"
    print(f"{name}: N={N} H={H} resets={len(ev_step)} |dL/da| max {np.abs(g).max():.3e} loss {float(loss):.4f}")
    save = {"kind": np.asarray("track"), "max_episode_steps": np.int32(max_episode_steps), "seed": np.int32(seed),
            "fs_init": fs_init, "actions": f32(acts), "Wr": f32(Wr), "Wo": f32(Wo), "d_actions": g, "loss": np.float64(float(loss)),
            "done": np.stack(dones), "reward": np.stack(rewards),
            "ev_step": np.asarray(ev_step, np.int32), "ev_agent": np.asarray(ev_agent, np.int32),
            "ev_fs": np.stack(ev_fs) if ev_fs else np.zeros((0, 22), np.float32),
            "dyn_kw": np.asarray(repr(dkw)), "label": np.asarray("cr-sqrt-oracle"),
            "target": f32(env.target[0]), "spawn": np.asarray("track-default")}
    save.update({"c_" + k: v for k, v in consts.items()})
    np.savez_compressed(os.path.join(G.OUT, name + ".npz"), **save)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    only = ap.parse_args().only
    for name, fn in (("track_env", gen_env), ("track_bptt", gen_bptt)):
        if only is None or name in only:
            fn(name)


if __name__ == "__main__":
    main()
