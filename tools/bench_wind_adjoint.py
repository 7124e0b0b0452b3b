#!/usr/bin/env python3
"""Mean microseconds per env-adjoint launch (vf_env_step_bwd, and vf_env_step_bwd_wind where the library has it), HIP events around
back-to-back launches on one stream: HoverEnv, 16 384 agents, bodyrate / Euler / delay ring -- the per-step cost of the reverse half
of a launch-by-launch BPTT / SHAC horizon.  The launches are reverse sweeps over a recorded horizon (t = H-1 .. 0, the adjoint slab
zeroed in front of every sweep: one small memset per H launches is inside the window), so every launch reads another tape row and the
adjoint stays finite, as in a trainer.

    python tools/bench_wind_adjoint.py [--root TREE] [--agents 16384] [--horizon 32] [--iters 4000] [--reps 5]

--root: import visfly_amd from another checkout (one that is already built), e.g. the parent commit's, to compare the no-wind launch
across commits; run the two alternately, one fresh process per run (profiles/wind_adjoint.txt).  A library without
vf_env_step_bwd_wind reports the no-wind launch only.  One JSON line per run.
"""
import argparse
import ctypes as C
import json
import os
import sys

WIND = ["0.3 - 0.05*x", "0.02*x*x", "0.5*y + 0.1", "0*x + 0.125", "-0.01*x", "0.25*y - 0.05"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--agents", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from visfly_amd import _lib
    from visfly_amd.envs import HoverEnv
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(a.root)), _lib.__file__
    L, dev = _lib.lib(), torch.device("cuda", 0)
    st = _lib.current_stream(dev)
    N, H = a.agents, a.horizon
    sweeps = max(1, a.iters // H)
    out = {"label": a.label, "agents": N, "horizon": H, "launches": sweeps * H, "device": torch.cuda.get_device_name(0)}
    g = torch.Generator(device=dev).manual_seed(1)
    acts = (torch.tensor([-1 / 3, 0, 0, 0], device=dev) + (torch.rand((H, N, 4), device=dev, generator=g) * 2 - 1) * 0.3).clamp(-1, 1)
    d_obs, d_rew = torch.randn((N, 13), device=dev, generator=g) * 0.1, torch.randn(N, device=dev, generator=g)
    for windy in (False, True):
        if windy and not hasattr(L, "vf_env_step_bwd_wind"):
            continue
        dkw = dict(action_type="bodyrate", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)
        if windy:
            dkw["wind_settings"] = WIND
        env = HoverEnv(num_agent_per_scene=N, seed=3, dynamics_kwargs=dkw, device="cuda:0", tensor_output=True, max_episode_steps=1000)
        env.reset()
        env.enable_tape(H)
        for t in range(H):
            env.step(acts[t], is_test=True)
        adj, da = torch.zeros_like(env._adj), torch.empty((N, 4), device=dev)
        refs, keep = [], []
        for t in range(H):
            b = _lib.EnvBwdArgs()
            b.tape_slab, b.action = env._tape[t].data_ptr(), env._tape_actions[t].data_ptr()
            b.d_obs, b.d_reward = d_obs.data_ptr(), d_rew.data_ptr()
            b.done, b.adj_slab, b.d_action = env._tape_done[t].data_ptr(), adj.data_ptr(), da.data_ptr()
            keep.append(b)
            refs.append(C.byref(b))
        if windy:
            rows = [env._tape_wind[t].data_ptr() for t in range(H)]
            launch = lambda t: L.vf_env_step_bwd_wind(env._h, refs[t], rows[t], st)
        else:
            launch = lambda t: L.vf_env_step_bwd(env._h, refs[t], st)

        def sweep():
            adj.zero_()
            for t in range(H - 1, -1, -1):
                launch(t)
        for t in range(H):
            _lib.check(launch(t))
        sweep()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(sweeps):
                sweep()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / (sweeps * H))
        out["wind_us" if windy else "nowind_us"] = [round(x, 3) for x in us]
        out["wind_finite" if windy else "nowind_finite"] = bool(torch.isfinite(da).all())
        env.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
