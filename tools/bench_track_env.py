#!/usr/bin/env python3
"""TrackEnv's two observation launches next to their torch forms and their byte floors, and TrackEnv.step() next to HoverEnv2.step().

    python tools/bench_track_env.py [--agents 16384 65536] [--iters 2000] [--reps 5] [--out profiles/track_env.txt]

Three comparisons per agent count, every one in the same process with the two sides alternating over `reps` repetitions (the spread of
the repetitions is printed next to every median; a difference inside it is no difference):
  1. vf_track_obs alone (without and with the terminal pair) | the same rows by the torch expressions of TrackEnv._track_state
     -- HIP events around `iters` back-to-back launches, microseconds per call; byte floor = (52 + 160) B per agent at 8 TB/s.
  2. TrackEnv.step() | HoverEnv2.step() (the same step kernel: HoverEnv's, observation formed in its epilogue) -- host clock around
     `iters` steps that end in a synchronise, microseconds per step.
  3. TrackEnv.backward_step (vf_track_obs_bwd + the step kernel's adjoint) | the same with the 40 -> 13 map written as torch column
     operations (RacingEnv2.backward_step's form) -- events around reverse sweeps over a recorded horizon; and the map alone.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(ROOT))
DYN = dict(action_type="bodyrate", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)
HBM = 8.0e12      # B/s (MI355X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="*", default=[16384, 65536])
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from visfly_amd import _lib
    from visfly_amd.envs import HoverEnv2, TrackEnv
    assert torch.cuda.is_available(), "bench_track_env.py measures on the GPU only"
    L, dev = _lib.lib(), torch.device("cuda", 0)
    st = _lib.current_stream(dev)

    def events(fn, iters):
        """microseconds per call of fn over `iters` back-to-back calls"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    def wall(fn, iters):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e6 / iters

    def alternate(sides, timer, iters):
        """{name: fn} -> {name: (median, min, max)} over a.reps alternating repetitions"""
        runs = {k: [] for k in sides}
        for _ in range(a.reps):
            for k, fn in sides.items():
                runs[k].append(timer(fn, iters))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}

    lines = [f"# tools/bench_track_env.py --iters {a.iters} --reps {a.reps} --horizon {a.horizon}; {torch.cuda.get_device_name(0)}",
             "# microseconds: median [min .. max] over the alternating repetitions"]
    fmt = lambda r: f"{r[0]:8.2f} [{r[1]:7.2f} .. {r[2]:7.2f}]"
    for N in a.agents:
        g = torch.Generator(device=dev).manual_seed(1)
        env = TrackEnv(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(DYN), device="cuda:0", tensor_output=True, max_episode_steps=64)
        env.reset()
        raw = env.envs.dynamics.state.detach().contiguous()
        term = raw.clone()
        out, tout = torch.empty((N, 40), device=dev), torch.empty((N, 40), device=dev)
        wp, R = env._wp_host, float(env.max_sense_radius)
        p = [x.data_ptr() for x in (raw, out, term, tout)]
        one = lambda: L.vf_track_obs(p[0], p[1], None, None, wp, 10, R, N, st)
        two = lambda: L.vf_track_obs(p[0], p[1], p[2], p[3], wp, 10, R, N, st)
        wpt, Rt, ten = env._wp, torch.full((1,), R, device=dev), torch.full((1,), 10.0, device=dev)

        def torch_rows(r=raw):
            return torch.hstack([(wpt.unsqueeze(0) - r[:, 0:3].unsqueeze(1)).reshape(N, -1) / Rt, r[:, 3:7], r[:, 7:10] / ten, r[:, 10:13] / ten])
        assert torch.equal(torch_rows(), env._track_rows(raw))
        r1 = alternate({"vf_track_obs": one, "vf_track_obs + terminal pair": two, "torch expressions": torch_rows,
                        "torch expressions x 2": lambda: (torch_rows(), torch_rows(term))}, events, a.iters)
        lines += ["", f"== {N} agents", f"1. observation rows (byte floor {212 * N / HBM * 1e6:.2f} us; with the terminal pair {424 * N / HBM * 1e6:.2f} us)"]
        lines += [f"   {k:32s} {fmt(v)}" for k, v in r1.items()]
        # 2. step()
        hov = HoverEnv2(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(DYN), device="cuda:0", tensor_output=True, max_episode_steps=64)
        hov.reset()
        act = (torch.tensor([-1 / 3, 0, 0, 0], device=dev) + (torch.rand((N, 4), device=dev, generator=g) * 2 - 1) * 0.3).clamp(-1, 1)
        envt = TrackEnv(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(DYN), device="cuda:0", tensor_output=True, max_episode_steps=64)
        envt.reset()
        envt._terminal_state_rows()          # as PPO / evaluate_policy do: from now on every step maps the terminal rows too
        steps = {"TrackEnv.step()": lambda: env.step(act), "TrackEnv.step() + terminal rows": lambda: envt.step(act),
                 "HoverEnv2.step()": lambda: hov.step(act)}
        r2 = alternate(steps, wall, a.iters)
        lines += ["2. step(), host clock, fresh output tensors"] + [f"   {k:32s} {fmt(v)}" for k, v in r2.items()]
        r2e = alternate(steps, events, a.iters)
        lines += ["   the same between two events"] + [f"   {k:32s} {fmt(v)}" for k, v in r2e.items()]
        # 3. the adjoint
        H = a.horizon
        env.reset()
        env.enable_tape(H)
        for _ in range(H):
            env.step(act, is_test=True)
        d_obs, d_rew = torch.randn((N, 40), device=dev, generator=g) * 0.1, torch.randn(N, device=dev, generator=g)
        d13 = torch.empty((N, 13), device=dev)
        base = super(TrackEnv, env).backward_step

        def torch_map(d=d_obs):
            dp = d[:, 0:3] / Rt
            for j in range(1, 10):
                dp = dp + d[:, 3 * j:3 * j + 3] / Rt
            return torch.cat([-dp, d[:, 30:34], d[:, 34:37] / ten, d[:, 37:40] / ten], dim=1)
        L.vf_track_obs_bwd(d_obs.data_ptr(), d13.data_ptr(), 10, R, N, st)
        assert torch.equal(torch_map(), d13)

        def sweep(kernel):
            env._adj.zero_()
            for t in reversed(range(H)):
                if kernel:
                    env.backward_step(t, d_obs, d_rew)
                else:
                    base(t, torch_map(), d_rew)
        sw = max(1, a.iters // H)
        r3 = alternate({"backward_step, vf_track_obs_bwd": lambda: sweep(True), "backward_step, torch columns": lambda: sweep(False)}, events, sw)
        r3 = {k: tuple(x / H for x in v) for k, v in r3.items()}
        r3m = alternate({"the map alone: vf_track_obs_bwd": lambda: L.vf_track_obs_bwd(d_obs.data_ptr(), d13.data_ptr(), 10, R, N, st),
                         "the map alone: torch columns": torch_map}, events, a.iters)
        lines += [f"3. adjoint, per step of a reverse sweep over H = {H} (byte floor of the map {212 * N / HBM * 1e6:.2f} us)"]
        lines += [f"   {k:32s} {fmt(v)}" for k, v in {**r3, **r3m}.items()]
        env.close()
        envt.close()
        hov.close()
        print("\n".join(lines[-18:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps({"ok": True, "agents": a.agents}))


if __name__ == "__main__":
    main()
