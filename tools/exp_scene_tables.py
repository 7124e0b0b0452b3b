#!/usr/bin/env python3
"""What per-scene obstacle tables and collision-free spawns cost the fused env step -> profiles/scene_tables.txt (the measured part;
the build facts at its end are kept from the file that is there).

Mean device microseconds per vf_env_step launch (HIP events around back-to-back launches on one stream, vf_env_time_steps), bodyrate /
Euler / delay ring, HoverEnv and NavigationEnv, hover action (nobody ends an episode):
  - no table and a shared table of 1, 4, 16 solids at 65 536 agents, this tree and -- with --parent -- the parent commit's build,
    alternating, one fresh process per run: the instruction streams of those launches are the parent's, the difference is read
    against the spread of the parent's own runs;
  - per-scene tables with the same counts: 1 024 scenes of 64 agents (every wave inside one scene: scalar table reads) and 1 365 scenes
    of 48 agents (65 520 agents; two waves in three straddle two scenes: per-lane table reads).
The reset regime: HoverEnv, is_collision_reset, 32-step episodes, U(-1, 1) actions, a ball and a pillar inside the spawn box, safe_spawn
off and on, with the mean number of attempts per spawn from the host restatement (tests/_scene_ref.py) for the same seed and agents.

    python tools/exp_scene_tables.py [--parent TREE] [--iters 2000] [--reps 5] [--rounds 3]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
from exp_obstacles import KW, stats, table  # noqa: E402

COUNTS = (1, 4, 16)
N, SEED = 65536, 3
RESET_TABLE = [dict(type="sphere", center=[1.0, 0.0, 1.5], radius=0.6), dict(type="pillar", center=[1.5, 0.5], radius=0.35, z=[0.0, 3.0])]
BUILD_FACTS = "Build facts"


def scene_tables(n, scenes):
    """`scenes` tables of n solids: exp_obstacles.table's layout, rotated by the scene index so that neighbouring scenes differ"""
    base = table(16)
    return [[base[(k + s) % 16] for k in range(n)] for s in range(scenes)]


def child(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from visfly_amd import _lib
    from visfly_amd.envs import HoverEnv, NavigationEnv
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(a.root)), _lib.__file__
    new = "vf_env_set_scene_obstacles" in _lib.SIGNATURES
    dev = torch.device("cuda", 0)
    out = {"label": a.label, "iters": a.iters, "device": torch.cuda.get_device_name(0)}

    def timed(cls, ns, aps, action=None, steps=100000, **kw):
        n = ns * aps
        env = cls(num_agent_per_scene=aps, num_scene=ns, seed=SEED, dynamics_kwargs=dict(KW), device="cuda:0", tensor_output=True,
                  max_episode_steps=steps, **kw)
        env.reset()
        act = torch.tensor([-1 / 3, 0, 0, 0], device=dev).repeat(n, 1).contiguous() if action is None else action(n)
        env.time_steps(act, iters=200)                                     # warm-up: code objects, constant blocks in L2
        us = [round(env.time_steps(act, iters=a.iters), 3) for _ in range(a.reps)]
        env.close()
        return us

    for name, cls in (("hover", HoverEnv), ("nav", NavigationEnv)):
        out[f"{name}_none"] = timed(cls, 1, N)
        for n in COUNTS:
            out[f"{name}_shared_{n}"] = timed(cls, 1, N, scene_kwargs=dict(obstacles=table(n)))
            if new:
                out[f"{name}_s64_{n}"] = timed(cls, N // 64, 64, scene_kwargs=dict(scene_obstacles=scene_tables(n, N // 64)))
                out[f"{name}_s48_{n}"] = timed(cls, N // 48, 48, scene_kwargs=dict(scene_obstacles=scene_tables(n, N // 48)))
    if new and a.reset:
        g = torch.Generator(device="cuda").manual_seed(1)
        rand = lambda n: (torch.rand((n, 4), device="cuda", generator=g) * 2 - 1).contiguous()
        for safe in (False, True):
            out[f"reset_safe_{int(safe)}"] = timed(HoverEnv, 1, N, action=rand, steps=32, scene_kwargs=dict(obstacles=RESET_TABLE, safe_spawn=safe))
        sys.path.insert(0, os.path.join(os.path.abspath(a.root), "tests"))
        import numpy as np
        import _scene_ref as S
        boxes = HoverEnv(num_agent_per_scene=64, seed=SEED, dynamics_kwargs=dict(KW), device="cuda:0")._boxes       # HoverEnv's own spawn box
        att = [S.safe_spawn_ref(SEED, np.arange(N), ep, boxes, [RESET_TABLE], N, 0.1, True)[2] for ep in (2, 3)]
        out["reset_attempts"] = [float(np.mean(x) + 1) for x in att]
        out["reset_attempts_max"] = int(max(x.max() for x in att) + 1)
    print("RESULT " + json.dumps(out))


def run(root, label, a, reset):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--label", label, "--iters", str(a.iters), "--reps", str(a.reps)]
    p = subprocess.run(cmd + (["--reset"] if reset else []), capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"{label}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--reset", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_tables.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    this, parent = [], []
    for rnd in range(a.rounds):                       # alternating, one fresh process each
        if a.parent:
            parent.append(run(a.parent, "parent", a, False))
        this.append(run(ROOT, "this", a, rnd == 0))
    L = [f"tools/exp_scene_tables.py: {this[0]['device']}, bodyrate / Euler / delay ring, hover action (no episode ends) unless stated",
         f"mean device us per vf_env_step launch: HIP events around {a.iters} back-to-back launches, {a.reps} repetitions per process, "
         f"{a.rounds} fresh processes per tree" + (", parent and this tree alternating" if a.parent else ""),
         "agents: 65 536 (no table, shared table, 1 024 scenes x 64) and 65 520 (1 365 scenes x 48: two waves in three straddle two scenes)", "",
         f"{'configuration':<36}{'mean':>9}{'min':>9}{'max':>9}   means of the runs"]

    def row(label, runs, key):
        m, lo, hi, means = stats(runs, key)
        L.append(f"{label:<36}{m:9.3f}{lo:9.3f}{hi:9.3f}   " + " ".join(f"{x:.3f}" for x in means))
        return m, lo, hi, means

    verdicts = []
    for name in ("hover", "nav"):
        for key, what in [("none", "no table")] + [(f"shared_{n}", f"shared table, {n:2d}") for n in COUNTS]:
            t = row(f"this    {name}  {what}", this, f"{name}_{key}")
            if parent:
                p = row(f"parent  {name}  {what}", parent, f"{name}_{key}")
                spread = max(max(p[3]) - min(p[3]), p[2] - p[1])
                verdicts.append(f"{name}, {what}: this - parent = {t[0] - p[0]:+.3f} us; the parent's own runs spread over {max(p[3]) - min(p[3]):.3f} us "
                                f"(repetitions {p[1]:.3f} .. {p[2]:.3f}), this tree's over {max(t[3]) - min(t[3]):.3f} us ({t[1]:.3f} .. {t[2]:.3f}) -> " +
                                ("within the parent's spread" if abs(t[0] - p[0]) <= spread else "OUTSIDE the parent's spread"))
        for n in COUNTS:
            row(f"this    {name}  per scene x64, {n:2d}", this, f"{name}_s64_{n}")
            row(f"this    {name}  per scene x48, {n:2d}", this, f"{name}_s48_{n}")
    off, on = row("this    reset regime, safe_spawn off", this[:1], "reset_safe_0"), row("this    reset regime, safe_spawn on", this[:1], "reset_safe_1")
    L += ["", *verdicts,
          f"reset regime (HoverEnv, 65 536 agents, 32-step episodes, U(-1, 1) actions, a ball and a pillar in the spawn box): safe_spawn on - off = "
          f"{on[0] - off[0]:+.3f} us per launch; host restatement, same seed: {this[0]['reset_attempts'][0]:.3f} / {this[0]['reset_attempts'][1]:.3f} attempts per "
          f"spawn on average (episodes 2 / 3), at most {this[0]['reset_attempts_max']}", ""]
    facts = []
    if os.path.exists(a.out):                          # the hand-written part of the file
        old = open(a.out).read().splitlines()
        at = [k for k, ln in enumerate(old) if ln.startswith(BUILD_FACTS)]
        facts = old[at[0]:] if at else []
    text = "\n".join(L + facts) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
