#!/usr/bin/env python3
"""What an obstacle table costs the fused env step -> profiles/obstacles.txt.

Mean device microseconds per vf_env_step launch (HIP events around back-to-back launches on one stream, vf_env_time_steps) at 65 536
agents, bodyrate / Euler / delay ring, HoverEnv and NavigationEnv, with 0, 1, 4 and 16 obstacles -- and, for one sphere, per step of the
split path the table replaces: step_begin, a closest point per agent in torch, step_finish (torch events around the loop: that path is
several launches per step).

    python tools/exp_obstacles.py [--parent TREE] [--agents 65536] [--iters 2000] [--reps 5] [--rounds 3]

--parent: another built checkout of this project (the parent commit's) whose 0-obstacle launch is timed in the same session, alternating
with this tree's, one fresh process per run; the spread of the parent's own repeated runs is what the 0-obstacle difference is read
against.  Without it only this tree is measured.  The driver starts the runs one after the other (--child is the measuring process).
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
KW = dict(action_type="bodyrate", integrator="euler", dt=0.0025, ctrl_dt=0.02, ctrl_delay=True)
COUNTS = (0, 1, 4, 16)


def table(n):
    """n solids spread over the room, away from the spawn boxes (the timed launches run the hover action: nobody ends an episode on them);
    the three primitives in turn"""
    out = []
    for k in range(n):
        x, y = 6.0 + 2.5 * (k % 4), -6.0 + 3.0 * (k // 4)
        out.append([dict(type="sphere", center=[x, y, 2.0], radius=0.5), dict(type="box", lo=[x - 0.4, y - 0.4, 0.0], hi=[x + 0.4, y + 0.4, 3.0]),
                    dict(type="pillar", center=[x, y], radius=0.4, z=[0.0, 4.0])][k % 3])
    return out


def child(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from visfly_amd import _lib
    from visfly_amd.envs import HoverEnv, NavigationEnv
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(a.root)), _lib.__file__
    has = "vf_env_set_obstacles" in _lib.SIGNATURES
    N, dev = a.agents, torch.device("cuda", 0)
    out = {"label": a.label, "agents": N, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    hover = torch.tensor([-1 / 3, 0, 0, 0], device=dev).repeat(N, 1).contiguous()
    for name, cls in (("hover", HoverEnv), ("nav", NavigationEnv)):
        for n in (COUNTS if has else (0,)):
            kw = dict(scene_kwargs=dict(obstacles=table(n))) if n else {}
            env = cls(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(KW), device="cuda:0", tensor_output=True, max_episode_steps=100000, **kw)
            env.reset()
            env.time_steps(hover, iters=200)                                   # warm-up: code objects, constant blocks in L2
            us = [round(env.time_steps(hover, iters=a.iters), 3) for _ in range(a.reps)]
            out[f"{name}_{n}"] = us
            env.close()
    if has and a.split:
        env = HoverEnv(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(KW), device="cuda:0", tensor_output=True, max_episode_steps=100000)
        env.reset()
        centre, radius = torch.tensor([8.0, 0.0, 2.0], device=dev), 0.5
        oob = torch.zeros(N, dtype=torch.bool, device=dev)
        pose = None

        def step():
            nonlocal pose
            pose = env.step_begin(hover, pose)
            d = pose["position"] - centre
            dist = d.norm(dim=1, keepdim=True).clamp_min(1e-6)
            cp = torch.where(dist <= radius, pose["position"], centre + d * (radius / dist))     # the solid sphere's closest point
            env.step_finish(cp, oob)
        for _ in range(50):
            step()
        torch.cuda.synchronize()
        us, k = [], max(200, a.iters // 4)
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                step()
            e1.record()
            torch.cuda.synchronize()
            us.append(round(e0.elapsed_time(e1) * 1e3 / k, 3))
        out["split_hover_1"] = us
        env.close()
    print("RESULT " + json.dumps(out))


def run(root, label, a, split):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--label", label, "--agents", str(a.agents),
           "--iters", str(a.iters), "--reps", str(a.reps)] + (["--split"] if split else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"{label}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def stats(runs, key):
    """all repetitions of all runs of one tree -> (mean, min, max, run means)"""
    vals = [v for r in runs for v in r[key]]
    means = [sum(r[key]) / len(r[key]) for r in runs]
    return sum(vals) / len(vals), min(vals), max(vals), means


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--agents", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacles.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    this, parent = [], []
    for rnd in range(a.rounds):                       # alternating, one fresh process each
        if a.parent:
            parent.append(run(a.parent, "parent", a, False))
        this.append(run(ROOT, "this", a, rnd == 0))
    L = []
    L.append(f"tools/exp_obstacles.py: {this[0]['device']}, {a.agents} agents, bodyrate / Euler / delay ring, hover action (no episode ends)")
    L.append(f"mean device us per vf_env_step launch: HIP events around {a.iters} back-to-back launches, {a.reps} repetitions per process, "
             f"{a.rounds} fresh processes per tree" + (", parent and this tree alternating" if a.parent else ""))
    L.append("")
    L.append(f"{'configuration':<28}{'mean':>9}{'min':>9}{'max':>9}   means of the runs")
    rows = {}
    for name in ("hover", "nav"):
        if parent:
            m, lo, hi, means = stats(parent, f"{name}_0")
            rows[f"parent {name}_0"] = (m, lo, hi, means)
            L.append(f"{'parent  ' + name + '  0 obstacles':<28}{m:9.3f}{lo:9.3f}{hi:9.3f}   " + " ".join(f"{x:.3f}" for x in means))
        for n in COUNTS:
            m, lo, hi, means = stats(this, f"{name}_{n}")
            rows[f"{name}_{n}"] = (m, lo, hi, means)
            L.append(f"{'this    ' + name + f' {n:2d} obstacles':<28}{m:9.3f}{lo:9.3f}{hi:9.3f}   " + " ".join(f"{x:.3f}" for x in means))
    m, lo, hi, means = stats(this[:1], "split_hover_1")
    rows["split"] = (m, lo, hi, means)
    L.append(f"{'this    split path, 1 sphere':<28}{m:9.3f}{lo:9.3f}{hi:9.3f}   (step_begin + torch closest point + step_finish, per step)")
    L.append("")
    if parent:
        for name in ("hover", "nav"):
            pm, plo, phi, pmeans = rows[f"parent {name}_0"]
            tm = rows[f"{name}_0"][0]
            spread = max(pmeans) - min(pmeans)
            L.append(f"{name}: 0 obstacles, this - parent = {tm - pm:+.3f} us; the parent's own runs spread over {spread:.3f} us "
                     f"(repetitions {plo:.3f} .. {phi:.3f}) -> " + ("within the parent's spread" if abs(tm - pm) <= max(spread, phi - plo) else "OUTSIDE the parent's spread"))
    f16, sp = rows["hover_16"][0], rows["split"][0]
    L.append(f"hover: 16 obstacles fused {f16:.3f} us vs the split path with one sphere {sp:.3f} us -> " +
             ("the fused step is faster" if f16 < sp else "the fused step is NOT faster"))
    for name in ("hover", "nav"):
        L.append(f"{name}: per obstacle (16 vs 1) {(rows[f'{name}_16'][0] - rows[f'{name}_1'][0]) / 15:.3f} us; the first obstacle (general kernel instead of "
                 f"the straight-line instance, + one entry) {rows[f'{name}_1'][0] - rows[f'{name}_0'][0]:+.3f} us")
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
