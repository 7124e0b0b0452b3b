#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden-vector generator for the navigation adjoint with analytic obstacles.  Runs ONLY where the reference is
importable.

tests/golden/bptt_nav_obstacles.npz: NavigationEnv, N = 64, H = 12, bodyrate, Euler -- oracle/gen_golden.py::gen_bptt's format for a case
with options (state, hits, noise_rel, judged, ...), plus the obstacle table and per-step counts of the agents whose closest scene point
lies on an obstacle.

The recorder is driven unmodified: this script adds one entry to the case table gen_bptt reads, swaps the function that plants the initial
states, and wraps the reference's ``DroneEnvsBase.update_collision``: the wrapped call first runs as it is (the bounding-box branch; its
point is checked against candidate 0 of the host reference), then once more as the reference's own visual branch with a scene manager
whose closest point is tests/_obstacle_ref.py's answer for ``position.detach()`` -- so that the reference's own lines form
``collision_vector = collision_point.detach() - position``, the distance and ``is_collision`` from it, on its own autograd tape.  In the
recorder's double-precision repeat the same rule answers in float64.

Usage:  python tools/gen_obstacle_golden.py [--seed S]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))
import gen_golden as G  # noqa: E402
import _obstacle_ref as R  # noqa: E402
from visfly_amd.envs.obstacles import obstacle_rows  # noqa: E402

NAME = "bptt_nav_obstacles"
# beside, behind and under the spawn region of plant_nav_branches (x in [0, 2], y in [-2, 2], z in [2.5, 4.5]); the fast agents fly along +x,
# away from all of them
TABLE = [dict(type="box", lo=[-1.0, 2.6, 2.0], hi=[3.0, 3.0, 5.0]),
         dict(type="pillar", center=[1.0, -2.8], radius=0.3, z=[0.0, 6.0]),
         dict(type="sphere", center=[-0.8, 0.0, 3.5], radius=0.5)]


def plant(rng, fs, consts):
    """plant_nav_branches, then agents 32-39 0.3..0.7 m in front of the box (32-35 flying at it, 36-39 away from it) and agents 40-47
    0.3..0.6 m from the pillar (40-43 at it, 44-47 away): obstacle winners with 1 - dis > 0 on both sides of the approach relu; the other
    slow agents are the obstacle winners with 1 - dis <= 0.  Nobody comes within uav_radius of a solid inside the horizon"""
    fs = PLANT_NAV(rng, fs, consts)
    u = lambda lo, hi, n: rng.uniform(lo, hi, size=n).astype(np.float32)
    fs[32:40, 1] = u(1.9, 2.3, 8)
    fs[32:36, 8], fs[36:40, 8] = u(0.3, 1.0, 4), -u(0.3, 1.0, 4)
    fs[40:48, 0], fs[40:48, 1] = u(0.8, 1.2, 8), -u(1.9, 2.2, 8)
    fs[40:44, 8], fs[44:48, 8] = -u(0.3, 1.0, 4), u(0.3, 1.0, 4)
    return fs


class _Scene:
    """what the visual branch of update_collision asks a scene manager (droneEnv.py:336-342)"""

    def __init__(self, envs, inner, log):
        self.envs, self.inner, self.log = envs, inner, log

    def __getattr__(self, k):
        return getattr(self.inner, k)

    def _answer(self):
        import torch as th
        pos = self.envs.dynamics.position.detach()
        p = pos.numpy()
        query = R.scene_query if p.dtype == np.float32 else R.scene_query64
        cp, g, win = query(p, TABLE)
        return th.from_numpy(cp).to(pos.dtype), win, p

    def get_collision_point(self, indices=None):
        cp, win, p = self._answer()
        if indices is None:
            if p.dtype == np.float32:
                self.log.append(win.copy())
            return cp
        return cp[indices]

    @property
    def is_out_bounds(self):
        import torch as th
        p = self.envs.dynamics.position.detach().numpy()
        return th.from_numpy(np.any((p < np.asarray(R.ROOM_LO)) | (p > np.asarray(R.ROOM_HI)), axis=1))


def wrap_update_collision(log):
    G.import_envs()
    import torch as th
    import VisFly.envs.base.droneEnv as DE
    real = DE.DroneEnvsBase.update_collision

    def update_collision(self, indices=None):
        real(self, indices)                                     # the bounding-box branch, as it is
        if indices is None:                                     # ... is candidate 0 of the rule
            p = self.dynamics.position.detach().numpy()
            room = R._room(p, R.ROOM_LO, R.ROOM_HI, p.dtype.type)
            assert np.array_equal(room, self._collision_point.numpy()), "the host reference's room-box candidate is not the reference's"
        once = self._once_collided.clone()
        scene, visual = self.sceneManager, self.visual
        self.sceneManager, self.visual = _Scene(self, scene, log), True
        try:
            real(self, indices)                                 # the visual branch + droneEnv.py:364-367 with the table's closest point
        finally:
            self.sceneManager, self.visual = scene, visual
        self._once_collided = once | self._is_collision
        assert not self._collision_point.requires_grad

    DE.DroneEnvsBase.update_collision = update_collision

    def stop():
        DE.DroneEnvsBase.update_collision = real
    return stop


def main(seed):
    global PLANT_NAV
    base = G.BPTT_CASES["bptt_nav_branches"]
    kind, dkw, kw, hover, scale, H, opts = base
    assert kind == "nav" and dkw["integrator"] == "euler" and dkw["action_type"] == "bodyrate" and H == 12 and opts["init"] == "nav_branches"
    G.BPTT_CASES[NAME] = (kind, dkw, kw, hover, scale, H, dict(opts, seed=seed, N=64))      # added at run time
    PLANT_NAV, G.plant_nav_branches = G.plant_nav_branches, plant
    log = []
    stop = wrap_update_collision(log)
    try:
        G.gen_bptt(NAME)
    finally:
        stop()
        G.plant_nav_branches = PLANT_NAV
        G.BPTT_CASES.pop(NAME, None)
    path = os.path.join(G.OUT, NAME + ".npz")
    fx = dict(np.load(path))
    N = fx["fs_init"].shape[0]
    assert N == 64 and fx["actions"].shape == (H, 64, 4) and len(log) >= H
    win = np.stack(log[-H:])                                    # the fp32 roll-out's H steps (its resets come before them)
    # cross-check against the stored post-step states, then count: live obstacle winners on each side of the two relus
    live = ~fx["done"].astype(bool)
    counts = np.zeros((H, 5), np.int64)
    for t in range(H):
        p, v = fx["state"][t][:, 0:3], fx["state"][t][:, 7:10]
        cp, g, w = R.scene_query(p, TABLE)
        assert np.array_equal(w, win[t])
        vec = cp - p
        dis = np.sqrt((vec * vec).sum(axis=1))
        ap = (vec * v).sum(axis=1)
        ob = (w > 0) & live[t]
        counts[t] = [ob.sum(), (ob & (1 - dis > 0)).sum(), (ob & (1 - dis <= 0)).sum(), (ob & (ap > 0)).sum(), (ob & (ap <= 0)).sum()]
    print("obstacle winners per step:", counts[:, 0].tolist(), "| near / far / approaching / receding:", counts[:, 1:].sum(axis=0).tolist())
    assert (counts.sum(axis=0) > 0).all(), "an obstacle branch is not taken: move the planted agents"
    names = dict(zip(fx["hit_names"].tolist(), fx["hits"].tolist()))
    assert all(names[k] > 0 for k in ("nav_near_hi", "nav_near_lo", "nav_appr_hi", "nav_appr_lo")), names
    rows = obstacle_rows(R.parse_obstacles(TABLE))            # (n, 8): vf_obstacle's fields [type, a, b, r]
    fx.update(obstacles=np.asarray(repr(R.parse_obstacles(TABLE))), obstacle_rows=rows, obst_winner=win.astype(np.int8), obst_counts=counts,
              obst_count_names=np.asarray(["winners", "near", "far", "approaching", "receding"]))
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) <= 1 << 20, os.path.getsize(path)
    print(f"{path}: {os.path.getsize(path)} bytes, noise_rel {float(fx['noise_rel']):.3e}, judged {int(fx['judged'].sum())}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    main(ap.parse_args().seed)
