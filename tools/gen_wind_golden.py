#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden-vector generator for the env adjoint under string wind functions.  Runs ONLY where the reference is
importable.

The reference re-evaluates ``wind_settings`` given as six expression strings before every step (envs/base/dynamics.py:132-174, 320,
384-388); they depend on the agent's time and their own previous value only, so on its autograd tape the wind is a per-step constant
and ``loss.backward()`` runs through it.  The strings are those of ``dyn_wind_functions`` (oracle/gen_golden.py::DYN_CASES): polynomials
and a recurrence, no transcendental, so evaluating them on the host with GPU tensors stays bit-equal to the reference's CPU.

Per-step adjoint fixtures (oracle/gen_golden.py::gen_bptt's format, N = 70: a multiple of neither 64 nor 256, so the last block of
the adjoint launch has dead lanes behind the last wind row).  Each also stores ``wind`` (H, N, 3), the reference's ``wind_velocity``
during every step, and ``d_actions_nowind``, the reference's gradient of the same case with ``wind_settings`` removed; the velocity
columns of ``fs_init`` / ``ev_fs`` hold the raw velocity (what reset(state=...) takes), not full_state's v + wind:
    bptt_wind_hover          HoverEnv, bodyrate, Euler, delay ring, H = 12, no resets
    bptt_wind_hover_resets   the same with max_episode_steps = 5 (every agent re-spawns, each with a new t, hence a new wind)
    bptt_wind_nav_rk4        NavigationEnv with the constructor arguments of bptt_nav_bodyrate, repaired RK4
Trainer fixtures, by the recorders of bptt_loop_hover.npz / shac_hover.npz with the wind strings in the dynamics kwargs:
    bptt_loop_hover_wind     oracle/gen_shac.py::gen_bptt_loop
    shac_hover_wind          oracle/gen_shac.py::gen_shac; the critic's update trajectory (critic_grad / critic_params / target_params /
                             critic_loss) is dropped from the file, which otherwise exceeds the 1 MiB cap on committed files: the
                             consumer checks the actor half of the iteration, where the wind acts

The recorders are driven unmodified: this script adds entries to the case table gen_bptt reads, swaps the dynamics kwargs the trainer
recorders read, and listens on the reference's ``Dynamics.update_wind`` for the wind of every step.

Usage:  python tools/gen_wind_golden.py [--only NAME ...]
"""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gen_shac as GS  # noqa: E402  (imports gen_golden: stubs, CR-sqrt patch, constants extraction)
import gen_golden as G  # noqa: E402

N = 70
REL_TOL = 1e-5           # tests/test_bptt_gpu.py::REL_TOL, the bound the adjoint tests hold
WIND = list(G.DYN_CASES["dyn_wind_functions"][0]["wind_settings"])
assert len(WIND) == 6 and all(isinstance(s, str) for s in WIND)


def _cases():
    kind, dkw, kw, hover, scale, H = G.BPTT_CASES["bptt_hover_bodyrate"][:6]
    assert kind == "hover" and dkw["integrator"] == "euler" and dkw["ctrl_delay"] and H == 12
    rk, rdkw, rkw, rhover, rscale, rH = G.BPTT_CASES["bptt_hover_resets"][:6]
    assert rkw["max_episode_steps"] == 5
    nk, ndkw, nkw, nhover, nscale, nH = G.BPTT_CASES["bptt_nav_bodyrate"][:6]
    assert nk == "nav"
    return {
        "bptt_wind_hover": (kind, dict(dkw), kw, hover, scale, H),
        "bptt_wind_hover_resets": (rk, dict(rdkw), rkw, rhover, rscale, rH),
        "bptt_wind_nav_rk4": (nk, dict(ndkw, integrator="rk4"), nkw, nhover, nscale, nH),
    }


def _listen():
    """the reference's wind_velocity after every update_wind() call (the first one is the constructor's, one per step follows), and
    with every read of ``full_state`` -- whose velocity columns are v + wind (dynamics.py:752,793) -- the raw velocity behind it"""
    G.import_envs()
    import VisFly.envs.base.dynamics as D
    real, real_fs, seen, reads = D.Dynamics.update_wind, D.Dynamics.full_state, [], []

    def update_wind(self):
        real(self)
        seen.append(G.f32(self.wind_velocity).T.copy())       # (N, 3) or (1, 3)

    def full_state(self):
        fs = real_fs.fget(self)
        reads.append((G.f32(fs).copy(), G.f32(self._velocity).T.copy()))
        return fs
    D.Dynamics.update_wind, D.Dynamics.full_state = update_wind, property(full_state)

    def stop():
        D.Dynamics.update_wind, D.Dynamics.full_state = real, real_fs
    return seen, reads, stop


def _raw_velocity(reads, rows, agents):
    """full_state rows as the recorder stored them -> the raw velocity of the read they came from (the latest one that matches bit
    for bit): what reset(state=...) takes, on both sides"""
    out = np.empty((len(rows), 3), np.float32)
    for j, (row, i) in enumerate(zip(rows, agents)):
        hit = [raw[i] for full, raw in reversed(reads) if np.array_equal(full[i].view(np.uint32), row.view(np.uint32))]
        assert hit, "no full_state read matches the stored row"
        out[j] = hit[0]
    return out


def gen_adjoint(name):
    kind, dkw, kw, hover, scale, H = _cases()[name]
    out, tmp = G.OUT, tempfile.mkdtemp(prefix="vf_wind_golden_")
    try:
        # the same case without wind_settings -> d_actions_nowind (into a scratch folder)
        G.BPTT_CASES[name] = (kind, dict(dkw), kw, hover, scale, H)
        G.OUT = tmp
        G.gen_bptt(name, N=N)
        bare = dict(np.load(os.path.join(tmp, name + ".npz")))
        # ... and with it
        G.BPTT_CASES[name] = (kind, dict(dkw, wind_settings=list(WIND)), kw, hover, scale, H)
        seen, reads, stop = _listen()
        try:
            G.gen_bptt(name, N=N)
        finally:
            stop()
        fx = dict(np.load(os.path.join(tmp, name + ".npz")))
    finally:
        G.OUT = out
        G.BPTT_CASES.pop(name, None)
        shutil.rmtree(tmp, ignore_errors=True)
    assert len(seen) == H + 1 and all(w.shape == (N, 3) for w in seen), (len(seen), seen[0].shape)
    wind = np.stack(seen[1:])
    # the same actions, weights and spawn; full_state's velocity columns carry the wind (dynamics.py:752)
    same = [c for c in range(22) if not 7 <= c < 10]
    assert fx["actions"].shape == (H, N, 4) and all(np.array_equal(fx[k], bare[k]) for k in ("actions", "Wr", "Wo"))
    assert np.array_equal(fx["fs_init"][:, same], bare["fs_init"][:, same])
    assert "wind_settings" in str(fx["dyn_kw"])
    g, g0 = fx["d_actions"], bare["d_actions"]
    moved = np.abs(g - g0).max() / (REL_TOL * np.abs(g).max())
    print(f"{name}: wind moves dL/da by {moved:.1f} x the adjoint tolerance; |wind| per axis {np.abs(wind).max((0, 1))}; "
          f"re-spawns {len(fx['ev_step'])}" + (f", {int((fx['ev_fs'][:, 21] != 0).sum())} with t != 0" if len(fx["ev_step"]) else ""))
    # conditions, not measurements: an adjoint that ignores the wind, or takes another step's, cannot pass on these files
    assert (np.abs(wind) > 0).any((0, 1)).all(), "wind is zero on an axis"
    if name != "bptt_wind_nav_rk4":
        assert moved >= 50, "the wind moves the gradient by less than 50 x the adjoint tolerance: scale the wind strings"
    if name == "bptt_wind_hover":
        assert len(fx["ev_step"]) == 0
    if name == "bptt_wind_hover_resets":
        assert len(fx["ev_step"]) and (fx["ev_fs"][:, 21] != 0).any(), "no re-spawn with t != 0"
    # reset(state=...) writes the velocity columns as the raw velocity (here and in the reference), so the stored spawn / re-spawn
    # states carry that instead of full_state's v + wind: the consumer replays them through reset(state=...) / reset_agent_by_id
    fx["fs_init"][:, 7:10] = _raw_velocity(reads, fx["fs_init"], range(N))
    assert np.array_equal(fx["fs_init"], bare["fs_init"])
    if len(fx["ev_step"]):
        fx["ev_fs"][:, 7:10] = _raw_velocity(reads, fx["ev_fs"], fx["ev_agent"])
    fx.update(wind=wind, d_actions_nowind=g0, wind_fn=np.asarray(WIND))
    np.savez_compressed(os.path.join(G.OUT, name + ".npz"), **fx)


def gen_trainer(name):
    """gen_bptt_loop / gen_shac read `G.ENV_DYN` when they build the env and when they store dyn_kw"""
    real = G.ENV_DYN
    G.ENV_DYN = dict(real, wind_settings=list(WIND))
    try:
        if name == "bptt_loop_hover_wind":
            GS.gen_bptt_loop(name=name)
        else:
            GS.gen_shac(name=name)
    finally:
        G.ENV_DYN = real
    path = os.path.join(GS.OUT, name + ".npz")
    fx = dict(np.load(path))
    assert "wind_settings" in str(fx["dyn_kw"])
    if name == "shac_hover_wind":
        for k in ("critic_grad", "critic_params", "target_params", "critic_loss"):
            del fx[k]
        np.savez_compressed(path, **fx)
    assert os.path.getsize(path) <= 1 << 20, (name, os.path.getsize(path))


ALL = ("bptt_wind_hover", "bptt_wind_hover_resets", "bptt_wind_nav_rk4", "bptt_loop_hover_wind", "shac_hover_wind")

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None, choices=ALL)
    a = ap.parse_args()
    os.makedirs(G.OUT, exist_ok=True)
    for nm in a.only or ALL:
        (gen_adjoint if nm.startswith("bptt_wind_") else gen_trainer)(nm)
