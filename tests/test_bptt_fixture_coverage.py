"""The saturation / clamp BPTT fixtures (oracle/gen_golden.py::gen_bptt, cases with an options entry) are where they claim to be:
recounted here in numpy fp32 from the stored actions, constants, post-step states and done flags, every thrust-clamp side and tie,
every _ugly_fix clamp and the done-cut agents equal the generator's `hits` (counted there from the reference's own tensors), and
every side a fixture is there for is populated.  Conditions on the INPUTS of the GPU tests (tests/test_bptt_masks_gpu.py), no GPU."""
import numpy as np
import pytest

from _golden import consts_of, load

# fixture -> the sides it must populate with >= MIN_SIDE live rotor-steps (thr_*) / state-component-steps / agent-steps.
# The thrust action type has no "below T_min" side: Traw = m (a acc_half + acc_mean) reaches T_min = 0 exactly at a = -1.0f, the
# lowest legal action, so its lower side is the tie alone.  p_z has no ceiling side (gen_golden.py, next to the case).
REQUIRED = {
    "bptt_racing_thrust_sat": ("thr_hi", "thr_free"),
    "bptt_hover_thrust_sat_nodelay": ("thr_hi", "thr_free"),
    "bptt_hover_thrust_sat_rk4": ("thr_hi", "thr_free"),
    "bptt_hover_bodyrate_sat": ("thr_lo", "thr_hi", "thr_free"),
    "bptt_hover_state_clamps": ("v_lo", "v_hi", "w_lo", "w_hi", "pz_lo", "thr_lo", "thr_hi", "thr_free"),
    "bptt_racing_thrust_h64": ("thr_hi", "thr_free", "done_cut"),
    # |v| == 0 (nav_v_zero) cannot be reached by a live agent: gen_golden.py, next to the case
    "bptt_nav_branches": ("nav_close_hi", "nav_close_lo", "nav_view_hi", "nav_view_lo", "nav_near_hi", "nav_near_lo", "nav_appr_hi", "nav_appr_lo"),
    "bptt_nav_rk4_drag": ("nav_close_hi", "nav_close_lo", "nav_view_hi", "nav_view_lo", "thr_free"),
}
TIES = {"bptt_racing_thrust_sat": ("thr_tie_lo", "thr_tie_hi"), "bptt_hover_thrust_sat_nodelay": ("thr_tie_lo", "thr_tie_hi"),
        "bptt_hover_thrust_sat_rk4": ("thr_tie_lo", "thr_tie_hi")}
SATURATION = ("bptt_racing_thrust_sat", "bptt_hover_thrust_sat_nodelay", "bptt_hover_thrust_sat_rk4", "bptt_hover_bodyrate_sat")
MIN_SIDE, MIN_TIE = 32, 8


def applied_thrust_actions(fx):
    """the action the thrust type applies in step t: the one given delay_steps earlier; the ring starts as zeros and an agent's slots
    are zeroed when it is re-spawned (dynamics.py:243,262-263,323-326)"""
    a, done = fx["actions"], fx["done"].astype(bool)
    H, N = a.shape[:2]
    D = int(fx["c_delay_steps"])
    ring = [np.zeros((N, 4), np.float32) for _ in range(D)]
    out = np.zeros_like(a)
    for t in range(H):
        ring.append(a[t].copy())
        out[t] = ring.pop(0)
        for slot in ring[:D]:
            slot[done[t]] = 0
    return out


@pytest.mark.parametrize("name", sorted(REQUIRED))
def test_fixture_populates_the_sides_it_is_there_for(name):
    fx = load(name)
    c = consts_of(fx)
    hits = dict(zip([str(k) for k in fx["hit_names"]], fx["hits"].tolist()))
    done = fx["done"].astype(bool)
    live = ~done
    state = fx["state"]
    H, N = done.shape
    assert state.shape == (H, N, 22) and state.dtype == np.float32
    got = {"done_cut": int(done.sum())}
    # _ugly_fix: a clipped component sits on the limit bit for bit
    for key, cols, lim in (("v_lo", slice(7, 10), -c["vel_lim"]), ("v_hi", slice(7, 10), c["vel_lim"]), ("w_lo", slice(10, 13), -c["omg_lim"]),
                           ("w_hi", slice(10, 13), c["omg_lim"]), ("pz_lo", slice(2, 3), c["pos_z_lo"]), ("pz_hi", slice(2, 3), c["pos_z_hi"])):
        got[key] = int(((state[:, :, cols] == np.float32(lim)) & live[:, :, None]).sum())
    if int(c["action_type"]) == 0:      # thrust: Traw from the actions alone, in fp32 with the reference's operation order
        a = applied_thrust_actions(fx)
        traw = np.float32(c["m"]) * (a * np.float32(c["acc_half"]) + np.float32(c["acc_mean"]))
        assert traw.dtype == np.float32
        T_min, T_max = np.float32(c["T_min"]), np.float32(c["T_max"])
        lr = live[:, :, None]
        got.update(thr_lo=int(((traw < T_min) & lr).sum()), thr_hi=int(((traw > T_max) & lr).sum()),
                   thr_free=int(((traw > T_min) & (traw < T_max) & lr).sum()),
                   thr_tie_lo=int(((traw == T_min) & lr).sum()), thr_tie_hi=int(((traw == T_max) & lr).sum()))
        assert np.float32(c["m"]) * (np.float32(-1.0) * np.float32(c["acc_half"]) + np.float32(c["acc_mean"])) == T_min
    print(f"{name}: " + ", ".join(f"{k} {v}" + (f" (recounted {got[k]})" if k in got else "") for k, v in hits.items()))
    for k, v in got.items():
        assert v == hits[k], f"{name}: {k} recounted {v}, generator {hits[k]}"
    for k in REQUIRED[name]:
        assert hits[k] >= MIN_SIDE, f"{name}: only {hits[k]} live hits on {k}"
    for k in TIES.get(name, ()):
        assert hits[k] >= MIN_TIE, f"{name}: planted tie {k} occurs {hits[k]} times"
    if name in TIES:
        assert int((fx["actions"] == np.float32(1.0)).sum()) >= MIN_TIE and int((fx["actions"] == np.float32(-1.0)).sum()) >= MIN_TIE
    if name == "bptt_racing_thrust_h64":          # gate passes and re-spawns inside the horizon
        assert hits["gate_pass"] >= 8 and len(fx["ev_step"]) == hits["done_cut"] and fx["actions"].shape[0] == 64
    if "drag_lin" in fx:      # per-agent coefficients, within the +-50 % of drag_random = 0.5 around the constants
        for key, mean in (("drag_lin", c["k_lin"]), ("drag_quad", c["k_quad"])):
            f = fx[key] / mean.reshape(1, 3)
            assert fx[key].shape == (N, 3) and len(np.unique(f[:, 0])) == N and f.min() >= 0.5 - 1e-6 and f.max() <= 1.5 + 1e-6
        assert int(c["integrator"]) == 1
    if name in SATURATION:
        rotor_steps = 4 * int(live.sum())
        clamped = hits["thr_lo"] + hits["thr_hi"]
        assert hits["thr_free"] + hits["thr_tie_lo"] + hits["thr_tie_hi"] + clamped == rotor_steps
        assert 4 * hits["thr_free"] >= rotor_steps, f"{name}: {hits['thr_free']} of {rotor_steps} rotor-steps unclamped"
        assert 4 * clamped >= rotor_steps, f"{name}: {clamped} of {rotor_steps} rotor-steps clamped"
    assert float(fx["noise_rel"]) > 0 and fx["same64"].mean() >= 0.9
