"""The references of tests/_glue_ref.py against torch's own autograd / optimiser in fp64, and the comparators' teeth.

Nothing here touches a GPU or the library.  Two halves:
  * every reference formula is what autograd (or torch.optim.Adam, clip_grad_norm_, the in-place Polyak pair) gives in fp64, at the
    edges the GPU cases use: log_std on, one fp32 step outside and far outside the clamp bounds, exact ties between the Q heads,
    M_global != M, done bytes other than 0 / 1, a stale episode-done bit on an agent that is not done;
  * for every comparator and every input set of tests/test_trainer_glue_gpu.py the float32 reference passes ("the reference alone
    stays within the bound"), and every listed mutant of the reference fails.  The mutants are applied in numpy / torch on the host;
    no wrong kernel is ever built.
"""
import numpy as np
import pytest
import torch

import _glue_ref as R
from _glue_ref import F32, F64

def rejects(check, got, inp):
    with pytest.raises(AssertionError):
        check(got, inp)


def close64(got, want, what, rtol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want).max()
    assert err <= rtol * max(np.abs(want).max(), 1e-300), f"{what}: {err:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# references against autograd / torch.optim in fp64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", R.HEAD_BOUNDS)
@pytest.mark.parametrize("phase", R.HEAD_PHASES)
def test_head_reference_is_autograd_of_the_forward(lo, hi, phase):
    inp = R.head_inputs(65, lo, hi, phase)
    sp = set(R.head_log_std_specials(lo, hi).tolist())
    assert sp <= set(inp["log_std"][-1].tolist()) | set(R.head_inputs(65, lo, hi, phase + 4)["log_std"][-1].tolist())
    for c in range(4):
        assert sp <= set(inp["log_std"][:, c].tolist())
    mu = torch.from_numpy(inp["mu"]).double().requires_grad_()
    ls = torch.from_numpy(inp["log_std"]).double().requires_grad_()
    eps, da = torch.from_numpy(inp["eps"]).double(), torch.from_numpy(inp["d_action"]).double()
    a = torch.tanh(mu + eps * torch.exp(torch.clamp(ls, R.f32(lo), R.f32(hi))))
    a.backward(da)
    close64(R.head_fwd(inp["mu"], inp["log_std"], inp["eps"], lo, hi, F64), a.detach().numpy(), "head_fwd", 1e-15)
    # the backward reads the SAVED action: give it autograd's own
    r = R.head_bwd(inp["d_action"], a.detach().numpy(), inp["log_std"], inp["eps"], lo, hi, F64)
    close64(r["d_mu"], mu.grad.numpy(), "d_mu")
    close64(r["d_log_std"], ls.grad.numpy(), "d_log_std")
    lsv = inp["log_std"]
    on_edge = (lsv == np.float32(lo)) | (lsv == np.float32(hi))
    live = on_edge & (np.abs(a.detach().numpy()) < 0.99)
    assert live.any() and np.all(ls.grad.numpy()[live] != 0), "th.clamp passes the gradient ON the bounds"
    outside = (lsv < np.float32(lo)) | (lsv > np.float32(hi))
    assert outside.sum() >= 4 and not np.any(ls.grad.numpy()[outside]) and not np.any(r["d_log_std"][outside])


def test_reparam_reference_is_autograd_of_the_forward():
    inp = R.reparam_inputs(65)
    mean = torch.from_numpy(inp["mean"]).double().requires_grad_()
    ls = torch.from_numpy(inp["log_std"]).double().requires_grad_()
    eps, da = torch.from_numpy(inp["eps"]).double(), torch.from_numpy(inp["d_action"]).double()
    a = torch.tanh(mean + torch.exp(ls) * eps)
    a.backward(da)
    close64(R.reparam_fwd(inp["mean"], inp["log_std"], inp["eps"], F64), a.detach().numpy(), "reparam_fwd", 1e-15)
    r = R.reparam_bwd(inp["d_action"], a.detach().numpy(), inp["log_std"], inp["eps"], inp["g_log_std"], F64)
    close64(r["d_mean"], mean.grad.numpy(), "d_mean")
    # per-row contributions on top of the accumulator; their sum over the rows is the parameter's gradient
    close64((r["g_log_std"] - inp["g_log_std"].astype(np.float64)).sum(0), ls.grad.numpy(), "g_log_std summed over rows", 1e-11)


@pytest.mark.parametrize("M,M_global", [(257, 257), (257, 772)])
def test_twin_q_reference_is_autograd_of_the_mse(M, M_global):
    inp = R.twin_q_inputs(M, M_global)
    assert (inp["q0"] == inp["q1"]).sum() >= M // 7
    q0 = torch.from_numpy(inp["q0"]).double().requires_grad_()
    q1 = torch.from_numpy(inp["q1"]).double().requires_grad_()
    values, _ = torch.cat([q0.view(-1, 1), q1.view(-1, 1)], dim=1).min(dim=1)
    loss = torch.nn.functional.mse_loss(torch.from_numpy(inp["target"]).double(), values) * M / M_global
    loss.backward()
    r = R.twin_q_loss(inp["q0"], inp["q1"], inp["target"], M_global, F64)
    close64(r["loss"], [loss.item()], "loss")
    close64(r["dq0"], q0.grad.numpy(), "dq0")
    close64(r["dq1"], q1.grad.numpy(), "dq1")
    tie = inp["q0"] == inp["q1"]
    assert np.all(q0.grad.numpy()[tie] != 0) and not np.any(q1.grad.numpy()[tie]), "a tie sends the whole gradient to the first head"
    assert np.array_equal(r["dq0"] == 0, q0.grad.numpy() == 0) and np.array_equal(r["dq1"] == 0, q1.grad.numpy() == 0)


def test_bptt_d_reward_is_autograd_of_the_mean_loss():
    H, N = 5, 65
    inp = R.horizon_inputs(H, N)
    rew = torch.from_numpy(inp["reward"]).double().requires_grad_()
    done = torch.from_numpy(inp["done"]) != 0
    gamma = R.f32(inp["gamma"])
    disc0, loss0 = torch.from_numpy(inp["disc"]).double(), torch.from_numpy(inp["loss"]).double()
    actor_loss, discount_factor = loss0, disc0
    for t in range(H):                                                   # BPTT.py:123-124
        actor_loss = actor_loss + -1 * rew[t] * discount_factor
        discount_factor = discount_factor * gamma * ~done[t] + done[t]
    actor_loss.mean().backward()
    d, l = inp["disc"].astype(np.float64), inp["loss"].astype(np.float64)
    for t in range(H):
        o = R.bptt_accumulate(inp["reward"][t], inp["done"][t], d, l, gamma, 1.0 / N, F64)
        close64(o["d_reward"], rew.grad[t].numpy(), f"d_reward[{t}]", 1e-7)       # scale is the fp32 1 / N
        d, l = o["disc"], o["loss"]
    close64(l, actor_loss.detach().numpy(), "loss", 1e-15)
    close64(d, discount_factor.numpy(), "disc", 1e-15)


def test_shac_d_reward_is_autograd_of_the_mean_loss():
    H, N = 5, 65
    inp = R.horizon_inputs(H, N)
    rew = torch.from_numpy(inp["reward"]).double().requires_grad_()
    done = torch.from_numpy(inp["done"]) != 0
    # the reference's episode_done is info[i]["episode_done"] of an agent that is done; a stale bit elsewhere means nothing
    episode_done = done & ((torch.from_numpy(inp["ep_flags"]) & 8) != 0)
    assert ((inp["done"] == 0) & ((inp["ep_flags"] & 8) != 0)).any() and (inp["done"] == 255).any()
    gamma = R.f32(inp["gamma"])
    q0, q1 = torch.from_numpy(inp["q0"]).double(), torch.from_numpy(inp["q1"]).double()
    actor_loss, discount_factor = torch.from_numpy(inp["loss"]).double(), torch.from_numpy(inp["disc"]).double()
    nvs = []
    for t in range(H):                                                   # shac.py:238-246
        next_values, _ = torch.cat([q0[t].view(-1, 1), q1[t].view(-1, 1)], dim=1).min(dim=1)
        actor_loss = actor_loss - rew[t] * discount_factor
        done_but_not_episode_end = (done[t] | (t == H - 1)) & ~episode_done[t]
        if done_but_not_episode_end.any():
            actor_loss = actor_loss - next_values * discount_factor * gamma * done_but_not_episode_end
        discount_factor = discount_factor * gamma * ~done[t] + done[t]
        nvs.append(next_values)
    actor_loss.mean().backward()
    o = R.shac_accumulate_horizon(inp["reward"], inp["done"], inp["ep_flags"], inp["q0"], inp["q1"], inp["disc"].astype(np.float64),
                                  inp["loss"].astype(np.float64), gamma, 1.0 / N, F64)
    close64(o["d_reward"], rew.grad.numpy(), "d_reward", 1e-7)                     # scale is the fp32 1 / N
    close64(o["loss"], actor_loss.detach().numpy(), "loss", 1e-15)
    close64(o["disc"], discount_factor.numpy(), "disc", 1e-15)
    assert np.array_equal(o["next_value"], torch.stack(nvs).numpy()) and np.array_equal(o["ep_done"], episode_done.numpy().astype(np.uint8))


def _torch_adam(inp, dtype, steps):
    cfg = inp["cfg"]
    p = torch.nn.Parameter(torch.from_numpy(inp["p"]).to(dtype).clone())
    opt = torch.optim.Adam([p], lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"], weight_decay=cfg["weight_decay"],
                           foreach=False)
    out = []
    for k in range(steps):
        p.grad = torch.from_numpy(inp["grads"][k]).to(dtype).clone()
        if cfg["max_grad_norm"] > 0:
            torch.nn.utils.clip_grad_norm_([p], cfg["max_grad_norm"])
        opt.step()
        st = opt.state[p]
        out.append({"p": p.detach().numpy().copy(), "m": st["exp_avg"].numpy().copy(), "v": st["exp_avg_sq"].numpy().copy()})
    return out


@pytest.mark.parametrize("kw", [{}, {"norm_factor": 0.5}, {"norm_factor": 2.0}, {"max_grad_norm": 0.0}], ids=str)
def test_adam_reference_is_clip_grad_norm_and_torch_adam(kw):
    inp = R.adam_inputs(1031, **kw)
    want = _torch_adam(inp, F64, 3)
    s = {k: inp[k].astype(np.float64) for k in "pmv"}
    for k in range(3):
        s = R.adam_step(s["p"], s["m"], s["v"], inp["grads"][k], k + 1, inp["cfg"], F64)
        for a in "pmv":
            close64(s[a], want[k][a], f"{a} step {k + 1}")
    # the float32 run is torch's own float32 path to a few ulp of the largest entry
    want32 = _torch_adam(inp, F32, 3)
    s = {k: inp[k] for k in "pmv"}
    for k in range(3):
        s = R.adam_step(s["p"], s["m"], s["v"], inp["grads"][k], k + 1, inp["cfg"], F32)
        for a in "pmv":
            assert s[a].dtype == np.float32
            close64(s[a], want32[k][a], f"{a} step {k + 1} (float32)", 2.0 ** -21)


def test_clip_coef_reference_on_both_sides_of_one():
    g = R.adam_inputs(1031)["grads"][0].astype(np.float64)
    for factor in (0.5, 2.0):
        gg = g * factor * 0.5 / np.sqrt((g * g).sum())
        p = torch.nn.Parameter(torch.zeros(g.size, dtype=F64))
        p.grad = torch.from_numpy(gg.copy())
        torch.nn.utils.clip_grad_norm_([p], 0.5)
        coef = R.clip_coef((gg * gg).sum(), 0.5, F64)
        close64(p.grad.numpy(), gg * coef, f"clipped gradient at {factor} x max_grad_norm")
        assert (coef[0] == 1.0) == (factor < 1)


@pytest.mark.parametrize("tau", R.POLYAK_TAU)
def test_polyak_reference_is_the_in_place_pair(tau):
    inp = R.polyak_inputs(257, tau)
    t = torch.from_numpy(inp["target"]).double()
    t.mul_(1 - tau)
    t.add_(torch.from_numpy(inp["param"]).double(), alpha=tau)
    close64(R.polyak(inp["target"], inp["param"], tau, F64), t.numpy(), "target", 1e-15)
    close64(R.polyak(inp["target"], inp["param"], tau, F64), (1 - tau) * inp["target"].astype(np.float64) + tau * inp["param"].astype(np.float64),
            "target, closed form", 1e-15)
    r32 = R.polyak(inp["target"], inp["param"], tau, F32)
    assert tau != 1.0 or np.array_equal(r32, inp["param"])
    assert tau != 0.0 or np.array_equal(r32, inp["target"])


# ---------------------------------------------------------------------------------------------------------------------------
# teeth: the float32 reference passes every comparator on the GPU cases' inputs, the mutants fail
# ---------------------------------------------------------------------------------------------------------------------------
def _swap_yz(x):
    return np.ascontiguousarray(x[:, [0, 2, 1, 3]])


def _pad_hit(got, key):
    g = {k: v.copy() for k, v in got.items()}
    g[key][-R.PAD] = 0
    return g


@pytest.mark.parametrize("N,lo,hi", R.HEAD_CASES)
def test_teeth_head(N, lo, hi):
    for phase in R.HEAD_PHASES:
        inp = R.head_inputs(N, lo, hi, phase)
        fwd = {"action": R.padded(inp["action"])}
        R.check_head_fwd(fwd, inp)
        bwd = R.got_of(R.head_bwd(inp["d_action"], inp["action"], inp["log_std"], inp["eps"], lo, hi, F32))
        R.check_head_bwd(bwd, inp)
        rejects(R.check_head_fwd, _pad_hit(fwd, "action"), inp)
        rejects(R.check_head_bwd, _pad_hit(bwd, "d_log_std"), inp)
        if N < 63:
            continue
        # clamp bounds ignored in the forward
        rejects(R.check_head_fwd, {"action": R.padded(R.head_fwd(inp["mu"], inp["log_std"], inp["eps"], -np.inf, np.inf, F32))}, inp)
        # the other pair's bounds (arguments not honoured)
        olo, ohi = R.HEAD_BOUNDS[1] if (lo, hi) == R.HEAD_BOUNDS[0] else R.HEAD_BOUNDS[0]
        rejects(R.check_head_fwd, {"action": R.padded(R.head_fwd(inp["mu"], inp["log_std"], inp["eps"], olo, ohi, F32))}, inp)
        rejects(R.check_head_bwd, R.got_of(R.head_bwd(inp["d_action"], inp["action"], inp["log_std"], inp["eps"], olo, ohi, F32)), inp)
        # float4 columns y and z of eps swapped
        rejects(R.check_head_fwd, {"action": R.padded(R.head_fwd(inp["mu"], inp["log_std"], _swap_yz(inp["eps"]), lo, hi, F32))}, inp)
        rejects(R.check_head_bwd, R.got_of(R.head_bwd(inp["d_action"], inp["action"], inp["log_std"], _swap_yz(inp["eps"]), lo, hi, F32)), inp)
        # an open interval in the backward, at either end alone
        r = R.head_bwd(inp["d_action"], inp["action"], inp["log_std"], inp["eps"], lo, hi, F32)
        for edge in (lo, hi):
            m = {k: v.copy() for k, v in r.items()}
            m["d_log_std"][inp["log_std"] == np.float32(edge)] = 0
            rejects(R.check_head_bwd, R.got_of(m), inp)
        # the gradient let through one fp32 step outside
        m = {k: v.copy() for k, v in r.items()}
        wide = R.head_bwd(inp["d_action"], inp["action"], inp["log_std"], inp["eps"], np.nextafter(np.float32(lo), np.float32(-np.inf)),
                          np.nextafter(np.float32(hi), np.float32(np.inf)), F32)
        rejects(R.check_head_bwd, R.got_of(wide), inp)


@pytest.mark.parametrize("N", R.ROWS)
def test_teeth_reparam(N):
    inp = R.reparam_inputs(N)
    fwd = {"action": R.padded(inp["action"])}
    R.check_reparam_fwd(fwd, inp)
    args = (inp["d_action"], inp["action"], inp["log_std"], inp["eps"])
    once = R.reparam_bwd(*args, inp["g_log_std"], F32)
    R.check_reparam_bwd(R.got_of(once), inp)
    twice = R.reparam_bwd(*args, once["g_log_std"], F32)                 # the second call accumulates on the first
    R.check_reparam_bwd(R.got_of(twice), dict(inp, g_log_std=once["g_log_std"]))
    rejects(R.check_reparam_bwd, _pad_hit(R.got_of(once), "d_mean"), inp)
    # g_log_std overwritten instead of accumulated
    rejects(R.check_reparam_bwd, R.got_of(R.reparam_bwd(*args, np.zeros_like(inp["g_log_std"]), F32)), inp)
    # columns y and z swapped: of eps, and of the shared log_std
    rejects(R.check_reparam_fwd, {"action": R.padded(R.reparam_fwd(inp["mean"], inp["log_std"], _swap_yz(inp["eps"]), F32))}, inp)
    rejects(R.check_reparam_fwd, {"action": R.padded(R.reparam_fwd(inp["mean"], inp["log_std"][[0, 2, 1, 3]], inp["eps"], F32))}, inp)
    rejects(R.check_reparam_bwd, R.got_of(R.reparam_bwd(inp["d_action"], inp["action"], inp["log_std"], _swap_yz(inp["eps"]), inp["g_log_std"], F32)), inp)


def _shac_step_np(s, disc, loss, gamma, scale, last_step, epd_without_done=False, ignore_last=False, no_reset=False):
    """one step in numpy float32, with the mutations switched in; unmutated it is the float32 reference bit for bit"""
    g, sc = np.float32(gamma), np.float32(scale)
    dn = s["done"] != 0
    epd = (s["ep_flags"] & 8) != 0
    if not epd_without_done:
        epd = dn & epd
    nv = np.where(s["q0"] <= s["q1"], s["q0"], s["q1"])
    l = loss - s["reward"] * disc
    cut = (dn | (bool(last_step) and not ignore_last)) & ~epd
    l = l - nv * disc * g * cut.astype(np.float32)
    d = disc * g if no_reset else disc * g * (~dn).astype(np.float32) + dn.astype(np.float32)
    return {"disc": d, "loss": l, "d_reward": -disc * sc, "next_value": nv, "ep_done": epd.astype(np.uint8)}


@pytest.mark.parametrize("last_step", [0, 1])
@pytest.mark.parametrize("N", R.ROWS)
def test_teeth_shac_accumulate(N, last_step):
    inp = R.accumulate_inputs(N)
    if N >= 63:
        for lo_, hi_ in ((0, 64), (max(N - 64, 0), N)):                          # the whole truth table in the first and in the last wave
            seen = set(zip(inp["steps"][0]["done"][lo_:hi_].tolist(), inp["steps"][0]["ep_flags"][lo_:hi_].tolist()))
            assert seen == set(R.TRUTH)
    disc, loss = inp["disc"], inp["loss"]
    for k, s in enumerate(inp["steps"]):
        one = dict(s, disc=disc, loss=loss, gamma=inp["gamma"], scale=inp["scale"], last_step=last_step)
        r = R.shac_accumulate(s["reward"], s["done"], s["ep_flags"], s["q0"], s["q1"], disc, loss, inp["gamma"], inp["scale"], last_step, F32)
        R.check_shac_accumulate(R.got_of(r), one)
        R.check_shac_accumulate(R.got_of(_shac_step_np(s, disc, loss, inp["gamma"], inp["scale"], last_step)), one)
        rejects(R.check_shac_accumulate, _pad_hit(R.got_of(r), "ep_done"), one)
        if N >= 63:
            rejects(R.check_shac_accumulate, R.got_of(_shac_step_np(s, disc, loss, inp["gamma"], inp["scale"], last_step, epd_without_done=True)), one)
            rejects(R.check_shac_accumulate, R.got_of(_shac_step_np(s, disc, loss, inp["gamma"], inp["scale"], last_step, no_reset=True)), one)
            if last_step:
                rejects(R.check_shac_accumulate, R.got_of(_shac_step_np(s, disc, loss, inp["gamma"], inp["scale"], last_step, ignore_last=True)), one)
            # done read as a 0 / 1 byte (== 1) instead of != 0
            rejects(R.check_shac_accumulate, R.got_of(_shac_step_np(dict(s, done=(s["done"] == 1).astype(np.uint8)), disc, loss, inp["gamma"],
                                                                    inp["scale"], last_step)), one)
        disc, loss = r["disc"], r["loss"]


@pytest.mark.parametrize("N", R.ROWS)
def test_teeth_bptt_accumulate(N):
    inp = R.accumulate_inputs(N)
    disc, loss = inp["disc"], inp["loss"]
    for s in inp["steps"]:
        one = dict(reward=s["reward"], done=s["done"], disc=disc, loss=loss, gamma=inp["gamma"], scale=inp["scale"])
        r = R.bptt_accumulate(s["reward"], s["done"], disc, loss, inp["gamma"], inp["scale"], F32)
        R.check_bptt_accumulate(R.got_of(r), one)
        rejects(R.check_bptt_accumulate, _pad_hit(R.got_of(r), "loss"), one)
        if N >= 63:
            rejects(R.check_bptt_accumulate, R.got_of(dict(r, disc=disc * np.float32(inp["gamma"]))), one)          # no reset on done
            rejects(R.check_bptt_accumulate, R.got_of(R.bptt_accumulate(s["reward"], (s["done"] == 1).astype(np.uint8), disc, loss,
                                                                         inp["gamma"], inp["scale"], F32)), one)
            rejects(R.check_bptt_accumulate, R.got_of(dict(r, d_reward=-r["disc"] * np.float32(inp["scale"]))), one)  # the NEW discount
        disc, loss = r["disc"], r["loss"]


@pytest.mark.parametrize("H,N", R.HORIZON_CASES)
def test_teeth_shac_accumulate_horizon(H, N):
    inp = R.horizon_inputs(H, N)
    r = R.shac_accumulate_horizon(inp["reward"], inp["done"], inp["ep_flags"], inp["q0"], inp["q1"], inp["disc"], inp["loss"], inp["gamma"],
                                  inp["scale"], F32)
    R.check_shac_accumulate_horizon(R.got_of(r), inp)
    rejects(R.check_shac_accumulate_horizon, _pad_hit(R.got_of(r), "next_value"), inp)

    def run(**mut):
        d, l, rows = inp["disc"], inp["loss"], {"d_reward": [], "next_value": [], "ep_done": []}
        for t in range(H):
            o = _shac_step_np({k: inp[k][t] for k in ("reward", "done", "ep_flags", "q0", "q1")}, d, l, inp["gamma"], inp["scale"], t == H - 1, **mut)
            d, l = o["disc"], o["loss"]
            for k in rows:
                rows[k].append(o[k])
        return R.got_of({"disc": d, "loss": l, **{k: np.stack(v) for k, v in rows.items()}})

    R.check_shac_accumulate_horizon(run(), inp)
    if N >= 63:
        for mut in ("epd_without_done", "ignore_last", "no_reset"):
            rejects(R.check_shac_accumulate_horizon, run(**{mut: True}), inp)


@pytest.mark.parametrize("M,M_global", R.TWIN_CASES)
def test_teeth_twin_q_loss(M, M_global):
    inp = R.twin_q_inputs(M, M_global)
    r = R.twin_q_loss(inp["q0"], inp["q1"], inp["target"], M_global, F32)
    R.check_twin_q_loss(R.got_of(r), inp)
    rejects(R.check_twin_q_loss, _pad_hit(R.got_of(r), "dq1"), inp)
    # ties sent to q1: the same function with the heads exchanged
    x = R.twin_q_loss(inp["q1"], inp["q0"], inp["target"], M_global, F32)
    rejects(R.check_twin_q_loss, R.got_of({"loss": x["loss"], "dq0": x["dq1"], "dq1": x["dq0"]}), inp)
    if M_global != M:                                                    # 1 / M where 1 / M_global belongs, in the gradient or in the loss
        w = R.twin_q_loss(inp["q0"], inp["q1"], inp["target"], M, F32)
        rejects(R.check_twin_q_loss, R.got_of(dict(r, dq0=w["dq0"], dq1=w["dq1"])), inp)
        rejects(R.check_twin_q_loss, R.got_of(dict(r, loss=w["loss"])), inp)
    if M > 256:                                                          # the fold drops the last block's partial
        last = slice((M - 1) // 256 * 256, M)
        short = (np.float64(r["loss"][0]) - ((np.minimum(inp["q0"], inp["q1"])[last].astype(np.float64) - inp["target"][last]) ** 2).sum() / M_global)
        rejects(R.check_twin_q_loss, R.got_of(dict(r, loss=np.array([short], dtype=np.float32))), inp)


@pytest.mark.parametrize("n,tau", R.POLYAK_CASES)
def test_teeth_polyak(n, tau):
    inp = R.polyak_inputs(n, tau)
    r = R.polyak(inp["target"], inp["param"], tau, F32)
    R.check_polyak({"target": R.padded(r)}, inp)
    rejects(R.check_polyak, _pad_hit({"target": R.padded(r)}, "target"), inp)
    if tau != 0.0:                                                       # the last element skipped
        m = r.copy()
        m[-1] = inp["target"][-1]
        rejects(R.check_polyak, {"target": R.padded(m)}, inp)
    if tau == 1.0 and n > 1:                                             # bit for bit, not merely close
        m = r.copy()
        m[n // 2] = np.nextafter(m[n // 2], np.float32(np.inf))
        rejects(R.check_polyak, {"target": R.padded(m)}, inp)


@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_teeth_sumsq(n):
    inp = R.sumsq_inputs(n)
    assert 1e-3 <= np.abs(inp["x"]).min() and np.abs(inp["x"]).max() <= 1e3
    R.check_sumsq({"sumsq": R.padded(R.sumsq(inp["x"], F32))}, inp)
    if n > 1:
        for skipped in (inp["x"][:-1], inp["x"][1:], np.delete(inp["x"], n - 1 - (n % 4 or 4))):       # last, first, last of the float4 part
            rejects(R.check_sumsq, {"sumsq": R.padded(R.sumsq(skipped, F32))}, inp)
    rejects(R.check_sumsq, {"sumsq": R.padded(np.zeros(1, np.float32))}, inp)


def _adam_step_mut(p, m, v, grad, step, cfg, uncapped=False, wd_after=False):
    """the float32 reference's step with the mutations switched in; unmutated it equals it bit for bit"""
    p, m, v, g = (torch.from_numpy(np.ascontiguousarray(x)) for x in (p, m, v, grad))
    if cfg["max_grad_norm"] > 0:
        coef = cfg["max_grad_norm"] / (torch.sqrt((g * g).sum()) + 1e-6)
        g = g * (coef if uncapped else torch.clamp(coef, max=1.0))
    if not wd_after:
        g = g + cfg["weight_decay"] * p
    m = m + (g - m) * (1.0 - cfg["beta1"])
    v = v * cfg["beta2"] + (1.0 - cfg["beta2"]) * g * g
    bc1, bc2 = 1.0 - cfg["beta1"] ** step, 1.0 - cfg["beta2"] ** step
    upd = m + cfg["weight_decay"] * p if wd_after else m
    p = p - (cfg["lr"] / bc1) * (upd / (torch.sqrt(v) / (bc2 ** 0.5) + cfg["eps"]))
    return {"p": p.numpy(), "m": m.numpy(), "v": v.numpy()}


def _adam_run(inp, **mut):
    s, got = {k: inp[k] for k in "pmv"}, []
    for k, grad in enumerate(inp["grads"]):
        s = _adam_step_mut(s["p"], s["m"], s["v"], grad, 1 + k, inp["cfg"], **mut)
        got.append(R.got_of(s))
    return got


@pytest.mark.parametrize("name", list(R.ADAM_CASES))
def test_teeth_adam(name):
    inp, extra = R.adam_case(name)
    n = inp["p"].size
    got = R.adam_ref32_got(inp)
    R.check_adam(got, inp)
    plain = _adam_run(inp)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(got, plain) for k in "pmv")
    # the last element skipped
    m = [{k: v.copy() for k, v in g.items()} for g in got]
    for g in m:
        for k in "pmv":
            g[k][n - 1] = inp[k][n - 1]
    rejects(R.check_adam, m, inp)
    # weight decay after the moment update instead of before
    rejects(R.check_adam, _adam_run(inp, wd_after=True) if "pack_map" not in inp else
            [dict(a, packed=b["packed"]) for a, b in zip(_adam_run(inp, wd_after=True), got)], inp)
    if name == "norm_half":                                              # clip coefficient not capped at 1
        rejects(R.check_adam, _adam_run(inp, uncapped=True), inp)
    if name in ("norm_double", "n43977"):                                # no clipping at all
        rejects(R.check_adam, R.adam_ref32_got(dict(inp, cfg=dict(inp["cfg"], max_grad_norm=0.0))), inp)
    if "pack_map" in inp:
        pm = inp["pack_map"]
        assert n == R.ADAM_TAIL_N and (pm[:262144] >= 0).any() and (pm[262144:] >= 0).any()
        per = (pm >= 0).sum(1)
        assert set(per[:512].tolist()) == set(per[262144:].tolist()) == {0, 1, 2, 3, 4}
        used = pm[pm >= 0]
        assert used.size == np.unique(used).size < inp["packed_size"]
        # packed slots not refreshed for indices >= 262 144 (the tail loop)
        m = [{k: v.copy() for k, v in g.items()} for g in got]
        for g in m:
            g["packed"][pm[262144:][pm[262144:] >= 0]] = R.SENT_F
        rejects(R.check_adam, m, inp)
        # ... and a slot written that no parameter maps to
        m = [{k: v.copy() for k, v in g.items()} for g in got]
        free = np.setdiff1d(np.arange(inp["packed_size"]), used)[0]
        m[0]["packed"][free] = 0
        rejects(R.check_adam, m, inp)
    if "tail" in extra:                                                  # the tail of the norm forgotten: the parameters the fold does not cover
        g = [x.copy() for x in inp["grads"]]
        for x in g:
            x[n - extra["tail"]:] = 0
        short = dict(inp, grads=g)
        s, bad = {k: inp[k] for k in "pmv"}, []
        for k in range(len(g)):
            coef = R.clip_coef(R.sumsq(g[k], F32), inp["cfg"]["max_grad_norm"], F32)[0]
            s = R.adam_step(s["p"], s["m"], s["v"], inp["grads"][k] * coef, 1 + k, dict(inp["cfg"], max_grad_norm=0.0), F32)
            bad.append(R.got_of(s))
        assert short is not inp
        rejects(R.check_adam, bad, inp)


@pytest.mark.parametrize("factor", [0.5, 3.0])
def test_teeth_clip_coef(factor):
    ss = np.float32((factor * 0.5) ** 2)
    inp = dict(sumsq=ss, max_grad_norm=0.5)
    r = R.clip_coef(ss, 0.5, F32)
    R.check_clip_coef({"coef": R.padded(r)}, inp)
    assert (r[0] == 1.0) == (factor < 1)
    uncapped = np.array([np.float32(0.5) / (np.sqrt(ss) + np.float32(1e-6))], dtype=np.float32)
    if factor < 1:                                                       # not capped at 1
        rejects(R.check_clip_coef, {"coef": R.padded(uncapped)}, inp)
    else:                                                                # the norm's square taken for the norm
        rejects(R.check_clip_coef, {"coef": R.padded(np.minimum(np.float32(0.5) / (ss + np.float32(1e-6)), np.float32(1)).reshape(1))}, inp)
