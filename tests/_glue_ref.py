"""Plain references and comparators for the glue kernels of the first-order trainers (vf_shac.hip, vf_bptt_ops.hip, vf_optim.hip).

No GPU and no ``visfly_amd`` import: numpy / torch-CPU only, written from the reference's formulas, not from the kernels.
Every reference takes ``dtype``: ``torch.float64`` is the truth, ``torch.float32`` is the reference's own arithmetic.  Arrays go
in and out as numpy; scalars that reach a kernel as ``float`` (gamma, scale, the clamp bounds, Adam's hyper-parameters) are
first rounded to fp32 (``f32``), so that truth and kernel work on the same inputs.

Comparators (``check_<op>(got, inputs)``), shared by the host tests and the GPU tests:
  * fp32 add / multiply / compare / select only (the accumulate kernels; zeros and head selection of the twin-Q gradient):
    bit identity with the float32 reference, exact ``==`` for zeros, ``ep_done``, ``next_value``, the selected head;
  * everything else (expf / tanhf, division, sqrtf, fmaf, fp64 sums cast to fp32):
        bound = max(4 * max|ref32 - ref64|, 2^-22 * max|ref64|)   per output array, from the references alone.
    4: ROCm's device expf / tanhf are specified to a few ulp, torch's CPU routines to one.  Not tuned.
  * every output buffer is PAD elements longer than needed and pre-filled with a sentinel; the pad must come back untouched.
Each comparator returns ``{array: (err, e32, bound)}`` with err = max|got - ref64| and e32 = max|ref32 - ref64|.
"""
import numpy as np
import torch

PAD = 64
SENT_F = np.float32(-12345.678)          # float buffers
SENT_B = np.uint8(0xA5)                  # byte buffers
EP_EPISODE_DONE = 8                      # VF_EP_EPISODE_DONE (include/visfly_amd.h)
F32, F64 = torch.float32, torch.float64


def f32(x):
    """the value a C ``float`` argument carries"""
    return float(np.float32(x))


def padded(a):
    """flat copy of ``a`` followed by PAD sentinel elements"""
    a = np.ascontiguousarray(a)
    sent = SENT_B if a.dtype == np.uint8 else SENT_F
    return np.concatenate([a.reshape(-1), np.full(PAD, sent, dtype=a.dtype)])


def blank(shape, dtype=np.float32):
    """an output buffer nobody wrote yet: sentinel everywhere, pad included"""
    sent = SENT_B if np.dtype(dtype) == np.uint8 else SENT_F
    return np.full(int(np.prod(shape)) + PAD, sent, dtype=dtype)


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def _np(t):
    return t.detach().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def head_fwd(mu, log_std, eps, lo, hi, dtype):
    """td_policies.py:230-244 + the squashed Gaussian's rsample: tanh(mu + eps * exp(clamp(log_std, lo, hi))), rows (N, 4)"""
    mu, log_std, eps = _t(mu, dtype), _t(log_std, dtype), _t(eps, dtype)
    return _np(torch.tanh(mu + eps * torch.exp(torch.clamp(log_std, f32(lo), f32(hi)))))


def head_bwd(d_action, action, log_std, eps, lo, hi, dtype):
    """reverse of head_fwd from the SAVED action: d_mu = d_action (1 - action^2); d_log_std = d_mu eps exp(log_std) on the
    closed interval [lo, hi] (th.clamp passes the gradient there, td_policies.py:244), else 0"""
    da, a, ls, e = _t(d_action, dtype), _t(action, dtype), _t(log_std, dtype), _t(eps, dtype)
    d_mu = da * (1.0 - a * a)
    inside = (ls >= f32(lo)) & (ls <= f32(hi))
    d_ls = torch.where(inside, d_mu * e * torch.exp(ls), torch.zeros_like(d_mu))
    return {"d_mu": _np(d_mu), "d_log_std": _np(d_ls)}


def reparam_fwd(mean, log_std, eps, dtype):
    """BPTT.py:107-116 with a state-independent log_std (4,): tanh(mean + exp(log_std) * eps)"""
    return _np(torch.tanh(_t(mean, dtype) + torch.exp(_t(log_std, dtype)) * _t(eps, dtype)))


def reparam_bwd(d_action, action, log_std, eps, g_log_std, dtype):
    """d_mean = d_action (1 - action^2);  g_log_std += d_mean exp(log_std) eps   (per row)"""
    da, a, e = _t(d_action, dtype), _t(action, dtype), _t(eps, dtype)
    d_mean = da * (1.0 - a * a)
    g = _t(g_log_std, dtype) + d_mean * torch.exp(_t(log_std, dtype)) * e
    return {"d_mean": _np(d_mean), "g_log_std": _np(g)}


def bptt_accumulate(reward, done, disc, loss, gamma, scale, dtype):
    """BPTT.py:123-124, per agent; d_reward = d(mean loss) / d reward_t = -disc * scale with scale = 1 / agents"""
    r, d, l = _t(reward, dtype), _t(disc, dtype), _t(loss, dtype)
    dn = torch.from_numpy(np.asarray(done)) != 0
    l = l + -1 * r * d
    d_reward = -d * f32(scale)
    d = d * f32(gamma) * ~dn + dn
    return {"disc": _np(d), "loss": _np(l), "d_reward": _np(d_reward)}


def shac_accumulate(reward, done, ep_flags, q0, q1, disc, loss, gamma, scale, last_step, dtype):
    """shac.py:238-254 for one horizon step, per agent, and the buffer rows of the step (next_value, episode_done)"""
    r, d, l = _t(reward, dtype), _t(disc, dtype), _t(loss, dtype)
    dn = torch.from_numpy(np.asarray(done)) != 0
    epd = dn & ((torch.from_numpy(np.asarray(ep_flags)) & EP_EPISODE_DONE) != 0)       # info["episode_done"] exists where done
    nv = torch.cat([_t(q0, dtype).view(-1, 1), _t(q1, dtype).view(-1, 1)], dim=1).min(dim=1).values
    l = l - r * d
    cut = (dn | bool(last_step)) & ~epd
    if cut.any():
        l = l - nv * d * f32(gamma) * cut
    d_reward = -d * f32(scale)
    d = d * f32(gamma) * ~dn + dn
    return {"disc": _np(d), "loss": _np(l), "d_reward": _np(d_reward), "next_value": _np(nv),
            "ep_done": _np(epd.to(torch.uint8))}


def shac_accumulate_horizon(reward, done, ep_flags, q0, q1, disc, loss, gamma, scale, dtype):
    """H steps of shac_accumulate in order, rows (H, N); the last one is the horizon's last step (shac.py:243)"""
    H = reward.shape[0]
    out = {"d_reward": [], "next_value": [], "ep_done": []}
    for t in range(H):
        o = shac_accumulate(reward[t], done[t], ep_flags[t], q0[t], q1[t], disc, loss, gamma, scale, t == H - 1, dtype)
        disc, loss = o["disc"], o["loss"]
        for k in out:
            out[k].append(o[k])
    return {"disc": disc, "loss": loss, **{k: np.stack(v) for k, v in out.items()}}


def twin_q_loss(q0, q1, target, M_global, dtype):
    """shac.py:269-271 on this rank's M rows of M_global: mse_loss(target, min(Q1, Q2)) * M / M_global and its gradient
    w.r.t. both heads; th.cat(...).min(dim=1) sends a tie to the first head"""
    a, b, tg = _t(q0, dtype), _t(q1, dtype), _t(target, dtype)
    M = a.numel()
    first = a <= b
    v = torch.where(first, a, b)
    loss = torch.nn.functional.mse_loss(tg, v) * M / M_global
    g = 2.0 * (v - tg) / M_global
    z = torch.zeros_like(g)
    return {"loss": _np(loss.reshape(1)), "dq0": _np(torch.where(first, g, z)), "dq1": _np(torch.where(first, z, g)),
            "first": _np(first)}


def polyak(target, param, tau, dtype):
    """SB3 polyak_update as shac.py:277 calls it: target.mul_(1 - tau); target.add_(param, alpha=tau)"""
    t = _t(target, dtype).clone()
    t.mul_(1.0 - tau)
    t.add_(_t(param, dtype), alpha=tau)
    return _np(t)


def sumsq(x, dtype):
    x = _t(x, dtype)
    return _np((x * x).sum().reshape(1))


def clip_coef(ss, max_norm, dtype):
    """th.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6), capped at 1"""
    total = torch.sqrt(torch.as_tensor(ss, dtype=dtype).reshape(()))
    return _np(torch.clamp(f32(max_norm) / (total + 1e-6), max=1.0).reshape(1))


def adam_cfg(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, max_grad_norm=0.5):
    """hyper-parameters as the fp32 fields of vf_adam_cfg carry them"""
    return dict(lr=f32(lr), beta1=f32(beta1), beta2=f32(beta2), eps=f32(eps), weight_decay=f32(weight_decay),
                max_grad_norm=f32(max_grad_norm))


def adam_step(p, m, v, grad, step, cfg, dtype):
    """clip_grad_norm_(max_grad_norm) (skipped when <= 0) then torch.optim.Adam.step with L2 weight decay (PPO.py:285-292):
    (p, m, v) of step - 1 -> those of `step` (1-based); the caller keeps m and v across calls"""
    p, m, v, g = _t(p, dtype), _t(m, dtype), _t(v, dtype), _t(grad, dtype)
    if cfg["max_grad_norm"] > 0:
        total = torch.sqrt((g * g).sum())
        g = g * torch.clamp(cfg["max_grad_norm"] / (total + 1e-6), max=1.0)
    g = g + cfg["weight_decay"] * p
    m = m + (g - m) * (1.0 - cfg["beta1"])
    v = v * cfg["beta2"] + (1.0 - cfg["beta2"]) * g * g
    bc1, bc2 = 1.0 - cfg["beta1"] ** step, 1.0 - cfg["beta2"] ** step
    denom = torch.sqrt(v) / (bc2 ** 0.5) + cfg["eps"]
    p = p - (cfg["lr"] / bc1) * (m / denom)
    return {"p": _np(p), "m": _np(m), "v": _np(v)}


# ---------------------------------------------------------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------------------------------------------------------
def body(name, arr, shape):
    """the first prod(shape) elements of a padded buffer; the PAD behind them must still hold the sentinel"""
    arr = np.asarray(arr)
    n = int(np.prod(shape))
    assert arr.ndim == 1 and arr.size == n + PAD, f"{name}: buffer of {arr.size} elements, expected {n} + {PAD} pad"
    sent = SENT_B if arr.dtype == np.uint8 else SENT_F
    bad = np.flatnonzero(arr[n:].view(np.uint8) != np.full(PAD, sent, dtype=arr.dtype).view(np.uint8))
    assert bad.size == 0, f"{name}: pad behind element {n} was written (first at pad byte {bad[:1]})"
    return arr[:n].reshape(shape)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def exact(name, got, ref32):
    """bit identity with the float32 reference"""
    got, ref32 = np.asarray(got), np.asarray(ref32)
    assert got.dtype == ref32.dtype and got.shape == ref32.shape, (name, got.dtype, ref32.dtype, got.shape, ref32.shape)
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(ref32).reshape(-1))
    assert bad.size == 0, (f"{name}: {bad.size} of {got.size} elements differ from the float32 reference, first at {bad[0]}: "
                           f"got {got.reshape(-1)[bad[0]]!r}, want {ref32.reshape(-1)[bad[0]]!r}")
    return (0.0, 0.0, 0.0)


def within(name, got, ref32, ref64):
    """max|got - ref64| <= max(4 max|ref32 - ref64|, 2^-22 max|ref64|): the bound comes from the references alone"""
    got, ref32, ref64 = np.asarray(got), np.asarray(ref32), np.asarray(ref64)
    assert got.shape == ref64.shape == ref32.shape, (name, got.shape, ref32.shape, ref64.shape)
    assert got.dtype == np.float32 and ref32.dtype == np.float32 and ref64.dtype == np.float64, name
    assert np.isfinite(ref64).all() and np.isfinite(got).all(), f"{name}: non-finite value"
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    bound = max(4.0 * e32, 2.0 ** -22 * float(np.abs(ref64).max()))
    d = np.abs(got.astype(np.float64) - ref64)
    err = float(d.max())
    assert err <= bound, (f"{name}: max|got - ref64| = {err:.3e} at {int(d.argmax())} > bound {bound:.3e} "
                          f"(max|ref32 - ref64| = {e32:.3e})")
    return (err, e32, bound)


def check_head_fwd(got, inp):
    args = (inp["mu"], inp["log_std"], inp["eps"], inp["lo"], inp["hi"])
    return {"action": within("action", body("action", got["action"], inp["mu"].shape), head_fwd(*args, F32), head_fwd(*args, F64))}


def check_head_bwd(got, inp):
    args = (inp["d_action"], inp["action"], inp["log_std"], inp["eps"], inp["lo"], inp["hi"])
    r32, r64 = head_bwd(*args, F32), head_bwd(*args, F64)
    shape = inp["action"].shape
    out = {k: within(k, body(k, got[k], shape), r32[k], r64[k]) for k in ("d_mu", "d_log_std")}
    g = body("d_log_std", got["d_log_std"], shape)
    ls = inp["log_std"]
    outside = (ls < np.float32(inp["lo"])) | (ls > np.float32(inp["hi"]))
    assert not np.any(_bits(g[outside])), "d_log_std: not +0 outside [lo, hi]"
    # on the closed interval the gradient passes: a product of three factors far from the underflow range is not zero
    live = ~outside & (np.abs(r32["d_log_std"]) > 1e-30)
    assert np.all(g[live] != 0), "d_log_std: zero inside the closed interval [lo, hi] where the reference passes the gradient"
    return out


def check_reparam_fwd(got, inp):
    args = (inp["mean"], inp["log_std"], inp["eps"])
    return {"action": within("action", body("action", got["action"], inp["mean"].shape), reparam_fwd(*args, F32), reparam_fwd(*args, F64))}


def check_reparam_bwd(got, inp):
    """inp["g_log_std"]: the accumulator BEFORE the call"""
    args = (inp["d_action"], inp["action"], inp["log_std"], inp["eps"], inp["g_log_std"])
    r32, r64 = reparam_bwd(*args, F32), reparam_bwd(*args, F64)
    return {k: within(k, body(k, got[k], inp["action"].shape), r32[k], r64[k]) for k in ("d_mean", "g_log_std")}


def check_bptt_accumulate(got, inp):
    r32 = bptt_accumulate(inp["reward"], inp["done"], inp["disc"], inp["loss"], inp["gamma"], inp["scale"], F32)
    return {k: exact(k, body(k, got[k], inp["reward"].shape), r32[k]) for k in ("disc", "loss", "d_reward")}


def check_shac_accumulate(got, inp):
    r32 = shac_accumulate(inp["reward"], inp["done"], inp["ep_flags"], inp["q0"], inp["q1"], inp["disc"], inp["loss"], inp["gamma"],
                          inp["scale"], inp["last_step"], F32)
    return {k: exact(k, body(k, got[k], inp["reward"].shape), r32[k]) for k in ("disc", "loss", "d_reward", "next_value", "ep_done")}


def check_shac_accumulate_horizon(got, inp):
    r32 = shac_accumulate_horizon(inp["reward"], inp["done"], inp["ep_flags"], inp["q0"], inp["q1"], inp["disc"], inp["loss"],
                                  inp["gamma"], inp["scale"], F32)
    N = inp["reward"].shape[1:]
    out = {k: exact(k, body(k, got[k], N), r32[k]) for k in ("disc", "loss")}
    out.update({k: exact(k, body(k, got[k], inp["reward"].shape), r32[k]) for k in ("d_reward", "next_value", "ep_done")})
    return out


def check_twin_q_loss(got, inp):
    args = (inp["q0"], inp["q1"], inp["target"], inp["M_global"])
    r32, r64 = twin_q_loss(*args, F32), twin_q_loss(*args, F64)
    shape = inp["q0"].shape
    dq0, dq1 = body("dq0", got["dq0"], shape), body("dq1", got["dq1"], shape)
    first = r32["first"]
    assert np.array_equal(first, r64["first"])
    assert not np.any(_bits(dq1[first])), "dq1: not +0 where q0 <= q1 (a tie goes to q0)"
    assert not np.any(_bits(dq0[~first])), "dq0: not +0 where q1 < q0"
    assert np.all(dq0[first & (r32["dq0"] != 0)] != 0) and np.all(dq1[~first & (r32["dq1"] != 0)] != 0), "gradient missing on the selected head"
    return {"loss": within("loss", body("loss", got["loss"], (1,)), r32["loss"], r64["loss"]),
            "dq0": within("dq0", dq0, r32["dq0"], r64["dq0"]), "dq1": within("dq1", dq1, r32["dq1"], r64["dq1"])}


def check_polyak(got, inp):
    args = (inp["target"], inp["param"], inp["tau"])
    t = body("target", got["target"], inp["target"].shape)
    if inp["tau"] == 1.0:
        exact("target (tau = 1: the parameters)", t, inp["param"])
    if inp["tau"] == 0.0:
        exact("target (tau = 0: unchanged)", t, inp["target"])
    return {"target": within("target", t, polyak(*args, F32), polyak(*args, F64))}


def check_sumsq(got, inp):
    return {"sumsq": within("sumsq", body("sumsq", got["sumsq"], (1,)), sumsq(inp["x"], F32), sumsq(inp["x"], F64))}


def check_clip_coef(got, inp):
    args = (inp["sumsq"], inp["max_grad_norm"])
    return {"coef": within("coef", body("coef", got["coef"], (1,)), clip_coef(*args, F32), clip_coef(*args, F64))}


def check_adam(got, inp):
    """got: one {"p", "m", "v"[, "packed"]} of padded buffers per step, in order; inp: p, m, v before the first step, grads (one
    per step), cfg, first_step, and optionally pack_map (n, 4) int32 with -1 = none, packed_size.  Each side keeps its own m and v."""
    n = inp["p"].shape
    s32 = {k: inp[k] for k in "pmv"}
    s64 = {k: inp[k].astype(np.float64) for k in "pmv"}
    out = {}
    assert len(got) == len(inp["grads"])
    for k, (g, grad) in enumerate(zip(got, inp["grads"])):
        step = inp.get("first_step", 1) + k
        s32 = adam_step(s32["p"], s32["m"], s32["v"], grad, step, inp["cfg"], F32)
        s64 = adam_step(s64["p"], s64["m"], s64["v"], grad, step, inp["cfg"], F64)
        for a in "pmv":
            r = within(f"{a} (step {step})", body(a, g[a], n), s32[a], s64[a])
            out[a] = max(out.get(a, r), r, key=lambda x: x[0] / x[2] if x[2] else 0.0)
        if inp.get("pack_map") is not None:
            pm = inp["pack_map"]
            packed = body("packed", g["packed"], (inp["packed_size"],))
            pnew = body("p", g["p"], n)
            want = np.full(inp["packed_size"], SENT_F, dtype=np.float32)
            rows, cols = np.nonzero(pm >= 0)
            want[pm[rows, cols]] = pnew[rows]
            exact(f"packed (step {step})", packed, want)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# inputs of the GPU cases (the host tests run the comparators over the same inputs)
# ---------------------------------------------------------------------------------------------------------------------------
ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)                  # around the wave (64) and block (256) edges
HEAD_BOUNDS = ((-10.0, 2.0), (-5.0, 0.5))                    # the reference's LOG_STD_MIN / MAX, and a pair that proves the arguments count
DONE_BYTES = (0, 1, 255)
EP_FLAGS = (0, 1, 2, 4, 8, 2 | 8, 4 | 8)
TRUTH = [(d, f) for d in DONE_BYTES for f in EP_FLAGS]       # 21 rows: any 21 consecutive agents hold every combination
TWIN_M = (1, 255, 256, 257, 16385)                           # 16 385 rows leave 65 block partials: the fold's second lane pass
POLYAK_N = (1, 255, 257, 70001)
POLYAK_TAU = (0.005, 1.0, 0.0)
SUMSQ_N = (1, 3, 4, 5, 1023, 1025, 4097, 1 << 20, (1 << 20) + 1, (1 << 20) + 4099)
ADAM_TAIL_N = 262144 + 257                                   # k_adam's grid is capped at 1024 blocks of 256: the rest is the tail loop


def _rng(*key):
    return np.random.default_rng([20260, *[int(k) for k in key]])


def _rows4(rng, N, scale=1.0):
    return (rng.standard_normal((N, 4)) * scale).astype(np.float32)


def head_log_std_specials(lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    ninf, pinf = np.float32(-np.inf), np.float32(np.inf)
    mid = np.float32(0.5) * (lo + hi)
    return np.array([lo, hi, np.nextafter(lo, ninf), np.nextafter(hi, pinf), -50.0, 50.0, mid, np.nextafter(lo, pinf)], dtype=np.float32)


def head_inputs(N, lo, hi, phase):
    """log_std[r, c] = special[(r + c + phase) % 8]: every special value in every column from 8 rows on, and the last row holds
    four of them; phase and phase + 4 together put all eight there.  |mu| up to 20 (saturated actions), distinct columns."""
    rng = _rng(1, N, phase, int(-lo * 10))
    sp = head_log_std_specials(lo, hi)
    r, c = np.meshgrid(np.arange(N), np.arange(4), indexing="ij")
    log_std = sp[(r + c + phase) % 8]
    mu = _rows4(rng, N) * np.array([0.3, 2.0, 20.0], dtype=np.float32)[(r + 2 * c) % 3]
    mu = np.clip(mu, -20, 20).astype(np.float32)
    if N > 8:
        mu[N // 2] = [20.0, -20.0, 19.5, -19.5]
    eps = _rows4(rng, N)
    inp = dict(mu=mu, log_std=log_std, eps=eps, lo=lo, hi=hi)
    inp["action"] = head_fwd(mu, log_std, eps, lo, hi, F32)      # the saved fp32 action the backward reads
    inp["d_action"] = _rows4(rng, N)
    return inp


def reparam_inputs(N):
    rng = _rng(2, N)
    log_std = np.array([0.25, -0.5, -1.75, -3.0], dtype=np.float32)
    mean, eps = _rows4(rng, N, 1.5), _rows4(rng, N)
    inp = dict(mean=mean, log_std=log_std, eps=eps, d_action=_rows4(rng, N), g_log_std=_rows4(rng, N, 0.1) + np.float32(0.5))
    inp["action"] = reparam_fwd(mean, log_std, eps, F32)
    return inp


def _table(shape, shift):
    idx = (np.arange(int(np.prod(shape))).reshape(shape) + shift) % len(TRUTH)
    t = np.array(TRUTH, dtype=np.uint8)
    return t[idx, 0].copy(), t[idx, 1].copy()


def accumulate_inputs(N, calls=3):
    """state (disc, loss) and `calls` steps of (reward, done, ep_flags, q0, q1); step k shifts the truth table by 5 k.  Every 5th
    agent has q0 == q1."""
    rng = _rng(3, N)
    steps = []
    for k in range(calls):
        done, flags = _table((N,), 5 * k)
        q0 = rng.standard_normal(N).astype(np.float32) * 3
        q1 = rng.standard_normal(N).astype(np.float32) * 3
        q1[k::5] = q0[k::5]
        steps.append(dict(reward=rng.standard_normal(N).astype(np.float32), done=done, ep_flags=flags, q0=q0, q1=q1))
    return dict(disc=rng.uniform(0.3, 1.0, N).astype(np.float32), loss=rng.standard_normal(N).astype(np.float32) * 2,
                gamma=0.99, scale=1.0 / N, steps=steps)


def horizon_inputs(H, N):
    rng = _rng(4, H, N)
    t, i = np.meshgrid(np.arange(H), np.arange(N), indexing="ij")
    idx = (5 * t + i) % len(TRUTH)
    tab = np.array(TRUTH, dtype=np.uint8)
    q0 = rng.standard_normal((H, N)).astype(np.float32) * 3
    q1 = rng.standard_normal((H, N)).astype(np.float32) * 3
    q1[:, ::5] = q0[:, ::5]
    return dict(reward=rng.standard_normal((H, N)).astype(np.float32), done=tab[idx, 0].copy(), ep_flags=tab[idx, 1].copy(), q0=q0, q1=q1,
                disc=rng.uniform(0.3, 1.0, N).astype(np.float32), loss=rng.standard_normal(N).astype(np.float32) * 2,
                gamma=0.99, scale=1.0 / N)


def twin_q_inputs(M, M_global):
    rng = _rng(5, M)
    q0 = rng.standard_normal(M).astype(np.float32) * 2
    q1 = (q0 + rng.standard_normal(M).astype(np.float32) * 0.5).astype(np.float32)
    q1[::7] = q0[::7]                                                    # every 7th row an exact tie
    return dict(q0=q0, q1=q1, target=rng.standard_normal(M).astype(np.float32) * 2 + np.float32(0.5), M_global=int(M_global))


def polyak_inputs(n, tau):
    rng = _rng(6, n)
    return dict(target=rng.standard_normal(n).astype(np.float32), param=rng.standard_normal(n).astype(np.float32), tau=float(tau))


def sumsq_inputs(n):
    """magnitudes 1e-3 .. 1e3, log-uniform; the first element and the last five are large, so that a loop which skips one of
    them misses more than the bound"""
    rng = _rng(7, n)
    x = (10.0 ** rng.uniform(-3, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    edge = np.array([937.0, -811.0, 659.0, -983.0, 773.0, -887.0], dtype=np.float32)
    if n < 6:
        x[:] = edge[:n]
    else:
        x[0], x[-5:] = edge[0], edge[1:]
    return dict(x=x)


def adam_inputs(n, steps=3, norm_factor=None, **cfg):
    """parameters O(1), gradients O(1) (far over max_grad_norm = 0.5: clipped) unless norm_factor asks for a total norm of
    norm_factor * max_grad_norm exactly-ish; m and v start from zero as a fresh optimiser's"""
    rng = _rng(8, n)
    c = adam_cfg(**cfg)
    grads = []
    for _ in range(steps):
        g = rng.standard_normal(n)
        if norm_factor is not None:
            g *= norm_factor * c["max_grad_norm"] / np.sqrt((g * g).sum())
        grads.append(g.astype(np.float32))
    return dict(p=rng.standard_normal(n).astype(np.float32), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32), grads=grads, cfg=c,
                first_step=1)


def adam_pack_map(n, packed_size):
    """parameter i -> (i % 5) distinct slots of `packed` (0 .. 4 of them, -1 = none), no slot used twice; slots go to the first
    512 parameters (first pass) and to the last 512 (for n = ADAM_TAIL_N all in the tail loop)"""
    pm = np.full((n, 4), -1, dtype=np.int32)
    who = np.unique(np.concatenate([np.arange(min(512, n)), np.arange(max(n - 512, 0), n)]))
    slots = _rng(9, n).permutation(packed_size)
    k = 0
    for i in who:
        c = int(i % 5)
        cols = _rng(10, i).permutation(4)[:c]
        pm[i, cols] = slots[k:k + c]
        k += c
    assert k <= packed_size
    return pm


# ---------------------------------------------------------------------------------------------------------------------------
# the case lists both test modules walk, and the float32 reference's answer in the comparators' `got` format
# ---------------------------------------------------------------------------------------------------------------------------
HEAD_CASES = [(N, lo, hi) for (lo, hi) in HEAD_BOUNDS for N in ROWS]
HEAD_PHASES = (0, 4)
HORIZON_CASES = [(H, N) for H in (1, 2, 5) for N in ROWS]
TWIN_CASES = [(M, Mg) for M in TWIN_M for Mg in (M, 3 * M + 1)]
POLYAK_CASES = [(n, tau) for n in POLYAK_N for tau in POLYAK_TAU]
# name -> (n, keyword arguments of adam_inputs, extras)
ADAM_CASES = {
    "n257": (257, {}, {}),
    "n43977": (43977, {}, {}),
    "tail_pack_map": (ADAM_TAIL_N, {}, {"packed_size": 4096}),
    "partials1": (43977, {}, {"n_partials": 1, "tail": 300}),
    "partials257": (43977, {}, {"n_partials": 257, "tail": 300}),
    "no_clip": (43977, {"max_grad_norm": 0.0}, {"null_sumsq": True}),
    "norm_half": (43977, {"norm_factor": 0.5}, {}),
    "norm_double": (43977, {"norm_factor": 2.0}, {}),
}


def adam_case(name):
    n, kw, extra = ADAM_CASES[name]
    inp = adam_inputs(n, **kw)
    if "packed_size" in extra:
        inp["packed_size"] = extra["packed_size"]
        inp["pack_map"] = adam_pack_map(n, extra["packed_size"])
    return inp, extra


def got_of(out):
    return {k: padded(v) for k, v in out.items() if k != "first"}


def adam_ref32_got(inp):
    s = {k: inp[k] for k in "pmv"}
    got = []
    packed = None if inp.get("pack_map") is None else np.full(inp["packed_size"], SENT_F, dtype=np.float32)
    for k, grad in enumerate(inp["grads"]):
        s = adam_step(s["p"], s["m"], s["v"], grad, inp.get("first_step", 1) + k, inp["cfg"], F32)
        g = got_of(s)
        if packed is not None:
            rows, cols = np.nonzero(inp["pack_map"] >= 0)
            packed[inp["pack_map"][rows, cols]] = s["p"][rows]
            g["packed"] = padded(packed)
        got.append(g)
    return got
