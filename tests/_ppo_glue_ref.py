"""Plain references, inputs and comparators for PPO's head, loss and buffer kernels (vf_ppo.hip, vf_ppo_device.hpp).

No GPU and no ``visfly_amd`` import: numpy / torch-CPU only, written from the reference's formulas (utils/algorithms/PPO.py:210-263,
utils/policies/policies.py:218-220, 250-251, SB3 2.2.1 restated and marked [SB3 2.2.1]), not from the kernels.  Every reference takes
``dtype``: ``torch.float64`` is the truth, ``torch.float32`` is the reference's own arithmetic.  Scalars that reach a kernel as a C
``float`` are rounded with ``f32`` first.

Inputs.  Every case of the head and of the loss is a row-PREFIX of one of two master tables (``table("core")``, 16 385 rows, pre-tanh
values within +-2.5; ``table("tail")``, 1 000 rows, pre-tanh values to +-9 and actions exactly +-1.0f), and the error scale of an
operation is taken over the WHOLE table the case is a prefix of:
    bound = max(4 * E32, 2^-22 * max|ref64|),   E32 = max|ref32 - ref64| over the master table   (per table, per output array)
A bound whose E32 comes from the case's own handful of rows is luck: the float32 reference of a single row is often exact to 1e-9 and
a correct kernel then sits above 4 E32 (M = 1 failed that way at 1.25 of the bound).  The factor 4 is _glue_ref's and is not tuned.
The nine statistics are fp32 sums in a fixed tree:  bound_k = 4 sum_i |t32_i - t64_i| + 32 * 2^-24 * sum_i |t64_i| over the case's
rows (32 >= the additions any term passes through: 6 wave levels, 2 block adds, <= 16 lane-strided adds for <= 1024 partials, 6 wave
levels); statistic 4 is a count and must EQUAL the fp64 count.
Advantage normalisation (the device sums in fp64): per element, mu and sigma from fp64,
    |got_i - ref64_i| <= 2^-23 (4 |a_i - mu| + |mu|) / (sigma + 1e-8)
(one rounding each of (float)mean, (float)sqrt(var), the add of 1e-8, the subtract, the divide).
Copies, selects and single fp32 adds (rollout_post, bootstrap_scatter, gather_rows, the fp32 episode accumulators): bit identity with
the float32 reference.  vf_episode_stats (fp64 accumulators): counts equal, sums within N 2^-53 sum|x|.
Every output buffer is PAD longer and sentinel-filled (``padded`` / ``blank`` / ``body`` of _glue_ref).
Each comparator returns ``{array: (err, scale, bound)}``.
"""
import functools
import math

import numpy as np
import torch

from _glue_ref import F32, F64, PAD, SENT_F, _bits, blank, body, exact, f32, padded  # noqa: F401  (re-exported for the test modules)

EP_SUCCESS, EP_TRUNCATED = 1, 2                      # VF_EP_SUCCESS, VF_EP_TRUNCATED (include/visfly_amd.h)
EPS32 = float(np.finfo(np.float32).eps)
LOG_STD = np.array([0.25, -0.5, -1.0, -0.125], dtype=np.float32)       # four different entries: a wrong dimension index shows


def _t(x, dtype):
    return torch.from_numpy(np.array(x, order="C")).to(dtype)            # a copy: the tables are read-only


def _np(t):
    return t.detach().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def _squashed_log_prob(mu, ls, a):
    """[SB3 2.2.1] common/distributions.py: SquashedDiagGaussianDistribution.log_prob(actions) with gaussian_actions=None, on torch
    tensors of one dtype (differentiable).  ls: (4,) or (M, 4)."""
    # TanhBijector.inverse: eps = th.finfo(y.dtype).eps of the float32 policy; atanh(y.clamp(min=-1.0 + eps, max=1.0 - eps))
    x = a.clamp(min=-1.0 + EPS32, max=1.0 - EPS32)
    g = 0.5 * (x.log1p() - (-x).log1p())
    # DiagGaussianDistribution.proba_distribution: Normal(mean_actions, th.ones_like(mean_actions) * log_std.exp());
    # torch.distributions.Normal.log_prob: -((value - loc) ** 2) / (2 * var) - log_scale - math.log(math.sqrt(2 * math.pi))
    sd = torch.ones_like(mu) * ls.exp()
    lp = (-((g - mu) ** 2) / (2 * sd ** 2) - sd.log() - math.log(math.sqrt(2 * math.pi))).sum(dim=1)       # sum_independent_dims
    lp = lp - torch.sum(torch.log(1 - a ** 2 + 1e-6), dim=1)                                                # self.epsilon = 1e-6
    return lp


def squashed_log_prob(mean, log_std, action, dtype):
    return _np(_squashed_log_prob(_t(mean, dtype), _t(log_std, dtype), _t(action, dtype)))


def head_from_noise(mean, log_std, eps, dtype):
    """policies.py:218-220 with the Gaussian sample given: action = tanh(mean + exp(log_std) eps), and its log-prob"""
    mu, ls = _t(mean, dtype), _t(log_std, dtype)
    a = torch.tanh(mu + ls.exp() * _t(eps, dtype))
    return {"action": _np(a), "log_prob": _np(_squashed_log_prob(mu, ls, a))}


def head_deterministic(mean, log_std, dtype):
    mu, ls = _t(mean, dtype), _t(log_std, dtype)
    a = torch.tanh(mu)
    return {"action": _np(a), "log_prob": _np(_squashed_log_prob(mu, ls, a))}


def loss_cfg(clip_range=0.2, ent_coef=0.01, vf_coef=0.5, inv_batch=1.0, clip_range_vf=0.0, use_old_value=False):
    """the fp32 fields of vf_ppo_loss_cfg; value clipping is on iff clip_range_vf > 0 and use_old_value"""
    return dict(clip_range=f32(clip_range), ent_coef=f32(ent_coef), vf_coef=f32(vf_coef), inv_batch=f32(inv_batch),
                clip_range_vf=f32(clip_range_vf), use_old_value=bool(use_old_value))


def ppo_loss(mean, value, log_std, action, old_lp, adv, ret, old_value, cfg, dtype):
    """PPO.py:210-263 with entropy None (entropy_loss = mean(log_prob)); means are over 1 / inv_batch rows.  Per row: d_mean, d_value
    (torch autograd of the restated loss), the per-row terms of the nine statistics (5..8: the log_std gradient) and the branch masks
    {ratio clipped low, ratio clipped high, value clip active, s1 <= s2}."""
    M = mean.shape[0]
    mu, v = _t(mean, dtype).requires_grad_(), _t(value, dtype).requires_grad_()
    ls = _t(log_std, dtype).expand(M, 4).clone().requires_grad_()         # one copy per row: the per-row terms of d_log_std
    a, olp, A, R = _t(action, dtype), _t(old_lp, dtype), _t(adv, dtype), _t(ret, dtype)
    cr, inv = cfg["clip_range"], cfg["inv_batch"]
    log_prob = _squashed_log_prob(mu, ls, a)
    ratio = torch.exp(log_prob - olp)
    s1 = A * ratio
    s2 = A * torch.clamp(ratio, 1 - cr, 1 + cr)
    pl_rows = -torch.min(s1, s2)
    policy_loss = pl_rows.sum() * inv
    vclip = cfg["clip_range_vf"] > 0 and cfg["use_old_value"]
    if vclip:                                                             # PPO.py:237-245
        ov, cvf = _t(old_value, dtype), cfg["clip_range_vf"]
        values_pred = ov + torch.clamp(v - ov, -cvf, cvf)
        v_active = ((v - ov) < -cvf) | ((v - ov) > cvf)
    else:
        values_pred = v
        v_active = torch.zeros(M, dtype=torch.bool)
    vl_rows = (R - values_pred) ** 2                                      # F.mse_loss(returns, values_pred), per row
    value_loss = vl_rows.sum() * inv
    entropy_loss = -((-log_prob).sum() * inv)
    loss = policy_loss + cfg["ent_coef"] * entropy_loss + cfg["vf_coef"] * value_loss
    loss.backward()
    with torch.no_grad():
        log_ratio = log_prob - olp
        kl_rows = (torch.exp(log_ratio) - 1) - log_ratio
        cf_rows = (torch.abs(ratio - 1) > cr).to(dtype)
        terms = torch.cat([torch.stack([pl_rows, vl_rows, log_prob, kl_rows, cf_rows], dim=1), ls.grad], dim=1)
        masks = torch.stack([ratio < 1 - cr, ratio > 1 + cr, v_active, s1 <= s2], dim=1)
    return {"d_mean": _np(mu.grad), "d_value": _np(v.grad), "terms": _np(terms), "masks": _np(masks)}


def adv_moments(a, rest=None):
    """fp64 mean and unbiased std of the GLOBAL minibatch: this rank's rows and the other ranks' (`rest`)"""
    x = np.asarray(a, dtype=np.float64).reshape(-1)
    if rest is not None:
        x = np.concatenate([x, np.asarray(rest, dtype=np.float64).reshape(-1)])
    return float(x.mean()), float(x.std(ddof=1))


def adv_normalize(a, count, dtype, rest=None):
    """PPO.py:215-220: (a - mean) / (std_unbiased + 1e-8) over `count` global rows.  The moments are the fp64 ones in both dtypes
    (the device sums in fp64); the float32 run rounds them and does the element's three operations in float32."""
    assert np.asarray(a).size + (0 if rest is None else np.asarray(rest).size) == count
    mu, sigma = adv_moments(a, rest)
    x = _t(a, dtype)
    return _np((x - torch.tensor(mu, dtype=dtype)) / (torch.tensor(sigma, dtype=dtype) + 1e-8))


def adv_normalize_segments(a, count, dtype, rest=None):
    """the same for every row of a (n_seg, seg_len): consecutive minibatches, each with its own moments"""
    return np.stack([adv_normalize(a[k], count, dtype, None if rest is None else rest[k]) for k in range(a.shape[0])])


def rollout_post(reward, done, ep_flags, terminal_value, gamma, dtype):
    """[SB3 2.2.1] OnPolicyAlgorithm.collect_rollouts: for idx where done and TimeLimit.truncated: rewards[idx] += gamma *
    terminal_value; the next step's episode_starts = dones.  Only truncated rows are touched."""
    r, tv = _t(reward, dtype).clone(), _t(terminal_value, dtype)
    dn = np.asarray(done) != 0
    for idx in np.flatnonzero(dn & ((np.asarray(ep_flags) & EP_TRUNCATED) != 0)):
        r[idx] += f32(gamma) * tv[idx]
    return {"reward_out": _np(r), "next_start": dn.astype(np.float32 if dtype == F32 else np.float64)}


def rollout_post_collect(reward, done, ep_flags, obs0, obs1, flat_base, ep_return, ep_length, stat, dtype):
    """the deferred form: rewards copied, every truncated row entered as (flat index, terminal observation rows) -- a SET, the order is
    free -- and the per-agent episode accumulators {episodes, sum of returns, sum of lengths, successes} advanced where done"""
    dn = np.asarray(done) != 0
    fl = np.asarray(ep_flags)
    entries = set()
    for i in np.flatnonzero(dn & ((fl & EP_TRUNCATED) != 0)):
        row1 = () if obs1 is None else tuple(_bits(obs1[i]).tolist())
        entries.add((int(flat_base + i), tuple(_bits(obs0[i]).tolist()), row1))
    out = {"reward_out": _np(_t(reward, dtype).clone()), "next_start": dn.astype(np.float32 if dtype == F32 else np.float64),
           "entries": entries}
    if stat is not None:
        s = _t(stat, dtype).clone()
        for i in np.flatnonzero(dn):
            s[i, 0] += 1.0
            s[i, 1] += _t(ep_return, dtype)[i]
            s[i, 2] += float(ep_length[i])
            s[i, 3] += 1.0 if fl[i] & EP_SUCCESS else 0.0
        out["stat"] = _np(s)
    return out


def bootstrap_scatter(idx_list, values, gamma, rewards_flat, dtype):
    """rewards_flat[idx[j]] += gamma * values[j] (the entries name distinct rewards)"""
    r, v = _t(rewards_flat, dtype).clone(), _t(values, dtype)
    for j, at in enumerate(np.asarray(idx_list).tolist()):
        r[at] += f32(gamma) * v[j]
    return _np(r)


def episode_stats(done, ep_return, ep_length, ep_flags, acc):
    """PPO._dump_logs' sums of one step, fp64: acc += {episodes finished, sum of returns, sum of lengths, successes}"""
    dn = np.asarray(done) != 0
    out = np.asarray(acc, dtype=np.float64).copy()
    out[0] += float(dn.sum())
    out[1] += float(np.asarray(ep_return, dtype=np.float64)[dn].sum())
    out[2] += float(np.asarray(ep_length, dtype=np.float64)[dn].sum())
    out[3] += float((dn & ((np.asarray(ep_flags) & EP_SUCCESS) != 0)).sum())
    return out


def gather_rows(src, perm):
    """[SB3 2.2.1] RolloutBuffer.get: field[indices]"""
    return np.ascontiguousarray(src[np.asarray(perm)])


# ---------------------------------------------------------------------------------------------------------------------------
# master tables of the head and the loss
# ---------------------------------------------------------------------------------------------------------------------------
MS = (1, 63, 64, 65, 255, 256, 257, 1000, 16385)             # 16 385 rows leave k_fold_stats 65 partials
TABLE_ROWS = {"core": 16385, "tail": 1000}
M_LIMIT = 262144                                             # vf_ppo_loss's scratch contract
CLIP_RANGE, CLIP_RANGE_VF = 0.2, 0.25                        # 0.25 is binary-exact: rows exactly ON the value-clip bounds exist
RATIO_MARGIN = 2e-3                                          # |log ratio - log(1 -+ clip)| of every row, from the fp64 log-prob
VCLIP_MARGIN = 1e-3                                          # ||value - old_value| - clip_range_vf| of every row but the designated
ROW_ADV0, ROW_VHI, ROW_VLO, ROW_VHI_OUT, ROW_VLO_OUT = 3, 7, 11, 15, 19      # designated rows: inside every size >= 63
ROWS_PLUS1, ROWS_MINUS1 = range(20, 28), range(28, 36)       # tail table: action[r, r % 4] is exactly +1.0f / -1.0f


def _rng(*key):
    return np.random.default_rng([20261, *[int(k) for k in key]])


@functools.lru_cache(maxsize=None)
def table(name):
    """the master table `name`; arrays are read-only, a case takes its first M rows"""
    n = TABLE_ROWS[name]
    rng = _rng(1, n)
    one = np.float32(1.0)
    umax = 2.45 if name == "core" else 9.0
    eps = np.clip(rng.standard_normal((n, 4)), -2.5, 2.5).astype(np.float32)
    u = rng.uniform(-umax, umax, (n, 4))
    if name == "core":
        u[0] = [2.4, -2.4, 2.4, -2.4]                        # row 0 (the M = 1 case) far out on the tanh: the 1e-6 counts there
    else:
        for r in ROWS_PLUS1:
            u[r, r % 4] = 9.0
        for r in ROWS_MINUS1:
            u[r, r % 4] = -9.0
    mean0 = (u - np.exp(LOG_STD.astype(np.float64)) * eps).astype(np.float32)        # the roll-out's mean
    pre = mean0.astype(np.float64) + np.exp(LOG_STD.astype(np.float64)) * eps
    assert np.abs(pre).max() <= (2.5 if name == "core" else 9.01)
    pre = pre.astype(np.float32)                             # the deterministic head's mean: tanh(pre) are the same actions
    action = head_from_noise(mean0, LOG_STD, eps, F32)["action"].copy()
    if name == "tail":
        for r in ROWS_PLUS1:
            action[r, r % 4] = one
        for r in ROWS_MINUS1:
            action[r, r % 4] = -one
    mean = (mean0 + 0.1 * rng.standard_normal((n, 4))).astype(np.float32)            # the policy moved since the roll-out
    value = rng.standard_normal(n).astype(np.float32)
    ret = (value + 0.5 * rng.standard_normal(n) + 0.2).astype(np.float32)
    adv = rng.standard_normal(n).astype(np.float32)                                  # mixed signs
    adv[ROW_ADV0] = 0.0
    # value clipping: value - old_value spread over +-0.6 and kept VCLIP_MARGIN away from +-clip_range_vf ...
    old_value = (value - rng.uniform(-0.6, 0.6, n)).astype(np.float32)
    for _ in range(4):
        dvo = value.astype(np.float64) - old_value
        near = np.abs(np.abs(dvo) - CLIP_RANGE_VF) < 2 * VCLIP_MARGIN
        old_value[near] += np.float32(8 * VCLIP_MARGIN)
    # ... except the designated rows: exactly on either bound (the gradient passes on the closed interval), one fp32 step outside
    ninf, pinf = np.float32(-np.inf), np.float32(np.inf)
    for r, v_, o_ in ((ROW_VHI, 0.75, 0.5), (ROW_VLO, 0.5, 0.75), (ROW_VHI_OUT, np.nextafter(np.float32(0.75), pinf), 0.5),
                      (ROW_VLO_OUT, np.nextafter(np.float32(0.5), ninf), 0.75)):
        value[r], old_value[r] = v_, o_
        ret[r] = value[r] - one                                                      # values_pred - return about 1: a gradient to lose
    # old log-prob: the fp64 log-prob plus noise of scale 0.3 (both clip sides fire), RATIO_MARGIN away from the clip edges
    lp64 = squashed_log_prob(mean, LOG_STD, action, F64)
    old_lp = (lp64 + 0.3 * rng.standard_normal(n)).astype(np.float32)
    edges = (math.log(1 - f32(CLIP_RANGE)), math.log(1 + f32(CLIP_RANGE)))
    for _ in range(4):
        lr = lp64 - old_lp
        near = (np.abs(lr - edges[0]) < 2 * RATIO_MARGIN) | (np.abs(lr - edges[1]) < 2 * RATIO_MARGIN)
        old_lp[near] += np.float32(8 * RATIO_MARGIN)
    t = dict(mean0=mean0, eps=eps, pre=pre, mean=mean, action=action, value=value, ret=ret, adv=adv, old_value=old_value, old_lp=old_lp,
             log_std=LOG_STD.copy())
    for a in t.values():
        a.setflags(write=False)
    return t


def case_rows(M):
    """row indices of a case: the first M rows; the 262 144-row case repeats the core table's first 16 384 rows 16 times"""
    return np.arange(M) if M <= 16385 else np.arange(M) % 16384


LOSS_FIELDS = ("mean", "value", "action", "old_lp", "adv", "ret", "old_value")


def loss_inputs(name, M):
    t = table(name)
    rows = case_rows(M)
    inp = {k: np.ascontiguousarray(t[k][rows]) for k in LOSS_FIELDS}
    inp["log_std"] = t["log_std"]
    return inp


def head_inputs(name, M):
    t = table(name)
    return dict(mean=np.ascontiguousarray(t["mean0"][:M]), pre=np.ascontiguousarray(t["pre"][:M]), eps=np.ascontiguousarray(t["eps"][:M]), log_std=t["log_std"])


VMODES = ("off", "on", "null_old_value", "on_ent0")          # the issue's three, and value clipping on with ent_coef = 0 (exact-zero d_mean rows)


def loss_case_cfg(M, vmode, inv_kind):
    inv = 1.0 / M if inv_kind == "local" else 1.0 / (3 * M + 1)
    if vmode == "off":
        return loss_cfg(CLIP_RANGE, inv_batch=inv)
    if vmode == "null_old_value":                            # clip_range_vf > 0 with old_value NULL: off by contract
        return loss_cfg(CLIP_RANGE, inv_batch=inv, clip_range_vf=CLIP_RANGE_VF, use_old_value=False)
    return loss_cfg(CLIP_RANGE, inv_batch=inv, clip_range_vf=CLIP_RANGE_VF, use_old_value=True, ent_coef=0.0 if vmode == "on_ent0" else 0.01)


LOSS_CASES = ([("core", M, vm, ik) for M in MS for vm in VMODES for ik in ("local", "global")] +
              [("tail", 1000, vm, ik) for vm in VMODES for ik in ("local", "global")])


@functools.lru_cache(maxsize=None)
def _head_refs(name, deterministic):
    t = table(name)
    if deterministic:
        return head_deterministic(t["pre"], t["log_std"], F32), head_deterministic(t["pre"], t["log_std"], F64)
    return head_from_noise(t["mean0"], t["log_std"], t["eps"], F32), head_from_noise(t["mean0"], t["log_std"], t["eps"], F64)


@functools.lru_cache(maxsize=64)
def _loss_refs(name, cfg_items):
    t, cfg = table(name), dict(cfg_items)
    args = (t["mean"], t["value"], t["log_std"], t["action"], t["old_lp"], t["adv"], t["ret"], t["old_value"], cfg)
    return ppo_loss(*args, F32), ppo_loss(*args, F64)


def loss_refs(name, cfg):
    """(float32, float64) reference over the WHOLE master table, under this case's cfg"""
    return _loss_refs(name, tuple(sorted(cfg.items())))


# ---------------------------------------------------------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------------------------------------------------------
def within_pooled(name, got, ref32_tab, ref64_tab, rows):
    """max over the case's rows of |got - ref64| <= max(4 E32, 2^-22 max|ref64|) with E32 and the maximum over the whole master
    table; where both references are exactly zero (a gradient a clip switched off) got must be zero (the sign is not compared)"""
    got = np.asarray(got)
    r32, r64 = ref32_tab[rows], ref64_tab[rows]
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert got.dtype == np.float32 and ref32_tab.dtype == np.float32 and ref64_tab.dtype == np.float64, name
    assert np.isfinite(ref64_tab).all() and np.isfinite(ref32_tab).all(), f"{name}: non-finite reference"
    assert np.isfinite(got).all(), f"{name}: non-finite value at {np.flatnonzero(~np.isfinite(got).reshape(-1))[:4]}"
    e32 = float(np.abs(ref32_tab.astype(np.float64) - ref64_tab).max())
    bound = max(4.0 * e32, 2.0 ** -22 * float(np.abs(ref64_tab).max()))
    d = np.abs(got.astype(np.float64) - r64)
    err = float(d.max())
    assert err <= bound, f"{name}: max|got - ref64| = {err:.3e} at {int(d.argmax())} > bound {bound:.3e} (table E32 = {e32:.3e})"
    zero = (r64 == 0) & (r32 == 0)
    assert not np.any(got[zero]), f"{name}: not zero where the reference's gradient is switched off ({int(np.count_nonzero(got[zero]))} elements)"
    return (err, e32, bound)


def check_head(got, name, M, deterministic=False):
    r32, r64 = _head_refs(name, bool(deterministic))
    rows = np.arange(M)
    return {"action": within_pooled("action", body("action", got["action"], (M, 4)), r32["action"], r64["action"], rows),
            "log_prob": within_pooled("log_prob", body("log_prob", got["log_prob"], (M,)), r32["log_prob"], r64["log_prob"], rows)}


def stats_bounds(t32, t64):
    """per statistic k: (fp64 sum, scale = sum|t32 - t64|, bound = 4 scale + 32 * 2^-24 * sum|t64|), over the rows given"""
    t32, t64 = np.asarray(t32, dtype=np.float64), np.asarray(t64, dtype=np.float64)
    s64 = np.array([math.fsum(t64[:, k]) for k in range(9)])
    scale = np.abs(t32 - t64).sum(0)
    return s64, scale, 4.0 * scale + 32.0 * 2.0 ** -24 * np.abs(t64).sum(0)


def check_ppo_loss(got, name, M, cfg):
    """got: padded d_mean (M, 4), d_value (M,), stats (16,)"""
    r32, r64 = loss_refs(name, cfg)
    rows = case_rows(M)
    out = {"d_mean": within_pooled("d_mean", body("d_mean", got["d_mean"], (M, 4)), r32["d_mean"], r64["d_mean"], rows),
           "d_value": within_pooled("d_value", body("d_value", got["d_value"], (M,)), r32["d_value"], r64["d_value"], rows)}
    st = body("stats", got["stats"], (16,))
    assert st.dtype == np.float32 and np.isfinite(st).all(), "stats: non-finite"
    assert not np.any(st[9:]), "stats[9..15]: not zero"
    s64, scale, bound = stats_bounds(r32["terms"][rows], r64["terms"][rows])
    for k in range(9):
        err = abs(float(st[k]) - s64[k])
        if k == 4:
            assert float(st[4]) == s64[4], f"stats[4] (clip fraction): {st[4]!r} rows counted, the fp64 reference counts {s64[4]!r}"
            out["stats4"] = (0.0, 0.0, 0.0)
            continue
        assert err <= bound[k], f"stats[{k}]: |got - sum64| = {err:.3e} > bound {bound[k]:.3e} (sum|t32 - t64| = {scale[k]:.3e})"
        out[f"stats{k}"] = (err, float(scale[k]), float(bound[k]))
    return out


def check_loss_side_outputs(stats_calls, stats_accum, accum_before, d_log_std_out):
    """stats_accum after the calls = the fp32 sum of their stats added one call at a time, d_log_std_out = the last stats[5..8]: bit
    for bit.  All arguments are padded buffers but accum_before (16,)."""
    acc = np.asarray(accum_before, dtype=np.float32).copy()
    for s in stats_calls:
        acc = acc + body("stats", s, (16,))
    exact("stats_accum", body("stats_accum", stats_accum, (16,)), acc)
    exact("d_log_std_out", body("d_log_std_out", d_log_std_out, (4,)), body("stats", stats_calls[-1], (16,))[5:9])
    return {"stats_accum": (0.0, 0.0, 0.0), "d_log_std_out": (0.0, 0.0, 0.0)}


def check_adv(name, got, a, mu, sigma, constant=False):
    """per element |got - ref64| <= 2^-23 (4 |a - mu| + |mu|) / (sigma + 1e-8); a constant segment must give finite zeros"""
    got, a64 = np.asarray(got), np.asarray(a, dtype=np.float64)
    assert got.dtype == np.float32 and got.shape == a64.shape, (name, got.dtype, got.shape, a64.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite value"
    if constant:
        assert sigma == 0.0 and not np.any(got), f"{name}: a constant segment must normalise to zeros"
        return (0.0, 0.0, 0.0)
    ref64 = (a64 - mu) / (sigma + 1e-8)
    bound = 2.0 ** -23 * (4.0 * np.abs(a64 - mu) + abs(mu)) / (sigma + 1e-8)
    d = np.abs(got.astype(np.float64) - ref64)
    worst = int((d / bound).argmax())
    assert np.all(d <= bound), (f"{name}: |got - ref64| = {d.reshape(-1)[worst]:.3e} at {worst} > bound {bound.reshape(-1)[worst]:.3e} "
                                f"({int((d > bound).sum())} of {d.size} elements over)")
    # (err, scale, bound) of the element closest to its bound; scale: ONE float32 rounding of mu and one of the element's result
    scale = 2.0 ** -24 * (np.abs(a64 - mu) + abs(mu)) / (sigma + 1e-8)
    return (float(d.reshape(-1)[worst]), float(scale.reshape(-1)[worst]), float(bound.reshape(-1)[worst]))


def check_adv_normalize(got, inp):
    n = inp["a"].size
    mu, sigma = adv_moments(inp["a"], inp.get("rest"))
    return {"out": check_adv("out", body("out", got["out"], (n,)), inp["a"], mu, sigma)}


def check_adv_segments(got, inp):
    a = inp["a"]
    out = body("out", got["out"], a.shape)
    res = None
    for k in range(a.shape[0]):
        mu, sigma = adv_moments(a[k], None if inp.get("rest") is None else inp["rest"][k])
        r = check_adv(f"out[segment {k}]", out[k], a[k], mu, sigma, constant=(k == inp.get("constant_segment")))
        res = r if res is None or (r[2] and r[0] / r[2] > (res[0] / res[2] if res[2] else -1.0)) else res
    return {"out": res}


def check_rollout_post(got, inp):
    r32 = rollout_post(inp["reward"], inp["done"], inp["ep_flags"], inp["terminal_value"], inp["gamma"], F32)
    N = inp["reward"].shape
    return {k: exact(k, body(k, got[k], N), r32[k]) for k in ("reward_out", "next_start")}


def check_collect(got, inp, entries_before=frozenset(), cursor_before=0):
    """got: padded reward_out, next_start, stat (N, 4), and the list as the caller read it: cursor (int), idx_list / rows0 / rows1
    (padded, `capacity` rows).  Entries are compared as a set; with capacity short of the truncated rows the cursor counts them all
    and the stored ones are `capacity` distinct members of the set."""
    r32 = rollout_post_collect(inp["reward"], inp["done"], inp["ep_flags"], inp["obs0"], inp.get("obs1"), inp["flat_base"],
                               inp["ep_return"], inp["ep_length"], inp.get("stat"), F32)
    N = inp["reward"].shape
    out = {k: exact(k, body(k, got[k], N), r32[k]) for k in ("reward_out", "next_start")}
    if inp.get("stat") is not None:
        out["stat"] = exact("stat", body("stat", got["stat"], inp["stat"].shape), r32["stat"])
    want = set(entries_before) | r32["entries"]
    assert len(want) == len(entries_before) + len(r32["entries"])
    assert got["cursor"] == cursor_before + len(r32["entries"]), f"cursor {got['cursor']}, expected {cursor_before + len(r32['entries'])}"
    cap, w0 = inp["capacity"], inp["obs0"].shape[1]
    w1 = 0 if inp.get("obs1") is None else inp["obs1"].shape[1]
    idx = body("idx_list", got["idx_list"], (cap,))
    rows0 = body("rows0", got["rows0"], (cap, w0))
    rows1 = body("rows1", got["rows1"], (cap, w1)) if w1 else None
    stored = min(got["cursor"], cap)
    have = {(int(idx[j]), tuple(_bits(rows0[j]).tolist()), () if rows1 is None else tuple(_bits(rows1[j]).tolist())) for j in range(stored)}
    assert len(have) == stored, "the list names a reward twice"
    assert have <= want, f"entries nobody truncated: {sorted(e[0] for e in have - want)[:8]}"
    assert stored == min(len(want), cap) and (have == want or len(want) > cap), f"entries missing: {sorted(e[0] for e in want - have)[:8]}"
    # slots past the cursor (and past capacity: the pad) were never written
    assert np.all(_bits(idx[stored:]) == _bits(np.full(cap - stored, SENT_I, dtype=np.int32))), "idx_list written past the cursor"
    assert np.all(_bits(rows0[stored:]) == _bits(np.full((cap - stored, w0), SENT_F, dtype=np.float32))), "rows0 written past the cursor"
    out["entries"] = (0.0, 0.0, 0.0)
    return out


def check_episode_stats(got_acc, inp, acc_before):
    want = episode_stats(inp["done"], inp["ep_return"], inp["ep_length"], inp["ep_flags"], acc_before)
    got = np.asarray(got_acc, dtype=np.float64)
    assert got.shape == (4,)
    dn = inp["done"] != 0
    N = dn.size
    assert got[0] == want[0] and got[3] == want[3], f"counts {got[0]}, {got[3]}; expected {want[0]}, {want[3]}"
    out = {"episodes": (0.0, 0.0, 0.0), "successes": (0.0, 0.0, 0.0)}
    for k, x in ((1, inp["ep_return"]), (2, inp["ep_length"])):
        mass = float(np.abs(np.asarray(x, dtype=np.float64)[dn]).sum()) + abs(float(acc_before[k]))
        bound = N * 2.0 ** -53 * mass
        err = abs(got[k] - want[k])
        assert err <= bound, f"acc[{k}]: |got - sum64| = {err:.3e} > {bound:.3e}"
        out["return_sum" if k == 1 else "length_sum"] = (err, 2.0 ** -53 * mass, bound)
    return out


def check_gather(got, inp):
    out = {}
    for i, (src, g) in enumerate(zip(inp["src"], got)):
        out[f"field{i}"] = exact(f"field {i} (width {src.shape[1]})", body(f"field {i}", g, (inp["perm"].size, src.shape[1])),
                                 gather_rows(src, inp["perm"]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# inputs of the buffer kernels
# ---------------------------------------------------------------------------------------------------------------------------
SENT_I = np.int32(SENT_F)                                    # what blank(..., np.int32) holds
ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)
DONE_BYTES = (1, 0, 255)
# every combination of the four ep_flags bits with every done byte; (1, TRUNCATED) first, so the single row of N = 1 bootstraps
TRUTH = sorted([(d, f) for f in range(16) for d in DONE_BYTES], key=lambda t: (t != (1, EP_TRUNCATED),))
ADV_N = (2, 255, 257, 65537, 262144 + 257)                   # both sides of the grid caps: 256 blocks for the sums, 1024 for the apply
SEG_N, SEG_LEN = (1, 3, 7), (1, 255, 257, 1025, 65537)
GATHER_WIDTHS = (1, 3, 4, 5, 13, 64, 255, 256)
GATHER_ROWS = (1, 255, 257, 70001)
EPISODE_N = (1, 1023, 1024, 1025, 8191, 8192, 8193, 70001)   # k_episode_stats unrolls 8 strides of 1024 with a clamped index


def rollout_inputs(N, shift=0, w0=13, w1=3):
    """agent i carries TRUTH[(i + shift) % 48]: any 48 consecutive agents hold every (done byte, ep_flags) combination.  Every
    fifth reward is -0.0; terminal_value is non-finite (nan, +inf, -inf in turn) on every row that does NOT truncate."""
    rng = _rng(2, N, shift)
    tab = np.array(TRUTH, dtype=np.uint8)[(np.arange(N) + shift) % len(TRUTH)]
    done, flags = tab[:, 0].copy(), tab[:, 1].copy()
    reward = rng.standard_normal(N).astype(np.float32)
    reward[(np.arange(N) + shift) % 5 == 1] = np.float32(-0.0)
    tv = (rng.standard_normal(N) * 3).astype(np.float32)
    trunc = (done != 0) & ((flags & EP_TRUNCATED) != 0)
    bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[np.arange(N) % 3]
    tv[~trunc] = bad[~trunc]
    stat = np.stack([rng.integers(0, 5, N), rng.standard_normal(N) * 10, rng.integers(0, 900, N), rng.integers(0, 3, N)], axis=1)
    return dict(reward=reward, done=done, ep_flags=flags, terminal_value=tv, gamma=0.99, truncated=trunc,
                obs0=rng.standard_normal((N, w0)).astype(np.float32), obs1=rng.standard_normal((N, w1)).astype(np.float32) if w1 else None,
                ep_return=(rng.standard_normal(N) * 20).astype(np.float32), ep_length=rng.integers(1, 600, N).astype(np.int32),
                stat=stat.astype(np.float32))


def episode_inputs(N, call=0):
    """done bytes 0 / 1 / 255 in turn, the last agent done (255) and successful with a return and a length nobody can miss"""
    rng = _rng(3, N, call)
    done = np.array([0, 1, 255], dtype=np.uint8)[(np.arange(N) + call) % 3]
    flags = rng.integers(0, 16, N).astype(np.uint8)
    ep_return = (rng.standard_normal(N) * 20).astype(np.float32)
    ep_length = rng.integers(1, 600, N).astype(np.int32)
    done[N - 1], flags[N - 1], ep_return[N - 1], ep_length[N - 1] = 255, EP_SUCCESS | 4, 777.25, 12345
    return dict(done=done, ep_flags=flags, ep_return=ep_return, ep_length=ep_length)


def adv_inputs(n, count):
    """this rank's n advantages 1.5 + 3 randn, and the count - n rows of the other ranks (same law, another mean: the all-reduce counts)"""
    rng = _rng(4, n, count)
    a = (1.5 + 3.0 * rng.standard_normal(n)).astype(np.float32)
    rest = None if count == n else (2.25 + 3.0 * rng.standard_normal(count - n)).astype(np.float32)
    return dict(a=a, rest=rest, count=count)


def adv_segment_inputs(n_seg, seg_len, count):
    """n_seg consecutive minibatches with means and spreads of their own; with count == seg_len > 1 and n_seg > 1 segment 1 is constant
    (every element the same fp32 value 0.1f)"""
    rng = _rng(5, n_seg, seg_len, count)
    a = np.stack([(1.5 * (k - 1) + (1.0 + k) * rng.standard_normal(seg_len)) for k in range(n_seg)]).astype(np.float32)
    rest = None if count == seg_len else np.stack([(0.5 * k + 2.0 * rng.standard_normal(count - seg_len)) for k in range(n_seg)]).astype(np.float32)
    const = 1 if (count == seg_len and seg_len > 1 and n_seg > 1) else None
    if const is not None:
        a[const] = np.float32(0.1)
    return dict(a=a, rest=rest, count=count, constant_segment=const)


ADV_CASES = [(n, c) for n in ADV_N for c in (n, 3 * n + 1)]
SEG_CASES = [(s, L, c) for s in SEG_N for L in SEG_LEN for c in (L, 3 * L + 1) if c >= 2]


def sums_of(x):
    """{sum, sum of squares} in fp64: what a rank contributes to the all-reduce between phase 0 and phase 1"""
    x = np.asarray(x, dtype=np.float64)
    return np.array([x.sum(), (x * x).sum()])


def gather_inputs(rows, kind, widths=GATHER_WIDTHS):
    """field f, source row r, column c holds the float whose BITS are (f << 27) | (r << 8) | c: every element names its origin (no
    NaN pattern: the exponent field never fills).  kind: "perm" (a permutation) or "repeats" (indices drawn with replacement)."""
    rng = _rng(6, rows, len(widths), kind == "perm")
    assert rows < (1 << 19) and len(widths) <= 8
    src = [(((np.uint32(f) << np.uint32(27)) | (np.arange(rows, dtype=np.uint32)[:, None] << np.uint32(8)) |
             np.arange(w, dtype=np.uint32)[None, :]).astype(np.uint32)).view(np.float32) for f, w in enumerate(widths)]
    perm = rng.permutation(rows) if kind == "perm" else rng.integers(0, rows, rows)
    if kind == "repeats" and rows > 2:
        perm[-1] = perm[0]                                               # at least one repeat, whatever the draw
    return dict(src=src, perm=perm.astype(np.int64))
