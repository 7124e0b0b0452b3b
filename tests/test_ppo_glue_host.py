"""The references of tests/_ppo_glue_ref.py against torch's own machinery in fp64, the condition the pooled bounds rest on, and the
comparators' teeth.  Nothing here touches a GPU or the library.

  * every restated reference equals torch in fp64: the squashed log-prob against torch.distributions.Normal plus the correction, the
    loss gradients against autograd of a second, independently written loss (th.min / th.clamp / F.mse_loss as PPO.py:223-263 has
    them) with identical zero sets, the log_std statistics against log_std.grad, the normalisation against mean() / std();
  * the condition: on every row of both master tables the float32 and the float64 reference take the same branches (ratio clipped
    low / high, value clip active, which of s1 / s2 is the minimum), under every configuration the GPU cases use, and every size
    >= 63 holds rows of every branch and the designated rows;
  * for every comparator and every input set of tests/test_ppo_glue_gpu.py the float32 reference passes, a numpy-float32
    restatement of the kernel's operation order (-0.5 z z - ls - c, z = (g - mu) / sd) passes, and every listed mutant fails on those
    very inputs.  Mutants are applied in numpy on the host; no wrong kernel is ever built.
"""
import math

import numpy as np
import pytest
import torch

import _ppo_glue_ref as P
from _ppo_glue_ref import F32, F64

f = np.float32


def rejects(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def close64(got, want, what, rtol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want).max()
    assert err <= rtol * max(np.abs(want).max(), 1e-300), f"{what}: {err:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# references against torch in fp64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.TABLE_ROWS))
def test_log_prob_reference_is_torch_normal_plus_correction(name):
    t = P.table(name)
    mu, a = torch.tensor(t["mean"]).double(), torch.tensor(t["action"]).double()
    sd = torch.ones_like(mu) * torch.tensor(t["log_std"]).double().exp()
    eps = torch.finfo(torch.float32).eps
    g = torch.atanh(a.clamp(min=-1.0 + eps, max=1.0 - eps))
    lp = torch.distributions.Normal(mu, sd).log_prob(g).sum(dim=1) - torch.sum(torch.log(1 - a ** 2 + 1e-6), dim=1)
    close64(P.squashed_log_prob(t["mean"], t["log_std"], t["action"], F64), lp.numpy(), "log_prob", 1e-11)
    h = P.head_from_noise(t["mean0"], t["log_std"], t["eps"], F64)
    close64(h["action"], np.tanh(t["mean0"].astype(np.float64) + np.exp(t["log_std"].astype(np.float64)) * t["eps"]), "action", 1e-15)
    close64(P.head_deterministic(t["pre"], t["log_std"], F64)["action"], np.tanh(t["pre"].astype(np.float64)), "action (deterministic)", 1e-15)
    if name == "tail":
        assert sum(t["action"][r, r % 4] == 1.0 for r in P.ROWS_PLUS1) >= 8 and sum(t["action"][r, r % 4] == -1.0 for r in P.ROWS_MINUS1) >= 8
        assert np.abs(t["pre"]).max() >= 9.0
    else:
        assert np.abs(t["pre"]).max() <= 2.5


def _independent_loss(t, M, cfg, vclip):
    """PPO.py:210-263 verbatim on the first M rows (M a power of two: 1 / M is exact), log-prob from torch.distributions"""
    import torch as th
    import torch.nn.functional as F
    mu = th.tensor(t["mean"][:M]).double().requires_grad_()
    values = th.tensor(t["value"][:M]).double().requires_grad_()
    log_std = th.tensor(t["log_std"]).double().requires_grad_()
    actions = th.tensor(t["action"][:M]).double()
    old_log_prob, advantages, returns, old_values = (th.tensor(t[k][:M]).double() for k in ("old_lp", "adv", "ret", "old_value"))
    clip_range, clip_range_vf = cfg["clip_range"], (cfg["clip_range_vf"] if vclip else None)
    eps = th.finfo(th.float32).eps
    gaussian_actions = th.atanh(actions.clamp(min=-1.0 + eps, max=1.0 - eps))
    log_prob = th.distributions.Normal(mu, th.ones_like(mu) * log_std.exp()).log_prob(gaussian_actions).sum(dim=1)
    log_prob = log_prob - th.sum(th.log(1 - actions ** 2 + 1e-6), dim=1)
    ratio = th.exp(log_prob - old_log_prob)
    policy_loss_1 = advantages * ratio
    policy_loss_2 = advantages * th.clamp(ratio, 1 - clip_range, 1 + clip_range)
    policy_loss = -th.min(policy_loss_1, policy_loss_2).mean()
    clip_fraction = th.mean((th.abs(ratio - 1) > clip_range).float()).item()
    if clip_range_vf is None:
        values_pred = values
    else:
        values_pred = old_values + th.clamp(values - old_values, -clip_range_vf, clip_range_vf)
    value_loss = F.mse_loss(returns, values_pred)
    entropy_loss = -th.mean(-log_prob)
    loss = policy_loss + cfg["ent_coef"] * entropy_loss + cfg["vf_coef"] * value_loss
    loss.backward()
    with th.no_grad():
        log_ratio = log_prob - old_log_prob
        approx_kl_div = th.mean((th.exp(log_ratio) - 1) - log_ratio).item()
    return dict(d_mean=mu.grad.numpy(), d_value=values.grad.numpy(), d_log_std=log_std.grad.numpy(),
                means=[policy_loss.item(), value_loss.item(), entropy_loss.item(), approx_kl_div, clip_fraction])


@pytest.mark.parametrize("vmode", P.VMODES)
@pytest.mark.parametrize("name,M", [("core", 256), ("core", 16384), ("tail", 512)])
def test_loss_reference_is_autograd_of_the_reference_loss(name, M, vmode):
    t = P.table(name)
    cfg = P.loss_case_cfg(M, vmode, "local")
    assert cfg["inv_batch"] == 1.0 / M
    want = _independent_loss(t, M, cfg, vclip=vmode in ("on", "on_ent0"))
    r = P.ppo_loss(*(t[k][:M] for k in ("mean", "value")), t["log_std"], *(t[k][:M] for k in ("action", "old_lp", "adv", "ret", "old_value")),
                   cfg, F64)
    close64(r["d_mean"], want["d_mean"], "d_mean", 1e-11)
    close64(r["d_value"], want["d_value"], "d_value", 1e-11)
    assert np.array_equal(r["d_mean"] == 0, want["d_mean"] == 0) and np.array_equal(r["d_value"] == 0, want["d_value"] == 0)
    close64(r["terms"][:, 5:9].sum(0), want["d_log_std"], "d_log_std: the statistics 5..8 summed over the rows", 1e-10)
    close64(r["terms"][:, :5].sum(0) / M, want["means"], "statistics 0..4 over M", 1e-10)
    if vmode in ("on", "on_ent0"):
        # th.clamp passes the gradient ON the bounds and nowhere outside: the designated rows
        assert want["d_value"][P.ROW_VHI] != 0 and want["d_value"][P.ROW_VLO] != 0
        assert want["d_value"][P.ROW_VHI_OUT] == 0 and want["d_value"][P.ROW_VLO_OUT] == 0
        assert (r["masks"][:, 2] == (want["d_value"] == 0)).all()
    if vmode == "on_ent0":
        dead = r["masks"][:, :2].any(1) & ~r["masks"][:, 3]
        assert dead.sum() > M // 8 and not np.any(want["d_mean"][dead]), "clipped with s2 the minimum: no gradient"


@pytest.mark.parametrize("n,count", [(257, 257), (1000, 1000)])
def test_adv_reference_is_mean_and_unbiased_std(n, count):
    inp = P.adv_inputs(n, count)
    a = torch.tensor(inp["a"]).double()
    close64(P.adv_normalize(inp["a"], count, F64), ((a - a.mean()) / (a.std() + 1e-8)).numpy(), "adv_normalize")
    seg = P.adv_segment_inputs(3, 257, 3 * 257 + 1)
    k = 2
    x = torch.tensor(np.concatenate([seg["a"][k], seg["rest"][k]])).double()
    close64(P.adv_normalize_segments(seg["a"], seg["count"], F64, seg["rest"])[k], ((x - x.mean()) / (x.std() + 1e-8)).numpy()[:257], "segment 2")


# ---------------------------------------------------------------------------------------------------------------------------
# the condition of the pooled bounds
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.TABLE_ROWS))
def test_fp32_and_fp64_references_take_the_same_branches(name):
    t = P.table(name)
    n = P.TABLE_ROWS[name]
    for vmode in P.VMODES:
        for M, ik in ((n, "local"), (63, "global")):
            r32, r64 = P.loss_refs(name, P.loss_case_cfg(M, vmode, ik))
            assert np.array_equal(r32["masks"], r64["masks"]), (vmode, np.flatnonzero((r32["masks"] != r64["masks"]).any(1))[:8])
    # the stated margins, from the fp64 log-prob and the exact value differences
    lr = P.squashed_log_prob(t["mean"], t["log_std"], t["action"], F64) - t["old_lp"]
    for edge in (math.log(1 - P.f32(P.CLIP_RANGE)), math.log(1 + P.f32(P.CLIP_RANGE))):
        assert np.abs(lr - edge).min() >= P.RATIO_MARGIN
    dvo = t["value"].astype(np.float64) - t["old_value"]
    free = np.ones(n, dtype=bool)
    free[[P.ROW_VHI, P.ROW_VLO, P.ROW_VHI_OUT, P.ROW_VLO_OUT]] = False
    assert np.abs(np.abs(dvo[free]) - P.CLIP_RANGE_VF).min() >= P.VCLIP_MARGIN
    assert dvo[P.ROW_VHI] == P.CLIP_RANGE_VF and dvo[P.ROW_VLO] == -P.CLIP_RANGE_VF and t["adv"][P.ROW_ADV0] == 0
    assert dvo[P.ROW_VHI_OUT] == float(np.nextafter(f(0.75), f(1)) - f(0.5)) > P.CLIP_RANGE_VF
    assert dvo[P.ROW_VLO_OUT] == float(np.nextafter(f(0.5), f(0)) - f(0.75)) < -P.CLIP_RANGE_VF
    # every size >= 63 holds every branch, both signs of the advantage, and both sides of the value clip
    m = P.loss_refs(name, P.loss_case_cfg(63, "on", "local"))[1]["masks"][:63]
    assert all(m[:, k].any() and not m[:, k].all() for k in range(4)) and (m[:, 0] & ~m[:, 3]).any() and (m[:, 1] & ~m[:, 3]).any()
    assert (t["adv"][:63] > 0).any() and (t["adv"][:63] < 0).any() and (dvo[:63] > P.CLIP_RANGE_VF).any() and (dvo[:63] < -P.CLIP_RANGE_VF).any()
    assert len(set(t["log_std"].tolist())) == 4


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's operation order in numpy float32, with the mutations switched in
# ---------------------------------------------------------------------------------------------------------------------------
def _lp_np32(mu, ls, a, drop_1e6=False, half_eps=False):
    eps = f(1.1920929e-07) * (f(0.5) if half_eps else f(1))
    x = np.minimum(np.maximum(a, f(-1) + eps), f(1) - eps)
    g = f(0.5) * (np.log1p(x) - np.log1p(-x))
    sd = np.exp(ls)
    lp = np.zeros(mu.shape[0], f)
    z = (g - mu) / sd
    for d in range(4):
        lp = lp + (f(-0.5) * z[:, d] * z[:, d] - ls[d] - f(0.91893853320467274178))
        lp = lp - np.log(f(1) - a[:, d] * a[:, d] + (f(0) if drop_1e6 else f(1e-6)))
    assert lp.dtype == np.float32
    return lp, z, sd


def _wave_sum(x):
    """the shuffle tree over the last axis (64 lanes): lanes i and i ^ 32, then ^ 16, ... -- halves added, six levels"""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def _stats_tree(terms, skip_last=False, twice=False):
    """k_ppo_loss + k_fold_stats in numpy float32: per block of 256 rows four wave trees and (w0 + w1) + (w2 + w3); then per
    statistic 64 lanes add the partials b = lane, lane + 64, ... in turn and one more wave tree"""
    M = terms.shape[0]
    nblk = (M + 255) // 256
    x = np.zeros((nblk * 256, 9), f)
    x[:M - 1 if skip_last else M] = terms[:M - 1 if skip_last else M]
    w = _wave_sum(np.ascontiguousarray(x.reshape(nblk, 4, 64, 9).transpose(0, 1, 3, 2)))          # (nblk, 4, 9)
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    if twice:
        part = np.concatenate([part, part[:1]])                          # the first block's partial once more
    lanes = np.zeros((64, 9), f)
    for b in range(part.shape[0]):
        lanes[b % 64] += part[b]
    out = np.zeros(16, f)
    out[:9] = _wave_sum(np.ascontiguousarray(lanes.T))
    assert part.dtype == np.float32
    return out


def _head_np32(inp, rotate=False, **mut):
    ls = np.roll(inp["log_std"], 1) if rotate else inp["log_std"]
    with np.errstate(all="ignore"):
        a = np.tanh(inp["mean"] + np.exp(ls) * inp["eps"])
        lp = _lp_np32(inp["mean"], ls, a, **mut)[0]
    return {"action": P.padded(a), "log_prob": P.padded(lp)}


def _loss_np32(inp, cfg, rotate=False, ent_sign=1.0, ent_unscaled=False, gate="closed", shift_old_value=False, skip_last=False,
               twice=False, **lp_mut):
    ls = np.roll(inp["log_std"], 1) if rotate else inp["log_std"]
    cr, ent, vfc, inv, cvf = (f(cfg[k]) for k in ("clip_range", "ent_coef", "vf_coef", "inv_batch", "clip_range_vf"))
    A, R, v = inp["adv"], inp["ret"], inp["value"]
    with np.errstate(all="ignore"):
        lp, z, sd = _lp_np32(inp["mean"], ls, inp["action"], **lp_mut)
        log_ratio = lp - inp["old_lp"]
        ratio = np.exp(log_ratio)
        lo, hi = f(1) - cr, f(1) + cr
        s1, s2 = A * ratio, A * np.minimum(np.maximum(ratio, lo), hi)
        clipped = (ratio < lo) | (ratio > hi)
        dl_dratio = np.where((s1 <= s2) | ~clipped, -A, f(0))
        vp, vgate = v, np.ones_like(v)
        if cvf > 0 and cfg["use_old_value"]:
            ov = np.roll(inp["old_value"], 1) if shift_old_value else inp["old_value"]
            dvo = v - ov
            vp = ov + np.minimum(np.maximum(dvo, -cvf), cvf)
            inside = {"closed": (dvo >= -cvf) & (dvo <= cvf), "open": (dvo > -cvf) & (dvo < cvf), "always": np.ones_like(v, dtype=bool)}[gate]
            vgate = inside.astype(f)
        dv = vp - R
        e = f(ent_sign) * ent
        dl_dlp = dl_dratio * ratio * inv + e if ent_unscaled else (dl_dratio * ratio + e) * inv
        d_mean = dl_dlp[:, None] * z / sd
        terms = np.concatenate([np.stack([-np.minimum(s1, s2), dv * dv, lp, (ratio - f(1)) - log_ratio, (np.abs(ratio - f(1)) > cr).astype(f)], 1),
                                dl_dlp[:, None] * (z * z - f(1))], 1)
        d_value = vfc * f(2) * dv * inv * vgate
    assert d_mean.dtype == d_value.dtype == terms.dtype == np.float32
    with np.errstate(all="ignore"):
        stats = _stats_tree(terms, skip_last, twice)
    return {"d_mean": P.padded(d_mean), "d_value": P.padded(d_value), "stats": P.padded(stats)}


def _ref32_loss_got(name, M, cfg):
    r32 = P.loss_refs(name, cfg)[0]
    rows = P.case_rows(M)
    stats = np.zeros(16, f)
    stats[:9] = torch.tensor(r32["terms"][rows]).sum(0).numpy()
    return {"d_mean": P.padded(r32["d_mean"][rows]), "d_value": P.padded(r32["d_value"][rows]), "stats": P.padded(stats)}


def _pad_hit(got, key):
    g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in got.items()}
    g[key][-P.PAD] = 0
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M", [("core", M) for M in P.MS] + [("tail", M) for M in P.MS if M <= 1000])
def test_teeth_head(name, M):
    inp = P.head_inputs(name, M)
    r32 = P._head_refs(name, False)[0]
    ref = {"action": P.padded(r32["action"][:M]), "log_prob": P.padded(r32["log_prob"][:M])}
    P.check_head(ref, name, M)
    P.check_head(_head_np32(inp), name, M)
    d32 = P._head_refs(name, True)[0]
    P.check_head({"action": P.padded(d32["action"][:M]), "log_prob": P.padded(d32["log_prob"][:M])}, name, M, deterministic=True)
    P.check_head(_head_np32(dict(inp, mean=inp["pre"], eps=np.zeros_like(inp["eps"]))), name, M, deterministic=True)
    rejects(P.check_head, _pad_hit(ref, "log_prob"), name, M)
    rejects(P.check_head, _head_np32(inp, rotate=True), name, M)                         # log_std[d] rotated by one dimension
    if name == "core" or M >= 63:                                                        # the 1e-6 dropped
        rejects(P.check_head, _head_np32(inp, drop_1e6=True), name, M)
    rejects(P.check_head, ref, name, M, deterministic=True)                              # the sample where the mode belongs


@pytest.mark.parametrize("name,M,vmode,inv_kind", P.LOSS_CASES + [("core", P.M_LIMIT, "on", "local")])
def test_teeth_ppo_loss(name, M, vmode, inv_kind):
    cfg = P.loss_case_cfg(M, vmode, inv_kind)
    inp = P.loss_inputs(name, M)
    ref = _ref32_loss_got(name, M, cfg)
    P.check_ppo_loss(ref, name, M, cfg)
    emu = _loss_np32(inp, cfg)
    P.check_ppo_loss(emu, name, M, cfg)
    for key in ("d_mean", "d_value", "stats"):
        rejects(P.check_ppo_loss, _pad_hit(ref, key), name, M, cfg)
    vclip = vmode in ("on", "on_ent0")

    def dead(**mut):
        rejects(P.check_ppo_loss, _loss_np32(inp, cfg, **mut), name, M, cfg)

    if M <= 16385:
        dead(skip_last=True)                                             # the last row missing from every statistic, at each M
        dead(twice=True)                                                 # a partial counted twice
    dead(rotate=True)                                                    # log_std[d] rotated by one dimension
    if M < 63:
        return
    dead(drop_1e6=True)                                                  # the 1e-6 dropped
    if name == "tail":
        dead(half_eps=True)                                              # the clamp eps halved: actions exactly +-1 move
    if cfg["ent_coef"] != 0:
        dead(ent_sign=-1.0)                                              # the entropy term's sign
        dead(ent_unscaled=True)                                          # ent_coef not scaled by inv_batch
    if vclip:
        dead(gate="always")                                              # value gate open outside the interval
        dead(gate="open")                                                # value gate closed ON the bounds
        dead(shift_old_value=True)                                       # old_value shifted by one row
        off = _loss_np32(inp, dict(cfg, use_old_value=False))            # value clipping ignored
        rejects(P.check_ppo_loss, off, name, M, cfg)
    s = ref["stats"].copy()
    if s[4] > 0:
        s[4] -= 1                                                        # the clip fraction is a count: one row off is off
        rejects(P.check_ppo_loss, dict(ref, stats=s), name, M, cfg)


def test_teeth_loss_side_outputs():
    a, b = P.padded(np.arange(16, dtype=f) * f(0.37)), P.padded(np.arange(16, dtype=f)[::-1] * f(1.13))
    before = np.full(16, f(0.5))
    acc = P.padded(before + a[:16] + b[:16])
    P.check_loss_side_outputs([a, b], acc, before, P.padded(b[5:9]))
    rejects(P.check_loss_side_outputs, [a, b], P.padded(before + b[:16]), before, P.padded(b[5:9]))       # overwritten, not accumulated
    rejects(P.check_loss_side_outputs, [a, b], acc, before, P.padded(b[4:8]))


def _adv_np32(a, mu, sigma):
    return P.padded((a - f(mu)) / (f(sigma) + f(1e-8)))


@pytest.mark.parametrize("n,count", P.ADV_CASES)
def test_teeth_adv_normalize(n, count):
    inp = P.adv_inputs(n, count)
    ref = {"out": P.padded(P.adv_normalize(inp["a"], count, F32, inp["rest"]))}
    P.check_adv_normalize(ref, inp)
    P.check_adv_normalize({"out": _adv_np32(inp["a"], *P.adv_moments(inp["a"], inp["rest"]))}, inp)
    rejects(P.check_adv_normalize, _pad_hit(ref, "out"), inp)
    x = np.concatenate([inp["a"], inp["rest"]]) if inp["rest"] is not None else inp["a"]
    if count <= 1000:                                                    # biased instead of unbiased std
        rejects(P.check_adv_normalize, {"out": _adv_np32(inp["a"], x.astype(np.float64).mean(), x.astype(np.float64).std(ddof=0))}, inp)
    if count != n:                                                       # count taken as n: the local moments
        rejects(P.check_adv_normalize, {"out": _adv_np32(inp["a"], *P.adv_moments(inp["a"]))}, inp)
        s = P.sums_of(x)                                                 # ... or the global sums over the local count
        mean = s[0] / n
        rejects(P.check_adv_normalize, {"out": _adv_np32(inp["a"], mean, math.sqrt(max((s[1] - s[0] * mean) / (n - 1), 0.0)))}, inp)
    skipped = ref["out"].copy()                                          # the last element not written
    skipped[n - 1] = P.SENT_F
    rejects(P.check_adv_normalize, {"out": skipped}, inp)


@pytest.mark.parametrize("n_seg,seg_len,count", P.SEG_CASES)
def test_teeth_adv_segments(n_seg, seg_len, count):
    inp = P.adv_segment_inputs(n_seg, seg_len, count)
    ref = {"out": P.padded(P.adv_normalize_segments(inp["a"], count, F32, inp["rest"]))}
    P.check_adv_segments(ref, inp)
    assert (inp["constant_segment"] is not None) == (count == seg_len and n_seg > 1)
    mom = [P.adv_moments(inp["a"][k], None if inp["rest"] is None else inp["rest"][k]) for k in range(n_seg)]
    if n_seg > 1:                                                        # segment k normalised with segment k - 1's sums
        bad = np.stack([(inp["a"][k] - f(mom[k - 1][0])) / (f(mom[k - 1][1]) + f(1e-8)) for k in range(n_seg)])
        rejects(P.check_adv_segments, {"out": P.padded(bad)}, inp)
    if inp["constant_segment"] is not None:                              # no clamp of a variance that rounds below zero
        bad = P.adv_normalize_segments(inp["a"], count, F32, inp["rest"])
        bad[inp["constant_segment"]] = np.nan
        rejects(P.check_adv_segments, {"out": P.padded(bad)}, inp)


def _rollout_post_np32(inp, multiply=False, terminated=False, byte_is_one=False):
    g = f(P.f32(inp["gamma"]))
    dn = (inp["done"] == 1) if byte_is_one else (inp["done"] != 0)
    fl = (inp["ep_flags"] & P.EP_TRUNCATED) != 0
    which = dn & ~fl if terminated else dn & fl
    with np.errstate(all="ignore"):
        if multiply:                                                     # the kernel as it was: every row through the add
            r = inp["reward"] + (g * inp["terminal_value"]) * which.astype(f)
        else:
            r = np.where(which, inp["reward"] + g * inp["terminal_value"], inp["reward"])
    return {"reward_out": P.padded(r.astype(f)), "next_start": P.padded(dn.astype(f))}


@pytest.mark.parametrize("N", P.ROWS)
def test_teeth_rollout_post(N):
    for shift in (0, 7):
        inp = P.rollout_inputs(N, shift)
        r32 = P.rollout_post(inp["reward"], inp["done"], inp["ep_flags"], inp["terminal_value"], inp["gamma"], F32)
        P.check_rollout_post({k: P.padded(v) for k, v in r32.items()}, inp)
        P.check_rollout_post(_rollout_post_np32(inp), inp)
        if N < 63:
            continue
        seen = set(zip(inp["done"][:48].tolist(), inp["ep_flags"][:48].tolist())) & set(zip(inp["done"][-48:].tolist(), inp["ep_flags"][-48:].tolist()))
        assert seen == set(P.TRUTH) and len(P.TRUTH) == 48
        keep = ~inp["truncated"]
        assert (np.signbit(inp["reward"]) & (inp["reward"] == 0) & keep).any() and not np.isfinite(inp["terminal_value"][keep]).any()
        rejects(P.check_rollout_post, _rollout_post_np32(inp, multiply=True), inp)       # NaN rewards on rows that did not truncate
        tame = dict(inp, terminal_value=np.where(keep, f(1.5), inp["terminal_value"]))
        rejects(P.check_rollout_post, _rollout_post_np32(tame, multiply=True), tame)     # -0.0 reward turned to +0.0
        rejects(P.check_rollout_post, _rollout_post_np32(tame, terminated=True), tame)   # bootstrap on terminated (not truncated) rows
        rejects(P.check_rollout_post, _rollout_post_np32(inp, byte_is_one=True), inp)    # done read as == 1


def _collect_got(inp, r32, order, capacity, before=None):
    w0 = inp["obs0"].shape[1]
    w1 = 0 if inp.get("obs1") is None else inp["obs1"].shape[1]
    idx, rows0, rows1 = P.blank((capacity,), np.int32), P.blank((capacity, w0)), P.blank((capacity, max(w1, 1)))
    ent = sorted(r32["entries"])
    ent = [ent[j] for j in order(len(ent))]
    start = 0
    if before is not None:
        idx, rows0, rows1, start = before["idx_list"].copy(), before["rows0"].copy(), before["rows1"].copy(), before["cursor"]
    for j, (at, o0, o1) in enumerate(ent):
        if start + j < capacity:
            idx[start + j] = at
            rows0[(start + j) * w0:(start + j + 1) * w0] = np.array(o0, dtype=np.uint32).view(f)
            if w1:
                rows1[(start + j) * w1:(start + j + 1) * w1] = np.array(o1, dtype=np.uint32).view(f)
    return {"reward_out": P.padded(r32["reward_out"]), "next_start": P.padded(r32["next_start"]), "stat": P.padded(r32["stat"]),
            "cursor": start + len(ent), "idx_list": idx, "rows0": rows0, "rows1": rows1 if w1 else None}


@pytest.mark.parametrize("N", P.ROWS)
def test_teeth_rollout_post_collect(N):
    inp = dict(P.rollout_inputs(N), flat_base=5 * N, capacity=N + 3)
    r32 = P.rollout_post_collect(inp["reward"], inp["done"], inp["ep_flags"], inp["obs0"], inp["obs1"], inp["flat_base"], inp["ep_return"],
                                 inp["ep_length"], inp["stat"], F32)
    n_tr = int(inp["truncated"].sum())
    assert len(r32["entries"]) == n_tr >= 1
    for order in (lambda n: range(n), lambda n: range(n - 1, -1, -1)):                    # the cursor order is free
        P.check_collect(_collect_got(inp, r32, order, inp["capacity"]), inp)
    got = _collect_got(inp, r32, lambda n: range(n), inp["capacity"])
    rejects(P.check_collect, dict(got, cursor=got["cursor"] - 1), inp)
    wrong_base = dict(got, idx_list=np.where(got["idx_list"] != P.SENT_I, got["idx_list"] - inp["flat_base"], got["idx_list"]).astype(np.int32))
    rejects(P.check_collect, wrong_base, inp)                                             # flat_base forgotten
    bad = dict(got, rows0=got["rows0"].copy())
    bad["rows0"][0] = f(9.75)
    rejects(P.check_collect, bad, inp)                                                    # an observation row that is nobody's
    st = r32["stat"].copy()
    st[N - 1] = inp["stat"][N - 1]
    if inp["done"][N - 1]:
        rejects(P.check_collect, dict(got, stat=P.padded(st)), inp)                       # the last agent's accumulators not advanced
    # the scatter over the collected list gives vf_rollout_post's rewards, bit for bit, whatever the list order
    ent = sorted(r32["entries"], reverse=True)
    idx = np.array([e[0] for e in ent], dtype=np.int32) - inp["flat_base"]
    sc = P.bootstrap_scatter(idx, inp["terminal_value"][idx], inp["gamma"], r32["reward_out"], F32)
    P.exact("scatter", sc, P.rollout_post(inp["reward"], inp["done"], inp["ep_flags"], inp["terminal_value"], inp["gamma"], F32)["reward_out"])
    # the second step of the GPU test (shift 7), and a single observation field (w1 = 0, no accumulators)
    for two in (dict(P.rollout_inputs(N, 7), flat_base=N, capacity=2 * N + 6), dict(P.rollout_inputs(N, 7, w0=5, w1=0), flat_base=0, capacity=N)):
        r2 = P.rollout_post_collect(two["reward"], two["done"], two["ep_flags"], two["obs0"], two["obs1"], two["flat_base"], two["ep_return"],
                                    two["ep_length"], two["stat"], F32)
        P.check_collect(_collect_got(two, r2, lambda n: range(n), two["capacity"]), two)
    if N >= 63:                                                                           # capacity short of the truncated rows
        short = dict(inp, capacity=n_tr - 1)
        P.check_collect(_collect_got(short, r32, lambda n: range(n), n_tr - 1), short)
        over = _collect_got(short, r32, lambda n: range(n), n_tr - 1)
        over["idx_list"][n_tr - 1] = 0                                                    # the entry past capacity stored: the pad is hit
        rejects(P.check_collect, over, short)


@pytest.mark.parametrize("N", P.EPISODE_N)
def test_teeth_episode_stats(N):
    acc0 = np.array([3.0, -41.5, 977.0, 2.0])
    inp1 = P.episode_inputs(N, 1)                                                         # the GPU test's second call
    P.check_episode_stats(P.episode_stats(inp1["done"], inp1["ep_return"], inp1["ep_length"], inp1["ep_flags"], acc0), inp1, acc0)
    inp = P.episode_inputs(N)
    want = P.episode_stats(inp["done"], inp["ep_return"], inp["ep_length"], inp["ep_flags"], acc0)
    P.check_episode_stats(want, inp, acc0)
    assert inp["done"][N - 1] == 255 and (N < 3 or set(inp["done"].tolist()) == {0, 1, 255})
    for k in range(4):                                                                    # agent N - 1 skipped: each of the four sums
        bad = want.copy()
        bad[k] -= (1.0, float(inp["ep_return"][N - 1]), float(inp["ep_length"][N - 1]), 1.0)[k]
        rejects(P.check_episode_stats, bad, inp, acc0)
    if N > 3:                                                                             # done read as == 1
        one = dict(inp, done=(inp["done"] == 1).astype(np.uint8))
        rejects(P.check_episode_stats, P.episode_stats(one["done"], inp["ep_return"], inp["ep_length"], inp["ep_flags"], acc0), inp, acc0)
    rejects(P.check_episode_stats, want - acc0, inp, acc0)                                # overwritten, not accumulated


@pytest.mark.parametrize("kind", ["perm", "repeats"])
@pytest.mark.parametrize("rows", P.GATHER_ROWS)
def test_teeth_gather(rows, kind):
    inp = P.gather_inputs(rows, kind)
    ref = [P.padded(P.gather_rows(s, inp["perm"])) for s in inp["src"]]
    P.check_gather(ref, inp)
    assert np.unique(np.concatenate([P._bits(s).reshape(-1) for s in inp["src"]])).size == rows * sum(P.GATHER_WIDTHS), "every element names its origin"
    if rows == 1 or rows > 257:                                          # the mutants at the small sizes (a Python loop per row)
        return
    assert (np.unique(inp["perm"]).size == rows) == (kind == "perm")
    # the row stride taken from the neighbouring field's width
    bad = []
    for i, s in enumerate(inp["src"]):
        w, wn = s.shape[1], P.GATHER_WIDTHS[(i + 1) % 8]
        flat = np.concatenate([s.reshape(-1), np.zeros(rows * 256, f)])
        bad.append(P.padded(np.stack([flat[p * wn:p * wn + w] for p in inp["perm"]])))
    for i in range(8):
        rejects(P.check_gather, ref[:i] + [bad[i]] + ref[i + 1:], inp)
    rejects(P.check_gather, [P.padded(s) for s in inp["src"]], inp)                       # the index list ignored
