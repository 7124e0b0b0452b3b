"""PPO's head, loss and buffer kernels (vf_ppo.hip, vf_ppo_device.hpp), each entry point on its own through the C ABI, against the
plain references of tests/_ppo_glue_ref.py: fp64 is the truth, the float32 run is the reference's own arithmetic.

  * head and loss, per row (action, log_prob, d_mean, d_value):  max|got - ref64| <= max(4 E32, 2^-22 max|ref64|) with E32 =
    max|ref32 - ref64| POOLED over the master table the case is a row-prefix of (core: 16 385 rows, tail: 1 000 rows, each its own
    E32), exact zeros where a clip switches the gradient off; the nine statistics within 4 sum|t32 - t64| + 32 * 2^-24 sum|t64| of
    the fp64 sum, the clip count equal; stats_accum and d_log_std_out bit for bit;
  * advantage normalisation: per element within 2^-23 (4 |a - mu| + |mu|) / (sigma + 1e-8) of fp64; a constant segment gives zeros;
  * rollout_post, rollout_post_collect, bootstrap_scatter, gather_rows: bit identity with the float32 reference; vf_episode_stats:
    counts equal, fp64 sums within N 2^-53 sum|x|;
  * every output buffer is 64 elements longer than needed and sentinel-filled: the pad must come back untouched.
tests/test_ppo_glue_host.py shows on these very inputs that the float32 reference and a numpy restatement of the kernel's operation
order pass every comparator and that the listed mutants fail.  Nothing fused is touched here: vf_ppo_update and the roll-out kernels
are pinned transitively by the existing "equals the separate launches" tests (test_ppo_gpu.py), whose root these tests now hold.

Every case prints ``PPOGLUE <op> <array> err=... scale=... bound=...`` before it asserts.  Observed on an MI355X, the largest
err / scale (and err / bound) over all cases of an operation -- measured values, recorded after the fact; no bound is taken from them:
(scale: the table's E32 for the per-row arrays, sum|t32 - t64| for a statistic, one rounding of mu and of the result for the
normalisation, 2^-53 sum|x| for the fp64 sums; [core] / [tail]: the master table, over all sizes, configurations and inv_batch)
  operation                array       err/scale (err/bound)
  head_eps[core]           action      1.02  (0.254)
  head_eps[core]           log_prob    1.07  (0.266)
  head_eps[tail]           action      1.00  (0.250)
  head_eps[tail]           log_prob    1.00  (0.250)
  head_det[core]           action      2.58  (0.328)
  head_det[core]           log_prob    1.04  (0.259)
  head_det[tail]           action      1.72  (0.217)
  head_det[tail]           log_prob    1.00  (0.250)
  ppo_loss[core]           d_mean      1.14  (0.286)
  ppo_loss[core]           d_value     1.00  (0.250)
  ppo_loss[core]           stats0      0.66  (0.141)
  ppo_loss[core]           stats1      2.16  (0.044)
  ppo_loss[core]           stats2      0.81  (0.060)
  ppo_loss[core]           stats3      0.58  (0.143)
  ppo_loss[core]           stats4      equal (0) in all 73 cases
  ppo_loss[core]           stats5      0.66  (0.141)
  ppo_loss[core]           stats6      0.69  (0.151)
  ppo_loss[core]           stats7      1.00  (0.237)
  ppo_loss[core]           stats8      0.63  (0.135)
  ppo_loss[tail]           d_mean      1.00  (0.250)
  ppo_loss[tail]           d_value     1.00  (0.250)
  ppo_loss[tail]           stats0      0.01  (0.002)
  ppo_loss[tail]           stats1      0.29  (0.005)
  ppo_loss[tail]           stats2      0.67  (0.111)
  ppo_loss[tail]           stats3      0.13  (0.032)
  ppo_loss[tail]           stats4      equal (0) in all 8 cases
  ppo_loss[tail]           stats5      0.01  (0.002)
  ppo_loss[tail]           stats6      0.13  (0.032)
  ppo_loss[tail]           stats7      0.17  (0.042)
  ppo_loss[tail]           stats8      0.07  (0.018)
  adv_normalize[phase2]    out         1.64  (0.254)
  adv_normalize[phase0+1]  out         1.80  (0.264)
  adv_segments[phase0+1]   out         1.81  (0.462)
  adv_segments[phase2]     out         1.76  (0.325)
  episode_stats            episodes    equal (0) in all 16 cases
  episode_stats            successes   equal (0) in all 16 cases
  episode_stats            return_sum  0.00  (0.000)
  episode_stats            length_sum  0.00  (0.000)
  stats_accum, d_log_std_out, old_value NULL against value clipping off, rollout_post, rollout_post_collect (rewards, episode_start,
  fp32 accumulators, the list as a set), bootstrap_scatter against vf_rollout_post, gather_rows, segment k under changed
  neighbours, phase 2 against phases 0 + 1 of the segmented normalisation: bit identical (0)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _ppo_glue_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1


def L():
    from visfly_amd import _lib
    return _lib, _lib.lib()


def st():
    from visfly_amd import _lib
    return _lib.current_stream(torch.device(DEV))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def host(*ts):
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in ts]
    return out[0] if len(out) == 1 else out


def ptr(t):
    return None if t is None else t.data_ptr()


def report(op, res):
    for k, (err, scale, bound) in res.items():
        print(f"PPOGLUE {op} {k} err={err:.3e} scale={scale:.3e} bound={bound:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# the head
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M", [("core", M) for M in P.MS] + [("tail", M) for M in P.MS if M <= 1000])
def test_head_sample_eps(name, M):
    _lib, lib = L()
    inp = P.head_inputs(name, M)
    mean, ls, eps = dev(inp["mean"]), dev(inp["log_std"]), dev(inp["eps"])
    action, lp = dev(P.blank((M, 4))), dev(P.blank((M,)))
    _lib.check(lib.vf_head_sample_eps(mean.data_ptr(), ls.data_ptr(), eps.data_ptr(), action.data_ptr(), lp.data_ptr(), M, st()))
    g_a, g_lp = host(action, lp)
    report(f"head_eps[{name}]", P.check_head({"action": g_a, "log_prob": g_lp}, name, M))


@pytest.mark.parametrize("name,M", [("core", M) for M in P.MS] + [("tail", 1000)])
def test_head_sample_deterministic(name, M):
    _lib, lib = L()
    inp = P.head_inputs(name, M)
    mean, ls = dev(inp["pre"]), dev(inp["log_std"])
    action, lp = dev(P.blank((M, 4))), dev(P.blank((M,)))
    _lib.check(lib.vf_head_sample(mean.data_ptr(), ls.data_ptr(), action.data_ptr(), lp.data_ptr(), M, 77, 5, 1, st()))
    g_a, g_lp = host(action, lp)
    report(f"head_det[{name}]", P.check_head({"action": g_a, "log_prob": g_lp}, name, M, deterministic=True))


def test_head_sample_eps_alignment():
    _lib, lib = L()
    M = 64
    mean, eps, action = (torch.zeros(M * 4 + 4, device=DEV) for _ in range(3))
    ls, lp = torch.zeros(4, device=DEV), torch.zeros(M, device=DEV)
    for off in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):
        assert lib.vf_head_sample_eps(mean.data_ptr() + off[0], ls.data_ptr(), eps.data_ptr() + off[1], action.data_ptr() + off[2],
                                      lp.data_ptr(), M, st()) == EINVAL
    _lib.check(lib.vf_head_sample_eps(mean.data_ptr(), ls.data_ptr(), eps.data_ptr(), action.data_ptr(), lp.data_ptr(), M, st()))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------------------------------
def _loss_call(_lib, lib, d, M, cfg, stats_accum=None, d_log_std_out=None, rows=None):
    """one vf_ppo_loss launch over the device inputs `d`; -> (rc, padded host d_mean, d_value, stats)"""
    rows = M if rows is None else rows
    d_mean, d_value, stats = dev(P.blank((rows, 4))), dev(P.blank((rows,))), dev(P.blank((16,)))
    scratch = torch.zeros(16 * 1024, device=DEV)
    c = _lib.PpoLossCfg(cfg["clip_range"], cfg["ent_coef"], cfg["vf_coef"], cfg["inv_batch"], ptr(d_log_std_out), ptr(stats_accum),
                        d["old_value"].data_ptr() if cfg["use_old_value"] else None, cfg["clip_range_vf"], 0, None, None, None)
    rc = lib.vf_ppo_loss(d["mean"].data_ptr(), d["value"].data_ptr(), d["log_std"].data_ptr(), d["action"].data_ptr(), d["old_lp"].data_ptr(),
                         d["adv"].data_ptr(), d["ret"].data_ptr(), d_mean.data_ptr(), d_value.data_ptr(), stats.data_ptr(), M, C.byref(c),
                         scratch.data_ptr(), st())
    g = host(d_mean, d_value, stats)
    return rc, {"d_mean": g[0], "d_value": g[1], "stats": g[2]}


def _loss_case(name, M, inv_kind):
    """the four configurations of one (table, M, inv_batch): off, on, old_value NULL (off by contract: the off case bit for bit), and
    on with ent_coef = 0; then the accumulator and the log_std copy over two calls"""
    _lib, lib = L()
    d = {k: dev(v) for k, v in P.loss_inputs(name, M).items()}
    got = {}
    for vmode in P.VMODES:
        cfg = P.loss_case_cfg(M, vmode, inv_kind)
        rc, got[vmode] = _loss_call(_lib, lib, d, M, cfg)
        _lib.check(rc)
        report(f"ppo_loss[{name},{vmode}]", P.check_ppo_loss(got[vmode], name, M, cfg))
    for k in ("d_mean", "d_value", "stats"):
        P.exact(f"{k}: clip_range_vf > 0 with old_value NULL against value clipping off", got["null_old_value"][k], got["off"][k])
    before = (np.arange(16) * 0.25 - 1.0).astype(np.float32)
    accum, d_ls = dev(P.padded(before)), dev(P.blank((4,)))
    calls = []
    for vmode in ("on", "off"):
        rc, g = _loss_call(_lib, lib, d, M, P.loss_case_cfg(M, vmode, inv_kind), stats_accum=accum, d_log_std_out=d_ls)
        _lib.check(rc)
        P.exact("stats with the side outputs on", g["stats"], got[vmode]["stats"])
        calls.append(g["stats"])
    P.check_loss_side_outputs(calls, host(accum), before, host(d_ls))


@pytest.mark.parametrize("inv_kind", ["local", "global"])
@pytest.mark.parametrize("M", P.MS)
def test_ppo_loss_core(M, inv_kind):
    _loss_case("core", M, inv_kind)


@pytest.mark.parametrize("inv_kind", ["local", "global"])
def test_ppo_loss_tail(inv_kind):
    _loss_case("tail", 1000, inv_kind)


def test_ppo_loss_row_limit():
    """262 144 rows (the scratch contract's limit: 1024 partials, 16 lane-strided adds) pass; one more returns VF_EINVAL untouched"""
    _lib, lib = L()
    M = P.M_LIMIT
    d = {k: dev(v) for k, v in P.loss_inputs("core", M).items()}
    cfg = P.loss_case_cfg(M, "on", "local")
    rc, got = _loss_call(_lib, lib, d, M, cfg)
    _lib.check(rc)
    report("ppo_loss[core,on,262144]", P.check_ppo_loss(got, "core", M, cfg))
    rc, got = _loss_call(_lib, lib, d, M + 1, cfg, rows=M)
    assert rc == EINVAL
    for k, shape in (("d_mean", (M, 4)), ("d_value", (M,)), ("stats", (16,))):
        assert np.all(P._bits(got[k]) == P._bits(P.blank(shape))), f"{k}: written by a refused call"


# ---------------------------------------------------------------------------------------------------------------------------
# advantage normalisation
# ---------------------------------------------------------------------------------------------------------------------------
def _edit_sums(sums, rest, n_seg):
    """what an all-reduce does between phase 0 and phase 1: the other ranks' fp64 sums are added to this rank's"""
    if rest is not None:
        extra = np.concatenate([P.sums_of(rest[k]) for k in range(n_seg)]) if n_seg else P.sums_of(rest)
        sums[:extra.size] += dev(extra)


@pytest.mark.parametrize("n,count", P.ADV_CASES)
def test_adv_normalize(n, count):
    _lib, lib = L()
    inp = P.adv_inputs(n, count)
    a = dev(inp["a"])
    scratch = torch.zeros(2 * 1024, device=DEV)
    assert lib.vf_adv_normalize(a.data_ptr(), a.data_ptr(), n, 1, None, scratch.data_ptr(), 2, st()) == EINVAL        # count < 2
    if count == n:                                                       # both phases in one call, the sums in the scratch
        out = dev(P.blank((n,)))
        _lib.check(lib.vf_adv_normalize(a.data_ptr(), out.data_ptr(), n, count, None, scratch.data_ptr(), 2, st()))
        report("adv_normalize[phase2]", P.check_adv_normalize({"out": host(out)}, inp))
    out, sums = dev(P.blank((n,))), dev(P.padded(np.zeros(2)))
    _lib.check(lib.vf_adv_normalize(a.data_ptr(), out.data_ptr(), n, count, sums.data_ptr(), scratch.data_ptr(), 0, st()))
    assert np.all(P._bits(host(out)) == P._bits(P.blank((n,)))), "phase 0 wrote the output"
    _edit_sums(sums, inp["rest"], 0)
    _lib.check(lib.vf_adv_normalize(a.data_ptr(), out.data_ptr(), n, count, sums.data_ptr(), scratch.data_ptr(), 1, st()))
    P.body("sums", host(sums), (2,))
    report("adv_normalize[phase0+1]", P.check_adv_normalize({"out": host(out)}, inp))


@pytest.mark.parametrize("n_seg,seg_len,count", P.SEG_CASES)
def test_adv_normalize_segments(n_seg, seg_len, count):
    _lib, lib = L()
    inp = P.adv_segment_inputs(n_seg, seg_len, count)
    a = dev(inp["a"])
    shape = inp["a"].shape
    assert lib.vf_adv_normalize_segments(a.data_ptr(), a.data_ptr(), n_seg, seg_len, 1, a.data_ptr(), 2, st()) == EINVAL

    def run(a_dev, rest, one_call):
        out, sums = dev(P.blank(shape)), dev(P.padded(np.zeros(2 * n_seg)))
        if one_call:
            _lib.check(lib.vf_adv_normalize_segments(a_dev.data_ptr(), out.data_ptr(), n_seg, seg_len, count, sums.data_ptr(), 2, st()))
        else:
            _lib.check(lib.vf_adv_normalize_segments(a_dev.data_ptr(), out.data_ptr(), n_seg, seg_len, count, sums.data_ptr(), 0, st()))
            _edit_sums(sums, rest, n_seg)
            _lib.check(lib.vf_adv_normalize_segments(a_dev.data_ptr(), out.data_ptr(), n_seg, seg_len, count, sums.data_ptr(), 1, st()))
        g_out, g_sums = host(out, sums)
        P.body("sums", g_sums, (2 * n_seg,))
        return g_out

    got = run(a, inp["rest"], False)
    report("adv_segments[phase0+1]", P.check_adv_segments({"out": got}, inp))
    if count == seg_len:
        one = run(a, None, True)
        report("adv_segments[phase2]", P.check_adv_segments({"out": one}, inp))
        P.exact("phase 2 against phases 0, 1", one, got)
    if n_seg > 1:                                                        # segment k's output depends on segment k only
        k = n_seg // 2
        other = inp["a"] * np.float32(-3.0) + np.float32(1.0)
        other[k] = inp["a"][k]
        rest = None if inp["rest"] is None else np.concatenate([inp["rest"][:k] * np.float32(2.0), inp["rest"][k:k + 1], inp["rest"][k + 1:] + np.float32(1.0)])
        again = P.body("out", run(dev(other), rest, False), shape)
        P.exact(f"segment {k} with every other segment changed", again[k], P.body("out", got, shape)[k])


# ---------------------------------------------------------------------------------------------------------------------------
# the epoch's row gather
# ---------------------------------------------------------------------------------------------------------------------------
def _gather(_lib, lib, inp, widths=None):
    rows = inp["perm"].size
    src = [dev(s) for s in inp["src"]]
    dst = [dev(P.blank(s.shape)) for s in inp["src"]]
    perm = dev(inp["perm"])
    fields = _lib.GatherFields()
    fields.n_fields = len(src)
    for i, (s, d_) in enumerate(zip(src, dst)):
        fields.width[i] = inp["src"][i].shape[1] if widths is None else widths[i]
        fields.src[i], fields.dst[i] = s.data_ptr(), d_.data_ptr()
    rc = lib.vf_gather_rows(C.byref(fields), perm.data_ptr(), rows, st())
    return rc, host(*dst) if len(dst) > 1 else [host(*dst)]


@pytest.mark.parametrize("kind", ["perm", "repeats"])
@pytest.mark.parametrize("rows", P.GATHER_ROWS)
def test_gather_rows(rows, kind):
    _lib, lib = L()
    inp = P.gather_inputs(rows, kind)
    rc, got = _gather(_lib, lib, inp)
    _lib.check(rc)
    P.check_gather(got, inp)


def test_gather_rows_past_the_grid_cap():
    """width 256, 65 537 rows: one row per block, one block more than the grid holds"""
    _lib, lib = L()
    inp = P.gather_inputs(65537, "perm", widths=(256,))
    rc, got = _gather(_lib, lib, inp)
    _lib.check(rc)
    P.check_gather(got, inp)


def test_gather_rows_argument_checks():
    _lib, lib = L()
    inp = P.gather_inputs(65, "perm", widths=(4, 256))
    for widths in ((4, 0), (4, 257), (0, 256)):
        rc, got = _gather(_lib, lib, inp, widths=widths)
        assert rc == EINVAL
        for g, s in zip(got, inp["src"]):
            assert np.all(P._bits(g) == P._bits(P.blank(s.shape))), "written by a refused call"


# ---------------------------------------------------------------------------------------------------------------------------
# roll-out bookkeeping
# ---------------------------------------------------------------------------------------------------------------------------
def _rollout_post(_lib, lib, inp):
    N = inp["reward"].size
    rew, done, flags, tv = (dev(inp[k]) for k in ("reward", "done", "ep_flags", "terminal_value"))
    out, nxt = dev(P.blank((N,))), dev(P.blank((N,)))
    _lib.check(lib.vf_rollout_post(rew.data_ptr(), done.data_ptr(), flags.data_ptr(), tv.data_ptr(), inp["gamma"], out.data_ptr(),
                                   nxt.data_ptr(), N, st()))
    g = host(out, nxt)
    return {"reward_out": g[0], "next_start": g[1]}


@pytest.mark.parametrize("N", P.ROWS)
def test_rollout_post(N):
    """done bytes 0 / 1 / 255 against every combination of the ep_flags bits, rewards of -0.0, and a non-finite terminal_value on
    every row that does not truncate: those rewards keep their bits"""
    _lib, lib = L()
    for shift in (0, 7):
        inp = P.rollout_inputs(N, shift)
        P.check_rollout_post(_rollout_post(_lib, lib, inp), inp)


class _List:
    """the compact list of truncated rows and its device cursor"""

    def __init__(self, capacity, w0, w1):
        self.capacity, self.w1 = capacity, w1
        self.cursor = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.idx, self.rows0 = dev(P.blank((capacity,), np.int32)), dev(P.blank((capacity, w0)))
        self.rows1 = dev(P.blank((capacity, w1))) if w1 else None

    def read(self):
        g = host(self.cursor, self.idx, self.rows0)
        return {"cursor": int(g[0][0]), "idx_list": g[1], "rows0": g[2], "rows1": host(self.rows1) if self.w1 else None}


def _collect(_lib, lib, inp, lst, reward_out, stat):
    N = inp["reward"].size
    w0 = inp["obs0"].shape[1]
    rew, done, flags, obs0, ret, length = (dev(inp[k]) for k in ("reward", "done", "ep_flags", "obs0", "ep_return", "ep_length"))
    obs1 = dev(inp["obs1"]) if lst.w1 else None
    nxt = dev(P.blank((N,)))
    _lib.check(lib.vf_rollout_post_collect(rew.data_ptr(), done.data_ptr(), flags.data_ptr(), reward_out, nxt.data_ptr(), obs0.data_ptr(),
                                           ptr(obs1), w0, lst.w1, lst.cursor.data_ptr(), lst.capacity, lst.idx.data_ptr(), lst.rows0.data_ptr(),
                                           ptr(lst.rows1), inp["flat_base"], N, ret.data_ptr(), length.data_ptr(), ptr(stat), st()))
    return host(nxt)


@pytest.mark.parametrize("N", P.ROWS)
def test_rollout_post_collect_and_scatter(N):
    """two steps appended to one list (flat_base = t N, step 1 behind step 0, the accumulators carried over), then the scatter: the
    rewards of the two steps are vf_rollout_post's, bit for bit"""
    _lib, lib = L()
    steps = [dict(P.rollout_inputs(N, shift), flat_base=t * N, capacity=2 * N + 6) for t, shift in enumerate((0, 7))]
    lst = _List(2 * N + 6, 13, 3)
    flat = dev(P.blank((2 * N,)))
    stat = dev(P.padded(steps[0]["stat"]))
    entries, cursor, stat_before = frozenset(), 0, steps[0]["stat"]
    for t, inp in enumerate(steps):
        inp = dict(inp, stat=stat_before)
        nxt = _collect(_lib, lib, inp, lst, flat.data_ptr() + 4 * t * N, stat)
        g_flat = host(flat)
        step_out = np.concatenate([g_flat[t * N:(t + 1) * N], np.full(P.PAD, P.SENT_F, dtype=np.float32)])
        got = dict(lst.read(), reward_out=step_out, next_start=nxt, stat=host(stat))
        P.check_collect(got, inp, entries_before=entries, cursor_before=cursor)
        entries = entries | P.rollout_post_collect(inp["reward"], inp["done"], inp["ep_flags"], inp["obs0"], inp["obs1"], inp["flat_base"],
                                                   inp["ep_return"], inp["ep_length"], None, P.F32)["entries"]
        cursor, stat_before = got["cursor"], P.body("stat", got["stat"], (N, 4)).copy()
    P.body("rewards_flat", host(flat), (2 * N,))
    # the caller evaluates the value head once over the collected rows: here the terminal values of the listed rewards
    got = lst.read()
    idx = got["idx_list"][:cursor]
    tv_all = np.concatenate([s["terminal_value"] for s in steps])
    values = dev(tv_all[idx])
    before = host(flat).copy()
    _lib.check(lib.vf_bootstrap_scatter(lst.idx.data_ptr(), values.data_ptr(), 0, 0.99, flat.data_ptr(), st()))           # count = 0: a no-op
    P.exact("rewards_flat after a scatter of nothing", host(flat), before)
    _lib.check(lib.vf_bootstrap_scatter(lst.idx.data_ptr(), values.data_ptr(), cursor, steps[0]["gamma"], flat.data_ptr(), st()))
    direct = np.concatenate([P.body("reward_out", _rollout_post(_lib, lib, s)["reward_out"], (N,)) for s in steps])
    P.exact("scatter against vf_rollout_post", P.body("rewards_flat", host(flat), (2 * N,)), direct)
    want = np.concatenate([P.rollout_post(s["reward"], s["done"], s["ep_flags"], s["terminal_value"], s["gamma"], P.F32)["reward_out"] for s in steps])
    P.exact("scatter against the reference", direct, want)
    ref_sc = P.bootstrap_scatter(idx, tv_all[idx], steps[0]["gamma"], P.body("rewards_flat", before, (2 * N,)), P.F32)
    P.exact("scatter against bootstrap_scatter", direct, ref_sc)


@pytest.mark.parametrize("N", [63, 257, 1000])
def test_rollout_post_collect_short_capacity_and_single_observation(N):
    _lib, lib = L()
    # capacity one short of the truncated rows: the cursor counts them all, nothing beyond capacity is stored, the pads are intact
    inp = dict(P.rollout_inputs(N), flat_base=3)
    inp["capacity"] = int(inp["truncated"].sum()) - 1
    lst = _List(inp["capacity"], 13, 3)
    out, stat = dev(P.blank((N,))), dev(P.padded(inp["stat"]))
    nxt = _collect(_lib, lib, inp, lst, out.data_ptr(), stat)
    got = dict(lst.read(), reward_out=host(out), next_start=nxt, stat=host(stat))
    assert got["cursor"] == inp["capacity"] + 1
    P.check_collect(got, inp)
    # w1 = 0 with a NULL second observation, no episode accumulators
    inp = dict(P.rollout_inputs(N, 7, w0=5, w1=0), flat_base=0, capacity=N, stat=None)
    lst = _List(N, 5, 0)
    out = dev(P.blank((N,)))
    nxt = _collect(_lib, lib, inp, lst, out.data_ptr(), None)
    P.check_collect(dict(lst.read(), reward_out=host(out), next_start=nxt), inp)


@pytest.mark.parametrize("N", P.EPISODE_N)
def test_episode_stats(N):
    _lib, lib = L()
    before = np.array([3.0, -41.5, 977.0, 2.0])
    acc = dev(P.padded(before))
    for call in range(2):                                                # the second call accumulates on the first
        inp = P.episode_inputs(N, call)
        done, ret, length, flags = (dev(inp[k]) for k in ("done", "ep_return", "ep_length", "ep_flags"))
        _lib.check(lib.vf_episode_stats(done.data_ptr(), ret.data_ptr(), length.data_ptr(), flags.data_ptr(), acc.data_ptr(), N, st()))
        got = P.body("acc4", host(acc), (4,)).copy()
        report("episode_stats", P.check_episode_stats(got, inp, before))
        before = got
