"""The glue kernels of the first-order trainers (vf_shac.hip, vf_bptt_ops.hip, vf_optim.hip), each on its own, against the plain
references of tests/_glue_ref.py: fp64 is the truth, the float32 run is the reference's own arithmetic.

  * the accumulate kernels, and the zeros / head selection of the twin-Q gradient: bit identity with the float32 reference;
  * everything else: max|got - ref64| <= max(4 max|ref32 - ref64|, 2^-22 max|ref64|) per output array, the bound computed from
    the references alone (tests/test_trainer_glue_host.py shows that the float32 reference passes and that the listed mutants fail
    on these very inputs);
  * every output buffer is 64 elements longer than needed and sentinel-filled: the pad must come back untouched.
Sizes sit around the wave (64) and block (256) edges and at every size where the code takes another path: 16 385 rows leave the
twin-Q fold 65 partials, n > 2^20 is vf_sumsq's two-launch form, n > 262 144 is k_adam's grid-stride tail.

Every case prints ``GLUE <op> <array> err=... e32=... bound=...`` (err = max|got - ref64|, e32 = max|ref32 - ref64|) before it
asserts.  Observed on an MI355X, the largest err / e32 (and err / bound) over all cases of an operation:
  operation    array       err/e32 (err/bound)
  head_fwd     action      1.69  (0.370)
  head_bwd     d_mu        1.00  (0.250)
  head_bwd     d_log_std   1.00  (0.250)
  reparam_fwd  action      1.81  (0.426)
  reparam_bwd  d_mean      1.00  (0.241)
  reparam_bwd  g_log_std   1.00  (0.250)
  twin_q_loss  loss        1.00  (0.180)
  twin_q_loss  dq0         1.47  (0.349)   [2 of 10 cases have e32 = 0; largest err there 0.0e+00]
  twin_q_loss  dq1         1.96  (0.445)   [2 of 10 cases have e32 = 0; largest err there 0.0e+00]
  polyak       target      1.00  (0.250)   [8 of 12 cases have e32 = 0; largest err there 0.0e+00]
  sumsq        sumsq       1.00  (0.200)   [4 of 11 cases have e32 = 0; largest err there 0.0e+00]
  adam         p           1.03  (0.258)
  adam         m           1.39  (0.347)
  adam         v           1.00  (0.250)
  the three accumulate kernels, ep_done, next_value, the zeros and the head selection of dq0 / dq1: bit identical (0)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _glue_ref as R

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
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(*ts):
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in ts]
    return out[0] if len(out) == 1 else out


def report(op, res):
    for k, (err, e32, bound) in res.items():
        print(f"GLUE {op} {k} err={err:.3e} e32={e32:.3e} bound={bound:.3e}")


@pytest.mark.parametrize("N,lo,hi", R.HEAD_CASES)
def test_shac_head_fwd_bwd(N, lo, hi):
    _lib, lib = L()
    for phase in R.HEAD_PHASES:
        inp = R.head_inputs(N, lo, hi, phase)
        mu, ls, eps = dev(inp["mu"]), dev(inp["log_std"]), dev(inp["eps"])
        action = dev(R.blank((N, 4)))
        _lib.check(lib.vf_shac_head_fwd(mu.data_ptr(), ls.data_ptr(), eps.data_ptr(), action.data_ptr(), N, lo, hi, st()))
        res = R.check_head_fwd({"action": host(action)}, inp)
        report("head_fwd", res)
        da, a = dev(inp["d_action"]), dev(inp["action"])
        d_mu, d_ls = dev(R.blank((N, 4))), dev(R.blank((N, 4)))
        _lib.check(lib.vf_shac_head_bwd(da.data_ptr(), a.data_ptr(), ls.data_ptr(), eps.data_ptr(), d_mu.data_ptr(), d_ls.data_ptr(), N, lo,
                                        hi, st()))
        g_mu, g_ls = host(d_mu, d_ls)
        report("head_bwd", R.check_head_bwd({"d_mu": g_mu, "d_log_std": g_ls}, inp))


@pytest.mark.parametrize("N", R.ROWS)
def test_reparam_fwd_bwd(N):
    _lib, lib = L()
    inp = R.reparam_inputs(N)
    mean, ls, eps = dev(inp["mean"]), dev(inp["log_std"]), dev(inp["eps"])
    action = dev(R.blank((N, 4)))
    _lib.check(lib.vf_reparam_fwd(mean.data_ptr(), ls.data_ptr(), eps.data_ptr(), action.data_ptr(), N, st()))
    report("reparam_fwd", R.check_reparam_fwd({"action": host(action)}, inp))
    da, a = dev(inp["d_action"]), dev(inp["action"])
    g = dev(R.padded(inp["g_log_std"]))
    before = inp["g_log_std"]
    for call in range(2):                                                # the second call accumulates on the first
        d_mean = dev(R.blank((N, 4)))
        _lib.check(lib.vf_reparam_bwd(da.data_ptr(), a.data_ptr(), ls.data_ptr(), eps.data_ptr(), d_mean.data_ptr(), g.data_ptr(), N, st()))
        g_dm, g_g = host(d_mean, g)
        report("reparam_bwd", R.check_reparam_bwd({"d_mean": g_dm, "g_log_std": g_g}, dict(inp, g_log_std=before)))
        before = g_g[:N * 4].reshape(N, 4).copy()


@pytest.mark.parametrize("N", R.ROWS)
def test_bptt_accumulate(N):
    _lib, lib = L()
    inp = R.accumulate_inputs(N)
    disc, loss = dev(R.padded(inp["disc"])), dev(R.padded(inp["loss"]))
    d0, l0 = inp["disc"], inp["loss"]
    for s in inp["steps"]:                                               # three steps in a row on the same state
        rew, done, drew = dev(s["reward"]), dev(s["done"]), dev(R.blank((N,)))
        _lib.check(lib.vf_bptt_accumulate(rew.data_ptr(), done.data_ptr(), disc.data_ptr(), loss.data_ptr(), drew.data_ptr(), inp["gamma"],
                                          inp["scale"], N, st()))
        g_d, g_l, g_r = host(disc, loss, drew)
        R.check_bptt_accumulate({"disc": g_d, "loss": g_l, "d_reward": g_r},
                                dict(reward=s["reward"], done=s["done"], disc=d0, loss=l0, gamma=inp["gamma"], scale=inp["scale"]))
        d0, l0 = g_d[:N].copy(), g_l[:N].copy()


@pytest.mark.parametrize("last_step", [0, 1])
@pytest.mark.parametrize("N", R.ROWS)
def test_shac_accumulate(N, last_step):
    _lib, lib = L()
    inp = R.accumulate_inputs(N)
    disc, loss = dev(R.padded(inp["disc"])), dev(R.padded(inp["loss"]))
    d0, l0 = inp["disc"], inp["loss"]
    for s in inp["steps"]:
        rew, done, flags, q0, q1 = (dev(s[k]) for k in ("reward", "done", "ep_flags", "q0", "q1"))
        drew, nv, epd = dev(R.blank((N,))), dev(R.blank((N,))), dev(R.blank((N,), np.uint8))
        _lib.check(lib.vf_shac_accumulate(rew.data_ptr(), done.data_ptr(), flags.data_ptr(), q0.data_ptr(), q1.data_ptr(), disc.data_ptr(),
                                          loss.data_ptr(), drew.data_ptr(), nv.data_ptr(), epd.data_ptr(), inp["gamma"], inp["scale"],
                                          last_step, N, st()))
        g_d, g_l, g_r, g_nv, g_epd = host(disc, loss, drew, nv, epd)
        R.check_shac_accumulate({"disc": g_d, "loss": g_l, "d_reward": g_r, "next_value": g_nv, "ep_done": g_epd},
                                dict(s, disc=d0, loss=l0, gamma=inp["gamma"], scale=inp["scale"], last_step=last_step))
        d0, l0 = g_d[:N].copy(), g_l[:N].copy()


@pytest.mark.parametrize("H,N", R.HORIZON_CASES)
def test_shac_accumulate_horizon(H, N):
    _lib, lib = L()
    inp = R.horizon_inputs(H, N)
    rew, done, flags, q0, q1 = (dev(inp[k]) for k in ("reward", "done", "ep_flags", "q0", "q1"))
    disc, loss = dev(R.padded(inp["disc"])), dev(R.padded(inp["loss"]))
    drew, nv, epd = dev(R.blank((H, N))), dev(R.blank((H, N))), dev(R.blank((H, N), np.uint8))
    _lib.check(lib.vf_shac_accumulate_horizon(rew.data_ptr(), done.data_ptr(), flags.data_ptr(), q0.data_ptr(), q1.data_ptr(), disc.data_ptr(),
                                              loss.data_ptr(), drew.data_ptr(), nv.data_ptr(), epd.data_ptr(), inp["gamma"], inp["scale"], H, N,
                                              st()))
    g_d, g_l, g_r, g_nv, g_epd = host(disc, loss, drew, nv, epd)
    R.check_shac_accumulate_horizon({"disc": g_d, "loss": g_l, "d_reward": g_r, "next_value": g_nv, "ep_done": g_epd}, inp)


@pytest.mark.parametrize("M,M_global", R.TWIN_CASES)
def test_twin_q_loss(M, M_global):
    _lib, lib = L()
    inp = R.twin_q_inputs(M, M_global)
    q0, q1, tg = dev(inp["q0"]), dev(inp["q1"]), dev(inp["target"])
    dq0, dq1, loss = dev(R.blank((M,))), dev(R.blank((M,))), dev(R.blank((1,)))
    nscr = int(lib.vf_twin_q_loss_scratch_doubles(M))
    assert nscr == (M + 255) // 256
    scr = torch.zeros(nscr, dtype=torch.float64, device=DEV)
    args = (q0.data_ptr(), q1.data_ptr(), tg.data_ptr(), dq0.data_ptr(), dq1.data_ptr(), loss.data_ptr(), scr.data_ptr(), M)
    if M > 1:
        assert lib.vf_twin_q_loss(*args, M - 1, st()) == EINVAL          # M_global < M: nothing launched
    _lib.check(lib.vf_twin_q_loss(*args, M_global, st()))
    g0, g1, gl = host(dq0, dq1, loss)
    report("twin_q_loss", R.check_twin_q_loss({"dq0": g0, "dq1": g1, "loss": gl}, inp))


@pytest.mark.parametrize("n,tau", R.POLYAK_CASES)
def test_polyak_update(n, tau):
    _lib, lib = L()
    inp = R.polyak_inputs(n, tau)
    target, param = dev(R.padded(inp["target"])), dev(inp["param"])
    _lib.check(lib.vf_polyak_update(target.data_ptr(), param.data_ptr(), n, tau, st()))
    report("polyak", R.check_polyak({"target": host(target)}, inp))      # tau = 1 / tau = 0: bit for bit, inside the comparator


@pytest.mark.parametrize("n,offset", [(n, 0) for n in R.SUMSQ_N] + [(4097, 1)])       # offset 1: a view one float past an aligned address
def test_sumsq(n, offset):
    _lib, lib = L()
    inp = R.sumsq_inputs(n)
    buf = dev(np.concatenate([np.full(offset, 3.0e4, dtype=np.float32), inp["x"]]))
    assert buf.data_ptr() % 16 == 0
    out, scratch = dev(R.blank((1,))), torch.zeros(4096, device=DEV)    # the scratch size the trainers give it
    _lib.check(lib.vf_sumsq(buf.data_ptr() + 4 * offset, n, out.data_ptr(), scratch.data_ptr(), st()))
    report("sumsq", R.check_sumsq({"sumsq": host(out)}, inp))


@pytest.mark.parametrize("name", list(R.ADAM_CASES))
def test_adam_step(name):
    _lib, lib = L()
    inp, extra = R.adam_case(name)
    cfg, n = inp["cfg"], inp["p"].size
    p, m, v = (dev(R.padded(inp[k])) for k in "pmv")
    ss, scratch = torch.zeros(1, device=DEV), torch.zeros(4096, device=DEV)
    pack_map = packed = None
    if "pack_map" in inp:
        pack_map, packed = dev(inp["pack_map"]), dev(R.blank((inp["packed_size"],)))
        assert int(inp["pack_map"].max()) < inp["packed_size"]
    got = []
    for k, grad in enumerate(inp["grads"]):
        g = dev(grad)
        c = _lib.AdamCfg(cfg["lr"], cfg["beta1"], cfg["beta2"], cfg["eps"], cfg["weight_decay"], cfg["max_grad_norm"], 1 + k, 0,
                         None if pack_map is None else pack_map.data_ptr(), None if packed is None else packed.data_ptr())
        ss_ptr, partials = ss.data_ptr(), None
        if "n_partials" in extra:                                        # the norm from per-block fp64 partials + the uncovered tail
            tail_from = n - extra["tail"]
            sq = grad[:tail_from].astype(np.float64) ** 2
            partials = dev(np.array([c_.sum() for c_ in np.array_split(sq, extra["n_partials"])], dtype=np.float64))
            c.sumsq_partials, c.n_sumsq_partials, c.sumsq_tail_from = partials.data_ptr(), extra["n_partials"], tail_from
            ss_ptr = None
        elif extra.get("null_sumsq"):
            ss_ptr = None                                                # max_grad_norm <= 0: no norm is read
        else:
            _lib.check(lib.vf_sumsq(g.data_ptr(), n, ss.data_ptr(), scratch.data_ptr(), st()))
        _lib.check(lib.vf_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, ss_ptr, C.byref(c), st()))
        snap = dict(zip("pmv", host(p, m, v)))
        if packed is not None:
            snap["packed"] = host(packed)
        got.append(snap)
    report(f"adam[{name}]", R.check_adam(got, inp))


def test_adam_step_argument_checks():
    _lib, lib = L()
    n = 257
    p, g, m, v = (torch.zeros(n, device=DEV) for _ in range(4))
    ss = torch.ones(1, device=DEV)
    pm = torch.full((n, 4), -1, dtype=torch.int32, device=DEV)

    def rc(step=1, max_grad_norm=0.5, sumsq=ss, pack_map=None, packed=None):
        c = _lib.AdamCfg(1e-3, 0.9, 0.999, 1e-8, 0.0, max_grad_norm, step, 0, None if pack_map is None else pack_map.data_ptr(),
                         None if packed is None else packed.data_ptr())
        return lib.vf_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, None if sumsq is None else sumsq.data_ptr(),
                                C.byref(c), st())

    assert rc(step=0) == EINVAL
    assert rc(pack_map=pm) == EINVAL                                     # a pack_map without packed
    assert rc(sumsq=None) == EINVAL                                      # clipping with no norm source
    assert rc() == 0 and rc(max_grad_norm=0.0, sumsq=None) == 0
    torch.cuda.synchronize()
    assert not p.any() and not m.any() and not v.any()                   # zero gradient, no weight decay: nothing moved
