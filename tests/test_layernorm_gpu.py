"""LayerNorm on the GPU: the row-wise kernels behind vf_layernorm_fwd / vf_layernorm_bwd (csrc/vf_layernorm.hip) against the plain
fp64 restatements of tests/_ln_ref.py (bound per output array: max(4 max|ref32 - ref64|, 2^-22 max|ref64|), sentinel pads), MlpPolicy
networks with ``layer_norm`` layer by layer against fp64 autograd of to_torch() (every block on its own scale, torch's fp32 autograd
as the yardstick), and PPO with ln / pi_ln / vf_ln on NavigationEnv.  BPTT and SHAC refuse layer norm."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import _ln_ref as R
from _gradcheck import assert_blocks, assert_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1          # VF_EINVAL (include/visfly_amd.h)
EPS = float(np.float32(R.EPS))


def L():
    from visfly_amd import _lib
    return _lib, _lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(bufs):
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def run_fwd(inp, alias=False):
    """-> padded output buffers {y, xhat, rstd} (device tensors); ``alias``: xhat is written over z"""
    _lib, lib = L()
    M, W = inp["z"].shape
    z = dev(R.padded(inp["z"]))
    gamma, beta = dev(inp["gamma"]), dev(inp["beta"])
    out = {"y": dev(R.blank((M, W))), "xhat": z if alias else dev(R.blank((M, W))), "rstd": dev(R.blank((M,)))}
    _lib.check(lib.vf_layernorm_fwd(z.data_ptr(), W, gamma.data_ptr(), beta.data_ptr(), EPS, out["y"].data_ptr(), W, out["xhat"].data_ptr(), W,
                                    out["rstd"].data_ptr(), M, W, inp["kind"], st()))
    return out


def run_bwd(inp, alias=False, init=None):
    """-> padded output buffers {dz, dgamma, dbeta}; ``alias``: dz is written over dy; ``init``: accumulate into buffers holding it"""
    _lib, lib = L()
    M, W = inp["dy"].shape
    dy = dev(R.padded(inp["dy"]))
    y, xhat, rstd, gamma = dev(inp["y"]), dev(inp["xhat"]), dev(inp["rstd"]), dev(inp["gamma"])
    start = R.blank((W,)) if init is None else R.padded(np.full(W, init, np.float32))
    out = {"dz": dy if alias else dev(R.blank((M, W))), "dgamma": dev(start), "dbeta": dev(start)}
    scratch = torch.empty(int(lib.vf_layernorm_bwd_scratch_floats(M, W)), device=DEV)
    _lib.check(lib.vf_layernorm_bwd(dy.data_ptr(), W, y.data_ptr() if inp["kind"] else None, W, xhat.data_ptr(), W, rstd.data_ptr(),
                                    gamma.data_ptr(), out["dz"].data_ptr(), W, out["dgamma"].data_ptr(), out["dbeta"].data_ptr(), M, W,
                                    inp["kind"], 0 if init is None else 1, scratch.data_ptr(), st()))
    return out


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _entry_points(M, W, kinds=R.KINDS, variance_rows=False):
    worst = {}
    for kind in kinds:
        inp = R.ln_inputs(M, W, kind, variance_rows=variance_rows)
        f = run_fwd(inp)
        assert _same(f, run_fwd(inp)), "forward: two runs differ"
        res = R.check_fwd(host(f), inp)
        fa = run_fwd(inp, alias=True)
        assert _same(fa, f), "forward with xhat == z differs from the plain call"
        b = run_bwd(inp)
        assert _same(b, run_bwd(inp)), "backward: two runs differ"
        res.update(R.check_bwd(host(b), inp))
        assert _same(run_bwd(inp, alias=True), b), "backward with dz == dy differs from the plain call"
        acc = run_bwd(inp, init=5.0)
        assert _same(acc, run_bwd(inp, init=5.0))
        ra = R.check_bwd(host(acc), inp, init=5.0)
        assert torch.equal(acc["dz"], b["dz"])
        for k, v in {**R.ratios(res), **{k + " (accumulate)": v for k, v in R.ratios(ra).items() if k != "dz"}}.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"layernorm M {M} W {W}: worst |got - ref64| / |ref32 - ref64| " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("W", R.WIDTHS)
@pytest.mark.parametrize("M", R.ROWS)
def test_layernorm_entry_points_vs_fp64(M, W):
    """forward (y, xhat, rstd) and backward (dz, dgamma, dbeta) for every activation kind, each call twice (bit-identical), the
    aliased forms xhat == z and dz == dy, and the accumulating backward from buffers filled with 5.0"""
    _entry_points(M, W)


def test_layernorm_many_partials():
    """25 600 rows of 64: 1600 wave partials of dgamma / dbeta (16 rows each) go through the fold"""
    _entry_points(*R.BIG, kinds=(0, 2))


@pytest.mark.parametrize("W", (48, 64, 65, 200))
def test_layernorm_rows_that_catch_a_wrong_variance(W):
    """a constant row, a row of 1000 + N(0, 1), a row scaled by 1e-4"""
    _entry_points(65, W, variance_rows=True)


@pytest.mark.parametrize("W", R.WIDTHS)
@pytest.mark.parametrize("pad,col", [(5, 2), (8, 4)])
def test_layernorm_strided_operands(W, pad, col):
    """every operand a slice [col, col + W) of a buffer W + pad wide: (5, 2) leaves nothing 16-byte aligned (one value per access
    at every width), (8, 4) keeps the 16-byte accesses with a leading dimension above W; columns outside the slice untouched"""
    _lib, lib = L()
    M, ld = 65, W + pad
    sent = float(R.SENT_F)
    p = lambda t: t.data_ptr() + 4 * col
    wide = lambda a=None: (torch.full((M, ld), sent, device=DEV) if a is None else
                           torch.cat([torch.full((M, col), sent, device=DEV), dev(a), torch.full((M, ld - col - W), sent, device=DEV)], dim=1).contiguous())

    def outside_untouched(t, what):
        assert bool((t[:, :col] == sent).all()) and bool((t[:, col + W:] == sent).all()), what + ": columns outside the slice were written"

    for kind in (1, 3):
        inp = R.ln_inputs(M, W, kind)
        gamma, beta = dev(inp["gamma"]), dev(inp["beta"])
        z, y, xhat, rstd = wide(inp["z"]), wide(), wide(), dev(R.blank((M,)))
        _lib.check(lib.vf_layernorm_fwd(p(z), ld, gamma.data_ptr(), beta.data_ptr(), EPS, p(y), ld, p(xhat), ld, rstd.data_ptr(), M, W, kind, st()))
        r32, r64 = R.fwd_refs(inp)
        for name, t in (("y", y), ("xhat", xhat)):
            outside_untouched(t, name)
            R.within(name, t[:, col:col + W].cpu().numpy(), r32[name], r64[name])
        R.within("rstd", R.body("rstd", rstd.cpu().numpy(), (M,)), r32["rstd"], r64["rstd"])
        assert torch.equal(z[:, col:col + W], dev(inp["z"]))
        dy, ys, xs, dz = wide(inp["dy"]), wide(inp["y"]), wide(inp["xhat"]), wide()
        dgamma, dbeta = dev(R.blank((W,))), dev(R.blank((W,)))
        scratch = torch.empty(int(lib.vf_layernorm_bwd_scratch_floats(M, W)), device=DEV)
        rs = dev(inp["rstd"])
        _lib.check(lib.vf_layernorm_bwd(p(dy), ld, p(ys), ld, p(xs), ld, rs.data_ptr(), gamma.data_ptr(), p(dz), ld,
                                        dgamma.data_ptr(), dbeta.data_ptr(), M, W, kind, 0, scratch.data_ptr(), st()))
        b32, b64 = R.bwd_refs(inp)
        outside_untouched(dz, "dz")
        R.within("dz", dz[:, col:col + W].cpu().numpy(), b32["dz"], b64["dz"])
        R.within("dgamma", R.body("dgamma", dgamma.cpu().numpy(), (W,)), b32["dgamma"], b64["dgamma"])
        R.within("dbeta", R.body("dbeta", dbeta.cpu().numpy(), (W,)), b32["dbeta"], b64["dbeta"])


def test_layernorm_refuses_bad_shapes():
    _lib, lib = L()
    t = torch.zeros(4096, device=DEV)
    q = t.data_ptr()
    fwd = lambda M, W, ldz, ldy, ldx, act=1: lib.vf_layernorm_fwd(q, ldz, q, q, EPS, q, ldy, q, ldx, q, M, W, act, st())
    bwd = lambda M, W, lddy, ldy, ldx, lddz, act=1: lib.vf_layernorm_bwd(q, lddy, q, ldy, q, ldx, q, q, q, lddz, q, q, M, W, act, 0, q, st())
    assert fwd(1, 0, 8, 8, 8) == EINVAL and fwd(1, 513, 513, 513, 513) == EINVAL and fwd(0, 8, 8, 8, 8) == EINVAL
    assert fwd(1, 8, 7, 8, 8) == EINVAL and fwd(1, 8, 8, 7, 8) == EINVAL and fwd(1, 8, 8, 8, 7) == EINVAL
    assert fwd(1, 8, 8, 8, 8, act=5) == EINVAL and fwd(1, 8, 8, 8, 8, act=-1) == EINVAL
    assert bwd(1, 0, 8, 8, 8, 8) == EINVAL and bwd(1, 513, 513, 513, 513, 513) == EINVAL and bwd(0, 8, 8, 8, 8, 8) == EINVAL
    assert bwd(1, 8, 7, 8, 8, 8) == EINVAL and bwd(1, 8, 8, 7, 8, 8) == EINVAL and bwd(1, 8, 8, 8, 7, 8) == EINVAL
    assert bwd(1, 8, 8, 8, 8, 7) == EINVAL and bwd(1, 8, 8, 8, 8, 8, act=5) == EINVAL
    assert fwd(1, 8, 8, 8, 8) == 0 and bwd(1, 8, 8, 8, 8, 8) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------------------------------
DIMS = {"state": 13, "target": 3}
EXT = {"state": [256, 64], "target": [48, 32]}       # widths 48 and 256 among them; the state branch ends in columns 0..63 of feat
PI, VF = [64, 48], [256, 64]
NETS = {"extractor": dict(extractor={"state": True, "target": True}), "pi": dict(pi=True), "vf": dict(vf=True),
        "all": dict(extractor={"state": True, "target": True}, pi=True, vf=True),
        "state_branch_only": dict(extractor={"state": True, "target": False})}
M_NET = 200


def _policy(which, acts, seed=5):
    from visfly_amd.ppo import MlpPolicy
    pol = MlpPolicy(DIMS, EXT, PI, VF, DEV, seed=seed, layer_norm=NETS[which], activation=acts[0], extractor_activation=acts[1])
    assert pol.ln and pol._plan is None and pol.chain_shape is None
    g = torch.Generator().manual_seed(seed + 1)
    for ly in pol.layers:         # gamma / beta away from 1 / 0: a kernel that ignores them is wrong by 30 %
        if ly.ln:
            pol.ln_weight(ly).add_((0.3 * torch.randn(ly.No, generator=g)).to(DEV))
            pol.ln_bias(ly).add_((0.2 * torch.randn(ly.No, generator=g)).to(DEV))
    pol.mark_updated()
    return pol


def _net_inputs(seed=0):
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    obs = {k: torch.randn((M_NET, d), device=DEV, generator=g) for k, d in DIMS.items()}
    return obs, torch.randn((M_NET, 4), device=DEV, generator=g) / M_NET, torch.randn((M_NET, 1), device=DEV, generator=g) / M_NET


def _forward_backward(pol, obs, d0, d1, fill):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mean, value = pol.forward(obs)
        mean, value = mean.clone(), value.clone()
        pol.grad.fill_(fill)
        d_in = pol.backward(d0, d1, None, need_input_grad=True)
    return mean, value, pol.grad.clone(), {k: v.clone() for k, v in d_in.items()}


@pytest.mark.parametrize("acts", [("tanh", "elu"), ("elu", "tanh")])
@pytest.mark.parametrize("which", list(NETS))
def test_network_with_layer_norm_vs_fp64_autograd(which, acts):
    """forward heads, every parameter block (gamma / beta blocks included) and every observation-gradient row against fp64 autograd of
    to_torch(); Tanh and ELU are C1, so no unit sits on a kink; two runs bit-identical"""
    pol = _policy(which, acts)
    obs, d0, d1 = _net_inputs()
    mean, value, grad, d_in = _forward_backward(pol, obs, d0, d1, 7.0)
    ref = R.network_reference(pol, obs, R.head_loss(d0, d1))
    what = f"{which} {acts}"
    R.assert_heads(mean, value, ref, what)
    assert_blocks(pol, grad, ref, what, untouched=7.0)
    R.assert_ln_blocks(pol, grad, ref, what, untouched=7.0)
    assert bool((grad[pol.log_std_off:] == 7.0).all())
    assert set(d_in) == set(DIMS)
    for k in DIMS:
        assert_rows(d_in[k], ref.d_in[k], ref.d_in32[k], f"{what} d obs:{k}")
    m2, v2, g2, d2 = _forward_backward(pol, obs, d0, d1, 7.0)
    assert torch.equal(mean, m2) and torch.equal(value, v2) and torch.equal(grad, g2) and all(torch.equal(d_in[k], d2[k]) for k in d_in)


@pytest.mark.parametrize("skip", ["vf", "pi"])
def test_skipped_trunk_leaves_its_layer_norm_blocks_untouched(skip):
    pol = _policy("all", ("tanh", "elu"))
    obs, d0, d1 = _net_inputs(1)
    if skip == "vf":
        d1 = None
    else:
        d0 = None
    _mean, _value, grad, _d_in = _forward_backward(pol, obs, d0, d1, 7.0)
    ref = R.network_reference(pol, obs, R.head_loss(d0, d1))
    assert_blocks(pol, grad, ref, f"skip {skip}", untouched=7.0)
    R.assert_ln_blocks(pol, grad, ref, f"skip {skip}", untouched=7.0)
    for ly in pol.layers:
        if ly.dst.startswith(skip + ":"):
            assert ly.ln and bool((grad[ly.g_off:ly.be_off + ly.No] == 7.0).all()), ly.dst


def test_accumulating_backward_adds_gamma_and_beta():
    pol = _policy("all", ("tanh", "elu"))
    obs, d0, d1 = _net_inputs(2)
    _m, _v, g1, _d = _forward_backward(pol, obs, d0, d1, 0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pol.forward(obs)
        pol.grad.copy_(g1)
        pol.backward(d0, d1, None, accumulate=True)
    for ly in pol.layers:
        if ly.ln:
            lo, hi = ly.g_off, ly.be_off + ly.No
            assert torch.equal(pol.grad[lo:hi], g1[lo:hi] + g1[lo:hi]), ly.dst


# ---------------------------------------------------------------------------------------------------------------------------
# trainers
# ---------------------------------------------------------------------------------------------------------------------------
LN_KWARGS = dict(activation_fn="tanh",
                 features_extractor_kwargs=dict(net_arch={"state": {"layer": [128, 64], "ln": True}, "target": {"layer": [128, 64], "ln": True}}),
                 net_arch=dict(pi=[64, 64], vf=[64, 64], pi_ln=True, vf_ln=True))


def _nav():
    from visfly_amd.envs import NavigationEnv
    from _golden import ENV_DYN
    return NavigationEnv(num_agent_per_scene=1024, seed=1, dynamics_kwargs=dict(ENV_DYN), device=DEV, max_episode_steps=64, tensor_output=True)


def _ppo(env, policy_kwargs=LN_KWARGS, **kw):
    from visfly_amd.ppo import PPO
    args = dict(n_steps=16, batch_size=4096, n_epochs=4, learning_rate=3e-4, ent_coef=0.01, seed=3, policy_kwargs=policy_kwargs)
    args.update(kw)
    return PPO(env, **args)


def test_ppo_minibatch_gradient_with_layer_norm_vs_fp64_autograd():
    """the constructor says once that the network runs layer by layer; one _minibatch_update on a fixed minibatch: pol.grad against
    fp64 autograd of the SB3 loss over to_torch(), block by block (gamma / beta and log_std included)"""
    from test_ppo_gpu import sb3_squashed_log_prob, torch_ppo_loss
    env = _nav()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ppo = _ppo(env)
        pol = ppo.policy
        assert pol.ln and all(ly.ln == (ly.dst not in ("mean", "value")) for ly in pol.layers)
        B = 4096
        g = torch.Generator(device=DEV).manual_seed(11)
        obs = {k: torch.randn((B, d), device=DEV, generator=g) for k, d in pol.obs_dims.items()}
        for ly in pol.layers:
            if ly.ln:
                pol.ln_weight(ly).add_(0.3 * torch.randn(ly.No, device=DEV, generator=g))
                pol.ln_bias(ly).add_(0.2 * torch.randn(ly.No, device=DEV, generator=g))
        pol.mark_updated()
        mean, _value = pol.forward(obs, save_activations=False)
        actions = torch.tanh(mean + 0.7 * torch.randn((B, 4), device=DEV, generator=g)).contiguous()
        old_lp = sb3_squashed_log_prob(mean, pol.log_std, actions) + 0.3 * torch.randn(B, device=DEV, generator=g)
        adv, ret = torch.randn(B, device=DEV, generator=g), torch.randn(B, device=DEV, generator=g)

        def loss_fn(net, xs):
            c = lambda t: t.detach().cpu().to(net.log_std.dtype)
            return torch_ppo_loss(net, xs, c(actions), c(old_lp), c(adv), c(ret), 0.2, 0.01, 0.5)[0]
        ref = R.network_reference(pol, obs, loss_fn, need_input_grad=False)       # before the optimiser step moves the parameters
        mb = {"actions": actions, "old_lp": old_lp.contiguous(), "adv": adv, "ret": ret, **{"obs:" + k: v for k, v in obs.items()}}
        assert ppo._minibatch_update(mb) is not None
        torch.cuda.synchronize()
    said = [str(x.message) for x in w if "layer norm" in str(x.message)]
    assert len(said) == 1 and "layer by layer" in said[0], [str(x.message)[:120] for x in w]
    assert_blocks(pol, pol.grad, ref, "PPO minibatch")
    R.assert_ln_blocks(pol, pol.grad, ref, "PPO minibatch")
    lo = pol.log_std_off
    r = R.hold_block(pol.grad[lo:].double().cpu(), ref.grad[lo:], ref.grad32[lo:], "PPO minibatch", "log_std")
    print(f"PPO minibatch log_std block: err / max {r[0]:.3e}, torch fp32 {r[1]:.3e}")
    env.close()


def test_ppo_learns_saves_and_loads_with_layer_norm(tmp_path):
    from visfly_amd import checkpoint
    from visfly_amd.ppo import PPO
    env = _nav()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ppo = _ppo(env)
        pol = ppo.policy
        vloss = []
        for _ in range(6):
            ppo.learn(16 * 1024)
            vloss.append(ppo.logs["train/value_loss"])
        torch.cuda.synchronize()
        print("value loss per iteration:", [f"{v:.4f}" for v in vloss])
        assert all(np.isfinite(vloss)) and vloss[-1] < vloss[0], vloss
        assert bool(torch.isfinite(pol.flat).all())
        for ly in pol.layers:
            if ly.ln:
                assert not bool((pol.ln_weight(ly) == 1).all()) and not bool((pol.ln_bias(ly) == 0).all()), ly.dst
        # the SB3-layout state_dict carries the key pattern read off the reference's modules
        gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ln_keys.json")))
        sd = checkpoint.policy_state_dict(pol)
        pattern = [k for k in gold if k.startswith(("features_extractor.state_extractor.", "mlp_extractor.policy_net."))]
        assert len(pattern) == 16 and all(k in sd for k in pattern)
        assert all(k.replace("policy_net", "value_net") in sd for k in pattern if "policy_net" in k)
        path = ppo.save(str(tmp_path / "ppo_ln"))
        data = json.loads(__import__("zipfile").ZipFile(path).read("data"))
        assert data["policy_spec"]["layer_norm"] == dict(extractor={"state": True, "target": True}, pi=True, vf=True)
        env2 = _nav()
        ppo2 = PPO.load(path, env2)
        assert ppo2.policy.ln and torch.equal(ppo2.policy.flat, pol.flat)
        assert torch.equal(ppo2.exp_avg, ppo.exp_avg) and torch.equal(ppo2.exp_avg_sq, ppo.exp_avg_sq) and ppo2._opt_step == ppo._opt_step
        g = torch.Generator(device=DEV).manual_seed(5)
        obs = {k: torch.randn((1024, d), device=DEV, generator=g) for k, d in pol.obs_dims.items()}
        a1, a2 = ppo.predict(obs, deterministic=True)[0], ppo2.predict(obs, deterministic=True)[0]
        assert torch.equal(a1, a2)
        # the same archive into a trainer whose policy has no LayerNorm
        plain = _ppo(env2, policy_kwargs=dict(activation_fn="tanh"))
        with pytest.raises(ValueError, match="layer_norm"):
            plain.set_parameters(path)
    env.close()
    env2.close()


def test_bptt_and_shac_refuse_layer_norm():
    from visfly_amd.bptt import BPTT
    from visfly_amd.envs import HoverEnv
    from visfly_amd.shac import SHAC
    from _golden import ENV_DYN
    env = HoverEnv(num_agent_per_scene=64, seed=5, dynamics_kwargs=dict(ENV_DYN), device=DEV, tensor_output=True)
    ext_ln = dict(features_extractor_kwargs=dict(net_arch={"state": {"layer": [128, 64], "ln": True}}))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for pk in (dict(net_arch=dict(pi=[64, 64], vf=[64, 64], pi_ln=True)), ext_ln):
            with pytest.raises(NotImplementedError, match="layer norm"):
                BPTT(env, horizon=8, seed=1, policy_kwargs=pk)
        with pytest.raises(NotImplementedError, match="layer norm"):
            BPTT(env, horizon=8, seed=1, policy="MTDPolicy", policy_kwargs=dict(net_arch=dict(pi=[64, 64], qf=[64, 64], pi_ln=True)))
        for pk in (ext_ln, dict(net_arch=dict(pi=[64, 64], qf=[64, 64], pi_ln=[True, True]))):
            with pytest.raises(NotImplementedError, match="layer norm"):
                SHAC(env, horizon=8, seed=1, policy_kwargs=pk)
    env.close()
