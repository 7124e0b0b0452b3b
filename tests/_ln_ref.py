"""Plain references and comparators for the LayerNorm kernels (csrc/vf_layernorm.hip) and for MlpPolicy networks with LayerNorm.

A helper module like _glue_ref.py, whose comparator forms it reuses: numpy / torch only, no ``visfly_amd`` import at module level,
written from the formulas of nn.LayerNorm (biased variance, eps inside the root) and of its reverse, not from the kernels.
``dtype``: ``torch.float64`` is the truth, ``torch.float32`` the reference's own arithmetic.

Per output array   bound = max(4 * max|ref32 - ref64|, 2^-22 * max|ref64|)   (_glue_ref.within), from the references alone; every
output buffer is PAD elements longer than needed, pre-filled with a sentinel that must come back untouched (_glue_ref.body).

The network half: ``network_reference`` is autograd of ``MlpPolicy.to_torch()`` in fp64 next to torch's own fp32 autograd, with the
gamma / beta blocks in the flat gradients (``_gradcheck._flat64`` knows the Linear blocks only); ``assert_ln_blocks`` holds every
gamma and beta block to _gradcheck's bound: max(BLOCK_TOL of the block's largest reference entry, TORCH32 x the fp32-autograd
distance on that block).
"""
import types

import numpy as np
import torch

from _glue_ref import F32, F64, PAD, SENT_F, blank, body, padded, within  # noqa: F401  (re-exported for the tests)

EPS = 1e-3                    # create_mlp: nn.LayerNorm(width, eps=1e-3) (utils/policies/extractors.py:429)
KINDS = (0, 1, 2, 3, 4)       # VF_ACTIVATION_*: none, ReLU, Tanh, ELU, LeakyReLU
WIDTHS = (4, 32, 33, 48, 64, 65, 128, 200, 256, 512)
ROWS = (1, 63, 64, 65, 257)
BIG = (25600, 64)             # the fold of dgamma / dbeta sees many partials


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def _np(t):
    return t.detach().numpy()


def act_fwd(z, kind):
    if kind == 1:
        return torch.relu(z)
    if kind == 2:
        return torch.tanh(z)
    if kind == 3:
        return torch.where(z > 0, z, torch.expm1(z))
    if kind == 4:
        return torch.where(z > 0, z, 0.01 * z)
    return z


def act_mul(v, y, kind):
    """upstream gradient v through the activation whose OUTPUT was y"""
    if kind == 1:
        return torch.where(y > 0, v, torch.zeros_like(v))
    if kind == 2:
        return v * (1.0 - y * y)
    if kind == 3:
        return torch.where(y > 0, v, v * (y + 1.0))
    if kind == 4:
        return torch.where(y > 0, v, 0.01 * v)
    return v


def ln_fwd(z, gamma, beta, kind, dtype, eps=EPS):
    """mean = sum z / W; var = sum (z - mean)^2 / W; rstd = 1 / sqrt(var + eps); xhat = (z - mean) rstd; y = act(gamma xhat + beta)"""
    z, gamma, beta = _t(z, dtype), _t(gamma, dtype), _t(beta, dtype)
    W = z.shape[1]
    mean = z.sum(dim=1, keepdim=True) / W
    c = z - mean
    var = (c * c).sum(dim=1, keepdim=True) / W
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = c * rstd
    return {"y": _np(act_fwd(gamma * xhat + beta, kind)), "xhat": _np(xhat), "rstd": _np(rstd.view(-1))}


def ln_bwd(dy, y, xhat, rstd, gamma, kind, dtype, init=None):
    """g = dy act'(y); dbeta = sum_rows g; dgamma = sum_rows g xhat; h = g gamma; dz = rstd (h - mean_W(h) - xhat mean_W(h xhat));
    ``init``: the value dgamma / dbeta held before an accumulating call"""
    dy, xhat, rstd, gamma = _t(dy, dtype), _t(xhat, dtype), _t(rstd, dtype).view(-1, 1), _t(gamma, dtype)
    g = act_mul(dy, _t(y, dtype), kind) if kind else dy
    W = dy.shape[1]
    h = g * gamma
    m1 = h.sum(dim=1, keepdim=True) / W
    m2 = (h * xhat).sum(dim=1, keepdim=True) / W
    dz = rstd * (h - m1 - xhat * m2)
    dgamma, dbeta = (g * xhat).sum(dim=0), g.sum(dim=0)
    if init is not None:
        dgamma, dbeta = dgamma + float(init), dbeta + float(init)
    return {"dz": _np(dz), "dgamma": _np(dgamma), "dbeta": _np(dbeta)}


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and comparators of the entry-point cases (the host tests run the comparators over the same inputs)
# ---------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([20261, *[int(k) for k in key]])


def ln_inputs(M, W, kind, variance_rows=False):
    """z ~ 0.3 + 1.5 N(0, 1), gamma ~ 1 + 0.3 N, beta ~ 0.2 N, dy ~ N(0, 1); the saved y / xhat / rstd the backward is handed are the
    fp64 reference's, rounded to fp32 (a ReLU / LeakyReLU unit at zero then has one side in kernel and references).
    ``variance_rows``: row 0 constant, row 1 = 1000 + N(0, 1), row 2 scaled by 1e-4 -- what a one-pass variance, a missing eps or a
    mean without care for cancellation gets wrong"""
    rng = _rng(M, W, kind, int(variance_rows))
    z = (0.3 + 1.5 * rng.standard_normal((M, W))).astype(np.float32)
    if variance_rows:
        assert M >= 3
        z[0] = 0.75
        z[1] = (1000.0 + rng.standard_normal(W)).astype(np.float32)
        z[2] = (1e-4 * rng.standard_normal(W)).astype(np.float32)
    inp = dict(z=z, gamma=(1.0 + 0.3 * rng.standard_normal(W)).astype(np.float32), beta=(0.2 * rng.standard_normal(W)).astype(np.float32),
               dy=rng.standard_normal((M, W)).astype(np.float32), kind=int(kind))
    saved = ln_fwd(z, inp["gamma"], inp["beta"], kind, F64, float(np.float32(EPS)))
    inp.update({k: saved[k].astype(np.float32) for k in ("y", "xhat", "rstd")})
    return inp


def fwd_refs(inp, eps=float(np.float32(EPS))):
    """(fp32, fp64) forward references; eps is the value a C ``float`` argument carries"""
    a = (inp["z"], inp["gamma"], inp["beta"], inp["kind"])
    return ln_fwd(*a, F32, eps), ln_fwd(*a, F64, eps)


def bwd_refs(inp, init=None):
    a = (inp["dy"], inp["y"], inp["xhat"], inp["rstd"], inp["gamma"], inp["kind"])
    return ln_bwd(*a, F32, init), ln_bwd(*a, F64, init)


def check_fwd(got, inp):
    """got: {"y", "xhat", "rstd"} padded flat buffers -> {array: (err, e32, bound)}"""
    r32, r64 = fwd_refs(inp)
    return {k: within(k, body(k, got[k], r64[k].shape), r32[k], r64[k]) for k in ("y", "xhat", "rstd")}


def check_bwd(got, inp, init=None):
    """got: {"dz", "dgamma", "dbeta"} padded flat buffers; ``init``: what an accumulating call started from"""
    r32, r64 = bwd_refs(inp, init)
    return {k: within(k, body(k, got[k], r64[k].shape), r32[k], r64[k]) for k in ("dz", "dgamma", "dbeta")}


def ratios(res):
    """{array: err / e32} of a comparator's result (inf where the fp32 reference is exact and the kernel is not)"""
    return {k: (err / e32 if e32 else (0.0 if err == 0 else float("inf"))) for k, (err, e32, _b) in res.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------------------------------
BLOCK_TOL, TORCH32 = 2e-5, 3.0        # tests/_gradcheck.py's constants


def flat_with_ln(pol, net):
    """the parameter gradients of a to_torch() module in the layout of pol.grad, widened to fp64, gamma / beta blocks included; a
    parameter the loss does not reach: zeros"""
    g = torch.zeros(pol.n_params, dtype=torch.float64)
    for i, (ly, m) in enumerate(zip(pol.layers, net.lin)):
        if ly.frozen or m.weight.grad is None:
            continue
        g[ly.w_off:ly.w_off + ly.K * ly.No] = m.weight.grad.reshape(-1).double()
        g[ly.b_off:ly.b_off + ly.No] = m.bias.grad.double()
        if ly.ln:
            g[ly.g_off:ly.g_off + ly.No] = net.norm[str(i)].weight.grad.double()
            g[ly.be_off:ly.be_off + ly.No] = net.norm[str(i)].bias.grad.double()
    if net.log_std.grad is not None and pol.n_params > pol.log_std_off:
        g[pol.log_std_off:] = net.log_std.grad.double()
    return g


def network_reference(pol, obs, loss_fn, need_input_grad=True):
    """autograd of ``loss_fn(net, obs)`` over pol.to_torch() on the CPU, in fp64 and in torch's fp32 -> namespace in the layout
    _gradcheck.assert_blocks / assert_rows read: grad, grad32 (flat, fp64 tensors), d_in, d_in32, mean, value, mean32, value32"""
    out = {}
    for tag, dt in (("", torch.float64), ("32", torch.float32)):
        net = pol.to_torch().to(dt)
        xs = {k: v.detach().cpu().to(dt).requires_grad_(bool(need_input_grad)) for k, v in obs.items()}
        loss_fn(net, xs).backward()
        mean, value = net.acts["mean"], net.acts["value"]
        out["grad" + tag] = flat_with_ln(pol, net)
        out["d_in" + tag] = {k: v.grad.double() for k, v in xs.items() if v.grad is not None}
        out["mean" + tag], out["value" + tag] = mean.detach().double(), value.detach().double()
    return types.SimpleNamespace(**out)


def head_loss(d0, d1):
    """sum(mean d0) + sum(value d1); either may be None (that trunk gets no gradient)"""
    def f(net, xs):
        m, v = net(xs)
        loss = 0.0
        if d0 is not None:
            loss = loss + (m * d0.detach().cpu().to(m.dtype)).sum()
        if d1 is not None:
            loss = loss + (v.view(d1.shape) * d1.detach().cpu().to(v.dtype)).sum()
        return loss
    return f


def hold_block(got, want, w32, what, name):
    """|got - want| <= max(BLOCK_TOL max|want|, TORCH32 max|w32 - want|) -> (err, fp32 distance) / max|want|"""
    bs = want.abs().max().item()
    dist = (w32 - want).abs().max().item()
    bound = max(BLOCK_TOL * bs, TORCH32 * dist)
    err = (got - want).abs().max().item()
    assert err <= bound, (what, name, f"err {err:.3e} = {err / max(bs, 1e-300):.3e} of the block's max {bs:.3e}; bound {bound:.3e}",
                          f"torch fp32 {dist:.3e}")
    return err / max(bs, 1e-300), dist / max(bs, 1e-300)


def assert_ln_blocks(pol, grad, ref, what, untouched=0.0):
    """every gamma and every beta block of the flat gradient against `ref` (network_reference), each on its own scale; a block whose
    reference is identically zero -- a trunk without head gradient -- must hold exactly `untouched`"""
    g = grad.detach().double().cpu()[:pol.n_params]
    worst, n = [0.0, 0.0], 0
    for ly in pol.layers:
        if not ly.ln:
            continue
        for kind, lo in (("gamma", ly.g_off), ("beta", ly.be_off)):
            n += 1
            name = f"{ly.src} -> {ly.dst} {kind}"
            want, w32, got = ref.grad[lo:lo + ly.No], ref.grad32[lo:lo + ly.No], g[lo:lo + ly.No]
            if not bool(want.any()):
                assert bool((got == untouched).all()), (what, name, "no gradient reaches this block: it must be left as it was")
                continue
            r = hold_block(got, want, w32, what, name)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    assert n > 0, "no LayerNorm block in this policy"
    print(f"gradcheck gamma / beta blocks {what}: worst err / block max {worst[0]:.3e}, worst torch-fp32 distance / block max {worst[1]:.3e}")
    return tuple(worst)


def assert_heads(mean, value, ref, what):
    """the forward heads on the scale of each head's largest reference entry, with torch's fp32 forward as the yardstick"""
    for name, got, want, w32 in (("mean", mean, ref.mean, ref.mean32), ("value", value, ref.value, ref.value32)):
        r = hold_block(got.detach().double().cpu().view(want.shape), want, w32, what, name)
        print(f"forward {what} {name}: err / max {r[0]:.3e}, torch fp32 {r[1]:.3e}")
