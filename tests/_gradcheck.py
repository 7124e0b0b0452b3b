"""The gradient reference of the MLP kernel tests and the per-block / per-row assertions on it (a plain helper module, like _golden.py).

`pinned_reference` is autograd of MlpPolicy.to_torch() in fp64, given the kernel's side of every ReLU / LeakyReLU unit whose
pre-activation lies within fp32 rounding of zero, next to torch's own fp32 autograd of the same network (the yardstick of what fp32
can do); it runs on whatever device its inputs are on.  `assert_blocks` holds every weight and bias block of the flat gradient to its
OWN largest entry, `assert_rows` every row of an observation gradient to its own: one tolerance over the whole flat gradient is set by
the action head's block alone and lets a per-cent error through in most of the others."""
import types
import warnings

import numpy as np
import torch

BLOCK_TOL = 2e-5          # of the block's largest reference entry
TORCH32 = 3.0             # ... or this many times the distance of torch's fp32 autograd from the fp64 reference on the same block
FLIP_CAP = 1e-6           # of the network's ReLU / LeakyReLU units may be given the kernel's side
PINNED_KINDS = (1, 4)     # VF_ACTIVATION_RELU, _LEAKY_RELU: the derivative jumps at zero (Tanh and ELU are C1)


def torch_activations(pol, net, obs):
    """the layer outputs of `net` (a to_torch() module) on `obs` in the layout of MlpPolicy._buffers: {buffer name: (M, width)} --
    what a test without kernels hands to pinned_reference as `saved`"""
    from visfly_amd.ppo import _TORCH_ACT
    M = next(iter(obs.values())).shape[0]
    out = {name: torch.zeros((M, w), dtype=torch.float32, device=next(iter(obs.values())).device) for name, w in pol.widths.items()}
    hooks = []

    def keep(ly):
        def hook(mod, inp, z):
            y = getattr(torch.nn, _TORCH_ACT[ly.relu])()(z) if ly.relu else z
            out[ly.dst][:, ly.dc:ly.dc + ly.No] = y.detach().float()
        return hook
    for ly, m in zip(pol.layers, net.lin):
        hooks.append(m.register_forward_hook(keep(ly)))
    with torch.no_grad():
        net(obs)
    for h in hooks:
        h.remove()
    return out


def _flat64(pol, net):
    """the parameter gradients of a to_torch() module in the layout of pol.grad, in the module's own precision widened to fp64 (its
    flat_grad() rounds to fp32); a parameter the loss does not reach: zeros"""
    dev = net.lin[0].weight.device
    g = torch.zeros(pol.n_params, dtype=torch.float64, device=dev)
    for ly, m in zip(pol.layers, net.lin):
        if ly.frozen or m.weight.grad is None:
            continue
        g[ly.w_off:ly.w_off + ly.K * ly.No] = m.weight.grad.reshape(-1).double()
        g[ly.b_off:ly.b_off + ly.No] = m.bias.grad.double()
    return g


def pinned_reference(pol, obs, saved, d0, d1, need_input_grad, second_head=True, flip_cap=FLIP_CAP, pin_torch32=True):
    """gradients of  sum(mean * d0) + sum(value * d1)  (`second_head` False: of the first term alone -- d1 may then be None and the
    value trunk's blocks are identically zero) over the network of `pol`, from autograd of to_torch() in fp64 on the device of `obs`.

    ReLU / LeakyReLU: a unit whose pre-activation lies within fp32 rounding of zero can be on in fp32 and off in fp64 (or the reverse);
    that one unit then moves whole gradient entries by ~1 / M, far above the rounding the bounds are about.  So the fp64 network is
    given the side that `saved` -- the kernel's saved activations, MlpPolicy._buffers(M, slot) after forward -- shows for exactly those
    units.  Every such unit must have |z| below the forward tolerance of the layer entry points (1e-5 sqrt(K), relative to 1 + the
    row's largest |z|), and there may be at most `flip_cap` of the network's ReLU / LeakyReLU units of them (fp32 torch itself:
    3.6e-8 of them at 131 072 rows); else it is an error of the forward and the assertion here fails.  `pin_torch32`: torch's fp32
    network is given the same sides, so that its distance from the fp64 one is rounding alone as well (one unit of its own on the
    other side puts that distance at 1e-3 of a block and the bound made of it far above the 2e-5).

    -> namespace: grad (flat fp64, pol.n_params; log_std entries zero), d_in {obs key: fp64 gradient} (need_input_grad), grad32 / d_in32
    (the same from torch's fp32 autograd, widened), mean / value (fp64 forward), flips, units"""
    dev = next(iter(obs.values())).device
    ref = pol.to_torch().double().to(dev)
    flips, units = [], 0

    def side_of_kernel(ly, count=True):
        def hook(mod, inp, z):
            on = saved[ly.dst][:, ly.dc:ly.dc + ly.No] > 0
            flip = on != (z > 0)
            if count and bool(flip.any()):
                lim = 1e-5 * np.sqrt(ly.K) * (1 + z.detach().abs().max(dim=1, keepdim=True).values)
                assert bool((z.detach().abs() <= lim)[flip].all()), (ly.dst, float(z.detach().abs()[flip].max()))
                flips.append(int(flip.sum()))
            # the derivative of the kernel's side (ReLU 1 | 0, LeakyReLU 1 | slope) there, the value stays ~0
            tiny = 1e-300 if z.dtype == torch.float64 else 1e-30
            side = torch.where(on, torch.full_like(z, tiny), torch.full_like(z, -tiny))
            return torch.where(flip, side + (z - z.detach()), z)
        return hook
    hooks = []
    for ly, m in zip(pol.layers, ref.lin):
        if ly.relu in PINNED_KINDS:
            hooks.append(m.register_forward_hook(side_of_kernel(ly)))
            units += ly.No
    M = next(iter(obs.values())).shape[0]
    units *= M
    xs = {k: v.double().requires_grad_(bool(need_input_grad)) for k, v in obs.items()}
    m0, v0 = ref(xs)
    loss = (m0 * d0.double()).sum()
    if second_head:
        loss = loss + (v0.view(d1.shape) * d1.double()).sum()
    loss.backward()
    for h in hooks:
        h.remove()
    print(f"ReLU units the fp64 reference was given the kernel's side of: {sum(flips)} of {units}")
    if flip_cap is not None:
        assert sum(flips) <= flip_cap * units, ("units on the other side of zero than in fp64", sum(flips), units)
    ref32 = pol.to_torch().to(dev)
    if pin_torch32:
        for ly, m in zip(pol.layers, ref32.lin):
            if ly.relu in PINNED_KINDS:
                m.register_forward_hook(side_of_kernel(ly, count=False))
    x32 = {k: v.clone().requires_grad_(bool(need_input_grad)) for k, v in obs.items()}
    m32, v32 = ref32(x32)
    loss = (m32 * d0).sum()
    if second_head:
        loss = loss + (v32.view(d1.shape) * d1).sum()
    loss.backward()
    grads = lambda x: {k: v.grad.double() for k, v in x.items() if v.grad is not None}
    return types.SimpleNamespace(grad=_flat64(pol, ref), d_in=grads(xs), grad32=_flat64(pol, ref32), d_in32=grads(x32),
                                 mean=m0.detach(), value=v0.detach(), flips=sum(flips), units=units)


def _blocks(pol):
    for ly in pol.layers:
        if not ly.frozen:
            yield ly, "w", ly.w_off, ly.w_off + ly.K * ly.No
            yield ly, "b", ly.b_off, ly.b_off + ly.No


def _ragged(ly, kind, t):
    """the entries of a block that the last, ragged 32-wide tile of the layer produces, as (name, vector) pairs: of the weight matrix
    every input column K - K % 32 .. K and every output unit's row No - No % 32 .. No on its own (vectors of No / K entries), of the
    bias the ragged units' entries together (a lone entry is a sum that can cancel to any fraction of its terms: no scale of its own)"""
    if kind == "b":
        return [(f"units {ly.No - ly.No % 32}..{ly.No}", t[ly.No - ly.No % 32:])] if ly.No % 32 else []
    w = t.view(ly.No, ly.K)
    out = [(f"input column {k}", w[:, k]) for k in range(ly.K - ly.K % 32, ly.K)] if ly.K % 32 else []
    return out + ([(f"output unit {n}", w[n]) for n in range(ly.No - ly.No % 32, ly.No)] if ly.No % 32 else [])


def assert_blocks(pol, grad, ref, what, floor=0.0, untouched=0.0, tol=BLOCK_TOL):
    """every weight block and every bias block of every non-frozen layer of the flat gradient `grad` against `ref` (pinned_reference):
    |err| <= max(tol * the block's own largest reference entry, 3 * the distance of torch's fp32 autograd from fp64 on that block).
    No floor tied to the global maximum unless `floor` says so (the wide-layer tests: 1e-3 of it).  A block whose reference is
    identically zero -- a trunk without head gradient -- must hold exactly `untouched`, what the test put there before the call.
    Where K or No is no multiple of 32, every input column / output unit of the ragged tile is held to the same bound on its own
    largest entry.  -> (worst err / block max, worst fp32-torch distance / block max), also printed"""
    g = grad.detach().double()[:pol.n_params].to(ref.grad.device)
    gmax = ref.grad.abs().max().item()
    worst = [0.0, 0.0]

    def hold(got, want, w32, name, lo_floor):
        bs = max(want.abs().max().item(), lo_floor)
        dist = (w32 - want).abs().max().item()
        bound = max(tol * bs, TORCH32 * dist)
        err = (got - want).abs().max().item()
        assert err <= bound, (what, name, f"err {err:.3e} = {err / bs:.3e} of the block's max {bs:.3e}; bound {bound / bs:.3e} of it",
                              f"torch fp32 {dist / bs:.3e}")
        worst[0], worst[1] = max(worst[0], err / bs), max(worst[1], dist / bs)

    for ly, kind, lo, hi in _blocks(pol):
        name = f"{ly.src} -> {ly.dst} {kind}"
        want, w32, got = ref.grad[lo:hi], ref.grad32[lo:hi], g[lo:hi]
        if floor == 0.0 and not bool(want.any()):
            assert bool((got == untouched).all()), (what, name, "no gradient reaches this block: it must be left as it was")
            continue
        hold(got, want, w32, name, floor * gmax)
        if floor == 0.0:
            for (part, gp), (_, wp), (_, w32p) in zip(_ragged(ly, kind, got), _ragged(ly, kind, want), _ragged(ly, kind, w32)):
                if bool(wp.any()):
                    hold(gp, wp, w32p, name + ", " + part, 0.0)
                else:
                    assert bool((gp == untouched).all()), (what, name, part)
    print(f"gradcheck blocks {what}: worst err / block max {worst[0]:.3e}, worst torch-fp32 distance / block max {worst[1]:.3e}")
    return tuple(worst)


def assert_rows(got, ref, ref32, what=""):
    """an observation gradient, every element: |err| <= max(1e-4 |want| + 1e-5 * that row's largest |want|, 3 * the distance of
    torch's fp32 autograd from fp64 on that row); no row is exempt"""
    want, got = ref.double(), got.detach().double().to(ref.device)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    rmax = want.abs().max(dim=1, keepdim=True).values
    dist = (ref32.double() - want).abs().max(dim=1, keepdim=True).values
    bound = torch.maximum(1e-4 * want.abs() + 1e-5 * rmax, TORCH32 * dist)
    bad = (err > bound).any(dim=1)
    rel = (err.max(dim=1, keepdim=True).values / rmax.clamp_min(1e-300)).max().item()
    print(f"gradcheck rows {what}: worst err / row max {rel:.3e}, worst torch-fp32 distance / row max "
          f"{(dist / rmax.clamp_min(1e-300)).max().item():.3e}")
    assert not bool(bad.any()), (what, f"{int(bad.sum())} rows outside their bound, first {int(bad.nonzero()[0])}",
                                 f"worst err / row max {rel:.3e}")
    return rel


def assert_blocks_agree(pol, g1, g0, tol, what):
    """two implementations of the same flat gradient (a fused step and its separate launches), block by block: each block of g1 within
    `tol` of that block's own largest entry in g0"""
    worst = 0.0
    for ly, kind, lo, hi in _blocks(pol):
        bs = g0[lo:hi].abs().max().item()
        err = (g1[lo:hi] - g0[lo:hi]).abs().max().item()
        assert err <= tol * bs, (what, f"{ly.src} -> {ly.dst} {kind}", f"diff {err:.3e} = {err / max(bs, 1e-300):.3e} of the block's max")
        worst = max(worst, err / max(bs, 1e-300))
    print(f"gradcheck fused vs separate {what}: worst diff / block max {worst:.3e}")
    return worst


def check_policy_vs_autograd(pol, obs, d0, d1, need_input_grad=True):
    """forward and backward(need_input_grad) of a layer-by-layer network against the pinned fp64 reference; every parameter block
    and every observation gradient is held to 2e-5 of its scale (a block's: at least 1e-3 of the largest gradient entry) OR three
    times the distance of torch's own fp32 autograd from the fp64 reference, whichever is larger (mode (c) of
    test_ppo_gpu.py::test_policy_with_other_activations_vs_torch); two runs are bit-identical"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mean, value = pol.forward(obs)
    mean, value = mean.clone(), value.clone()
    M = mean.shape[0]
    ref = pinned_reference(pol, obs, pol._buffers(M, 0), d0, d1, True, flip_cap=None, pin_torch32=False)
    m0, v0 = ref.mean, ref.value
    sc = max(m0.abs().max().item(), v0.abs().max().item(), 1e-3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        e = max((mean.double() - m0).abs().max().item(), (value.double() - v0.view(value.shape)).abs().max().item())
        print(f"forward: max abs err {e:.3e} of scale {sc:.3e}")
        assert e <= 4e-6 * sc
        d_in = pol.backward(d0, d1, None, need_input_grad=need_input_grad)
    assert_blocks(pol, pol.grad, ref, "layer by layer", floor=1e-3)
    for k, v in d_in.items():
        if k not in ref.d_in:
            continue
        bound = max(2e-5 * max(ref.d_in[k].abs().max().item(), 1e-12), 3.0 * (ref.d_in32[k] - ref.d_in[k]).abs().max().item())
        assert (v.double() - ref.d_in[k]).abs().max().item() <= bound, k
    g1 = pol.grad.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pol.forward(obs)
        pol.backward(d0, d1, None, need_input_grad=need_input_grad)
    assert torch.equal(g1, pol.grad), "two runs differ"
