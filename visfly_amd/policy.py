"""The MLP policy every trainer shares: PPO's actor-critic, the actor of BPTT and SHAC, SHAC's twin critic.

Restates the reference's ``CustomMultiInputActorCriticPolicy`` with ``StateExtractor`` / ``StateTargetExtractor`` /
``StateGateExtractor`` MLPs (utils/policies/policies.py:195-254, utils/policies/extractors.py:376-449,578-592,662-678,752-761; the last
one reads the racing envs' "gate" index as one float column that holds the index the observation's "state" rows were formed with --
the agent's current gate, ``terminal_gate`` for a terminal row): the layer schedule, the flat parameter buffer, and the host side of
every forward / backward launch over it (vf_mlp_* / vf_linear_* / vf_layernorm_* of the C-ABI).  No trainer and no archive format
is known here: the trainers, evaluate.py and checkpoint.py import this module, never the other way round.
"""
import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch as th

from . import _jit, _lib


def _ptr(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


# create_mlp's activation_fn (utils/policies/extractors.py:376-449) under the aliases of CustomMultiInputActorCriticPolicy
# (utils/policies/policies.py:64-69) -> VF_ACTIVATION_* of include/visfly_amd.h; ACTIVATION_NAMES: the inverse, the names of ``spec``
ACTIVATIONS = {"relu": 1, "tanh": 2, "elu": 3, "leaky_relu": 4}
ACTIVATION_NAMES = {v: k for k, v in ACTIVATIONS.items()}
_TORCH_ACT = {1: "ReLU", 2: "Tanh", 3: "ELU", 4: "LeakyReLU"}

# weight_grad_slots: rows per weight-gradient launch of a horizon (profiles/r06_bptt_wgrad_chunks.txt)
WGRAD_SPLIT_ROWS = 524288

# nn.LayerNorm's eps in create_mlp (utils/policies/extractors.py:429)
LN_EPS = 1e-3

# widest layer (in or out) of an MlpPolicy: the per-layer kernels' limit (vf_linear_*: K, No <= 512) / of a network the one-launch,
# register-chained and persistent kernels can run (K, No <= 128: vf_linear_is_wide)
MAX_WIDTH, FUSED_MAX_WIDTH = 512, 128


# observation keys a trainer may feed its policy, and the ones among them that are integer indices: fed as one exact float32 column
# (SB3's preprocess_obs is .float() for a Box space), never differentiated
POLICY_OBS_KEYS = ("state", "target", "gate")
INDEX_OBS_KEYS = ("gate",)


def obs_width(t) -> int:
    """columns of an observation entry as the policy reads it (RacingEnv's "gate" is (N,): one column)"""
    return 1 if t.dim() == 1 else int(t.shape[1])


def policy_rows(obs, keys):
    """{key: the (N, w) contiguous float32 rows the policy reads} of an env observation.  "gate" (int32, (N,) from RacingEnv, (N, 1)
    from RacingEnv2) becomes an (N, 1) float32 column holding the index exactly; float entries are passed as they are"""
    out = {}
    for k in keys:
        t = obs[k].detach()
        if k in INDEX_OBS_KEYS:
            t = t.reshape(t.shape[0], -1).to(th.float32)
        out[k] = t.contiguous()
    return out


def activation_kind(a) -> int:
    """'relu' / 'Tanh' / nn.ELU / nn.LeakyReLU() ... -> VF_ACTIVATION_*"""
    if isinstance(a, int):
        if a in _TORCH_ACT:
            return a
        raise ValueError(f"activation kind {a}")
    name = a if isinstance(a, str) else getattr(a, "__name__", type(a).__name__)
    key = name.lower().replace("leakyrelu", "leaky_relu")
    if key not in ACTIVATIONS:
        raise NotImplementedError(f"activation_fn {name}: the MLP kernels implement {sorted(ACTIVATIONS)} (policies.py:64-69)")
    return ACTIVATIONS[key]


class _Linear:
    """one nn.Linear (+ activation) of the schedule: reads src[:, sc:sc+K], writes dst[:, dc:dc+No]; ``relu``: the activation kind
    (VF_ACTIVATION_*: 0 none, 1 ReLU, 2 Tanh, 3 ELU, 4 LeakyReLU -- the name is the ABI's)"""

    def __init__(self, K, No, relu, src, sc, dst, dc, w_off, b_off, first):
        self.K, self.No, self.relu = K, No, relu
        self.src, self.sc, self.dst, self.dc = src, sc, dst, dc
        self.w_off, self.b_off, self.first = w_off, b_off, first
        self.frozen = False       # identity pass-through (MlpPolicy ``passthrough``): no gradient, not in the backward tables
        # nn.LayerNorm(No, eps=1e-3) between the Linear and its activation (create_mlp's ``ln``): gamma / beta sit right behind the
        # layer's own bias in ``flat`` (g_off, be_off); ``ln_key`` names the layer's pre-norm / rstd buffers
        self.ln, self.g_off, self.be_off, self.ln_key = False, None, None, None
        # separate pi / vf extractors (MlpPolicy ``vf_extractor``): the side of the network the layer belongs to ("pi" / "vf"); None in a
        # network with a shared extractor, whose extractor layers serve both trunks
        self.side = None
        self.ext = False          # a layer of an extractor MLP (either side's)


class MlpPolicy:
    """Actor-critic MLP over dict observations of flat vectors.

    ``extractor``: {obs key: hidden layer sizes} -- one ReLU MLP per key, outputs concatenated
    (StateExtractor / StateTargetExtractor); ``pi`` / ``vf``: hidden sizes of the policy / value
    trunks (MlpExtractor2); heads: action_net (-> 4) and value_net (-> 1); state-independent
    ``log_std`` (4), tanh-squashed Gaussian (policies.py:114,177-181).  All parameters live in one
    flat fp32 device buffer (weights [No][K] row-major like nn.Linear, then biases, ... , log_std).
    """

    def __init__(self, obs_dims: Dict[str, int], extractor: Dict[str, List[int]], pi: List[int], vf: List[int],
                 device, action_dim: int = 4, log_std_init: float = 0.0, seed: int = 0, ortho_init: bool = True,
                 head_dims=None, passthrough=(), log_std_param: bool = True, activation="relu", extractor_activation="relu",
                 layer_norm=None, vf_extractor=None, vf_extractor_activation=None):
        """``head_dims`` (default (action_dim, 1)): widths of the two heads "mean" / "value" -- the SHAC actor of the reference
        has two 4-wide heads (mu and a state-dependent log_std, utils/policies/td_policies.py:230-243), its twin critic two
        1-wide ones.  ``passthrough``: input keys whose columns are appended to the features unchanged, after the extractor
        outputs -- ``th.cat([features, actions], dim=-1)`` of ContinuousCritic.forward (:137); realised as a frozen identity
        layer (W = I, b = 0: exact in fp32) whose parameters sit BEHIND the trainable ones in ``flat`` and never receive a
        gradient.  ``log_std_param`` False: no state-independent log_std parameter.
        ``activation`` / ``extractor_activation``: activation of the trunks' hidden layers (the policy's ``activation_fn``,
        policies.py:108: the reference's default there is Tanh) and of the extractor MLPs (``features_extractor_kwargs.activation_fn``,
        extractors.py:560,583: default ReLU): relu | tanh | elu | leaky_relu.  The register-chained classes built into the library are
        ReLU networks; for another activation the class is generated and compiled on first use like a non-default net_arch
        (visfly_amd/_jit.py: the activation is part of the class), else the block-tile kernels run it.
        ``layer_norm``: dict(extractor={key: bool}, pi=bool, vf=bool) -- create_mlp's ``ln`` (extractors.py:428-430; the YAMLs'
        features_extractor_kwargs.net_arch.<key>.ln and net_arch.pi_ln / vf_ln): nn.LayerNorm(width, eps=1e-3) between every hidden
        Linear of that MLP and its activation; the heads are never normalised.  gamma (ones) and beta (zeros) follow the layer's own
        weight and bias in ``flat``: W, b, gamma, beta.  Such a network has no fused plan: it runs layer by layer on vf_linear_* with
        vf_layernorm_* in between (csrc/vf_layernorm.hip).  None / all flags false: the network, its parameter layout and its path
        are exactly what they are without the argument.
        ``vf_extractor`` ({obs key: hidden sizes}, like ``extractor``) [+ ``vf_extractor_activation``, default: the pi side's]: the
        critic gets a feature extractor of its own -- the reference's ``share_features_extractor=False`` (SB3 builds a second instance
        of the extractor class) and its ``pi_features_extractor_class`` / ``vf_features_extractor_class`` (policies.py:117-175: the two
        sides may differ in class and net_arch, e.g. an asymmetric critic that also reads "target").  ``extractor`` then feeds the pi
        trunk only (buffers ``x:<key>:<i>`` / ``feat`` as ever), ``vf_extractor`` the vf trunk only (``vx:<key>:<i>`` / ``vfeat``);
        ``flat`` holds: pi extractor layers, vf extractor layers, pi trunk + mean head, vf trunk + value head, log_std; ``obs_keys`` =
        the pi side's keys, then the keys only the vf side reads.  Actor-critic heads (4, 1) with the log_std parameter only, without
        pass-through inputs and LayerNorm.  Two independent pipelines: on the chain kernels they are the two waves of one workgroup
        (csrc/vf_mlp_chain_sep.hpp; generated on first use like any non-default shape).  None: the network, its parameter layout, its
        spec and its path are exactly what they are without the argument."""
        assert action_dim == 4, "the head kernels are written for the 4-d drone action"
        self.device = th.device(device)
        self.passthrough = [k for k in passthrough]
        self.sep = vf_extractor is not None
        if self.sep:
            hd = tuple(head_dims) if head_dims is not None else (action_dim, 1)
            bad = [n for n, c in (("passthrough inputs", bool(self.passthrough)), (f"head_dims {hd}", hd != (4, 1)),
                                  ("log_std_param=False", not log_std_param),
                                  ("layer_norm", bool(layer_norm) and (any((layer_norm.get("extractor") or {}).values()) or
                                                                        layer_norm.get("pi") or layer_norm.get("vf")))) if c]
            if bad:
                raise NotImplementedError(f"vf_extractor (separate pi / vf feature extractors) with {', '.join(bad)} is not implemented: "
                                          "the PPO actor-critic (heads (4, 1), log_std parameter) without pass-through inputs or LayerNorm only")
            if not vf_extractor:
                raise ValueError("vf_extractor: at least one observation branch")
            vf_extractor = {k: list(v) for k, v in vf_extractor.items()}
        self.obs_keys = list(extractor.keys()) + self.passthrough + [k for k in (vf_extractor or {}) if k not in extractor]
        self.obs_dims = {k: int(obs_dims[k]) for k in self.obs_keys}
        self.head_dims = tuple(head_dims) if head_dims is not None else (action_dim, 1)
        self.act, self.ext_act = activation_kind(activation), activation_kind(extractor_activation)
        self.spec = dict(extractor={k: list(v) for k, v in extractor.items()}, pi=list(pi), vf=list(vf))
        if (self.act, self.ext_act) != (1, 1):        # (archives of ReLU networks keep the r05 spec)
            self.spec.update(activation=ACTIVATION_NAMES[self.act], extractor_activation=ACTIVATION_NAMES[self.ext_act])
        self.vf_ext_act = self.ext_act if vf_extractor_activation is None else activation_kind(vf_extractor_activation)
        if self.sep:
            self.spec["vf_extractor"] = {k: list(v) for k, v in vf_extractor.items()}
            if self.vf_ext_act != self.ext_act:
                self.spec["vf_extractor_activation"] = ACTIVATION_NAMES[self.vf_ext_act]
        ln = dict(layer_norm or {})
        unknown = set(ln) - {"extractor", "pi", "vf"} | set(ln.get("extractor") or {}) - set(extractor)
        if unknown:
            raise ValueError(f"layer_norm: unknown entries {sorted(unknown)} (dict(extractor={{key: bool}}, pi=bool, vf=bool))")
        ln_ext = {k: bool((ln.get("extractor") or {}).get(k, False)) for k in extractor}
        ln_trunk = {"pi": bool(ln.get("pi", False)), "vf": bool(ln.get("vf", False))}
        self.ln = any(ln_ext.values()) or any(ln_trunk.values())
        if self.ln:                                   # (archives of networks without LayerNorm keep their spec)
            self.spec["layer_norm"] = dict(extractor=ln_ext, pi=ln_trunk["pi"], vf=ln_trunk["vf"])
        # ---- activation buffers (name -> width) and the layer schedule ----
        self.widths: Dict[str, int] = {}
        self.layers: List[_Linear] = []
        off = 0

        def add(K, No, relu, src, sc, dst, dc, first=False, ln=False):
            nonlocal off
            self.layers.append(_Linear(K, No, relu, src, sc, dst, dc, off, off + K * No, first))
            off += K * No + No
            if ln:
                ly = self.layers[-1]
                ly.ln, ly.g_off, ly.be_off, ly.ln_key = True, off, off + No, f"{dst}:{dc}"
                off += 2 * No

        feat_w = sum((v[-1] if v else self.obs_dims[k]) for k, v in extractor.items()) + sum(self.obs_dims[k] for k in self.passthrough)
        self.widths["feat"] = feat_w
        def lay_extractor(branches, prefix, feat, act, ln_of, side):
            """one extractor: an MLP per observation key (hidden buffers <prefix>:<key>:<i>), the last layers side by side in `feat`
            -> the columns they fill"""
            col = 0
            for k, hidden in branches.items():
                src, sc, K = "obs:" + k, 0, self.obs_dims[k]
                if not hidden:
                    raise NotImplementedError("identity extractor branches are not supported")
                for li, h in enumerate(hidden):
                    last = li == len(hidden) - 1
                    dst = feat if last else f"{prefix}:{k}:{li}"
                    dc = col if last else 0
                    if not last:
                        self.widths[dst] = h
                    add(K, h, act, src, sc, dst, dc, first=(li == 0), ln=ln_of.get(k, False))
                    self.layers[-1].ext, self.layers[-1].side = True, side
                    src, sc, K = dst, dc, h
                col += hidden[-1]
            return col

        col = lay_extractor(extractor, "x", "feat", self.ext_act, ln_ext, "pi" if self.sep else None)
        # the vf side's extractor: buffers of its own (vx:<key>:<i>, vfeat); no buffer of either side has two readers
        vfeat_w = 0
        if self.sep:
            vfeat_w = self.widths["vfeat"] = sum(v[-1] for v in vf_extractor.values() if v)
            lay_extractor(vf_extractor, "vx", "vfeat", self.vf_ext_act, {}, "vf")
        pass_cols = []
        for k in self.passthrough:
            pass_cols.append((k, col))
            col += self.obs_dims[k]
        for trunk, hidden, head_dim, head in (("pi", pi, self.head_dims[0], "mean"), ("vf", vf, self.head_dims[1], "value")):
            src, sc, K = ("vfeat", 0, vfeat_w) if self.sep and trunk == "vf" else ("feat", 0, feat_w)
            for li, h in enumerate(hidden):
                dst = f"{trunk}:{li}"
                self.widths[dst] = h
                add(K, h, self.act, src, sc, dst, 0, ln=ln_trunk[trunk])
                self.layers[-1].side = trunk if self.sep else None
                src, sc, K = dst, 0, h
            self.widths[head] = head_dim
            add(K, head_dim, 0, src, sc, head, 0)
            self.layers[-1].side = trunk if self.sep else None
        self.log_std_off = off
        self.n_params = off + (action_dim if log_std_param else 0)      # trainable parameters (what Adam / the all-reduce see)
        # frozen identity layers of the pass-through inputs: executed with the extractors, parameters behind the trainable ones
        off = self.n_params
        n_ext = sum(len(v) for v in extractor.values()) + sum(len(v) for v in (vf_extractor or {}).values())
        for j, (k, c) in enumerate(pass_cols):
            d = self.obs_dims[k]
            ly = _Linear(d, d, 0, "obs:" + k, 0, "feat", c, off, off + d * d, True)
            ly.frozen = True
            self.layers.insert(n_ext + j, ly)
            off += d * d + d
        self.n_total = off
        for ly in self.layers:
            if ly.K > MAX_WIDTH or ly.No > MAX_WIDTH:
                raise ValueError(f"layer widths up to {MAX_WIDTH} are supported by the MFMA linear kernels (layer {ly.src} -> {ly.dst} is {ly.K} -> {ly.No}"
                                 + (f": the extractor outputs {feat_w - sum(self.obs_dims[k] for k in self.passthrough)} features (+) "
                                    f"{sum(self.obs_dims[k] for k in self.passthrough)} pass-through columns -- narrow the extractors' last layers"
                                    if self.passthrough and ly.K == feat_w else "") + ")")
        # ---- parameters, reproducible from `seed`.  ortho_init (the reference's default, policies.py:109): SB3's
        # ActorCriticPolicy._build -- orthogonal weights with gain sqrt(2) for the extractor and trunk layers, 0.01 for
        # action_net, 1 for value_net, zero biases; otherwise nn.Linear's default (kaiming-uniform) ----
        g = th.Generator().manual_seed(seed)
        flat = th.zeros(self.n_total)
        self.ortho_init = bool(ortho_init)
        for ly in self.layers:
            if ly.frozen:
                flat[ly.w_off:ly.w_off + ly.K * ly.No] = th.eye(ly.K).reshape(-1)
                continue
            if ly.ln:        # nn.LayerNorm's own initialisation; SB3's orthogonal init touches nn.Linear only
                flat[ly.g_off:ly.g_off + ly.No] = 1.0
            if ortho_init:
                gain = {"mean": 0.01, "value": 1.0}.get(ly.dst, float(np.sqrt(2.0)))
                w = th.empty(ly.No, ly.K)
                th.nn.init.orthogonal_(w, gain=gain, generator=g)
                flat[ly.w_off:ly.w_off + ly.K * ly.No] = w.reshape(-1)
            else:
                bound = 1.0 / np.sqrt(ly.K)
                flat[ly.w_off:ly.w_off + ly.K * ly.No] = (th.rand(ly.K * ly.No, generator=g) * 2 - 1) * bound
                flat[ly.b_off:ly.b_off + ly.No] = (th.rand(ly.No, generator=g) * 2 - 1) * bound
        flat[self.log_std_off:self.n_params] = log_std_init
        self.flat = flat.to(self.device)
        self.grad = th.zeros(self.n_params, device=self.device)
        self._bufs: Dict[tuple, Dict[str, th.Tensor]] = {}
        self._gbufs: Dict[int, Dict[str, th.Tensor]] = {}
        self._scratch = None
        # a layer wider than 128 in or out: only the per-layer entry points (vf_linear_*) have kernels for it -- operands streamed
        # instead of a resident weight matrix (csrc/vf_linear_wide.hip); the one-launch kernels, the chain classes and the persistent
        # horizons stop at 128, so such a network has no plan and runs layer by layer like one with too many buffers
        self.wide = any(ly.K > FUSED_MAX_WIDTH or ly.No > FUSED_MAX_WIDTH for ly in self.layers)
        # LayerNorm (``self.ln``): the one-launch, chain and persistent kernels have no normalisation step -- no plan either, the
        # layers run one by one with vf_layernorm_fwd / _bwd between them
        self._plan = None if (self.wide or self.ln) else self._plan_fused()
        self._descs = {}
        # chain kernels of a shape the library holds no instance of: compiled on first use (visfly_amd/_jit.py)
        # (heads (4, 1) with the log_std parameter: the PPO policies' actor-critic; (4, 4) without: the SAC-style Actor of BPTT / SHAC;
        # (1, 1) without, behind a pass-through action input: its twin critic)
        if self.sep:
            self.chain_shape = _jit.shape_of(self.obs_dims, extractor, pi, vf, self.head_dims, self.passthrough, acts=(self.act, self.ext_act),
                                             vf_extractor=vf_extractor, vf_extractor_act=self.vf_ext_act)
        else:
            self.chain_shape = (_jit.shape_of(self.obs_dims, extractor, pi, vf, self.head_dims, self.passthrough, acts=(self.act, self.ext_act))
                                if bool(log_std_param) == (self.head_dims == (4, 1)) else None)
        self.chain_jit = False
        if self._plan is None:          # more activation buffers than a vf_mlp_desc names (VF_MLP_MAX_BUFS): layer-by-layer launches
            self.chain_shape = None
        if self.chain_shape is not None and not _jit.is_builtin(self.chain_shape) and self.device.type == "cuda":
            try:
                self.chain_jit = _jit.ensure(self.chain_shape)
            except Exception as e:      # no hipcc on this machine, a shape the compiler rejects, ...: the block-tile kernels run it
                import warnings
                warnings.warn(f"visfly_amd: no chain kernels for {_jit.name_of(self.chain_shape)} ({e})")
        self.fused = True
        self.fused_backward = True
        self._packed, self._pack_desc, self._stamp, self._packed_stamp, self.lazy_pack = None, None, 0, -1, False
        self._pack_map = None
        self._pi_only_ok = True
        self._fused_ppo = None             # None: untried, False: vf_ppo_update does not support this network
        self._fused_twin_q = None          # the same for vf_twin_q_update (a twin critic's fused update step)
        self._steps_ok, self._steps_out = None, {}      # vf_mlp_forward_steps (forward_steps)
        self._act_fused = None             # likewise for vf_mlp_forward_act
        self._sq_part = None
        self._slot_blocks: Dict[int, tuple] = {}

    def _warn_fallback(self, what):
        """the register-chained kernels exist for the reference-default shapes (instantiated in the library) and for every shape
        visfly_amd/_jit.py can generate an instance of (1-2 observation branches, 1-4 layers per branch / trunk, widths in multiples
        of 32 up to 128: compiled on first use); any other net_arch runs on the general block-tile / per-layer kernels -- correct,
        but at roughly half the MFMA throughput.  Say so once instead of silently."""
        if not getattr(self, "_warned_fallback", False):
            self._warned_fallback = True
            import warnings
            if self.ln:
                warnings.warn(f"visfly_amd: {what}: this network has layer norm (nn.LayerNorm in {self.spec['layer_norm']}); networks "
                              "with LayerNorm run layer by layer on the per-layer MFMA linear kernels with the row-wise LayerNorm "
                              "kernels in between -- no one-launch, register-chained or persistent path", stacklevel=3)
                return
            if self.wide:
                warnings.warn(f"visfly_amd: {what}: this network has layers wider than {FUSED_MAX_WIDTH} "
                              f"(extractor {self.spec['extractor']}, pi {self.spec['pi']}, vf {self.spec['vf']}); they run layer by layer "
                              "on the wide (streamed-operand) MFMA linear kernels -- no one-launch, register-chained or persistent path",
                              stacklevel=3)
                return
            warnings.warn(f"visfly_amd: {what} has no register-chained instance for this network "
                          f"(extractor {self.spec['extractor']}, pi {self.spec['pi']}, vf {self.spec['vf']}); "
                          "falling back to the block-tile MFMA kernels (about half the throughput)", stacklevel=3)

    def _plan_fused(self):
        """LDS layout for the one-launch forward (vf_mlp_forward): every activation gets a [64][w|1] region
        (odd row stride); regions are recycled once their last reader has run (first fit over a coalescing
        free list).  The weights do not occupy LDS (packed copy in global memory, read as the MFMA B operand).
        None if the activations do not fit the 160 KiB LDS -> layer-by-layer launches."""
        rows = 64
        odd = lambda w: ((w + 15) & ~15) + 1                      # odd stride covering the width padded to 16
        names = ["obs:" + k for k in self.obs_keys]
        if len(names) > 4 or len(self.layers) > _lib.MLP_MAX_LAYERS:
            return None
        last_read = {}
        for li, ly in enumerate(self.layers):
            last_read[ly.src] = li
        ids, off, stride, size = {}, {}, {}, {}
        free, top = [], 0

        def release(o, n):
            free.append((o, n))
            free.sort()
            merged = []
            for fo, fs in free:
                if merged and merged[-1][0] + merged[-1][1] == fo:
                    merged[-1] = (merged[-1][0], merged[-1][1] + fs)
                else:
                    merged.append((fo, fs))
            free[:] = merged

        def alloc(name, w):
            nonlocal top
            st = odd(w)
            need = rows * st
            for fi, (fo, fs) in enumerate(free):
                if fs >= need:
                    free.pop(fi)
                    if fs > need:
                        release(fo + need, fs - need)
                    off[name], stride[name], size[name] = fo, st, need
                    return
            off[name], stride[name], size[name] = top, st, need
            top += need

        for bi, n in enumerate(names):
            ids[n] = bi
            alloc(n, self.obs_dims[n[4:]])
        nxt = 4
        for li, ly in enumerate(self.layers):
            if ly.dst not in ("mean", "value") and ly.dst not in ids:
                ids[ly.dst] = nxt
                nxt += 1
                alloc(ly.dst, self.widths[ly.dst])
            for n in list(off):            # release regions nobody reads any more (never the one being written)
                if last_read.get(n, -1) <= li and n in size and n != ly.dst and n not in ("mean", "value"):
                    release(off[n], size.pop(n))
        if nxt > _lib.MLP_MAX_BUFS:
            return None
        if top * 4 > 160 * 1024:
            return None
        wt_off, wb_off, wr_off, wq_off, o = [], [], [], [], 0
        for ly in self.layers:               # packed weights: forward [round16(K)][round32(No)], data gradient [round16(No)][round32(K)],
            wt_off.append(o)                 # register-chain image: ceil(No / 32) * G blocks of 256 floats (include/visfly_amd.h)
            o += ((ly.K + 15) & ~15) * ((ly.No + 31) & ~31)
            wb_off.append(o)
            o += ((ly.No + 15) & ~15) * ((ly.K + 31) & ~31)
            wr_off.append(o)
            o += ((ly.No + 31) >> 5) * self._chain_groups(ly) * 256
            wq_off.append(o)                 # reverse-chain image: ceil(K / 32) * ceil(No / 8) blocks
            o += ((ly.K + 31) >> 5) * ((ly.No + 7) >> 3) * 256
        return dict(ids=ids, off=off, stride=stride, total=top, wt_off=wt_off, wb_off=wb_off, wr_off=wr_off, wq_off=wq_off,
                    packed_floats=o)

    @staticmethod
    def _chain_groups(ly):
        """reduction groups (of 8) of a layer's register-chain image: observation layers keep the natural k order"""
        return (ly.K + 7) >> 3 if ly.first else ((ly.K + 31) >> 5) * 4

    def _fused_desc(self, b, save: bool):
        p = self._plan
        d = _lib.MlpDesc()
        d.n_layers, d.n_inputs = len(self.layers), len(self.obs_keys)
        d.identity_mask = sum(1 << i for i, ly in enumerate(self.layers) if ly.frozen)
        for i, k in enumerate(self.obs_keys):
            d.in_dim[i] = self.obs_dims[k]
        for n, bid in p["ids"].items():
            d.lds_off[bid], d.lds_stride[bid] = p["off"][n], p["stride"][n]
        d.lds_floats = p["total"]
        for li, ly in enumerate(self.layers):
            L = d.layer[li]
            L.K, L.No, L.relu = ly.K, ly.No, int(ly.relu)
            L.src, L.src_col = p["ids"][ly.src], ly.sc
            L.dst = {"mean": _lib.MLP_OUT0, "value": _lib.MLP_OUT1}.get(ly.dst, p["ids"].get(ly.dst, 0))
            L.dst_col, L.w_off, L.b_off, L.wt_off, L.wb_off = ly.dc, ly.w_off, ly.b_off, p["wt_off"][li], p["wb_off"][li]
            L.wr_off, L.wq_off = p["wr_off"][li], p["wq_off"][li]
            if save and b is not None and ly.dst not in ("mean", "value"):
                L.save, L.save_ld = b[ly.dst].data_ptr(), b[ly.dst].shape[1]
        return d

    def mark_updated(self, packed_current: bool = False):
        """call after writing ``self.flat`` (optimiser step, load): the packed forward weights are refreshed
        by the next forward.  With ``lazy_pack`` False (default) every forward repacks -- safe for callers that
        write ``flat`` directly; the trainers set ``lazy_pack`` and call this after each step.
        ``packed_current``: the writer already refreshed the packed images (adam_step below, with a pack map)."""
        self._stamp += 1
        if packed_current and self._packed is not None:
            self._packed_stamp = self._stamp

    def pack_map(self):
        """-> (int32 [n_params, 4] device tensor, packed buffer): for every parameter the float offsets of its copies in
        the packed forward / data-gradient weight images (-1: biases, log_std), for vf_adam_cfg.pack_map"""
        if self._plan is None:
            return None, None
        if self._pack_map is None:
            m = np.full((self.n_total, 4), -1, np.int32)
            for li, ly in enumerate(self.layers):
                n, k = np.meshgrid(np.arange(ly.No), np.arange(ly.K), indexing="ij")
                flat = ly.w_off + n * ly.K + k
                m[flat, 0] = self._plan["wt_off"][li] + k * ((ly.No + 31) & ~31) + n
                m[flat, 1] = self._plan["wb_off"][li] + n * ((ly.K + 31) & ~31) + k
                G, a, i = self._chain_groups(ly), n >> 5, n & 31
                if ly.first:          # k = 8 g + 2 j + h
                    g, j, h = k >> 3, (k & 7) >> 1, k & 1
                else:                 # k = 32 (g / 4) + 8 (g % 4) + 4 h + j
                    g, h, j = (k >> 5) * 4 + ((k & 31) >> 3), (k & 7) >> 2, k & 3
                m[flat, 2] = self._plan["wr_off"][li] + (((a * G + g) * 64 + h * 32 + i) << 2) + j
                # reverse chain: block (k / 32, n / 8), lane (n % 8) / 4 * 32 + k % 32, word n % 4
                GQ = (ly.No + 7) >> 3
                m[flat, 3] = self._plan["wq_off"][li] + ((((k >> 5) * GQ + (n >> 3)) * 64 + ((n & 7) >> 2) * 32 + (k & 31)) << 2) + (n & 3)
            self._pack_map = th.from_numpy(m).to(self.device)
            self._stamp += 1          # force one full pack (zero pads) before the incremental refreshes
            self._pack()
        return self._pack_map, self._packed

    def adam_step(self, exp_avg, exp_avg_sq, sumsq, scratch, lr, betas, eps, weight_decay, max_grad_norm, step,
                  sumsq_partials=None, sumsq_tail_from=0):
        """clip ``self.grad`` to ``max_grad_norm`` (None / 0: no clip) and take one Adam step on ``self.flat``; the launch refreshes
        the packed MFMA weight images as well (pack_map).  The squared gradient norm goes through ``sumsq`` (1 float; ``scratch``: 4096
        floats of reduction scratch) unless ``sumsq_partials`` = (fp64 device tensor, count) carries it as the per-block partial sums the
        weight-gradient fold left, to which the launch adds grad[sumsq_tail_from:]^2 (what the fold does not cover: log_std)."""
        L, st = _lib.lib(), self._stream()
        if sumsq_partials is None:
            _lib.check(L.vf_sumsq(_ptr(self.grad), self.n_params, _ptr(sumsq), _ptr(scratch), st))
        pmap, packed = self.pack_map()
        part, n_part = (None, 0) if sumsq_partials is None else (sumsq_partials[0].data_ptr(), sumsq_partials[1])
        cfg = _lib.AdamCfg(lr, betas[0], betas[1], eps, weight_decay, max_grad_norm if max_grad_norm is not None else 0.0, step, 0,
                           _ptr(pmap), _ptr(packed), part, n_part, sumsq_tail_from)
        _lib.check(L.vf_adam_step(_ptr(self.flat), _ptr(self.grad), _ptr(exp_avg), _ptr(exp_avg_sq), self.n_params, _ptr(sumsq),
                                  C.byref(cfg), st))
        self.mark_updated(packed_current=pmap is not None)

    def _pack(self):
        if self._packed is None:
            self._packed = th.empty(self._plan["packed_floats"], dtype=th.float32, device=self.device)
            self._pack_desc = self._fused_desc(None, False)
        if self.lazy_pack and self._packed_stamp == self._stamp:
            return
        _lib.check(_lib.lib().vf_mlp_pack_weights(C.byref(self._pack_desc), _ptr(self.flat), _ptr(self._packed), self._stream()))
        self._packed_stamp = self._stamp

    def forward_desc(self, M, slot, save):
        """the vf_mlp_desc of the fused forward over buffer set (M, slot), built once per (M, slot, save); ``save`` keeps the activations"""
        key = (M, slot, bool(save))
        d = self._descs.get(key)
        if d is None:
            d = self._descs[key] = self._fused_desc(self._buffers(M, slot), save)
        return d

    def reverse_flat_desc(self, M, H, d_means, d_log_stds=None):
        """the reverse descriptor over the first H reserved slots of M rows as ONE (H M)-row matrix, built once per (M, H, heads), with
        the heads' gradients pointed at the caller's d_means (H, M, 4) [/ d_log_stds: both trunks are swept]
        -> (desc, {obs key: dLoss/d obs}, (H, M, 4) action-gradient scratch)"""
        key = ("bwd_flat", M, H, d_log_stds is not None)
        b = None if key in self._descs else {name: t[:H].reshape(-1, t.shape[-1]) for name, t in self._slot_blocks[M][1].items()}
        c = self._reverse_desc(key, b, H * M, d_means, d_log_stds, True,
                               extra=lambda: th.empty((H, M, 4), dtype=th.float32, device=self.device))
        return c[0], c[1], c[4]

    def _reverse_desc(self, key, b, M, d_mean, d_value, need_input_grad, rebind_x=False, extra=None):
        """the reverse descriptor over buffer set ``b``, built once per ``key`` (None: b's buffers are not fixed -- built per call)
        -> (desc, d_in, head entries, first-layer entries, what ``extra()`` made when the entry was built).  On a hit only what is the
        caller's is pointed anew: with ``rebind_x`` the first layers' X at the observation rows now bound into b (the heads'
        gradients are b's own then), else the heads' dY at d_mean / d_value (``b`` is not read)"""
        c = self._descs.get(key) if key is not None else None
        if c is None:
            d, d_in = self._bwd_desc(b, M, d_mean, d_value, need_input_grad)
            # entries whose X is an observation: that pointer is the caller's tensor and may change from call to call
            firsts = [(i, ly.src) for i, ly in enumerate(self._reverse_layers(True, d_value is not None)) if ly.first]
            c = (d, d_in, self._head_entries(d_value is not None), firsts, extra() if extra else None)
            if key is not None:
                self._descs[key] = c
            return c
        d = c[0]
        if rebind_x:
            for i, src in c[3]:
                d.layer[i].X = _ptr(b[src])
            return c
        im, iv = c[2]
        d.layer[im].dY = _lib.ptr(d_mean)          # the heads' gradients are the caller's tensors
        if iv is not None:
            d.layer[iv].dY = _lib.ptr(d_value)
        return c

    # -------------------------------------------------------------------------------------------
    def weight(self, ly):
        return self.flat[ly.w_off:ly.w_off + ly.K * ly.No].view(ly.No, ly.K)

    def bias(self, ly):
        return self.flat[ly.b_off:ly.b_off + ly.No]

    def ln_weight(self, ly):
        return self.flat[ly.g_off:ly.g_off + ly.No]

    def ln_bias(self, ly):
        return self.flat[ly.be_off:ly.be_off + ly.No]

    @property
    def log_std(self):
        return self.flat[self.log_std_off:self.n_params]

    def _buffers(self, M, slot=0):
        """activation buffers of one forward pass (kept for backward).  ``slot`` selects one of several resident
        sets for the same M -- a BPTT horizon keeps every step's activations (HBM is plentiful: 60 MB per step at
        16 384 rows) instead of recomputing the forward in the reverse sweep; gradient buffers are shared."""
        b = self._bufs.get((M, slot))
        if b is None:
            if len({m for m, _ in self._bufs}) > 4 and M not in {m for m, _ in self._bufs}:
                self._bufs.clear()
                self._gbufs.clear()
                self._descs.clear()
                self._slot_blocks.clear()
            b = {name: th.empty((M, w), dtype=th.float32, device=self.device) for name, w in self.widths.items()}
            for ly in self.layers:
                if ly.ln:     # the Linear's output, overwritten by xhat (what the backward needs), and 1 / sqrt(var + eps) per row
                    b["z:" + ly.ln_key] = th.empty((M, ly.No), dtype=th.float32, device=self.device)
                    b["r:" + ly.ln_key] = th.empty(M, dtype=th.float32, device=self.device)
            g = self._gbufs.get(M)
            if g is None:
                g = self._gbufs[M] = {"g:" + name: th.empty((M, w), dtype=th.float32, device=self.device)
                                      for name, w in self.widths.items() if name not in ("mean", "value")}
            b.update(g)
            self._bufs[(M, slot)] = b
        return b

    def reserve_slots(self, M, n):
        """activation / gradient buffers of slots 0..n-1 stored back to back per buffer ([n][M][w]), observations
        copied in: the rows of all slots then form ONE (n M, w) matrix per buffer, which is what lets
        ``weight_grad_slots`` reduce the weight gradient of a whole BPTT horizon in one launch"""
        if self.ln:
            raise NotImplementedError("layer norm: the horizon paths (reserved slots) are not implemented for networks with LayerNorm")
        if self._slot_blocks.get(M, (0,))[0] >= n:
            return
        for key in [k for k in self._bufs if k[0] == M]:
            del self._bufs[key]
        self._descs = {k: v for k, v in self._descs.items() if M not in k[:2]}
        f = dict(dtype=th.float32, device=self.device)
        blk = {name: th.empty((n, M, w), **f) for name, w in self.widths.items()}
        blk.update({"g:" + name: th.empty((n, M, w), **f) for name, w in self.widths.items() if name not in ("mean", "value")})
        blk.update({"obs:" + k: th.empty((n, M, d), **f) for k, d in self.obs_dims.items()})
        self._slot_blocks[M] = (n, blk)
        for s in range(n):
            b = {name: t[s] for name, t in blk.items()}
            b["_contig"] = True
            self._bufs[(M, s)] = b

    def _stream(self):
        return _lib.current_stream(self.device)

    def _check_rows(self, obs, M=None):
        """every observation entry the policy reads is a contiguous float32 device matrix of its width, of M rows (None: any)"""
        for k in self.obs_keys:
            t = obs[k]
            assert t.is_cuda and t.dtype == th.float32 and t.is_contiguous() and t.shape[1:] == (self.obs_dims[k],) and M in (None, t.shape[0])

    def _bind_obs(self, b, obs, M):
        """checks the observation rows and makes them buffer set b's: reserved slots own their rows (copied in), any other set
        reads the caller's tensors"""
        self._check_rows(obs, M)
        for k in self.obs_keys:
            if b.get("_contig"):
                b["obs:" + k].copy_(obs[k])
            else:
                b["obs:" + k] = obs[k]

    def _scratch_for(self, need):
        """the float scratch of the backward launches, grown to ``need`` floats if it is smaller"""
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = th.empty(need, dtype=th.float32, device=self.device)
        return self._scratch

    def _latched_off(self, flag, rc):
        """a one-launch entry point returned ``rc`` != 0 (callers test that inline: the launch paths are host-bound): EUNSUPPORTED
        latches ``flag`` to False -- that path stays off for this network -- and gives True (the caller falls back); any other
        error raises"""
        if rc != _lib.EUNSUPPORTED:
            _lib.check(rc)
        setattr(self, flag, False)
        return True

    def _put_log_std_grad(self, d_log_std, accumulate):
        if d_log_std is None:
            return
        if accumulate:
            self.grad[self.log_std_off:self.n_params] += d_log_std
        else:
            self.grad[self.log_std_off:self.n_params] = d_log_std

    def _reverse_layers(self, has_mean=True, has_value=True):
        """the layers of the reverse table, in its order: reversed, without the frozen ones and without a trunk (its head, its hidden
        layers, its side's extractor) that gets no head gradient"""
        for ly in reversed(self.layers):
            if ly.frozen:
                continue
            if not has_value and (ly.dst == "value" or ly.dst.startswith("vf:") or ly.side == "vf"):
                continue
            if not has_mean and (ly.dst == "mean" or ly.dst.startswith("pi:") or ly.side == "pi"):
                continue
            yield ly

    def forward(self, obs: Dict[str, th.Tensor], save_activations: bool = True, slot: int = 0, need_value: bool = True,
                out_value: Optional[th.Tensor] = None):
        """-> mean (M,4), value (M,1) (``need_value=False``: value is None and, where the kernel supports it, the value
        trunk is not run; ``out_value``: the value head is written there -- a (M,) row of the rollout buffer -- instead
        of the internal buffer).  One launch for the whole network when the LDS plan fits
        (``self.fused``); ``save_activations`` keeps every layer output in HBM for ``backward``
        (inference passes False and moves only observations in and heads out)."""
        M = obs[self.obs_keys[0]].shape[0]
        b = self._buffers(M, slot)
        L, st = _lib.lib(), self._stream()
        self._bind_obs(b, obs, M)
        self._last_M, self._last_slot = M, slot
        if self._plan is not None and self.fused:
            d = self.forward_desc(M, slot, save_activations)
            ins = [_ptr(b["obs:" + k]) for k in self.obs_keys] + [None] * (4 - len(self.obs_keys))
            self._pack()
            skip_vf = not need_value and self._pi_only_ok
            vout = b["value"] if out_value is None else out_value
            rc = L.vf_mlp_forward(C.byref(d), _ptr(self.flat), _ptr(self._packed), ins[0], ins[1], ins[2], ins[3],
                                  _ptr(b["mean"]), None if skip_vf else _ptr(vout), M, st)
            if skip_vf and rc and self._latched_off("_pi_only_ok", rc):      # this layer table runs on the LDS kernel: it computes both heads
                rc = L.vf_mlp_forward(C.byref(d), _ptr(self.flat), _ptr(self._packed), ins[0], ins[1], ins[2], ins[3],
                                      _ptr(b["mean"]), _ptr(vout), M, st)
            if rc:
                _lib.check(rc)
            return b["mean"], (vout if need_value else None)
        if self.wide or self.ln:
            self._warn_fallback("forward")
        for ly in self.layers:
            X, Y = b[ly.src], b[ly.dst]
            if ly.ln:        # Linear into the pre-norm buffer, then LayerNorm + activation into the destination (xhat replaces z)
                Z = b["z:" + ly.ln_key]
                rc = L.vf_linear_fwd(_ptr(X, ly.sc), X.shape[1], _ptr(self.flat, ly.w_off), _ptr(self.flat, ly.b_off),
                                     _ptr(Z), ly.No, M, ly.K, ly.No, 0, st)
                rc = rc or L.vf_layernorm_fwd(_ptr(Z), ly.No, _ptr(self.flat, ly.g_off), _ptr(self.flat, ly.be_off), LN_EPS,
                                              _ptr(Y, ly.dc), Y.shape[1], _ptr(Z), ly.No, _ptr(b["r:" + ly.ln_key]), M, ly.No,
                                              int(ly.relu), st)
                if rc:
                    _lib.check(rc)
                continue
            rc = L.vf_linear_fwd(_ptr(X, ly.sc), X.shape[1], _ptr(self.flat, ly.w_off), _ptr(self.flat, ly.b_off),
                                 _ptr(Y, ly.dc), Y.shape[1], M, ly.K, ly.No, int(ly.relu), st)
            if rc:
                _lib.check(rc)
        if out_value is not None:
            out_value.copy_(b["value"].view(out_value.shape))
            return b["mean"], out_value
        return b["mean"], b["value"]

    def backward(self, d_mean: th.Tensor, d_value: Optional[th.Tensor], d_log_std: Optional[th.Tensor],
                 accumulate: bool = False, need_input_grad: bool = False, slot: Optional[int] = None):
        """fills (or, with ``accumulate``, adds into) ``self.grad`` -- flat, same layout as ``self.flat`` --
        from the head gradients.  d_value None skips the value trunk (first-order policy optimisation has
        no critic), d_mean None the policy trunk (a critic network uses the value trunk only);
        need_input_grad also returns {obs key: dLoss/d obs} (BPTT differentiates through obs)."""
        M = self._last_M
        b = self._buffers(M, self._last_slot if slot is None else slot)
        L, st = _lib.lib(), self._stream()
        if self.fused_backward and self._plan is not None:
            return self._backward_fused(b, M, d_mean, d_value, d_log_std, accumulate, need_input_grad)
        self._scratch_for(max(max(int(L.vf_linear_bwd_scratch_floats(M, ly.K, ly.No)), int(L.vf_layernorm_bwd_scratch_floats(M, ly.No)) if ly.ln else 0)
                              for ly in self.layers))
        gbuf = {} if d_mean is None else {"mean": d_mean}
        if d_value is not None:
            gbuf["value"] = d_value.view(M, self.head_dims[1])
        wgrad = L.vf_linear_bwd_weight_acc if accumulate else L.vf_linear_bwd_weight
        touched = set()
        d_in = {}
        for ly in self._reverse_layers(d_mean is not None, d_value is not None):
            dY = gbuf.get(ly.dst, b.get("g:" + ly.dst))
            Y, X = b[ly.dst], b[ly.src]
            ym = _ptr(Y, ly.dc) if ly.relu else None
            act = int(ly.relu)
            if ly.ln:
                # through activation and LayerNorm first: dY becomes the gradient of the Linear's own output (in place: this layer is
                # the only reader of its slice of the g: buffer), dgamma / dbeta go straight into the flat gradient; the Linear's
                # three products then see a layer without activation
                rc = L.vf_layernorm_bwd(_ptr(dY, ly.dc), dY.shape[1], ym, Y.shape[1], _ptr(b["z:" + ly.ln_key]), ly.No,
                                        _ptr(b["r:" + ly.ln_key]), _ptr(self.flat, ly.g_off), _ptr(dY, ly.dc), dY.shape[1],
                                        _ptr(self.grad, ly.g_off), _ptr(self.grad, ly.be_off), M, ly.No, act, 1 if accumulate else 0,
                                        _ptr(self._scratch), st)
                if rc:
                    _lib.check(rc)
                ym, act = None, 0
            rc = wgrad(_ptr(dY, ly.dc), dY.shape[1], ym, Y.shape[1], _ptr(X, ly.sc), X.shape[1],
                       _ptr(self.grad, ly.w_off), _ptr(self.grad, ly.b_off), M, ly.K, ly.No, _ptr(self._scratch), act, st)
            if rc:
                _lib.check(rc)
            if ly.first and not need_input_grad:
                continue
            if ly.first and ly.src[4:] in INDEX_OBS_KEYS:     # an index column carries no gradient: the branch stops at its first layer
                continue
            if ly.first:
                dX = d_in.setdefault(ly.src[4:], th.empty((M, ly.K), dtype=th.float32, device=self.device))
            else:
                dX = b["g:" + ly.src]
            key = (ly.src, ly.sc)
            rc = L.vf_linear_bwd_data(_ptr(dY, ly.dc), dY.shape[1], ym, Y.shape[1], _ptr(self.flat, ly.w_off),
                                      _ptr(dX, ly.sc), dX.shape[1], M, ly.K, ly.No, 1 if key in touched else 0, act, st)
            if rc:
                _lib.check(rc)
            touched.add(key)
        self._put_log_std_grad(d_log_std, accumulate)
        return d_in

    def _bwd_desc(self, b, M, d_mean, d_value, need_input_grad):
        """vf_mlp_bwd_desc of the reverse sweep over buffer set b: layers in reverse order, a trunk without head
        gradient skipped -> (desc, {obs key: dLoss/d obs tensor})"""
        gbuf = {} if d_mean is None else {"mean": d_mean}
        if d_value is not None:
            gbuf["value"] = d_value.view(-1, self.head_dims[1])
        d = _lib.MlpBwdDesc()
        d.n_fold = self.log_std_off
        touched, d_in, n = set(), {}, 0
        for ly in self._reverse_layers(d_mean is not None, d_value is not None):
            dY = gbuf.get(ly.dst, b.get("g:" + ly.dst))
            Y, X = b[ly.dst], b[ly.src]
            e = d.layer[n]
            n += 1
            e.K, e.No, e.w_off, e.b_off = ly.K, ly.No, ly.w_off, ly.b_off
            li = self.layers.index(ly)
            e.wb_off, e.wq_off = self._plan["wb_off"][li], self._plan["wq_off"][li]
            e.dY, e.ld_dy = _ptr(dY, ly.dc), dY.shape[-1]
            e.Y, e.ld_y, e.act = (_ptr(Y, ly.dc) if ly.relu else None), Y.shape[-1], int(ly.relu)
            e.X, e.ld_x = _ptr(X, ly.sc), X.shape[-1]
            e.need_dx = 0
            if ly.first and not need_input_grad:
                continue
            if ly.first:
                # (an index column -- "gate" -- carries no gradient: the one-launch reverse kernels form every first layer's input tile
                # or none, so its 1-wide tile goes to a buffer of its own that is never handed out)
                dX = self._index_sink(M, ly.K) if ly.src[4:] in INDEX_OBS_KEYS else d_in.setdefault(ly.src[4:], th.empty((M, ly.K), dtype=th.float32, device=self.device))
            else:
                dX = b["g:" + ly.src]
            key = (ly.src, ly.sc)
            e.dX, e.ld_dx, e.need_dx = _ptr(dX, ly.sc), dX.shape[-1], (2 if key in touched else 1)
            touched.add(key)
        d.n_layers = n
        return d, d_in

    def _index_sink(self, M, K):
        """where the one-launch reverse kernels put the input tile of an index column: one buffer per row count, owned by the policy like its
        other gradient buffers (dropped with them), never handed out"""
        t = self._gbufs.get(("index_sink", M, K))
        if t is None:
            t = self._gbufs[("index_sink", M, K)] = th.empty((M, K), dtype=th.float32, device=self.device)
        return t

    def forward_act(self, obs, eps, action, slot=0):
        """policy trunk + action head in one launch (vf_mlp_forward_act): ``action`` (M,4) <- tanh(mean + exp(log_std) eps),
        activations saved for the reverse pass of `slot`.  -> False when the network is not a register-chained class."""
        if self._act_fused is False or self._plan is None or not self.fused:
            return False
        M = action.shape[0]
        b = self._buffers(M, slot)
        self._check_rows(obs, M)
        ins, copies = [], []
        for k in self.obs_keys:
            ins.append(_ptr(obs[k]))
            if b.get("_contig"):
                copies.append(_ptr(b["obs:" + k]))       # reserved slots own their observation rows: written by the kernel
            else:
                b["obs:" + k] = obs[k]
                copies.append(None)
        ins += [None] * (2 - len(ins))
        copies += [None] * (2 - len(copies))
        self._last_M, self._last_slot = M, slot
        d = self.forward_desc(M, slot, True)
        self._pack()
        rc = _lib.lib().vf_mlp_forward_act(C.byref(d), _ptr(self.flat), _ptr(self._packed), ins[0], ins[1], _ptr(self.log_std),
                                           _ptr(eps), _ptr(action), copies[0], copies[1], M, self._stream())
        return not (rc and self._latched_off("_act_fused", rc))

    def backward_data_act(self, d_action, action, eps, g_log_std, d_mean, slot):
        """``backward_data`` with the action head's reverse fused in (vf_mlp_backward_data_act): d_mean (M,4) is written for
        ``weight_grad_slots``, g_log_std (M,4) accumulated; -> {obs key: dLoss/d obs}"""
        M = d_action.shape[0]
        b = self._buffers(M, slot)
        d, d_in = self._slot_reverse_desc(b, M, slot, d_mean, None)
        self._pack()
        _lib.check(_lib.lib().vf_mlp_backward_data_act(C.byref(d), _ptr(self._packed), _ptr(d_action), _ptr(action), _ptr(self.log_std),
                                                       _ptr(eps), _ptr(g_log_std), M, self._stream()))
        return d_in

    def backward_data_supported(self, M, slot=0, both_heads=False):
        """can ``backward_data`` (policy trunk [+ second trunk: ``both_heads``] + observation gradient) run for this network?"""
        if self._plan is None or not self.fused_backward:
            return False
        b = self._buffers(M, slot)
        dm = th.empty((M, self.head_dims[0]), dtype=th.float32, device=self.device)
        dv = th.empty((M, self.head_dims[1]), dtype=th.float32, device=self.device) if both_heads else None
        d, _ = self._bwd_desc(b, M, dm, dv, True)
        return bool(_lib.lib().vf_mlp_backward_data_supported(C.byref(d)))

    def _head_entries(self, both_heads):
        """indices of the (mean, value) head layers in the reverse layer table ``_bwd_desc`` builds (reversed layer order, a
        trunk without head gradient skipped)"""
        order = [ly.dst for ly in self._reverse_layers(True, both_heads)]
        return order.index("mean"), (order.index("value") if both_heads else None)

    def _slot_reverse_desc(self, b, M, slot, d_mean, d_value):
        """(desc, d_in) of the reverse chain over buffer set (M, slot) with the observation gradient; kept for reserved slots only
        (fixed buffers)"""
        key = ("bwd_data", M, slot, d_value is not None) if b.get("_contig") else None
        return self._reverse_desc(key, b, M, d_mean, d_value, True)[:2]

    def backward_data(self, d_mean, slot, d_value=None):
        """reverse chain of slot `slot` only (policy trunk; with ``d_value`` both trunks -- the reference's Actor, whose second
        head is log_std): masked layer gradients stay in the slot's g: buffers for ``weight_grad_slots``; -> {obs key: dLoss/d obs}
        (for reserved slots the returned tensors are reused by the next call on the same slot)"""
        M = d_mean.shape[0]
        b = self._buffers(M, slot)
        d, d_in = self._slot_reverse_desc(b, M, slot, d_mean, d_value)
        self._pack()
        _lib.check(_lib.lib().vf_mlp_backward_data(C.byref(d), _ptr(self._packed), M, self._stream()))
        return d_in

    def weight_grad_slots(self, M, n, d_mean_all, accumulate=False, d_value_all=None, lo=0):
        """weight / bias gradients of the policy trunk (+ the second trunk when ``d_value_all`` is given) + extractors summed over
        slots lo..lo+n-1 (reserved with ``reserve_slots``; d_mean_all (n, M, 4) [d_value_all (n, M, w)] hold the head gradients the
        ``backward_data`` calls were given for THOSE slots)"""
        nblk, blk = self._slot_blocks[M]
        assert lo + n <= nblk and d_mean_all.shape == (n, M, 4) and d_mean_all.is_contiguous()
        assert d_value_all is None or (d_value_all.shape == (n, M, self.head_dims[1]) and d_value_all.is_contiguous())
        # one launch over 1 M rows runs at 67 TF/s, two over 512 K rows each at 76 (profiles/r06_bptt_wgrad_chunks.txt: not a cache effect --
        # the rows are as fast cold as hot): a horizon above WGRAD_SPLIT_ROWS is reduced in equal runs of whole slots, in slot order
        if n > 1 and n * M > WGRAD_SPLIT_ROWS:
            per = max(1, min(n - 1, WGRAD_SPLIT_ROWS // M))
            per = (n + ((n + per - 1) // per) - 1) // ((n + per - 1) // per)        # equal runs
            for s0 in range(0, n, per):
                k = min(per, n - s0)
                self.weight_grad_slots(M, k, d_mean_all[s0:s0 + k], accumulate or s0 > 0, None if d_value_all is None else d_value_all[s0:s0 + k], lo + s0)
            return
        b = {name: t[lo:lo + n].reshape(-1, t.shape[-1]) for name, t in blk.items()}
        d, _ = self._bwd_desc(b, n * M, d_mean_all.view(-1, 4), None if d_value_all is None else d_value_all.view(n * M, -1), False)
        L = _lib.lib()
        scr = self._scratch_for(int(L.vf_mlp_backward_partial_floats(C.byref(d), n * M)))
        _lib.check(L.vf_mlp_weight_grad(C.byref(d), _ptr(scr), _ptr(self.grad), n * M, 1 if accumulate else 0, self._stream()))

    def bucket_split(self):
        """first flat-parameter offset of the trunks: [0, split) = the extractor MLPs' parameters, [split, n_params) = both trunks, the
        heads and log_std -- the two gradient buckets of the two-bucket exchange (PPO.grad_buckets)"""
        return min(ly.w_off for ly in self.layers if not ly.frozen and not ly.ext)

    def ppo_update(self, obs, actions, old_lp, adv, ret, loss_cfg, stats, loss_scratch, want_sumsq=False, row_index=None, between=None):
        """forward + PPO loss + reverse chain in one launch, then the weight gradients into ``self.grad`` (vf_ppo_update +
        vf_mlp_weight_grad).  -> False when the network is not one of the register-chained classes (the caller then
        runs forward / vf_ppo_loss / backward).  ``want_sumsq``: -> (fp64 partials tensor, count) of the squared norm of the
        gradient the fold wrote, for vf_adam_cfg.sumsq_partials (no separate grad-norm launch).
        ``between`` (callable): the weight gradients are formed in TWO launch pairs -- trunks + heads first, then the extractor MLPs -- and
        ``between()`` runs after the first pair was enqueued (the trainer starts the first bucket's all-reduce there).
        ``row_index`` (int64, M entries; vf_ppo_loss_cfg.row_index): obs / actions / old_lp / ret (and loss_cfg.old_value) are the
        WHOLE rollout buffer and row m of the minibatch is their row row_index[m] -- no shuffled copy; ``adv`` stays in minibatch order."""
        if self._fused_ppo is False or self._plan is None or not (self.fused and self.fused_backward) or (self.sep and len(self.obs_keys) > 2):
            return False
        M = actions.shape[0] if row_index is None else row_index.numel()
        b = self._buffers(M, 0)
        L, st = _lib.lib(), self._stream()
        if row_index is None:
            self._bind_obs(b, obs, M)
        else:
            # the launch leaves the minibatch's observation rows, in minibatch order, where the weight gradients read them
            self._check_rows(obs)
            assert row_index.dtype == th.int64 and row_index.is_contiguous() and adv.numel() == M
            for k in () if b.get("_contig") else self.obs_keys:        # (reserved slots own their observation rows already)
                own = b.get("_own:" + k)
                if own is None:
                    own = b["_own:" + k] = th.empty((M, self.obs_dims[k]), dtype=th.float32, device=self.device)
                b["obs:" + k] = own
            loss_cfg.row_index = row_index.data_ptr()
            loss_cfg.obs_copy0 = _ptr(b["obs:" + self.obs_keys[0]])
            loss_cfg.obs_copy1 = _ptr(b["obs:" + self.obs_keys[1]]) if len(self.obs_keys) > 1 else None
        self._last_M, self._last_slot = M, 0
        d = self.forward_desc(M, 0, True)
        if "d:mean" not in b:
            b["d:mean"], b["d:value"] = th.empty((M, 4), dtype=th.float32, device=self.device), th.empty(M, dtype=th.float32, device=self.device)
        bd = self._reverse_desc(("ppo_bwd", M), b, M, b["d:mean"], b["d:value"], False, rebind_x=True)[0]
        ins = [_ptr(obs[k] if row_index is not None else b["obs:" + k]) for k in self.obs_keys] + [None] * (2 - len(self.obs_keys))
        self._pack()
        # want_sumsq: the loss-statistic rows are folded by the weight-gradient fold launch (one launch less)
        rc = L.vf_ppo_update(C.byref(d), C.byref(bd), _ptr(self.flat), _ptr(self._packed), ins[0], ins[1], _ptr(self.log_std),
                             _ptr(actions), _ptr(old_lp), _ptr(adv), _ptr(ret), None if want_sumsq else _ptr(stats), M,
                             C.byref(loss_cfg), _ptr(loss_scratch), st)
        if rc and self._latched_off("_fused_ppo", rc):
            self._warn_fallback("vf_ppo_update")
            return False
        scr = self._scratch_for(int(L.vf_mlp_backward_partial_floats(C.byref(bd), M)))
        if want_sumsq:
            nb = int(L.vf_mlp_weight_grad_fold_blocks(C.byref(bd)))
            if self._sq_part is None or self._sq_part.numel() < nb:
                self._sq_part = th.empty(nb, dtype=th.float64, device=self.device)
            ls = _lib.StatsFold(_ptr(loss_scratch), (M + 31) // 32, 0, _ptr(stats), loss_cfg.d_log_std_out, loss_cfg.stats_accum)
            _lib.check(L.vf_mlp_weight_grad_sumsq(C.byref(bd), _ptr(scr), _ptr(self.grad), M, 0, self._sq_part.data_ptr(),
                                                  C.byref(ls), st))
            return self._sq_part, nb
        if between is not None:        # two launch pairs on the plan of the whole table (same bits): trunk / head layers, then the extractors'
            split = self.bucket_split()
            first = sum(1 << i for i in range(bd.n_layers) if bd.layer[i].w_off >= split)
            _lib.check(L.vf_mlp_weight_grad_layers(C.byref(bd), _ptr(scr), _ptr(self.grad), M, 0, first, st))
            between()
            _lib.check(L.vf_mlp_weight_grad_layers(C.byref(bd), _ptr(scr), _ptr(self.grad), M, 0, ((1 << bd.n_layers) - 1) & ~first, st))
            return True
        _lib.check(L.vf_mlp_weight_grad(C.byref(bd), _ptr(scr), _ptr(self.grad), M, 0, st))
        return True

    def forward_steps(self, obs, m_step, n_steps):
        """inference forward of ``n_steps`` consecutive blocks of ``m_step`` rows in one launch, every row as ``forward`` computes it
        in a launch over its block alone (vf_mlp_forward_steps) -> (mean, value) of (n_steps m_step) rows, or None when the library
        has no register-chained class for this network / row count (the caller loops ``forward``).  The returned tensors are the
        policy's own output buffers for this row count: the next call with the same (m_step, n_steps) overwrites them."""
        if self._steps_ok is False or self._plan is None or not self.fused or m_step % 32:
            return None
        M = m_step * n_steps
        self._check_rows(obs, M)
        if self._pack_desc is None:
            self._pack_desc = self._fused_desc(None, False)
        out = self._steps_out.get(M)
        if out is None:
            f = dict(dtype=th.float32, device=self.device)
            out = self._steps_out[M] = (th.empty((M, self.head_dims[0]), **f), th.empty((M, self.head_dims[1]), **f))
        ins = [_ptr(obs[k]) for k in self.obs_keys] + [None] * (3 - len(self.obs_keys))
        self._pack()
        rc = _lib.lib().vf_mlp_forward_steps(C.byref(self._pack_desc), _ptr(self.flat), _ptr(self._packed), ins[0], ins[1], ins[2],
                                             _ptr(out[0]), _ptr(out[1]), int(m_step), int(n_steps), self._stream())
        return None if rc and self._latched_off("_steps_ok", rc) else out

    def twin_q_update(self, obs, target, loss_out, m_global):
        """a twin critic's update step up to the flat gradient (shac.py:267-270): forward + mse_loss(target, min(Q1, Q2)) + reverse
        chain in one launch (vf_twin_q_update / vf_twin_q_update_in3), then the weight gradients into ``self.grad``.  ``obs``: the
        observations of the extractor's one or two branches + the pass-through "action" rows; ``loss_out`` (1,) device tensor.  -> False when the network is not the register-chained
        critic class (the caller then runs forward / vf_twin_q_loss / backward)."""
        if self._fused_twin_q is False or self._plan is None or not (self.fused and self.fused_backward) or len(self.obs_keys) not in (2, 3):
            return False
        M = target.shape[0]
        b = self._buffers(M, 0)
        L, st = _lib.lib(), self._stream()
        self._bind_obs(b, obs, M)
        self._last_M, self._last_slot = M, 0
        d = self.forward_desc(M, 0, True)
        if "d:q0" not in b:
            b["d:q0"] = th.empty((M, self.head_dims[0]), dtype=th.float32, device=self.device)
            b["d:q1"] = th.empty((M, self.head_dims[1]), dtype=th.float32, device=self.device)
        c = self._reverse_desc(("twin_q_bwd", M), b, M, b["d:q0"], b["d:q1"], False, rebind_x=True,
                               extra=lambda: th.empty(int(L.vf_twin_q_update_scratch_doubles(M)), dtype=th.float64, device=self.device))
        bd, scr = c[0], c[4]
        self._pack()
        ins = [_ptr(b["obs:" + k]) for k in self.obs_keys] + [None] * (3 - len(self.obs_keys))      # (two branches: the action rows are in2)
        rc = L.vf_twin_q_update_in3(C.byref(d), C.byref(bd), _ptr(self.flat), _ptr(self._packed), ins[0], ins[1], ins[2], _ptr(target),
                                    _ptr(loss_out), scr.data_ptr(), M, int(m_global), st)
        if rc and self._latched_off("_fused_twin_q", rc):
            self._warn_fallback("vf_twin_q_update")
            return False
        _lib.check(L.vf_mlp_weight_grad(C.byref(bd), _ptr(self._scratch_for(int(L.vf_mlp_backward_partial_floats(C.byref(bd), M)))),
                                        _ptr(self.grad), M, 0, st))
        return True

    def _backward_fused(self, b, M, d_mean, d_value, d_log_std, accumulate, need_input_grad):
        """the same sweep as the layer-by-layer path, as ONE launch + one fold (vf_mlp_backward): a block owns
        its 64-row tiles for every layer, so g:* buffers written by one entry are read by the next without
        a grid-wide barrier."""
        L, st = _lib.lib(), self._stream()
        d, d_in = self._bwd_desc(b, M, d_mean, d_value, need_input_grad)
        scr = self._scratch_for(int(L.vf_mlp_backward_partial_floats(C.byref(d), M)))
        self._pack()
        _lib.check(L.vf_mlp_backward(C.byref(d), _ptr(self._packed), _ptr(scr), _ptr(self.grad), M,
                                     1 if accumulate else 0, st))
        self._put_log_std_grad(d_log_std, accumulate)
        return d_in

    # -------------------------------------------------------------------------------------------
    def to_torch(self):
        """equivalent torch.nn module (fp32) sharing NO storage -- the plain-PyTorch reference the
        numerics tests compare against"""
        import torch.nn as nn
        pol = self

        class Ref(nn.Module):
            def __init__(s):
                super().__init__()
                s.lin = nn.ModuleList()
                s.norm = nn.ModuleDict()        # str(index into pol.layers) -> that layer's nn.LayerNorm; `lin` still zips with pol.layers
                for i, ly in enumerate(pol.layers):
                    m = nn.Linear(ly.K, ly.No)
                    m.weight.data.copy_(pol.weight(ly).cpu())
                    m.bias.data.copy_(pol.bias(ly).cpu())
                    s.lin.append(m)
                    if ly.ln:
                        n = nn.LayerNorm(ly.No, eps=LN_EPS)
                        n.weight.data.copy_(pol.ln_weight(ly).cpu())
                        n.bias.data.copy_(pol.ln_bias(ly).cpu())
                        s.norm[str(i)] = n
                s.log_std = nn.Parameter(pol.log_std.detach().cpu().clone())

            def forward(s, obs):
                acts = {"obs:" + k: v for k, v in obs.items()}
                M = next(iter(obs.values())).shape[0]
                for i, (ly, m) in enumerate(zip(pol.layers, s.lin)):
                    x = acts[ly.src][:, ly.sc:ly.sc + ly.K]
                    y = m(x)
                    if ly.ln:
                        y = s.norm[str(i)](y)
                    y = getattr(nn, _TORCH_ACT[ly.relu])()(y) if ly.relu else y
                    if ly.dst in ("feat", "vfeat"):
                        f = ly.dst
                        if f not in acts:
                            acts[f] = th.zeros((M, pol.widths[f]), dtype=y.dtype, device=y.device)
                        acts[f] = th.cat([acts[f][:, :ly.dc], y, acts[f][:, ly.dc + ly.No:]], dim=1)
                    else:
                        acts[ly.dst] = y
                s.acts = acts                   # the last pass's layer outputs by buffer name (tests read the trunks' from here)
                return acts["mean"], acts["value"]

            def flat_grad(s):
                g = th.zeros(pol.n_params)
                for i, (ly, m) in enumerate(zip(pol.layers, s.lin)):
                    if ly.frozen or m.weight.grad is None:
                        continue
                    g[ly.w_off:ly.w_off + ly.K * ly.No] = m.weight.grad.reshape(-1)
                    g[ly.b_off:ly.b_off + ly.No] = m.bias.grad
                    if ly.ln:
                        g[ly.g_off:ly.g_off + ly.No] = s.norm[str(i)].weight.grad
                        g[ly.be_off:ly.be_off + ly.No] = s.norm[str(i)].bias.grad
                if s.log_std.grad is not None and pol.n_params > pol.log_std_off:
                    g[pol.log_std_off:] = s.log_std.grad
                return g

        return Ref()
