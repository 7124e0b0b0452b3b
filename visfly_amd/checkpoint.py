"""Data formats either side of the trainers: the reference's YAML blocks and its SB3-style checkpoints.

* ``load_yaml_config`` / ``policy_kwargs_from_reference``: the ``algorithm:`` / ``env:`` blocks of the reference's
  experiment files (exps/examples/alg_cfgs/*/PPO.yaml, env_cfgs/*.yaml; utils/common.py:232-237) are accepted as they
  are; the SB3-style ``policy_kwargs`` (features_extractor_class / features_extractor_kwargs.net_arch.<key>.layer /
  net_arch.pi|vf / activation_fn / optimizer_kwargs) are translated to ``MlpPolicy``'s arguments; the vector extractors are
  ``StateExtractor``, ``StateTargetExtractor`` and ``StateGateExtractor`` (the racing envs' "gate" index as a second branch).  Anything the MFMA
  policy does not implement (image extractors, batch norm, recurrent extractors) raises instead of being dropped;
  layer norm (``ln`` / ``pi_ln`` / ``vf_ln``) becomes ``MlpPolicy``'s ``layer_norm``.
* ``policy_state_dict`` / ``load_policy_state_dict``: the flat parameter buffer <-> the parameter names the
  reference's ``CustomMultiInputActorCriticPolicy`` has in its ``state_dict()`` (utils/policies/policies.py:55-190,
  utils/policies/extractors.py:464-486; SB3 2.2.1 ``ActorCriticPolicy``: features_extractor.<key>_extractor.<i>,
  mlp_extractor.policy_net|value_net.<i>, action_net, value_net, log_std; with a shared extractor SB3 registers the
  same module as pi_features_extractor / vf_features_extractor too, so those aliases are written and accepted).
* ``save`` / ``load``: a zip archive laid out like SB3's ``BaseAlgorithm.save`` (utils/algorithms/PPO.py:418-572 defers
  to it): ``policy.pth`` (torch state_dict, reference names), ``policy.optimizer.pth`` (torch.optim.Adam state_dict
  layout), ``data`` (JSON of the hyper-parameters; plain values, no pickled objects), ``_stable_baselines3_version``.
  ``load`` reads archives written by the reference as well: only ``policy.pth`` and, when present, the optimiser
  moments are taken from them; the pickled ``data`` entries of SB3 are ignored.
"""
import copy
import io
import json
import zipfile
from typing import Dict, List, Optional

import torch as th

from .policy import ACTIVATION_NAMES, INDEX_OBS_KEYS, POLICY_OBS_KEYS, activation_kind

_EXTRACTORS = {"StateExtractor": ("state",), "StateTargetExtractor": ("state", "target"), "StateGateExtractor": ("state", "gate")}
_HEAD_NAMES = {"mean": "action_net", "value": "value_net"}
ARCHIVE_VERSION = "2.2.1"       # environment.yml:275 pins stable-baselines3==2.2.1


def deep_merge(origin: dict, target: dict) -> dict:
    """utils/common.py:210-229: recursive dict merge, `target` wins"""
    out = copy.deepcopy(origin)
    for k, v in target.items():
        out[k] = deep_merge(out[k], v) if isinstance(out.get(k), dict) and isinstance(v, dict) else copy.deepcopy(v)
    return out


def load_yaml_config(path: str) -> dict:
    """utils/common.py:232-237: eval_env inherits from env"""
    import yaml
    with open(path, "r") as f:
        cfg = yaml.safe_load(f)
    if "env" in cfg:
        cfg["eval_env"] = deep_merge(cfg["env"], cfg.get("eval_env") or {})
    return cfg


def extractor_keys(pk: Optional[dict], obs_keys: List[str]) -> tuple:
    """the observation keys the extractor of `pk` reads (SB3-style or native policy_kwargs), by the rule of
    ``policy_kwargs_from_reference``: the named class's, else StateTargetExtractor's where the env has a "target", else StateExtractor's.
    An unknown class name gives () -- the translation raises for it"""
    pk = pk or {}
    if "extractor" in pk:
        return tuple(pk["extractor"].keys()) + tuple(k for k in (pk.get("vf_extractor") or {}) if k not in pk["extractor"])
    name = lambda c: c if isinstance(c, str) else c.__name__
    if pk.get("features_extractor_class") is None and (pk.get("pi_features_extractor_class") is not None or
                                                        pk.get("vf_features_extractor_class") is not None):
        # separate pi / vf extractor classes: the union of both sides' keys, the pi side's first
        sides = [_EXTRACTORS.get(name(pk[k]), ()) for k in ("pi_features_extractor_class", "vf_features_extractor_class") if pk.get(k) is not None]
        return tuple(dict.fromkeys(k for side in sides for k in side))
    cls = pk.get("features_extractor_class", "StateTargetExtractor" if "target" in obs_keys else "StateExtractor")
    return _EXTRACTORS.get(name(cls), ())


def trainer_obs_keys(obs, policy_kwargs):
    """the observation keys a trainer keeps: "state" and "target" as ever, "gate" only when the extractor the policy_kwargs name reads
    it (StateGateExtractor / a native `extractor` dict with a "gate" branch)"""
    avail = [k for k in obs.keys() if k in POLICY_OBS_KEYS]
    named = extractor_keys(policy_kwargs, avail)
    return [k for k in avail if k not in INDEX_OBS_KEYS or k in named]


def _separate_sides(pk):
    """the reference policy's own rules about its extractor arguments (policies.py:132-138) -> None for a network with ONE extractor
    class (shared, or instantiated twice by share_features_extractor=False), else ((pi class, pi kwargs), (vf class, vf kwargs)).
    What its asserts refuse is a ValueError here"""
    pic, vfc = pk.get("pi_features_extractor_class"), pk.get("vf_features_extractor_class")
    if "features_extractor_class" in pk and pk["features_extractor_class"] is None or \
            ("features_extractor_class" not in pk and (pic is not None or vfc is not None)):
        if pic is None or vfc is None:
            raise ValueError("features_extractor_class=None needs both pi_features_extractor_class and vf_features_extractor_class "
                             "(policies.py:133)")
        if pk.get("share_features_extractor", True):
            raise ValueError("pi_features_extractor_class / vf_features_extractor_class need share_features_extractor=False "
                             "(policies.py:136)")
        return (pic, pk.get("pi_features_extractor_kwargs")), (vfc, pk.get("vf_features_extractor_kwargs"))
    if pic is not None or vfc is not None:
        raise ValueError("pi_features_extractor_class / vf_features_extractor_class next to features_extractor_class: the reference "
                         "takes one or the other (policies.py:138)")
    return None


def policy_kwargs_from_reference(pk: Optional[dict], obs_keys: List[str]) -> dict:
    """SB3-style policy_kwargs of the reference's YAMLs -> MlpPolicy arguments (`extractor`, `pi`, `vf`,
    `log_std_init`) plus `weight_decay` from optimizer_kwargs.  Already-native dicts pass through."""
    pk = dict(pk or {})
    if "extractor" in pk:       # already MlpPolicy arguments
        return pk
    out: Dict[str, object] = {}
    sep = _separate_sides(pk)
    if sep is not None:        # pi_features_extractor_class / vf_features_extractor_class: the pi side takes the shared extractor's place below
        pk["features_extractor_class"], pk["features_extractor_kwargs"] = sep[0]
    cls = pk.get("features_extractor_class", "StateTargetExtractor" if "target" in obs_keys else "StateExtractor")
    cls = cls if isinstance(cls, str) else cls.__name__
    if cls not in _EXTRACTORS:
        raise NotImplementedError(f"features_extractor_class {cls}: only the vector extractors "
                                  f"{sorted(_EXTRACTORS)} are on the visual=False path")
    missing = [k for k in _EXTRACTORS[cls] if k not in obs_keys]
    if missing:
        raise ValueError(f"{cls} needs observation keys {missing}")
    arch = (pk.get("features_extractor_kwargs") or {}).get("net_arch") or {}
    # create_mlp (extractors.py:421-430) tests `bn`, then `ln`, by truthiness once for the whole MLP: True or a non-empty list puts
    # the norm behind every hidden Linear, and bn wins over ln
    ext, ln_ext = {}, {}
    for k in _EXTRACTORS[cls]:
        a = arch.get(k) or {}
        if a.get("bn"):
            raise NotImplementedError("batch norm in the extractor MLPs is not implemented")
        ln_ext[k] = bool(a.get("ln"))
        ext[k] = list(a.get("layer", []))
    if arch:        # (no features_extractor_kwargs.net_arch: the trainers' default, the YAMLs' [128, 64] per key)
        out["extractor"] = ext
    # trunks: the policy's activation_fn -- the reference's default is Tanh (policies.py:108; its YAMLs set relu); extractor MLPs:
    # features_extractor_kwargs.activation_fn -- default ReLU (extractors.py:560,583,666).  relu | tanh | elu | leaky_relu
    # (policies.py:64-69) as strings or torch classes
    out["activation"] = activation_kind(pk.get("activation_fn", "tanh"))
    out["extractor_activation"] = activation_kind((pk.get("features_extractor_kwargs") or {}).get("activation_fn", "relu"))
    if pk.get("squash_output", True) is False:
        raise NotImplementedError("squash_output=False: the action head is the tanh-squashed Gaussian (policies.py:114,177-181)")
    if pk.get("use_sde"):
        raise NotImplementedError("use_sde: state-dependent exploration is not implemented")
    out["ortho_init"] = bool(pk.get("ortho_init", True))           # policies.py:109, SB3 ActorCriticPolicy._build
    na = pk.get("net_arch") or {}
    if isinstance(na, list):        # SB3 shorthand: shared sizes for both trunks
        na = dict(pi=na, vf=na)
    for flag in ("pi_bn", "vf_bn", "squash_output"):
        if na.get(flag):
            raise NotImplementedError(f"net_arch.{flag} is not implemented")
    out["pi"], out["vf"] = list(na.get("pi", [64, 64])), list(na.get("vf", [64, 64]))
    # net_arch.pi_ln / vf_ln (policies.py:34-49) and features_extractor_kwargs.net_arch.<key>.ln -> MlpPolicy's layer_norm; the key
    # is there only when some MLP is normalised
    if any(ln_ext.values()) or na.get("pi_ln") or na.get("vf_ln"):
        out["layer_norm"] = dict(extractor=ln_ext, pi=bool(na.get("pi_ln")), vf=bool(na.get("vf_ln")))
    if "log_std_init" in pk:
        out["log_std_init"] = float(pk["log_std_init"])
    if pk.get("share_features_extractor", True) is False:
        # SB3 ActorCriticPolicy: a second instance of the same class and kwargs for the critic; or the vf side's own class / kwargs
        if out.get("layer_norm", {}).get("extractor") and any(out["layer_norm"]["extractor"].values()):
            raise NotImplementedError("layer norm (ln) in the extractor MLPs of a network with separate pi / vf feature extractors is not implemented")
        vcls, vkw = sep[1] if sep is not None else (cls, pk.get("features_extractor_kwargs"))
        vcls = vcls if isinstance(vcls, str) else vcls.__name__
        if vcls not in _EXTRACTORS:
            raise NotImplementedError(f"vf_features_extractor_class {vcls}: only the vector extractors {sorted(_EXTRACTORS)} are on the "
                                      "visual=False path")
        missing = [k for k in _EXTRACTORS[vcls] if k not in obs_keys]
        if missing:
            raise ValueError(f"{vcls} (vf side) needs observation keys {missing}")
        varch = (vkw or {}).get("net_arch") or {}
        vext = {}
        for k in _EXTRACTORS[vcls]:
            a = varch.get(k) or {}
            if a.get("bn"):
                raise NotImplementedError("batch norm in the extractor MLPs is not implemented")
            if a.get("ln"):
                raise NotImplementedError("layer norm (ln) in the extractor MLPs of a network with separate pi / vf feature extractors is not implemented")
            vext[k] = list(a.get("layer", [])) or [128, 64]          # (no net_arch: the trainers' default per key)
        out.setdefault("extractor", {k: [128, 64] for k in _EXTRACTORS[cls]})
        out["vf_extractor"] = vext
        out["vf_extractor_activation"] = activation_kind((vkw or {}).get("activation_fn", "relu"))
    wd = (pk.get("optimizer_kwargs") or {}).get("weight_decay")
    if wd is not None:
        out["weight_decay"] = float(wd)
    return out


def _names(policy):
    """[(layer, reference module prefixes)] in schedule order.  Inside a create_mlp Sequential the i-th Linear is module 2 i (Linear,
    activation) or, in a normalised MLP, 3 i (Linear, LayerNorm, activation: its LayerNorm is module 3 i + 1, `_ln_prefixes`)"""
    out, idx = [], {}
    for ly in policy.layers:
        if ly.dst in _HEAD_NAMES:
            out.append((ly, [_HEAD_NAMES[ly.dst]]))
            continue
        if ly.ext:
            key = ly.src.split(":")[1] if ly.src.startswith(("obs:", "x:", "vx:")) else None
            i = idx.get(("ext", ly.side, key), 0)
            idx[("ext", ly.side, key)] = i + 1
            # separate extractors: the pi side is pi_features_extractor -- and features_extractor, which SB3 registers as the same module
            # with share_features_extractor=False (with pi / vf classes of their own the reference keeps it as a module of the pi class
            # that no forward reads: written as a copy, never preferred on load) -- the vf side vf_features_extractor alone
            pre = {None: ("features_extractor", "pi_features_extractor", "vf_features_extractor"),
                   "pi": ("pi_features_extractor", "features_extractor"), "vf": ("vf_features_extractor",)}[ly.side]
            out.append((ly, [f"{p}.{key}_extractor.{(3 if ly.ln else 2) * i}" for p in pre]))
            continue
        trunk = ly.dst.split(":")[0]
        i = idx.get(trunk, 0)
        idx[trunk] = i + 1
        out.append((ly, [f"mlp_extractor.{'policy_net' if trunk == 'pi' else 'value_net'}.{(3 if ly.ln else 2) * i}"]))
    return out


def _ln_prefixes(prefixes):
    """module names of the nn.LayerNorm behind the Linear named `prefixes`: the next index of the same Sequential"""
    return [f"{p.rsplit('.', 1)[0]}.{int(p.rsplit('.', 1)[1]) + 1}" for p in prefixes]


def policy_state_dict(policy) -> Dict[str, th.Tensor]:
    sd = {"log_std": policy.log_std.detach().cpu().clone()}
    for ly, prefixes in _names(policy):
        w, b = policy.weight(ly).detach().cpu().clone(), policy.bias(ly).detach().cpu().clone()
        for p in prefixes:
            sd[p + ".weight"], sd[p + ".bias"] = w, b
        if ly.ln:
            g, be = policy.ln_weight(ly).detach().cpu().clone(), policy.ln_bias(ly).detach().cpu().clone()
            for p in _ln_prefixes(prefixes):
                sd[p + ".weight"], sd[p + ".bias"] = g, be
    return sd


def _check_shapes(policy, sd):
    """every layer's tensors before any is copied: a refused state_dict leaves the policy as it was.  Shapes first (ValueError at the
    first layer, in schedule order, whose tensors are there with another shape -- a network with or without an extractor branch differs
    in the trunks' first layers at the latest), then missing names (KeyError)"""
    missing = None
    for ly, prefixes in _names(policy):
        p = next((p for p in prefixes if p + ".weight" in sd), None)
        if p is None:
            missing = missing or f"state_dict has none of {[q + '.weight' for q in prefixes]}"
            continue
        w, b = sd[p + ".weight"], sd[p + ".bias"]
        if tuple(w.shape) != (ly.No, ly.K) or tuple(b.shape) != (ly.No,):
            raise ValueError(f"{p}: shape {tuple(w.shape)} does not match the policy's layer ({ly.No}, {ly.K})")
        if ly.ln:
            q = _ln_prefixes(prefixes)[prefixes.index(p)]
            if q + ".weight" not in sd or q + ".bias" not in sd:
                missing = missing or f"state_dict has no {q}.weight / .bias (the LayerNorm behind {p})"
            elif tuple(sd[q + ".weight"].shape) != (ly.No,) or tuple(sd[q + ".bias"].shape) != (ly.No,):
                raise ValueError(f"{q}: shape {tuple(sd[q + '.weight'].shape)} does not match the policy's LayerNorm ({ly.No},)")
    if missing:
        raise KeyError(missing)


def load_policy_state_dict(policy, sd: Dict[str, th.Tensor], strict: bool = True):
    used = set()
    _check_shapes(policy, sd)
    with th.no_grad():
        for ly, prefixes in _names(policy):
            p = next((p for p in prefixes if p + ".weight" in sd), None)
            if p is None:
                raise KeyError(f"state_dict has none of {[q + '.weight' for q in prefixes]}")
            w, b = sd[p + ".weight"], sd[p + ".bias"]
            if tuple(w.shape) != (ly.No, ly.K) or tuple(b.shape) != (ly.No,):
                raise ValueError(f"{p}: shape {tuple(w.shape)} does not match the policy's layer ({ly.No}, {ly.K})")
            policy.weight(ly).copy_(w.to(policy.device, th.float32))
            policy.bias(ly).copy_(b.to(policy.device, th.float32))
            used.update(q + s for q in prefixes for s in (".weight", ".bias"))
            if ly.ln:
                lp = _ln_prefixes(prefixes)
                q = lp[prefixes.index(p)]
                if q + ".weight" not in sd or q + ".bias" not in sd:
                    raise KeyError(f"state_dict has no {q}.weight / .bias (the LayerNorm behind {p})")
                g, be = sd[q + ".weight"], sd[q + ".bias"]
                if tuple(g.shape) != (ly.No,) or tuple(be.shape) != (ly.No,):
                    raise ValueError(f"{q}: shape {tuple(g.shape)} does not match the policy's LayerNorm ({ly.No},)")
                policy.ln_weight(ly).copy_(g.to(policy.device, th.float32))
                policy.ln_bias(ly).copy_(be.to(policy.device, th.float32))
                used.update(r + s for r in lp for s in (".weight", ".bias"))
        if "log_std" in sd:
            policy.log_std.copy_(sd["log_std"].to(policy.device, th.float32).reshape(-1))
            used.add("log_std")
        elif strict:
            raise KeyError("state_dict has no log_std")
    extra = sorted(set(sd) - used)
    if strict and extra:
        raise KeyError(f"unexpected keys in state_dict (layers the MFMA policy does not have): {extra[:8]}")
    policy.mark_updated()
    return extra


def _param_order(policy):
    """torch.optim.Adam numbers parameters in module registration order (SB3: features_extractor, mlp_extractor,
    action_net, value_net; log_std is registered first in ActorCriticPolicy._build): -> [(offset, shape)]"""
    order = [(policy.log_std_off, (policy.n_params - policy.log_std_off,))]
    named = _names(policy)
    rank = lambda pre: (0 if "features_extractor" in pre else 1 if pre.startswith("mlp_extractor.policy") else
                        2 if pre.startswith("mlp_extractor.value") else 3 if pre == "action_net" else 4)
    for ly, prefixes in sorted(named, key=lambda x: rank(x[1][0])):
        order += [(ly.w_off, (ly.No, ly.K)), (ly.b_off, (ly.No,))]
        if ly.ln:          # the LayerNorm is registered right behind its Linear: weight, bias
            order += [(ly.g_off, (ly.No,)), (ly.be_off, (ly.No,))]
    return order


def activation_spec(policy) -> dict:
    """the (trunk, extractor) activations of a policy under the names MlpPolicy.spec uses, ReLU included"""
    return dict(activation=ACTIVATION_NAMES[policy.act], extractor_activation=ACTIVATION_NAMES[policy.ext_act])


def check_activations(policy, spec):
    """weights must never run through another nonlinearity than the one they were trained with: ValueError when the activations an
    archive's spec names differ from the policy's.  A spec without the fields (archives written before they existed) is a ReLU network."""
    spec = spec if isinstance(spec, dict) else {}
    want = activation_kind(spec.get("activation", "relu")), activation_kind(spec.get("extractor_activation", "relu"))
    if want != (policy.act, policy.ext_act):
        have = activation_spec(policy)
        raise ValueError(f"the archive holds a network with activations {spec.get('activation', 'relu')} (trunks) / "
                         f"{spec.get('extractor_activation', 'relu')} (extractor), this trainer's policy has {have['activation']} / "
                         f"{have['extractor_activation']}: pass the archive's activation_fn (or use load(), which reads it)")


def layer_norm_spec(spec) -> dict:
    """the `layer_norm` entry of a policy spec with every flag spelled out; a spec without it (every archive written before LayerNorm,
    every network without it) is all false"""
    spec = spec if isinstance(spec, dict) else {}
    ln = spec.get("layer_norm") or {}
    return dict(extractor={k: bool((ln.get("extractor") or {}).get(k, False)) for k in spec.get("extractor", {})},
                pi=bool(ln.get("pi", False)), vf=bool(ln.get("vf", False)))


def check_layer_norm(policy, spec):
    """like check_activations: weights trained with (without) LayerNorm must not run without (with) it.  ValueError when the archive's
    spec and the policy disagree about which MLPs are normalised"""
    if not isinstance(spec, dict) or "extractor" not in spec:
        return
    want, have = layer_norm_spec(spec), layer_norm_spec(policy.spec)
    if (want["pi"], want["vf"], sorted(k for k, v in want["extractor"].items() if v)) != \
            (have["pi"], have["vf"], sorted(k for k, v in have["extractor"].items() if v)):
        raise ValueError(f"the archive holds a network with layer_norm {want}, this trainer's policy has {have}: pass the archive's "
                         "ln / pi_ln / vf_ln flags (or use load(), which reads them)")


def check_separate_extractors(policy, spec):
    """like check_activations: an archive's spec and the policy must agree about the critic's own extractor (``vf_extractor``) --
    ValueError otherwise, before any tensor is compared"""
    if not isinstance(spec, dict) or "extractor" not in spec:
        return
    want, have = spec.get("vf_extractor"), policy.spec.get("vf_extractor")
    norm = lambda e: None if e is None else {k: list(v) for k, v in e.items()}
    if norm(want) != norm(have):
        raise ValueError(f"the archive holds a network with vf_extractor {want} (None: one shared feature extractor), this trainer's policy "
                         f"has {have}: pass the archive's share_features_extractor / vf_features_extractor_class (or use load(), which "
                         "reads them)")
    if want is not None and spec.get("vf_extractor_activation", spec.get("extractor_activation", "relu")) != \
            policy.spec.get("vf_extractor_activation", policy.spec.get("extractor_activation", "relu")):
        raise ValueError(f"the archive's vf extractor runs {spec.get('vf_extractor_activation')}, this trainer's policy "
                         f"{policy.spec.get('vf_extractor_activation')}")


def _hyper(trainer) -> dict:
    keys = ("n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "clip_range", "ent_coef", "vf_coef", "max_grad_norm",
            "lr", "weight_decay", "adam_eps", "betas", "normalize_advantage", "target_kl", "seed", "H", "num_timesteps", "_opt_step",
            "clip_range_vf", "_noise_step")
    out = {k: getattr(trainer, k) for k in keys if hasattr(trainer, k)}
    # schedules (callables of progress_remaining) are archived as their current value: an archive holds data, not code
    out = {k: (trainer._now(v) if callable(v) else v) for k, v in out.items()}
    out["learning_rate"] = out.pop("lr", None)
    out["algorithm"], out["policy_spec"] = type(trainer).__name__, dict(trainer.policy.spec)
    if hasattr(trainer, "any_activation"):       # BPTT / SHAC: the activations are always named (PPO's ReLU archives keep the r05 spec)
        out["policy_spec"].update(activation_spec(trainer.policy))
    out["obs_dims"] = trainer.policy.obs_dims
    return out


def save(trainer, path: str):
    """trainer: PPO / BPTT / SHAC of this package (policy + Adam moments + hyper-parameters)"""
    pol = trainer.policy
    path = path if str(path).endswith(".zip") else f"{path}.zip"
    opt_state = {}
    for i, (off, shape) in enumerate(_param_order(pol)):
        n = 1
        for s in shape:
            n *= s
        opt_state[i] = dict(step=th.tensor(float(trainer._opt_step)),
                            exp_avg=trainer.exp_avg[off:off + n].detach().cpu().reshape(shape).clone(),
                            exp_avg_sq=trainer.exp_avg_sq[off:off + n].detach().cpu().reshape(shape).clone())
    group = dict(lr=trainer.lr, betas=tuple(trainer.betas), eps=trainer.adam_eps, weight_decay=trainer.weight_decay,
                 amsgrad=False, params=list(range(len(opt_state))))
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("data", json.dumps(_hyper(trainer), indent=1, default=str))
        for name, obj in (("policy.pth", policy_state_dict(pol)),
                          ("policy.optimizer.pth", dict(state=opt_state, param_groups=[group]))):
            buf = io.BytesIO()
            th.save(obj, buf)
            z.writestr(name, buf.getvalue())
        z.writestr("_stable_baselines3_version", ARCHIVE_VERSION)
    return path


def read_archive(path: str):
    """-> (policy state_dict, optimiser state_dict or None, data dict or None)"""
    path = path if str(path).endswith(".zip") else f"{path}.zip"
    with zipfile.ZipFile(path) as z:
        names = set(z.namelist())
        if "policy.pth" not in names:
            raise FileNotFoundError(f"{path}: no policy.pth in the archive")
        sd = th.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
        opt = None
        if "policy.optimizer.pth" in names:
            opt = th.load(io.BytesIO(z.read("policy.optimizer.pth")), map_location="cpu", weights_only=True)
        data = None
        if "data" in names:
            try:
                data = json.loads(z.read("data").decode())
            except (ValueError, UnicodeDecodeError):
                data = None
    return sd, opt, data


_CTOR_KEYS = ("n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "clip_range", "clip_range_vf", "ent_coef", "vf_coef",
              "max_grad_norm", "learning_rate", "weight_decay", "adam_eps", "betas", "normalize_advantage", "target_kl", "seed",
              "horizon")


def ctor_kwargs_from_archive(path: str, overrides: Optional[dict] = None) -> dict:
    """constructor kwargs for ``cls.load`` (SB3 BaseAlgorithm.load restores them from the archive's `data`, PPO.py:432-572):
    the saved hyper-parameters and network shape, overridden by the caller's kwargs.  Archives written by the reference carry
    a pickled `data` this package does not unpickle -- then only the caller's kwargs apply."""
    _sd, _opt, data = read_archive(path)
    kw = {}
    if isinstance(data, dict):
        for k in _CTOR_KEYS:
            v = data.get("H") if k == "horizon" else data.get(k)
            if v is not None and not isinstance(v, dict):
                kw[k] = tuple(v) if k == "betas" else v
        spec = data.get("policy_spec")
        if isinstance(spec, dict) and "extractor" in spec:
            kw["policy_kwargs"] = dict(extractor=spec["extractor"], pi=spec["pi"], vf=spec["vf"], activation=spec.get("activation", "relu"),
                                       extractor_activation=spec.get("extractor_activation", "relu"))
            if spec.get("layer_norm"):
                kw["policy_kwargs"]["layer_norm"] = spec["layer_norm"]
            if spec.get("vf_extractor"):
                kw["policy_kwargs"]["vf_extractor"] = spec["vf_extractor"]
                if spec.get("vf_extractor_activation"):
                    kw["policy_kwargs"]["vf_extractor_activation"] = spec["vf_extractor_activation"]
    kw.update(overrides or {})
    return kw


def load_into(trainer, path: str, load_optimizer: bool = True):
    """in-place load (SB3 ``set_parameters``): policy parameters and, if the archive has them and the layout matches,
    the Adam moments and step count"""
    sd, opt, data = read_archive(path)
    pol = trainer.policy
    if hasattr(trainer, "any_activation") and isinstance(data, dict):      # BPTT / SHAC archives (see _hyper)
        check_activations(pol, data.get("policy_spec"))
    if isinstance(data, dict):
        check_layer_norm(pol, data.get("policy_spec"))
        check_separate_extractors(pol, data.get("policy_spec"))
    load_policy_state_dict(pol, sd, strict=True)
    if load_optimizer and opt and opt.get("state"):
        order = _param_order(pol)
        st = opt["state"]
        if len(st) == len(order) and all(tuple(st[i]["exp_avg"].shape) == order[i][1] for i in range(len(order))):
            for i, (off, shape) in enumerate(order):
                n = st[i]["exp_avg"].numel()
                trainer.exp_avg[off:off + n] = st[i]["exp_avg"].reshape(-1).to(pol.device, th.float32)
                trainer.exp_avg_sq[off:off + n] = st[i]["exp_avg_sq"].reshape(-1).to(pol.device, th.float32)
            trainer._opt_step = int(float(st[0]["step"]))
        else:
            import warnings
            warnings.warn(f"{path}: the optimiser state does not match this policy's parameter layout "
                          f"({len(st)} vs {len(order)} tensors) -- Adam moments NOT restored", stacklevel=2)
    if isinstance(data, dict) and "num_timesteps" in data and not isinstance(data["num_timesteps"], dict):
        trainer.num_timesteps = int(data["num_timesteps"])
    if isinstance(data, dict) and hasattr(trainer, "_noise_step") and isinstance(data.get("_noise_step"), int):
        trainer._noise_step = data["_noise_step"]     # BPTT / SHAC over a globally keyed env: rows of vf_noise_fill drawn so far
    return trainer
