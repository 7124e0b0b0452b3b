"""Register-chained MLP kernels for network shapes libvisfly_amd.so holds no instance of: compiled on first use.

The chain kernels keep a wave's activations in MFMA accumulator registers, so the layer shapes are compile-time
(csrc/vf_mlp_chain.hpp).  The library carries the YAML-default shapes of the reference (one or two [128, 64] extractor branches,
[64, 64] trunks); for any other `features_extractor_kwargs.net_arch` / `net_arch=dict(pi=.., vf=..)` (utils/policies/extractors.py:376-449)
this module writes a translation unit that names the shape (csrc/vf_mlp_chain_gen.hpp: ChainNetG<Spec>), compiles it with hipcc for gfx950
into ``csrc/jit/libvf_chain_<hash>.so`` (four parts in parallel, ~40 s once; cached by the hash of the shape, the chain headers and the
flags) and registers it with the library (vf_chain_plugin_load).  ``__graft_entry__.build()`` pre-builds the shapes the tests use, so
the GPU box finds them in the snapshot.

Shapes that qualify: 1-2 observation branches of <= 32 columns (the second one: NavigationEnv's constant "target" rows, or the racing envs'
1-wide "gate" column, which the persistent launches of a racing kind take from the index the wave holds instead of from memory), 1-4 layers per branch / trunk, widths in multiples of 32 up to 128,
the actor-critic heads (4, 1), the SAC-style Actor's (4, 4), or the twin critic's (1, 1) with its pass-through action input (<= 4 columns)
behind one or two observation branches, as long as features (+) action fit the trunks' 128 input columns (the pass-through tile counts as
one of the four: sum of the branches' last widths + action columns <= 128; the reference-default two-branch critic, 64 + 64 + 4 = 132
columns, does not qualify).  Everything else keeps running on the block-tile kernels (MlpPolicy warns once).
``VISFLY_AMD_JIT=0`` switches the compilation off.

An actor-critic with SEPARATE pi / vf feature extractors (MlpPolicy ``vf_extractor``: the reference's share_features_extractor=False and
its pi_features_extractor_class / vf_features_extractor_class) qualifies when each side alone does and the two sides read at most two
observation keys in all.  Its translation unit names two single-trunk Specs -- A: pi-side extractor + pi trunk + the 4-wide mean head, B:
vf-side extractor + vf trunk + the 1-wide value head -- and its forward / fused PPO step give each of two waves per 32 rows one of them
(csrc/vf_mlp_chain_sep.hpp).  Own slug, name and cache file; never a built-in class; no roll-out, BPTT or evaluation plugin.

Three more plugin kinds hold ONE instance each of a persistent launch for a generated class under one env kind / action type / integrator /
motor-lag setting, built when a trainer first needs them: the roll-out plugin (PPO's collect_rollouts: ``ensure_rollout``,
csrc/vf_ppo_rollout_kernel.hpp), the BPTT plugin (both halves of a BPTT / SHAC horizon for an actor class: ``ensure_bptt``,
csrc/vf_bptt_rollout_kernel.hpp + csrc/vf_bptt_reverse_kernel.hpp) and the evaluation plugin (deterministic episodes of
``visfly_amd.evaluate``: ``ensure_eval``, csrc/vf_eval_rollout_kernel.hpp) of a class with a 4-wide mean head.  What tells the kinds apart
-- slug suffix, compile parts, hashed headers, source tail, which shapes qualify -- is one row each of ``_KINDS``; the ``ensure*`` functions
are one call each into ``_ensure``.
"""
import hashlib
import os
import shutil
import subprocess
import tempfile
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

from ._build import CSRC, HIPCC_FLAGS, INCLUDE

JIT_DIR = os.path.join(CSRC, "jit")
MAX_DEPTH = 4
# the shapes libvisfly_amd.so itself instantiates (NetHover / NetNav and their policy-only classes)
_BUILTIN = {((16,), ((4, 2),), (2, 2), (2, 2)), ((16, 8), ((4, 2), (4, 2)), (2, 2), (2, 2)),
            ((16,), ((4, 2),), (2, 2), (2, 2), (4, 4)), ((16, 8), ((4, 2), (4, 2)), (2, 2), (2, 2), (4, 4)),      # (.., (4, 4)): the SAC-style Actor
            ((16,), ((4, 2),), (2, 2), (2, 2), (1, 1))}                                                            # (.., (1, 1)): its twin critic (NetCriticHover)
_HEADERS = ("vf_mlp_chain.hpp", "vf_mlp_chain_bwd.hpp", "vf_mlp_chain_kernels.hpp", "vf_mlp_chain_gen.hpp", "vf_chain_plugin.hpp",
            "vf_common.hpp", "vf_ppo_device.hpp")
_ROLLOUT_HEADERS = ("vf_ppo_rollout_kernel.hpp", "vf_env_epilogue.hpp", "vf_env_device.hpp", "vf_dyn_device.hpp", "vf_xmath.hpp",
                    "vf_quad.hpp", "vf_handles.hpp")
_BPTT_HEADERS = _ROLLOUT_HEADERS[1:] + ("vf_bptt_rollout_kernel.hpp", "vf_bptt_reverse_kernel.hpp", "vf_env_bwd_body.hpp", "vf_env_bwd_quad.hpp",
                                        "vf_dyn_quad.hpp")
_EVAL_HEADERS = _ROLLOUT_HEADERS + ("vf_eval_rollout_kernel.hpp",)
_loaded = {}
# shapes compiled ahead of time by __graft_entry__.build() (name -> observation widths, extractor layers, pi, vf): the ones the parity
# tests run (tests/test_chain_jit_gpu.py), so that a GPU box without a warm cache finds them in the snapshot
PREBUILD = {
    "verdict": ({"state": 13, "target": 3}, {"state": [128, 64], "target": [128, 64]}, [128, 128], [32]),
    "one_layer_extractor": ({"state": 13}, {"state": [64]}, [64], [64, 64, 32]),
    "ragged": ({"state": 13, "target": 3}, {"state": [96, 64, 32], "target": [32]}, [32, 32, 32], [128]),
    # 30 forward tiles: the fused PPO step keeps the ReLU masks as bits (csrc/vf_mlp_chain_gen.hpp: kGenLiveTiles)
    "wide": ({"state": 13, "target": 3}, {"state": [128, 64], "target": [128, 64]}, [128, 128], [128, 128]),
    # StateGateExtractor on the racing envs (tests/test_gate_extractor_gpu.py): the second branch is the 1-wide gate column (KIN 8).
    # RacingEnv2's 16 and RacingEnv's 13 state columns both pad to KIN 16: one class
    "gate_pi": ({"state": 16, "gate": 1}, {"state": [64, 32], "gate": [32]}, [32], [32]),
}
# the SAC-style Actor (heads (4, 4); td_policies.Actor: `pi` = latent_pi, `vf` = log_latent_pi) on a non-default shape: (.., head_dims)
# the reference policy's DEFAULT activations (Tanh trunks, policies.py:108; ReLU extractor MLPs, extractors.py:666) on the YAMLs' shapes:
# (.., head_dims, (trunk, extractor) activations)
PREBUILD_ACT = {
    "tanh_nav": ({"state": 13, "target": 3}, {"state": [128, 64], "target": [128, 64]}, [64, 64], [64, 64], (4, 1), (2, 1)),
    "tanh_hover": ({"state": 13}, {"state": [128, 64]}, [64, 64], [64, 64], (4, 1), (2, 1)),
    "elu_leaky_nav": ({"state": 13, "target": 3}, {"state": [128, 64], "target": [128, 64]}, [64, 64], [64, 64], (4, 1), (3, 4)),
    # BPTT's two actors with a Tanh / ELU / LeakyReLU trunk (activation_fn; the extractor MLP keeps its default ReLU) on the sac_hover sizes:
    # the SAC-style Actor (policy="MultiInputPolicy") and the one-head MlpPolicy actor, whose horizons step the policy-only class
    "sac_hover_tanh": ({"state": 13}, {"state": [64, 64, 32]}, [32], [32], (4, 4), (2, 1)),
    "sac_hover_elu": ({"state": 13}, {"state": [64, 64, 32]}, [32], [32], (4, 4), (3, 1)),
    "sac_hover_leaky": ({"state": 13}, {"state": [64, 64, 32]}, [32], [32], (4, 4), (4, 1)),
    "pi_hover_tanh": ({"state": 13}, {"state": [64, 64, 32]}, [32], [32], (4, 1), (2, 1)),
    "pi_hover_elu": ({"state": 13}, {"state": [64, 64, 32]}, [32], [32], (4, 1), (3, 1)),
    "pi_hover_leaky": ({"state": 13}, {"state": [64, 64, 32]}, [32], [32], (4, 1), (4, 1)),
    # ... and on the reference's sizes: the actor of tests/golden/bptt_loop_hover_tanh.npz (the reference's own BPTT.learn with activation_fn=Tanh; its
    # env replays recorded spawns, so its horizon steps launch by launch: the chain class alone)
    "sac_loop_tanh": ({"state": 13}, {"state": [128, 64]}, [64, 64], [64, 64], (4, 4), (2, 1)),
}
# the twin critic (heads (1, 1) + pass-through action; td_policies.ContinuousCritic) on non-default shapes: (.., head_dims, passthrough)
PREBUILD_CRITIC = {
    "critic_hover": ({"state": 13, "action": 4}, {"state": [64, 64, 32]}, [32], [32], (1, 1), ("action",)),      # SHAC(net_arch pi=[32]) over features [64, 64, 32]
    "critic_wide": ({"state": 13, "action": 4}, {"state": [128, 96]}, [128, 64], [128, 64], (1, 1), ("action",)),
    # ... over a two-branch extractor (NB = 2 with PASS; feature tiles in the order branch 0, branch 1, action):
    # the critic SHAC builds next to PREBUILD_SAC["gate_sac"] (StateGateExtractor on the racing envs; the gate column is branch 1, KIN 8)
    "critic_gate": ({"state": 16, "gate": 1, "action": 4}, {"state": [64, 32], "gate": [32]}, [32], [32], (1, 1), ("action",)),
    # ... and next to "sac_nav_bptt" (StateTargetExtractor on NavigationEnv): 64 + 32 + 4 = 100 columns into qf0 / qf1
    "critic_nav": ({"state": 13, "target": 3, "action": 4}, {"state": [64, 64], "target": [32]}, [64], [64], (1, 1), ("action",)),
}
PREBUILD_SAC = {
    "sac_nav": ({"state": 13, "target": 3}, {"state": [128, 64], "target": [64]}, [128, 64], [64], (4, 4)),
    "sac_hover": ({"state": 13}, {"state": [64, 64, 32]}, [32], [32], (4, 4)),      # (the Actor BPTT builds for pi=[32]: log_latent_pi mirrors latent_pi)
    "sac_nav_bptt": ({"state": 13, "target": 3}, {"state": [64, 64], "target": [32]}, [64], [64], (4, 4)),      # ... over StateTargetExtractor, pi=[64]
    "gate_sac": ({"state": 16, "gate": 1}, {"state": [64, 32], "gate": [32]}, [32], [32], (4, 4)),              # ... over StateGateExtractor (BPTT's Actor, SHAC)
}
# separate pi / vf feature extractors (MlpPolicy ``vf_extractor``; tests/test_separate_extractors_gpu.py): (observation widths, pi-side
# extractor, pi, vf, vf-side extractor, (trunk, pi extractor, vf extractor) activations)
PREBUILD_SEP = {
    "sep_sym": ({"state": 13}, {"state": [64, 32]}, [32], [32], {"state": [64, 32]}, (1, 1, 1)),
    # an asymmetric critic: the actor reads "state", the critic "state" and "target"; different depths and widths per role
    "sep_asym": ({"state": 13, "target": 3}, {"state": [64]}, [32, 32], [64], {"state": [64, 32], "target": [32]}, (1, 1, 1)),
    "sep_asym_tanh": ({"state": 13, "target": 3}, {"state": [64]}, [32, 32], [64], {"state": [64, 32], "target": [32]}, (2, 1, 1)),
    # the reference's two forms on NavigationEnv with its default Tanh trunks: StateTargetExtractor twice, and StateExtractor /
    # StateTargetExtractor (what the trainer tests and the fixture run)
    "sep_nav_tanh": ({"state": 13, "target": 3}, {"state": [64, 32], "target": [32]}, [32], [32], {"state": [64, 32], "target": [32]}, (2, 1, 1)),
    # the YAMLs' sizes on both sides (tools/bench_separate_extractors.py): 17 forward tiles per role -- the fused step keeps its ReLU masks
    # as bits (csrc/vf_mlp_chain_sep.hpp: kSepLiveTiles)
    "sep_default": ({"state": 13, "target": 3}, {"state": [128, 64], "target": [128, 64]}, [64, 64], [64, 64],
                    {"state": [128, 64], "target": [128, 64]}, (1, 1, 1)),
}
# ... and their roll-out plugins for the configurations tests/test_ppo_gpu.py runs: (shape name, (VF_ENV_*, VF_ACT_*, VF_INT_*, ctrl_delay))
# ... and the BPTT plugins (both persistent launches of a horizon) tests/test_chain_jit_gpu.py runs: (shape name in PREBUILD_SAC / PREBUILD,
# (kernel-side env kind, VF_ACT_*, VF_INT_*, ctrl_delay)); the names ending in an activation are PREBUILD_ACT's (tests/test_bptt_activations_gpu.py)
PREBUILD_BPTT = [("sac_hover", (0, 1, 0, True)), ("sac_nav_bptt", (1, 1, 0, True)), ("one_layer_extractor", (0, 0, 0, True)),
                 ("sac_hover", (3, 0, 0, True)),        # RacingEnv2: kernel-side kind VF_ENV_RACING2, thrust
                 ("sac_hover_tanh", (0, 1, 0, True)), ("sac_hover_elu", (0, 1, 0, True)), ("sac_hover_leaky", (0, 1, 0, True)),
                 ("pi_hover_tanh", (0, 1, 0, True)), ("pi_hover_elu", (0, 1, 0, True)), ("pi_hover_leaky", (0, 1, 0, True)),
                 ("sac_hover_tanh", (2, 0, 0, True)),   # RacingEnv, thrust
                 # StateGateExtractor: the gate column as branch 1 over the racing kinds (RacingEnv2 / RacingEnv, thrust)
                 ("gate_sac", (3, 0, 0, True)), ("gate_pi", (3, 0, 0, True)), ("gate_sac", (2, 0, 0, True))]
PREBUILD_ROLLOUT = [("verdict", (1, 1, 0, True)), ("one_layer_extractor", (0, 1, 1, False)), ("one_layer_extractor", (1, 1, 0, True)),
                    ("one_layer_extractor", (2, 1, 0, True)), ("one_layer_extractor", (3, 1, 0, True)),      # RacingEnv / RacingEnv2 (kernel-side kind 3)
                    ("gate_pi", (3, 1, 0, True)),                                                             # StateGateExtractor on RacingEnv2
                    # the geometric controller's action types (tests/test_geometric_rollout_gpu.py): velocity on HoverEnv, position on NavigationEnv2
                    ("one_layer_extractor", (0, 2, 0, True)), ("one_layer_extractor", (1, 3, 0, True)),
                    ("tanh_nav", (1, 1, 0, True))]                                                            # the Tanh default policy on NavigationEnv
# ... and the evaluation plugins tests/test_evaluate_gpu.py runs: (shape name, (kernel-side env kind, VF_ACT_*, VF_INT_*, ctrl_delay)) -- the Tanh
# default policy on NavigationEnv, StateGateExtractor's actor-critic on RacingEnv2, BPTT's Tanh SAC-style Actor on HoverEnv
PREBUILD_EVAL = [("tanh_nav", (1, 1, 0, True)), ("gate_pi", (3, 1, 0, True)), ("sac_hover_tanh", (0, 1, 0, True)),
                 ("tanh_nav", (1, 3, 0, True))]                                                               # ... with position actions


def shape_of(obs_dims, extractor, pi, vf, head_dims=(4, 1), passthrough=(), acts=(1, 1), vf_extractor=None, vf_extractor_act=None):
    """(KIN, extractor widths in tiles, pi tiles, vf tiles[, (4, 4)][, ("act", trunks, extractor)]) of a network the generated chain classes
    cover, else None.  Heads (4, 1): the actor-critic of the PPO policies; (4, 4): the SAC-style Actor of BPTT / SHAC (mu / log_std heads).
    acts: VF_ACTIVATION_* of the trunks / the extractor MLPs -- (1, 1) = ReLU networks (no element: the keys of r05's shapes).
    vf_extractor ({key: hidden sizes}; vf_extractor_act: its activation, default the pi side's): the critic has an extractor of its own
    (MlpPolicy ``vf_extractor``) -- `extractor` is then the pi side's, and the shape gains the element ("sep", KIN of the vf side, its
    extractor widths in tiles, which of the network's inputs each of its branches reads, its activation).  Such a network qualifies when
    each side alone does and the union of the two sides' observation keys is at most two inputs"""
    if vf_extractor is not None:
        if tuple(head_dims) != (4, 1) or passthrough or not vf_extractor:
            return None
        union = list(extractor) + [k for k in vf_extractor if k not in extractor]
        if len(union) > 2:
            return None
        a = shape_of(obs_dims, extractor, pi, vf, acts=acts)
        eact = int(acts[1] if vf_extractor_act is None else vf_extractor_act)
        b = shape_of(obs_dims, vf_extractor, pi, vf)
        if a is None or b is None:
            return None
        return a + (("sep", b[0], b[1], tuple(union.index(k) for k in vf_extractor), eact),)
    critic = tuple(head_dims) == (1, 1)      # td_policies.ContinuousCritic: th.cat([features, actions]) -> qf0 / qf1 (one pass-through input of <= 4 columns)
    if critic != bool(passthrough) or tuple(head_dims) not in ((4, 1), (4, 4), (1, 1)) or not 1 <= len(extractor) <= 2:
        return None
    if critic and (len(passthrough) != 1 or not 1 <= int(obs_dims[list(passthrough)[0]]) <= 4):
        return None
    # features (+) pass-through columns are the K of the trunks' first layers: at most 128 (four input tiles, the pass-through tile included)
    if critic and sum(int(h[-1]) for h in extractor.values() if h) + int(obs_dims[list(passthrough)[0]]) > 128:
        return None
    kin, ew = [], []
    for k, hidden in extractor.items():
        d = int(obs_dims[k])
        if not 1 <= d <= 32 or not 1 <= len(hidden) <= MAX_DEPTH:
            return None
        kin.append((d + 7) & ~7)
        ew.append(tuple(int(h) for h in hidden))
    trunks = (tuple(int(h) for h in pi), tuple(int(h) for h in vf))
    if not all(1 <= len(t) <= MAX_DEPTH for t in trunks):
        return None
    widths = [h for e in ew for h in e] + [h for t in trunks for h in t]
    if any(h % 32 or not 32 <= h <= 128 for h in widths):
        return None
    tiles = lambda t: tuple(h // 32 for h in t)
    sh = tuple(kin), tuple(tiles(e) for e in ew), tiles(trunks[0]), tiles(trunks[1])
    sh = sh if tuple(head_dims) == (4, 1) else sh + (tuple(head_dims),)
    return sh if tuple(acts) == (1, 1) else sh + (("act", int(acts[0]), int(acts[1])),)


def is_builtin(shape):
    return shape in _BUILTIN          # (ReLU networks only: a shape with an ("act", ..) element is never one of these)


def _heads(shape):
    return (4, 4) if (4, 4) in shape[4:] else (1, 1) if (1, 1) in shape[4:] else (4, 1)


def _acts(shape):
    """(trunk activation, extractor activation) as VF_ACTIVATION_*"""
    for e in shape[4:]:
        if e and e[0] == "act":
            return e[1], e[2]
    return 1, 1


def _sep(shape):
    """the ("sep", ..) element of a network with separate pi / vf extractors, else None"""
    for e in shape[4:]:
        if e and e[0] == "sep":
            return e
    return None


_ACT_NAME = {1: "relu", 2: "tanh", 3: "elu", 4: "leaky_relu"}


def name_of(shape):
    kin, ew, pw, vw = shape[:4]
    f = lambda t: "[" + ",".join(str(32 * x) for x in t) + "]"
    a = _acts(shape)
    sep = _sep(shape)
    if sep:
        return ("pi: " + " ".join(f"in{k}{f(e)}" for k, e in zip(kin, ew)) + f" pi{f(pw)} | vf: " +
                " ".join(f"in{k}@{i}{f(e)}" for k, e, i in zip(sep[1], sep[2], sep[3])) + f" vf{f(vw)}" +
                ("" if a == (1, 1) and sep[4] == 1 else f" act {_ACT_NAME[a[0]]}/{_ACT_NAME[a[1]]}/{_ACT_NAME[sep[4]]}"))
    return (" ".join(f"in{k}{f(e)}" for k, e in zip(kin, ew)) + f" pi{f(pw)} vf{f(vw)}" + {(4, 4): " heads 4/4", (1, 1): " (+) action, heads 1/1", (4, 1): ""}[_heads(shape)] +
            ("" if a == (1, 1) else f" act {_ACT_NAME[a[0]]}/{_ACT_NAME[a[1]]}"))


def source(shape):
    """the generated translation unit: a Spec (csrc/vf_mlp_chain_gen.hpp) and the plugin's entry points"""
    kin, ew, pw, vw = shape[:4]
    pad = lambda t, n=MAX_DEPTH: ", ".join(str(x) for x in (tuple(t) + (0,) * n)[:n])
    nb = len(kin)
    if _sep(shape):
        return _sep_source(shape)
    return f"""// generated by visfly_amd/_jit.py -- chain plugin for: {name_of(shape)}
#define VF_CHAIN_PLUGIN 1
#include "vf_mlp_chain_gen.hpp"
#include "vf_chain_plugin.hpp"
namespace {{
struct Spec {{
    static constexpr int NB = {nb};
    static constexpr int KIN[2] = {{{pad(kin, 2)}}};
    static constexpr int DE[2] = {{{pad([len(e) for e in ew], 2)}}};
    static constexpr int EW[2][{MAX_DEPTH}] = {{{{{pad(ew[0])}}}, {{{pad(ew[1] if nb > 1 else ())}}}}};
    static constexpr int DP = {len(pw)}, DV = {len(vw)};
    static constexpr int PW[{MAX_DEPTH}] = {{{pad(pw)}}};
    static constexpr int VW[{MAX_DEPTH}] = {{{pad(vw)}}};
    static constexpr bool VF = true;
    static constexpr int HM = {_heads(shape)[0]}, HV = {_heads(shape)[1]};
    static constexpr int PASS = {1 if _heads(shape) == (1, 1) else 0};
    static constexpr int ACT = {_acts(shape)[0]}, EACT = {_acts(shape)[1]};       // VF_ACTIVATION_* of the trunks / the extractor MLPs
}};
struct SpecPi : Spec {{
    static constexpr bool VF = false;
}};
}}  // namespace
using Net = vf::ChainNetG<Spec>;
using NetPi = vf::ChainNetG<SpecPi>;
VF_CHAIN_PLUGIN_DEFINE(Net, NetPi, "{name_of(shape)}")
"""


def _sep_source(shape):
    """the translation unit of a network with separate pi / vf extractors: two single-trunk Specs -- A: pi-side extractor + pi trunk + the
    4-wide mean head, B: vf-side extractor + vf trunk + the 1-wide value head -- placed in the common layer table
    [pi extractor][vf extractor][pi trunk, mean][vf trunk, value] (csrc/vf_mlp_chain_sep.hpp)"""
    kin, ew, pw, vw = shape[:4]
    _, kin_v, ew_v, in_v, eact_v = _sep(shape)
    act, eact = _acts(shape)
    pad = lambda t, n=MAX_DEPTH: ", ".join(str(x) for x in (tuple(t) + (0,) * n)[:n])

    def spec(name, kin, ew, tw, eact):
        nb = len(kin)
        return f"""struct {name} {{
    static constexpr int NB = {nb};
    static constexpr int KIN[2] = {{{pad(kin, 2)}}};
    static constexpr int DE[2] = {{{pad([len(e) for e in ew], 2)}}};
    static constexpr int EW[2][{MAX_DEPTH}] = {{{{{pad(ew[0])}}}, {{{pad(ew[1] if nb > 1 else ())}}}}};
    static constexpr int DP = {len(tw)}, DV = {len(tw)};      // (one trunk: the second is never run)
    static constexpr int PW[{MAX_DEPTH}] = {{{pad(tw)}}};
    static constexpr int VW[{MAX_DEPTH}] = {{{pad(tw)}}};
    static constexpr bool VF = false;
    static constexpr int HM = 4, HV = 1;
    static constexpr int PASS = 0;
    static constexpr int ACT = {act}, EACT = {eact};
}};
"""
    n_a, n_b = sum(len(e) for e in ew), sum(len(e) for e in ew_v)
    n_all = n_a + n_b + len(pw) + 1 + len(vw) + 1
    in_a = tuple(range(len(kin)))
    idx = lambda t: ", ".join(str(x) for x in (tuple(t) + (-1, -1))[:2])
    copy_b = sum(1 << b for b, i in enumerate(in_v) if i not in in_a)       # an input both sides read is copied by role 0
    return f"""// generated by visfly_amd/_jit.py -- chain plugin for: {name_of(shape)}
#define VF_CHAIN_PLUGIN 1
#include "vf_mlp_chain_sep.hpp"
namespace {{
{spec("SpecA", kin, ew, pw, eact)}{spec("SpecB", kin_v, ew_v, vw, eact_v)}}}  // namespace
static_assert({n_all} <= VF_MLP_MAX_LAYERS, "layer table");
//                     Spec, role, first extractor layer, first trunk layer, layers, inputs of branch 0 / 1, copies
using NetA = vf::SepNet<SpecA, 0, 0, {n_a + n_b}, {n_all}, {idx(in_a)}, {(1 << len(kin)) - 1}>;
using NetB = vf::SepNet<SpecB, 1, {n_a}, {n_a + n_b + len(pw) + 1}, {n_all}, {idx(in_v)}, {copy_b}>;
VF_CHAIN_PLUGIN_SEP_DEFINE(NetA, NetB, "{name_of(shape)}")
"""


def rollout_source(shape, cfg):
    """the roll-out plugin of `shape` under cfg = (env kind, action type, integrator, ctrl_delay) -- VF_ENV_* / VF_ACT_* / VF_INT_* values:
    ONE instance of the persistent roll-out launch (csrc/vf_ppo_rollout_kernel.hpp)"""
    kind, act, integ, delay = cfg
    return source(shape) + f"""#include "vf_ppo_rollout_kernel.hpp"
VF_CHAIN_PLUGIN_ROLLOUT_DEFINE(Net, {int(kind)}, {int(act)}, {int(integ)}, {"true" if delay else "false"}, "{name_of(shape)} roll-out kind {int(kind)} act {int(act)} int {int(integ)} delay {int(bool(delay))}")
"""


def bptt_source(shape, cfg):
    """the BPTT plugin of `shape` (an actor class: the SAC-style Actor, or an actor-critic whose policy-only class the horizon steps) under
    cfg = (KERNEL-side env kind, action type, integrator, ctrl_delay): ONE instance each of the two persistent launches of a horizon
    (csrc/vf_bptt_rollout_kernel.hpp, csrc/vf_bptt_reverse_kernel.hpp), compiled as parts 5 / 6 (+ 7: the table)"""
    kind, act, integ, delay = cfg
    return source(shape) + f"""#if VF_CHAIN_PLUGIN_PART != 6
#include "vf_bptt_rollout_kernel.hpp"
#endif
#if VF_CHAIN_PLUGIN_PART != 5
#include "vf_bptt_reverse_kernel.hpp"
#endif
VF_CHAIN_PLUGIN_BPTT_DEFINE(Net, NetPi, {int(kind)}, {int(act)}, {int(integ)}, {"true" if delay else "false"}, "{name_of(shape)} BPTT horizon kind {int(kind)} act {int(act)} int {int(integ)} delay {int(bool(delay))}")
"""


def eval_source(shape, cfg):
    """the evaluation plugin of `shape` (heads (4, 1) or (4, 4)) under cfg = (KERNEL-side env kind, action type, integrator, ctrl_delay): ONE
    class's instances (16 / 32 rows per wave) of the evaluation launch (csrc/vf_eval_rollout_kernel.hpp), compiled as part 8"""
    kind, act, integ, delay = cfg
    return source(shape) + f"""#include "vf_eval_rollout_kernel.hpp"
VF_CHAIN_PLUGIN_EVAL_DEFINE(Net, {int(kind)}, {int(act)}, {int(integ)}, {"true" if delay else "false"}, "{name_of(shape)} evaluation kind {int(kind)} act {int(act)} int {int(integ)} delay {int(bool(delay))}")
"""


def _flags():
    extra = os.environ.get("VISFLY_AMD_JIT_FLAGS", "").split()       # e.g. -DVF_GEN_LIVE_TILES=0 (A/B builds; part of the cache key)
    return [f for f in HIPCC_FLAGS if f not in ("-shared", "-Wall")] + ["-ftemplate-depth=4096", "-Wno-unused-const-variable"] + extra + [
        "-I", INCLUDE, "-I", CSRC]


def _launch_ok(shape):
    """separate pi / vf extractors: no persistent launch -- the trainers step launch by launch"""
    return not is_builtin(shape) and not _sep(shape)


def _actor_ok(shape):
    return _launch_ok(shape) and _heads(shape) != (1, 1)


# one row per plugin kind: `tag` = what precedes the cfg in the `rollout` argument and in the keys of _loaded, `suffix` = what follows the
# shape in the slug, `parts` = the -DVF_CHAIN_PLUGIN_PART values compiled, `headers` = hashed into the cache key on top of _HEADERS,
# `source(shape, cfg)` = the translation unit, `serves(shape)` = can a generated class of this shape have such a plugin
_Kind = namedtuple("_Kind", "tag suffix parts headers source serves")
_KINDS = {
    "chain": _Kind((), "", (0, 1, 2, 3), (), lambda shape, cfg: source(shape), lambda shape: not is_builtin(shape)),
    "rollout": _Kind((), "_roll", (4,), _ROLLOUT_HEADERS, rollout_source, _launch_ok),
    "bptt": _Kind(("bptt",), "_bptt", (5, 6, 7), _BPTT_HEADERS, bptt_source, _actor_ok),
    "eval": _Kind(("eval",), "_eval", (8,), _EVAL_HEADERS, eval_source, _actor_ok),
}


def _kind_of(rollout):
    """the `rollout` argument of build / path_of -- None (the chain plugin), (kind, act, integ, delay) (PPO's roll-out plugin),
    ("bptt", kind, act, integ, delay) or ("eval", kind, act, integ, delay) -- as (row of _KINDS, cfg)"""
    if rollout is None:
        return _KINDS["chain"], ()
    if rollout[0] in ("bptt", "eval"):
        return _KINDS[rollout[0]], tuple(rollout[1:])
    return _KINDS["rollout"], tuple(rollout)


def _source_of(shape, rollout):
    k, cfg = _kind_of(rollout)
    return k.source(shape, cfg)


def _key(shape, rollout=None):
    h = hashlib.sha256()
    h.update(_source_of(shape, rollout).encode())
    h.update(" ".join(_flags()[:-4]).encode())
    for n in _HEADERS + (("vf_mlp_chain_sep.hpp",) if _sep(shape) else ()) + _kind_of(rollout)[0].headers + (os.path.join(INCLUDE, "visfly_amd.h"),):
        with open(n if os.path.isabs(n) else os.path.join(CSRC, n), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _slug(shape, rollout=None):
    kin, ew, pw, vw = shape[:4]
    t = lambda x: "".join(str(v) for v in x)
    s = "e" + "_".join(f"{k}x{t(e)}" for k, e in zip(kin, ew)) + f"_p{t(pw)}_v{t(vw)}" + {(4, 4): "_h44", (1, 1): "_h11", (4, 1): ""}[_heads(shape)]
    if _acts(shape) != (1, 1):
        s += "_a%d%d" % _acts(shape)
    sep = _sep(shape)
    if sep:
        s += "_sep" + "_".join(f"{k}i{i}x{t(e)}" for k, e, i in zip(sep[1], sep[2], sep[3])) + ("" if sep[4] == 1 else f"a{sep[4]}")
    k, cfg = _kind_of(rollout)
    return s + k.suffix + "".join(str(int(x)) for x in cfg)


def path_of(shape, rollout=None):
    """<cache>/libvf_chain_<shape>[_roll<cfg> | _bptt<cfg> | _eval<cfg>]_<hash of source + headers + flags>.so"""
    return os.path.join(JIT_DIR, f"libvf_chain_{_slug(shape, rollout)}_{_key(shape, rollout)}.so")


def build(shape, verbose=False, rollout=None):
    """compile the plugin of `shape` (rollout: which kind and configuration, see _kind_of; None = the chain plugin) unless the cache holds
    it -> path of the shared object"""
    out = path_of(shape, rollout)
    if os.path.exists(out):
        return out
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: the chain kernels of a non-default network shape are compiled on first use")
    os.makedirs(JIT_DIR, exist_ok=True)
    # one compiler run per shape and machine: the ranks of a job construct the same policy at the same time -- the first takes the
    # lock and compiles, the others wait on it and find the file
    import fcntl
    lock = open(os.path.join(JIT_DIR, f".{_slug(shape, rollout)}.lock"), "w")
    fcntl.flock(lock, fcntl.LOCK_EX)
    tmpdir = None
    try:
        if os.path.exists(out):
            return out
        tmpdir = tempfile.mkdtemp(prefix="visfly_amd_jit_")
        src = os.path.join(tmpdir, "plugin.hip")
        with open(src, "w") as f:
            f.write(_source_of(shape, rollout))

        def part(p):
            obj = os.path.join(tmpdir, f"part{p}.o")
            cmd = [hipcc] + _flags() + [f"-DVF_CHAIN_PLUGIN_PART={p}", "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed on the chain plugin for {name_of(shape)}:\n{r.stderr[-4000:]}")
            return obj

        with ThreadPoolExecutor(max_workers=4) as pool:
            objs = list(pool.map(part, _kind_of(rollout)[0].parts))
        tmp = f"{out}.{os.getpid()}.tmp"       # private name, then rename: concurrent builders (ranks) never see a torn file
        try:
            r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", tmp], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"linking the chain plugin for {name_of(shape)} failed:\n{r.stderr[-4000:]}")
            os.replace(tmp, out)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        for old in [] if os.environ.get("VISFLY_AMD_JIT_FLAGS") else os.listdir(JIT_DIR):          # builds of this shape against older headers
            stem = old[:-20] if len(old) > 20 else old          # libvf_chain_<slug>_<16 hex>.so
            if stem == f"libvf_chain_{_slug(shape, rollout)}" and old.endswith(".so") and old != os.path.basename(out):
                os.remove(os.path.join(JIT_DIR, old))
    finally:
        if tmpdir:
            shutil.rmtree(tmpdir, ignore_errors=True)
        fcntl.flock(lock, fcntl.LOCK_UN)
        lock.close()
    return out


def _ensure(kind, shape, cfg=()):
    """build (or find) and register the `kind` plugin of `shape` under cfg -> True when the library now holds it"""
    k = _KINDS[kind]
    if shape is None or os.environ.get("VISFLY_AMD_JIT", "1") == "0" or not k.serves(shape):
        return False
    rollout = k.tag + tuple(int(x) for x in cfg) or None
    key = shape if rollout is None else (shape, rollout)
    if key not in _loaded:
        from . import _lib
        _loaded[key] = None                  # (a failed build is not repeated by every policy / roll-out of this shape: the caller warns once and falls back)
        path = build(shape, rollout=rollout)
        _lib.check(_lib.lib().vf_chain_plugin_load(path.encode()))
        _loaded[key] = path
    return _loaded[key] is not None


def ensure(shape):
    """build (or find; ~40 s of hipcc) and register the plugin of `shape` -> True when the library now has chain kernels for it"""
    if shape is None or os.environ.get("VISFLY_AMD_JIT", "1") == "0":
        return False
    return is_builtin(shape) or _ensure("chain", shape)


def ensure_rollout(shape, cfg):
    """the same for the roll-out plugin of `shape` under cfg = (env kind, action type, integrator, ctrl_delay)"""
    return _ensure("rollout", shape, cfg)


def ensure_bptt(shape, cfg):
    """the same for the BPTT plugin (the two persistent launches of a horizon) of an actor class `shape` under cfg = (KERNEL-side env kind,
    action type, integrator, ctrl_delay); ~2 min of hipcc on first use"""
    return _ensure("bptt", shape, cfg)


def ensure_eval(shape, cfg):
    """the same for the evaluation plugin (the deterministic-episode launch of visfly_amd.evaluate) of a class with a 4-wide mean head under
    cfg = (KERNEL-side env kind, action type, integrator, ctrl_delay)"""
    return _ensure("eval", shape, cfg)


def prebuild_shape(name):
    """the shape a PREBUILD* table names: an entry of PREBUILD / PREBUILD_SAC / PREBUILD_CRITIC, or of PREBUILD_ACT (with its activations);
    or an entry of PREBUILD_SEP"""
    if name in PREBUILD_SEP:
        v = PREBUILD_SEP[name]
        return shape_of(*v[:4], acts=v[5][:2], vf_extractor=v[4], vf_extractor_act=v[5][2])
    if name in PREBUILD_ACT:
        v = PREBUILD_ACT[name]
        return shape_of(*v[:5], acts=v[5])
    return shape_of(*{**PREBUILD, **PREBUILD_SAC, **PREBUILD_CRITIC}[name])


def prebuild(verbose=False):
    """compile the PREBUILD shapes (in parallel) -> paths"""
    chains = list(PREBUILD) + list(PREBUILD_SAC) + list(PREBUILD_CRITIC) + list(PREBUILD_ACT) + list(PREBUILD_SEP)
    jobs = ([(prebuild_shape(n), None) for n in chains] + [(prebuild_shape(n), cfg) for n, cfg in PREBUILD_ROLLOUT] +
            [(prebuild_shape(n), ("bptt",) + cfg) for n, cfg in PREBUILD_BPTT] +
            [(prebuild_shape(n), ("eval",) + cfg) for n, cfg in PREBUILD_EVAL])
    # every chain job runs four hipcc parts of fully unrolled kernels: bound the number in flight by the cores of the build box
    with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), (os.cpu_count() or 4) // 4))) as pool:
        paths = list(pool.map(lambda j: build(j[0], verbose, rollout=j[1]), jobs))
    return paths
