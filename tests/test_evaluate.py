"""Deterministic evaluation episodes, the part that needs no GPU: the reference trainers' three deques (utils/algorithms/BPTT.py:85-91,
148-162) restated literally against ``visfly_amd.evaluate.EpisodeWindow``, the C ABI's new entries, the evaluation plugin of generated
classes (source, cache key per env configuration, cross-compilation for gfx950, the bumped class-table stamp) and the argument errors
(tests/test_evaluate_gpu.py runs the evaluations)."""
import os
import subprocess
from collections import deque
from types import SimpleNamespace

import numpy as np
import pytest
import torch


# ---- the reference's rule, restated: one evaluation from a (T, N) sticky done matrix and per-step info values -------------------
def reference_feed(deques, done, ret, length, success):
    """BPTT.py:139-156: `for index in reversed(eval_info_id_list): if done[index]: remove, append r / l / is_success`, step by step,
    until done.all().  ret / length / success: (T, N) -- what info[i] holds at step t (it keeps changing after the first done)"""
    rew, ln, suc = deques
    ids = list(range(done.shape[1]))
    for t in range(done.shape[0]):
        for index in reversed(list(ids)):
            if done[t, index]:
                ids.remove(index)
                rew.append(float(ret[t, index]))
                ln.append(int(length[t, index]))
                suc.append(bool(success[t, index]))
        if done[t].all():
            break
    assert not ids


def reference_deques():
    rew, ln, suc = deque(maxlen=100), deque(maxlen=100), deque(maxlen=100)
    for _ in range(100):
        suc.append(False)
    return rew, ln, suc


def reference_means(deques):
    rew, ln, suc = deques
    return {"rollout/ep_rew_mean": sum(rew) / len(rew), "rollout/ep_len_mean": sum(ln) / len(ln), "rollout/success_rate": sum(suc) / len(suc)}


def synthetic(N, T, seed):
    """sticky done with several agents per step, everyone done at T - 1; the info values keep changing after the first done"""
    rng = np.random.default_rng(seed)
    first = rng.integers(0, T, N)
    first[:3] = (0, T - 1, T - 1)
    first[3:6] = first[6 % N]                          # several agents finish in one step
    done = np.arange(T)[:, None] >= first[None, :]
    ret = rng.standard_normal((T, N)).astype(np.float32)
    length = np.broadcast_to(np.arange(1, T + 1)[:, None], (T, N)).copy()
    success = rng.random((T, N)) < 0.4
    return done, ret, length, success, first


def result_of(done, ret, length, success, first):
    """the EvalResult an evaluation of that run leaves: every agent's values at its first done step (CPU tensors)"""
    from visfly_amd.evaluate import EvalResult
    idx = np.arange(done.shape[1])
    flags = torch.from_numpy(success[first, idx].astype(np.uint8))         # VF_EP_SUCCESS = 1
    return EvalResult(torch.from_numpy(ret[first, idx].copy()), torch.from_numpy(length[first, idx].astype(np.int32)), flags)


@pytest.mark.parametrize("N", [7, 130, 250])
def test_c1_c2_episode_window_is_the_reference_deques(N):
    from visfly_amd.evaluate import EpisodeWindow
    ref, win, stepwise = reference_deques(), EpisodeWindow(), EpisodeWindow()
    assert list(win.successes) == [False] * 100 and len(win.rewards) == 0
    for k, seed in enumerate((11, 12)):                # two evaluations in a row feed the same window
        run = synthetic(N, 9, seed + N)
        reference_feed(ref, *run[:4])
        res = result_of(*run)
        assert res.is_success.dtype == torch.bool and res.path == "loop"
        win.extend(res)
        # C2: the same window fed episode by episode in the reference's order
        done, ret, length, success, first = run
        for t in range(done.shape[0]):
            for i in reversed(range(N)):
                if first[i] == t:
                    stepwise.add(ret[t, i], length[t, i], success[t, i])
        for w in (win, stepwise):
            assert list(w.rewards) == list(ref[0]) and list(w.lengths) == list(ref[1]) and list(w.successes) == list(ref[2])
            assert w.means() == reference_means(ref)
        if (k + 1) * N < 100:                          # fewer than 100 episodes: the pre-filled Falses count in the rate
            assert list(ref[2])[:100 - (k + 1) * N] == [False] * (100 - (k + 1) * N)
            assert win.means()["rollout/success_rate"] == sum(ref[2]) / 100
        assert len(win.rewards) == min((k + 1) * N, 100)
    # the lazily computed means of one evaluation: TestBase.test's two numbers
    assert res.mean_r == pytest.approx(float(np.mean(res.ep_return.numpy().astype(np.float64))), rel=1e-12)
    assert res.mean_l == float(res.ep_length.double().mean()) and res.success_rate == float(res.is_success.double().mean())


def test_c3_signatures():
    from visfly_amd import _lib
    for name in ("vf_eval_rollout", "vf_eval_latch", "vf_eval_action"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vf_eval_latch"][1]) == 13 and _lib.ABI_VERSION == 11
    header = open(os.path.join(os.path.dirname(_lib.LIB), "..", "..", "include", "visfly_amd.h")).read()
    fields = [n for n, _ in _lib.EvalRolloutArgs._fields_]
    body = header[header.index("typedef struct vf_eval_rollout_args {"):header.index("} vf_eval_rollout_args;")]
    import re
    at = [re.search(r"\b%s[;,]" % f, body).start() for f in fields]
    assert at == sorted(at)         # the mirror keeps the header's order


def test_c4_eval_plugin_source_key_and_build(tmp_path):
    """the evaluation plugin: source for a (4, 1) and a (4, 4) shape, one cache file per env configuration, cross-compiles for gfx950 and
    registers (cached: __graft_entry__.build() made the PREBUILD_EVAL entries); a plugin stamped with the previous class-table constant
    is refused"""
    from visfly_amd import _jit, _lib
    lib = _lib.lib()
    names = dict(_jit.PREBUILD_EVAL)
    assert {"tanh_nav", "gate_pi", "sac_hover_tanh"} <= set(names)
    pi, sac = _jit.prebuild_shape("gate_pi"), _jit.prebuild_shape("sac_hover_tanh")
    assert _jit._heads(pi) == (4, 1) and _jit._heads(sac) == (4, 4)
    for sh, cfg in ((pi, names["gate_pi"]), (sac, names["sac_hover_tanh"])):
        src = _jit.eval_source(sh, cfg)
        k, a, i, d = cfg
        assert f"VF_CHAIN_PLUGIN_EVAL_DEFINE(Net, {k}, {a}, {i}, {'true' if d else 'false'}," in src and '#include "vf_eval_rollout_kernel.hpp"' in src
        key = ("eval",) + cfg
        other = ("eval", cfg[0], 1 - cfg[1], cfg[2], cfg[3])
        assert len({_jit.path_of(sh), _jit.path_of(sh, key), _jit.path_of(sh, other), _jit.path_of(sh, cfg), _jit.path_of(sh, ("bptt",) + cfg)}) == 5
        assert "_eval" + "".join(str(int(x)) for x in cfg) + "_" in _jit.path_of(sh, key)
        path = _jit.build(sh, rollout=key)
        assert os.path.exists(path) and os.path.dirname(path) == _jit.JIT_DIR
        _lib.check(lib.vf_chain_plugin_load(path.encode()))
    loaded = [lib.vf_chain_plugin_name(i) for i in range(lib.vf_chain_plugin_count())]
    assert any(n.startswith(_jit.name_of(pi).encode()) and b"evaluation kind 3 act 1 int 0 delay 1" in n for n in loaded)
    assert any(n.startswith(_jit.name_of(sac).encode()) and b"evaluation kind 0 act 1 int 0 delay 1" in n for n in loaded)
    # not for a critic's shape, not for a built-in one
    assert _jit.ensure_eval(_jit.shape_of(*_jit.PREBUILD_CRITIC["critic_hover"]), (0, 1, 0, True)) is False
    assert _jit.ensure_eval(_jit.shape_of({"state": 13}, {"state": [128, 64]}, [64, 64], [64, 64]), (0, 1, 0, True)) is False
    # a plugin built before ChainPlugin grew its evaluation members carries the previous constant in its stamp (same struct sizes): refused
    assert lib.vf_chain_plugin_load(_lib.LIB.encode()) != 0
    msg = lib.vf_last_error().decode()
    expected = int(msg[msg.index("expected ") + 9:].split(")")[0], 16)
    old = expected ^ 0x56460006 ^ 0x56460005
    src = tmp_path / "old_plugin.c"
    src.write_text("struct plugin { unsigned abi; const char* name; void* members[4]; unsigned rollout_abi; void* ppo_rollout; };\n"
                   f"static int forward(void) {{ return 0; }}\n"
                   f"static const struct plugin p = {{0x{old:08x}u, \"old\", {{(void*)forward, (void*)forward, (void*)forward, 0}}, 0u, 0}};\n"
                   "const struct plugin* vf_chain_plugin(void) { return &p; }\n")
    so = tmp_path / "libold_plugin.so"
    subprocess.check_call(["cc", "-shared", "-fPIC", str(src), "-o", str(so)])
    n = lib.vf_chain_plugin_count()
    assert lib.vf_chain_plugin_load(str(so).encode()) != 0
    msg = lib.vf_last_error().decode()
    assert "not a chain plugin of this library build" in msg and f"abi {old:08x}" in msg and lib.vf_chain_plugin_count() == n


def test_c5_argument_errors():
    from visfly_amd import _lib
    from visfly_amd.evaluate import evaluate_policy
    env = SimpleNamespace()
    with pytest.raises(ValueError, match="different object"):
        evaluate_policy(SimpleNamespace(env=env, policy=None, obs_keys=["state"]), env)
    # learn(eval_env=...) needs a trainer, a trainer an env, and an env a device: without one it fails as every constructor does
    from visfly_amd.bptt import BPTT
    from visfly_amd.envs import HoverEnv

    def learn_with_eval_env():
        mk = lambda: HoverEnv(num_agent_per_scene=4, device="cpu", tensor_output=True, max_episode_steps=8)
        BPTT(mk(), horizon=2).learn(8, eval_env=mk())
    with pytest.raises(_lib.VisflyError):
        learn_with_eval_env()
    import inspect
    from visfly_amd.ppo import PPO
    from visfly_amd.shac import SHAC
    for cls in (BPTT, SHAC, PPO):
        assert inspect.signature(cls.learn).parameters["eval_env"].default is None
    assert inspect.signature(PPO.learn).parameters["eval_freq"].default is None
    assert inspect.signature(BPTT.__init__).parameters["dump_step"].default == 1e4 == inspect.signature(SHAC.__init__).parameters["dump_step"].default
