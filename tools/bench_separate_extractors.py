"""Optimiser-step time of PPO with separate pi / vf feature extractors (MlpPolicy ``vf_extractor``) at the PPO leg's shape: NavigationEnv,
32 768 agents, minibatches of 25 600 rows, [128, 64] per extractor branch and [64, 64] trunks on both sides, ReLU.

    python tools/bench_separate_extractors.py [--out profiles/separate_extractors.txt] [--steps 40] [--repeats 7]

One optimiser step = PPO._minibatch_update on a fixed minibatch of a collected roll-out: fused forward + loss + reverse chain (or forward,
vf_ppo_loss, backward), weight gradients, grad-norm clip + Adam with the packed weight refresh.  Three variants, same process, same card:
  (a) the separate network on its chain plugin (k_ppo_update_sep: two waves per 32 rows, one per side);
  (b) the same network with the plugins switched off (vf_chain_plugin_set_enabled(0)): the block-tile kernels;
  (c) the network of the same sizes with ONE shared extractor on the built-in class (k_ppo_update_split).
HIP events around `--steps` back-to-back steps after a warm-up; the variants' repetitions are interleaved (a, b, c, a, b, c, ...), the
median of `--repeats` and the spread (max - min) / median are reported.  (a) against (b) is the gain of the kernels, (a) against (c) the
price of the second extractor."""
import argparse
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfly_amd import _lib      # noqa: E402

DEV = "cuda:0"
EXT = dict(net_arch=dict(state=dict(layer=[128, 64]), target=dict(layer=[128, 64])), activation_fn="relu")


def trainer(sep, agents, batch):
    import bench
    from visfly_amd.envs import NavigationEnv
    from visfly_amd.ppo import PPO
    spawn = {"state_generator": {"class": "Uniform", "kwargs": [{"position": {"mean": [1., 0., 1.5], "half": [0., 2., 1.]}}]}}
    env = NavigationEnv(num_agent_per_scene=agents, seed=42, dynamics_kwargs=dict(bench.DYN_KW), random_kwargs=spawn, device=DEV, max_episode_steps=256)
    pk = dict(features_extractor_class="StateTargetExtractor", features_extractor_kwargs=EXT, net_arch=dict(pi=[64, 64], vf=[64, 64]),
              activation_fn="relu", share_features_extractor=not sep)
    ppo = PPO(env, n_steps=4, batch_size=batch, n_epochs=1, learning_rate=1e-6, seed=0, policy_kwargs=pk)
    ppo.collect_rollouts()
    buf = ppo.buf
    flat = {"actions": buf.actions.view(-1, 4), "old_lp": buf.log_probs.view(-1), "adv": buf.advantages.view(-1), "ret": buf.returns.view(-1)}
    flat.update({"obs:" + k: buf.obs[k].view(-1, buf.obs[k].shape[-1]) for k in ppo.obs_keys})
    perm = torch.randperm(4 * agents, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    shuf = ppo._prepare_epoch(flat, perm, batch)
    mb = {k: v[:batch] for k, v in shuf.items()}
    return ppo, mb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--agents", type=int, default=32768)
    ap.add_argument("--batch", type=int, default=25600)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_separate_extractors.py measures on the GPU; there is no fallback"
    lib = _lib.lib()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        variants = [("(a) separate, chain plugin (k_ppo_update_sep)", trainer(True, a.agents, a.batch), True),
                    ("(b) separate, plugins off (block-tile kernels)", trainer(True, a.agents, a.batch), False),
                    ("(c) shared extractor, built-in class (k_ppo_update_split)", trainer(False, a.agents, a.batch), True)]
        assert variants[0][1][0].policy.chain_jit and variants[0][1][0].policy.sep and not variants[2][1][0].policy.sep
        served = {}

        def window(name, ppo, mb, plugins, n):
            lib.vf_chain_plugin_set_enabled(1 if plugins else 0)
            n0 = lib.vf_chain_plugin_launches()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                ppo._minibatch_update(mb)
            e1.record()
            e1.synchronize()
            lib.vf_chain_plugin_set_enabled(1)
            served[name] = (lib.vf_chain_plugin_launches() - n0) / n
            return e0.elapsed_time(e1) * 1e3 / n

        us = {name: [] for name, _, _ in variants}
        for name, (ppo, mb), plugins in variants:        # warm-up: every shape the timed windows use
            window(name, ppo, mb, plugins, 10)
        for _ in range(a.repeats):
            for name, (ppo, mb), plugins in variants:
                us[name].append(window(name, ppo, mb, plugins, a.steps))
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; fp32; {a.agents} agents, minibatch {a.batch} rows; one optimiser step = "
             f"PPO._minibatch_update; HIP events around {a.steps} steps, median of {a.repeats} interleaved repetitions, spread = (max - min) / median",
             f"{'variant':>58} {'us / step':>10} {'spread':>7} {'plugin launches / step':>23} {'parameters':>11}"]
    med = {}
    for name, (ppo, _), _ in variants:
        med[name] = statistics.median(us[name])
        lines.append(f"{name:>58} {med[name]:>10.1f} {(max(us[name]) - min(us[name])) / med[name]:>6.1%} {served[name]:>23.1f} {ppo.policy.n_params:>11d}")
    n = [v[0] for v in variants]
    lines.append(f"(b) / (a) = {med[n[1]] / med[n[0]]:.2f}   (a) / (c) = {med[n[0]] / med[n[2]]:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
