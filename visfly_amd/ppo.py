"""On-device PPO for the state-vector drone envs.

Restates the reference's PPO path (utils/algorithms/PPO.py:116-337 on top of SB3 2.2.1
``OnPolicyAlgorithm.collect_rollouts`` / ``RolloutBuffer``; the policy is ``MlpPolicy`` of visfly_amd/policy.py) with every
arithmetic piece running as a HIP
kernel behind the C-ABI: policy/value MLP forward + backward on the fp32 MFMA, squashed-Gaussian
head sampling, GAE scan, advantage normalisation, clipped-surrogate loss, grad-norm clip + Adam.
The rollout buffer lives on the device ([T][N] SoA); nothing crosses PCIe inside ``learn``.

Multi-GPU: one process per GPU, agents sharded by rank; the only exchange is ONE all-reduce of the
flat fp32 gradient buffer per optimiser step (plus the two fp64 advantage sums so that the
normalisation is over the global minibatch) through ``torch.distributed`` (RCCL on ROCm).
"""
import ctypes as C
import os
import time
from typing import Dict, Optional

import numpy as np
import torch as th

from . import _lib, checkpoint, parallel
from .checkpoint import trainer_obs_keys
# the policy and its helpers live in policy.py; the names stay importable from here
from .policy import (ACTIVATIONS, FUSED_MAX_WIDTH, INDEX_OBS_KEYS, LN_EPS, MAX_WIDTH, POLICY_OBS_KEYS, WGRAD_SPLIT_ROWS,  # noqa: F401
                     _TORCH_ACT, MlpPolicy, _Linear, _ptr, activation_kind, obs_width, policy_rows)


class RolloutBuffer:
    """[T][N] device-resident rollout storage (SB3 RolloutBuffer semantics; mirror at
    utils/algorithms/common.py:46-215)"""

    def __init__(self, T, N, obs_dims: Dict[str, int], device):
        f = dict(dtype=th.float32, device=device)
        self.T, self.N = T, N
        self.obs = {k: th.zeros((T, N, d), **f) for k, d in obs_dims.items()}
        self.actions = th.zeros((T, N, 4), **f)
        self.rewards, self.values, self.log_probs = th.zeros((T, N), **f), th.zeros((T, N), **f), th.zeros((T, N), **f)
        self.episode_starts = th.zeros((T, N), **f)
        self.advantages, self.returns = th.zeros((T, N), **f), th.zeros((T, N), **f)


class PPO:
    """PPO.learn / collect_rollouts / train of the reference (utils/algorithms/PPO.py:116-337)."""

    def __init__(self, env, n_steps=256, batch_size=25600, n_epochs=5, gamma=0.99, gae_lambda=0.95, clip_range=0.2,
                 ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, learning_rate=1e-4, weight_decay=1e-5,
                 normalize_advantage=True, policy_kwargs: Optional[dict] = None, seed=0, adam_eps=1e-8,
                 betas=(0.9, 0.999), target_kl=None, policy=None, verbose=0, device=None, clip_range_vf=None):
        # `policy`, `verbose`, `device`: accepted so that the `algorithm:` block of the reference's YAMLs can be passed
        # as **kwargs (exps/examples/alg_cfgs/*/PPO.yaml); the policy is always the MFMA MlpPolicy on the env's device
        if policy not in (None, "CustomMultiInputPolicy", "MultiInputPolicy", "MlpPolicy"):
            raise NotImplementedError(f"policy {policy}: vector-observation actor-critic policies only")
        self.env = env
        env.tensor_output, env.requires_grad = True, False        # PPO.py:80-82 forces the non-grad path
        self.device = env.device
        self.n_envs = env.num_envs
        self.n_steps, self.batch_size, self.n_epochs = n_steps, batch_size, n_epochs
        # learning_rate / clip_range / clip_range_vf: a float or, as SB3's get_schedule_fn accepts them, a callable of
        # progress_remaining (1 at the start of learn(), 0 at its end; PPO.py:150-152,184-189) evaluated once per train() call
        self.gamma, self.gae_lambda, self.clip_range = gamma, gae_lambda, clip_range
        self.ent_coef, self.vf_coef, self.max_grad_norm = ent_coef, vf_coef, max_grad_norm
        self.lr_schedule, self.weight_decay, self.adam_eps, self.betas = learning_rate, weight_decay, adam_eps, betas
        self.normalize_advantage, self.target_kl, self.seed = normalize_advantage, target_kl, seed
        self.clip_range_vf = clip_range_vf                          # PPO.py:237-243; None = no value clipping
        self._current_progress_remaining = 1.0
        # TimeLimit bootstrap valued once per rollout (collect_rollouts) from the terminal rows the step kernel wrote; envs that
        # assemble their observation on the host (RacingEnv2: 16 gate-relative columns) have no such kernel rows -> valued per step
        self.defer_bootstrap, self._boot = (not getattr(env, "_HOST_OBS", False)) or getattr(env, "_OBS_W", 13) != 13, None
        if hasattr(env, "obs_gate_exact"):       # RacingEnv / RacingEnv2: the "state" rows use the agent's current gate (what the persistent
            env.obs_gate_exact = False           # roll-out forms), as under BPTT / SHAC; a policy that reads "gate" (StateGateExtractor) is
                                                 # fed that same index -- the one its "state" rows were formed with
        self.fused_rollout = True           # collect_rollouts as one persistent launch where the library has the kernel (vf_ppo_rollout)
        self._last_obs = None
        if not getattr(env, "_is_initial", False):
            self._last_obs = env.reset()
        obs = env.get_observation()
        self.obs_keys = trainer_obs_keys(obs, policy_kwargs)
        # the one key besides "state" (constant "target" rows, or the "gate" index column): what the bootstrap list's rows1 hold
        self._key1 = next((k for k in self.obs_keys if k != "state"), None)
        assert self._key1 in (None, "target", "gate")
        obs_dims = {k: obs_width(obs[k]) for k in self.obs_keys}
        pk = checkpoint.policy_kwargs_from_reference(policy_kwargs, self.obs_keys)
        self.weight_decay = pk.get("weight_decay", self.weight_decay)   # optimizer_kwargs.weight_decay of the YAMLs
        extractor = pk.get("extractor", {k: [128, 64] for k in self.obs_keys})
        self.policy = MlpPolicy(obs_dims, extractor, pk.get("pi", [64, 64]), pk.get("vf", [64, 64]), self.device,
                                log_std_init=pk.get("log_std_init", 0.0), seed=seed, ortho_init=pk.get("ortho_init", True),
                                activation=pk.get("activation", "relu"), extractor_activation=pk.get("extractor_activation", "relu"),
                                layer_norm=pk.get("layer_norm"), vf_extractor=pk.get("vf_extractor"),
                                vf_extractor_activation=pk.get("vf_extractor_activation"))
        if self.policy.ln:
            self.policy._warn_fallback("PPO")
        self.policy.lazy_pack = True        # this trainer calls mark_updated() after every optimiser step
        self.world, self.rank = parallel.world_size(), parallel.rank()
        # every rank must start from the SAME parameters (only gradients are exchanged afterwards) and draw DIFFERENT
        # exploration noise for its agents: rank 0's initial weights go to everybody, the rank goes into the Philox key
        parallel.broadcast_(self.policy.flat)
        self.policy.mark_updated()
        self._noise_key = (int(seed) ^ (self.rank << 32)) & (2 ** 64 - 1)
        # ... unless the env is globally keyed (envs/base.py: agent_offset): then the counter row of agent i is agent_offset + i on
        # every rank and the key is the seed alone -- the shards' noise is the matching rows of ONE stream over the whole population
        self._row0 = getattr(env, "agent_offset", None)
        if self._row0 is not None:
            self._noise_key = int(seed) & (2 ** 64 - 1)
        self._row0 = self._row0 or 0
        self.buf = RolloutBuffer(n_steps, self.n_envs, obs_dims, self.device)
        n = self.policy.n_params
        dev = self.device
        self.exp_avg, self.exp_avg_sq = th.zeros(n, device=dev), th.zeros(n, device=dev)
        # loss-statistic partial rows of a minibatch (16 floats per 32-row tile; vf_ppo_loss / vf_ppo_update) + 4096 floats of reduction scratch
        self._scratch = th.zeros(16 * max(1024, (min(batch_size, n_steps * self.n_envs) + 31) // 32) + 4096, device=dev)
        # flat gradient and the 16 loss statistics in ONE buffer: an optimiser step on several GPUs is exactly one all-reduce
        self._gbuf = th.zeros(n + 16, device=dev)
        self.policy.grad = self._gbuf[:n]
        self._stats = self._gbuf[n:]
        self._ep_stats = th.zeros(4, dtype=th.float64, device=dev)   # episodes, sum return, sum length, successes
        self._sumsq = th.zeros(1, device=dev)
        self._sums = th.zeros(2, dtype=th.float64, device=dev)
        self._opt_step = 0
        self._n_updates = 0            # SB3's counter: epochs (PPO.py:294), what train/n_updates logs
        self._sample_step = 0
        self.num_timesteps = 0
        self._last_starts = th.ones(self.n_envs, device=dev)
        self._shuf = None
        # gradient exchange of a multi-GPU step.  1 (default): ONE all-reduce of [gradient | 16 loss statistics] between the fold and
        # Adam.  2 (VISFLY_AMD_GRAD_BUCKETS=2): the weight gradients are formed in two launch pairs -- trunks + heads, then the extractor
        # MLPs -- and the first bucket ([trunks | log_std | statistics]) is all-reduced on a second stream UNDER the second pair; the
        # second bucket follows on that stream, Adam waits for both.  Same sums, same bits (tests/test_parallel_*); whether it pays is a
        # question for real xGMI links: 176 KB is latency, not bandwidth (bench.py prints both modes for N > 1)
        self.grad_buckets = int(os.environ.get("VISFLY_AMD_GRAD_BUCKETS", "1"))
        self._xstream, self._xev = None, None
        self.index_minibatches = False     # True: train() reads its minibatches through the permutation slice (vf_ppo_loss_cfg.row_index) instead of a shuffled copy -- measured 2 % slower, see train()
        self.logs: Dict[str, float] = {}

    def _stream(self):
        return _lib.current_stream(self.device)

    def _now(self, v):
        """a schedule's value at the current progress_remaining (floats are constant schedules)"""
        return None if v is None else float(v(self._current_progress_remaining) if callable(v) else v)

    @property
    def lr(self):
        return self._now(self.lr_schedule)

    @lr.setter
    def lr(self, v):
        self.lr_schedule = v

    def _terminal_gate_rows(self):
        """(N, 1) float32: the gate index each agent's terminal "state" row was formed with (valid where the agent just ended an episode);
        None for a policy without the gate branch"""
        return self.env._terminal_gate.view(self.n_envs, 1).to(th.float32) if self._key1 == "gate" else None

    def _bootstrap_list(self):
        """compact list of the rollout's truncated rows (vf_rollout_post_collect): an agent is truncated at most once per
        max_episode_steps steps, plus the episode it is in when the rollout starts"""
        if self._boot is None:
            N, dev = self.n_envs, self.device
            per_agent = self.n_steps // max(int(getattr(self.env, "max_episode_steps", self.n_steps)), 1) + 2
            cap = (N * per_agent + 8191) // 8192 * 8192
            w1 = self.policy.obs_dims[self._key1] if self._key1 else 0
            self._boot = {"cap": cap, "cursor": th.zeros(1, dtype=th.int32, device=dev), "idx": th.zeros(cap, dtype=th.int32, device=dev),
                          "rows0": th.zeros((cap, self.policy.obs_dims["state"]), device=dev),
                          "rows1": th.zeros((cap, w1), device=dev) if w1 else None,
                          "stat": th.zeros((N, 4), device=dev)}
        self._boot["cursor"].zero_()
        self._boot["stat"].zero_()
        return self._boot

    def save(self, path: str):
        """zip archive in the layout of SB3's BaseAlgorithm.save (PPO.py:418-430): see checkpoint.py"""
        return checkpoint.save(self, path)

    def set_parameters(self, path: str, load_optimizer: bool = True):
        return checkpoint.load_into(self, path, load_optimizer)

    @classmethod
    def load(cls, path: str, env, **kwargs):
        """PPO.py:432-572: re-create the trainer on `env`, then load policy (and optimiser) state; also reads
        archives written by the reference (policy.pth with the reference's parameter names)"""
        return checkpoint.load_into(cls(env, **checkpoint.ctor_kwargs_from_archive(path, kwargs)), path)

    # ------------------------------------------------------------------------------------------
    def _act(self, obs, deterministic=False):
        """policy.forward (policies.py:195-226): action, value, log_prob"""
        mean, value = self.policy.forward(policy_rows(obs, self.obs_keys), save_activations=False)
        M = mean.shape[0]
        action = th.empty((M, 4), device=self.device)
        logp = th.empty(M, device=self.device)
        self._sample_step += 1
        _lib.check(_lib.lib().vf_head_sample_at(_ptr(mean), _ptr(self.policy.log_std), _ptr(action), _ptr(logp), M, self._row0,
                                                self._noise_key, self._sample_step, 1 if deterministic else 0,
                                                self._stream()))
        return action, value.view(M), logp

    def predict_values(self, obs):
        _, value = self.policy.forward(policy_rows(obs, self.obs_keys), save_activations=False)
        return value.view(-1).clone()

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = False):
        """SB3 ``BaseAlgorithm.predict`` as the evaluation harness calls it (utils/evaluate.py:94): -> (action, None);
        deterministic: a = tanh(mean)"""
        return self._act(obs, deterministic)[0], None

    def collect_rollouts(self, replay=None):
        """SB3 OnPolicyAlgorithm.collect_rollouts: n_steps of policy -> env.step -> buffer, with the
        TimeLimit bootstrap reward += gamma * V(terminal_obs) for truncated episodes, then GAE.
        `replay`: dict(eps=(T,N,4), actions=(T,N,4)) of a recorded roll-out -- the head takes its noise from eps[t] instead of Philox
        (vf_head_sample_eps: the same device function as vf_head_sample_at's) and keeps its own sample and log-prob in the buffer rows,
        while the env is stepped with the recorded actions[t] -- how tests replay a recorded run of the reference's collect_rollouts
        with the env held on the recorded trajectory (tests/test_ppo_loop_gpu.py).  Launch by launch: the persistent launch draws its
        own noise."""
        env, buf = self.env, self.buf
        if replay is not None:
            as_dev = lambda a: th.as_tensor(a, dtype=th.float32).to(self.device).contiguous()
            r_eps, r_act = as_dev(replay["eps"]), as_dev(replay["actions"])
            if r_eps.shape != buf.actions.shape or r_act.shape != buf.actions.shape:
                raise ValueError(f"collect_rollouts(replay=...): eps and actions must be {tuple(buf.actions.shape)}")
        if self._last_obs is None:
            self._last_obs = env.reset()
            self._last_starts = th.ones(self.n_envs, device=self.device)
        obs = self._last_obs
        L, pol, N = _lib.lib(), self.policy, self.n_envs
        buf.episode_starts[0].copy_(self._last_starts)
        bs = self._bootstrap_list() if self.defer_bootstrap else None
        fused = False
        if replay is None and self.fused_rollout and self.defer_bootstrap and hasattr(env, "collect_policy"):
            # the whole loop below as one persistent launch (vf_ppo_rollout); same buffer rows, same Philox counters
            rows = policy_rows(obs, self.obs_keys)
            for k in self.obs_keys:
                if k == "target":
                    buf.obs[k].copy_(rows[k].unsqueeze(0).expand_as(buf.obs[k]))       # constant per env
                else:
                    buf.obs[k][0].copy_(rows[k])          # ("gate": the launch writes the rows of the later steps, like "state")
            fused = env.collect_policy(pol, self.obs_keys, buf, bs, self._noise_key, self._sample_step, self._last_starts)
            if fused is not False:
                obs = fused
                self._sample_step += self.n_steps
            else:
                self.fused_rollout = False
        for t in range(self.n_steps if fused is False else 0):
            # policy.forward (policies.py:195-226) straight into row t of the buffer: value head, sampled action, log-prob
            action, logp = buf.actions[t], buf.log_probs[t]
            rows = policy_rows(obs, self.obs_keys)
            mean, _ = pol.forward(rows, save_activations=False, out_value=buf.values[t])
            self._sample_step += 1
            if replay is None:
                _lib.check(L.vf_head_sample_at(_ptr(mean), _ptr(pol.log_std), _ptr(action), _ptr(logp), N, self._row0, self._noise_key,
                                               self._sample_step, 0, self._stream()))
            else:
                _lib.check(L.vf_head_sample_eps(_ptr(mean), _ptr(pol.log_std), _ptr(r_eps[t]), _ptr(action), _ptr(logp), N, self._stream()))
            for k in self.obs_keys:
                buf.obs[k][t].copy_(rows[k])
            obs, reward, done, _info = env.step(action if replay is None else r_act[t])
            if not self.defer_bootstrap:
                _lib.check(L.vf_episode_stats(done.data_ptr(), _ptr(env._ep_return), _ptr(env._ep_length), _ptr(env._ep_flags),
                                              self._ep_stats.data_ptr(), N, self._stream()))
            # TimeLimit.truncated bootstrap: SB3 adds gamma * V(terminal_observation) where the info says truncated.  Deferred:
            # the few truncated rows of this step are appended to a compact list, valued once after the loop
            nxt = buf.episode_starts[t + 1] if t + 1 < self.n_steps else self._last_starts
            trows = env._terminal_state_rows()               # (N, w) in the env's observation map, w = the policy's row width
            assert trows.shape[1] == pol.obs_dims["state"], (trows.shape, pol.obs_dims)
            if self.defer_bootstrap:
                # the second entry of a truncated agent's terminal observation: its constant "target" row, or the gate index its terminal
                # "state" row was formed with (terminal_gate)
                o1 = obs["target"] if self._key1 == "target" else self._terminal_gate_rows()
                _lib.check(L.vf_rollout_post_collect(_ptr(reward), done.data_ptr(), _ptr(env._ep_flags), _ptr(buf.rewards[t]), _ptr(nxt),
                                                     _ptr(trows), _ptr(o1), trows.shape[1], 0 if o1 is None else o1.shape[1],
                                                     bs["cursor"].data_ptr(), bs["cap"], bs["idx"].data_ptr(), _ptr(bs["rows0"]),
                                                     _ptr(bs["rows1"]), t * N, N, _ptr(env._ep_return), env._ep_length.data_ptr(),
                                                     _ptr(bs["stat"]), self._stream()))
            else:
                tobs = {"state": trows.contiguous()}
                if self._key1 == "target":
                    tobs["target"] = obs["target"]
                elif self._key1 == "gate":
                    tobs["gate"] = self._terminal_gate_rows()
                _, tv = pol.forward(tobs, save_activations=False)
                _lib.check(L.vf_rollout_post(_ptr(reward), done.data_ptr(), _ptr(env._ep_flags), _ptr(tv), float(self.gamma),
                                             _ptr(buf.rewards[t]), _ptr(nxt), N, self._stream()))
        if self.defer_bootstrap:
            self._ep_stats += bs["stat"].double().sum(dim=0)     # episode statistics of the rollout, per-agent sums folded once
            cnt = int(bs["cursor"].item())                       # one host sync per rollout
            if cnt > bs["cap"]:
                raise _lib.VisflyError(f"deferred bootstrap list overflow ({cnt} > {bs['cap']} truncated rows in one rollout)")
            CH = 8192                                            # fixed chunk: one set of forward buffers whatever the count
            for s0 in range(0, cnt, CH):
                m = min(CH, cnt - s0)
                rows = {"state": bs["rows0"][s0:s0 + CH]}
                if bs["rows1"] is not None:
                    rows[self._key1] = bs["rows1"][s0:s0 + CH]
                _, tv = pol.forward(rows, save_activations=False)
                _lib.check(L.vf_bootstrap_scatter(bs["idx"].data_ptr() + 4 * s0, _ptr(tv), m, float(self.gamma), _ptr(buf.rewards),
                                                  self._stream()))
        self._last_obs = obs
        last_values = self.predict_values(obs)
        _lib.check(_lib.lib().vf_gae(_ptr(buf.rewards), _ptr(buf.values), _ptr(buf.episode_starts), _ptr(last_values),
                                     _ptr(self._last_starts), _ptr(buf.advantages), _ptr(buf.returns), self.n_steps,
                                     self.n_envs, float(self.gamma), float(self.gae_lambda), self._stream()))
        self.num_timesteps += self.n_steps * self.n_envs * self.world

    # ------------------------------------------------------------------------------------------
    def _minibatch_update(self, mb, stats_acc=None):
        """one optimiser step on a minibatch {obs:*, actions, old_lp, adv, ret[, old_v]} of contiguous rows (PPO.py:203-292).
        Returns the loss statistics of the (global) minibatch, or None when target_kl stopped the update BEFORE the
        optimiser step (PPO.py:269-282)."""
        L, st, pol = _lib.lib(), self._stream(), self.policy
        rows = mb.get("rows")        # indexed minibatch: the fields are the whole rollout buffer, `rows` the minibatch's row indices
        obs = {k: mb["obs:" + k] for k in self.obs_keys}
        actions, old_lp, adv, ret = mb["actions"], mb["old_lp"], mb["adv"], mb["ret"]
        B = adv.numel()
        gB = B * self.world
        # the loss launch also writes d(loss)/d(log_std) into the tail of the flat gradient and adds the minibatch
        # statistics to the epoch accumulator (no separate copy / add launches)
        vclip = self.clip_range_vf is not None
        cfg = _lib.PpoLossCfg(self._now(self.clip_range), self.ent_coef, self.vf_coef, 1.0 / gB, _ptr(pol.grad, pol.log_std_off),
                              None if stats_acc is None else _ptr(stats_acc),
                              _ptr(mb["old_v"]) if vclip else None, self._now(self.clip_range_vf) if vclip else 0.0, 0)
        # reference-default policy shapes: forward + loss + reverse chain are one launch (vf_ppo_update)
        # single GPU: the weight-gradient fold also leaves the squared gradient norm as partial sums, which Adam adds up itself
        two = self.grad_buckets == 2 and (self.world > 1 or os.environ.get("VISFLY_AMD_GRAD_BUCKETS_FORCE") == "1")
        between = None
        if two:
            if self._xstream is None:
                self._xstream, self._xev = th.cuda.Stream(device=self.device), [th.cuda.Event() for _ in range(3)]
            split, xs, ev = pol.bucket_split(), self._xstream, self._xev

            def between():        # trunks' gradients, log_std's and the statistics are final: their all-reduce runs under the second launch pair
                ev[0].record()
                xs.wait_event(ev[0])
                parallel.allreduce_sum_(self._gbuf[split:], stream=xs)
        res = pol.ppo_update(obs, actions, old_lp, adv, ret, cfg, self._stats, self._scratch, want_sumsq=self.world == 1 and not two,
                             row_index=rows, between=between)
        if two and res is True:
            ev[1].record()
            xs.wait_event(ev[1])
            parallel.allreduce_sum_(self._gbuf[:split], stream=xs)
            ev[2].record(xs)
            th.cuda.current_stream(self.device).wait_event(ev[2])
        elif two:       # no fused step for this network: one bucket after the layer-by-layer backward (below)
            two = False
        sq = res if isinstance(res, tuple) else None
        if res is False and rows is not None:       # no fused step for this network: materialise the minibatch (what the gather did)
            obs = {k: v.index_select(0, rows) for k, v in obs.items()}
            actions, old_lp, ret = actions.index_select(0, rows), old_lp.index_select(0, rows), ret.index_select(0, rows)
            if vclip:
                old_v_sel = mb["old_v"].index_select(0, rows)       # bound to a name: it must outlive vf_ppo_loss (cfg holds its raw pointer)
                cfg.old_value = _ptr(old_v_sel)
            cfg.row_index, cfg.obs_copy0, cfg.obs_copy1 = None, None, None
        if res is False:
            mean, value = pol.forward(obs)
            d_mean, d_value = th.empty((B, 4), device=self.device), th.empty(B, device=self.device)
            _lib.check(L.vf_ppo_loss(_ptr(mean), _ptr(value), _ptr(pol.log_std), _ptr(actions), _ptr(old_lp), _ptr(adv), _ptr(ret),
                                     _ptr(d_mean), _ptr(d_value), _ptr(self._stats), B, C.byref(cfg), _ptr(self._scratch), st))
            pol.backward(d_mean, d_value, None)
        if self.world > 1 and not two:
            # ONE collective per optimiser step: the flat gradient and the 16 loss statistics are one buffer
            # (sum over ranks: every gradient term is already / global batch, the statistics are per-rank sums)
            parallel.allreduce_sum_(self._gbuf)
        if self.target_kl is not None:
            # PPO.py:269-282: approx_kl of THIS minibatch, checked before optimizer.step() (one host sync per minibatch,
            # only when target_kl is set; with several ranks the statistics came back with the gradient)
            kl = float(self._stats[3].item()) / gB
            if kl > 1.5 * self.target_kl:
                return None
        self._opt_step += 1
        # (with the fold's partials `sq` no separate grad-norm launch; Adam adds them and the log_std tail up itself)
        pol.adam_step(self.exp_avg, self.exp_avg_sq, self._sumsq, self._scratch, self.lr, self.betas, self.adam_eps, self.weight_decay,
                      self.max_grad_norm, self._opt_step, sumsq_partials=sq, sumsq_tail_from=pol.log_std_off)
        return self._stats

    def train(self, permutations=None):
        """PPO.train (PPO.py:177-337): n_epochs passes over random minibatches (SB3 RolloutBuffer.get: the trailing
        partial minibatch of an epoch is trained on too).  `permutations`: one row permutation per epoch (rows = step * n_envs + env)
        instead of the trainer's own draws -- how tests replay the minibatches of a recorded run of the reference's train()
        (tests/test_ppo_loop_gpu.py)"""
        total = self.n_steps * self.n_envs
        bs = min(self.batch_size, total)
        g = th.Generator(device=self.device)
        g.manual_seed(self.seed + 7919 * (self._opt_step + 1))
        # loss statistics: one row per evaluated minibatch.  The reference appends every minibatch's MEAN to a list and logs np.mean of
        # the lists -- equal weight per minibatch, whatever its row count (the trailing partial one counts like a full one); approx_kl's
        # list is reset per epoch (PPO.py:197), so its log is the mean over the minibatches of the LAST epoch started, including the one
        # that tripped target_kl (PPO.py:263-282: appended before the check)
        n_mb = (total + bs - 1) // bs
        stats_mb = th.zeros((self.n_epochs * n_mb, 16), device=self.device)
        rows_mb, epoch_mb = [], []
        stop = False
        buf = self.buf
        flat = {"actions": buf.actions.view(-1, 4), "old_lp": buf.log_probs.view(-1), "adv": buf.advantages.view(-1),
                "ret": buf.returns.view(-1)}
        if self.clip_range_vf is not None:
            flat["old_v"] = buf.values.view(-1)
        flat.update({"obs:" + k: buf.obs[k].view(-1, buf.obs[k].shape[-1]) for k in self.obs_keys})
        for _epoch in range(self.n_epochs):
            if permutations is not None:
                perm = th.as_tensor(permutations[_epoch], dtype=th.int64, device=self.device).contiguous()
                assert perm.numel() == total
            else:
                perm = th.randperm(total, device=self.device, generator=g)
            # (preparing epoch e + 1's copy on a side stream under epoch e's optimiser steps gains nothing: the gather takes the HBM
            # bandwidth the weight-gradient kernel runs on -- profiles/r05_side_streams.txt, tools/exp_ppo_prefetch.py)
            # r05 (ABI 9), `index_minibatches`: the fused step can read its minibatch through the permutation slice
            # (vf_ppo_loss_cfg.row_index), like SB3's RolloutBuffer.get indexes the buffer -- only the advantages are gathered then.
            # Bit-identical, and SLOWER: 145.3 vs 142.5 ms per train() of 1280 steps (tools/exp_ppo_indexed.py) -- the 1.14 ms-per-epoch
            # streaming gather (5.7 ms) is replaced by 25 600 random 100-byte rows behind a dependent index load at the head of every
            # fused launch, +6.6 us of a lone wave's latency each (8.5 ms).  Off by default; the shuffled copy stays
            pol = self.policy
            indexed = (self.index_minibatches and pol._fused_ppo is not False and pol._plan is not None and pol.fused and pol.fused_backward)
            shuf = self._prepare_epoch({"adv": flat["adv"]} if indexed else flat, perm, bs)
            for s in range(0, total, bs):
                e = min(s + bs, total)
                if indexed:
                    mb = dict(flat, adv=shuf["adv"][s:e], rows=perm[s:e])
                else:
                    mb = {k: v[s:e] for k, v in shuf.items()}
                st = self._minibatch_update(mb, stats_mb[len(rows_mb)])
                rows_mb.append(e - s)
                epoch_mb.append(_epoch)
                if st is None:
                    stop = True
                    break
            self._n_updates += 1        # PPO.py:294: once per epoch started, the early-stopped one included
            if stop:
                break
        if self.world > 1:
            parallel.allreduce_sum_(stats_mb)                        # log the global means, like a single-process run would
        n_eval = len(rows_mb)
        means = stats_mb[:max(n_eval, 1)].double().cpu().numpy() / (np.asarray(rows_mb or [1], np.float64)[:, None] * self.world)
        last = [i for i in range(n_eval) if epoch_mb[i] == epoch_mb[-1]] or [0]
        ep = parallel.allreduce_sum_(self._ep_stats.clone()).tolist()          # rollout statistics of this iteration (:398-414)
        self._ep_stats.zero_()
        if ep[0] > 0:
            self.logs.update({"rollout/ep_rew_mean": ep[1] / ep[0], "rollout/ep_len_mean": ep[2] / ep[0],
                              "rollout/ep_success_rate": ep[3] / ep[0], "rollout/episodes": ep[0]})
        # PPO.py:322-336
        ret, val = buf.returns.view(-1).double(), buf.values.view(-1).double()
        var_y = float(ret.var(unbiased=False))
        self.logs.update({"train/policy_gradient_loss": float(means[:, 0].mean()), "train/value_loss": float(means[:, 1].mean()),
                          "train/entropy_loss": float(means[:, 2].mean()), "train/approx_kl": float(means[last, 3].mean()),
                          "train/clip_fraction": float(means[:, 4].mean()),
                          "train/loss": float(means[-1, 0] + self.ent_coef * means[-1, 2] + self.vf_coef * means[-1, 1]),
                          "train/explained_variance": float("nan") if var_y == 0 else 1.0 - float((ret - val).var(unbiased=False)) / var_y,
                          "train/std": float(self.policy.log_std.exp().mean()),
                          "train/n_updates": self._n_updates, "train/optimiser_steps": self._opt_step, "train/learning_rate": self.lr,
                          "train/clip_range": self._now(self.clip_range), "train/early_stop": float(stop)})
        if self.clip_range_vf is not None:
            self.logs["train/clip_range_vf"] = self._now(self.clip_range_vf)

    def _prepare_epoch(self, flat, perm, bs, slot=0):
        """the epoch's shuffled copy of the rollout (buffer set `slot`), advantages normalised per minibatch"""
        total = perm.numel()
        n_seg, rem = divmod(total, bs)
        # one gather per epoch instead of one per minibatch: the shuffled copy makes every minibatch a
        # contiguous slice (same rows, same order as indexing the buffer with perm[s:s+bs])
        shuf = self._gather(flat, perm, slot)
        if self.normalize_advantage and bs * self.world > 1:
            # PPO.py:215-220 normalises per minibatch; all minibatches of the epoch in one launch (+ one
            # all-reduce of the per-minibatch sums when the minibatch spans several GPUs)
            scr = self._shuf.setdefault(("advn", slot), {})
            if scr.get("advn") is None or scr["advn"].shape != shuf["adv"].shape or scr["sums"].shape[0] != n_seg + 1:
                scr["advn"] = th.empty_like(shuf["adv"])
                scr["sums"] = th.empty((n_seg + 1, 2), dtype=th.float64, device=self.device)
            advn, sums = scr["advn"], scr["sums"]
            L, stv = _lib.lib(), self._stream()
            calls = [(_ptr(shuf["adv"]), _ptr(advn), n_seg, bs, bs * self.world, sums.data_ptr())]
            if rem > 1 or (rem == 1 and self.world > 1):       # PPO.py:216: only `if len(advantages) > 1`
                calls.append((_ptr(shuf["adv"], n_seg * bs), _ptr(advn, n_seg * bs), 1, rem, rem * self.world,
                              sums.data_ptr() + 16 * n_seg))
            elif rem == 1:
                advn[n_seg * bs:] = shuf["adv"][n_seg * bs:]
            if self.world > 1:
                for args in calls:
                    _lib.check(L.vf_adv_normalize_segments(*args, 0, stv))
                parallel.allreduce_sum_(sums)
                for args in calls:
                    _lib.check(L.vf_adv_normalize_segments(*args, 1, stv))
            else:
                for args in calls:
                    _lib.check(L.vf_adv_normalize_segments(*args, 2, stv))
            shuf["adv"] = advn
        return shuf

    def _gather(self, flat, perm, slot=0):
        """{name: rows of flat[name] in the order of perm} -- all fields in one launch (vf_gather_rows); the destination
        buffers (set `slot`) are kept between epochs"""
        if self._shuf is None:
            self._shuf = {}
        dst = self._shuf.get(slot)
        if dst is None or any(k not in dst or dst[k].shape != v.shape for k, v in flat.items()):
            dst = self._shuf[slot] = {k: th.empty_like(v) for k, v in flat.items()}
        gf = _lib.GatherFields()
        gf.n_fields = len(flat)
        for i, (k, v) in enumerate(flat.items()):
            gf.width[i], gf.src[i], gf.dst[i] = (v.shape[1] if v.dim() == 2 else 1), _ptr(v), _ptr(dst[k])
        _lib.check(_lib.lib().vf_gather_rows(C.byref(gf), perm.data_ptr(), perm.numel(), self._stream()))
        return dict(dst)

    def learn(self, total_timesteps: int, log_interval: Optional[int] = None, eval_env=None, eval_freq: Optional[int] = None):
        """PPO.learn (PPO.py:116-175): alternate rollout collection and training.  ``eval_env``: after an iteration, once ``eval_freq``
        timesteps have passed since the last evaluation (None: after every iteration), one deterministic episode per agent of that env
        (visfly_amd.evaluate.evaluate_policy) -> logs["rollout/ep_rew_mean" | "rollout/ep_len_mean" | "rollout/success_rate"] by the
        reference's 100-episode window of this call (in place of the training episodes' means), logs["eval/..."] over the last
        evaluation's episodes.  Draws no noise; without ``eval_env`` nothing changes"""
        t0 = time.time()
        start = self.num_timesteps
        it = 0
        sched = None
        if eval_env is not None:
            from .evaluate import EvalSchedule
            sched = self._eval_schedule = EvalSchedule(self, eval_env, 0 if eval_freq is None else eval_freq)
        while self.num_timesteps - start < total_timesteps:
            self.collect_rollouts()
            # SB3 _update_current_progress_remaining (PPO.py:150-152): after the rollout, before train()
            self._current_progress_remaining = 1.0 - float(self.num_timesteps - start) / float(total_timesteps)
            self.train()
            if sched is not None:          # (measured from the end of the iteration: an evaluation every eval_freq timesteps)
                sched.after_update(self.num_timesteps - start, self.num_timesteps - start, self.logs)
            it += 1
            if log_interval and it % log_interval == 0:
                th.cuda.synchronize(self.device)
                fps = (self.num_timesteps - start) / max(time.time() - t0, 1e-9)       # PPO._dump_logs :394-395
                self.logs["time/fps"] = fps
                print(f"[ppo] it {it} steps {self.num_timesteps} fps {fps:.3e} "
                      f"pg {self.logs['train/policy_gradient_loss']:.4f} v {self.logs['train/value_loss']:.4f}")
        th.cuda.synchronize(self.device)
        self.logs["time/fps"] = (self.num_timesteps - start) / max(time.time() - t0, 1e-9)
        return self
