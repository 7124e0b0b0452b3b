"""The persistent launches of the envs -- a whole BPTT / SHAC horizon (both halves), PPO's collect_rollouts, the deterministic evaluation
episodes: policy and env step in ONE launch each -- as a mixin of ``DroneGymEnvsBase`` (envs/base.py).

Every entry point answers False when the launch does not serve the env / network / dynamics configuration at hand, and the caller then
steps launch by launch.  What they share is written once: the eligibility test (``_persistent_ok``), the kernel-side configuration tuple
(``_kernel_cfg``), the plugin of a generated chain class (``_ensure_plugin``), the result code (``_launched``) and the scratch the launches
write their last step's rows to (``_launch_scratch``).
"""
import ctypes as C
import warnings

import torch as th

from .. import _lib
from .._lib import VisflyError

_RACING = 2     # DroneGymEnvsBase.KIND of the racing envs
# launch kind -> (its function in visfly_amd/_jit.py, the word for it in the fall-back warning)
_PLUGIN = {"bptt": ("ensure_bptt", "BPTT"), "rollout": ("ensure_rollout", "roll-out"), "eval": ("ensure_eval", "evaluation")}


def _launched(rc, name):
    """result code of the persistent launch `name` -> True, or False (with the library's warning) when it has no kernel for this
    env / network / dynamics configuration"""
    if rc == _lib.EUNSUPPORTED:
        _lib.warn_unsupported(name)
        return False
    if rc:
        _lib.check(rc)
    return True


class PersistentLaunches:
    # the persistent launches (rollout_policy / reverse_policy / collect_policy / evaluate_policy_launch) exist for this env's "state" rows:
    # 13 columns, or RacingEnv2's 16.  False (TrackEnv: 40 columns behind the step kernel): every one of them answers False before any
    # library call -- their kernels are instantiated for the two widths above and would index such rows out of bounds
    _PERSISTENT = True

    def _persistent_ok(self, tape=None, obs_keys=None, policy=None):
        """does the env as it stands take a persistent launch?  tape: True = it must be recording, False = it must not, None = either.
        The PPO-side launches (collect_policy / evaluate_policy_launch) pass their obs_keys and policy: the launch then also needs the
        step kernel's own terminal rows, observation keys it takes, and a fused network over this env's "state" width."""
        W = self._OBS_W        # 13, or the 16 gate-relative columns the persistent launches form themselves for RacingEnv2 (VF_OBS_RACE2)
        if ((tape is not None and tape != (self._tape is not None)) or self.spawn_mode != "device" or self._imu_noise is not None
                or self._half_step or self.envs.dynamics._wind_fn is not None or (getattr(self, "_HOST_OBS", False) and W == 13)
                or not self.tensor_output or getattr(self, "obs_gate_exact", False)):
            return False
        return policy is None or not ((W == 13 and self._terminal_state_rows() is not self._terminal_obs)
                                      or not self._persistent_keys_ok(obs_keys) or policy._plan is None or not policy.fused
                                      or policy.obs_dims.get("state") != W)

    def _persistent_keys_ok(self, obs_keys):
        """observation keys the persistent launches take: "state", plus at most one of the constant "target" rows or -- racing envs
        only -- the "gate" index column"""
        keys = list(obs_keys)
        return (all(k in ("state", "target", "gate") for k in keys) and not ("target" in keys and "gate" in keys)
                and ("gate" not in keys or self.KIND == _RACING))

    def _kernel_cfg(self):
        """(kernel-side env kind, VF_ACT_*, VF_INT_*, ctrl_delay): what a persistent launch is instantiated for"""
        c = self.envs.dynamics.constants
        kind = 3 if self._OBS_W == 16 else self.KIND       # kernel-side kind: VF_ENV_RACING2 forms RacingEnv2's 16 columns itself
        return kind, int(c["action_type"]), int(c["integrator"]), bool(c["ctrl_delay"])

    def _ensure_plugin(self, policy, kind):
        """a generated chain class: its persistent launches are one more plugin each -- "bptt" (both launches of a horizon), "rollout",
        "eval" -- per env kind / action type / integrator / motor lag (visfly_amd/_jit.py: ensure_bptt / ensure_rollout / ensure_eval;
        ~15 s of hipcc on first use, the BPTT plugin ~2 min; its launches run 16 agents per wave: N <= 16 384)"""
        if not getattr(policy, "chain_jit", False) or (kind == "bptt" and self.num_agent > 16384):
            return
        ensure, word = _PLUGIN[kind]
        try:
            from .. import _jit
            getattr(_jit, ensure)(policy.chain_shape, self._kernel_cfg())
        except Exception as e:          # no hipcc, ...: launch by launch, with the library's warning
            warnings.warn(f"visfly_amd: no {word} plugin for this network ({e})")

    def _after_persistent_launch(self):
        """host-side caches of per-step state that a persistent launch stepped past (overridden where an env keeps any)"""

    def _launch_scratch(self):
        """reward / done / observation scratch and the vf_env_out of the persistent launches"""
        sc = getattr(self, "_collect_scratch", None)
        if sc is None:
            N, W, dev = self.num_agent, self._OBS_W, self.device
            sc = self._collect_scratch = {"reward": th.empty(N, dtype=th.float32, device=dev),
                                          "done": th.empty(N, dtype=th.bool, device=dev),
                                          "state": th.empty((N, W), dtype=th.float32, device=dev)}
            sc["out"] = self._out(sc["state"], sc["reward"], sc["done"])
            if W != 13:         # the launch's terminal rows are W wide as well: a buffer of their own
                sc["terminal"] = th.zeros((N, W), dtype=th.float32, device=dev)
                sc["out"].terminal_obs = _lib.ptr(sc["terminal"])
        return sc

    def rollout_policy(self, policy, obs_keys, eps, actions, d_reward, loss, disc, gamma, scale, reward_rows=None, ep_flag_rows=None):
        """H = eps.shape[0] closed-loop control steps -- policy forward (slots 0..H-1 of `policy`, reserved back to back), action
        head, state checkpoint on the tape, fused env step, loss / discount recurrence -- in ONE persistent launch
        (vf_bptt_rollout).  obs_keys: "state", plus the constant "target" rows or, on the racing envs, the "gate" index column
        (StateGateExtractor: the launch takes the index it holds after every step and writes it to the slots' "obs:gate").  Leaves exactly what H rounds of policy.forward_act + _step_no_grad(record=True) +
        vf_bptt_accumulate leave.  A policy with two 4-wide heads and no log_std parameter is the reference's own Actor
        (td_policies.py:146-252): state-dependent log_std, what H rounds of policy.forward + vf_shac_head_fwd leave, the heads of
        every step in the slots' "mean" / "value" buffers.  -> False when the library has no roll-out kernel for this env / network
        / dynamics configuration (the caller then steps launch by launch).  ``reward_rows`` (H,N) / ``ep_flag_rows`` (H,N) uint8:
        optional per-step copies of the reward and of the episode flags (valid where done) -- SHAC's horizon buffer."""
        if not self._PERSISTENT:
            return False
        if not self._persistent_ok(tape=True):
            return False
        H, N, W, dev = eps.shape[0], self.num_agent, self._OBS_W, self.device
        t0 = self._tape_t
        if t0 + H > self._tape.shape[0]:
            raise VisflyError("tape is full: call env.detach() (BPTT horizon exceeded)")
        nblk, blk = policy._slot_blocks.get(N, (0, None))
        if nblk < H or not self._persistent_keys_ok(obs_keys):
            return False
        obs = self.get_observation()
        blk["obs:state"][0].copy_(obs["state"].detach())
        o1 = None
        if "target" in obs_keys:
            blk["obs:target"][:H].copy_(obs["target"].detach().unsqueeze(0).expand(H, N, -1))     # constant per env
            o1 = blk["obs:target"]
        elif "gate" in obs_keys:
            # the gate column (StateGateExtractor): slot 0 = the agents' current index, the one the "state" rows above were formed with
            # (obs_gate_exact is False here); the launch writes the later slots from the index it holds after every step
            blk["obs:gate"][0].copy_(obs["gate"].detach().reshape(N, 1))
            o1 = blk["obs:gate"]
        d = policy.forward_desc(N, 0, True)
        policy._pack()
        sc = self._launch_scratch()
        final = th.empty((N, W), dtype=th.float32, device=dev)
        # sub-step tape (include/visfly_amd.h, vf_bptt_rollout): what the reverse launch reads instead of replaying every interval;
        # one (S + 3 rows, waves of 16 agents, 64) float4 record block per tape row, allocated with the first persistent roll-out
        # ... and only where the reverse launch reads it (vf_bptt_reverse: 16 agents per wave, i.e. N <= 16 384 per launch, and a
        # delay ring of at most 4 slots): elsewhere it would be (S + 3) KiB per wave-step of stores nobody loads
        sub = None
        if self.substep_tape and N <= 16384 and self.envs.dynamics._comm_delay_steps <= 4:
            S = int(self.envs.dynamics.constants["interval_steps"])
            shape = (self._tape.shape[0], S + 3, (N + 15) // 16, 64, 4)
            if getattr(self, "_substep", None) is None or tuple(self._substep.shape) != shape:
                self._substep = th.empty(shape, dtype=th.float32, device=dev)
            sub = self._substep[t0]
        self._substep_range = None
        two_heads = tuple(policy.head_dims) == (4, 4) and policy.log_std.numel() == 0
        self._ensure_plugin(policy, "bptt")
        with th.cuda.device(dev):
            rc = _lib.lib().vf_bptt_rollout(
                self._h, C.byref(d), _lib.ptr(policy.flat), _lib.ptr(policy._packed), _lib.ptr(blk["obs:state"]), _lib.ptr(o1),
                None if two_heads else _lib.ptr(policy.log_std), _lib.ptr(eps), _lib.ptr(actions), C.byref(sc["out"]), _lib.ptr(final),
                _lib.ptr(self._tape[t0]), self._slab.numel(), self._tape_done[t0].data_ptr(), _lib.ptr(d_reward), _lib.ptr(loss),
                _lib.ptr(disc), float(gamma), float(scale), H, _lib.ptr(sub), _lib.ptr(blk["mean"]) if two_heads else None,
                _lib.ptr(blk["value"]) if two_heads else None, _lib.ptr(reward_rows),
                None if ep_flag_rows is None else ep_flag_rows.data_ptr(), self._stream())
        if not _launched(rc, "vf_bptt_rollout"):
            return False
        if sub is not None:
            self._substep_range = (t0, t0 + H)
        for t in range(H):
            self._tape_action_ref[t0 + t] = actions[t]
        self._tape_t = t0 + H
        self._qcache = self._imu_cache = self._ext_col = None
        self._action = actions[H - 1]
        self._reward, self._done = sc["reward"], self._tape_done[t0 + H - 1]
        self._after_persistent_launch()
        self._observations = self._full_obs(final)
        policy._last_M, policy._last_slot = N, H - 1
        return True

    def evaluate_policy_launch(self, policy, obs_keys, rows, ep_return, ep_length, ep_flags, terminal_rows=None):
        """one deterministic episode per agent from the current (freshly reset) state -- a = tanh(mean(obs)) -> step(is_test=True)
        until every agent is done, max_episode_steps steps at the latest -- in ONE persistent launch (vf_eval_rollout).  rows: the
        policy's observation rows of the current state (ppo.policy_rows); ep_return (N,) f32 / ep_length (N,) i32 / ep_flags (N,) u8 /
        terminal_rows (N, W) or None take every agent's episode as reported at its FIRST done step.  -> True, or False when the launch
        does not serve this env / network / dynamics configuration: collect_policy's conditions, except that a tape may exist (nothing is
        recorded).  Afterwards the env needs a reset() (waves leave the launch once their agents are done)."""
        if not self._PERSISTENT:
            return False
        if not self._persistent_ok(None, obs_keys, policy):
            return False
        assert self._is_initial, "You should call reset() before step()"
        d = policy.forward_desc(self.num_agent, 0, False)
        policy._pack()
        sc = self._launch_scratch()
        o1 = rows["target"] if "target" in obs_keys else rows["gate"] if "gate" in obs_keys else None
        a = _lib.EvalRolloutArgs()
        a.T_max, a.w1 = self.max_episode_steps, 0 if o1 is None else o1.shape[-1]
        a.obs_state, a.obs_second, a.obs_scratch = _lib.ptr(rows["state"]), _lib.ptr(o1), _lib.ptr(sc["state"])
        a.ep_return, a.ep_length, a.ep_flags = _lib.ptr(ep_return), ep_length.data_ptr(), ep_flags.data_ptr()
        a.terminal_rows = _lib.ptr(terminal_rows)
        a.out = C.addressof(sc["out"])
        self._ensure_plugin(policy, "eval")
        with th.cuda.device(self.device):
            rc = _lib.lib().vf_eval_rollout(self._h, C.byref(d), _lib.ptr(policy.flat), _lib.ptr(policy._packed), C.byref(a), self._stream())
        if not _launched(rc, "vf_eval_rollout"):
            return False
        self._qcache = self._imu_cache = self._ext_col = None
        self._reward, self._done = sc["reward"], sc["done"]
        self._after_persistent_launch()
        self._is_initial = False
        return True

    def collect_policy(self, policy, obs_keys, buf, boot, noise_key, sample_step, last_starts):
        """T = buf.actions.shape[0] rounds of PPO's collect_rollouts loop -- policy.forward (both heads), squashed-Gaussian
        sample + log-prob (Philox counters sample_step + 1 ..), env.step, RolloutBuffer rows, TimeLimit list / episode
        statistics -- in ONE persistent launch (vf_ppo_rollout).  buf.obs["state"][0] (and every row of buf.obs["target"])
        and buf.episode_starts[0] are the caller's.  -> the final observation TensorDict, or False when the library has no
        roll-out kernel for this env / network / dynamics configuration (the caller then steps launch by launch)."""
        if not self._PERSISTENT:
            return False
        W = self._OBS_W        # 13, or RacingEnv2's 16 columns (formed inside the launch: VF_OBS_RACE2)
        if not self._persistent_ok(False, obs_keys, policy) or buf.obs["state"].shape[-1] != W:
            return False
        assert self._is_initial, "You should call reset() before step()"
        T, N, dev = buf.actions.shape[0], self.num_agent, self.device
        d = policy.forward_desc(N, 0, False)
        policy._pack()
        sc = self._launch_scratch()
        final = th.empty((N, W), dtype=th.float32, device=dev)
        # the second observation: the constant "target" rows, or the "gate" column (row 0 the caller's, the later rows the launch's)
        o1 = buf.obs["target"] if "target" in obs_keys else buf.obs["gate"] if "gate" in obs_keys else None
        a = _lib.PpoRolloutArgs()
        a.T, a.w1, a.capacity = T, 0 if o1 is None else o1.shape[-1], boot["cap"]
        a.obs_state, a.obs_target = _lib.ptr(buf.obs["state"]), _lib.ptr(o1)
        a.obs_target_row = None if o1 is None else _lib.ptr(o1[0])
        a.obs_final, a.means, a.values = _lib.ptr(final), None, _lib.ptr(buf.values)
        a.actions, a.log_probs, a.rewards = _lib.ptr(buf.actions), _lib.ptr(buf.log_probs), _lib.ptr(buf.rewards)
        a.episode_starts, a.last_starts, a.log_std = _lib.ptr(buf.episode_starts), _lib.ptr(last_starts), _lib.ptr(policy.log_std)
        a.noise_key, a.sample_step = noise_key, sample_step
        a.cursor, a.idx_list, a.rows0 = boot["cursor"].data_ptr(), boot["idx"].data_ptr(), _lib.ptr(boot["rows0"])
        a.rows1, a.stat = _lib.ptr(boot["rows1"]), _lib.ptr(boot["stat"])
        a.out = C.addressof(sc["out"])
        self._ensure_plugin(policy, "rollout")
        with th.cuda.device(dev):
            rc = _lib.lib().vf_ppo_rollout(self._h, C.byref(d), _lib.ptr(policy.flat), _lib.ptr(policy._packed), C.byref(a), self._stream())
        if not _launched(rc, "vf_ppo_rollout"):
            return False
        self._qcache = self._imu_cache = self._ext_col = None
        self._action = buf.actions[T - 1]
        self._reward, self._done = sc["reward"], sc["done"]
        self._after_persistent_launch()
        self._observations = obs = self._full_obs(final)
        return obs

    def reverse_policy(self, policy, H, eps, actions, d_reward, d_means, g_log_std, d_log_stds=None):
        """the reverse half of the last H recorded steps in ONE persistent launch (vf_bptt_reverse): for t = H-1 .. 0 the adjoint of
        env step t and the policy's action-head reverse + reverse chain of slot t.  -> False when the library has no kernel for
        this configuration (the caller then sweeps launch by launch).  d_means (H,N,4) out, g_log_std (H,N,4) zeroed in / out.
        ``d_log_stds`` (H,N,4) out instead of g_log_std: the reference's Actor (two heads, see rollout_policy) -- both trunks are
        swept, the head gradients of every step land in d_means / d_log_stds."""
        if not self._PERSISTENT:
            return False
        N = self.num_agent
        t0 = self._tape_t - H
        nblk, blk = policy._slot_blocks.get(N, (0, None))
        if self._tape is None or t0 < 0 or nblk < H or self.envs.dynamics._wind_fn is not None:    # (wind rows: one launch per step)
            return False
        two_heads = d_log_stds is not None
        d, d_in, d_action = policy.reverse_flat_desc(N, H, d_means, d_log_stds)
        policy._pack()
        # the sub-step tape only if exactly these H steps were recorded by ONE persistent roll-out with the tape on
        sub = self._substep[t0] if getattr(self, "_substep_range", None) == (t0, t0 + H) else None
        with th.cuda.device(self.device):
            rc = _lib.lib().vf_bptt_reverse(self._h, C.byref(d), _lib.ptr(policy._packed), None if two_heads else _lib.ptr(policy.log_std),
                                            _lib.ptr(eps), _lib.ptr(actions), _lib.ptr(self._tape[t0]), self._slab.numel(),
                                            self._tape_done[t0].data_ptr(), _lib.ptr(d_reward), _lib.ptr(self._adj), _lib.ptr(d_action),
                                            _lib.ptr(d_in["state"]), None if two_heads else _lib.ptr(g_log_std), H, _lib.ptr(sub),
                                            _lib.ptr(blk["value"]) if two_heads else None, self._stream())
        return _launched(rc, "vf_bptt_reverse")
