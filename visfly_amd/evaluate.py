"""Deterministic evaluation episodes of a trained policy, and the reference trainers' ``rollout/*`` window.

The reference evaluates with the closed loop ``a = tanh(mean(obs))`` -> ``eval_env.step(a, is_test=True)`` until every agent has finished
one episode (utils/algorithms/BPTT.py:138-156, shac.py:284-300, utils/evaluate.py:79-129, ``visual=False``): done agents are not
re-spawned, ``done`` is sticky, and an agent's episode is what ``info[i]`` reported at the FIRST step that set its ``done``.  Here that is
one persistent launch (``vf_eval_rollout``, csrc/vf_eval_rollout.hip) where the library has the kernel for the network class and the env
configuration, else ``max_episode_steps`` rounds of forward -> ``vf_eval_action`` -> ``env.step`` -> ``vf_eval_latch`` without a host
sync; both leave the same bits.  Out of scope: plots / videos, ``visual=True``, world-model ``latent_func``.
"""
from collections import deque
from typing import Optional

import torch as th

from . import _lib, parallel
from .envs.base import EP_SUCCESS
from .policy import _ptr, policy_rows


class EvalResult:
    """one episode per agent, as device tensors: ``ep_return`` (N,) f32, ``ep_length`` (N,) i32, ``flags`` (N,) u8 (VF_EP_* bits),
    ``is_success`` (N,) bool, ``terminal_state`` (N, W) or None; ``path``: "persistent" or "loop".  ``record=True`` adds ``state_all``
    (T, N, W), ``action_all`` (T, N, 4), ``reward_all`` (T, N), ``done_all`` (T, N).  ``mean_r`` / ``mean_l`` (TestBase.test's two numbers)
    and ``success_rate`` are computed on first use: the only host syncs."""

    def __init__(self, ep_return, ep_length, flags, terminal_state=None, path="loop", **stacks):
        self.ep_return, self.ep_length, self.flags, self.terminal_state, self.path = ep_return, ep_length, flags, terminal_state, path
        self.is_success = (flags & EP_SUCCESS) != 0
        self.state_all, self.action_all = stacks.get("state_all"), stacks.get("action_all")
        self.reward_all, self.done_all = stacks.get("reward_all"), stacks.get("done_all")
        self._host = None

    def host(self):
        """(3, N) float64 host rows (ep_return, ep_length, is_success): ONE device-to-host copy, kept"""
        if self._host is None:
            self._host = th.stack([self.ep_return.to(th.float64), self.ep_length.to(th.float64), self.is_success.to(th.float64)]).cpu()
        return self._host

    @property
    def mean_r(self) -> float:
        return float(self.host()[0].mean())

    @property
    def mean_l(self) -> float:
        return float(self.host()[1].mean())

    @property
    def success_rate(self) -> float:
        return float(self.host()[2].mean())


class EpisodeWindow:
    """the reference's three ``deque(maxlen=100)`` of a ``learn()`` call (BPTT.py:85-91): episode returns, lengths and successes, the
    success deque pre-filled with ``maxlen`` times False"""

    def __init__(self, maxlen: int = 100):
        self.rewards, self.lengths, self.successes = deque(maxlen=maxlen), deque(maxlen=maxlen), deque([False] * maxlen, maxlen=maxlen)

    def add(self, r, l, success):
        """one finished episode (BPTT.py:151-153)"""
        self.rewards.append(float(r))
        self.lengths.append(int(l))
        self.successes.append(bool(success))

    def extend(self, result: EvalResult):
        """a whole evaluation in the reference's order (BPTT.py:142-156): ascending first-done step -- all agents start together, so that is
        the episode length -- and within a step descending agent index (``for index in reversed(eval_info_id_list)``)"""
        r, l, s = result.host().tolist()
        for i in sorted(range(len(r)), key=lambda i: (l[i], -i)):
            self.add(r[i], l[i], s[i] != 0.0)
        return self

    def means(self):
        """``rollout/ep_rew_mean | ep_len_mean | success_rate`` by the ``sum / len`` rule (BPTT.py:160-162)"""
        n = len(self.rewards)
        return {"rollout/ep_rew_mean": sum(self.rewards) / n if n else float("nan"),
                "rollout/ep_len_mean": sum(self.lengths) / n if n else float("nan"),
                "rollout/success_rate": sum(self.successes) / len(self.successes)}


def _loop(model, env, obs, res, want_terminal, record):
    """launch by launch: max_episode_steps rounds, no host sync, no ``done.all()`` test (``done`` is sticky: later rounds change nothing
    that is latched)"""
    pol, keys, N, dev = model.policy, model.obs_keys, env.num_agent, env.device
    L, st = _lib.lib(), _lib.current_stream(dev)
    slot = getattr(model, "H", -1) + 1         # (BPTT / SHAC: the slot predict() uses, behind the horizon's)
    latched = th.zeros(N, dtype=th.uint8, device=dev)
    T = env.max_episode_steps
    stacks = None
    if record:
        W = policy_rows(obs, ["state"])["state"].shape[-1]
        f = dict(dtype=th.float32, device=dev)
        stacks = dict(state_all=th.empty((T, N, W), **f), action_all=th.empty((T, N, 4), **f), reward_all=th.empty((T, N), **f),
                      done_all=th.empty((T, N), dtype=th.bool, device=dev))
    action = th.empty((N, 4), dtype=th.float32, device=dev)
    for t in range(T):
        mean, _ = pol.forward(policy_rows(obs, keys), save_activations=False, slot=slot)
        a = stacks["action_all"][t] if record else action
        _lib.check(L.vf_eval_action(_ptr(mean), _ptr(a), N, st))
        obs, reward, done, _ = env._step_no_grad(a, True, borrow=True)
        term = env._terminal_state_rows() if want_terminal else None
        _lib.check(L.vf_eval_latch(done.data_ptr(), _ptr(env._ep_return), env._ep_length.data_ptr(), env._ep_flags.data_ptr(), _ptr(term),
                                   latched.data_ptr(), _ptr(res["ep_return"]), res["ep_length"].data_ptr(), res["flags"].data_ptr(),
                                   _ptr(res["terminal_state"]), N, 0 if term is None else term.shape[-1], st))
        if record:
            stacks["state_all"][t].copy_(obs["state"])
            stacks["reward_all"][t].copy_(reward)
            stacks["done_all"][t].copy_(done)
    return stacks or {}


def evaluate_policy(model, eval_env, *, persistent: bool = True, terminal_rows: bool = False, record: bool = False) -> EvalResult:
    """One deterministic episode per agent of ``eval_env`` under ``model.policy`` (a ``PPO``, ``BPTT`` or ``SHAC``) -> ``EvalResult``.

    ``eval_env`` must not be ``model.env`` (a BPTT env holds the tape, a PPO env the trainer's last observation).  The function sets on
    ``eval_env`` what the trainers set on their own env -- ``tensor_output = True`` and, on the racing envs, ``obs_gate_exact = False`` (the
    policy is fed every agent's CURRENT gate) --, resets it, and runs the evaluation: one persistent launch where the library serves the
    configuration (``persistent=True``; not with replay spawn, IMU noise, string wind, a pending step_begin(), host-formed observations, or
    a network on the layer-by-layer paths: these fall back with one warning), else launch by launch.  ``terminal_rows``: also keep every
    agent's terminal "state" row.  ``record=True`` runs the loop and keeps the (T, N, .) stacks of state, action, reward and done.  Draws
    no noise and touches no generator.  Afterwards ``eval_env`` needs a ``reset()`` before it is stepped again."""
    if eval_env is getattr(model, "env", None):
        raise ValueError("evaluate_policy: eval_env must be a different object from model.env")
    env = eval_env
    env.tensor_output = True
    if hasattr(env, "obs_gate_exact"):
        env.obs_gate_exact = False
    env.reset()
    obs = env.get_observation()
    N, dev = env.num_agent, env.device
    rows = policy_rows(obs, model.obs_keys)
    W = rows["state"].shape[-1]
    res = dict(ep_return=th.zeros(N, dtype=th.float32, device=dev), ep_length=th.zeros(N, dtype=th.int32, device=dev),
               flags=th.zeros(N, dtype=th.uint8, device=dev),
               terminal_state=th.zeros((N, W), dtype=th.float32, device=dev) if terminal_rows else None)
    path, stacks = "loop", {}
    if persistent and not record and env.evaluate_policy_launch(model.policy, model.obs_keys, rows, res["ep_return"], res["ep_length"],
                                                                res["flags"], res["terminal_state"]):
        path = "persistent"
    else:
        if persistent and not record and "evaluate_policy" not in _lib._warned:       # (once, like _lib.warn_unsupported)
            _lib._warned.add("evaluate_policy")
            import warnings
            warnings.warn("visfly_amd: no persistent evaluation launch for this env / network configuration (replay spawn, IMU noise, string "
                          "wind, host-formed observations, a network on the layer-by-layer paths, or no kernel for the class: see the "
                          "vf_eval_rollout warning); evaluating launch by launch (same results)", stacklevel=2)
        stacks = _loop(model, env, obs, res, terminal_rows, record)
        env._is_initial = False         # every agent is done: reset() before the next step(), as after the persistent launch
    return EvalResult(res["ep_return"], res["ep_length"], res["flags"], res["terminal_state"], path, **stacks)


class EvalSchedule:
    """the evaluation part of a trainer's ``learn()`` call: one ``EpisodeWindow``, evaluations every ``dump_step`` timesteps by the
    reference's test (BPTT.py:137,174: the timesteps completed BEFORE the update, minus those at the last dump, reach ``dump_step``)"""

    def __init__(self, model, eval_env, dump_step):
        self.model, self.env, self.dump_step = model, eval_env, dump_step
        self.window, self.previous = EpisodeWindow(), 0
        self.results = []          # the EvalResult of every evaluation of this learn() call

    def after_update(self, before: int, current: int, logs: dict) -> Optional[EvalResult]:
        """before / current: timesteps of this learn() call before / after the update that just ended"""
        if self.env is None or before - self.previous < self.dump_step:
            return None
        res = evaluate_policy(self.model, self.env)
        self.results.append(res)
        logs.update(self.window.extend(res).means())
        tot = th.cat([res.host().sum(dim=1), th.tensor([float(res.host().shape[1])], dtype=th.float64)]).to(self.env.device)
        parallel.allreduce_sum_(tot)          # over all episodes of this evaluation, on every rank
        tot = tot.tolist()
        logs.update({"eval/ep_rew_mean": tot[0] / tot[3], "eval/ep_len_mean": tot[1] / tot[3], "eval/success_rate": tot[2] / tot[3]})
        self.previous = current
        return res
