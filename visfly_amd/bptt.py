"""First-order (differentiable-simulation) policy optimisation: BPTT over a horizon of env steps.

Restates ``BPTT.learn`` of the reference (utils/algorithms/BPTT.py:77-180): roll the policy through
H env steps with ``requires_grad=True``, loss = mean_i sum_t -reward_t * discount_t with
``discount <- discount * gamma * ~done + done`` (:107-124), back-propagate through the simulator,
clip the gradient norm to 0.5, Adam step, ``env.detach()`` (:127-134).

Where the reference relies on a torch autograd tape of ~3.8k nodes per control step, here the
simulator's reverse pass is the hand-written adjoint kernel ``vf_env_step_bwd`` (one launch per
step) and the policy's is the MFMA linear-layer kernels; ``torch.autograd`` is only the scheduler
that orders those launches (two custom Functions), so any torch policy can be dropped in as well.

Extractors: ``StateExtractor``, ``StateTargetExtractor`` and, on the racing envs, ``StateGateExtractor`` (both actors): the "gate" index
is fed as one float32 column holding the agent's current gate, carries no gradient (``env.backward_step`` receives d obs["state"] only),
and on the persistent launches of a generated class comes from the index the wave holds.  Not part of this: a full ``BPTT.learn``
fixture of the reference on the racing envs (the loop is pinned by bptt_loop_hover*, RacingEnv2's adjoint by bptt_racing2_thrust).

String wind functions (``wind_settings`` of six expressions) are host lambdas re-evaluated before every step, so under them a horizon
steps launch by launch in both directions (``rollout_policy`` / ``reverse_policy`` answer False): the tape keeps the per-agent wind rows
of every recorded step and ``env.backward_step`` hands them to ``vf_env_step_bwd_wind``; on the reference's tape the wind is a constant
of the step as well (fixtures ``bptt_wind_*``, ``bptt_loop_hover_wind``).
"""
import os
import time
from typing import Dict, Optional

import torch as th

from . import _lib, checkpoint, parallel
from .checkpoint import trainer_obs_keys
from .policy import INDEX_OBS_KEYS, MlpPolicy, _ptr, activation_kind, obs_width, policy_rows


class EnvStepFunction(th.autograd.Function):
    """env.step with the adjoint kernel as backward.  `token` threads the hidden simulator state through
    the graph so that autograd runs step t's backward after step t+1's (the adjoint slab is in/out)."""

    @staticmethod
    def forward(ctx, action, token, env, is_test):
        obs, reward, done, info = env._step_no_grad(action.detach(), is_test, record=True)
        ctx.env, ctx.t = env, env._tape_t - 1
        env._last_step_aux = (obs, done, info)
        return obs["state"], reward, token + 1

    @staticmethod
    def backward(ctx, d_obs, d_reward, d_token):
        d_action = ctx.env.backward_step(ctx.t, d_obs, d_reward)
        return d_action, d_token, None, None


class PolicyFunction(th.autograd.Function):
    """MlpPolicy mean head: forward / backward on the MFMA linear kernels; parameter gradients are
    accumulated into ``policy.grad`` (flat), the observation gradient is returned to autograd."""

    @staticmethod
    def forward(ctx, policy, keys, anchor, *obs):
        # `anchor` is a dummy leaf that requires grad: the parameters live outside autograd (flat buffer), so without
        # it the node of the FIRST step -- whose observation carries no graph -- would never run its backward and
        # that step's parameter gradient would be lost
        ctx.policy, ctx.keys = policy, keys
        ctx.save_for_backward(*obs)
        mean, _ = policy.forward({k: o.detach().contiguous() for k, o in zip(keys, obs)})
        return mean.clone()

    @staticmethod
    def backward(ctx, d_mean):
        pol = ctx.policy
        obs = ctx.saved_tensors
        pol.forward({k: o.detach().contiguous() for k, o in zip(ctx.keys, obs)})   # activations of THIS step
        d_in = pol.backward(d_mean.contiguous(), None, None, accumulate=True, need_input_grad=True)
        return (None, None, None) + tuple(d_in.get(k) for k in ctx.keys)


# the reference constructs ``BPTT(env, policy, policy_kwargs, ...)`` with one of utils/policies/td_policies.py's policies (BPTT.py:13,
# 29-49); its loop then runs ``self.policy.actor.action_log_prob(obs)`` (:113), i.e. the SAC-style Actor with the state-dependent
# log_std head (td_policies.py:146-252).  These names select that actor here; None keeps the MlpPolicy with a state-independent log_std
REFERENCE_ACTOR_POLICIES = ("MultiInputPolicy", "MTDPolicy", "CnnPolicy", "MlpPolicy")
LOG_STD_MAX, LOG_STD_MIN = 2.0, -10.0        # td_policies.py:31-32


def _require_differentiable_actions(env, trainer):
    """the adjoint (vf_env_step_bwd, vf_bptt_rollout / vf_bptt_reverse) covers the thrust and bodyrate action types.  The geometric
    controller of velocity / position has no reference gradient to pin: the reference's own autograd raises on it (the per-agent loop of
    envs/base/dynamics.py:446-450,481-488 writes in place into tensors the graph needs, and builds pose_err / the yaw-rate vector with
    th.as_tensor / th.tensor, which detach them).  PPO and evaluate_policy run these two action types."""
    from .constants import ACTION_TYPES
    dyn = getattr(getattr(env, "envs", None), "dynamics", None)
    act = None if dyn is None else int(dyn.constants["action_type"])
    for name in ("velocity", "position"):
        if act == ACTION_TYPES[name]:
            raise NotImplementedError(
                f"{trainer} over action_type=\"{name}\": the reference's autograd raises for the geometric controller of the velocity / "
                "position action types (\"one of the variables needed for gradient computation has been modified by an inplace "
                "operation\"; parts of its graph are detached as well), so there is no gradient to reproduce.  The env-step adjoint covers "
                "\"thrust\" and \"bodyrate\"; train these action types with PPO")


def _pth(path):
    """file name of a plain torch archive (reference actor, SHAC)"""
    return path if path.endswith(".pth") else path + ".pth"


class BPTT:
    # True: the reference's own actor (two trunks, mu / clamped state-dependent log_std heads) -- set by naming a td_policies policy;
    # SHAC always uses it.  _critic_arch / _share_extractor: what _make_reference_actor parses for SHAC's critics
    reference_actor = False
    _critic_arch = None
    _share_extractor = False

    def __init__(self, env, horizon: int = 32, gamma: float = 0.99, learning_rate: float = 1e-3,
                 max_grad_norm: float = 0.5, weight_decay: float = 0.0, policy_kwargs: Optional[dict] = None,
                 seed: int = 0, betas=(0.9, 0.999), adam_eps: float = 1e-8, policy=None, dump_step: float = 1e4):
        if policy is not None and not isinstance(policy, str):
            policy = getattr(policy, "__name__", str(policy))
        if policy is not None and policy not in REFERENCE_ACTOR_POLICIES:
            raise NotImplementedError(f"policy {policy}: one of {REFERENCE_ACTOR_POLICIES} (vector observations) or None")
        _require_differentiable_actions(env, type(self).__name__)
        if policy is not None:
            self.reference_actor = True
        self._eps_override = None           # tests: the exploration noise of the next horizon(s), fed instead of drawn
        self.env, self.H, self.gamma = env, horizon, gamma
        self.dump_step = dump_step          # learn(eval_env=...): timesteps between two evaluations (BPTT.py:137)
        self.lr, self.max_grad_norm, self.weight_decay, self.betas, self.adam_eps = learning_rate, max_grad_norm, weight_decay, betas, adam_eps
        self.device = env.device
        env.set_requires_grad(True, horizon=horizon)        # shac.py:124 sets env.requires_grad = True
        env.tensor_output = True
        if not env._is_initial:
            env.reset()
        obs = env.get_observation()
        self.obs_keys = trainer_obs_keys(obs, policy_kwargs)
        if hasattr(env, "obs_gate_exact"):       # RacingEnv: skip the per-step bookkeeping launches of the returned "gate" entry; a policy
            env.obs_gate_exact = False           # that reads it (StateGateExtractor) is fed the agent's CURRENT gate, the index its "state"
                                                 # rows are formed with
        self.policy = self._make_policy(obs, policy_kwargs, seed)
        self.policy.lazy_pack = True        # this trainer calls mark_updated() after every optimiser step
        self.world, self.rank = parallel.world_size(), parallel.rank()
        # same initial parameters on every rank (only gradients are exchanged afterwards), different exploration noise
        parallel.broadcast_(self.policy.flat)
        self.policy.mark_updated()
        self.use_autograd = False           # True: torch.autograd schedules the same kernels (cross-check path)
        self.fused_rollout = True           # forward half of a horizon as one persistent launch where the library has the kernel
        self.fused_reverse = True           # ... and the reverse half (only after a fused forward: same tape / slot buffers)
        self._defer_wgrad = None            # decided at the first update (MlpPolicy.backward_data_supported)
        n = self.policy.n_params
        self.exp_avg, self.exp_avg_sq = th.zeros(n, device=self.device), th.zeros(n, device=self.device)
        self._sumsq, self._scratch = th.zeros(1, device=self.device), th.zeros(4096, device=self.device)
        self.seed = seed
        self._gen = th.Generator(device=self.device).manual_seed(int(seed) + 1000003 * self.rank)
        # over a globally keyed env (envs/base.py: agent_offset) the per-agent exploration noise is vf_noise_fill's stream instead:
        # a function of (seed, agent_offset + row, step) alone, the same on every rank.  _noise_step counts the rows drawn so far
        self._row0 = getattr(env, "agent_offset", None)
        self._noise_step = 0
        self._opt_step = 0
        self.num_timesteps = 0
        self.logs: Dict[str, float] = {}

    def _noise(self, T, N):
        """(T, N, 4) standard normals: exploration noise of T consecutive steps of N agents"""
        if self._row0 is None:
            return th.randn((T, N, 4), device=self.device, generator=self._gen)
        eps = th.empty((T, N, 4), dtype=th.float32, device=self.device)
        _lib.check(_lib.lib().vf_noise_fill(_lib.ptr(eps), T, N, self._row0, int(self.seed) & (2 ** 64 - 1), self._noise_step,
                                            _lib.current_stream(self.device)))
        self._noise_step += T
        return eps

    def _make_reference_actor(self, obs, policy_kwargs, seed):
        """td_policies.Actor (:146-252): extractor -> (latent_pi -> mu | log_latent_pi -> log_std); nn.Linear default initialisation
        (SB3's SAC policies do not use orthogonal init), log_latent_pi = deepcopy(latent_pi) (:205).  One MlpPolicy layer table with
        two 4-wide heads; sets self._extractor / _ext_keys / _critic_arch (SHAC builds its critics from them).
        ``net_arch``: dict(pi=..., qf=...) or a plain list (SB3's get_actor_critic_arch: the same sizes for actor and critics).  Without
        one the trunks are [64, 64] here; the REFERENCE's default is [256, 256] (MTDPolicy's net_arch=None, td_policies.py:295, which
        SB3's SACPolicy turns into [256, 256]) -- ask for it with ``policy_kwargs=dict(net_arch=[256, 256])``.  Layers wider than 128 (up
        to 512) run layer by layer on the wide linear kernels: no persistent horizon launches for such a network."""
        pk = dict(policy_kwargs or {})
        na = pk.get("net_arch")
        if isinstance(na, dict) and "qf" in na:                       # SB3 get_actor_critic_arch: dict(pi=..., qf=...)
            self._critic_arch = list(na["qf"])
            pk["net_arch"] = dict({k: v for k, v in na.items() if k != "qf"}, pi=list(na["pi"]), vf=list(na["pi"]))    # (flags such as pi_ln stay)
        # share_features_extractor=True (td_policies.py:127, SACPolicy._build): the critic runs the ACTOR's extractor under no_grad.  BPTT has
        # no critic (nothing changes); SHAC reads the flag (shac.py: _share_extractor)
        if pk.get("pi_features_extractor_class") is not None or pk.get("vf_features_extractor_class") is not None:
            raise NotImplementedError(f"{type(self).__name__}: pi_features_extractor_class / vf_features_extractor_class (separate pi / vf "
                                      "feature extractors of the actor-critic policy) are not implemented for the td policies; PPO runs them")
        self._share_extractor = bool(pk.pop("share_features_extractor", False))
        pk.setdefault("activation_fn", "relu")                        # MTDPolicy's default activation IS ReLU (td_policies.py:297)
        pk = checkpoint.policy_kwargs_from_reference(pk, self.obs_keys)
        act, ext_act = self._activations(pk)
        self._extractor = pk.get("extractor", {k: [128, 64] for k in self.obs_keys})
        self._ext_keys = list(self._extractor.keys())
        arch = list(pk.get("pi", [64, 64]))
        if self._critic_arch is None:
            self._critic_arch = list(arch)
        pol = MlpPolicy({k: obs_width(obs[k]) for k in self.obs_keys}, self._extractor, arch, arch, self.device, seed=seed,
                        ortho_init=False, head_dims=(4, 4), log_std_param=False, activation=act, extractor_activation=ext_act)
        hidden = lambda trunk: [ly for ly in pol.layers if ly.dst.startswith(trunk + ":")]
        for a, b in zip(hidden("pi"), hidden("vf")):                  # log_latent_pi starts as a copy of latent_pi
            pol.weight(b).copy_(pol.weight(a))
            pol.bias(b).copy_(pol.bias(a))
        return pol

    # MTDPolicy takes any activation_fn (td_policies.py:297).  BPTT's two actors run ReLU, Tanh, ELU and LeakyReLU through every path of a
    # horizon: the activation is part of the generated chain class (visfly_amd/_jit.py) and of the layer tables the block-tile / per-layer
    # kernels read.  SHAC (its actor and its twin critic) still runs ReLU networks only
    any_activation = True

    def _activations(self, pk):
        """(trunk, extractor) VF_ACTIVATION_* of translated policy_kwargs; refuses what this trainer does not run"""
        if pk.get("vf_extractor"):
            raise NotImplementedError(f"{type(self).__name__}: separate pi / vf feature extractors (share_features_extractor=False of the "
                                      "actor-critic policy, pi_features_extractor_class / vf_features_extractor_class) are not implemented: "
                                      "this trainer's actor has no critic side; PPO runs such networks")
        if pk.get("layer_norm"):
            raise NotImplementedError(f"{type(self).__name__}: layer norm (ln / pi_ln / vf_ln, layer_norm={pk['layer_norm']}) is not implemented: "
                                      "the horizon kernels have no normalisation step; PPO runs networks with LayerNorm")
        # (native MlpPolicy arguments pass through the translation untouched: there `activation` may be spelt `activation_fn`)
        kinds = activation_kind(pk.get("activation", pk.get("activation_fn", 1))), activation_kind(pk.get("extractor_activation", 1))
        if not self.any_activation:
            self._relu_only(kinds)
        return kinds

    @staticmethod
    def _relu_only(kinds):
        """SHAC runs its horizons and its twin critic's update as ReLU networks (td_policies' own default, td_policies.py:297);
        Tanh / ELU / LeakyReLU actors: BPTT, PPO"""
        if tuple(kinds) != (1, 1):
            raise NotImplementedError("SHAC: activation_fn other than relu is not implemented (SHAC's actor and twin critic run as ReLU "
                                      "networks; BPTT and PPO take tanh / elu / leaky_relu)")

    def _head_fwd(self, mu, log_std, eps, action):
        """action = tanh(mu + eps exp(clamp(log_std))) -- Actor.action_log_prob's sample (SB3 squashed Gaussian)"""
        _lib.check(_lib.lib().vf_shac_head_fwd(_ptr(mu), _ptr(log_std), _ptr(eps), _ptr(action), mu.shape[0], LOG_STD_MIN,
                                               LOG_STD_MAX, _lib.current_stream(self.device)))

    def _make_policy(self, obs, policy_kwargs, seed):
        """the actor network: the reference's Actor when a td_policies policy was named (or by SHAC), else the MlpPolicy with a
        state-independent log_std"""
        if self.reference_actor:
            return self._make_reference_actor(obs, policy_kwargs, seed)
        pk = dict(policy_kwargs or {})
        pk.setdefault("activation_fn", "relu")             # (this actor is not a reference class: its default stays what it was)
        pk = checkpoint.policy_kwargs_from_reference(pk, self.obs_keys)
        act, ext_act = self._activations(pk)
        self.weight_decay = pk.get("weight_decay", self.weight_decay)
        return MlpPolicy({k: obs_width(obs[k]) for k in self.obs_keys},
                         pk.get("extractor", {k: [128, 64] for k in self.obs_keys}), pk.get("pi", [64, 64]),
                         pk.get("vf", [64, 64]), self.device, log_std_init=pk.get("log_std_init", -1.0), seed=seed,
                         ortho_init=pk.get("ortho_init", True), activation=act, extractor_activation=ext_act)

    def _update(self):
        """one horizon: roll out, back-propagate through simulator and policy, clip + Adam (BPTT.py:100-134)"""
        loss = self._grad_autograd() if self.use_autograd else self._grad_reverse_sweep()
        return self._apply(loss)

    def _grad_reverse_sweep_reference_actor(self):
        """BPTT.py:107-134 with the reference's actor: per step actor.action_log_prob(obs) (both trunks, clamped log_std, squashed
        reparameterised sample; the log-prob it also returns is discarded by the loop) -> env.step -> loss / discount recurrence
        (:123-124); reverse, t = H-1 .. 0: adjoint env step -> action head reverse (d mu, d log_std) -> both trunks + extractor
        -> gradient w.r.t. the observation of step t, which step t-1 returned.  Like the MlpPolicy sweep: the activations of every
        step stay in their slot, the weight gradient is reduced once over the rows of all H steps, and where the library has the
        kernels each half is ONE persistent launch (vf_bptt_rollout / vf_bptt_reverse, actor class (b)) that leaves what the
        launch-by-launch loop below leaves, bit for bit."""
        env, pol, keys = self.env, self.policy, self.obs_keys
        L, st, dev = _lib.lib(), _lib.current_stream(self.device), self.device
        N, H, defer, disc, loss_vec, eps, t0, scale = self._open_sweep(self.H, two_heads=True)
        f = dict(dtype=th.float32, device=dev)
        acts, drews = th.empty((H, N, 4), **f), th.empty((H, N), **f)
        fused = False
        if defer and self.fused_rollout:
            fused = env.rollout_policy(pol, keys, eps, acts, drews, loss_vec, disc, float(self.gamma), scale)
        if fused:
            self._last_rollout = dict(action=acts, done=env._tape_done[t0:t0 + H])
        else:
            self._last_rollout = dict(action=acts, reward=th.empty((H, N), **f), done=th.empty((H, N), dtype=th.bool, device=dev))
            obs = env.get_observation()
        for t in range(0 if not fused else H, H):
            o = policy_rows(obs, keys)
            mu, ls = pol.forward(o, slot=t)                                            # actor.action_log_prob(obs) :113
            self._head_fwd(mu, ls, eps[t], acts[t])                                    # tanh output: the clip of :114-116 is the identity
            obs, reward, done, _ = env._step_no_grad(acts[t], False, record=True, borrow=True)      # :119
            self._last_rollout["reward"][t].copy_(reward)
            self._last_rollout["done"][t].copy_(done)
            _lib.check(L.vf_bptt_accumulate(_ptr(reward), done.data_ptr(), _ptr(disc), _ptr(loss_vec), _ptr(drews[t]),
                                            float(self.gamma), scale, N, st))                      # :123-124
        self._reverse_two_heads(t0, eps, acts, drews, fused)
        self._horizon = dict(actions=acts, loss_vec=loss_vec)       # per-agent rows of the last horizon (tests, diagnostics)
        return loss_vec.mean() / self.world

    def _open_sweep(self, noise_rows, two_heads):
        """what every reverse sweep starts with -> (N, H, defer, disc, loss_vec, eps, t0, scale): policy.grad zeroed, the activation slots
        of the H steps reserved, the weight gradient deferred to one reduction per horizon where the network has the data-gradient kernel
        (decided at the first update), discount / loss rows, the exploration noise of the horizon in one draw ((noise_rows, N, 4): H rows,
        SHAC 2 H; the two-head sweeps take the tests' ``_eps_override`` instead), the tape position of step 0 and the loss scale
        1 / global agent count"""
        pol, N, H, dev = self.policy, self.env.num_envs, self.H, self.device
        pol.grad.zero_()
        # reference-default policy shapes: the weight gradient is reduced ONCE per horizon over the rows of all H
        # steps (their activations / masked gradients are stored back to back), the per-step reverse pass is the
        # register-chained data-gradient kernel only
        pol.reserve_slots(N, H)          # no-op while the slots exist (they are dropped if many other batch sizes pass through)
        if self._defer_wgrad is None:
            self._defer_wgrad = pol.backward_data_supported(N, both_heads=True) if two_heads else pol.backward_data_supported(N)
        disc, loss_vec = th.ones(N, dtype=th.float32, device=dev), th.zeros(N, dtype=th.float32, device=dev)
        eps = self._eps_override if two_heads and self._eps_override is not None else self._noise(noise_rows, N)
        assert eps.shape == (noise_rows, N, 4)
        return N, H, self._defer_wgrad, disc, loss_vec, eps, self.env._tape_t, 1.0 / (N * self.world)

    def _reverse_two_heads(self, t0, eps_a, actions, drews, fused):
        """reverse half of a horizon of the reference's actor (BPTT and SHAC), t = H-1 .. 0: adjoint env step -> action head reverse
        (d mu, d log_std) -> both trunks + extractor -> gradient w.r.t. the observation of step t; ONE persistent launch after a fused
        forward half (``fused``) where the library has the kernel.  Returns once policy.grad holds the horizon's weight gradient"""
        env, pol, N, H, defer = self.env, self.policy, self.env.num_envs, self.H, self._defer_wgrad
        L, st = _lib.lib(), _lib.current_stream(self.device)
        ls_rows = pol._slot_blocks[N][1]["value"]                                      # (slots, N, 4): slot t's log_std head
        g_obs = None
        d_mus, d_lss = th.empty((H, N, 4), device=self.device), th.empty((H, N, 4), device=self.device)
        rev = False
        if fused and self.fused_reverse:
            rev = env.reverse_policy(pol, H, eps_a, actions, drews, d_mus, None, d_log_stds=d_lss)
        for t in reversed(range(0 if not rev else H, H)):
            d_action = env.backward_step(t0 + t, g_obs, drews[t])
            _lib.check(L.vf_shac_head_bwd(_ptr(d_action), _ptr(actions[t]), _ptr(ls_rows[t]), _ptr(eps_a[t]), _ptr(d_mus[t]),
                                          _ptr(d_lss[t]), N, LOG_STD_MIN, LOG_STD_MAX, st))
            if defer:
                d_in = pol.backward_data(d_mus[t], t, d_value=d_lss[t])
            else:
                d_in = pol.backward(d_mus[t], d_lss[t], None, accumulate=True, need_input_grad=t > 0, slot=t)
            g_obs = d_in.get("state") if t > 0 else None
        if defer:
            pol.weight_grad_slots(N, H, d_mus, accumulate=True, d_value_all=d_lss)

    def _grad_reverse_sweep(self):
        """explicit reverse sweep: no autograd tape.  Forward: policy (activations of every step stay resident in their
        own slot) -> reparameterised action -> fused env step (state checkpoint on the tape) -> loss / discount
        bookkeeping, one launch each.  Reverse, t = H-1 .. 0: adjoint env step -> action head -> whole-network backward
        (parameter gradients accumulate in MFMA partials + fold) -> gradient w.r.t. the observation of step t, which
        is what step t-1 returned.  dLoss/d reward_t = -disc_t / N is known in the forward pass (:123)."""
        if self.reference_actor:
            return self._grad_reverse_sweep_reference_actor()
        env, pol = self.env, self.policy
        L, st, dev = _lib.lib(), _lib.current_stream(self.device), self.device
        N, H, defer, disc, loss_vec, epss, t0, scale = self._open_sweep(self.H, two_heads=False)
        g_ls = th.zeros((N, 4), device=dev)
        log_std = pol.log_std
        obs = env.get_observation()
        # per-horizon buffers in one allocation each
        acts, drews = th.empty((H, N, 4), device=dev), th.empty((H, N), device=dev)
        ckpt_done = False
        fused = False
        if defer and self.fused_rollout and pol._act_fused is not False:
            # the whole forward half as one persistent launch (vf_bptt_rollout): same kernels' arithmetic, same buffers
            fused = env.rollout_policy(pol, self.obs_keys, epss, acts, drews, loss_vec, disc, float(self.gamma), scale)
        for t in range(0 if not fused else H, H):
            action = acts[t]
            o = policy_rows(obs, self.obs_keys)
            if not (defer and pol.forward_act(o, epss[t], action, slot=t)):      # action head fused into the forward launch
                mean, _ = pol.forward(o, slot=t, need_value=False)
                _lib.check(L.vf_reparam_fwd(_ptr(mean), _ptr(log_std), _ptr(epss[t]), _ptr(action), N, st))
            obs, reward, done, _ = env._step_no_grad(action, False, record=True, borrow=True,   # acts[t] outlives the reverse sweep
                                                     prefilled=ckpt_done)
            # loss / discount bookkeeping, fused with the state checkpoint of step t + 1 (one launch instead of two)
            ckpt_done = t + 1 < H and env._tape_t < env._tape.shape[0]
            if ckpt_done:
                _lib.check(L.vf_bptt_accumulate_checkpoint(_ptr(reward), done.data_ptr(), _ptr(disc), _ptr(loss_vec), _ptr(drews[t]),
                                                           float(self.gamma), scale, N, _ptr(env._slab),
                                                           _ptr(env._tape[env._tape_t]), env._slab.numel(), st))
            else:
                _lib.check(L.vf_bptt_accumulate(_ptr(reward), done.data_ptr(), _ptr(disc), _ptr(loss_vec), _ptr(drews[t]),
                                                float(self.gamma), scale, N, st))
        g_obs = None
        d_means = th.empty((H, N, 4), device=dev)
        g_ls_rows = th.zeros((H, N, 4), device=dev) if defer else None     # log_std gradient terms, one row per (step, agent)
        rev = False
        if fused and self.fused_reverse:
            # the whole reverse half as one persistent launch (vf_bptt_reverse)
            rev = env.reverse_policy(pol, H, epss, acts, drews, d_means, g_ls_rows)
        for t in reversed(range(0 if not rev else H, H)):
            d_action = env.backward_step(t0 + t, g_obs, drews[t])
            d_mean = d_means[t]
            if defer:       # action head's reverse + reverse chain in one launch (step 0's observation gradient is unused)
                d_in = pol.backward_data_act(d_action, acts[t], epss[t], g_ls_rows[t], d_mean, slot=t)
            else:
                _lib.check(L.vf_reparam_bwd(_ptr(d_action), _ptr(acts[t]), _ptr(log_std), _ptr(epss[t]), _ptr(d_mean), _ptr(g_ls), N, st))
                d_in = pol.backward(d_mean, None, None, accumulate=True, need_input_grad=t > 0, slot=t)
            g_obs = d_in.get("state") if t > 0 else None
        if defer:
            pol.weight_grad_slots(N, H, d_means, accumulate=True)
        pol.grad[pol.log_std_off:] = g_ls_rows.sum(dim=(0, 1)) if defer else g_ls.sum(dim=0)
        self._horizon = dict(actions=acts, loss_vec=loss_vec)       # per-agent rows of the last horizon (tests, diagnostics)
        return loss_vec.mean() / self.world

    def _grad_autograd(self):
        """the same gradient with torch.autograd as the scheduler (two custom Functions wrap the kernels); kept as the
        cross-check of the reverse sweep and as the template for dropping in an arbitrary torch policy"""
        env, pol, N = self.env, self.policy, self.env.num_envs
        if self.reference_actor:
            raise NotImplementedError("use_autograd=True drives the one-head MlpPolicy actor (log_std parameter); the reference's "
                                      "two-head actor runs on the reverse sweep only")
        pol.grad.zero_()
        log_std = pol.log_std.detach().clone().requires_grad_(True)
        anchor = th.zeros(1, device=self.device, requires_grad=True)
        disc = th.ones(N, device=self.device)
        loss_vec = th.zeros(N, device=self.device)
        obs = env.get_observation()
        epss = self._noise(self.H, N)     # same draw as the reverse sweep
        for t in range(self.H):
            gate = policy_rows(obs, [k for k in self.obs_keys if k in INDEX_OBS_KEYS])      # (the index column: no graph; "state" keeps its own)
            mean = PolicyFunction.apply(pol, self.obs_keys, anchor, *[gate.get(k, obs[k]) for k in self.obs_keys])
            action = th.tanh(mean + log_std.exp() * epss[t])     # reparameterised squashed Gaussian (td_policies Actor)
            obs, reward, done, _ = env.step(action)
            loss_vec = loss_vec + -1 * reward * disc          # :123
            disc = disc * self.gamma * ~done + done           # :124
        loss = loss_vec.mean() / self.world
        loss.backward()
        pol.grad[pol.log_std_off:] = log_std.grad
        return loss.detach()

    def _apply(self, loss):
        env, pol, N = self.env, self.policy, self.env.num_envs
        parallel.allreduce_sum_(pol.grad)
        self._opt_step += 1
        pol.adam_step(self.exp_avg, self.exp_avg_sq, self._sumsq, self._scratch, self.lr, self.betas, self.adam_eps, self.weight_decay,
                      self.max_grad_norm, self._opt_step)
        env.detach()                                         # :134
        self.num_timesteps += self.H * N * self.world
        return loss.detach() * self.world

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = False):
        """SB3-style predict (utils/evaluate.py:94): -> (action, None); deterministic: a = tanh(mean)"""
        N = obs[self.obs_keys[0]].shape[0]
        # (reference actor -- shac.py:334-343 / MTDPolicy.predict: the second head is the state-dependent log_std)
        mean, ls = self.policy.forward(policy_rows(obs, self.obs_keys), save_activations=False, slot=self.H + 1,
                                       need_value=self.reference_actor)
        if deterministic:
            return th.tanh(mean), None
        eps = self._noise(1, N)[0]
        if not self.reference_actor:
            return th.tanh(mean + self.policy.log_std.exp() * eps), None
        action = th.empty((N, 4), device=self.device)
        self._head_fwd(mean, ls.contiguous(), eps, action)
        return action, None

    # ---- checkpoints ----
    # MlpPolicy actor: the SB3-layout zip of checkpoint.py.  Reference actor (and SHAC): the reference pickles the whole SB3 policy
    # object (shac.py:328-332), which cannot exist here; a plain torch archive of the flat parameter buffers, the Adam moments and
    # step counters, the generator state and the spec the networks are rebuilt from.
    def _state(self):
        return {"actor": self.policy.flat.cpu(), "exp_avg": self.exp_avg.cpu(), "exp_avg_sq": self.exp_avg_sq.cpu(),
                "opt_step": int(self._opt_step), "num_timesteps": int(self.num_timesteps), "rng": self._gen.get_state().cpu(),
                "noise_step": int(self._noise_step),
                "spec": dict(extractor=self._extractor, pi=self.policy.spec["pi"], qf=self._critic_arch, horizon=self.H,
                             gamma=self.gamma, learning_rate=self.lr, algo=type(self).__name__, **checkpoint.activation_spec(self.policy),
                             share_features_extractor=self._share_extractor)}

    def _load_state(self, d, load_optimizer=True):
        checkpoint.check_activations(self.policy, d.get("spec"))
        assert d["actor"].numel() == self.policy.flat.numel(), "actor: the archive holds a different network (pass the same policy_kwargs, or use load())"
        self.policy.flat.copy_(d["actor"])
        self.policy.mark_updated()
        if load_optimizer and "exp_avg" in d:
            self.exp_avg.copy_(d["exp_avg"])
            self.exp_avg_sq.copy_(d["exp_avg_sq"])
            self._opt_step, self.num_timesteps = int(d["opt_step"]), int(d.get("num_timesteps", 0))
            self._gen.set_state(d["rng"])
            self._noise_step = int(d.get("noise_step", 0))

    def save(self, path: str):
        if not self.reference_actor:
            return checkpoint.save(self, path)
        th.save(self._state(), _pth(path))

    def set_parameters(self, path: str, load_optimizer: bool = True):
        if not self.reference_actor:
            return checkpoint.load_into(self, path, load_optimizer)
        self._load_state(th.load(_pth(path), map_location="cpu"), load_optimizer)
        return self

    @staticmethod
    def _policy_kwargs_from_spec(spec):
        """the stored network shapes as SB3-style policy_kwargs (what _make_reference_actor parses)"""
        return dict(features_extractor_class="StateGateExtractor" if "gate" in spec["extractor"] else
                    "StateTargetExtractor" if len(spec["extractor"]) > 1 else "StateExtractor",
                    features_extractor_kwargs={"net_arch": {k: {"layer": list(v)} for k, v in spec["extractor"].items()},
                                               "activation_fn": spec.get("extractor_activation", "relu")},
                    net_arch=dict(pi=list(spec["pi"]), qf=list(spec["qf"])), activation_fn=spec.get("activation", "relu"),
                    share_features_extractor=bool(spec.get("share_features_extractor", False)))

    @classmethod
    def load(cls, path: str, env, **kwargs):
        if path.endswith(".pth") or (not path.endswith(".zip") and os.path.exists(path + ".pth")):
            d = th.load(_pth(path), map_location="cpu")
            spec, load_opt = d["spec"], kwargs.pop("load_optimizer", True)
            kwargs.setdefault("policy_kwargs", cls._policy_kwargs_from_spec(spec))
            kwargs.setdefault("horizon", spec["horizon"])
            # the hyper-parameters the archive was trained with (a resumed run silently trained with the constructor's
            # defaults next to the restored Adam moments); an explicit keyword argument still wins
            import inspect
            accepted = set(inspect.signature(cls.__init__).parameters)     # (BPTT.load on an archive SHAC wrote: tau / gradient_steps / lamda are not BPTT's)
            for k in ("gamma", "learning_rate", "tau", "gradient_steps", "lamda"):
                if k in spec and k in accepted:
                    kwargs.setdefault(k, spec[k])
            if cls is BPTT:
                kwargs.setdefault("policy", "MultiInputPolicy")
            algo = cls(env, **kwargs)
            algo._load_state(d, load_opt)
            return algo
        return checkpoint.load_into(cls(env, **checkpoint.ctor_kwargs_from_archive(path, kwargs)), path)

    def learn(self, total_timesteps: int, log_interval: Optional[int] = None, eval_env=None):
        """``eval_env``: every ``dump_step`` timesteps (BPTT.py:137,174) one deterministic episode per agent of that env
        (visfly_amd.evaluate.evaluate_policy) -> logs["rollout/ep_rew_mean" | "rollout/ep_len_mean" | "rollout/success_rate"] by the
        reference's 100-episode window of this call, logs["eval/..."] over the episodes of the last evaluation (all ranks).  The
        evaluation draws no noise and leaves the training env, its tape and every generator alone; without ``eval_env`` nothing changes"""
        t0, start, it = time.time(), self.num_timesteps, 0
        sched = None
        if eval_env is not None:
            from .evaluate import EvalSchedule
            sched = self._eval_schedule = EvalSchedule(self, eval_env, self.dump_step)
        while self.num_timesteps - start < total_timesteps:
            before = self.num_timesteps - start
            loss = self._update()
            if sched is not None:
                sched.after_update(before, self.num_timesteps - start, self.logs)
            it += 1
            if log_interval and it % log_interval == 0:
                self.logs["train/actor_loss"] = float(loss)
                print(f"[bptt] it {it} steps {self.num_timesteps} actor_loss {self.logs['train/actor_loss']:.4f}")
        th.cuda.synchronize(self.device)
        self.logs["train/actor_loss"] = float(loss)
        self.logs["time/fps"] = (self.num_timesteps - start) / max(time.time() - t0, 1e-9)
        return self.policy
