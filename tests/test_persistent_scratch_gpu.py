"""The persistent launches of an env (visfly_amd/envs/persistent.py) write the rows of their last step -- reward, done, "state" -- into ONE
scratch per env (``_launch_scratch``): a BPTT roll-out that finds the scratch another launch left must compute what it computes on a fresh
env."""
import warnings

import pytest
import torch

from _golden import ENV_DYN, assert_bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_rollout_after_an_evaluation_launch_equals_the_rollout_alone():
    """HoverEnv, the built-in SAC-style Actor, a tape, N = 40 (two full 16-agent waves and a partial one), H = 3.  Env A runs
    evaluate_policy_launch first -- the scratch exists and holds that launch's rows --, then both envs are reset to the same explicit
    states and run rollout_policy: actions, d_reward rows, loss / discount rows, final observation and env._reward are bit-equal.
    The states hover at rest 1.25 .. 1.75 m above the floor and metres inside the [-30, 30] x [-30, 30] x [0, 8] box: in 3 steps of 20 ms
    an agent moves by centimetres, and the time limit is 8 steps, so no agent finishes (asserted from the tape's done rows), none is
    re-spawned, and the spawn streams -- the only state the evaluation on A may leave different after a reset to explicit states -- are
    never read."""
    from visfly_amd.bptt import BPTT
    from visfly_amd.envs import HoverEnv
    from visfly_amd.ppo import policy_rows
    N, H = 40, 3
    f = dict(dtype=torch.float32, device=DEV)
    make = lambda: HoverEnv(num_agent_per_scene=N, seed=3, dynamics_kwargs=dict(ENV_DYN), device=DEV, max_episode_steps=8, tensor_output=True,
                            requires_grad=True)
    env_a, env_b = make(), make()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        algo = BPTT(env_a, policy="MultiInputPolicy", horizon=H, learning_rate=1e-3, seed=7)
    pol, keys = algo.policy, algo.obs_keys
    assert not getattr(pol, "chain_jit", False)
    pol.reserve_slots(N, H)
    g = torch.Generator().manual_seed(11)
    c = env_a.envs.dynamics.constants
    fs = torch.zeros((N, 22))
    fs[:, 0:3] = torch.tensor([1.0, 0.0, 1.5]) + (torch.rand((N, 3), generator=g) - 0.5) * torch.tensor([1.0, 1.0, 0.5])
    fs[:, 3] = 1.0                                                      # identity attitude (wxyz), zero velocities
    fs[:, 13:17], fs[:, 17:21] = float(c["w_init"]), float(c["T_init"])
    eps = torch.randn((H, N, 4), generator=g).to(DEV)

    def rollout(env):
        env.set_requires_grad(True, horizon=H)
        env.reset(state=fs)
        env.clear_tape()                                                # the horizon is rows 0 .. H-1 of the tape
        out = dict(actions=torch.empty((H, N, 4), **f), d_reward=torch.empty((H, N), **f), loss=torch.zeros(N, **f), disc=torch.ones(N, **f))
        assert env.rollout_policy(pol, keys, eps, out["actions"], out["d_reward"], out["loss"], out["disc"], 0.99, 1.0 / N) is True
        torch.cuda.synchronize()
        assert not bool(env._tape_done[:H].any()), "an agent finished: the two envs' spawn streams are in play"
        assert env._reward is env._launch_scratch()["reward"]           # the shared scratch is the one this launch wrote
        out.update(final=env.get_observation()["state"], reward=env._reward)
        return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}

    env_a.reset()
    res = dict(ep_return=torch.zeros(N, **f), ep_length=torch.zeros(N, dtype=torch.int32, device=DEV), flags=torch.zeros(N, dtype=torch.uint8, device=DEV))
    assert env_a.evaluate_policy_launch(pol, keys, policy_rows(env_a.get_observation(), keys), res["ep_return"], res["ep_length"], res["flags"]) is True
    torch.cuda.synchronize()
    assert int(res["ep_length"].min()) >= 1                             # the evaluation ran: its last rows are in A's scratch
    scratch = env_a._launch_scratch()
    a = rollout(env_a)
    assert env_a._launch_scratch() is scratch
    b = rollout(env_b)
    for k in a:
        assert_bits_equal(a[k], b[k], k)
