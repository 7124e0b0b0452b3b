// vf_eval_rollout.hip -- deterministic evaluation episodes as ONE persistent launch (gfx950).
//
// The reference evaluates a policy with the closed loop a = tanh(mean(obs)) -> eval_env.step(a, is_test=True) until every agent has
// finished one episode (utils/algorithms/BPTT.py:138-156, shac.py:284-300, utils/evaluate.py:79-129): done agents are not re-spawned,
// `done` is sticky, and an agent's episode is what collect_info reported at the FIRST step that set its `done`.  Launch by launch that is
// max_episode_steps x (forward + head + env step + latch).  Here, as in vf_ppo_rollout.hip, a wave owns its agents for the whole
// evaluation:
//   * ROWS = 32 or 16 agents per wave -- the SAME choice vf_mlp_forward makes for N rows with both heads (chain16_ok), so the means are the
//     per-step path's to the bit; lanes ROWS..63 replicate lane & (ROWS - 1) outside the chain;
//   * the mean never leaves registers: tanhf, delay-ring exchange, control interval, env epilogue with auto_reset = 0; the next observation
//     goes through the wave's LDS tile (and to one (N,OW) scratch row block, overwritten every step);
//   * the owner lane copies the epilogue's episode outputs to the evaluation outputs at the first `done` (the env's own outputs keep being
//     overwritten afterwards: the latch cannot be done after the launch);
//   * a wave leaves the step loop once all of its agents are latched.  Its agents then stand where their last step left them, not where
//     max_episode_steps steps would have: the env needs a reset afterwards (on either path: every agent is done).
// The launch-by-launch loop's pieces are here too: vf_eval_action (the same tanhf) and vf_eval_latch.
#include "vf_chain_plugin.hpp"
#include "vf_eval_rollout_kernel.hpp"

namespace vf {

// the one-observation actor-critic class (PPO; the one-head BPTT actor); the state + target class: vf_eval_rollout_nav.hip; the SAC-style
// Actor's instances: vf_eval_rollout_sac.hip
template EvalRolloutFn Builtin<NetHover, NetHoverPi>::eval_rollout;

__global__ __launch_bounds__(kBlock) void k_eval_action(const float* __restrict__ mean, float* __restrict__ action, int n)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n) action[j] = tanhf(mean[j]);
}

// one thread per agent: the first step that sets `done` copies the env's episode outputs of that step
__global__ __launch_bounds__(kBlock) void k_eval_latch(const unsigned char* __restrict__ done, const float* __restrict__ ep_return,
                                                       const int* __restrict__ ep_length, const unsigned char* __restrict__ ep_flags,
                                                       const float* __restrict__ terminal_obs, unsigned char* __restrict__ latched,
                                                       float* __restrict__ out_return, int* __restrict__ out_length,
                                                       unsigned char* __restrict__ out_flags, float* __restrict__ out_terminal, int N, int OW)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N || !done[i] || latched[i]) return;
    latched[i] = 1;
    out_return[i] = ep_return[i];
    out_length[i] = ep_length[i];
    out_flags[i] = ep_flags[i];
    if (out_terminal)
        for (int k = 0; k < OW; ++k) out_terminal[(size_t)i * OW + k] = terminal_obs[(size_t)i * OW + k];
}

}  // namespace vf

extern "C" int vf_eval_rollout(vf_env* h, const vf_mlp_desc* desc, const float* params, const float* packed, const vf_eval_rollout_args* a,
                               vf_stream_t stream)
{
    if (!h || !desc || !params || !packed || !a || !a->out || !a->obs_state || !a->obs_scratch || !a->ep_return || !a->ep_length ||
        !a->ep_flags || a->T_max <= 0 || a->w1 < 0 || (a->w1 > 0 && !a->obs_second))
        return vf::fail(VF_EINVAL, "vf_eval_rollout: bad argument");
    const vf_env_out* out = a->out;
    if (!out->reward || !out->done || !out->ep_return || !out->ep_length || !out->ep_flags || !out->terminal_obs)
        return vf::fail(VF_EINVAL, "vf_eval_rollout: out needs reward / done scratch and the episode outputs");
    for (int l = 0; l < desc->n_layers; ++l)
        if (desc->layer[l].save) return vf::fail(VF_EINVAL, "vf_eval_rollout: the layer table must not keep activation copies (layer %d has a save pointer)", l);
    if (!h->dyn.S) return vf::fail(VF_ESTATE, "vf_eval_rollout: vf_env_bind has not been called");
    if (h->dyn.wind) return vf::fail(VF_EUNSUPPORTED, "vf_eval_rollout: per-agent wind rows are set");
    if (h->n_obst > 0) return vf::fail(VF_EUNSUPPORTED, "vf_eval_rollout: the handle has an obstacle table (vf_env_set_obstacles): step launch by launch");
    const int N = h->dyn.N, T = a->T_max;
    const bool race2 = h->cfg.kind == VF_ENV_RACING && h->cfg.obs_mode == VF_OBS_RACE2;      // RacingEnv2: 16 gate-relative columns
    const int OW = race2 ? 16 : 13;
    if (desc->in_dim[0] != OW)
        return vf::fail(VF_EUNSUPPORTED, "vf_eval_rollout: the first observation must be the %d-wide state row", OW);
    vf::EnvArgs ge{vf::DynArgs{N, h->dyn.G, h->dyn.g_drag, h->dyn.S, nullptr, nullptr, vf::ring_head(&h->dyn), nullptr, h->dyn.vel_strided},
                   *out, h->g_race, 0};      // auto_reset = 0: is_test
    ge.out.done_list = ge.out.done_count = nullptr;
    ge.out.obs = a->obs_scratch;
    // a racing env's second observation is the gate column: the launch takes row 0 from obs_second and keeps the index in a register
    const bool gate = h->cfg.kind == VF_ENV_RACING && a->w1 == 1;
    vf::ChainArgs gc{*desc, params, packed, vf::ChainIo{{a->obs_state, gate ? nullptr : a->obs_second}, nullptr, nullptr}, N, nullptr, nullptr,
                     nullptr, {nullptr, nullptr}};
    vf::EvalRollArgs r{T, N, a->obs_state, gate ? a->obs_second : nullptr, a->ep_return, a->ep_length, a->ep_flags, a->terminal_rows};
    const int rc = vf::chain_serve("vf_eval_rollout", true, &vf::ChainPlugin::eval_rollout, desc, params, race2 ? vf::VF_ENV_RACING2 : h->cfg.kind,
                                   &h->dyn.cfg, a->obs_second != nullptr, h->dyn.d_cfg, h->d_cfg, &ge, &gc, &r, N, vf::as_stream(stream));
    if (rc < 0) return rc;
    if (rc == 0)
        return vf::fail(VF_EUNSUPPORTED, "vf_eval_rollout: no persistent evaluation for this network class / env kind / dynamics configuration "
                                         "(built in: the [128, 64] x [64, 64] actor-critic -- thrust / bodyrate / velocity / position -- and SAC-style Actor "
                                         "-- thrust / bodyrate --, Hover / Navigation / Racing, Euler / RK4; generated classes: through their evaluation plugin)");
    h->dyn.tick += T;
    h->stale_all = 1;
    return VF_OK;
}

extern "C" int vf_eval_latch(const uint8_t* done, const float* ep_return, const int32_t* ep_length, const uint8_t* ep_flags,
                             const float* terminal_obs, uint8_t* latched, float* out_return, int32_t* out_length, uint8_t* out_flags,
                             float* out_terminal, int32_t N, int32_t OW, vf_stream_t stream)
{
    if (!done || !ep_return || !ep_length || !ep_flags || !latched || !out_return || !out_length || !out_flags || N <= 0 ||
        (out_terminal && (!terminal_obs || OW <= 0)))
        return vf::fail(VF_EINVAL, "vf_eval_latch: bad argument");
    hipLaunchKernelGGL(vf::k_eval_latch, dim3(vf::blocks_for(N)), dim3(vf::kBlock), 0, vf::as_stream(stream), done, ep_return, ep_length, ep_flags,
                       terminal_obs, latched, out_return, out_length, out_flags, out_terminal, N, OW);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

extern "C" int vf_eval_action(const float* mean, float* action, int32_t N, vf_stream_t stream)
{
    if (!mean || !action || N <= 0) return vf::fail(VF_EINVAL, "vf_eval_action: bad argument");
    hipLaunchKernelGGL(vf::k_eval_action, dim3(vf::blocks_for(4 * N)), dim3(vf::kBlock), 0, vf::as_stream(stream), mean, action, 4 * N);
    VF_HIP(hipGetLastError());
    return VF_OK;
}
