// vf_ppo_rollout.hip -- PPO's collect_rollouts as ONE persistent launch (gfx950).
//
// SB3 OnPolicyAlgorithm.collect_rollouts (run by utils/algorithms/PPO.py:146) is the closed loop policy.forward(obs_t) ->
// distribution.sample / log_prob -> env.step -> RolloutBuffer.add, n_steps times.  Launch by launch that is, per control step
// at 32 768 agents: the register-chained forward (30 us), the head sampler (5 us), two observation copies (2 x 5 us), the env
// step (11 us) and the TimeLimit bookkeeping (4 us) -- 60 us, of which the launch boundaries and the cold first touches of
// every launch are a third (profiles/r03_ppo_kernel_stats.txt).  Here, as in vf_bptt_rollout.hip, a wave owns its agents for
// all n_steps:
//   * ROWS = 32 agents per wave with the 32-row chain (v_mfma_f32_32x32x2_f32) or 16 with the 16-row chain -- the SAME choice
//     vf_mlp_forward makes from the row count (chain16_ok), so heads, values, actions and log-probs are the per-step path's
//     to the bit.  Lanes ROWS..63 replicate lane & (ROWS - 1) outside the chain (k_bptt_rollout's construction);
//   * nothing of a step travels through memory: the accumulator lane that holds the heads of row m IS lane m (replicas take
//     them by ds_bpermute), the sampled action feeds the env step in registers, the reward / done of the epilogue feed the buffer
//     rows and the TimeLimit list, and the next forward reads its "state" row from the LDS tile the epilogue staged it through
//     on its way to RolloutBuffer.obs["state"][t + 1].  Global memory sees only the buffer rows, written once, never re-read.
#include "vf_ppo_rollout_builtin.hpp"

namespace vf {

// the one-observation class (the two-observation class: vf_ppo_rollout_nav.hip)
template PpoRolloutFn Builtin<NetHover, NetHoverPi>::ppo_rollout;

}  // namespace vf

extern "C" int vf_ppo_rollout(vf_env* h, const vf_mlp_desc* desc, const float* params, const float* packed, const vf_ppo_rollout_args* a,
                              vf_stream_t stream)
{
    if (!h || !desc || !params || !packed || !a || !a->out || !a->obs_state || !a->values || !a->actions || !a->log_probs || !a->rewards ||
        !a->episode_starts || !a->last_starts || !a->obs_final || !a->log_std || !a->cursor || !a->idx_list || !a->rows0 ||
        !a->stat || a->T <= 0 || a->w1 < 0 || (a->w1 > 0 && (!a->rows1 || !a->obs_target)))
        return vf::fail(VF_EINVAL, "vf_ppo_rollout: bad argument");
    const vf_env_out* out = a->out;
    if (!out->reward || !out->done || !out->ep_return || !out->ep_length || !out->ep_flags || !out->terminal_obs)
        return vf::fail(VF_EINVAL, "vf_ppo_rollout: out needs reward / done scratch and the episode outputs");
    for (int l = 0; l < desc->n_layers; ++l)
        if (desc->layer[l].save) return vf::fail(VF_EINVAL, "vf_ppo_rollout: the layer table must not keep activation copies (layer %d has a save pointer)", l);
    if (!h->dyn.S) return vf::fail(VF_ESTATE, "vf_ppo_rollout: vf_env_bind has not been called");
    if (h->dyn.wind) return vf::fail(VF_EUNSUPPORTED, "vf_ppo_rollout: per-agent wind rows are set");
    if (h->n_obst > 0) return vf::fail(VF_EUNSUPPORTED, "vf_ppo_rollout: the handle has an obstacle table (vf_env_set_obstacles): step launch by launch");
    // (observation / reward variants -- HoverEnv2, NavigationEnv2 -- are the epilogue's own: the rows it stages through the wave's
    // tile for the next forward are already in the env's obs_mode, the terminal rows too; r05)
    if ((reinterpret_cast<uintptr_t>(a->means) | reinterpret_cast<uintptr_t>(a->actions) | reinterpret_cast<uintptr_t>(a->stat)) & 15)
        return vf::fail(VF_EINVAL, "vf_ppo_rollout: means / actions / stat must be 16-byte aligned");
    const int N = h->dyn.N, T = a->T;
    const bool race2 = h->cfg.kind == VF_ENV_RACING && h->cfg.obs_mode == VF_OBS_RACE2;      // RacingEnv2: 16 gate-relative columns
    const int OW = race2 ? 16 : 13;
    // (a class padded to the same 16 input columns would match 13- and 16-wide rows alike: only the width the env kind's epilogue forms)
    if (desc->in_dim[0] != OW)
        return vf::fail(VF_EUNSUPPORTED, "vf_ppo_rollout: the first observation must be the %d-wide state row", OW);
    vf::EnvArgs ge{vf::DynArgs{N, h->dyn.G, h->dyn.g_drag, h->dyn.S, nullptr, nullptr, vf::ring_head(&h->dyn), nullptr, h->dyn.vel_strided},
                   *out, h->g_race, 1};
    ge.out.done_list = ge.out.done_count = nullptr;
    ge.out.obs = T > 1 ? a->obs_state + (size_t)N * OW : a->obs_final;
    vf::ChainArgs gc{*desc, params, packed, vf::ChainIo{{a->obs_state, a->obs_target}, a->means, a->values}, T * N, nullptr, nullptr, nullptr,
                     {nullptr, nullptr}};
    // a racing env's second observation is the gate column: its rows are written by the launch, obs_target_row is not read
    const bool gate = h->cfg.kind == VF_ENV_RACING && a->w1 == 1;
    if (a->w1 > 0 && !gate && !a->obs_target_row) return vf::fail(VF_EINVAL, "vf_ppo_rollout: obs_target_row is required with constant target rows");
    vf::PpoRollArgs r{T, N, reinterpret_cast<float4*>(a->actions), a->log_probs, a->rewards, a->episode_starts, a->last_starts,
                      a->obs_state, a->obs_final, a->log_std, a->noise_key, a->sample_step, a->obs_target_row, a->w1, a->capacity, a->cursor,
                      a->idx_list, a->rows0, a->rows1, a->stat,
                      // a racing env's second observation is the gate column (StateGateExtractor): obs_target = RolloutBuffer.obs["gate"],
                      // [T][N][1], row 0 the caller's, the later rows written by the launch
                      gate ? a->obs_target : nullptr};
    const int rc = vf::chain_serve("vf_ppo_rollout", true, &vf::ChainPlugin::ppo_rollout, desc, race2 ? vf::VF_ENV_RACING2 : h->cfg.kind, &h->dyn.cfg,
                                   a->obs_target != nullptr, h->dyn.d_cfg, h->d_cfg, &ge, &gc, &r, N, vf::as_stream(stream));
    if (rc < 0) return rc;
    if (rc == 0)
        return vf::fail(VF_EUNSUPPORTED, "vf_ppo_rollout: no persistent roll-out for this network class / env kind / dynamics "
                                         "configuration (built in: [128, 64] x [64, 64] actor-critic, Hover / Navigation / Racing, thrust / "
                                         "bodyrate / velocity / position, Euler / RK4; generated classes: through their roll-out plugin)");
    h->dyn.tick += T;
    h->stale_all = 1;       // agents re-spawned inside the launch: the prefetched copies' stale bits no longer cover them
    return VF_OK;
}

#ifdef VF_PPO_TRACE
extern "C" int vf_debug_ppo_trace(long long* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(vf::vf_ppo_trace), sizeof(long long) * 8, 0, hipMemcpyDeviceToHost);
}
#endif
