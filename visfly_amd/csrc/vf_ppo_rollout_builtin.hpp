// vf_ppo_rollout_builtin.hpp -- Builtin<Net, NetPi>::ppo_rollout: the dispatch of PPO's persistent roll-out over the kernel instances of a built-in
// actor-critic class (scheme: vf_ppo_rollout.hip).  One translation unit per class instantiates it: vf_ppo_rollout.hip (NetHover),
// vf_ppo_rollout_nav.hip (NetNav) -- four action types x two integrators x two motor-lag forms x 16 / 32 rows per wave are ~100 s of hipcc each.
#pragma once
#include "vf_chain_plugin.hpp"
#include "vf_ppo_rollout_kernel.hpp"

namespace vf {

// the roll-out of an actor-critic class (vf_chain_plugin.hpp: Builtin::ppo_rollout): the one-observation class over the Hover and
// Navigation kinds (NavigationEnv2: the target is inside the "state" row) with either form of the interval, over RacingEnv's raw row and
// RacingEnv2's 16 gate-relative columns (kernel-side kind VF_ENV_RACING2) with the motor lag; the state + target class over the
// Navigation kind and, with the motor lag, over the racing kinds, where its second observation is the gate column (StateGateExtractor).  ROWS: the rows-per-wave choice of vf_mlp_forward for N rows (chain16_ok), so that the heads are the per-step path's
// to the bit
template <class Net, class NetPi>
int Builtin<Net, NetPi>::ppo_rollout(const vf_mlp_desc* d, int env_kind, const vf_dyn_cfg* c, int has_target, const vf_dyn_cfg* d_dyn,
                                     const vf_env_cfg* d_env, const void* env_args, const ChainArgs* gc, const void* roll_args, int N, hipStream_t st)
{
    if (!chain_matches<Net>(*d) || (Net::NB == 2 ? !has_target : has_target && env_kind != VF_ENV_HOVER)) return 0;
    const bool r16 = chain16_ok<Net>(*d, gc->params, N);
    const EnvArgs& ge = *static_cast<const EnvArgs*>(env_args);
    const PpoRollArgs& r = *static_cast<const PpoRollArgs*>(roll_args);
    // a two-observation class over a racing kind reads the gate column (1 wide, rows written by the launch)
    if (Net::NB == 2 && (env_kind == VF_ENV_RACING || env_kind == VF_ENV_RACING2) && (!r.gate_slots || d->in_dim[1] != 1)) return 0;
    // all four action types: the interval's controller is control_interval's own (thrust, bodyrate, the geometric controller of velocity /
    // position), evaluated once per control step in the lane that holds the agent
    return with_env_config<true>(env_kind, *c, [&](auto kind, auto act, auto integ, auto delay) -> int {
        constexpr int K = decltype(kind)::value, A = decltype(act)::value, I = decltype(integ)::value;
        constexpr bool D = decltype(delay)::value;
        if constexpr (Net::NB == 2 ? K == VF_ENV_NAV || (kind_is_racing(K) && D) : K == VF_ENV_HOVER || K == VF_ENV_NAV || D) {
            if (r16) hipLaunchKernelGGL((k_ppo_rollout<Net, 16, K, A, I, D>), dim3((N + 15) / 16), dim3(64), 0, st, d_dyn, d_env, ge, *gc, r);
            else hipLaunchKernelGGL((k_ppo_rollout<Net, 32, K, A, I, D>), dim3((N + 31) / 32), dim3(64), 0, st, d_dyn, d_env, ge, *gc, r);
            VF_HIP(hipGetLastError());
            return 1;
        } else {
            return 0;
        }
    });
}
extern template PpoRolloutFn Builtin<NetHover, NetHoverPi>::ppo_rollout;      // vf_ppo_rollout.hip
extern template PpoRolloutFn Builtin<NetNav, NetNavPi>::ppo_rollout;          // vf_ppo_rollout_nav.hip

}  // namespace vf
