// vf_ppo_rollout_nav.hip -- k_ppo_rollout for the state + target class (NetNav / NetNavPi: StateTargetExtractor on NavigationEnv, the gate column
// of StateGateExtractor on the racing kinds); scheme and the one-observation class: vf_ppo_rollout.hip
#include "vf_ppo_rollout_builtin.hpp"

namespace vf {
template PpoRolloutFn Builtin<NetNav, NetNavPi>::ppo_rollout;
}  // namespace vf
