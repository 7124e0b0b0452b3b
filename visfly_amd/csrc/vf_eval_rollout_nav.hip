// vf_eval_rollout_nav.hip -- k_eval_rollout for the state + target actor-critic class (NetNav / NetNavPi), all four action types; scheme and the
// one-observation class: vf_eval_rollout.hip
#include "vf_eval_rollout_kernel.hpp"

namespace vf {
template EvalRolloutFn Builtin<NetNav, NetNavPi>::eval_rollout;
}  // namespace vf
