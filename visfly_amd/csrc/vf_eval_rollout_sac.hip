// vf_eval_rollout_sac.hip -- k_eval_rollout for the reference's own actor (NetSacHover / NetSacNav; utils/policies/td_policies.py:146-252:
// what BPTT(policy=...) and SHAC train): both trunks of the chain run per step as in the per-step forward, only the mu head is read.
#include "vf_eval_rollout_kernel.hpp"

namespace vf {
template EvalRolloutFn Builtin<NetSacHover>::eval_rollout;
template EvalRolloutFn Builtin<NetSacNav>::eval_rollout;
}  // namespace vf
