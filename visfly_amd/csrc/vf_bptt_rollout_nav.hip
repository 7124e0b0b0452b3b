// vf_bptt_rollout_nav.hip -- k_bptt_rollout of the state + target classes over NavigationEnv (NetNavPi: the policy trunk over
// StateTargetExtractor; NetSacNav: the reference's own actor over it), both forms of the interval
#include "vf_bptt_rollout_kernel.hpp"

template struct vf::BpttRolloutSet<vf::NetNavPi, true>;
template struct vf::BpttRolloutSet<vf::NetNavPi, false>;
template struct vf::BpttRolloutSet<vf::NetSacNav, true>;
template struct vf::BpttRolloutSet<vf::NetSacNav, false>;
