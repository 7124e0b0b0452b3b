// vf_bptt_reverse_nav.hip -- k_bptt_reverse of the state + target classes over NavigationEnv (NetNav's policy trunk over
// StateTargetExtractor; NetSacNav: the reference's own actor over it), both forms of the interval
#include "vf_bptt_reverse_kernel.hpp"

template struct vf::BpttReverseSet<vf::NetNav, true>;
template struct vf::BpttReverseSet<vf::NetNav, false>;
template struct vf::BpttReverseSet<vf::NetSacNav, true>;
template struct vf::BpttReverseSet<vf::NetSacNav, false>;
