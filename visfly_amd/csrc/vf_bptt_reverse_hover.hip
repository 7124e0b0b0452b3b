// vf_bptt_reverse_hover.hip -- k_bptt_reverse of the policy trunk over one observation (NetHover's reverse chain with observation gradient,
// state-independent log_std) with the motor lag: HoverEnv, NavigationEnv2, RacingEnv and RacingEnv2 (the kernel-side kinds of
// bptt_instance; RacingEnv2's 16-column observation's adjoint is race2_obs_bwd in front of the raw row's, vf_env_bwd_body.hpp).  The
// instance sets compile side by side, one translation unit each (vf_bptt_reverse_kernel.hpp).
#include "vf_bptt_reverse_kernel.hpp"

template struct vf::BpttReverseSet<vf::NetHover, true>;
