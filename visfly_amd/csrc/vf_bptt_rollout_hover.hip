// vf_bptt_rollout_hover.hip -- k_bptt_rollout of the policy trunk over one observation (NetHoverPi: the MlpPolicy classes over
// StateExtractor; state-independent log_std) with the motor lag: HoverEnv, NavigationEnv2, RacingEnv and RacingEnv2 (the kernel-side kinds
// of bptt_instance).  The instance sets compile side by side, one translation unit each (vf_bptt_rollout_kernel.hpp).
#include "vf_bptt_rollout_kernel.hpp"

template struct vf::BpttRolloutSet<vf::NetHoverPi, true>;
