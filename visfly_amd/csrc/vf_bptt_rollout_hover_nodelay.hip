// vf_bptt_rollout_hover_nodelay.hip -- k_bptt_rollout of the policy trunk over one observation (NetHoverPi) for dynamics WITHOUT the
// motor lag (ctrl_delay = False: the rotors take their set points at once, envs/base/dynamics.py:534-554 -- not the reference's default)
#include "vf_bptt_rollout_kernel.hpp"

template struct vf::BpttRolloutSet<vf::NetHoverPi, false>;
