// vf_bptt_reverse_hover_nodelay.hip -- k_bptt_reverse of the policy trunk over one observation (NetHover) for dynamics WITHOUT the motor
// lag (ctrl_delay = False, envs/base/dynamics.py:534-554): the direct form of the interval's adjoint
#include "vf_bptt_reverse_kernel.hpp"

template struct vf::BpttReverseSet<vf::NetHover, false>;
