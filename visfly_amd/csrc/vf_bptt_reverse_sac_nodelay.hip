// vf_bptt_reverse_sac_nodelay.hip -- k_bptt_reverse for the reference's own actor over one observation (NetSacHover) for dynamics
// WITHOUT the motor lag (envs/base/dynamics.py:534-554)
#include "vf_bptt_reverse_kernel.hpp"

template struct vf::BpttReverseSet<vf::NetSacHover, false>;
