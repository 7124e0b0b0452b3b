// vf_bptt_rollout_sac_nodelay.hip -- k_bptt_rollout for the reference's own actor over one observation (NetSacHover) for dynamics
// WITHOUT the motor lag (envs/base/dynamics.py:534-554)
#include "vf_bptt_rollout_kernel.hpp"

template struct vf::BpttRolloutSet<vf::NetSacHover, false>;
