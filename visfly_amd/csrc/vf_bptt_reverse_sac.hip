// vf_bptt_reverse_sac.hip -- k_bptt_reverse for the reference's own actor over one observation (NetSacHover; utils/policies/td_policies.py:146-252)
// with the motor lag: per step the adjoint of the env step, then k_shac_head_bwd's arithmetic in the reverse chain's head prologue
// (d_mu = d_a (1 - a^2), d_log_std = d_mu eps exp(log_std) inside the clamp interval, from the log_std rows the forward launch saved) and
// BOTH trunks of the reverse chain down to the observation gradient.
#include "vf_bptt_reverse_kernel.hpp"

template struct vf::BpttReverseSet<vf::NetSacHover, true>;
