// vf_bptt_rollout_sac.hip -- k_bptt_rollout for the reference's own actor over one observation (NetSacHover; utils/policies/td_policies.py:146-252,
// what BPTT.learn / SHAC's roll-out call per step: utils/algorithms/BPTT.py:113, shac.py:219) with the motor lag: both trunks of the
// 16-row chain run per step -- latent_pi -> mu, log_latent_pi -> log_std -- and the action head is k_shac_head_fwd's arithmetic on the two
// heads still in registers, a = tanh(mu + eps exp(clamp(log_std, -10, 2))) (chain16_epilogue, HV == 4).  The log_std rows of every step
// are kept (the head's reverse reads them), like every layer's activations.
#include "vf_bptt_rollout_kernel.hpp"

template struct vf::BpttRolloutSet<vf::NetSacHover, true>;
