// vf_mlp_chain_reverse.hip -- the reverse chain (data gradients) of every built-in class (vf_chain_plugin.hpp: Builtin::backward):
// k_mlp_backward_chain <BwdProg<Net, pi, vf, IG>> from the head gradients, the masked layer gradients left for k_mlp_wgrad.  Variants:
//   both trunks, no observation gradient     the PPO update, SHAC's actor and twin critic (dQ1 / dQ2)
//   with observation gradient                what a BPTT sweep runs per step: the policy trunk of an actor-critic (+ the action head's
//                                            reverse, rp), both trunks of the SAC-style Actor (d_mu / d_log_std); 16 rows per wave
//                                            for small row counts (bwd16_ok)
// A translation unit of its own so that its instances compile next to the forward's (vf_mlp_chain.hip).
#include "vf_chain_plugin.hpp"

namespace vf {

// packed == nullptr: capability query only
template <class Net, class NetPi>
int Builtin<Net, NetPi>::backward(const vf_mlp_bwd_desc* d, const float* packed, int M, hipStream_t st, const ReparamBwd* rpp)
{
    constexpr bool sac = Net::HV == 4;      // td_policies.Actor: both heads carry gradient
    if ((Net::HM != 4 || Net::HV != 1) && rpp) return 0;      // (the action head's reverse: the actor-critic classes)
    const ReparamBwd rp = rpp ? *rpp : ReparamBwd{};
    if (bwd_chain_matches<Net, true, true, false>(*d)) return packed ? bwd_chain_launch<Net, true, true, false>(*d, packed, M, st, rp) : 1;
    if constexpr (!Net::PASS) {
        if (bwd_chain_matches<Net, true, sac, true>(*d)) return packed ? bwd_chain_launch<Net, true, sac, true>(*d, packed, M, st, rp) : 1;
    }
    return 0;
}
template ChainBackwardFn Builtin<NetHover, NetHoverPi>::backward;
template ChainBackwardFn Builtin<NetNav, NetNavPi>::backward;
template ChainBackwardFn Builtin<NetSacHover>::backward;
template ChainBackwardFn Builtin<NetSacNav>::backward;
template ChainBackwardFn Builtin<NetCriticHover>::backward;

}  // namespace vf
