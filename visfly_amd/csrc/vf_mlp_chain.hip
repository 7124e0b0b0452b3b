// Register-chained actor-critic forward for gfx950: one wave64 carries 32 rows through the WHOLE network, the
// activations never leave its registers.
//
// Every layer is computed transposed, Y^T = W X^T, with v_mfma_f32_32x32x2_f32:
//     A operand = weights   A[i = n][k]      lane = n + 32 kk
//     B operand = X^T       B[k][j = m]      lane = m + 32 kk
//     C / D     = Y^T       D[i = n][j = m]  lane (m, h = lane >> 5) holds n = 4 h + (r & 3) + 8 (r >> 2), r = 0..15
// A lane of the accumulator therefore holds 16 features of ITS OWN row m -- exactly what the B operand of the next
// layer wants from that lane, provided step s of the next layer reduces over k = kidx(s, h) = the feature register
// r = s % 16 of tile s / 16 holds: kidx = 32 (s / 16) + 8 ((s % 16) / 4) + 4 h + (s % 4).  The reduction order
// is free (a sum), so the weights are packed once in that order (k_mlp_pack_weights, image at vf_mlp_layer.wr_off:
// one contiguous 1 KiB block = the A fragments of four consecutive steps of one 32-feature output tile, one float4
// per lane) and the accumulator registers are fed back as B operands untouched: no LDS, no barriers, no
// inter-wave traffic.  Bias + ReLU run on the accumulator registers; the copies the backward needs are stored from
// them (float4 = 4 consecutive features of a row).
//
// The layer shapes must be compile-time (register arrays cannot be indexed at run time): the kernel is a template
// over the network class of the reference's policies (utils/policies/extractors.py:578-592,662-678;
// policies.py:18-49): NB extractor branches of two ReLU layers, concatenated, then policy / value trunks of two
// ReLU layers with a 4-wide / 1-wide head -- or, for its SAC-style Actor (td_policies.py:146-252), two 4-wide heads
// (mu, log_std), and for its twin ContinuousCritic (:82-143) the action appended to the features (a pass-through
// input tile, the layer table's frozen identity layer) and two 1-wide heads (Q1, Q2).  The classes form a table
// (vf_chain_plugin.hpp): this file holds the chain entry points, which ask it, and the forward member of every
// built-in class; vf_mlp_forward falls back to the LDS kernel (k_mlp_forward) when no class serves a call.
#include "vf_chain_plugin.hpp"

namespace vf {

// (the 32-row forward's device code -- chain_load .. chain_prologue -- lives in vf_mlp_chain.hpp: vf_ppo_rollout.hip runs it too)

// the built-in classes' forward: the actor-critic classes with and without the value trunk (out1 == null: NetPi) and with the action head
// (rp); the SAC-style Actor and the twin critic compute both heads, without action head.  in2: not an input of any built-in class
template <class Net, class NetPi>
int Builtin<Net, NetPi>::forward(const vf_mlp_desc* d, const float* params, const float* packed, const float* in0, const float* in1,
                                 const float* /*in2*/, float* out0, float* out1, int M, hipStream_t st, const ReparamFwd* rpp, int M_choice)
{
    constexpr bool two_inputs = Net::NB + Net::PASS == 2;
    if (two_inputs && !in1) return 0;
    const float* x1 = two_inputs ? in1 : nullptr;
    const ReparamFwd rp = rpp ? *rpp : ReparamFwd{};
    if constexpr (Net::HM == 4 && Net::HV == 1) {
        if (!out1) return chain_matches<NetPi>(*d) ? chain_launch<NetPi>(*d, params, packed, in0, x1, out0, out1, M, st, rp, nullptr, M_choice) : 0;
    } else {
        if (rpp || !out0 || !out1) return 0;
        if (Net::HV == 4 && ((reinterpret_cast<uintptr_t>(out0) | reinterpret_cast<uintptr_t>(out1)) & 15)) return 0;   // (float4 head rows)
    }
    return chain_matches<Net>(*d) ? chain_launch<Net>(*d, params, packed, in0, x1, out0, out1, M, st, rp, nullptr, M_choice) : 0;
}
template ChainForwardFn Builtin<NetHover, NetHoverPi>::forward;
template ChainForwardFn Builtin<NetNav, NetNavPi>::forward;
template ChainForwardFn Builtin<NetSacHover>::forward;
template ChainForwardFn Builtin<NetSacNav>::forward;
template ChainForwardFn Builtin<NetCriticHover>::forward;

// 1: launched, 0: no class of the table serves the call, < 0: error
int mlp_forward_chain_try(const vf_mlp_desc* d, const float* params, const float* packed, const float* in0, const float* in1,
                          float* out0, float* out1, int M, hipStream_t st, const ReparamFwd* rpp, const float* in2, int M_choice)
{
    const ReparamFwd rp = rpp ? *rpp : ReparamFwd{};
    if ((!out0 && !rp.action) || (reinterpret_cast<uintptr_t>(out0) & 15) || (reinterpret_cast<uintptr_t>(rp.action) & 15)) return 0;
    for (int i = 0; i < d->n_layers; ++i)
        if (d->layer[i].save && !rows_fit_u32(M, d->layer[i].save_ld)) return 0;
    return chain_serve("vf_mlp_forward", true, &ChainPlugin::forward, d, params, packed, in0, in1, in2, out0, out1, M, st, rpp, M_choice);
}

int mlp_backward_chain_try(const vf_mlp_bwd_desc* d, const float* packed, int M, hipStream_t st, const ReparamBwd* rpp)
{
    for (int l = 0; l < d->n_layers; ++l)
        if (!rows_fit_u32(M, d->layer[l].ld_dy)) return 0;
    return chain_serve("vf_mlp_backward_data", packed != nullptr, &ChainPlugin::backward, d, packed, M, st, rpp);
}

// fused PPO step (forward + loss + reverse chain): 1 launched, 0 no class serves it, < 0 error.
// part: ceil(M / 32) x kStats floats of loss-statistic partials
int ppo_update_chain_try(const vf_mlp_desc* d, const vf_mlp_bwd_desc* bd, const float* params, const float* packed, const float* in0,
                         const float* in1, const float* log_std, const float* action, const float* old_lp, const float* adv,
                         const float* ret, float* part, const vf_ppo_loss_cfg* cfg, int M, hipStream_t st)
{
    for (int i = 0; i < d->n_layers; ++i)
        if (d->layer[i].dst < VF_MLP_OUT0 && !d->layer[i].save) return 0;          // the weight gradients need every layer input
    for (int i = 0; i < d->n_layers; ++i)
        if (d->layer[i].save && !rows_fit_u32(M, d->layer[i].save_ld)) return 0;
    for (int l = 0; l < bd->n_layers; ++l)
        if (!rows_fit_u32(M, bd->layer[l].ld_dy)) return 0;
    if (cfg->row_index && (!cfg->obs_copy0 || (in1 && !cfg->obs_copy1)))
        return fail(VF_EINVAL, "vf_ppo_update: row_index needs obs_copy0 / obs_copy1 (the weight gradients read the observation rows in call order)");
    const ChainArgs g{*d, params, packed, ChainIo{{in0, in1}, nullptr, nullptr}, M, nullptr, nullptr, nullptr,
                      {cfg->row_index ? cfg->obs_copy0 : nullptr, cfg->row_index ? cfg->obs_copy1 : nullptr}};
    const BwdArgsChain gb{*bd, packed, M, nullptr, nullptr, nullptr, nullptr, nullptr};
    const PpoRowArgs pr{log_std, reinterpret_cast<const float4*>(action), old_lp, adv, ret, part, *cfg};
    return chain_serve("vf_ppo_update", true, &ChainPlugin::ppo_update, &g, &gb, &pr, M, st);
}

// fused critic step (forward + twin-Q loss + reverse chain): 1 launched, 0 no class serves it, < 0 error.  part: ceil(M / 32) doubles.
// in2: the pass-through rows of a critic over two observation branches (in0 / in1), else null (in1 = the pass-through rows)
int twin_q_update_chain_try(const vf_mlp_desc* d, const vf_mlp_bwd_desc* bd, const float* params, const float* packed, const float* in0,
                            const float* in1, const float* in2, const float* target, double* part, float scale, int M, hipStream_t st)
{
    for (int i = 0; i < d->n_layers; ++i)
        if (d->layer[i].dst < VF_MLP_OUT0 && !d->layer[i].save && !((d->identity_mask >> i) & 1)) return 0;   // the weight gradients need every layer input
    for (int i = 0; i < d->n_layers; ++i)
        if (d->layer[i].save && !rows_fit_u32(M, d->layer[i].save_ld)) return 0;
    for (int l = 0; l < bd->n_layers; ++l)
        if (!rows_fit_u32(M, bd->layer[l].ld_dy)) return 0;
    const ChainArgs g{*d, params, packed, ChainIo{{in0, in1, in2}, nullptr, nullptr}, M, nullptr, nullptr, nullptr, {nullptr, nullptr}};
    const BwdArgsChain gb{*bd, packed, M, nullptr, nullptr, nullptr, nullptr, nullptr};
    return chain_serve("vf_twin_q_update", true, &ChainPlugin::twin_q_update, &g, &gb, target, part, scale, M, st);
}

}  // namespace vf

#ifdef VF_CHAIN_TRACE
extern "C" int vf_debug_chain_trace(long long* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(vf::vf_chain_trace), sizeof(long long) * 64, 0, hipMemcpyDeviceToHost);
}
#endif
