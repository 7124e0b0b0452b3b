// vf_bptt_reverse.hip -- the reverse half of a BPTT horizon as ONE persistent launch (gfx950).
//
// loss.backward() over a horizon (utils/algorithms/BPTT.py:127-129) is a strictly serial chain: the adjoint of env step t needs
// dLoss/d obs_{t+1} from the policy's reverse pass of step t + 1, which needs dLoss/d action_{t+1} from the adjoint of step
// t + 1.  As separate launches that is 2 H launches of 256-512 waves, each latency-bound (~20 us at 16 384 agents).  Agents are
// independent, so here a wave owns ROWS = 16 or 32 agents (the rows-per-wave choice of vf_mlp_backward_data for N rows) for the
// whole sweep t = H-1 .. 0:
//   * adjoint of the control interval + env epilogue for its agents (env_step_bwd_agent, one lane per agent; lanes ROWS..63
//     replicate lane & (ROWS - 1) -- same loads, same arithmetic, same stores of the same values, so no special case);
//   * action head reverse + reverse register chain for the same rows (vf_mlp_chain_bwd.hpp): masked layer gradients into
//     the slot's dZ buffers for the horizon-wide weight-gradient launch, dLoss/d observation for the next adjoint step;
// d_action and the observation gradient travel through per-step rows of scratch (the same wave reads what it wrote).
// Bit-identical to the launch-by-launch sweep (tests/test_bptt_gpu.py).  The launch is served by the class table (vf_chain_plugin.hpp): the
// built-in actor classes' member below, whose kernel instances are compiled in vf_bptt_reverse_<class>[_nodelay].hip, or a generated
// class's BPTT plugin (16 agents per wave with the sub-step tape only).
#include "vf_chain_plugin.hpp"
#include "vf_bptt_reverse_kernel.hpp"

namespace vf {

template <class Net, class NetPi>
int Builtin<Net, NetPi>::bptt_reverse(const vf_mlp_bwd_desc* d, int env_kind, const vf_dyn_cfg* c, const vf_dyn_cfg* d_dyn,
                                      const vf_env_cfg* d_env, const BwdArgsChain* gb, const void* rev_args, int N, hipStream_t st)
{
    constexpr bool sac = Net::HV == 4;      // td_policies.Actor: both head gradients come from d_action and the saved log_std rows
    if (!bwd_chain_matches<Net, true, sac, true>(*d)) return 0;
    if (sac ? !gb->rp_ls_rows : (!gb->rp_log_std || !gb->rp_g_log_std))
        return fail(VF_EINVAL, sac ? "vf_bptt_reverse: log_std_rows (H N, 4) is required for the two-headed actor classes"
                                   : "vf_bptt_reverse: log_std / g_log_std are required for the state-independent-log_std classes");
    const RevArgs& r = *static_cast<const RevArgs*>(rev_args);
    const bool r16 = bwd16_ok<Net, true, sac, true>(*d, N);
    // the tape is read only by the 16-agents-per-wave sweep (its records are the forward launch's waves); with 32 agents per wave
    // (N > 16 384 per launch) the interval is replayed -- same results to the bit -- and with at most kRingRegs delay-ring slots
    const bool ckpt = r.ck && r16 && c->delay_steps <= kRingRegs;
    return c->ctrl_delay ? BpttReverseSet<Net, true>::launch(env_kind, *c, r16, ckpt, d_dyn, d_env, *gb, r, N, st)
                         : BpttReverseSet<Net, false>::launch(env_kind, *c, r16, ckpt, d_dyn, d_env, *gb, r, N, st);
}
template BpttReverseFn Builtin<NetHover, NetHoverPi>::bptt_reverse;
template BpttReverseFn Builtin<NetNav, NetNavPi>::bptt_reverse;
template BpttReverseFn Builtin<NetSacHover>::bptt_reverse;
template BpttReverseFn Builtin<NetSacNav>::bptt_reverse;

}  // namespace vf

extern "C" int vf_bptt_reverse(vf_env* h, const vf_mlp_bwd_desc* desc, const float* packed, const float* log_std, const float* eps,
                               const float* actions, const float* tape, int64_t tape_stride, const uint8_t* tape_done,
                               const float* d_reward, float* adj_slab, float* d_action, const float* g_obs, float* g_log_std, int32_t H,
                               const float* substep_tape, const float* log_std_rows, vf_stream_t stream)
{
    if (!h || !desc || !packed || !eps || !actions || !tape || !tape_done || !d_reward || !adj_slab || !d_action || !g_obs || H <= 0)
        return vf::fail(VF_EINVAL, "vf_bptt_reverse: bad argument");
    if (!h->dyn.S) return vf::fail(VF_ESTATE, "vf_bptt_reverse: vf_env_bind has not been called");
    if (tape_stride < (int64_t)h->dyn.Npad * h->dyn.G * 4) return vf::fail(VF_EINVAL, "vf_bptt_reverse: tape rows are shorter than the slab");
    // rows the kernel reads / writes as float4
    auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    if (misaligned(actions) || misaligned(d_action) || misaligned(eps) || misaligned(g_log_std) || misaligned(log_std_rows) || misaligned(tape) ||
        misaligned(adj_slab) || (tape_stride & 3))
        return vf::fail(VF_EINVAL, "vf_bptt_reverse: actions / d_action / eps / g_log_std / log_std_rows / tape / adj_slab must be 16-byte aligned (float4 rows)");
    if (h->dyn.wind) return vf::fail(VF_EUNSUPPORTED, "vf_bptt_reverse: per-agent wind rows are set");
    if (h->n_obst > 0) return vf::fail(VF_EUNSUPPORTED, "vf_bptt_reverse: the handle has an obstacle table (vf_env_set_obstacles): step launch by launch");
    const int S = h->dyn.cfg.interval_steps;
    if (S > 10) return vf::fail(VF_EUNSUPPORTED, "vf_bptt_reverse: at most 10 sub-steps per control interval");
    const int N = h->dyn.N;
    if ((int64_t)H * N * 128 * 4 >= (1ll << 32))             // the reverse chain addresses its dZ stores with 32-bit byte offsets
        return vf::fail(VF_EUNSUPPORTED, "vf_bptt_reverse: H x N rows of layer gradients pass 4 GiB per buffer");
    // the two-headed actor classes need log_std_rows, the others log_std / g_log_std (each class checks its own: Builtin::bptt_reverse)
    if (!log_std_rows && (!log_std || !g_log_std))
        return vf::fail(VF_EINVAL, "vf_bptt_reverse: log_std_rows (two-headed actor classes) or log_std / g_log_std (state-independent log_std) are required");
    if (reinterpret_cast<uintptr_t>(substep_tape) & 15) return vf::fail(VF_EINVAL, "vf_bptt_reverse: substep_tape must be 16-byte aligned");
    const bool race2 = h->cfg.kind == VF_ENV_RACING && h->cfg.obs_mode == VF_OBS_RACE2;      // RacingEnv2: 16 gate-relative columns
    const int OW = race2 ? 16 : 13;
    bool found = false;        // g_obs must be the (rows, OW) buffer the "state" branch's first layer writes its data gradient to
    for (int l = 0; l < desc->n_layers; ++l) found = found || (desc->layer[l].need_dx && desc->layer[l].dX == g_obs && desc->layer[l].ld_dx == OW);
    if (!found) return vf::fail(VF_EINVAL, "vf_bptt_reverse: g_obs is not the (rows, %d) observation-gradient buffer of the layer table", OW);
    vf::BwdArgsChain gb{*desc, packed, H * N, reinterpret_cast<const float4*>(d_action), reinterpret_cast<const float4*>(actions), log_std,
                        reinterpret_cast<const float4*>(eps), reinterpret_cast<float4*>(g_log_std), reinterpret_cast<const float4*>(log_std_rows),
                        VF_SAC_LOG_STD_MIN, VF_SAC_LOG_STD_MAX};
    vf::RevArgs r{H, N, h->dyn.G, h->dyn.g_drag, h->g_race, tape, tape_stride, reinterpret_cast<const float4*>(actions), tape_done, d_reward,
                  adj_slab, reinterpret_cast<float4*>(d_action), g_obs, reinterpret_cast<const float4*>(substep_tape)};
    const int rc = vf::chain_serve("vf_bptt_reverse", true, &vf::ChainPlugin::bptt_reverse, desc, race2 ? vf::VF_ENV_RACING2 : h->cfg.kind,
                                   &h->dyn.cfg, h->dyn.d_cfg, h->d_cfg, &gb, &r, N, vf::as_stream(stream));
    if (rc < 0) return rc;
    if (rc == 0)
        return vf::fail(VF_EUNSUPPORTED, "vf_bptt_reverse: no persistent reverse sweep for this network class / env kind / dynamics configuration "
                                         "(a generated actor class sweeps 16 agents per wave from the sub-step tape only: N <= 16 384, "
                                         "substep_tape of the forward launch, delay ring <= %d slots)", vf::kRingRegs);
    return VF_OK;
}

#ifdef VF_PPO_TRACE
extern "C" int vf_debug_rev_trace(long long* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(vf::vf_rev_trace), sizeof(long long) * 8, 0, hipMemcpyDeviceToHost);
}
#endif
