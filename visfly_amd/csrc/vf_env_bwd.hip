// vf_env_bwd.hip -- adjoint of the fused env step (gfx950), for first-order policy optimisation.
//
// The reference builds a torch autograd tape of ~3.8k nodes per control step when
// requires_grad=True (utils/algorithms/BPTT.py:107-134, envs/base/dynamics.py:176-190); here the
// reverse pass of one control interval is ONE launch: the thread re-plays the interval from the
// checkpointed pre-step state (tape), parks each sub-step's inputs in LDS, then walks the
// sub-steps backwards with hand-derived adjoints of every op in SURVEY App. A.
//
// Conventions: clamp passes the gradient on the closed interval, abs'(0) = 0,
// quaternion products are differentiated as the polynomial expressions the reference evaluates
// (d(a*b): lam_a = lam * conj(b), lam_b = conj(a) * lam), comparisons / done masks carry no gradient,
// agents reset at the end of a step stop the gradient there.
#include <type_traits>

#include "vf_env_bwd_body.hpp"

namespace vf {

// WIND: the step ran with per-agent wind rows (BwdArgsWind::wind, N rows); the no-wind instances are the code they were without the parameter
template <bool WIND> using BwdArgsOf = std::conditional_t<WIND, BwdArgsWind, BwdArgs>;

// OBST: the handle has an obstacle table, shared or per scene (Navigation kind only: the hover and racing rewards read nothing of the collision)
template <int KIND, int ACT, int INTEG, bool CTRL_DELAY, bool WIND = false, int OBST = vf::VF_TABLE_NONE>
__global__ __launch_bounds__(kBlock) void k_env_step_bwd(const vf_dyn_cfg* __restrict__ cp, const vf_env_cfg* __restrict__ ep, const BwdArgsOf<WIND> g)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [S*kSave][kBlock]
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ((g.N + kBlock - 1) / kBlock) * kBlock) return;
    if constexpr (WIND)
        env_step_bwd_agent<KIND, ACT, INTEG, CTRL_DELAY, kBlock, false, false, true, OBST>(*cp, *ep, g, i, i < g.N, lds + threadIdx.x, nullptr, nullptr,
                                                                                           nullptr, nullptr, nullptr, g.wind);
    else
        env_step_bwd_agent<KIND, ACT, INTEG, CTRL_DELAY, kBlock, false, false, false, OBST>(*cp, *ep, g, i, i < g.N, lds + threadIdx.x);
}

}  // namespace vf

namespace {

template <bool WIND> using BwdKernel = void (*)(const vf_dyn_cfg*, const vf_env_cfg*, const vf::BwdArgsOf<WIND>);

template <int KIND, bool WIND, int OBST = vf::VF_TABLE_NONE>
BwdKernel<WIND> pick_bwd(const vf_dyn_cfg& c)
{
    const int key = (c.integrator == VF_INT_RK4 ? 4 : 0) | (c.action_type == VF_ACT_BODYRATE ? 2 : 0) | (c.ctrl_delay ? 1 : 0);
    switch (key) {
    case 0: return vf::k_env_step_bwd<KIND, VF_ACT_THRUST, VF_INT_EULER, false, WIND, OBST>;
    case 1: return vf::k_env_step_bwd<KIND, VF_ACT_THRUST, VF_INT_EULER, true, WIND, OBST>;
    case 2: return vf::k_env_step_bwd<KIND, VF_ACT_BODYRATE, VF_INT_EULER, false, WIND, OBST>;
    case 3: return vf::k_env_step_bwd<KIND, VF_ACT_BODYRATE, VF_INT_EULER, true, WIND, OBST>;
    case 4: return vf::k_env_step_bwd<KIND, VF_ACT_THRUST, VF_INT_RK4, false, WIND, OBST>;
    case 5: return vf::k_env_step_bwd<KIND, VF_ACT_THRUST, VF_INT_RK4, true, WIND, OBST>;
    case 6: return vf::k_env_step_bwd<KIND, VF_ACT_BODYRATE, VF_INT_RK4, false, WIND, OBST>;
    default: return vf::k_env_step_bwd<KIND, VF_ACT_BODYRATE, VF_INT_RK4, true, WIND, OBST>;
    }
}

template <bool WIND>
int launch_bwd(BwdKernel<WIND> k, int S, int Npad, vf_stream_t stream, const vf_dyn_cfg* d_dyn, const vf_env_cfg* d_env, const vf::BwdArgsOf<WIND>& g)
{
    const size_t lds = (size_t)S * vf::kSave * vf::kBlock * sizeof(float);
    if (lds > 64 * 1024)
        VF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3(Npad / vf::kBlock), dim3(vf::kBlock), lds, vf::as_stream(stream), d_dyn, d_env, g);
    VF_HIP(hipGetLastError());
    return VF_OK;
}

template <bool WIND>
BwdKernel<WIND> pick_env_bwd(int kind, const vf_dyn_cfg& c, int obst)
{
    // (the other kinds' rewards read nothing of the collision)
    if (obst == vf::VF_TABLE_SHARED && kind == VF_ENV_NAV) return pick_bwd<VF_ENV_NAV, WIND, vf::VF_TABLE_SHARED>(c);
    if (obst == vf::VF_TABLE_SCENES && kind == VF_ENV_NAV) return pick_bwd<VF_ENV_NAV, WIND, vf::VF_TABLE_SCENES>(c);
    return kind == VF_ENV_RACING ? pick_bwd<VF_ENV_RACING, WIND>(c) : (kind == VF_ENV_NAV ? pick_bwd<VF_ENV_NAV, WIND>(c) : pick_bwd<VF_ENV_HOVER, WIND>(c));
}

// one body for vf_env_step_bwd (wind == nullptr) and vf_env_step_bwd_wind: `wind` = the rows the forward step ran with, or null = the
// constant vf_dyn_cfg.wind (refused while the handle has rows set: this call cannot know which rows that step ran with)
int env_step_bwd(vf_env* h, const vf_env_bwd_args* a, const float* wind, vf_stream_t stream, const char* who)
{
    if (!h || !a || !a->tape_slab || !a->action || !a->done || !a->adj_slab || !a->d_action)
        return vf::fail(VF_EINVAL, "%s: null argument", who);
    if (reinterpret_cast<uintptr_t>(wind) & 15) return vf::fail(VF_EINVAL, "%s: wind rows must be 16-byte aligned", who);
    if (h->dyn.cfg.action_type != VF_ACT_THRUST && h->dyn.cfg.action_type != VF_ACT_BODYRATE)
        return vf::fail(VF_EINVAL, "%s: the adjoint covers the thrust and bodyrate action types only", who);
    if (h->dyn.cfg.integrator != VF_INT_EULER && h->dyn.cfg.integrator != VF_INT_RK4)
        return vf::fail(VF_EINVAL, "%s: unknown integrator", who);
    if (h->dyn.wind && !wind)
        return vf::fail(VF_EUNSUPPORTED, "%s: per-agent wind rows are set (vf_dyn_set_wind); the adjoint replays the interval with the "
                                         "constant vf_dyn_cfg.wind and would differentiate another trajectory: pass the rows that step "
                                         "ran with to vf_env_step_bwd_wind", who);
    const int S = h->dyn.cfg.interval_steps;
    if (S > 10) return vf::fail(VF_EINVAL, "%s: at most 10 sub-steps per control interval (LDS budget)", who);
    const vf::BwdArgs g{h->dyn.N, h->dyn.G, h->dyn.g_drag, h->g_race, a->tape_slab, reinterpret_cast<const float4*>(a->action),
                        a->d_obs, a->d_reward, a->done, a->adj_slab, reinterpret_cast<float4*>(a->d_action)};
    if (wind)
        return launch_bwd<true>(pick_env_bwd<true>(h->cfg.kind, h->dyn.cfg, vf::table_form(h)), S, h->dyn.Npad, stream, h->dyn.d_cfg, h->d_cfg,
                                vf::BwdArgsWind{g, reinterpret_cast<const float4*>(wind)});
    return launch_bwd<false>(pick_env_bwd<false>(h->cfg.kind, h->dyn.cfg, vf::table_form(h)), S, h->dyn.Npad, stream, h->dyn.d_cfg, h->d_cfg, g);
}

// Dynamics.step's own reverse pass (SURVEY 8b.4 `vf_dyn_step_bwd`): what autograd does for a loss on the states a bare
// `Dynamics` object returns (no env layer, hence no reward term and no episode ends) -- the env adjoint above with d_reward = NULL
// and nobody done, on a vf_dyn handle.  The kernel wants an env constant block: a zeroed one, uploaded once per handle.
int dyn_step_bwd(vf_dyn* h, const float* tape_slab, const float* action, const float* d_state, float* adj_slab, float* d_action,
                 const float* wind, vf_stream_t stream, const char* who)
{
    if (!h || !tape_slab || !action || !adj_slab || !d_action) return vf::fail(VF_EINVAL, "%s: null argument", who);
    if (reinterpret_cast<uintptr_t>(wind) & 15) return vf::fail(VF_EINVAL, "%s: wind rows must be 16-byte aligned", who);
    if (h->cfg.action_type != VF_ACT_THRUST && h->cfg.action_type != VF_ACT_BODYRATE)
        return vf::fail(VF_EINVAL, "%s: the adjoint covers the thrust and bodyrate action types only", who);
    if (h->wind && !wind)
        return vf::fail(VF_EUNSUPPORTED, "%s: per-agent wind rows are set (vf_dyn_set_wind): see vf_env_step_bwd", who);
    const int S = h->cfg.interval_steps;
    if (S > 10) return vf::fail(VF_EINVAL, "%s: at most 10 sub-steps per control interval (LDS budget)", who);
    if (!h->d_cfg) return vf::fail(VF_ESTATE, "%s: the handle has no device constant block", who);
    if (!h->d_env_dummy) {
        vf_env_cfg z{};
        z.kind = VF_ENV_HOVER;
        if (int rc = vf::upload_env_dev(z, 0u, &h->d_env_dummy)) return rc;
    }
    const vf::BwdArgs g{h->N, h->G, h->g_drag, -1, tape_slab, reinterpret_cast<const float4*>(action), d_state, nullptr, nullptr, adj_slab,
                        reinterpret_cast<float4*>(d_action)};
    if (wind)
        return launch_bwd<true>(pick_bwd<VF_ENV_HOVER, true>(h->cfg), S, h->Npad, stream, h->d_cfg, h->d_env_dummy,
                                vf::BwdArgsWind{g, reinterpret_cast<const float4*>(wind)});
    return launch_bwd<false>(pick_bwd<VF_ENV_HOVER, false>(h->cfg), S, h->Npad, stream, h->d_cfg, h->d_env_dummy, g);
}

}  // namespace

extern "C" int vf_env_step_bwd(vf_env* h, const vf_env_bwd_args* a, vf_stream_t stream)
{
    return env_step_bwd(h, a, nullptr, stream, "vf_env_step_bwd");
}

extern "C" int vf_env_step_bwd_wind(vf_env* h, const vf_env_bwd_args* a, const float* wind_Nx4, vf_stream_t stream)
{
    return env_step_bwd(h, a, wind_Nx4, stream, "vf_env_step_bwd_wind");
}

extern "C" int vf_dyn_step_bwd(vf_dyn* h, const float* tape_slab, const float* action, const float* d_state, float* adj_slab,
                               float* d_action, vf_stream_t stream)
{
    return dyn_step_bwd(h, tape_slab, action, d_state, adj_slab, d_action, nullptr, stream, "vf_dyn_step_bwd");
}

extern "C" int vf_dyn_step_bwd_wind(vf_dyn* h, const float* tape_slab, const float* action, const float* d_state, float* adj_slab,
                                    float* d_action, const float* wind_Nx4, vf_stream_t stream)
{
    return dyn_step_bwd(h, tape_slab, action, d_state, adj_slab, d_action, wind_Nx4, stream, "vf_dyn_step_bwd_wind");
}
