// vf_eval_rollout_kernel.hpp -- the deterministic evaluation episodes of a policy as ONE persistent launch, a template over the network class
// (scheme: vf_eval_rollout.hip), shared by vf_eval_rollout.hip (the built-in classes) and the evaluation plugins of generated classes
// (vf_chain_plugin.hpp, part 8).  A sibling of k_ppo_rollout (vf_ppo_rollout_kernel.hpp): the same wave <-> agent map, the same forward, the
// same env step -- without sampler, buffer rows and re-spawn, with a first-done latch and a wave exit instead.
#pragma once
#include "vf_ppo_rollout_kernel.hpp"

#pragma clang fp contract(off)

namespace vf {

struct EvalRollArgs {
    int T, N;                       // T: max_episode_steps -- `done` is set for every agent after that many steps at the latest
    const float* obs0;              // (N,OW) the observation the episodes start from
    const float* gate0;             // (N,) racing kinds, two-branch class: the gate column of obs0 (the index as a float), else null
    // the latched outputs: what the env epilogue wrote for the agent at the FIRST step that set its `done` (later steps keep
    // overwriting the env's own episode outputs: without re-spawn `done` is sticky)
    float* ep_return;               // (N,)
    int* ep_length;                 // (N,)
    unsigned char* ep_flags;        // (N,) VF_EP_*
    float* terminal_rows;           // (N,OW) or null
};

// EnvArgs::out.obs is ONE (N,OW) row block, overwritten every step (the next forward reads the rows from the wave's LDS tile they are staged
// through); EnvArgs::auto_reset = 0; the second observation (ChainIo::in[1]) is the (N,w1) block of constant "target" rows
template <class Net, int ROWS, int KIND, int ACT, int INTEG, bool CTRL_DELAY>
__global__ __launch_bounds__(64) void k_eval_rollout(const vf_dyn_cfg* __restrict__ cp, const vf_env_cfg* __restrict__ ep, const EnvArgs ge,
                                                     const ChainArgs gc, const EvalRollArgs r)
{
    prefetch_kernarg<sizeof(EnvArgs) + sizeof(ChainArgs) + sizeof(EvalRollArgs) + 16>();
    const vf_dyn_cfg& c = *cp;
    const vf_env_cfg& e = *ep;
    constexpr int OW = obs_width(KIND);
    constexpr bool GATE = kGateBranch<Net, KIND>;
    __shared__ __attribute__((aligned(16))) float tile[64 * OW];
    const int lane = threadIdx.x, m = lane & (ROWS - 1);
    const int wave_first = blockIdx.x * ROWS;
    // lanes ROWS..63 and the lanes past the last agent are REPLICAS of a live lane (k_ppo_rollout's construction): same index, loads,
    // arithmetic, `done` and latch state; the latched outputs are written by the owner
    const int i = min(wave_first + m, r.N - 1);
    const bool owner = lane < ROWS && wave_first + lane < r.N;
    EnvArgs g = ge;
    g.d.N = min(r.N, wave_first + ROWS);                  // the wave's observation tile holds ROWS rows
    Agent s;
    Spares sp;
    load_agent<true>(g.d.S, g.d.G, i, s, sp);
    load_wind(c, g.d, i, true, s);
    const int Gx = g.d.G;
    for (int k = 0; k < OW; ++k) tile[lane * OW + k] = r.obs0[(size_t)i * OW + k];
    float gate_col = 0.0f;
    if constexpr (GATE) gate_col = r.gate0[i];
    __builtin_amdgcn_wave_barrier();
    bool latched = false;
    for (int t = 0; t < r.T; ++t) {
        // (k_ppo_rollout: an opaque lane id and an opaque zero in the weight pointers per iteration keep the chain's loop-invariant load
        // offsets and base addresses out of registers across the t loop; the delay-ring slot is loaded ahead of the forward)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const float4 ring_old = *granule(g.d.S, Gx, i, c.delay_steps > 0 ? VF_G_RING + g.d.head : 0);
        long zero_t = 0;
        asm volatile("" : "+s"(zero_t));
        ChainArgs gct = gc;
        gct.packed = gc.packed + zero_t;
        gct.params = gc.params + zero_t;
        float4 mean = policy_rows<Net, ROWS, OW, GATE>(gct, lane_t, i, tile, gate_col);
        mean.x = __shfl(mean.x, m); mean.y = __shfl(mean.y, m); mean.z = __shfl(mean.z, m); mean.w = __shfl(mean.w, m);
        // the deterministic action of either actor kind: tanh(mean) (k_eval_action's arithmetic)
        float4 an = make_float4(tanhf(mean.x), tanhf(mean.y), tanhf(mean.z), tanhf(mean.w));
        float a[4];
        if (c.delay_steps > 0) {
            const int head = g.d.head;
            *granule(g.d.S, Gx, i, VF_G_RING + head) = an;
            an = ring_old;
            sp.vel = __int_as_float(head + 1 == c.delay_steps ? 0 : head + 1);
        }
        a[0] = an.x; a[1] = an.y; a[2] = an.z; a[3] = an.w;
        float kl[3], kq[3];
        drag_of(c, g.d, i, kl, kq);
        control_interval<ACT, INTEG, CTRL_DELAY>(c, s, a, kl, kq, g.d.vstrided != 0);
        float reward = 0.0f;
        bool done = false;
        int gate_next = 0;
        env_epilogue<KIND, false>(c, e, g, i, true, s, sp, wave_first, tile, &reward, &done, nullptr, GATE ? &gate_next : nullptr);
        if (done && !latched && owner) {
            // ep_return / ep_length / ep_flags / terminal row: this lane's own stores of the epilogue
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            r.ep_return[i] = g.out.ep_return[i];
            r.ep_length[i] = g.out.ep_length[i];
            r.ep_flags[i] = g.out.ep_flags[i];
            if (r.terminal_rows) {
                const float* to = g.out.terminal_obs + OW * (size_t)i;
                for (int k = 0; k < OW; ++k) r.terminal_rows[(size_t)i * OW + k] = to[k];
            }
        }
        latched = latched || done;
        if constexpr (GATE) gate_col = (float)gate_next;
        g.d.head = g.d.head + 1 == c.delay_steps ? 0 : g.d.head + 1;
        // every agent of the wave has its episode: what it does afterwards is ignored (wave-uniform: replicas latch with their lane)
        if (__builtin_amdgcn_ballot_w64(!latched) == 0) break;
    }
    store_agent(g.d.S, Gx, i, s, sp);
}

// layout stamp of what an evaluation plugin is handed (vf_chain_plugin.hpp: ChainPlugin::eval_abi)
constexpr unsigned kEvalPluginAbi = 0x45560001u ^ (unsigned)(sizeof(EnvArgs) * 31u + sizeof(EvalRollArgs) * 17u + sizeof(vf_dyn_cfg) * 7u +
                                                            sizeof(vf_env_dev) * 5u + sizeof(ChainArgs) * 3u);

// which kernel-side env kinds / motor-lag forms a class with NB observation branches is evaluated over: what k_ppo_rollout serves
// (vf_ppo_rollout.hip: Builtin::ppo_rollout)
constexpr bool eval_instance(int NB, int kind, bool delay)
{
    return NB == 2 ? kind == VF_ENV_NAV || (kind_is_racing(kind) && delay) : kind == VF_ENV_HOVER || kind == VF_ENV_NAV || delay;
}

}  // namespace vf

#ifndef VF_CHAIN_PLUGIN
#include "vf_chain_plugin.hpp"
namespace vf {

// the evaluation of a built-in class with a 4-wide mean head: the actor-critic classes (PPO; the one-head BPTT actor) and the SAC-style
// Actor (BPTT(policy=...), SHAC: only the mu head is read), over the env kinds / motor-lag forms of eval_instance
template <class Net, class NetPi>
int Builtin<Net, NetPi>::eval_rollout(const vf_mlp_desc* d, const float* params, int env_kind, const vf_dyn_cfg* c, int has_target,
                                      const vf_dyn_cfg* d_dyn, const vf_env_cfg* d_env, const void* env_args, const ChainArgs* gc,
                                      const void* roll_args, int N, hipStream_t st)
{
    if (!chain_matches<Net>(*d) || (Net::NB == 2 ? !has_target : has_target && env_kind != VF_ENV_HOVER)) return 0;
    const bool r16 = chain16_ok<Net>(*d, params, N);
    const EnvArgs& ge = *static_cast<const EnvArgs*>(env_args);
    const EvalRollArgs& r = *static_cast<const EvalRollArgs*>(roll_args);
    if (Net::NB == 2 && (env_kind == VF_ENV_RACING || env_kind == VF_ENV_RACING2) && (!r.gate0 || d->in_dim[1] != 1)) return 0;
    // the actor-critic classes (what PPO trains) over all four action types; the SAC-style Actor is BPTT's / SHAC's, which have no
    // velocity / position horizon (vf_env_device.hpp: with_env_config)
    return with_env_config<Net::HV == 1>(env_kind, *c, [&](auto kind, auto act, auto integ, auto delay) -> int {
        constexpr int K = decltype(kind)::value, A = decltype(act)::value, I = decltype(integ)::value;
        constexpr bool D = decltype(delay)::value;
        if constexpr (eval_instance(Net::NB, K, D)) {
            if (r16) hipLaunchKernelGGL((k_eval_rollout<Net, 16, K, A, I, D>), dim3((N + 15) / 16), dim3(64), 0, st, d_dyn, d_env, ge, *gc, r);
            else hipLaunchKernelGGL((k_eval_rollout<Net, 32, K, A, I, D>), dim3((N + 31) / 32), dim3(64), 0, st, d_dyn, d_env, ge, *gc, r);
            VF_HIP(hipGetLastError());
            return 1;
        } else {
            return 0;
        }
    });
}
extern template EvalRolloutFn Builtin<NetHover, NetHoverPi>::eval_rollout;      // vf_eval_rollout.hip
extern template EvalRolloutFn Builtin<NetNav, NetNavPi>::eval_rollout;
extern template EvalRolloutFn Builtin<NetSacHover>::eval_rollout;               // vf_eval_rollout_sac.hip
extern template EvalRolloutFn Builtin<NetSacNav>::eval_rollout;

}  // namespace vf
#endif

#if defined(VF_CHAIN_PLUGIN) && VF_CHAIN_PLUGIN_PART == 8
#include "vf_mlp_chain_gen.hpp"
#include "vf_chain_plugin.hpp"
namespace vf {

// the evaluation launch of ONE generated class with a 4-wide mean head under ONE env kind / action type / integrator / motor-lag setting.
// Rows per wave: the choice of the plugin's per-step forward with both heads (vf_chain_plugin.hpp: plugin_forward) -- 32 for the
// actor-critic classes, chain16_ok's for the SAC-style Actor -- so that the means are the launch-by-launch loop's to the bit
template <class Net, int KIND, int ACT, int INTEG, bool DELAY>
int plugin_eval_rollout(const vf_mlp_desc* d, const float* params, int env_kind, const vf_dyn_cfg* c, int has_target, const vf_dyn_cfg* d_dyn,
                        const vf_env_cfg* d_env, const void* env_args, const ChainArgs* gc, const void* roll_args, int N, hipStream_t st)
{
    if constexpr (Net::HM != 4 || Net::PASS != 0) {
        return 0;
    } else {
        if (env_kind != KIND || c->action_type != ACT || c->integrator != INTEG || (c->ctrl_delay != 0) != DELAY) return 0;
        if ((Net::NB == 2) != (has_target != 0) || (Net::NB == 2 && KIND != VF_ENV_NAV && !kind_is_racing(KIND))) return 0;
        if (kGateBranch<Net, KIND> && (!static_cast<const EvalRollArgs*>(roll_args)->gate0 || d->in_dim[1] != 1)) return 0;
        if (!chain_matches_gen<Net>(*d)) return 0;
        const EnvArgs& ge = *static_cast<const EnvArgs*>(env_args);
        const EvalRollArgs& r = *static_cast<const EvalRollArgs*>(roll_args);
        if constexpr (Net::HV == 4) {       // (an actor-critic class has no 16-row instance: one kernel per plugin)
            if (chain16_ok<Net>(*d, params, N)) {
                hipLaunchKernelGGL((k_eval_rollout<Net, 16, KIND, ACT, INTEG, DELAY>), dim3((N + 15) / 16), dim3(64), 0, st, d_dyn, d_env, ge, *gc, r);
                VF_HIP(hipGetLastError());
                return 1;
            }
        }
        hipLaunchKernelGGL((k_eval_rollout<Net, 32, KIND, ACT, INTEG, DELAY>), dim3((N + 31) / 32), dim3(64), 0, st, d_dyn, d_env, ge, *gc, r);
        VF_HIP(hipGetLastError());
        return 1;
    }
}

}  // namespace vf

#define VF_CHAIN_PLUGIN_EVAL_DEFINE(Net, KIND, ACT, INTEG, DELAY, NAME)                                                                      \
    static int vf_plugin_eval_rollout(const vf_mlp_desc* d, const float* params, int env_kind, const vf_dyn_cfg* c, int has_target,          \
                                      const vf_dyn_cfg* d_dyn, const vf_env_cfg* d_env, const void* ea, const vf::ChainArgs* gc,             \
                                      const void* ra, int N, hipStream_t st)                                                                 \
    { return vf::plugin_eval_rollout<Net, KIND, ACT, INTEG, DELAY>(d, params, env_kind, c, has_target, d_dyn, d_env, ea, gc, ra, N, st); }   \
    extern "C" const vf::ChainPlugin* vf_chain_plugin()                                                                                      \
    {                                                                                                                                        \
        static const vf::ChainPlugin p{vf::kChainPluginAbi, NAME, nullptr, nullptr, nullptr, nullptr, 0u, nullptr, 0u, 0u, nullptr, nullptr, \
                                       vf::kEvalPluginAbi, vf_plugin_eval_rollout};                                                          \
        return &p;                                                                                                                           \
    }
#endif
