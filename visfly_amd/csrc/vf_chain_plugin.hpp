// vf_chain_plugin.hpp -- the class table of the register-chained kernels.  An entry (ChainPlugin) serves one network class: its members
// answer "is this call mine?" and launch the class's kernel instance if it is.  Two kinds of entry, asked in this order:
//   * the built-in classes, compiled into libvisfly_amd.so (Builtin<Net, NetPi> below, table in vf_chain_plugin.hip): NetHover, NetNav
//     (with their policy-only forms NetHoverPi / NetNavPi), NetSacHover, NetSacNav, NetCriticHover;
//   * the chain plugins: shared objects, compiled on first use for one network shape (visfly_amd/_jit.py), that hold the kernels of that
//     shape (vf_mlp_chain_gen.hpp) and the member functions below; loaded with vf_chain_plugin_load (include/visfly_amd.h).
// Every chain entry point (mlp_forward_chain_try, mlp_backward_chain_try, ppo_update_chain_try, twin_q_update_chain_try, vf_ppo_rollout,
// vf_bptt_rollout, vf_bptt_reverse, vf_eval_rollout) validates its arguments, then asks the table once through chain_serve.  Return values of a member:
// 1 launched (or, for a query, "would launch"), 0 not this class / configuration, < 0 error (a plugin: -1000 - hipError_t).
#pragma once
#include "vf_mlp_chain_kernels.hpp"
#ifdef VF_CHAIN_PLUGIN
#include "vf_mlp_chain_gen.hpp"
#endif

namespace vf {

// layout stamp: both sides are compiled from the same headers; a plugin built against other struct layouts is refused
// (0005: the env constant block the persistent launches are handed is a vf_env_dev -- vf_env_cfg + the first global agent id;
// 0006: ChainPlugin ends in eval_abi / eval_rollout)
constexpr unsigned kChainPluginAbi = 0x56460006u ^ (unsigned)(sizeof(vf_mlp_desc) * 31u + sizeof(vf_mlp_bwd_desc) * 17u + sizeof(ChainArgs) * 7u +
                                                            sizeof(BwdArgsChain) * 5u + sizeof(PpoRowArgs) * 3u + sizeof(ReparamFwd) + sizeof(ReparamBwd));

// out1 == null: the policy-only class (no value trunk).  M_choice > 0: the rows-per-wave choice is made for M_choice rows
// (vf_mlp_forward_steps).  in2: a third input -- the pass-through rows of a twin critic over two observation branches; a class with fewer
// inputs answers 0 when it is set
using ChainForwardFn = int(const vf_mlp_desc* d, const float* params, const float* packed, const float* in0, const float* in1, const float* in2,
                           float* out0, float* out1, int M, hipStream_t st, const ReparamFwd* rp, int M_choice);
// packed == null: capability query
using ChainBackwardFn = int(const vf_mlp_bwd_desc* d, const float* packed, int M, hipStream_t st, const ReparamBwd* rp);
using PpoUpdateFn = int(const ChainArgs* g, const BwdArgsChain* gb, const PpoRowArgs* pr, int M, hipStream_t st);
using TwinQUpdateFn = int(const ChainArgs* g, const BwdArgsChain* gb, const float* target, double* part, float scale, int M, hipStream_t st);
// the persistent launches.  env_kind: the KERNEL-side kind (VF_ENV_RACING2 for RacingEnv2's 16-column rows); c: the host copy of the
// dynamics constants; has_target: a second observation input was passed (the constant "target" rows; over a racing
// kind the "gate" column, which the launch itself writes from step 1 on: PpoRollArgs / RollArgs::gate_slots).  env_args / roll_args: vf::EnvArgs / vf::PpoRollArgs
// (vf_ppo_rollout_kernel.hpp), vf::EnvArgs / vf::RollArgs (vf_bptt_rollout_kernel.hpp); rev_args: vf::RevArgs (vf_bptt_reverse_kernel.hpp)
using PpoRolloutFn = int(const vf_mlp_desc* d, int env_kind, const vf_dyn_cfg* c, int has_target, const vf_dyn_cfg* d_dyn, const vf_env_cfg* d_env,
                         const void* env_args, const ChainArgs* gc, const void* roll_args, int N, hipStream_t st);
using BpttRolloutFn = int(const vf_mlp_desc* d, const float* params, int env_kind, const vf_dyn_cfg* c, int has_target, const vf_dyn_cfg* d_dyn,
                          const vf_env_cfg* d_env, const void* env_args, const ChainArgs* gc, const void* roll_args, int N, hipStream_t st);
// the evaluation launch (vf_eval_rollout.hip): env_args / roll_args are vf::EnvArgs / vf::EvalRollArgs (vf_eval_rollout_kernel.hpp); params: the
// rows-per-wave choice reads their alignment (chain16_ok)
using EvalRolloutFn = int(const vf_mlp_desc* d, const float* params, int env_kind, const vf_dyn_cfg* c, int has_target, const vf_dyn_cfg* d_dyn,
                          const vf_env_cfg* d_env, const void* env_args, const ChainArgs* gc, const void* roll_args, int N, hipStream_t st);
using BpttReverseFn = int(const vf_mlp_bwd_desc* d, int env_kind, const vf_dyn_cfg* c, const vf_dyn_cfg* d_dyn, const vf_env_cfg* d_env,
                          const BwdArgsChain* gb, const void* rev_args, int N, hipStream_t st);

struct ChainPlugin {
    unsigned abi;
    const char* name;      // the class / shape, for messages
    // The classes a BPTT / SHAC horizon steps -- the SAC-style Actor, the policy-only class -- run 16 rows per wave where chain16_ok
    // holds, so that their persistent launches (16 agents per wave) equal the per-step path to the bit
    ChainForwardFn* forward;
    ChainBackwardFn* backward;
    PpoUpdateFn* ppo_update;
    // the twin critic's classes (heads (1, 1), pass-through action tile): SHAC's fused critic step (k_twin_q_update_chain); null: not a critic
    TwinQUpdateFn* twin_q_update;
    // a ROLL-OUT plugin (one more shared object per shape AND env kind / action type / integrator / ctrl_delay: the persistent launch of
    // vf_ppo_rollout.hip is a template over all of them) sets only this one; rollout_abi stamps the layout of its arguments
    unsigned rollout_abi;
    PpoRolloutFn* ppo_rollout;
    // a BPTT plugin (per shape AND env kind / action type / integrator / ctrl_delay like the roll-out plugin): the two persistent launches
    // of a BPTT / SHAC horizon for an actor class -- k_bptt_rollout (bptt_roll_abi) and k_bptt_reverse (bptt_rev_abi); a generated class
    // runs 16 agents per wave with the sub-step tape only
    unsigned bptt_roll_abi, bptt_rev_abi;
    BpttRolloutFn* bptt_rollout;
    BpttReverseFn* bptt_reverse;
    // an EVALUATION plugin (per shape AND env kind / action type / integrator / ctrl_delay, like the roll-out plugin): the deterministic
    // episode launch k_eval_rollout for a class with a 4-wide mean head; eval_abi stamps the layout of its arguments
    unsigned eval_abi;
    EvalRolloutFn* eval_rollout;
};

}  // namespace vf

#ifndef VF_CHAIN_PLUGIN
// ---- the library side ----
namespace vf {

// the members of built-in class Net (NetPi: its policy-only form, the class a BPTT horizon steps), each defined and instantiated in the
// translation unit that holds its kernel instances: forward vf_mlp_chain.hip, backward vf_mlp_chain_reverse.hip, ppo_update /
// twin_q_update vf_mlp_chain_split.hip, ppo_rollout vf_ppo_rollout.hip, bptt_rollout vf_bptt_rollout.hip, bptt_reverse vf_bptt_reverse.hip,
// eval_rollout vf_eval_rollout.hip
template <class Net, class NetPi = Net>
struct Builtin {
    static ChainForwardFn forward;
    static ChainBackwardFn backward;
    static PpoUpdateFn ppo_update;
    static TwinQUpdateFn twin_q_update;
    static PpoRolloutFn ppo_rollout;
    static BpttRolloutFn bptt_rollout;
    static BpttReverseFn bptt_reverse;
    static EvalRolloutFn eval_rollout;
};

// the table: the built-in classes (vf_chain_plugin.hip), then the loaded plugins (registry, vf_chain_plugin.hip)
constexpr int kBuiltinClassCount = 5;
const ChainPlugin* builtin_classes();      // kBuiltinClassCount entries
int chain_plugin_count();
const ChainPlugin* chain_plugin(int i);
void chain_plugin_count_launch();      // vf_chain_plugin_launches(): how tests see that a plugin, not the block-tile kernels, served a call

// asks member `fn` of every entry of the table in order and returns the first non-zero answer; 0: nobody serves the call.  `what` names
// the entry point in the message of a plugin's HIP error; launch: a real call, not a capability query -- counted when a plugin serves it
template <class Fn, class... A>
int chain_serve(const char* what, bool launch, Fn* ChainPlugin::*fn, A... a)
{
    auto ask = [&](const ChainPlugin& p, bool plugin) {
        const int rc = p.*fn ? (p.*fn)(a...) : 0;
        if (rc == 1 && launch && plugin) chain_plugin_count_launch();
        if (rc <= -1000) return fail(VF_EHIP, "%s (chain plugin) failed: %s", what, hipGetErrorString((hipError_t)(-rc - 1000)));
        return rc;
    };
    const ChainPlugin* b = builtin_classes();
    for (int i = 0; i < kBuiltinClassCount; ++i)
        if (int rc = ask(b[i], false)) return rc;
    for (int i = 0, n = chain_plugin_count(); i < n; ++i)
        if (int rc = ask(*chain_plugin(i), true)) return rc;
    return 0;
}

}  // namespace vf
#endif

#ifdef VF_CHAIN_PLUGIN
// ---- the plugin side: VF_CHAIN_PLUGIN_PART selects what this translation unit compiles (the parts compile in parallel) ----
//   1: forward kernels, 2: reverse chains, 3: fused PPO step, 0: the table
namespace vf {

template <class Net, class NetPi>
int plugin_forward(const vf_mlp_desc* d, const float* params, const float* packed, const float* in0, const float* in1, const float* in2, float* out0,
                   float* out1, int M, hipStream_t st, const ReparamFwd* rpp, int M_choice)
{
    constexpr int n_in = Net::NB + Net::PASS;      // observation branches, then the pass-through input (ChainIo::in)
    if ((n_in >= 2 && !in1) || (n_in == 3 ? !in2 : in2 != nullptr)) return 0;
    const ReparamFwd rp = rpp ? *rpp : ReparamFwd{};
    if (Net::PASS && (rpp || !out0 || !out1)) return 0;      // the twin critic: Q1 / Q2 (M,), no action head
    ChainArgs g{*d, params, packed, ChainIo{{in0, in1, n_in == 3 ? in2 : nullptr}, out0, out1}, M, rp.log_std, reinterpret_cast<const float4*>(rp.eps),
                reinterpret_cast<float4*>(rp.action), {rp.obs_copy[0], rp.obs_copy[1]}};
    if (!out1) {
        if constexpr (Net::HV != 1 || Net::HM != 4) {
            return 0;             // (the SAC-style Actor always runs both trunks)
        } else {
            if (!chain_matches_gen<NetPi>(*d)) return 0;
            // with the action head (vf_mlp_forward_act: what a BPTT horizon steps) 16 rows per wave for small row counts, like the
            // persistent launch that replaces the loop (k_bptt_rollout); the plain policy-only forward keeps the full class's 32 rows,
            // whose mean it reproduces bit for bit
            if (rp.action && chain16_ok<NetPi>(*d, params, M_choice > 0 ? M_choice : M))
                hipLaunchKernelGGL(k_mlp_forward_chain16<NetPi>, dim3((M + 15) / 16), dim3(64), 0, st, g);
            else
                hipLaunchKernelGGL(k_mlp_forward_chain<NetPi>, dim3((M + 31) / 32), dim3(64), 0, st, g);
        }
    } else {
        if (!chain_matches_gen<Net>(*d)) return 0;
        if constexpr (Net::HV == 4) {      // the SAC-style Actor: 16 rows per wave for small row counts (chain_launch's rule)
            if (chain16_ok<Net>(*d, params, M_choice > 0 ? M_choice : M)) {
                hipLaunchKernelGGL(k_mlp_forward_chain16<Net>, dim3((M + 15) / 16), dim3(64), 0, st, g);
                VF_HIP(hipGetLastError());
                return 1;
            }
        }
        hipLaunchKernelGGL(k_mlp_forward_chain<Net>, dim3((M + 31) / 32), dim3(64), 0, st, g);
    }
    VF_HIP(hipGetLastError());
    return 1;
}

template <class Net>
int plugin_backward(const vf_mlp_bwd_desc* d, const float* packed, int M, hipStream_t st, const ReparamBwd* rpp)
{
    using PU = typename Net::template Bwd<true, true, false>;      // PPO update / SHAC actor: both trunks, no observation gradient
    // with observation gradient: the policy trunk alone (first-order optimisation of an actor-critic's policy) or, for the SAC-style
    // Actor, both trunks (mu and log_std heads both carry gradient)
    // (the twin critic has no such variant: PG = PU)
    using PG = std::conditional_t<Net::PASS != 0, PU, typename Net::template Bwd<true, Net::HV == 4, true>>;
    const ReparamBwd rp = rpp ? *rpp : ReparamBwd{};
    BwdArgsChain g{*d, packed, M, reinterpret_cast<const float4*>(rp.d_action), reinterpret_cast<const float4*>(rp.action), rp.log_std,
                   reinterpret_cast<const float4*>(rp.eps), reinterpret_cast<float4*>(rp.g_log_std)};
    const dim3 grid((M + 31) / 32);
    if (bwd_chain_matches_gen<PU>(*d, false)) {
        if (packed) hipLaunchKernelGGL(k_mlp_backward_chain<PU>, grid, dim3(64), 0, st, g);
    } else if (!Net::PASS && bwd_chain_matches_gen<PG>(*d, true)) {
        if constexpr (!Net::PASS) {        // what a BPTT sweep runs per step: 16 rows per wave for small row counts (bwd_chain_launch's rule)
            if (packed && bwd16_ok_gen<PG>(*d, M)) {
                hipLaunchKernelGGL((k_mlp_backward_chain<PG, 16>), dim3((M + 15) / 16), dim3(64), 0, st, g);
                VF_HIP(hipGetLastError());
                return 1;
            }
        }
        if (packed) hipLaunchKernelGGL(k_mlp_backward_chain<PG>, grid, dim3(64), 0, st, g);
    } else {
        return 0;
    }
    VF_HIP(hipGetLastError());
    return 1;
}

template <class Net0>
int plugin_ppo_update(const ChainArgs* g, const BwdArgsChain* gb, const PpoRowArgs* pr, int M, hipStream_t st)
{
    // more forward tiles than stay live beside the reverse chain: the variant that keeps the ReLU masks as bits (vf_mlp_chain_gen.hpp)
    // (a Tanh / ELU / LeakyReLU network needs the values: above the live-tile limit it has no fused step -- forward, loss and reverse chain
    // then run as the chain launches of their own)
    constexpr bool packable = Net0::all_relu;
    using Net = std::conditional_t<(Net0::n_tiles > kGenLiveTiles && packable), ChainNetG<typename Net0::Spec, true>, Net0>;
    if constexpr (Net::HV != 1 || Net::HM != 4 || (Net0::n_tiles > kGenLiveTiles && !packable)) {
        return 0;                 // (no PPO step on the SAC-style Actor / the twin critic: the kernel is not instantiated)
    } else {
        using PU = typename Net::template Bwd<true, true, false>;
        if (Net::NB == 2 && !g->io.in[1]) return 0;
        if (!chain_matches_gen<Net>(g->d) || !bwd_chain_matches_gen<PU>(gb->d, false)) return 0;
        hipLaunchKernelGGL(k_ppo_update_chain<Net>, dim3((M + 31) / 32), dim3(64), 0, st, *g, *gb, *pr);
        VF_HIP(hipGetLastError());
        return 1;
    }
}

// SHAC's fused critic step on a generated twin-critic class (vf_mlp_chain.hip: twin_q_update_chain_try checked the save pointers / row counts)
template <class Net0>
int plugin_twin_q_update(const ChainArgs* g, const BwdArgsChain* gb, const float* target, double* part, float scale, int M, hipStream_t st)
{
    constexpr bool packable = Net0::all_relu;
    using Net = std::conditional_t<(Net0::n_tiles > kGenLiveTiles && packable), ChainNetG<typename Net0::Spec, true>, Net0>;
    if constexpr (!Net::PASS || (Net0::n_tiles > kGenLiveTiles && !packable)) {
        return 0;
    } else {
        using PU = typename Net::template Bwd<true, true, false>;
        for (int b = 0; b <= Net::NB; ++b)      // the branches' observation rows, then the pass-through rows (chain_pass_tile: io.in[NB])
            if (!g->io.in[b]) return 0;
        if (Net::NB == 1 && g->io.in[2]) return 0;
        if (!chain_matches_gen<Net>(g->d) || !bwd_chain_matches_gen<PU>(gb->d, false)) return 0;
        hipLaunchKernelGGL(k_twin_q_update_chain<Net>, dim3((M + 31) / 32), dim3(64), 0, st, *g, *gb, target, part, scale);
        VF_HIP(hipGetLastError());
        return 1;
    }
}

}  // namespace vf

extern "C" {
int vf_plugin_twin_q_update(const vf::ChainArgs*, const vf::BwdArgsChain*, const float*, double*, float, int, hipStream_t);
int vf_plugin_forward(const vf_mlp_desc*, const float*, const float*, const float*, const float*, const float*, float*, float*, int, hipStream_t,
                      const vf::ReparamFwd*, int);
int vf_plugin_backward(const vf_mlp_bwd_desc*, const float*, int, hipStream_t, const vf::ReparamBwd*);
int vf_plugin_ppo_update(const vf::ChainArgs*, const vf::BwdArgsChain*, const vf::PpoRowArgs*, int, hipStream_t);
const vf::ChainPlugin* vf_chain_plugin();
}

// VF_CHAIN_PLUGIN_DEFINE(Net, NetPi, "name"): the part of the plugin this translation unit holds
#if VF_CHAIN_PLUGIN_PART == 1
#define VF_CHAIN_PLUGIN_DEFINE(Net, NetPi, NAME)                                                                                             \
    extern "C" int vf_plugin_forward(const vf_mlp_desc* d, const float* params, const float* packed, const float* in0, const float* in1,    \
                                     const float* in2, float* out0, float* out1, int M, hipStream_t st, const vf::ReparamFwd* rp, int M_choice) \
    { return vf::plugin_forward<Net, NetPi>(d, params, packed, in0, in1, in2, out0, out1, M, st, rp, M_choice); }
#elif VF_CHAIN_PLUGIN_PART == 2
#define VF_CHAIN_PLUGIN_DEFINE(Net, NetPi, NAME)                                                                                             \
    extern "C" int vf_plugin_backward(const vf_mlp_bwd_desc* d, const float* packed, int M, hipStream_t st, const vf::ReparamBwd* rp)        \
    { return vf::plugin_backward<Net>(d, packed, M, st, rp); }
#elif VF_CHAIN_PLUGIN_PART == 3
#define VF_CHAIN_PLUGIN_DEFINE(Net, NetPi, NAME)                                                                                             \
    extern "C" int vf_plugin_ppo_update(const vf::ChainArgs* g, const vf::BwdArgsChain* gb, const vf::PpoRowArgs* pr, int M, hipStream_t st) \
    { return vf::plugin_ppo_update<Net>(g, gb, pr, M, st); }                                                                                 \
    extern "C" int vf_plugin_twin_q_update(const vf::ChainArgs* g, const vf::BwdArgsChain* gb, const float* target, double* part,            \
                                           float scale, int M, hipStream_t st)                                                               \
    { return vf::plugin_twin_q_update<Net>(g, gb, target, part, scale, M, st); }
#elif VF_CHAIN_PLUGIN_PART == 4
// the roll-out plugin: one translation unit, one kernel instance (vf_ppo_rollout_kernel.hpp defines VF_CHAIN_PLUGIN_ROLLOUT_DEFINE)
#define VF_CHAIN_PLUGIN_DEFINE(Net, NetPi, NAME)
#elif VF_CHAIN_PLUGIN_PART >= 5
// the BPTT plugin: parts 5 (k_bptt_rollout), 6 (k_bptt_reverse), 7 (the table): vf_bptt_rollout_kernel.hpp / vf_bptt_reverse_kernel.hpp
// define VF_CHAIN_PLUGIN_BPTT_DEFINE; part 8: the evaluation plugin (vf_eval_rollout_kernel.hpp defines VF_CHAIN_PLUGIN_EVAL_DEFINE)
#define VF_CHAIN_PLUGIN_DEFINE(Net, NetPi, NAME)
#else
#define VF_CHAIN_PLUGIN_DEFINE(Net, NetPi, NAME)                                                                                             \
    extern "C" const vf::ChainPlugin* vf_chain_plugin()                                                                                      \
    {                                                                                                                                        \
        static const vf::ChainPlugin p{vf::kChainPluginAbi, NAME, vf_plugin_forward, vf_plugin_backward, vf_plugin_ppo_update,               \
                                       Net::PASS ? vf_plugin_twin_q_update : nullptr, 0u, nullptr, 0u, 0u, nullptr, nullptr, 0u, nullptr};                \
        return &p;                                                                                                                           \
    }
#endif
#endif
