// vf_mlp_chain_sep.hpp -- register chains for an actor-critic whose policy and value sides have feature extractors of their own
// (utils/policies/policies.py:117-175,210-215: share_features_extractor=False, or pi_features_extractor_class / vf_features_extractor_class).
//
// Such a network is two pipelines that never meet:  pi extractor(s) -> pi trunk -> action mean  ||  vf extractor(s) -> vf trunk -> value.
// MlpPolicy lists it as ONE layer table,
//     [pi extractor layers][vf extractor layers][pi trunk, mean head][vf trunk, value head]
// over the union of the two sides' observation inputs (<= 2), with one feature buffer per side.  Each side alone is a single-trunk class of
// vf_mlp_chain_gen.hpp (Spec::VF == false): SepNet<Spec, R, ..> is that class with its layer numbers mapped into the common table, and a
// workgroup of two waves owns a tile of 32 rows -- role 0 walks side A (the policy) and role 1 side B (the value), each with the forward,
// its part of the loss (ppo_update_role's division, vf_mlp_chain_split.hip) and the reverse chain of its own layers.  Unlike the split of a
// network with a SHARED extractor (vf_mlp_chain_split.hpp) the waves owe each other nothing: no LDS, no barrier.  Both waves keep under
// 256 VGPRs (amdgpu_waves_per_eu(2, 2)), so the two share a SIMD and fill each other's idle MFMA pipe.
//
// Bits: every value is the same sum of the same products in the same order as in the one-wave chain of that side alone; neither side's
// result depends on the other side's parameters.
//
// Included by the generated translation unit of such a shape only (visfly_amd/_jit.py: source()); served through ChainPlugin::forward /
// ::ppo_update.  The reverse chain on its own (vf_mlp_backward_data) and the persistent launches are not instantiated for these networks.
#pragma once
#include "vf_chain_plugin.hpp"

namespace vf {

// side R of the network: the single-trunk class ChainNetG<S> with its layers at their places in the common table.
//   OE / OT: table index of the side's first extractor layer / first trunk layer;  N_ALL: layers of the whole table
//   I0 / I1: which of the table's inputs branch 0 / 1 of this side reads;  COPY: bit b set = this role writes the call-order copy of
//   branch b's rows (ChainArgs::obs_copy: an input both sides read is copied by role 0)
//   PACK: the variant of vf_mlp_chain_gen.hpp that keeps the ReLU masks of tiles past their last reader as bits (the fused step of a side
//   with more than kSepLiveTiles forward tiles: with every tile live beside the reverse chain such a role does not fit 256 VGPRs)
constexpr int kSepLiveTiles = 12;

template <class S, int R, int OE, int OT, int N_ALL, int I0, int I1, int COPY, bool PACK = false>
struct SepNet : ChainNetG<S, PACK> {
    using Base = ChainNetG<S, PACK>;
    using Packed = SepNet<S, R, OE, OT, N_ALL, I0, I1, COPY, true>;
    using Sh = typename Base::Shape;
    static_assert(!S::VF && S::PASS == 0 && S::HM == 4 && S::HV == 1, "one side: a single-trunk class");
    static constexpr int role = R;
    static constexpr int n_all = N_ALL;
    static constexpr int map(int fl) { return fl < Sh::base() ? OE + fl : OT + (fl - Sh::base()); }
    static constexpr int in_idx(int b) { return b == 0 ? I0 : I1; }
    static constexpr bool copies(int b) { return (COPY >> b) & 1; }
    static constexpr int fl_head = Sh::L_mean();              // the side's head in its own numbering
    static constexpr int head_w = R == 0 ? 4 : 1;
    // what the forward's epilogue keys on: role 0's head is the 4-wide mean (ChainIo::mean), role 1's the 1-wide value (ChainIo::value)
    static constexpr int L_mean = R == 0 ? map(fl_head) : -1, L_value = R == 0 ? -1 : map(fl_head);
    static constexpr int t_head = Base::t_mean;
    static constexpr ChainLayer layer(int i)
    {
        ChainLayer l = Base::tab.l[i];
        l.desc = map(l.desc);
        return l;
    }
};

// its reverse program: the policy-trunk variant without observation gradient over the side's own layers; entries are numbered in the
// reverse table of the WHOLE network (every layer, reversed)
template <class N>
struct SepBwd : BwdProgG<N, true, false, false> {
    using Net = N;
    using Sh = typename N::Sh;
    static constexpr int role = N::role;
    static constexpr int entry(int fl) { return N::n_all - 1 - N::map(fl); }
    static constexpr int fl_head = N::fl_head;
};

// ---- does the table describe side N?  (chain_matches_gen / bwd_chain_matches_gen over the side's layers) ----
template <class N>
bool sep_side_matches(const vf_mlp_desc& d)
{
    using Sh = typename N::Sh;
    for (int b = 0; b < N::NB; ++b) {
        const int i = N::in_idx(b);
        if (i < 0 || i >= d.n_inputs || i > 1 || d.in_dim[i] < 1 || ((d.in_dim[i] + 7) & ~7) != N::kin(b)) return false;
    }
    const int fid = d.layer[N::map(Sh::ext(0, Sh::de(0) - 1))].dst;
    if (fid < 4 || fid >= VF_MLP_MAX_BUFS) return false;
    for (int fl = 0; fl <= N::fl_head; ++fl) {
        const vf_mlp_layer& L = d.layer[N::map(fl)];
        const int b = Sh::branch_of(fl), p = Sh::producer(fl);
        const int K = p == -1 ? d.in_dim[N::in_idx(b)] : p == -2 ? 32 * Sh::n_feat_b() : 32 * Sh::in_tiles(fl);
        const int No = fl == N::fl_head ? N::head_w : 32 * Sh::width(fl);
        if (L.K != K || L.No != No || L.relu != Sh::act_of(fl) || L.wr_off < 0 || (L.wr_off & 3)) return false;
        if (p == -1) {
            if (L.src != N::in_idx(b) || L.src_col != 0) return false;
        } else if (p == -2) {
            if (L.src != fid || L.src_col != 0) return false;
        } else if (L.src != d.layer[N::map(p)].dst || L.src_col != d.layer[N::map(p)].dst_col) {
            return false;
        }
        if (b >= 0 && fl == Sh::ext(b, Sh::de(b) - 1) && (L.dst != fid || L.dst_col != 32 * Sh::feat_off(b))) return false;
        if (b >= 0 && fl != Sh::ext(b, Sh::de(b) - 1) && (L.dst_col != 0 || L.dst == fid)) return false;
        if (b < 0 && fl != N::fl_head && (L.dst_col != 0 || L.dst == fid)) return false;
        if (fl == N::fl_head && L.dst != (N::role == 0 ? VF_MLP_OUT0 : VF_MLP_OUT1)) return false;
        if (L.save && ((L.save_ld & 3) || (L.dst_col & 3) || (reinterpret_cast<uintptr_t>(L.save) & 15))) return false;
    }
    return true;
}

template <class A, class B>
bool sep_matches(const vf_mlp_desc& d)
{
    static_assert(A::n_all == B::n_all, "one table");
    constexpr int n_in = (A::in_idx(0) == 1 || (A::NB == 2 && A::in_idx(1) == 1) || B::in_idx(0) == 1 || (B::NB == 2 && B::in_idx(1) == 1)) ? 2 : 1;
    if (d.n_layers != A::n_all || d.n_inputs != n_in || d.identity_mask) return false;
    if (!sep_side_matches<A>(d) || !sep_side_matches<B>(d)) return false;
    // one feature buffer per side: nothing the one role writes is read by the other
    return d.layer[A::map(A::Sh::ext(0, A::Sh::de(0) - 1))].dst != d.layer[B::map(B::Sh::ext(0, B::Sh::de(0) - 1))].dst;
}

template <class P>
bool sep_bwd_side_matches(const vf_mlp_bwd_desc& d)
{
    using N = typename P::Net;
    using Sh = typename N::Sh;
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    for (int fl = 0; fl <= N::fl_head; ++fl) {
        const vf_mlp_bwd_layer& E = d.layer[P::entry(fl)];
        const int b = Sh::branch_of(fl), p = Sh::producer(fl);
        const bool hidden = fl != N::fl_head;
        if (p == -1) {
            if (E.K < 1 || ((E.K + 7) & ~7) != N::kin(b) || E.need_dx != 0) return false;
        } else if (E.K != 32 * Sh::in_tiles(fl) || E.need_dx != 1) {      // (1: stored, never added -- no buffer of this network has two writers)
            return false;
        }
        const int No = hidden ? 32 * Sh::width(fl) : N::head_w;
        if (E.No != No || (E.Y != nullptr) != hidden || E.wq_off < 0 || (E.wq_off & 3) || !E.dY) return false;
        if (hidden && (E.act ? E.act : VF_ACTIVATION_RELU) != Sh::act_of(fl)) return false;
        if (hidden && (!al16(E.Y) || (E.ld_y & 3) || !al16(E.dY) || (E.ld_dy & 3))) return false;
        if (!hidden && N::head_w == 4 && (!al16(E.dY) || (E.ld_dy & 3))) return false;      // float4 rows of d_mean
        // wiring: the gradient this layer's weights produce is its producer's dY buffer (the feature gradient: the branch's columns)
        if (p >= 0 && E.dX != d.layer[P::entry(p)].dY) return false;
        if (p == -2) {
            for (int bb = 0; bb < N::NB; ++bb) {
                const vf_mlp_bwd_layer& X = d.layer[P::entry(Sh::ext(bb, Sh::de(bb) - 1))];
                if (X.dY != E.dX + 32 * Sh::feat_off(bb) || X.ld_dy != E.ld_dx) return false;
            }
        }
    }
    return true;
}

template <class A, class B>
bool sep_bwd_matches(const vf_mlp_bwd_desc& d)
{
    return d.n_layers == A::n_all && sep_bwd_side_matches<SepBwd<A>>(d) && sep_bwd_side_matches<SepBwd<B>>(d);
}

// observation fragments of the side's branches.  rs: the buffer row the lane loads; rc_copy / live: where (and whether) the row is also
// written in call order (ChainArgs::obs_copy: the fused PPO step on an indexed minibatch)
template <class N>
__device__ __forceinline__ void sep_load_obs(const ChainArgs& g, ChainState<N>& fs, int rs, int h, int rc_copy, bool live)
{
#pragma unroll
    for (int b = 0; b < N::NB; ++b) {
        constexpr int i0 = N::in_idx(0), i1 = N::in_idx(1);
        const int i = b == 0 ? i0 : i1;
        const int w = g.d.in_dim[i];
        const float* x = g.io.in[i] + (size_t)rs * w;
        float* xc = (N::copies(b) && g.obs_copy[i] && live) ? g.obs_copy[i] + (size_t)rc_copy * w : nullptr;
#pragma unroll
        for (int s = 0; s < N::kin(b) / 2; ++s) {
            const int k = 2 * s + h;
            const float v = x[k < w ? k : w - 1];
            fs.x[b][s] = k < w ? v : 0.0f;
            if (xc && k < w) xc[k] = v;
        }
    }
}

template <class N>
__device__ __forceinline__ void sep_forward_role(const ChainArgs& g)
{
    const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
    const int row = blockIdx.x * 32 + m;
    const bool live = row < g.M;
    const int rc = live ? row : g.M - 1;
    ChainState<N> st;
    chain_prologue<N, 0>(g, st, lane);
    sep_load_obs<N>(g, st, rc, h, rc, live);
    chain_items<N, 0>(g, st, lane, row, live, rc);
}

// blockDim 128: role 0 -> io.mean, role 1 -> io.value; blockDim 64 (the caller does not need the value): role 0 alone
template <class A, class B>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_chain_forward_sep(const ChainArgs g)
{
    prefetch_kernarg<sizeof(ChainArgs)>();
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (role == 0) sep_forward_role<A>(g);
    else sep_forward_role<B>(g);
}

// one role of the fused PPO minibatch step: forward chain of its side -> its terms of the row's loss (role 0: the policy terms and every
// statistic but the value loss; role 1: the value terms) -> head gradient -> reverse chain of its side.  Leaves what k_ppo_update_split
// leaves: the saved layer inputs, the masked dZ of every layer, d_mean / d_value, one row of kStats partials per tile.
template <class N>
__device__ __forceinline__ void sep_ppo_update_role(const ChainArgs& g, const BwdArgsChain& gb, const PpoRowArgs& pr)
{
    using P = SepBwd<N>;
    constexpr int R = N::role;
    const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
    const int row = blockIdx.x * 32 + m;
    const bool live = row < g.M;
    const int rc = live ? row : g.M - 1;
    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float old_lp = 0.0f, adv = 0.0f, ret = 0.0f, ls[4] = {0.f, 0.f, 0.f, 0.f};
    const int rs = ppo_source_row(pr, rc);
    if constexpr (R == 0) {
        a4 = pr.action[rs];
#pragma unroll
        for (int k = 0; k < 4; ++k) ls[k] = pr.log_std[k];
        old_lp = pr.old_lp[rs];
        adv = pr.adv[rc];
    } else {
        ret = pr.ret[rs];
    }
    ChainState<N> fs;
    if constexpr (N::pack_or) {
#pragma unroll
        for (int i = 0; i < N::n_mb; ++i) fs.mb[i] = 0u;
    }
    chain_prologue<N, 0>(g, fs, lane);
    sep_load_obs<N>(g, fs, rs, h, rc, live);
    PpoRowPre pre{};
    if constexpr (R == 0) {
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
        pre = ppo_row_pre(a);
#pragma unroll
        for (int d = 0; d < 4; ++d)     // pinned here (k_ppo_update_chain)
            asm volatile("" : "+v"(pre.g[d]), "+v"(pre.corr[d]));
    }
    chain_items<N, 0>(g, fs, lane, row, live, rc);
    BwdState<P> bs;
    bwd_prologue<P, 0>(gb, bs, lane);                  // first weight blocks of the reverse chain: in flight during the loss arithmetic
    const bool on = live && h == 0;
    const vf_mlp_bwd_layer& Eh = gb.d.layer[P::entry(P::fl_head)];
    // head gradients in lane half 0 of EVERY lane: lanes past the last row are replicas of row M - 1 and stay replicas through the
    // reverse chain, whose dZ stores are unguarded (k_ppo_update_chain).  The side's head is the FIRST head of its class: hin[0]
    if constexpr (R == 0) {
        const f32x16& mt = fs.t[N::t_head];
        const float mu[4] = {mt[0], mt[1], mt[2], mt[3]};
        float st1[9], dm1[4], dv1;
        ppo_row_post(pre, mu, 0.0f, ls, old_lp, adv, 0.0f, pr.cfg, dm1, dv1, st1, rc);
#pragma unroll
        for (int k = 0; k < 4; ++k) bs.hin[0][k] = h == 0 ? dm1[k] : 0.0f;
        if (on) *reinterpret_cast<float4*>(const_cast<float*>(Eh.dY) + (size_t)row * Eh.ld_dy) = make_float4(dm1[0], dm1[1], dm1[2], dm1[3]);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (k == 1) continue;
            float s = on ? st1[k] : 0.0f;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
            if (lane == 0) pr.part[(size_t)blockIdx.x * kStats + k] = s;
        }
    } else {
        const float mu[4] = {0.f, 0.f, 0.f, 0.f};
        float st1[9], dm1[4], dv1;
        ppo_row_post(pre, mu, fs.t[N::t_head][0], ls, 0.0f, 0.0f, ret, pr.cfg, dm1, dv1, st1, rs);     // (only the value terms are used)
        const float dvl = h == 0 ? dv1 : 0.0f;
        bs.hin[0][0] = dvl; bs.hin[0][1] = 0.0f; bs.hin[0][2] = 0.0f; bs.hin[0][3] = 0.0f;
        if (on) const_cast<float*>(Eh.dY)[(size_t)row * Eh.ld_dy] = dvl;
        float s = on ? st1[1] : 0.0f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) pr.part[(size_t)blockIdx.x * kStats + 1] = s;
    }
    bs.hin[1][0] = 0.0f; bs.hin[1][1] = 0.0f; bs.hin[1][2] = 0.0f; bs.hin[1][3] = 0.0f;
    bwd_items<P, ChainState<N>, 0>(gb, bs, fs, lane, row, rc, live);
    bwd_tail_store<P>(gb, bs, row, h, live);
}

template <class A, class B>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_ppo_update_sep(const ChainArgs g, const BwdArgsChain gb, const PpoRowArgs pr)
{
    prefetch_kernarg<sizeof(ChainArgs) + sizeof(BwdArgsChain) + sizeof(PpoRowArgs)>();
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (role == 0) sep_ppo_update_role<A>(g, gb, pr);
    else sep_ppo_update_role<B>(g, gb, pr);
}

// ---- the plugin's members ----
template <class A, class B>
int plugin_forward_sep(const vf_mlp_desc* d, const float* params, const float* packed, const float* in0, const float* in1, const float* in2, float* out0,
                       float* out1, int M, hipStream_t st, const ReparamFwd* rpp)
{
    if (in2 || rpp || !out0 || M < 1) return 0;        // (no action head on these classes: vf_mlp_forward_act is a horizon's call)
    if (!sep_matches<A, B>(*d)) return 0;
    if (d->n_inputs == 2 && !in1) return 0;
    const ChainArgs g{*d, params, packed, ChainIo{{in0, in1, nullptr}, out0, out1}, M, nullptr, nullptr, nullptr, {nullptr, nullptr}};
    hipLaunchKernelGGL((k_chain_forward_sep<A, B>), dim3((M + 31) / 32), dim3(out1 ? 128 : 64), 0, st, g);
    VF_HIP(hipGetLastError());
    return 1;
}

// a side with many forward tiles runs the fused step with its ReLU masks as bits (a Tanh / ELU / LeakyReLU side needs the values: it
// keeps them and spills what does not fit)
template <class N>
using SepFused = std::conditional_t<(N::n_tiles > kSepLiveTiles && N::all_relu), typename N::Packed, N>;

template <class A0, class B0>
int plugin_ppo_update_sep(const ChainArgs* g, const BwdArgsChain* gb, const PpoRowArgs* pr, int M, hipStream_t st)
{
    using A = SepFused<A0>;
    using B = SepFused<B0>;
    if (M < 1 || !g->io.in[0] || g->io.in[2]) return 0;
    if (!sep_matches<A, B>(g->d) || !sep_bwd_matches<A, B>(gb->d)) return 0;
    if (g->d.n_inputs == 2 && !g->io.in[1]) return 0;
    hipLaunchKernelGGL((k_ppo_update_sep<A, B>), dim3((M + 31) / 32), dim3(128), 0, st, *g, *gb, *pr);
    VF_HIP(hipGetLastError());
    return 1;
}

}  // namespace vf

// VF_CHAIN_PLUGIN_SEP_DEFINE(A, B, "name"): the part of the plugin this translation unit holds (parts as in vf_chain_plugin.hpp:
// 1 forward, 2 reverse chain -- not instantiated for these networks --, 3 fused PPO step, 0 the table)
#if VF_CHAIN_PLUGIN_PART == 1
#define VF_CHAIN_PLUGIN_SEP_DEFINE(A, B, NAME)                                                                                               \
    extern "C" int vf_plugin_forward(const vf_mlp_desc* d, const float* params, const float* packed, const float* in0, const float* in1,    \
                                     const float* in2, float* out0, float* out1, int M, hipStream_t st, const vf::ReparamFwd* rp, int)       \
    { return vf::plugin_forward_sep<A, B>(d, params, packed, in0, in1, in2, out0, out1, M, st, rp); }
#elif VF_CHAIN_PLUGIN_PART == 2
#define VF_CHAIN_PLUGIN_SEP_DEFINE(A, B, NAME)                                                                                               \
    extern "C" int vf_plugin_backward(const vf_mlp_bwd_desc*, const float*, int, hipStream_t, const vf::ReparamBwd*) { return 0; }
#elif VF_CHAIN_PLUGIN_PART == 3
#define VF_CHAIN_PLUGIN_SEP_DEFINE(A, B, NAME)                                                                                               \
    extern "C" int vf_plugin_ppo_update(const vf::ChainArgs* g, const vf::BwdArgsChain* gb, const vf::PpoRowArgs* pr, int M, hipStream_t st) \
    { return vf::plugin_ppo_update_sep<A, B>(g, gb, pr, M, st); }
#else
#define VF_CHAIN_PLUGIN_SEP_DEFINE(A, B, NAME)                                                                                               \
    extern "C" const vf::ChainPlugin* vf_chain_plugin()                                                                                      \
    {                                                                                                                                        \
        static const vf::ChainPlugin p{vf::kChainPluginAbi, NAME, vf_plugin_forward, vf_plugin_backward, vf_plugin_ppo_update,               \
                                       nullptr, 0u, nullptr, 0u, 0u, nullptr, nullptr, 0u, nullptr};                                         \
        return &p;                                                                                                                           \
    }
#endif
