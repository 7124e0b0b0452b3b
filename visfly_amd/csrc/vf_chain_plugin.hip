// vf_chain_plugin.hip -- the class table (vf_chain_plugin.hpp): the entries of the built-in classes, and the registry of the chain
// plugins -- shared objects with the register-chained kernels of ONE network shape each, compiled on first use by the host side
// (visfly_amd/_jit.py) for shapes libvisfly_amd.so holds no instance of.
#include "vf_chain_plugin.hpp"
#include "vf_ppo_rollout_kernel.hpp"
#include "vf_bptt_rollout_kernel.hpp"
#include "vf_bptt_reverse_kernel.hpp"
#include "vf_eval_rollout_kernel.hpp"

#include <dlfcn.h>

#include <atomic>
#include <deque>
#include <mutex>
#include <string>

namespace vf {

// PPO: the actor-critic classes (fused PPO step, PPO roll-out); BPTT: the actor classes (a horizon's two persistent launches, and the
// evaluation launch: every class with a 4-wide mean head)
template <class Net, class NetPi, bool PPO, bool BPTT>
constexpr ChainPlugin builtin_entry(const char* name)
{
    using B = Builtin<Net, NetPi>;
    ChainPlugin e{kChainPluginAbi, name, B::forward, B::backward, nullptr, nullptr, kRolloutPluginAbi, nullptr, kBpttRollPluginAbi,
                  kBpttRevPluginAbi, nullptr, nullptr, kEvalPluginAbi, nullptr};
    if constexpr (PPO) e.ppo_update = B::ppo_update, e.ppo_rollout = B::ppo_rollout;
    if constexpr (Net::PASS != 0) e.twin_q_update = B::twin_q_update;
    if constexpr (BPTT) e.bptt_rollout = B::bptt_rollout, e.bptt_reverse = B::bptt_reverse, e.eval_rollout = B::eval_rollout;
    return e;
}

// (a layer table matches at most one class; a function-local table: a namespace-scope constant would be compiled for the device too)
const ChainPlugin* builtin_classes()
{
    static const ChainPlugin t[kBuiltinClassCount] = {
        builtin_entry<NetHover, NetHoverPi, true, true>("NetHover"),      // MlpPolicy actor-critic over StateExtractor; NetHoverPi: its policy trunk
        builtin_entry<NetNav, NetNavPi, true, true>("NetNav"),            // ... over StateTargetExtractor
        builtin_entry<NetSacHover, NetSacHover, false, true>("NetSacHover"),   // td_policies.Actor: mu / log_std heads
        builtin_entry<NetSacNav, NetSacNav, false, true>("NetSacNav"),
        builtin_entry<NetCriticHover, NetCriticHover, false, false>("NetCriticHover"),   // td_policies.ContinuousCritic
    };
    return t;
}

namespace {
struct Loaded {
    std::string path;
    void* handle;
    ChainPlugin p;           // the plugin's entry, less the members whose argument layout stamp is not this build's
};
std::mutex g_mu;
std::deque<Loaded>& loaded()         // (a deque: entries stay where they are while others are added)
{
    static std::deque<Loaded> v;
    return v;
}
}  // namespace

static std::atomic<long long> g_launches{0};
void chain_plugin_count_launch() { g_launches.fetch_add(1, std::memory_order_relaxed); }

static std::atomic<int> g_enabled{1};

int chain_plugin_count()
{
    if (!g_enabled.load(std::memory_order_relaxed)) return 0;
    std::lock_guard<std::mutex> lk(g_mu);
    return (int)loaded().size();
}

const ChainPlugin* chain_plugin(int i)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return i >= 0 && i < (int)loaded().size() ? &loaded()[i].p : nullptr;
}

}  // namespace vf

extern "C" int vf_chain_plugin_load(const char* path)
{
    using namespace vf;
    if (!path) return fail(VF_EINVAL, "vf_chain_plugin_load: null path");
    std::lock_guard<std::mutex> lk(g_mu);
    for (const Loaded& l : loaded())
        if (l.path == path) return VF_OK;
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(VF_EINVAL, "vf_chain_plugin_load: %s", dlerror());
    typedef const ChainPlugin* (*entry_t)();
    entry_t entry = reinterpret_cast<entry_t>(dlsym(h, "vf_chain_plugin"));
    const ChainPlugin* p = entry ? entry() : nullptr;
    if (!p || p->abi != kChainPluginAbi || !((p->forward && p->backward && p->ppo_update) || p->ppo_rollout || (p->bptt_rollout && p->bptt_reverse) ||
                                              p->eval_rollout)) {
        const unsigned abi = p ? p->abi : 0u;      // (p points into the object: read before it is unmapped)
        dlclose(h);
        return fail(VF_EINVAL, "vf_chain_plugin_load: %s is not a chain plugin of this library build (abi %08x, expected %08x)", path,
                    abi, kChainPluginAbi);
    }
    ChainPlugin q = *p;
    if (q.rollout_abi != kRolloutPluginAbi) q.ppo_rollout = nullptr;
    if (q.bptt_roll_abi != kBpttRollPluginAbi) q.bptt_rollout = nullptr;
    if (q.bptt_rev_abi != kBpttRevPluginAbi) q.bptt_reverse = nullptr;
    if (q.eval_abi != kEvalPluginAbi) q.eval_rollout = nullptr;
    loaded().push_back(Loaded{path, h, q});
    return VF_OK;
}

extern "C" int vf_chain_plugin_count()
{
    std::lock_guard<std::mutex> lk(vf::g_mu);
    return (int)vf::loaded().size();
}

extern "C" int vf_chain_plugin_set_enabled(int on)
{
    return vf::g_enabled.exchange(on ? 1 : 0);
}

extern "C" const char* vf_chain_plugin_name(int i)
{
    std::lock_guard<std::mutex> lk(vf::g_mu);
    return i >= 0 && i < (int)vf::loaded().size() ? vf::loaded()[i].p.name : nullptr;
}

extern "C" int64_t vf_chain_plugin_launches() { return vf::g_launches.load(std::memory_order_relaxed); }
