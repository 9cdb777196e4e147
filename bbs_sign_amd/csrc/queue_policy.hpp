#pragma once
// Hardware-queue policy of the runtime layer (runtime.hpp stream_create): which kind of stream the next one is.  Pure
// functions of integers -- no HIP, no environment, no state -- so that the policy compiles and is tested on a CPU
// (tests/cpp/queue_policy.cpp).  DESIGN.md 5 rule 6.
//
// Two kinds of stream exist.  A POOLED stream is bound by the runtime to one of the GPU_MAX_HW_QUEUES hardware queues of the
// process, round robin; a DEDICATED stream (created with an all-ones compute-unit mask) gets a hardware queue of its own
// outside that pool.  Every hardware queue that has run a kernel reserves scratch for that kernel's frame, so the number of
// queues the library touches is a budget (`total`, runtime.hpp queue_budget); past it the runtime aborts the process.
//
// Two pools are told apart:
//   env_pool        GPU_MAX_HW_QUEUES as the environment has it NOW (4 when unset).  The library's own load-time default may
//                   have written it after the runtime had read it, so it is an UPPER bound on the pooled queues, not the truth.
//   effective_pool  what the runtime most probably really uses (load_pool below); decides how much there is to gain.
// Whatever was guessed, the streams handed out satisfy   dedicated_made + min(env_pool, pooled_made) <= total   (total > 0):
// a wrong guess costs speed, never the runtime's abort.
namespace qpolicy {

constexpr int AUTO = -1;             // setting: nothing was asked for, the library decides from the effective pool
constexpr int OWN_POOL = 20;         // the pool the library sets for itself when it is loaded before the runtime starts (capi.hip)
constexpr int RUNTIME_POOL = 4;      // the runtime's own default
constexpr int MAX_DEDICATED = 16;    // the most dedicated streams per device that can be asked for
// the most the automatic setting wishes for.  Measured at a pool of 4 (profiles/auto_queues_ab.log), six 4096-item jobs in flight
// = 19 streams: 16 is 1.7 % ahead of 12 over 128 steps (1.596 against 1.569 M proof_verify/s, about the run-to-run spread) and
// 18 % behind over 20 steps right after the warm-up (0.93 against 1.13 M/s: every queue pays for its scratch when it first runs
// a large kernel frame, and 12 + 4 queues are through with that sooner than 16 + 3)
constexpr int AUTO_MAX = 12;

inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }

// what was found when the library was loaded (capi.hip records it once, before it touches the environment)
enum Runtime { RT_UNKNOWN = -1, RT_NOT_STARTED = 0, RT_STARTED = 1 };
inline int load_pool(bool variable_was_set, int value_found, int runtime_at_load) {
    if (variable_was_set) return value_found > 0 ? value_found : RUNTIME_POOL;      // somebody else's choice: that value
    return runtime_at_load == RT_NOT_STARTED ? OWN_POOL : RUNTIME_POOL;             // ours took effect only if it came first
}

// dedicated streams wished for per device: an explicit setting is taken as it is, AUTO makes up what the effective pool lacks
// of the library's own, up to AUTO_MAX (4 -> 12, 14 -> 6, 20 or more -> none)
inline int wish(int setting, int effective_pool) {
    const int w = setting == AUTO ? imin(OWN_POOL - effective_pool, AUTO_MAX) : setting;
    return w < 0 ? 0 : (w > MAX_DEDICATED ? MAX_DEDICATED : w);
}

enum Kind { DEDICATED = 0, POOLED = 1, NONE = 2 };      // NONE: no queue left in the budget, the caller shares a stream it has
// total <= 0: the budget is unknown (the device could not be asked), nothing is cut.
// A dedicated stream is granted while the wish lasts and the budget still holds it BESIDE the pooled queues already touched and
// beside the effective pool (whose queues later streams will touch); a pooled stream while the pooled queues touched stay in
// the budget.  Since a dedicated stream always leaves room for one pooled queue, a first pooled stream is never refused.
inline Kind next_stream(int effective_pool, int env_pool, int total, int setting, int dedicated_made, int pooled_made) {
    env_pool = imax(env_pool, 1);
    const int reserve = imax(imin(env_pool, pooled_made), imin(env_pool, imax(effective_pool, 1)));
    if (dedicated_made < wish(setting, effective_pool) && (total <= 0 || dedicated_made + 1 + reserve <= total)) return DEDICATED;
    if (total <= 0 || dedicated_made + imin(env_pool, pooled_made + 1) <= total) return POOLED;
    return NONE;
}

}  // namespace qpolicy
