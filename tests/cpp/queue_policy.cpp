// Stand-alone check of the hardware-queue policy (bbs_sign_amd/csrc/queue_policy.hpp): no HIP, no library -- the header
// alone.  Simulates stream creation as runtime.hpp stream_create does it (ask next_stream, count what was made) from
// every starting point and asserts what the policy promises.  tests/test_queue_policy.py compiles and runs it.
#include <cstdio>
#include <cstdlib>

#include "../../bbs_sign_amd/csrc/queue_policy.hpp"

using namespace qpolicy;

static long checks = 0;
#define CHECK(c, ...) do { checks++; if (!(c)) { std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

// the rule of the library before the automatic setting, for the explicit settings where both apply: how many of `n` streams
// created from nothing came out dedicated / pooled / refused, with dedicated_cap = max(0, total - pool)
static void old_rule(int pool, int total, int k, int n, int& d, int& p, int& none) {
    d = p = none = 0;
    int want = k;
    if (total > 0) want = want < (total - pool > 0 ? total - pool : 0) ? want : (total - pool > 0 ? total - pool : 0);
    for (int i = 0; i < n; i++) {
        if (want > 0 && d < want) { d++; continue; }
        const int room = total - d > 1 ? total - d : 1;
        if (total > 0 && pool > total - d && p >= room) { none++; continue; }
        p++;
    }
}

int main() {
    const int pools[] = {1, 4, 8, 14, 20, 32}, totals[] = {1, 8, 25, 64}, settings[] = {AUTO, 0, 1, 12, 16};
    for (int eff : pools) {
        // the pool the environment shows is the effective one, or -- the library wrote its own default too late -- 20 above it
        const int envs[] = {eff, eff < OWN_POOL ? OWN_POOL : eff};
        for (int env : envs) for (int total : totals) for (int setting : settings) {
            const int w = wish(setting, eff);
            CHECK(w >= 0 && w <= MAX_DEDICATED, "wish %d", w);
            if (setting == AUTO) {
                CHECK(w == (eff >= OWN_POOL ? 0 : (OWN_POOL - eff > AUTO_MAX ? AUTO_MAX : OWN_POOL - eff)), "auto wish %d at pool %d", w, eff);
                if (eff >= OWN_POOL) CHECK(w == 0, "auto must be off at pool %d", eff);
            } else CHECK(w == setting, "explicit %d became %d", setting, w);
            // streams already made: every state the invariant allows (and that a run could have reached under another setting)
            for (int d0 = 0; d0 <= MAX_DEDICATED; d0++) for (int p0 = 0; p0 <= 40; p0++) {
                if (d0 + imin(env, p0) > total) continue;
                int d = d0, p = p0, refused = 0;
                for (int i = 0; i < 48; i++) {
                    const Kind k = next_stream(eff, env, total, setting, d, p);
                    if (k == DEDICATED) d++; else if (k == POOLED) p++; else refused++;
                    CHECK(d + imin(env, p) <= total, "invariant: eff %d env %d total %d setting %d d %d p %d", eff, env, total, setting, d, p);
                    if (k == DEDICATED) CHECK(d <= w, "more dedicated (%d) than wished (%d)", d, w);
                    if (k == NONE) CHECK(d + imin(env, p + 1) > total, "refused with room left: d %d p %d total %d", d, p, total);
                }
                if (setting == 0 || w == 0) CHECK(d == d0, "off, yet %d dedicated streams were made", d - d0);
                if (d0 == 0 && p0 == 0) CHECK(p >= 1, "not even one stream: eff %d env %d total %d setting %d", eff, env, total, setting);
            }
            // explicit settings behave as before wherever the environment tells the truth about the pool
            if (setting != AUTO && env == eff) {
                int od, op, on, d = 0, p = 0, none = 0;
                old_rule(env, total, setting, 48, od, op, on);
                for (int i = 0; i < 48; i++) {
                    const Kind k = next_stream(eff, env, total, setting, d, p);
                    if (k == DEDICATED) d++; else if (k == POOLED) p++; else none++;
                }
                CHECK(d == od && p == op && none == on, "explicit %d at pool %d total %d: %d/%d/%d, before %d/%d/%d", setting, env, total, d, p, none, od, op, on);
            }
        }
    }
    // an unknown budget (total 0) cuts nothing
    CHECK(next_stream(4, 4, 0, 12, 11, 100) == DEDICATED && next_stream(4, 4, 0, 12, 12, 100) == POOLED, "unknown budget");
    // the cases of the design: a late-loaded process (the environment says 20, the runtime uses 4) is no longer cut to total - 20
    { int d = 0, p = 0; for (int i = 0; i < 19; i++) { const Kind k = next_stream(4, 20, 25, 12, d, p); if (k == DEDICATED) d++; else if (k == POOLED) p++; }
      CHECK(d == 12 && p == 7, "late load, 12 asked: %d dedicated, %d pooled", d, p); }
    { int d = 0, p = 0; for (int i = 0; i < 19; i++) { const Kind k = next_stream(4, 4, 25, AUTO, d, p); if (k == DEDICATED) d++; else if (k == POOLED) p++; }
      CHECK(d == 12 && p == 7, "pool 4, automatic: %d dedicated, %d pooled", d, p); }
    { int d = 0, p = 0; for (int i = 0; i < 19; i++) { const Kind k = next_stream(14, 14, 25, AUTO, d, p); if (k == DEDICATED) d++; else if (k == POOLED) p++; }
      CHECK(d == 6 && p == 13, "pool 14, automatic: %d dedicated, %d pooled", d, p); }
    // what was found at load -> effective pool
    CHECK(load_pool(true, 4, RT_STARTED) == 4 && load_pool(true, 14, RT_NOT_STARTED) == 14 && load_pool(true, 0, RT_UNKNOWN) == 4, "variable set");
    CHECK(load_pool(false, 0, RT_NOT_STARTED) == 20 && load_pool(false, 0, RT_STARTED) == 4 && load_pool(false, 0, RT_UNKNOWN) == 4, "variable absent");
    std::printf("all checks passed (%ld)\n", checks);
    return 0;
}
