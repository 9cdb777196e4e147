// The bookkeeping of the job-local key cache (bbs_sign_amd/csrc/key_cache.hpp) alone, against a naive model: a few thousand
// random operations -- a job's plan (lookup and insert), commit, rollback of an upload that failed, release of a finished job, a
// change of generation -- and after every one the book's answers, counters and internal consistency against a model that keeps
// plain lists and scans them.  Plain C++: tests/test_key_cache_model.py builds it with the address and undefined-behaviour
// sanitizers and runs it.
#include "../../bbs_sign_amd/csrc/key_cache.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>

using namespace bbs;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); if (++failures > 20) std::exit(1); } } while (0)

static constexpr size_t KB = 12;          // bytes of a key string here (the library: 64 or 96)

// key id -> its string; ids that differ in ONE byte somewhere (a digest of a prefix would confuse them)
static std::string key_string(uint32_t id) {
    std::string s(KB, '\x5a');
    s[KB - 1] = (char)(id & 0xff);
    s[KB / 2] = (char)((id >> 8) & 0xff);
    s[0] = (char)((id >> 16) & 0xff);
    return s;
}

// The model: what every slot holds, by scanning.
struct Model {
    struct Slot { bool used = false, ready = false; std::string str; unsigned pins = 0; uint64_t tick = 0; };
    std::vector<Slot> slots;
    std::vector<uint32_t> free_order;     // the book hands out slot 0 first, a slot given back is reused first
    uint64_t clock = 0;
    KeyCacheCounters c;
    explicit Model(size_t cap) : slots(cap) { for (size_t s = cap; s-- > 0;) free_order.push_back((uint32_t)s); }
    int find(const std::string& s) const {
        for (size_t i = 0; i < slots.size(); i++) if (slots[i].used && slots[i].str == s) return (int)i;
        return -1;
    }
    struct Job { std::vector<uint32_t> slot_of, hit_slots, miss_slot; uint32_t hits = 0, misses = 0; bool committed = false; };
    bool plan(const std::vector<uint32_t>& ids, Job& j) {
        j = Job{};
        if (ids.size() > slots.size()) return false;
        std::vector<std::string> fresh;
        std::vector<int> want(ids.size());             // >= 0 slot, < 0: -(1 + miss number)
        size_t hit_unpinned = 0;
        std::vector<uint32_t> hit_slots;
        uint32_t hits = 0;
        for (size_t k = 0; k < ids.size(); k++) {
            const std::string s = key_string(ids[k]);
            const int at = find(s);
            if (at >= 0) {
                if (!slots[at].ready) return false;
                if (std::find(hit_slots.begin(), hit_slots.end(), (uint32_t)at) == hit_slots.end()) {
                    hit_slots.push_back((uint32_t)at);
                    if (!slots[at].pins) hit_unpinned++;
                }
                want[k] = at; hits++;
                continue;
            }
            const auto f = std::find(fresh.begin(), fresh.end(), s);
            if (f != fresh.end()) { want[k] = -(1 + (int)(f - fresh.begin())); hits++; continue; }
            fresh.push_back(s);
            want[k] = -(int)fresh.size();
        }
        size_t evictable = 0;
        for (const Slot& sl : slots) if (sl.used && sl.ready && !sl.pins) evictable++;
        if (fresh.size() > free_order.size() + (evictable - hit_unpinned)) return false;
        for (uint32_t s : hit_slots) { slots[s].pins++; slots[s].tick = ++clock; }
        for (const std::string& s : fresh) {
            uint32_t at;
            if (!free_order.empty()) { at = free_order.back(); free_order.pop_back(); }
            else {
                int victim = -1;
                for (size_t i = 0; i < slots.size(); i++)
                    if (slots[i].used && slots[i].ready && !slots[i].pins && (victim < 0 || slots[i].tick < slots[victim].tick)) victim = (int)i;
                at = (uint32_t)victim;
                c.evictions++;
            }
            slots[at] = Slot{true, false, s, 1, ++clock};
            j.miss_slot.push_back(at);
        }
        j.hit_slots = hit_slots;
        j.slot_of.resize(ids.size());
        for (size_t k = 0; k < ids.size(); k++) j.slot_of[k] = want[k] >= 0 ? (uint32_t)want[k] : j.miss_slot[-want[k] - 1];
        j.hits = hits; j.misses = (uint32_t)fresh.size();
        c.hits += j.hits; c.misses += j.misses;
        return true;
    }
    void commit(Job& j) { for (uint32_t s : j.miss_slot) slots[s].ready = true; j.committed = true; }
    void release(Job& j) {
        for (uint32_t s : j.hit_slots) slots[s].pins--;
        for (uint32_t s : j.miss_slot) {
            if (j.committed) { slots[s].pins--; continue; }
            slots[s] = Slot{};
            free_order.push_back(s);
        }
    }
    size_t resident() const { size_t r = 0; for (const Slot& s : slots) r += s.used; return r; }
    size_t pinned() const { size_t r = 0; for (const Slot& s : slots) r += s.pins != 0; return r; }
};

struct LiveJob { KeyCachePlan plan; Model::Job mj; std::vector<uint32_t> ids; };

static void compare(const KeyCacheBook& book, const KeyCacheCounters& c, const Model& m, uint32_t id_space) {
    CHECK(book.consistent());
    CHECK(book.resident() == m.resident());
    CHECK(book.pinned() == m.pinned());
    CHECK(c.hits == m.c.hits && c.misses == m.c.misses && c.evictions == m.c.evictions && c.bypassed_jobs == m.c.bypassed_jobs);
    for (uint32_t id = 0; id < id_space; id++) {
        const std::string s = key_string(id);
        uint32_t slot = 0xdeadbeef;
        const bool got = book.find_ready(reinterpret_cast<const uint8_t*>(s.data()), slot);
        const int at = m.find(s);
        CHECK(got == (at >= 0 && m.slots[at].ready));
        if (got) CHECK((int)slot == at);
    }
}

static void run(uint32_t seed, size_t cap, uint32_t id_space, int n_ops) {
    std::mt19937 rng(seed);
    auto book = std::make_unique<KeyCacheBook>(cap, KB);
    auto model = std::make_unique<Model>(cap);
    KeyCacheCounters c;
    std::vector<std::unique_ptr<LiveJob>> live;           // planned, not yet released (committed or not)
    // the jobs of a generation that was replaced keep THEIR book alive and release into it
    struct Old { std::unique_ptr<KeyCacheBook> book; std::unique_ptr<Model> model; std::vector<std::unique_ptr<LiveJob>> live; KeyCacheCounters c; };
    std::vector<Old> old;
    for (int op = 0; op < n_ops; op++) {
        const unsigned what = rng() % 100;
        if (what < 45) {                                   // a job's plan
            const size_t nk = rng() % (cap + 3);           // (now and then more keys than slots)
            auto j = std::make_unique<LiveJob>();
            for (size_t k = 0; k < nk; k++) j->ids.push_back(rng() % id_space);
            std::string oct;
            for (uint32_t id : j->ids) oct += key_string(id);
            const bool ok = book->plan(reinterpret_cast<const uint8_t*>(oct.data()), nk, j->plan, c);
            const bool mok = model->plan(j->ids, j->mj);
            CHECK(ok == mok);
            if (!ok) {
                c.bypassed_jobs++; model->c.bypassed_jobs++;
                CHECK(!j->plan.planned && j->plan.slot_of.empty());
            } else {
                CHECK(j->plan.hits + j->plan.misses == nk);
                CHECK(j->plan.hits == j->mj.hits && j->plan.misses == j->mj.misses);
                CHECK(j->plan.slot_of == j->mj.slot_of);
                CHECK(j->plan.miss_slot == j->mj.miss_slot);
                for (size_t k = 0; k < nk; k++) {
                    CHECK(j->plan.slot_of[k] < cap);
                    for (size_t q = 0; q < k; q++) CHECK((j->ids[k] == j->ids[q]) == (j->plan.slot_of[k] == j->plan.slot_of[q]));
                }
                for (size_t t = 0; t < j->plan.miss_key.size(); t++) CHECK(j->plan.slot_of[j->plan.miss_key[t]] == j->plan.miss_slot[t]);
                live.push_back(std::move(j));
            }
        } else if (what < 65 && !live.empty()) {           // the publishing kernel of a planned job has been enqueued
            LiveJob& j = *live[rng() % live.size()];
            if (!j.plan.committed) { book->commit(j.plan); model->commit(j.mj); }
        } else if (what < 95 && !live.empty()) {           // a job goes: released if committed, rolled back if not
            const size_t at = rng() % live.size();
            book->release(live[at]->plan);
            model->release(live[at]->mj);
            book->release(live[at]->plan);                 // (a second release is nothing)
            live.erase(live.begin() + (long)at);
        } else if (what >= 98) {                           // a change of generation: a new, empty book; the old jobs keep theirs
            old.push_back(Old{std::move(book), std::move(model), std::move(live), c});
            live.clear();
            book = std::make_unique<KeyCacheBook>(cap, KB);
            model = std::make_unique<Model>(cap);
            model->c = c;                                  // the counters are the context's: they go on
            CHECK(book->resident() == 0 && book->pinned() == 0);
        } else if (!old.empty()) {                         // a job of an old generation is freed
            Old& o = old[rng() % old.size()];
            if (!o.live.empty()) {
                o.book->release(o.live.back()->plan);
                o.model->release(o.live.back()->mj);
                o.live.pop_back();
                CHECK(o.book->consistent() && o.book->pinned() == o.model->pinned() && o.book->resident() == o.model->resident());
            }
        }
        compare(*book, c, *model, id_space);
    }
    // everything is freed: nothing stays pinned, nothing claimed stays behind
    for (auto& j : live) { book->release(j->plan); model->release(j->mj); }
    compare(*book, c, *model, id_space);
    CHECK(book->pinned() == 0);
    std::printf("seed %u: %d operations, %llu hits, %llu misses, %llu evictions, %llu bypassed jobs, %zu generations\n", seed, n_ops,
                (unsigned long long)c.hits, (unsigned long long)c.misses, (unsigned long long)c.evictions, (unsigned long long)c.bypassed_jobs, old.size() + 1);
    for (Old& o : old) {
        for (auto& j : o.live) o.book->release(j->plan);
        CHECK(o.book->consistent() && o.book->pinned() == 0);
    }
}

// the shapes the issue names, by hand
static void fixed_cases() {
    auto oct = [](std::initializer_list<uint32_t> ids) { std::string s; for (uint32_t id : ids) s += key_string(id); return s; };
    auto plan = [&](KeyCacheBook& b, KeyCacheCounters& c, std::initializer_list<uint32_t> ids, KeyCachePlan& p) {
        const std::string s = oct(ids);
        return b.plan(reinterpret_cast<const uint8_t*>(s.data()), ids.size(), p, c);
    };
    {   // eviction: capacity 4; A {0,1,2} freed; B {3,4,0}: one free slot, one eviction, not of key 0; C {1,2}: one hit, one miss
        KeyCacheBook b(4, KB); KeyCacheCounters c; KeyCachePlan A, B, C;
        CHECK(plan(b, c, {0, 1, 2}, A) && A.misses == 3 && A.hits == 0);
        b.commit(A); b.release(A);
        CHECK(plan(b, c, {3, 4, 0}, B) && B.hits == 1 && B.misses == 2 && c.evictions == 1);
        CHECK(B.slot_of[2] == A.slot_of[0]);
        b.commit(B); b.release(B);
        CHECK(plan(b, c, {1, 2}, C) && C.hits == 1 && C.misses == 1 && c.evictions == 2);
        b.commit(C); b.release(C);
        CHECK(b.pinned() == 0 && b.resident() == 4);
    }
    {   // pins and bypass: capacity 3; A {0,1,2} alive; B {3} is bypassed; after A goes, {3} is a miss with an eviction
        KeyCacheBook b(3, KB); KeyCacheCounters c; KeyCachePlan A, B, D;
        CHECK(plan(b, c, {0, 1, 2}, A));
        b.commit(A);
        CHECK(!plan(b, c, {3}, B) && b.pinned() == 3 && c.misses == 3);
        b.release(A);
        CHECK(plan(b, c, {3}, B) && B.misses == 1 && c.evictions == 1);
        CHECK(!plan(b, c, {5, 6, 7, 8}, D));               // more keys than slots
        b.commit(B); b.release(B);
    }
    {   // the same string twice in one call: one miss, then a hit, one slot; a claimed string is no hit for another job
        KeyCacheBook b(4, KB); KeyCacheCounters c; KeyCachePlan A, B;
        CHECK(plan(b, c, {7, 8, 7}, A) && A.misses == 2 && A.hits == 1 && A.slot_of[0] == A.slot_of[2] && A.slot_of[0] != A.slot_of[1]);
        CHECK(!plan(b, c, {8}, B));                        // claimed by A, not committed: B is bypassed
        CHECK(plan(b, c, {9}, B) && B.misses == 1);        // (a stranger is served)
        b.release(A);                                      // A's upload failed: rollback
        CHECK(b.resident() == 1 && b.consistent());
        uint32_t s;
        const std::string k7 = key_string(7);
        CHECK(!b.find_ready(reinterpret_cast<const uint8_t*>(k7.data()), s));
        b.commit(B); b.release(B);
    }
}

int main() {
    fixed_cases();
    run(1, 1, 3, 400);
    run(2, 4, 9, 1500);
    run(3, 8, 12, 1500);
    run(4, 16, 64, 1500);
    run(5, 5, 300, 800);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
