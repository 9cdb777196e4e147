// Bookkeeping of the job-local key cache (bbs_ctx_set_job_key_cache; job_form.hpp JobKeys, DESIGN.md 8 "Job-local key cache"):
// which compressed key string lives in which slot of ONE generation of the cache, which slots are free, which are pinned by
// jobs, which unpinned slot was used longest ago.  Host code only -- no device call, no HIP type: the device arrays, the
// events and the mutex belong to the caller (runtime.hpp Ctx::KeyCacheGen; every call here is made under the context's mutex).
// tests/cpp/key_cache_model.cpp drives this header alone against a naive model.
//
// A slot is FREE, CLAIMED or READY.  plan() looks up the keys of one job, all or nothing: a hit pins a READY slot, a miss claims a
// slot (free list first, then the unpinned READY slot used longest ago -- an eviction) and enters its string at once.  A CLAIMED
// slot belongs to the upload that is still being put together: its entry is not on its way to the device yet, so a plan of
// ANOTHER job that meets it does not hit it -- that job is bypassed.  commit() (the publishing kernel has been enqueued) makes
// the claimed slots READY: from then on they are hits, ordered on the device by the slot's event.  rollback() (the upload failed
// before that) gives the claimed slots back and removes their strings; nobody else can have named them.  release() (the job is
// freed) drops the job's pins.  The lookup key is the WHOLE string, compared in full: two strings never share a slot.
#pragma once
#include <cstddef>
#include <cstdint>
#include <set>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace bbs {

struct KeyCacheCounters {
    uint64_t hits = 0, misses = 0, evictions = 0, bypassed_jobs = 0;
};

// what plan() decided for one job
struct KeyCachePlan {
    std::vector<uint32_t> slot_of;       // [n_keys] slot of job key k
    std::vector<uint32_t> miss_key;      // job key of miss t: the first place its string stands at
    std::vector<uint32_t> miss_slot;     // slot_of[miss_key[t]]: the slots this job claimed
    std::vector<uint32_t> hit_slots;     // the distinct READY slots this job pinned
    uint32_t hits = 0, misses = 0;
    bool planned = false;                // plan() succeeded: the job holds pins
    bool committed = false;
};

class KeyCacheBook {
public:
    KeyCacheBook(size_t capacity, size_t key_bytes) : cap_(capacity), kb_(key_bytes), slots_(capacity) {
        free_.reserve(capacity);
        for (size_t s = capacity; s-- > 0;) free_.push_back((uint32_t)s);        // slot 0 is handed out first
    }
    size_t capacity() const { return cap_; }
    size_t key_bytes() const { return kb_; }
    size_t resident() const { return cap_ - free_.size(); }
    size_t pinned() const { return n_pinned_; }

    // The keys of one job: n_keys strings of key_bytes() each.  false: the job is bypassed and NOTHING has changed -- more keys
    // than slots, a string another upload has claimed and not yet committed, or more misses than free and evictable slots.
    // true: p is filled, every slot it names is pinned, hits and misses are counted (hits + misses == n_keys).
    bool plan(const uint8_t* octets, size_t n_keys, KeyCachePlan& p, KeyCacheCounters& c) {
        p = KeyCachePlan{};
        if (n_keys > cap_) return false;
        constexpr uint32_t NEW = 0x80000000u;                 // slot_of while planning: NEW | t = miss t, not placed yet
        std::unordered_map<std::string, uint32_t> fresh;      // strings of this call that are in no slot: -> miss number
        std::vector<std::string> miss_str;
        size_t hit_unpinned = 0;                              // distinct READY slots this job hits that nobody pins yet
        p.slot_of.resize(n_keys);
        for (size_t k = 0; k < n_keys; k++) {
            std::string s(reinterpret_cast<const char*>(octets) + k * kb_, kb_);
            const auto it = map_.find(s);
            if (it != map_.end()) {
                Slot& sl = slots_[it->second];
                if (sl.state != READY) { unmark(p); p = KeyCachePlan{}; return false; }
                if (!sl.mark) { sl.mark = true; p.hit_slots.push_back(it->second); if (!sl.pins) hit_unpinned++; }
                p.slot_of[k] = it->second;
                p.hits++;
                continue;
            }
            const auto f = fresh.find(s);
            if (f != fresh.end()) { p.slot_of[k] = NEW | f->second; p.hits++; continue; }
            const uint32_t t = (uint32_t)p.miss_key.size();
            fresh.emplace(s, t);
            miss_str.push_back(std::move(s));
            p.miss_key.push_back((uint32_t)k);
            p.slot_of[k] = NEW | t;
            p.misses++;
        }
        unmark(p);
        if (p.miss_key.size() > free_.size() + (lru_.size() - hit_unpinned)) { p = KeyCachePlan{}; return false; }
        // from here on nothing fails.  The hits first: a slot this job reads is in use, never its own victim
        for (const uint32_t s : p.hit_slots) pin(s);
        p.miss_slot.resize(p.miss_key.size());
        for (size_t t = 0; t < p.miss_key.size(); t++) {
            uint32_t s;
            if (!free_.empty()) { s = free_.back(); free_.pop_back(); }
            else {
                s = lru_.begin()->second;
                lru_.erase(lru_.begin());
                map_.erase(slots_[s].str);
                c.evictions++;
            }
            Slot& sl = slots_[s];
            sl.str = std::move(miss_str[t]);
            sl.state = CLAIMED;
            sl.pins = 1;
            sl.tick = ++clock_;
            n_pinned_++;
            map_.emplace(sl.str, s);
            p.miss_slot[t] = s;
        }
        for (size_t k = 0; k < n_keys; k++)
            if (p.slot_of[k] & NEW) p.slot_of[k] = p.miss_slot[p.slot_of[k] & ~NEW];
        c.hits += p.hits;
        c.misses += p.misses;
        p.planned = true;
        return true;
    }
    // the entries of the claimed slots are on their way: hits from now on
    void commit(KeyCachePlan& p) {
        if (!p.planned || p.committed) return;
        for (const uint32_t s : p.miss_slot) slots_[s].state = READY;
        p.committed = true;
    }
    // the job is gone.  Committed: its pins are dropped.  Not committed: its claimed slots go back to the free list and their
    // strings leave the map (the misses it counted stay counted: they were looked up); the pins of its hits are dropped.
    void release(KeyCachePlan& p) {
        if (!p.planned) return;
        for (const uint32_t s : p.hit_slots) unpin(s);
        for (const uint32_t s : p.miss_slot) {
            if (p.committed) { unpin(s); continue; }
            Slot& sl = slots_[s];
            map_.erase(sl.str);
            sl = Slot{};
            n_pinned_--;
            free_.push_back(s);
        }
        p.planned = false;
    }
    // the READY slot of a string (bbs_selftest_job_key_cache_entries)
    bool find_ready(const uint8_t* octets, uint32_t& slot) const {
        const auto it = map_.find(std::string(reinterpret_cast<const char*>(octets), kb_));
        if (it == map_.end() || slots_[it->second].state != READY) return false;
        slot = it->second;
        return true;
    }
    // for the model test: the whole state, checked against itself
    bool consistent() const {
        size_t res = 0, pinned = 0, unpinned_ready = 0;
        for (size_t s = 0; s < cap_; s++) {
            const Slot& sl = slots_[s];
            if (sl.state == FREE) { if (sl.pins || !sl.str.empty()) return false; continue; }
            res++;
            const auto it = map_.find(sl.str);
            if (it == map_.end() || it->second != s || sl.str.size() != kb_) return false;
            if (sl.state == CLAIMED && sl.pins != 1) return false;
            if (sl.pins) pinned++;
            else { unpinned_ready++; if (!lru_.count({sl.tick, (uint32_t)s})) return false; }
        }
        return res == map_.size() && res == resident() && pinned == n_pinned_ && unpinned_ready == lru_.size();
    }

private:
    enum State : uint8_t { FREE, CLAIMED, READY };
    struct Slot {
        std::string str;
        State state = FREE;
        bool mark = false;               // inside plan(): already among this job's hits
        uint32_t pins = 0;               // jobs that name the slot
        uint64_t tick = 0;               // last use: a hit, or the claim
    };
    void unmark(const KeyCachePlan& p) { for (const uint32_t s : p.hit_slots) slots_[s].mark = false; }
    void pin(uint32_t s) {
        Slot& sl = slots_[s];
        if (!sl.pins++) { lru_.erase({sl.tick, s}); n_pinned_++; }
        sl.tick = ++clock_;
    }
    void unpin(uint32_t s) {
        Slot& sl = slots_[s];
        if (!--sl.pins) { lru_.insert({sl.tick, s}); n_pinned_--; }
    }
    size_t cap_, kb_;
    std::vector<Slot> slots_;
    std::vector<uint32_t> free_;
    std::unordered_map<std::string, uint32_t> map_;
    std::set<std::pair<uint64_t, uint32_t>> lru_;      // the unpinned READY slots, longest unused first
    size_t n_pinned_ = 0;
    uint64_t clock_ = 0;
};

}  // namespace bbs
