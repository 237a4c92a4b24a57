// q3_lookup.h -- the prompt-lookup drafter of q3_generate_lookup (host only, no device code).
//
// Definition (include/qwen3_hip.h section 2c): over the sequence S, with g = ngram, take the LARGEST i < |S| - g with
// S[i..i+g) == S[|S|-g..|S|); the draft is S[i+g .. min(i+g+draft_len, |S|)).  No such i, |S| <= g or an empty draft: no draft.
//
// lookup_draft_rescan is that sentence in code (q3_lookup_draft).  LookupIndex answers the same question while S grows by
// one token at a time, in O(1) amortised per token: a polynomial prefix hash gives the hash of any window in O(1), every
// window that has a successor is entered into a hash table whose buckets chain the window starts in descending order, and
// a query walks the bucket of the suffix window from the latest start, comparing tokens (a hash collision is skipped, never
// believed).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

namespace q3 {

inline size_t lookup_draft_rescan(const int32_t* seq, size_t n, int ngram, int draft_len, int32_t* draft) {
    if (!seq || ngram < 1 || draft_len < 1 || n <= (size_t)ngram) return 0;
    const size_t g = (size_t)ngram;
    const int32_t* suffix = seq + (n - g);
    for (size_t i = n - g; i-- > 0;) {
        bool same = true;
        for (size_t k = 0; k < g && same; ++k) same = seq[i + k] == suffix[k];
        if (!same) continue;
        size_t len = n - (i + g);
        if (len > (size_t)draft_len) len = (size_t)draft_len;
        for (size_t k = 0; k < len; ++k) draft[k] = seq[i + g + k];
        return len;
    }
    return 0;
}

class LookupIndex {
public:
    explicit LookupIndex(int ngram) : g_(ngram < 1 ? 1 : (size_t)ngram), pow_g_(1) {
        for (size_t k = 0; k < g_; ++k) pow_g_ *= kBase;
        prefix_.push_back(0);
    }
    void reserve(size_t n) {
        seq_.reserve(n);
        prefix_.reserve(n + 1);
        prev_.reserve(n);
        head_.reserve(n);
    }
    void push(int32_t token) {
        seq_.push_back(token);
        prefix_.push_back(prefix_.back() * kBase + ((uint64_t)(uint32_t)token + 1));
        prev_.push_back(kNone);
        // the window that has just gained a successor: start i = |S| - g - 1 (the suffix window itself is never a candidate)
        const size_t n = seq_.size();
        if (n > g_) {
            const size_t i = n - g_ - 1;
            auto it = head_.find(window_hash(i));
            if (it == head_.end()) head_.emplace(window_hash(i), (uint32_t)i);
            else { prev_[i] = it->second; it->second = (uint32_t)i; }
        }
    }
    size_t size() const { return seq_.size(); }
    size_t draft(int draft_len, int32_t* out) const {
        const size_t n = seq_.size();
        if (draft_len < 1 || n <= g_) return 0;
        auto it = head_.find(window_hash(n - g_));
        if (it == head_.end()) return 0;
        for (uint32_t i = it->second; i != kNone; i = prev_[i]) {
            bool same = true;
            for (size_t k = 0; k < g_ && same; ++k) same = seq_[i + k] == seq_[n - g_ + k];
            if (!same) continue;
            size_t len = n - (i + g_);
            if (len > (size_t)draft_len) len = (size_t)draft_len;
            for (size_t k = 0; k < len; ++k) out[k] = seq_[i + g_ + k];
            return len;
        }
        return 0;
    }

private:
    static constexpr uint64_t kBase = 0x9E3779B97F4A7C15ull;        // odd: multiplication by it is a bijection modulo 2^64
    static constexpr uint32_t kNone = 0xffffffffu;
    uint64_t window_hash(size_t i) const { return prefix_[i + g_] - prefix_[i] * pow_g_; }
    size_t g_;
    uint64_t pow_g_;
    std::vector<int32_t> seq_;
    std::vector<uint64_t> prefix_;       // prefix_[m] = hash of S[0..m)
    std::vector<uint32_t> prev_;         // prev_[i]: the next smaller window start in the same bucket
    std::unordered_map<uint64_t, uint32_t> head_;   // window hash -> largest start entered so far
};

}  // namespace q3
