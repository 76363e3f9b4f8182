// search_internal.h — what the translation units of libkamisearch.so share: the error slot behind
// ks_last_error and the synthetic evaluator of the reference harness (`kami_ref mcts`, test infrastructure).
#pragma once
#include "mcts.h"

#include <cstdint>
#include <string>

namespace kami::detail {

int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));      // sets ks_last_error's text, returns 1

inline uint64_t fnv1a(const std::string& s)
{
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
    return h;
}
inline uint64_t splitmix(uint64_t x)
{
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// FNV-1a of the leaf position's FEN: the evaluator sees the leaf, so the path is replayed on the tree's environment
inline uint64_t leaf_hash(MCTS& tree, const MCTS::Leaf& leaf)
{
    Env& e = tree.get_env();
    for (size_t d = 1; d < leaf.path.size(); ++d) e.push(leaf.path[d]->action);
    const uint64_t h = fnv1a(e.print());
    for (size_t d = 1; d < leaf.path.size(); ++d) e.pop();
    return h;
}

// a full policy row and a value out of the hash `h`, reduced to the leaf's legal actions as MCTS::expand does
// (mcts.h:273-276); `policy` is PSIZE floats of scratch
inline void synthetic_eval(uint64_t h, const std::vector<int>& actions, float* policy, float* priors, float* value)
{
    double sum = 0.0;
    for (int a = 0; a < PSIZE; ++a) { policy[a] = (float)(splitmix(h + (uint64_t)a) % 16777213ull + 1); sum += policy[a]; }
    for (int a = 0; a < PSIZE; ++a) policy[a] = (float)(policy[a] / sum);
    *value = ((float)(splitmix(h ^ 0x7777) % 2001) - 1000.0f) / 1000.0f;
    float ptotal = 0.0f;
    for (int a : actions) ptotal += policy[a];
    for (size_t i = 0; i < actions.size(); ++i) priors[i] = policy[actions[i]] / ptotal;
}

}  // namespace kami::detail
