// match.cpp — ks_match_run / ks_match_synthetic (include/kami_search.h): kami::eval (kami/evaluate.cpp:10-160) on the
// machinery of the self-play pool.  "evaluate_games" trees, one per game, are shared out to host workers; a tree's leaves
// go to the model whose turn it is at that tree's ROOT; each worker's round is one batch per model, through the engine's
// queue when asked to.  The verdict is the reference's arithmetic replayed in game-index order, so it does not depend on
// which worker finishes first.
#include "kami_search.h"
#include "mcts.h"
#include "search_internal.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

using namespace kami;
using kami::detail::fail;

namespace {

struct Game {
    std::unique_ptr<MCTS> tree;
    std::vector<MCTS::Leaf> leaves;     // leaves[0 .. nleaves) are in flight, as in the pool
    int nleaves = 0;
    std::vector<int32_t> moves;
    float cturn = 1.0f;                 // Env::turn() of the candidate's colour (+1: white)
    float result = 0.0f;                // Env::terminal's value once done
    bool done = false;                  // (the owning worker's; `finished` below is the shared one)
};

struct Verdict { bool decided = false, accepted = false; float score = 0.0f; int counted = 0; };

struct Match {
    kh_engine* eng[2] = { nullptr, nullptr };       // [0] current, [1] candidate; both null: the synthetic evaluators
    uint64_t salt[2] = { 0, 0 };
    ks_match_config cfg;
    std::vector<Game> games;
    std::mutex mu;                                  // finished, verdict, error
    std::vector<char> finished;
    Verdict verdict;
    std::string error;
    std::atomic<bool> stop{ false }, failed{ false }, skipped{ false };
    std::atomic<int64_t> evals[2], batches{ 0 }, moves{ 0 };
    Match() { evals[0] = 0; evals[1] = 0; }
};

// evaluate.cpp:100-125 over the finished prefix of the table
Verdict replay(const Match& m)
{
    Verdict v;
    const int n = m.cfg.games;
    const float target = (float)((n * m.cfg.target_pct) / 100);
    for (int k = 0; k < n && m.finished[k]; ++k) {
        v.score += m.games[k].result * m.games[k].cturn / 2.0f + 0.5f;
        v.counted += 1;
        if (v.score + (n - v.counted) < target) { v.decided = true; v.accepted = false; return v; }
        if (v.score >= target && v.counted < n) { v.decided = true; v.accepted = true; return v; }
    }
    if (v.counted == n) { v.decided = true; v.accepted = v.score * 100 / n >= m.cfg.target_pct; }
    return v;
}

// the tree has its visits: play the visit maximum (evaluate.cpp:95-99)
void play_move(Match& m, Game& g, int gi)
{
    MCTS& tree = *g.tree;
    const int a = tree.pick();
    g.moves.push_back(a);
    tree.push(a);
    m.moves += 1;
    float value;
    if (!tree.get_env().terminal(&value)) return;
    g.result = value;
    g.done = true;
    std::lock_guard<std::mutex> lk(m.mu);
    m.finished[gi] = 1;
    m.verdict = replay(m);
    if (m.verdict.decided && m.cfg.early_stop) m.stop = true;
}

// One round of a worker over a range of its trees, LeafSet's structure with the rows split by evaluator.
struct Half {
    std::vector<kh_board> boards;
    std::vector<int32_t> offsets, actions;
    std::vector<float> priors, values;
    std::vector<std::pair<int, int>> owner;         // (game, leaf slot) of each row
    int64_t ticket = 0;
    bool in_flight = false;
    void clear() { boards.clear(); offsets.assign(1, 0); actions.clear(); owner.clear(); }
};

struct Set {
    int g0 = 0, g1 = 0;
    Half half[2];
    bool flying = false;

    int build(Match& m, int L)
    {
        half[0].clear(); half[1].clear();
        for (int gi = g0; gi < g1; ++gi) {
            Game& g = m.games[gi];
            if (g.done) continue;
            MCTS& tree = *g.tree;
            if ((int)g.leaves.size() < L) g.leaves.resize((size_t)L);
            g.nleaves = 0;
            for (;;) {
                if (g.nleaves == 0 && tree.n() >= m.cfg.nodes) {
                    play_move(m, g, gi);
                    if (g.done) break;
                    continue;
                }
                if (g.nleaves >= L || tree.n() + g.nleaves >= m.cfg.nodes) break;
                bool blocked = false;
                if (tree.select_leaf(&g.leaves[g.nleaves], &blocked)) { ++g.nleaves; continue; }
                if (blocked) break;
            }
            // the model whose turn it is at this tree's root evaluates its leaves (evaluate.cpp:68-92)
            Half& h = half[tree.get_env().turn() == g.cturn ? 1 : 0];
            for (int j = 0; j < g.nleaves; ++j) {
                h.boards.push_back(g.leaves[j].record);
                h.actions.insert(h.actions.end(), g.leaves[j].actions.begin(), g.leaves[j].actions.end());
                h.offsets.push_back((int32_t)h.actions.size());
                h.owner.emplace_back(gi, j);
            }
        }
        for (Half& h : half) { h.priors.resize(h.actions.size() + 1); h.values.resize(h.boards.size() + 1); }
        return (int)(half[0].boards.size() + half[1].boards.size());
    }

    void expand(Match& m)
    {
        for (int who = 0; who < 2; ++who) {
            Half& h = half[who];
            const int nb = (int)h.boards.size();
            for (int j = 0; j < nb; ++j) {
                Game& g = m.games[h.owner[j].first];
                g.tree->expand_leaf(g.leaves[h.owner[j].second], h.priors.data() + h.offsets[j], h.values[j]);
                if (h.owner[j].second + 1 == g.nleaves) g.nleaves = 0;
            }
            m.evals[who] += nb;
        }
    }
};

void engine_failed(const char* what) { throw std::runtime_error(std::string(what) + ": " + kh_last_error()); }

// One evaluator's rows of a round to its engine: through the queue when asked to and taken, by the synchronous call
// otherwise (a refused submission — the engine's outstanding tickets are shared with whoever else uses it — costs
// nothing but the overlap: the bits are the same).
void submit(Match& m, Half& h, int who)
{
    const int nb = (int)h.boards.size();
    if (nb == 0) return;
    m.batches += 1;
    if (m.cfg.pipeline >= 1 &&
        kh_submit_encode_infer_legal(m.eng[who], h.boards.data(), nb, h.offsets.data(), h.actions.data(), h.priors.data(), h.values.data(),
                                     &h.ticket) == KH_OK) {
        h.in_flight = true;
        return;
    }
    if (kh_encode_infer_legal(m.eng[who], h.boards.data(), nb, h.offsets.data(), h.actions.data(), h.priors.data(), h.values.data()) != KH_OK)
        engine_failed("kh_encode_infer_legal");
}

void wait(Match& m, Set& s)
{
    std::string err;                                    // both tickets are consumed whatever the first one says
    for (int who = 0; who < 2; ++who) {
        Half& h = s.half[who];
        if (!h.in_flight) continue;
        h.in_flight = false;
        if (kh_wait(m.eng[who], h.ticket) != KH_OK && err.empty()) err = kh_last_error();
    }
    if (!err.empty()) throw std::runtime_error("kh_encode_infer_legal: " + err);
}

void evaluate_synthetic(Match& m, Set& s, std::vector<float>& policy)
{
    for (int who = 0; who < 2; ++who) {
        Half& h = s.half[who];
        if (!h.boards.empty()) m.batches += 1;
        for (size_t j = 0; j < h.boards.size(); ++j) {
            Game& g = m.games[h.owner[j].first];
            const MCTS::Leaf& leaf = g.leaves[h.owner[j].second];
            const uint64_t hash = detail::leaf_hash(*g.tree, leaf) ^ detail::splitmix(m.salt[who]);
            detail::synthetic_eval(hash, leaf.actions, policy.data(), h.priors.data() + h.offsets[j], &h.values[j]);
        }
    }
}

void worker(Match& m, int g0, int g1)
{
    const int L = m.cfg.leaves_per_tree > 0 ? m.cfg.leaves_per_tree : 1;
    const bool synthetic = m.eng[0] == nullptr;
    // pipeline 2: the worker's trees in two sets, one on the device while the other is expanded and selected
    const int nsets = !synthetic && m.cfg.pipeline == 2 && g1 - g0 >= 2 ? 2 : 1;
    Set sets[2];
    for (int k = 0; k < nsets; ++k) {
        sets[k].g0 = g0 + (g1 - g0) * k / nsets;
        sets[k].g1 = g0 + (g1 - g0) * (k + 1) / nsets;
    }
    std::vector<float> policy(synthetic ? PSIZE : 0);
    // evaluate.cpp:53-59, once per round: somebody else installed this generation (or a later one) meanwhile
    auto halt = [&] {
        if (!synthetic && !m.stop && kh_generation(m.eng[0]) >= kh_generation(m.eng[1])) { m.skipped = true; m.stop = true; }
        return m.stop || m.failed;
    };
    try {
        bool live[2] = { true, nsets == 2 };
        for (int k = 0;; k = (k + 1) % nsets) {
            Set& s = sets[k];
            if (s.flying) { wait(m, s); s.flying = false; s.expand(m); }
            if (halt()) break;
            if (live[k]) {
                if (s.build(m, L) == 0) live[k] = false;       // every game of the set is over
                else if (synthetic) { evaluate_synthetic(m, s, policy); s.expand(m); }
                else {
                    submit(m, s.half[0], 0);                    // current, then candidate (evaluate.cpp:136-151)
                    submit(m, s.half[1], 1);
                    if (nsets == 2) s.flying = true;
                    else { wait(m, s); s.expand(m); }
                }
            }
            if (!live[0] && !live[1] && !sets[0].flying && !sets[1].flying) break;
        }
        for (Set& s : sets)
            if (s.flying) { wait(m, s); s.flying = false; s.expand(m); }
    } catch (std::exception& e) {
        // a failed engine call leaves no ticket un-waited and no leaf marked in a tree
        for (Set& s : sets)
            for (int who = 0; who < 2; ++who)
                if (s.half[who].in_flight) { s.half[who].in_flight = false; (void)kh_wait(m.eng[who], s.half[who].ticket); }
        for (int gi = g0; gi < g1; ++gi) {
            Game& g = m.games[gi];
            for (int j = 0; j < g.nleaves; ++j) g.tree->release_leaf(g.leaves[j]);
            g.nleaves = 0;
        }
        std::lock_guard<std::mutex> lk(m.mu);
        if (m.error.empty()) m.error = e.what();
        m.failed = true;
    }
}

int run(Match& m, const ks_match_config* cfg, ks_match_result* out, ks_match_game* games, int32_t* moves, int64_t moves_cap)
{
    if (!cfg || !out) return fail("null argument");
    if (cfg->games < 1 || cfg->threads < 1 || cfg->nodes < 2) return fail("games >= 1, threads >= 1, nodes >= 2 required");
    if (cfg->pipeline < 0 || cfg->pipeline > 2) return fail("pipeline is 0, 1 or 2");
    if (cfg->leaves_per_tree < 0 || cfg->leaves_per_tree > 64) return fail("leaves_per_tree in [0, 64]");
    if (moves && moves_cap < 0) return fail("moves_cap < 0");
    const auto t0 = std::chrono::steady_clock::now();
    m.cfg = *cfg;
    const int n = cfg->games, T = std::min(cfg->threads, n);
    m.games.resize((size_t)n);
    m.finished.assign((size_t)n, 0);
    for (int g = 0; g < n; ++g) {
        MCTSConfig mc;
        mc.cpuct = cfg->cpuct > 0 ? cfg->cpuct : 1.0f;
        mc.mcts_noise_weight = cfg->noise_weight;
        mc.seed = cfg->seed * 2654435761u + (unsigned)g;            // as the pool seeds its trees
        m.games[g].tree.reset(new MCTS(mc));
        const bool white = (g % 2 == 0) == (cfg->candidate_white_first != 0);
        m.games[g].cturn = white ? 1.0f : -1.0f;
    }
    std::vector<std::thread> th;
    for (int t = 0, g0 = 0; t < T; ++t) {                           // game g belongs to worker g * T / games
        int g1 = g0;
        while (g1 < n && (int)((int64_t)g1 * T / n) == t) ++g1;
        th.emplace_back(worker, std::ref(m), g0, g1);
        g0 = g1;
    }
    for (auto& x : th) x.join();
    if (m.failed) return fail("%s", m.error.c_str());

    const Verdict v = replay(m);
    *out = ks_match_result{};
    out->skipped = m.skipped ? 1 : 0;
    out->accepted = !m.skipped && v.decided && v.accepted ? 1 : 0;
    out->games_counted = v.counted;
    out->score = v.score;
    int64_t off = 0;
    for (int g = 0; g < n; ++g) {
        const Game& gm = m.games[g];
        const float for_candidate = gm.result * gm.cturn;
        if (gm.done) (for_candidate > 0 ? out->candidate_wins : for_candidate < 0 ? out->current_wins : out->draws) += 1;
        if (games) games[g] = ks_match_game{ gm.done ? 1 : 0, gm.cturn > 0 ? 1 : 0, (int32_t)gm.moves.size(), gm.done ? gm.result : 0.0f, (int32_t)off };
        if (moves) {
            if (off + (int64_t)gm.moves.size() > moves_cap) return fail("the move lists need more than moves_cap = %lld entries", (long long)moves_cap);
            std::copy(gm.moves.begin(), gm.moves.end(), moves + off);
        }
        off += (int64_t)gm.moves.size();
    }
    out->evals_current = m.evals[0];
    out->evals_candidate = m.evals[1];
    out->batches = m.batches;
    out->moves = m.moves;
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

}  // namespace

extern "C" {

int ks_match_run(kh_engine* current, kh_engine* candidate, const ks_match_config* cfg, ks_match_result* out, ks_match_game* games,
                 int32_t* moves, int64_t moves_cap)
{
    if (!current || !candidate) return fail("null engine");
    try {
        Match m;
        m.eng[0] = current;
        m.eng[1] = candidate;
        return run(m, cfg, out, games, moves, moves_cap);
    } catch (std::exception& e) {
        return fail("%s", e.what());
    }
}

int ks_match_synthetic(uint64_t salt_current, uint64_t salt_candidate, const ks_match_config* cfg, ks_match_result* out,
                       ks_match_game* games, int32_t* moves, int64_t moves_cap)
{
    try {
        Match m;
        m.salt[0] = salt_current;
        m.salt[1] = salt_candidate;
        return run(m, cfg, out, games, moves, moves_cap);
    } catch (std::exception& e) {
        return fail("%s", e.what());
    }
}

}  // extern "C"
