// replaybuffer.h — kami::ReplayBuffer with the reference's public methods (kami/replaybuffer.h:10-92):
// a fixed ring of (observation[obsize], mcts policy[psize], result) records under one mutex, uniform
// selection with replacement over the whole ring (written or not).  Records are stored interleaved,
// one contiguous row per record.
#ifndef KAMI_AMD_HOST_REPLAYBUFFER_H
#define KAMI_AMD_HOST_REPLAYBUFFER_H

#include "kami_hip.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <vector>

namespace kami {

class ReplayBuffer {
    const int obs_len, pol_len, capacity;
    const size_t row;                       // floats per record: observation, policy, result
    std::vector<float> ring;
    std::mutex lock;
    int head = 0;                           // next slot to write
    long added = 0;                         // records ever added (the reference's `total`)

public:
    ReplayBuffer(int obsize, int psize, int bufsize)
        : obs_len(obsize), pol_len(psize), capacity(bufsize), row((size_t)obsize + psize + 1), ring(row * (size_t)bufsize, 0.0f) {}

    int size() { return capacity; }
    long count() { return added; }

    void clear()
    {
        head = 0;
        added = 0;
    }

    void add(const float* input, const float* mcts, float result)
    {
        std::lock_guard<std::mutex> hold(lock);
        float* slot = ring.data() + row * (size_t)head;
        std::copy(input, input + obs_len, slot);
        std::copy(mcts, mcts + pol_len, slot + obs_len);
        slot[obs_len + pol_len] = result;
        head = (head + 1) % capacity;
        ++added;
    }

    // n draws with replacement over ALL slots (replaybuffer.h:61-84: duplicates and never-written slots included)
    void select_batch(float* dst_input, float* dst_mcts, float* dst_result, int n)
    {
        std::lock_guard<std::mutex> hold(lock);
        for (int k = 0; k < n; ++k) {
            const float* slot = ring.data() + row * (size_t)(rand() % capacity);
            std::copy(slot, slot + obs_len, dst_input + (size_t)k * obs_len);
            std::copy(slot + obs_len, slot + obs_len + pol_len, dst_mcts + (size_t)k * pol_len);
            dst_result[k] = slot[obs_len + pol_len];
        }
    }
};

// One trajectory step as a compact record: the board, the value target and the visit shares of its moves.  A record
// holds KH_MAX_RECORD_ACTIONS moves; of a position with more (rare) the most visited ones are kept, in action order.
inline kh_record make_record(const kh_board& board, float value, const int* actions, const float* visits, size_t nmoves)
{
    kh_record r;
    memset(&r, 0, sizeof(r));
    r.board = board;
    r.value = value;
    std::vector<int> idx(nmoves);
    for (size_t i = 0; i < nmoves; ++i) idx[i] = (int)i;
    if (idx.size() > KH_MAX_RECORD_ACTIONS) {
        std::partial_sort(idx.begin(), idx.begin() + KH_MAX_RECORD_ACTIONS, idx.end(), [&](int a, int b) { return visits[a] > visits[b]; });
        idx.resize(KH_MAX_RECORD_ACTIONS);
        std::sort(idx.begin(), idx.end());
    }
    r.nact = (int32_t)idx.size();
    for (size_t i = 0; i < idx.size(); ++i) { r.actions[i] = (int16_t)actions[idx[i]]; r.visits[i] = visits[idx[i]]; }
    return r;
}

// The same ring over compact records (kh_record, 664 bytes where a dense row takes 26 372): what NN::train_records
// consumes.  A never-written slot is the all-zero record (empty board, no moves, value 0), which is a valid sample.
// The draws come from the ring's own seeded generator, so a run can be repeated.
class CompactReplayBuffer {
    const int capacity;
    std::vector<kh_record> ring;
    std::mutex lock;
    std::mt19937_64 rng;
    int head = 0;
    long added = 0;

public:
    explicit CompactReplayBuffer(int bufsize, uint64_t seed = 0) : capacity(bufsize), ring((size_t)bufsize), rng(seed)
    {
        memset(ring.data(), 0, ring.size() * sizeof(kh_record));
    }

    int size() { return capacity; }
    long count()
    {
        std::lock_guard<std::mutex> hold(lock);
        return added;
    }

    void clear()
    {
        std::lock_guard<std::mutex> hold(lock);
        head = 0;
        added = 0;
        memset(ring.data(), 0, ring.size() * sizeof(kh_record));
    }

    void add(const kh_record* rec, long n)
    {
        std::lock_guard<std::mutex> hold(lock);
        for (long k = 0; k < n; ++k) {
            ring[(size_t)head] = rec[k];
            head = (head + 1) % capacity;
        }
        added += n;
    }

    // n draws with replacement over ALL slots (replaybuffer.h:61-84)
    void select_batch(kh_record* dst, int n)
    {
        std::lock_guard<std::mutex> hold(lock);
        for (int k = 0; k < n; ++k) dst[k] = ring[(size_t)(rng() % (uint64_t)capacity)];
    }
};

}  // namespace kami
#endif
