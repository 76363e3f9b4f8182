// replay_ring.h — what replay_ring.hip (the device replay ring, kh_replay_*) and train_ingest.hip (kh_train_replay, which
// trains from it) share.  Not part of the public boundary (that is include/kami_hip.h).
#pragma once
#include "engine.h"

#include <random>

namespace kh {

// records_check's three failures, stated once: the device validator (replay_ring.hip) reports the same offence in the
// same words.  value: the nact or the action; entry: its index k (unused for RECORD_BAD_NACT)
enum { RECORD_BAD_NACT = 0, RECORD_BAD_RANGE = 1, RECORD_BAD_TWICE = 2 };
int record_fail(int rule, int record, int value, int entry);

}  // namespace kh

// CompactReplayBuffer's state on the host, its records in device memory in RecordBlock(capacity) layout, which is what
// launch_expand_records reads: kh_train_replay trains from `mem` in place.  Every call holds `mu` from its first look
// at the state until its device work has finished.
struct kh_replay {
    int device = 0, capacity = 0;
    kh::RecordBlock lay{ 0 };
    kh::DevMem mem;                  // the ring
    kh::DevMem stage, slots, err;    // records as structs on their way in or out; a gather's slot list; the validator's word
    kh::PinMem pin;                  // the word coming down, the slot list going up
    hipStream_t st = nullptr;
    std::mutex mu;
    std::mt19937_64 rng;
    int head = 0;                    // next slot to write
    int64_t added = 0;               // records ever added
};
