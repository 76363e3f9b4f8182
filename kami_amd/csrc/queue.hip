// queue.hip — the coalescing queue behind kh_submit_* / kh_wait: callers' small batches merged into
// launches by one dispatcher thread per engine.  Its types are this file's own; the C ABI reaches it through the co_*
// functions engine.h declares.
#include "engine.h"

#include <sched.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace kh {
namespace {

// ------------------------------------------------------------------------------- coalescing queue
// SURVEY §8(b), threading row: "per-thread stream + staging slot, OR internal queue that coalesces callers into
// bigger batches".  The slots above are the first; this is the second.  Callers hand over small batches
// (kh_submit_* returns a ticket at once, kh_wait blocks for it; the synchronous entry points use the same queue when
// other small calls are in flight), each caller copies its own rows into the open batch's merge buffers, and ONE
// dispatcher thread turns whatever has accumulated into a launch on one of four streams without waiting for it (one
// pinned block each way), polls the launches' completion words and publishes the results: every waiter copies its own
// rows out of the block.  While launches are on the device the next batch fills up, so the batch size adapts to the
// load; kh_set_coalesce adds a target size and a bounded wait for callers that know how much will be in flight (the
// self-play pool).
//
// Never blocks a submitter on its own outstanding work: tickets are a fixed pool (exhaustion -> KH_ERR_INVALID),
// merge buffers come back when their launch has completed and its rows have been fetched — by the waiters, or by the
// dispatcher for tickets nobody waits on — so the only wait inside kh_submit_* is for launches that are on the device.
constexpr int CO_ROWS = 1024;                   // boards per coalesced launch (merge buffer capacity)
constexpr int CO_ACTS = CO_ROWS * 48;           // legal actions per coalesced launch
constexpr int CO_SMALL_LEGAL = 512;             // a submission larger than this takes the direct path
constexpr int CO_SMALL_PLANES = 128;
constexpr int CO_BUFFERS = 12;                  // up to max_inflight on the device, one filling, the rest waiting for their callers to fetch

// The queue's lock.  Its critical sections are a few hundred nanoseconds (reserve rows, look at the batches) and a dozen
// workers hit it within the same microsecond when a launch hands their tickets back: with std::mutex the losers sleep
// on the futex and are woken one after the other (2-3 us each: measured as 33-37 us of "filling" per launch with 14
// workers), so it spins.  Sleeping paths (idle lane, buffers all on the device, waiters past their spin time) go
// through std::condition_variable_any, which takes any lock type.
struct SpinLock {
    // test-and-test-and-set.  (A ticket lock — FIFO hand-over, waiters on a plain load — was measured: the same with two sets
    // per worker, worse with four: 3.3-3.5 -> 2.8-3.0 M/s; a FIFO queue turns one descheduled waiter into everybody's wait.)
    std::atomic<int> held{ 0 };
    void lock()
    {
        for (int k = 0;; ++k) {
            if (!held.exchange(1, std::memory_order_acquire)) return;
            while (held.load(std::memory_order_relaxed)) {
                __builtin_ia32_pause();
                if ((++k & 1023) == 0) sched_yield();       // more threads than cores: the holder may need this one
            }
        }
    }
    bool try_lock() { return !held.exchange(1, std::memory_order_acquire); }
    void unlock() { held.store(0, std::memory_order_release); }
};

// (A waiter polls `state` in a tight loop, the dispatcher writes the other fields right before it publishes: the polled word
//  has a cache line of its own, and no two tickets share one — a dozen pollers on the lines the dispatcher was writing made
//  its hand-back 10-18 us per launch with three sets per worker.)
struct alignas(64) CoTicket {
    alignas(64) std::atomic<int> state{ 0 };    // 0 free, 1 queued, 2 done: results in the caller's buffers (waiters spin on it, then
                                                // sleep), 4 results in the batch's page-locked block, 5 somebody is copying them out
    uint32_t serial = 0;                        // (same line as `state`: written at submit time only, read by every poll)
    alignas(64) struct CoBatch* from = nullptr; // state 4 / 5: the batch that holds this ticket's rows
    int status = KH_OK;
    std::string err;
    int kind = 0, row0 = 0, rows = 0, act0 = 0, nact = 0;
    // the caller's buffers (valid until kh_wait returns): inputs for the rare per-ticket re-run, outputs for the scatter
    const kh_board* boards = nullptr; const float* planes = nullptr;
    const int32_t *offsets = nullptr, *actions = nullptr;
    float *priors = nullptr, *value = nullptr, *policy = nullptr;
};

struct CoBatch {
    int state = 0;                              // 0 free, 1 open, 2 sealed (the dispatcher owns it; after completion until the last
                                                // ticket's rows have been copied out)
    int kind = 0;                               // 0: records + legal actions -> priors; 1: planes -> full policy rows
    int rows = 0, nact = 0;
    std::atomic<int> copying{ 0 };              // submitters that have reserved rows and are still copying them in
    std::atomic<int> readers{ 0 };              // tickets whose rows are still in the block (state 4 / 5)
    unsigned* done = nullptr;                   // word in pin_out that signal_kernel sets to `serial` behind the launch
    unsigned serial = 0;
    bool full = false;
    std::chrono::steady_clock::time_point first, last;     // first / latest submission into this batch
    std::vector<CoTicket*> tickets;
    // kind 0 merges straight into page-locked memory that the kernels read and write THEMSELVES (no copy engine on
    // the path: 100 KB each way per launch is latency, not bandwidth): boards | offsets | actions in, priors | values
    // | NaN flags out
    PinMem pin_in, pin_out;
    kh_board* boards = nullptr;
    int32_t *offsets = nullptr, *actions = nullptr;
    float *priors = nullptr, *values = nullptr;
    int* flags_out = nullptr;
    Slot* lane = nullptr;                       // stream + device scratch of the launch this buffer is on (Coalescer::lanes)
    std::shared_ptr<Weights> W;                 // the weights a launch that is on the device runs on
    std::chrono::steady_clock::time_point t_seal, t_run, t_launched;
    std::vector<float> planes, vfull, policy;   // kind 1 / reference value copy-out: plain host staging for infer_host
};

struct Coalescer {
    kh_engine* e;
    SpinLock mu;
    std::condition_variable_any cv_lane, cv_done, cv_space;
    CoTicket tickets[KH_MAX_OUTSTANDING];
    CoBatch batches[CO_BUFFERS];
    std::atomic<uint64_t> free_mask{ ~0ull };   // bit i: ticket i is free (a submit takes the lowest under mu, a wait gives its own
                                                // back without the lock); KH_MAX_OUTSTANDING == 64 == its width
    std::atomic<unsigned> submits{ 0 };         // bumped by every submission: the dispatcher scans the batches (under mu) only when
                                                // it has changed, a deadline is due or a launch slot has come back
    std::atomic<bool> asleep{ false };          // the dispatcher sleeps on cv_lane: only then does a submitter notify it
    std::thread dispatcher;
    // Launches on the device at once: each on a lane = a stream of its own + device scratch.  FOUR streams, created one
    // after the other, because that is how many hardware queues the runtime spreads streams over: with a stream per
    // merge buffer (12) launches that were "in flight together" shared a queue and ran one behind the other (engine
    // call 80-110 us with four in flight against 38-41 with two).  KAMI_CO_INFLIGHT lowers it.
    static constexpr int MAX_LANES = 4;
    Slot lanes[MAX_LANES];
    bool lane_busy[MAX_LANES] = { false, false, false, false };
    int max_inflight = MAX_LANES;
    int sleepers = 0;
    int spin_us = 1000;                         // kh_wait spins this long on its ticket before it sleeps (KAMI_WAIT_SPIN_US): a
                                                // sleeper costs the dispatcher a futex wake per launch and itself 10-50 us, and one
                                                // slow cycle (> 150 us, round 2's value) used to tip a pool into that regime for good
    bool stop = false;
    int64_t launches = 0, rows_launched = 0;
    // KAMI_CO_TRACE=1: where a coalesced launch's time goes (printed when the engine is destroyed)
    bool trace = false;
    double us_fill = 0, us_copywait = 0, us_launch = 0, us_run = 0, us_finish = 0;
};

// records + legal actions -> priors + one value per position, straight out of / into the batch's page-locked blocks:
// forward kernel(s) and the gather kernel on the buffer's own stream.  Launch only: the dispatcher polls the stream
// (hipStreamQuery) and calls co_finish_legal when it has drained — the launch's latency is what every waiting caller pays.
int co_launch_legal(kh_engine* e, CoBatch& b)
{
    const int B = b.rows;
    b.W = current_weights(e);                   // kept until the launch has completed
    if (!b.W) return fail(KH_ERR_NO_WEIGHTS, "kh_infer before kh_load_weights");
    const Weights& W = *b.W;
    int rc = set_device(e);
    if (rc) return rc;
    Slot& s = *b.lane;
    if ((rc = slot_ensure(e, s, CO_ROWS, true))) return rc;        // sized once for the largest merged launch: no allocation (= device sync) mid-run
    hipStream_t st = s.stream;
    if (fused_ingest(e, W)) {
        // one launch: records in, legal priors + values + NaN flags out, all through the batch's page-locked blocks
        b.flags_out[0] = b.flags_out[1] = 0;
        const LegalDev lg{ b.offsets, b.actions, b.priors, b.values, b.flags_out };
        rc = forward_tower(e, W, s, st, nullptr, B, s.policy.as<float>(), s.vfull.as<float>(), nullptr, b.boards, &lg);
        if (rc) return rc;
    } else {
        kh::launch_encode_f32(b.boards, B, s.planes.as<float>(), st);
        rc = forward_dispatch(e, W, s, st, s.planes.as<float>(), B, s.policy.as<float>(), s.vfull.as<float>(), nullptr);
        if (rc) return rc;
        kh::launch_gather_legal(s.policy.as<float>(), b.offsets, b.actions, b.priors, B, st, s.vfull.as<float>(), KH_VALUE_WIDTH, b.values,
                                s.flags.as<int>(), b.flags_out);
    }
    // (the forward kernel's LAST workgroup writing the word itself was tried: its results then have to be system-scope
    //  stores, ~8 000 four-byte PCIe writes per launch instead of L2-combined lines — engine call 43-46 us against 38-40)
    if (++b.serial == 0) b.serial = 1;
    kh::launch_signal(b.done, b.serial, st);
    HIPCHK(hipGetLastError());
    return KH_OK;
}

int co_finish_legal(CoBatch& b)
{
    b.W.reset();
    return nan_status(*b.lane, b.flags_out);
}

// Starts a sealed batch.  Returns true when it is now on the device (records + legal actions, per-sample values: the
// self-play path) and the dispatcher has to poll for it; false when it ran synchronously (plane submissions and the
// reference's flattened value tensor go through infer_host: uploads, downloads and a stream wait) and `rc` is final.
bool co_start(kh_engine* e, CoBatch& b, int& rc)
{
    const int B = b.rows;
    const bool flat = e->cfg.value_mode == KH_VALUE_REFERENCE_FLAT;
    if (b.kind == 0 && !flat) {
        rc = co_launch_legal(e, b);
        if (rc) b.W.reset();
        return rc == KH_OK;
    }
    if (b.kind == 0) {
        // nn.cpp:186 hands back the first `batch` floats of the caller's OWN flattened [batch,256] tensor: take the
        // whole tensor and cut each caller's slice out of it below
        LegalIO l{ b.offsets, b.actions, b.priors };
        b.vfull.resize((size_t)B * KH_VALUE_WIDTH);
        rc = infer_host(e, { .boards = b.boards, .batch = B, .value_full = b.vfull.data(), .legal = &l });
    } else {
        b.policy.resize((size_t)B * KH_PSIZE);
        b.vfull.resize((size_t)B * KH_VALUE_WIDTH);
        rc = infer_host(e, { .input = b.planes.data(), .batch = B, .policy = b.policy.data(), .value_full = b.vfull.data() });
    }
    return false;
}

// One ticket's rows out of a finished records-and-legal-actions batch's page-locked block (per-sample values)
inline void co_fetch(CoTicket* t)
{
    const CoBatch* b = t->from;
    if (t->nact) memcpy(t->priors, b->priors + t->act0, (size_t)t->nact * 4);
    memcpy(t->value, b->values + t->row0, (size_t)t->rows * 4);
}

// the last ticket's rows are out: the buffer can be filled again
void co_release(Coalescer* c, CoBatch* b)
{
    std::lock_guard<SpinLock> lk(c->mu);
    b->tickets.clear();
    b->rows = b->nact = 0; b->full = false; b->state = 0;
    c->cv_space.notify_all();
}

// a ticket in state 4: whoever wins the claim copies its rows out (its waiter, or the dispatcher going round)
inline bool co_claim_fetch(Coalescer* c, CoTicket* t)
{
    int expect = 4;
    if (!t->state.compare_exchange_strong(expect, 5, std::memory_order_acquire)) return false;
    CoBatch* b = t->from;
    co_fetch(t);
    t->state.store(2, std::memory_order_release);
    if (b->readers.fetch_sub(1, std::memory_order_acq_rel) == 1) co_release(c, b);
    return true;
}

// results (or the error) of a finished batch into every caller's own buffers, by the dispatcher alone: the synchronous
// kinds, errors, and the rare per-ticket re-run
void co_deliver(kh_engine* e, CoBatch& b, int rc)
{
    const bool flat = e->cfg.value_mode == KH_VALUE_REFERENCE_FLAT;
    const std::string err = rc ? g_err : std::string();
    for (CoTicket* t : b.tickets) {
        if (rc == KH_ERR_NAN_POLICY || rc == KH_ERR_NAN_VALUE) {
            // a NaN somewhere in the merged batch: the reference's exception belongs to the caller whose rows hold it.
            // Rare: run every ticket of this batch on its own (its inputs are still the caller's to keep until kh_wait).
            if (t->kind == 0) {
                LegalIO l{ t->offsets, t->actions, t->priors };
                t->status = infer_host(e, { .boards = t->boards, .batch = t->rows, .value = t->value, .legal = &l });
            } else {
                t->status = infer_host(e, { .input = t->planes, .batch = t->rows, .policy = t->policy, .value = t->value });
            }
            t->err = t->status ? g_err : std::string();
            continue;
        }
        t->status = rc; t->err = err;
        if (rc) continue;
        if (t->kind == 0) {
            if (t->nact) memcpy(t->priors, b.priors + t->act0, (size_t)t->nact * 4);
        } else {
            memcpy(t->policy, b.policy.data() + (size_t)t->row0 * KH_PSIZE, (size_t)t->rows * KH_PSIZE * 4);
        }
        if (b.kind == 0 && !flat) memcpy(t->value, b.values + t->row0, (size_t)t->rows * 4);
        else if (flat) memcpy(t->value, b.vfull.data() + (size_t)t->row0 * KH_VALUE_WIDTH, (size_t)t->rows * 4);    // rows <= 256 here
        else for (int i = 0; i < t->rows; ++i) t->value[i] = b.vfull[(size_t)(t->row0 + i) * KH_VALUE_WIDTH];
    }
}

// ONE dispatcher thread per engine: seals a batch when the rule says so, launches it WITHOUT waiting for it, polls the
// launches that are on the device (up to `max_inflight`, each on its buffer's own stream) and hands results back.
// Round 2 had two lanes that each blocked on their launch: two spinning threads of the 16 the search needs, and a batch
// that became ready while both were busy waited out a whole engine call.
// Completion: signal_kernel's word in the batch's page-locked block (hipStreamQuery only as the safety net that notices
// a failed stream).  Hand-back: a finished batch's tickets go to state 4 at once and every waiter copies its OWN rows
// out of the block (a dozen callers in parallel: the block was written over PCIe, every line is a DRAM miss — one
// thread copying 30 KB took 6-8 us of every caller's time); the dispatcher goes round the tickets nobody has claimed
// yet, so a buffer comes back whether or not its callers are waiting.
void co_dispatch(Coalescer* c)
{
    kh_engine* e = c->e;
    CoBatch* fly[CO_BUFFERS];
    CoBatch* drain[CO_BUFFERS];                 // finished batches whose tickets may still be in state 4
    int drain_age[CO_BUFFERS];
    int nfly = 0, ndrain = 0;
    auto us = [](std::chrono::steady_clock::duration d) { return std::chrono::duration<double, std::micro>(d).count(); };
    auto complete = [&](CoBatch* b, int rc, bool in_block) {
        const auto t_ran = std::chrono::steady_clock::now();
        CoTicket* mine[KH_MAX_OUTSTANDING];
        const int nt = (int)b->tickets.size();
        for (int i = 0; i < nt; ++i) mine[i] = b->tickets[i];
        const int rows = b->rows;
        if (in_block && rc == KH_OK) {
            b->readers.store(nt, std::memory_order_relaxed);
            for (int i = 0; i < nt; ++i) { mine[i]->status = KH_OK; mine[i]->err.clear(); mine[i]->from = b; }
            for (int i = 0; i < nt; ++i) mine[i]->state.store(4, std::memory_order_release);
        } else {
            co_deliver(e, *b, rc);
            for (int i = 0; i < nt; ++i) mine[i]->state.store(2, std::memory_order_release);
        }
        bool wake;
        {
            std::lock_guard<SpinLock> lk(c->mu);
            c->launches += 1; c->rows_launched += rows;
            wake = c->sleepers > 0;
        }
        if (wake) c->cv_done.notify_all();          // (sleepers re-check their ticket under the lock: states were stored before it)
        if (in_block && rc == KH_OK) {                          // its waiters fetch their rows; the dispatcher sweeps up later
            int i = 0;
            while (i < ndrain && drain[i] != b) ++i;            // (still listed from its previous launch: released since)
            if (i == ndrain) ++ndrain;
            drain[i] = b; drain_age[i] = 0;
        }
        else co_release(c, b);
        if (c->trace) {
            c->us_fill += us(b->t_seal - b->first); c->us_copywait += us(b->t_run - b->t_seal); c->us_launch += us(b->t_launched - b->t_run);
            c->us_run += us(t_ran - b->t_run); c->us_finish += us(std::chrono::steady_clock::now() - t_ran);
        }
    };
    // The batches are looked at (under the queue's lock) only when something can have changed: a submission since the last
    // look, a deadline of an open batch, a launch slot that has come back, a settings change / stop (they bump `submits`
    // too).  Looking every time round made the dispatcher the 15th contender for a lock 14 workers submit through.
    unsigned seen = c->submits.load(std::memory_order_acquire) - 1;
    bool open_any = false, slot_back = false;
    auto next_due = std::chrono::steady_clock::time_point::max();
    for (unsigned spin = 0;; ++spin) {
        CoBatch* take = nullptr;
        const unsigned subs = c->submits.load(std::memory_order_acquire);
        if (subs != seen || slot_back || (open_any && std::chrono::steady_clock::now() >= next_due) ||
            (!open_any && nfly == 0 && ndrain == 0)) {
            std::unique_lock<SpinLock> lk(c->mu);
            seen = c->submits.load(std::memory_order_acquire);
            slot_back = false;
            open_any = false;
            next_due = std::chrono::steady_clock::time_point::max();
            const int target = e->co_target.load(), wait_us = e->co_wait_us.load(), callers = e->co_callers.load();
            for (auto& b : c->batches) {
                if (b.state != 1 || b.rows == 0) continue;
                open_any = true;
                if (nfly >= c->max_inflight) { next_due = std::chrono::steady_clock::time_point::max(); break; }   // (a slot coming back re-opens the question)
                // immediate mode (no target): whatever has accumulated goes at once;
                // target mode: wait for `target` rows or `callers` submissions — but no longer than wait_us after the
                // batch's first submission, and not once the burst of submissions has ended (nothing added for
                // wait_us / 8: callers that keep a fixed number of positions in flight rarely hit the target exactly —
                // terminal leaves need no evaluation)
                bool ready = b.full || target <= 0 || b.rows >= target || (callers > 0 && (int)b.tickets.size() >= callers);
                if (!ready) {
                    const auto due = std::min(b.first + std::chrono::microseconds(wait_us), b.last + std::chrono::microseconds(wait_us / 8 + 1));
                    ready = std::chrono::steady_clock::now() >= due;
                    if (!ready) next_due = std::min(next_due, due);
                }
                if (ready) { take = &b; break; }
            }
            if (!take && !open_any && nfly == 0 && ndrain == 0) {
                if (c->stop) return;
                c->asleep.store(true, std::memory_order_release);
                c->cv_lane.wait(lk);                 // nothing queued, nothing on the device
                c->asleep.store(false, std::memory_order_release);
                seen = c->submits.load(std::memory_order_acquire) - 1;
                continue;
            }
            if (take) { take->state = 2; take->t_seal = std::chrono::steady_clock::now(); seen = subs - 1; }   // (look again: another batch may be ready)
        }
        if (take) {
            while (take->copying.load(std::memory_order_acquire) > 0) __builtin_ia32_pause();   // submitters still copying their rows in: a microsecond
            take->t_run = std::chrono::steady_clock::now();
            int rc = KH_OK;
            int li = 0;
            while (c->lane_busy[li]) ++li;              // nfly < max_inflight <= MAX_LANES: one is free
            take->lane = &c->lanes[li];
            const bool on_device = co_start(e, *take, rc);
            if (on_device) c->lane_busy[li] = true;
            take->t_launched = std::chrono::steady_clock::now();
            if (on_device) fly[nfly++] = take;
            else complete(take, rc, false);
        }
        for (int i = 0; i < nfly;) {
            CoBatch* b = fly[i];
            bool done = __atomic_load_n(b->done, __ATOMIC_ACQUIRE) == b->serial;
            hipError_t q = hipSuccess;
            if (!done && (spin & 4095) == 4095) {         // safety net: a stream that failed never writes the word
                q = hipStreamQuery(b->lane->stream);
                done = q != hipErrorNotReady;
            }
            if (!done) { ++i; continue; }
            const int rc = q == hipSuccess ? co_finish_legal(*b) : fail(KH_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(q));
            b->W.reset();
            c->lane_busy[b->lane - c->lanes] = false;
            complete(b, rc, true);
            fly[i] = fly[--nfly];
            slot_back = true;
        }
        // Finished batches whose rows have not all been fetched: their waiters do that themselves, in parallel, the
        // moment they see state 4 — the dispatcher only sweeps up what is left after a few rounds' grace (callers that
        // are busy with another set, or never wait), so that a buffer always comes back.  A buffer is in the list at
        // most once (a second publish needs a release in between), so the list never outgrows the buffers.
        for (int i = 0; i < ndrain;) {
            CoBatch* b = drain[i];
            if (b->readers.load(std::memory_order_acquire) > 0 && (take || ++drain_age[i] <= 16)) { ++i; continue; }
            if (b->readers.load(std::memory_order_acquire) > 0) {
                CoTicket* mine[KH_MAX_OUTSTANDING];
                int nt = 0;
                { std::lock_guard<SpinLock> lk(c->mu); if (b->state == 2) for (CoTicket* t : b->tickets) mine[nt++] = t; }
                for (int k = 0; k < nt; ++k) if (mine[k]->from == b) (void)co_claim_fetch(c, mine[k]);
            }
            --ndrain;
            drain[i] = drain[ndrain]; drain_age[i] = drain_age[ndrain];
        }
        if (!take) {
            // a batch is filling or a launch is on the device: poll (a sleeping thread's wake-up, 5-15 us, would be
            // paid by every caller of the launch), but let a caller's thread have the core when it needs one
            for (int k = 0; k < 8; ++k) __builtin_ia32_pause();
            if ((spin & 15) == 15) sched_yield();
        }
    }
}

// a synchronous small call goes through the queue when other small calls are inside the engine right now
struct SmallCall {
    kh_engine* e;                // null: not a small call
    bool others = false;
    SmallCall(kh_engine* e_, bool small) : e(small ? e_ : nullptr) { if (e) others = e->small_calls.fetch_add(1) > 0; }
    ~SmallCall() { if (e) e->small_calls.fetch_sub(1); }
};

}  // namespace

// kh_engine::co: the engine's handle on its queue
struct Queue : Coalescer {};

namespace {

Coalescer* co_get(kh_engine* e)
{
    std::lock_guard<std::mutex> lk(e->co_mu);
    if (!e->co) {
        Queue* c = new Queue();
        c->e = e;
        c->trace = getenv("KAMI_CO_TRACE") != nullptr;
        if (getenv("KAMI_WAIT_SPIN_US")) c->spin_us = std::max(0, atoi(getenv("KAMI_WAIT_SPIN_US")));
        if (getenv("KAMI_CO_INFLIGHT")) c->max_inflight = std::min((int)Coalescer::MAX_LANES, std::max(1, atoi(getenv("KAMI_CO_INFLIGHT"))));
        // the lanes' streams now, one after the other (see Coalescer::lanes); a failure here shows up at the first launch
        if (set_device(e) == KH_OK)
            for (auto& l : c->lanes) (void)hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking);
        c->dispatcher = std::thread(co_dispatch, c);
        e->co = c;
        e->co_ready.store(c, std::memory_order_release);
    }
    return e->co;
}

}  // namespace

void co_destroy(kh_engine* e)
{
    Queue* c = e->co;
    if (!c) return;
    { std::lock_guard<SpinLock> lk(c->mu); c->stop = true; c->submits.fetch_add(1); }
    c->cv_lane.notify_all();
    if (c->dispatcher.joinable()) c->dispatcher.join();
    (void)hipSetDevice(e->cfg.device);
    for (auto& l : c->lanes) {
        if (l.stream) { (void)hipStreamSynchronize(l.stream); (void)hipStreamDestroy(l.stream); l.stream = nullptr; }
    }
    if (c->trace && c->launches)
        fprintf(stderr, "[kami queue] %lld launches, %.1f rows each; per launch: filling %.1f us, waiting for copies %.1f us, "
                "engine call %.1f us (of which the launch call %.1f), hand-back %.1f us\n", (long long)c->launches, (double)c->rows_launched / c->launches,
                c->us_fill / c->launches, c->us_copywait / c->launches, c->us_run / c->launches, c->us_launch / c->launches, c->us_finish / c->launches);
    delete c;
    e->co = nullptr;
    e->co_ready.store(nullptr, std::memory_order_release);
}

int co_submit(kh_engine* e, int kind, const kh_board* boards, const float* planes, int batch, const int32_t* offsets,
              const int32_t* actions, float* priors, float* value, float* policy, int64_t* ticket)
{
    if (!e || !ticket || !value || batch < 1) return fail(KH_ERR_INVALID, "bad submit arguments");
    int nact = 0;
    if (kind == 0) {
        if (!boards || !offsets || !actions || !priors) return fail(KH_ERR_INVALID, "null buffer");
        if (int rc = check_records(e, nullptr)) return rc;
        if (int rc = check_offsets(offsets, batch)) return rc;
        nact = offsets[batch];
        if (batch > CO_SMALL_LEGAL || nact > CO_ACTS) return fail(KH_ERR_INVALID, "submissions hold at most %d positions / %d actions (use the synchronous call for more)", CO_SMALL_LEGAL, CO_ACTS);
    } else {
        if (!planes || !policy) return fail(KH_ERR_INVALID, "null buffer");
        if (batch > CO_SMALL_PLANES) return fail(KH_ERR_INVALID, "plane submissions hold at most %d positions (use kh_infer for more)", CO_SMALL_PLANES);
    }
    if (!e->has_weights.load(std::memory_order_acquire)) return fail(KH_ERR_NO_WEIGHTS, "submit before kh_load_weights");   // (no shared_ptr copy under wmu per submission)
    Coalescer* c = e->co_ready.load(std::memory_order_acquire);
    if (!c) c = co_get(e);
    const size_t F = e->cfg.features;
    const int cap_rows = kind == 0 ? CO_ROWS : 2 * CO_SMALL_PLANES;
    std::unique_lock<SpinLock> lk(c->mu);
    static_assert(KH_MAX_OUTSTANDING == 64, "free_mask is one 64-bit word");
    const uint64_t fm = c->free_mask.load(std::memory_order_acquire);
    if (fm == 0) return fail(KH_ERR_INVALID, "%d submissions are outstanding on this engine: kh_wait for some before submitting more", KH_MAX_OUTSTANDING);
    const int tid = __builtin_ctzll(fm);               // taken NOW: the wait for a free buffer below drops the lock
    c->free_mask.fetch_and(~(1ull << tid), std::memory_order_acq_rel);
    CoTicket* t = &c->tickets[tid];
    t->state.store(1, std::memory_order_relaxed);
    CoBatch* b = nullptr;
    for (;;) {
        for (auto& x : c->batches)
            if (x.state == 1 && x.kind == kind && !x.full) {
                if (x.rows + batch <= cap_rows && x.nact + nact <= CO_ACTS) { b = &x; break; }
                x.full = true;                                   // does not fit: it goes as it is
                c->submits.fetch_add(1, std::memory_order_release);
            }
        if (b) break;
        for (auto& x : c->batches)
            if (x.state == 0) { b = &x; break; }
        if (b) {
            b->state = 1; b->kind = kind; b->rows = 0; b->nact = 0; b->full = false;
            b->first = b->last = std::chrono::steady_clock::now();
            if (kind == 0) {
                if (!b->boards) {
                    const size_t o_offs = (size_t)CO_ROWS * sizeof(kh_board), o_acts = o_offs + (((size_t)CO_ROWS + 1) * 4 + 15) / 16 * 16;
                    const size_t o_vals = (size_t)CO_ACTS * 4, o_flags = o_vals + (size_t)CO_ROWS * 4;
                    if (set_device(e) || b->pin_in.ensure(o_acts + (size_t)CO_ACTS * 4) || b->pin_out.ensure(o_flags + 128)) {
                        b->state = 0;
                        t->state.store(0, std::memory_order_release);
                        c->free_mask.fetch_or(1ull << tid, std::memory_order_release);
                        return KH_ERR_HIP;
                    }
                    b->boards = reinterpret_cast<kh_board*>(b->pin_in.at(0));
                    b->offsets = reinterpret_cast<int32_t*>(b->pin_in.at(o_offs));
                    b->actions = reinterpret_cast<int32_t*>(b->pin_in.at(o_acts));
                    b->priors = reinterpret_cast<float*>(b->pin_out.at(0));
                    b->values = reinterpret_cast<float*>(b->pin_out.at(o_vals));
                    b->flags_out = reinterpret_cast<int*>(b->pin_out.at(o_flags));
                    b->done = reinterpret_cast<unsigned*>(b->pin_out.at(o_flags + 64));       // a cache line of its own
                    *b->done = 0;
                }
                b->offsets[0] = 0;
            } else if (b->planes.size() < (size_t)cap_rows * 64 * F) b->planes.resize((size_t)cap_rows * 64 * F);
            break;
        }
        c->cv_space.wait(lk);                                    // every buffer is on the device: one of them comes back
    }
    // under the lock: only what the batch's bookkeeping needs; the ticket's own fields are written after it (the dispatcher
    // reads them when the launch completes, which is behind `copying` reaching zero)
    const int row0 = b->rows, act0 = b->nact;
    b->rows += batch; b->nact += nact;
    b->tickets.push_back(t);
    b->copying.fetch_add(1, std::memory_order_relaxed);
    b->last = std::chrono::steady_clock::now();           // (under the lock: the dispatcher reads it there)
    c->submits.fetch_add(1, std::memory_order_release);
    lk.unlock();
    t->status = KH_OK; t->err.clear(); ++t->serial;
    t->kind = kind; t->row0 = row0; t->rows = batch; t->act0 = act0; t->nact = nact;
    t->boards = boards; t->planes = planes; t->offsets = offsets; t->actions = actions;
    t->priors = priors; t->value = value; t->policy = policy;
    // this caller's rows into the merge buffers (every caller copies its own, in parallel)
    if (kind == 0) {
        memcpy(b->boards + t->row0, boards, (size_t)batch * sizeof(kh_board));
        if (nact) memcpy(b->actions + t->act0, actions, (size_t)nact * 4);
        for (int i = 1; i <= batch; ++i) b->offsets[t->row0 + i] = t->act0 + offsets[i];
    } else {
        memcpy(b->planes.data() + (size_t)t->row0 * 64 * F, planes, (size_t)batch * 64 * F * 4);
    }
    const uint32_t serial = t->serial;
    b->copying.fetch_sub(1, std::memory_order_release);   // (no lock: the dispatcher spins on it once it has sealed this batch; after
                                                          //  this the launch may complete and the ticket be waited for)
    if (c->asleep.load(std::memory_order_acquire)) {      // (a notify per submission was a std::mutex every caller met at once)
        std::lock_guard<SpinLock> lk2(c->mu);
        c->cv_lane.notify_all();
    }
    *ticket = (int64_t)tid | ((int64_t)serial << 32);
    return KH_OK;
}

int co_wait(kh_engine* e, int64_t ticket)
{
    if (!e || !e->co) return fail(KH_ERR_INVALID, "no such ticket");
    Coalescer* c = e->co;
    const int tid = (int)(ticket & 0xffffffff);
    const uint32_t serial = (uint32_t)(ticket >> 32);
    if (tid < 0 || tid >= KH_MAX_OUTSTANDING) return fail(KH_ERR_INVALID, "no such ticket");
    CoTicket& t = c->tickets[tid];
    if (t.state.load(std::memory_order_acquire) == 0 || t.serial != serial)
        return fail(KH_ERR_INVALID, "ticket already waited for (or never issued)");
    // a launch is ~100 us away at most: spin on the ticket first (no wake-up latency, no mutex convoy when a launch
    // releases many callers at once), sleep on the condition variable only when it takes longer.  State 4: the rows are
    // in the batch's block and this thread fetches them itself (unless the dispatcher got there first: state 5, then 2).
    auto settled = [&] {
        const int st = t.state.load(std::memory_order_acquire);
        if (st == 2) return true;
        if (st == 4) (void)co_claim_fetch(c, &t);
        return t.state.load(std::memory_order_acquire) == 2;
    };
    if (!settled() && c->spin_us > 0) {
        const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(c->spin_us);
        for (int k = 0; !settled(); ++k) {
            __builtin_ia32_pause();
            if ((k & 63) == 63) {
                sched_yield();                  // lets the dispatcher (or another caller) have the core if it needs one
                if (std::chrono::steady_clock::now() >= until) break;
            }
        }
    }
    if (!settled()) {
        std::unique_lock<SpinLock> lk(c->mu);
        ++c->sleepers;
        for (;;) {
            const int st = t.state.load(std::memory_order_acquire);
            if (st == 2) break;
            if (st == 4 || st == 5) { lk.unlock(); while (!settled()) __builtin_ia32_pause(); lk.lock(); break; }
            c->cv_done.wait(lk);
        }
        --c->sleepers;
    }
    const int rc = t.status;
    if (rc) g_err = t.err;
    t.state.store(0, std::memory_order_release);
    c->free_mask.fetch_or(1ull << tid, std::memory_order_release);
    return rc;
}


int co_try_wait(kh_engine* e, int64_t ticket, int* done)
{
    if (!done) return fail(KH_ERR_INVALID, "null done");
    *done = 0;
    if (!e || !e->co) return fail(KH_ERR_INVALID, "no such ticket");
    Coalescer* c = e->co;
    const int tid = (int)(ticket & 0xffffffff);
    if (tid < 0 || tid >= KH_MAX_OUTSTANDING) return fail(KH_ERR_INVALID, "no such ticket");
    CoTicket& t = c->tickets[tid];
    int st = t.state.load(std::memory_order_acquire);
    if (st == 0 || t.serial != (uint32_t)(ticket >> 32)) return fail(KH_ERR_INVALID, "ticket already waited for (or never issued)");
    if (st == 4) { (void)co_claim_fetch(c, &t); st = t.state.load(std::memory_order_acquire); }
    if (st != 2) return KH_OK;                  // queued, on the device, or the dispatcher is copying its rows right now
    *done = 1;
    return co_wait(e, ticket);                  // settled: returns at once with the ticket's status
}

int co_set_coalesce(kh_engine* e, int target_batch, int max_wait_us)
{
    if (!e || target_batch < 0 || target_batch > CO_ROWS || max_wait_us < 0 || max_wait_us > 1000000)
        return fail(KH_ERR_INVALID, "target_batch in [0, %d], max_wait_us in [0, 1000000]", CO_ROWS);
    e->co_target = target_batch;
    e->co_wait_us = max_wait_us;
    if (e->co) { e->co->submits.fetch_add(1); e->co->cv_lane.notify_all(); }
    return KH_OK;
}

int co_set_callers(kh_engine* e, int callers)
{
    if (!e || callers < 0 || callers > KH_MAX_OUTSTANDING) return fail(KH_ERR_INVALID, "callers in [0, %d]", KH_MAX_OUTSTANDING);
    e->co_callers = callers;
    if (e->co) { e->co->submits.fetch_add(1); e->co->cv_lane.notify_all(); }
    return KH_OK;
}

int co_stats(kh_engine* e, int64_t* launches, int64_t* rows)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    int64_t l = 0, r = 0;
    if (e->co) { std::lock_guard<SpinLock> lk(e->co->mu); l = e->co->launches; r = e->co->rows_launched; }
    if (launches) *launches = l;
    if (rows) *rows = r;
    return KH_OK;
}

int co_encode_infer_legal(kh_engine* e, const kh_board* boards, int batch, const int32_t* action_offsets,
                          const int32_t* actions, float* priors, float* value)
{
    const LegalIO l{ action_offsets, actions, priors };
    // counts this call as inside the engine until it returns, whichever path it takes
    SmallCall sc(e, batch >= 1 && batch <= CO_SMALL_LEGAL / 4 && action_offsets && actions && priors);
    if (sc.others) {
        int64_t t;
        const int rc = co_submit(e, 0, boards, nullptr, batch, action_offsets, actions, priors, value, nullptr, &t);
        return rc ? rc : co_wait(e, t);
    }
    return infer_host(e, { .boards = boards, .batch = batch, .value = value, .legal = &l });
}

}  // namespace kh
