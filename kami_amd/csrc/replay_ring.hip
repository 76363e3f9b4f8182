// replay_ring.hip — the replay ring of compact records in device memory (kh_replay_*).
//
// CompactReplayBuffer (host/replaybuffer.h) with its storage on the GPU.  head, the count of records ever added and the
// generator stay on the host under the ring's mutex and follow the host ring step for step; the records lie in
// RecordBlock(capacity) layout, the one expand_records_kernel reads, so kh_train_replay (train_ingest.hip) trains from
// the ring in place.  Records arrive and leave as kh_record structs (664-byte stride):
//
//   validate   one wavefront per record: records_check's rules and its first offence, found without the host
//   scatter    structs -> the ring's arrays at slot (start + w) % capacity; does nothing once the validator has spoken
//   gather     the ring's arrays -> structs, driven by a slot list (kh_replay_read, kh_replay_select)
//
// A record is 83 eight-byte words and every array of the ring starts 16-byte aligned with a stride that is a multiple
// of 8, so scatter and gather move whole words: lane q takes word q, lanes 0..18 also word q + 64.  Word 10 holds value
// and nact, which go to two arrays.
#include "replay_ring.h"

#include <algorithm>
#include <cstddef>
#include <cstring>

namespace kh {

constexpr int RR_WAVES = 4;                                        // records per workgroup
constexpr int RR_WORDS = (int)(sizeof(kh_record) / 8);             // 83
constexpr int RR_CHUNK = 1 << 15;                                  // records per staged pass of a host add, read or select: 21 MB
constexpr unsigned long long RR_CLEAN = ~0ull;                     // the validator's word while no record has offended
static_assert(sizeof(kh_record) == 664 && sizeof(kh_record) % 8 == 0, "records move as 8-byte words");
static_assert(offsetof(kh_record, value) == 80 && offsetof(kh_record, nact) == 84 && offsetof(kh_record, actions) == 88 &&
              offsetof(kh_record, visits) == 280, "the word map below");
constexpr int RR_W_VALUE = 10, RR_W_ACTIONS = 11, RR_W_VISITS = 35;     // first word of each field (boards: 0)

// The validator's word: the smallest key of the launch, by one atomicMin per offending record.  Keys order by record
// index first; a record has one offence (its first), so the rest of the key only carries it to the host:
//   bits 63..33 record index | bit 32: 0 = nact, 1 = an entry | nact (32 bits), or entry k << 17 | twice << 16 | action
__device__ __forceinline__ unsigned long long rr_key_nact(long long i, int nact)
{
    return (unsigned long long)i << 33 | (unsigned)nact;
}
__device__ __forceinline__ unsigned long long rr_key_entry(long long i, int k, bool twice, int action)
{
    return (unsigned long long)i << 33 | 1ull << 32 | (unsigned long long)k << 17 | (twice ? 1u << 16 : 0u) | ((unsigned)action & 0xffffu);
}

// Lane l holds entries l and l + 64 (l < 32).  Entry k offends when k < nact and it is out of range or equals an
// earlier entry j < k (an earlier entry that is itself out of range offends first, at j: the smallest k decides, as in
// records_check's scan).  Distinctness by broadcast: entry j goes to every lane, which compares its own entries behind j.
__global__ __launch_bounds__(64 * RR_WAVES) void replay_validate_kernel(const char* __restrict__ rec, int n, unsigned long long* __restrict__ err)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long i = (long long)blockIdx.x * RR_WAVES + wave;                 // wave-uniform
    if (i >= n) return;
    const char* r = rec + (size_t)i * sizeof(kh_record);
    const int nact = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int32_t*>(r + offsetof(kh_record, nact)));
    if (nact < 0 || nact > KH_MAX_RECORD_ACTIONS) {
        if (lane == 0) atomicMin(err, rr_key_nact(i, nact));
        return;
    }
    const int16_t* act = reinterpret_cast<const int16_t*>(r + offsetof(kh_record, actions));
    const int a0 = act[lane];
    const int a1 = lane < KH_MAX_RECORD_ACTIONS - 64 ? act[lane + 64] : 0;
    bool twice0 = false, twice1 = false;
    const int lo = nact < 64 ? nact : 64;
    for (int j = 0; j < lo; ++j) {
        const int v = __shfl(a0, j);
        twice0 |= j < lane && v == a0;
        twice1 |= v == a1;                                                       // (j < 64 <= lane + 64)
    }
    for (int j = 64; j < nact; ++j) {
        const int v = __shfl(a1, j - 64);
        twice1 |= j < lane + 64 && v == a1;
    }
    const bool bad0 = lane < nact && ((unsigned)a0 >= (unsigned)KH_PSIZE || twice0);
    const bool bad1 = lane + 64 < nact && ((unsigned)a1 >= (unsigned)KH_PSIZE || twice1);      // (nact <= 96: lane < 32)
    const unsigned long long b0 = __ballot(bad0), b1 = __ballot(bad1);
    if (!(b0 | b1)) return;
    const int src = b0 ? __ffsll((long long)b0) - 1 : __ffsll((long long)b1) - 1;             // the first offending entry's lane
    const int a = b0 ? __shfl(a0, src) : __shfl(a1, src);
    const int k = b0 ? src : src + 64;
    // out of range is judged before distinctness (records_check)
    if (lane == 0) atomicMin(err, rr_key_entry(i, k, (unsigned)a < (unsigned)KH_PSIZE, a));
}

struct RingArrays { uint64_t* boards; float* value; int32_t* nact; uint64_t* actions; uint64_t* visits; };

__device__ __forceinline__ void rr_put(const RingArrays& g, size_t slot, int q, uint64_t w)
{
    if (q < RR_W_VALUE) g.boards[slot * RR_W_VALUE + q] = w;
    else if (q == RR_W_VALUE) {
        g.value[slot] = __uint_as_float((uint32_t)w);
        g.nact[slot] = (int32_t)(uint32_t)(w >> 32);
    } else if (q < RR_W_VISITS) g.actions[slot * (RR_W_VISITS - RR_W_ACTIONS) + (q - RR_W_ACTIONS)] = w;
    else g.visits[slot * (RR_WORDS - RR_W_VISITS) + (q - RR_W_VISITS)] = w;
}

__device__ __forceinline__ uint64_t rr_get(const RingArrays& g, size_t slot, int q)
{
    if (q < RR_W_VALUE) return g.boards[slot * RR_W_VALUE + q];
    if (q == RR_W_VALUE) return (uint64_t)__float_as_uint(g.value[slot]) | (uint64_t)(uint32_t)g.nact[slot] << 32;
    if (q < RR_W_VISITS) return g.actions[slot * (RR_W_VISITS - RR_W_ACTIONS) + (q - RR_W_ACTIONS)];
    return g.visits[slot * (RR_WORDS - RR_W_VISITS) + (q - RR_W_VISITS)];
}

// record w of `rec` -> slot (start + w) % capacity, count <= capacity records: no two of a launch share a slot
__global__ __launch_bounds__(64 * RR_WAVES) void replay_scatter_kernel(const uint64_t* __restrict__ rec, int count, int start, int capacity,
                                                                       RingArrays g, const unsigned long long* __restrict__ err)
{
    if (*err != RR_CLEAN) return;                                               // a record of this add is invalid: the ring stays as it was
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long w = (long long)blockIdx.x * RR_WAVES + wave;
    if (w >= count) return;
    const size_t slot = (size_t)(((long long)start + w) % capacity);
    const uint64_t* src = rec + (size_t)w * RR_WORDS;
    rr_put(g, slot, lane, src[lane]);
    if (lane + 64 < RR_WORDS) rr_put(g, slot, lane + 64, src[lane + 64]);
}

// slot slots[w] -> record w of `rec`
__global__ __launch_bounds__(64 * RR_WAVES) void replay_gather_kernel(uint64_t* __restrict__ rec, int count, const int32_t* __restrict__ slots,
                                                                      int capacity, RingArrays g)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long w = (long long)blockIdx.x * RR_WAVES + wave;
    if (w >= count) return;
    const int s = slots[w];
    if (s < 0 || s >= capacity) return;                                         // (the host sends none such)
    uint64_t* dst = rec + (size_t)w * RR_WORDS;
    dst[lane] = rr_get(g, (size_t)s, lane);
    if (lane + 64 < RR_WORDS) dst[lane + 64] = rr_get(g, (size_t)s, lane + 64);
}

namespace {

RingArrays arrays(const kh_replay* r)
{
    char* p = r->mem.as<char>();
    return { reinterpret_cast<uint64_t*>(p + r->lay.boards), reinterpret_cast<float*>(p + r->lay.value),
             reinterpret_cast<int32_t*>(p + r->lay.nact), reinterpret_cast<uint64_t*>(p + r->lay.actions),
             reinterpret_cast<uint64_t*>(p + r->lay.visits) };
}

dim3 grid_for(int records) { return dim3((unsigned)((records + RR_WAVES - 1) / RR_WAVES)); }

// the pinned block: the validator's word in front, a slot list behind it
unsigned long long* pin_word(kh_replay* r) { return reinterpret_cast<unsigned long long*>(r->pin.at(0)); }
int32_t* pin_slots(kh_replay* r) { return reinterpret_cast<int32_t*>(r->pin.at(16)); }

int use_ring(kh_replay* r) { HIPCHK(hipSetDevice(r->device)); return KH_OK; }

// the message records_check gives for the offence a key names
int key_fail(unsigned long long key, int* bad_index)
{
    const int record = (int)(key >> 33);
    if (bad_index) *bad_index = record;
    if (!(key >> 32 & 1)) return record_fail(RECORD_BAD_NACT, record, (int)(int32_t)(uint32_t)key, 0);
    const int entry = (int)(key >> 17 & 0x7fff), action = (int)(int16_t)(uint16_t)key;
    return record_fail(key >> 16 & 1 ? RECORD_BAD_TWICE : RECORD_BAD_RANGE, record, action, entry);
}

void advance(kh_replay* r, int n)
{
    r->head = (int)(((int64_t)r->head + n) % r->capacity);
    r->added += n;
}

// the slots of `count` records from `slots` (pinned) into out, through the staging block
int gather_out(kh_replay* r, int count, kh_record* out)
{
    HIPCHK(hipMemcpyAsync(r->slots.p, pin_slots(r), (size_t)count * 4, hipMemcpyHostToDevice, r->st));
    hipLaunchKernelGGL(replay_gather_kernel, grid_for(count), dim3(64 * RR_WAVES), 0, r->st, r->stage.as<uint64_t>(), count,
                       r->slots.as<int32_t>(), r->capacity, arrays(r));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, r->stage.p, (size_t)count * sizeof(kh_record), hipMemcpyDeviceToHost, r->st));
    HIPCHK(hipStreamSynchronize(r->st));                      // the slot list and the staging block are written again for the next chunk
    return KH_OK;
}

template <class NextSlot> int read_slots(kh_replay* r, int n, kh_record* out, NextSlot next)
{
    int rc = use_ring(r);
    if (rc) return rc;
    const int chunk = std::min(n, RR_CHUNK);
    if (r->stage.ensure((size_t)chunk * sizeof(kh_record)) || r->slots.ensure((size_t)chunk * 4) || r->pin.ensure(16 + (size_t)chunk * 4))
        return KH_ERR_HIP;
    for (int base = 0; base < n; base += chunk) {
        const int m = std::min(chunk, n - base);
        int32_t* s = pin_slots(r);
        for (int k = 0; k < m; ++k) s[k] = next();
        if ((rc = gather_out(r, m, out + base))) return rc;
    }
    return KH_OK;
}

}  // namespace
}  // namespace kh

using namespace kh;

extern "C" {

int kh_replay_create(kh_engine* e, int capacity, uint64_t seed, kh_replay** out)
{
    if (!out) return fail(KH_ERR_INVALID, "null out");
    *out = nullptr;
    if (capacity < 1 || capacity > (1 << 24)) return fail(KH_ERR_INVALID, "ring capacity %d outside [1, %d]", capacity, 1 << 24);
    if (!e) return fail(KH_ERR_INVALID, "null argument");
    int rc = set_device(e);
    if (rc) return rc;
    std::unique_ptr<kh_replay, void (*)(kh_replay*)> r(new kh_replay(), kh_replay_destroy);
    r->device = e->cfg.device;
    r->capacity = capacity;
    r->lay = RecordBlock((size_t)capacity);
    r->rng.seed(seed);
    HIPCHK(hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking));
    if (r->mem.ensure(r->lay.bytes) || r->err.ensure(8) || r->pin.ensure(16 + 4096)) return KH_ERR_HIP;
    HIPCHK(hipMemsetAsync(r->mem.p, 0, r->lay.bytes, r->st));
    HIPCHK(hipStreamSynchronize(r->st));
    *out = r.release();
    return KH_OK;
}

void kh_replay_destroy(kh_replay* r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->st) { (void)hipStreamSynchronize(r->st); (void)hipStreamDestroy(r->st); }
    delete r;
}

int kh_replay_add(kh_replay* r, const kh_record* rec, int n, int* bad_index)
{
    if (bad_index) *bad_index = -1;
    if (!r) return fail(KH_ERR_INVALID, "null argument");
    int rc = records_check(rec, n, bad_index);
    if (rc) return rc;
    if (n == 0) return KH_OK;
    std::lock_guard<std::mutex> lk(r->mu);
    if ((rc = use_ring(r))) return rc;
    // of more records than the ring holds only the last `capacity` stay: the others are never sent
    const int first = std::max(0, n - r->capacity), count = n - first;
    const int chunk = std::min(count, RR_CHUNK);
    if (r->stage.ensure((size_t)chunk * sizeof(kh_record))) return KH_ERR_HIP;
    *pin_word(r) = RR_CLEAN;                                   // validated above
    HIPCHK(hipMemcpyAsync(r->err.p, pin_word(r), 8, hipMemcpyHostToDevice, r->st));
    for (int base = 0; base < count; base += chunk) {
        const int m = std::min(chunk, count - base);
        HIPCHK(hipMemcpyAsync(r->stage.p, rec + first + base, (size_t)m * sizeof(kh_record), hipMemcpyHostToDevice, r->st));
        hipLaunchKernelGGL(replay_scatter_kernel, grid_for(m), dim3(64 * RR_WAVES), 0, r->st, r->stage.as<uint64_t>(), m,
                           (int)(((int64_t)r->head + first + base) % r->capacity), r->capacity, arrays(r), r->err.as<unsigned long long>());
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(r->st));
    advance(r, n);
    return KH_OK;
}

int kh_replay_add_device(kh_replay* r, const void* d_rec, int n, void* stream, int* bad_index)
{
    if (bad_index) *bad_index = -1;
    if (!r) return fail(KH_ERR_INVALID, "null argument");
    if (n < 0 || (n > 0 && !d_rec)) return fail(KH_ERR_INVALID, "records: a buffer and n >= 0 required");
    if (n == 0) return KH_OK;
    {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, d_rec) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != r->device) {
            (void)hipGetLastError();
            return fail(KH_ERR_INVALID, "d_rec is not device memory of device %d", r->device);
        }
        if (reinterpret_cast<uintptr_t>(d_rec) % 8) return fail(KH_ERR_INVALID, "d_rec must be 8-byte aligned");
        void* base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, const_cast<void*>(d_rec)) != hipSuccess) (void)hipGetLastError();
        else if (static_cast<const char*>(d_rec) + (size_t)n * sizeof(kh_record) > static_cast<const char*>(base) + size)
            return fail(KH_ERR_INVALID, "d_rec: %d records do not fit its allocation", n);
    }
    std::lock_guard<std::mutex> lk(r->mu);
    int rc = use_ring(r);
    if (rc) return rc;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : r->st;
    const int first = std::max(0, n - r->capacity), count = n - first;
    const char* rec = static_cast<const char*>(d_rec);
    unsigned long long* word = r->err.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(word, 0xff, 8, st));
    hipLaunchKernelGGL(replay_validate_kernel, grid_for(n), dim3(64 * RR_WAVES), 0, st, rec, n, word);
    hipLaunchKernelGGL(replay_scatter_kernel, grid_for(count), dim3(64 * RR_WAVES), 0, st,
                       reinterpret_cast<const uint64_t*>(rec + (size_t)first * sizeof(kh_record)), count,
                       (int)(((int64_t)r->head + first) % r->capacity), r->capacity, arrays(r), word);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pin_word(r), word, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                          // the one synchronisation of the call
    if (*pin_word(r) != RR_CLEAN) return key_fail(*pin_word(r), bad_index);
    advance(r, n);
    return KH_OK;
}

int64_t kh_replay_count(kh_replay* r)
{
    if (!r) return 0;
    std::lock_guard<std::mutex> lk(r->mu);
    return r->added;
}

int kh_replay_size(kh_replay* r) { return r ? r->capacity : 0; }

int kh_replay_clear(kh_replay* r)
{
    if (!r) return fail(KH_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(r->mu);
    int rc = use_ring(r);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(r->mem.p, 0, r->lay.bytes, r->st));
    HIPCHK(hipStreamSynchronize(r->st));
    r->head = 0;
    r->added = 0;
    return KH_OK;
}

int kh_replay_read(kh_replay* r, int first_slot, int n, kh_record* out)
{
    if (!r) return fail(KH_ERR_INVALID, "null argument");
    if (n < 0 || (n > 0 && !out)) return fail(KH_ERR_INVALID, "kh_replay_read: a buffer and n >= 0 required");
    if (first_slot < 0 || first_slot >= r->capacity) return fail(KH_ERR_INVALID, "kh_replay_read: slot %d outside [0, %d)", first_slot, r->capacity);
    if (n == 0) return KH_OK;
    std::lock_guard<std::mutex> lk(r->mu);
    int slot = first_slot;
    return read_slots(r, n, out, [&]() { const int s = slot; slot = slot + 1 == r->capacity ? 0 : slot + 1; return s; });
}

int kh_replay_select(kh_replay* r, int n, kh_record* out)
{
    if (!r) return fail(KH_ERR_INVALID, "null argument");
    if (n < 0 || (n > 0 && !out)) return fail(KH_ERR_INVALID, "kh_replay_select: a buffer and n >= 0 required");
    if (n == 0) return KH_OK;
    std::lock_guard<std::mutex> lk(r->mu);
    return read_slots(r, n, out, [&]() { return (int32_t)(r->rng() % (uint64_t)r->capacity); });
}

}  // extern "C"
