// eval.hip — the loss of the network as served on compact replay records (kh_eval_records, kh_eval_replay).
//
// No forward of its own: a call runs the engine's serving forward — the internal path of kh_encode_infer_device, at the
// engine's dtype, through the existing dispatch — on at most KH_EVAL_CHUNK boards at a time, which leaves policy[4672]
// and value[256] per position in per-engine scratch, and eval_rows_kernel turns those rows and the records' targets
// (RecordBlock layout: the call's own upload, or a replay ring read where it lies) into three numbers per record:
//
//   Lp    = - sum_{k < nact} visits[k] * log(p[actions[k]] + 0.001)       (0 for nact == 0)
//   Lv    = (1 / 256) sum_j (v[j] - value)^2                               (the target broadcast, as nn.cpp:96 does)
//   agree = nact > 0 and the entry with the most visits is the entry with the largest p[actions[k]]
//
// in double, whatever the forward's dtype.  One wavefront per record; lane k owns entries k and k + 64 and one float4
// of the value row; every reduction is a butterfly over the wave in a fixed order, so a record's results depend on
// nothing but that record and its two rows.  eval_reduce_kernel adds the records of one chunk of the call (records
// c * KH_EVAL_CHUNK ... in call order, wherever a ring's wrap cuts the forward) in a fixed order and the host adds the
// chunks' sums in chunk order: the totals' order of summation depends on n alone.
#include "replay_ring.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace kh {

constexpr int EV_WAVES = 4;                    // records per workgroup
constexpr int EV_NONE = 0x7fffffff;            // "no entry" in an argmax pair
constexpr int EV_PART = 4;                     // doubles per chunk sum: Lp, Lv, agreeing records, records with nact > 0
static_assert(KH_VALUE_WIDTH == 64 * 4, "the value row is one float4 per lane");
static_assert(KH_MAX_RECORD_ACTIONS > 64 && KH_MAX_RECORD_ACTIONS <= 128, "lane k owns entries k and k + 64");
static_assert(sizeof(kh_eval_result) == 64, "kh_eval_result is 64 bytes");

// butterfly sums: after the six exchanges every lane holds the same bits (a + b and b + a round alike)
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int lo = __shfl_xor(__double2loint(x), m), hi = __shfl_xor(__double2hiint(x), m);
        x += __hiloint2double(hi, lo);
    }
    return x;
}

__device__ __forceinline__ int wave_sum(int x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// (value, entry) pairs: the larger value wins, the lower entry among equals; EV_NONE loses to everything
__device__ __forceinline__ void best_of(float& v, int& k, float ov, int ok)
{
    if (ok != EV_NONE && (k == EV_NONE || ov > v || (ov == v && ok < k))) { v = ov; k = ok; }
}

__device__ __forceinline__ void wave_best(float& v, int& k)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(v, m);
        const int ok = __shfl_xor(k, m);
        best_of(v, k, ov, ok);
    }
}

// rows [0, count) of policy / vfull against the records in slots base + r; results to lp / lv / tag[r]
// (tag: bit 0 agree, bit 1 nact > 0); flags[0] |= 1 on a NaN policy entry, flags[1] |= 1 on a NaN value
__global__ __launch_bounds__(64 * EV_WAVES) void eval_rows_kernel(
    const float* __restrict__ policy, const float* __restrict__ vfull, const float* __restrict__ value,
    const int32_t* __restrict__ nact, const int16_t* __restrict__ actions, const float* __restrict__ visits, int base, int count,
    double* __restrict__ lp, double* __restrict__ lv, int32_t* __restrict__ tag, int* __restrict__ flags)
{
    using f4 = float __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.x * EV_WAVES + wave;            // row of the chunk, wave-uniform
    if (r >= count) return;
    const size_t src = (size_t)base + r;
    int n = __builtin_amdgcn_readfirstlane(nact[src]);
    n = n < 0 ? 0 : (n > KH_MAX_RECORD_ACTIONS ? KH_MAX_RECORD_ACTIONS : n);      // (validated: never out of range)
    const float* p = policy + (size_t)r * KH_PSIZE;
    const size_t row = src * KH_MAX_RECORD_ACTIONS;

    double s = 0.0;
    float vis_v = 0.0f, pol_v = 0.0f;
    int vis_k = EV_NONE, pol_k = EV_NONE;
    bool nan_p = false;
    if (lane == 0) { const float p0 = p[0]; nan_p = p0 != p0; }                    // a record without entries is covered too
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        if (k < n) {
            int a = actions[row + k];
            a = (unsigned)a < (unsigned)KH_PSIZE ? a : 0;                         // (validated: never out of range)
            const float pk = p[a], vk = visits[row + k];
            nan_p |= pk != pk;
            s += (double)vk * log((double)pk + 0.001);
            best_of(vis_v, vis_k, vk, k);
            best_of(pol_v, pol_k, pk, k);
        }
    }

    const f4 v = reinterpret_cast<const f4*>(vfull + (size_t)r * KH_VALUE_WIDTH)[lane];
    const double target = (double)value[src];
    const double d0 = (double)v.x - target, d1 = (double)v.y - target, d2 = (double)v.z - target, d3 = (double)v.w - target;
    double q = d0 * d0;
    q += d1 * d1;
    q += d2 * d2;
    q += d3 * d3;
    const bool nan_v = v.x != v.x || v.y != v.y || v.z != v.z || v.w != v.w;

    s = wave_sum(s);
    q = wave_sum(q);
    wave_best(vis_v, vis_k);
    wave_best(pol_v, pol_k);
    const bool any_p = __ballot(nan_p) != 0, any_v = __ballot(nan_v) != 0;
    if (lane == 0) {
        lp[r] = 0.0 - s;
        lv[r] = q * (1.0 / KH_VALUE_WIDTH);
        tag[r] = n > 0 ? 2 | (vis_k == pol_k ? 1 : 0) : 0;
        if (any_p) atomicOr(&flags[0], 1);
        if (any_v) atomicOr(&flags[1], 1);
    }
}

// the sums of one chunk's `count` records: one wavefront, lane l adds records l, l + 64, ... in that order, then the wave.
// All of a lane's loads are issued before the first addition: a loop that loads as it adds pays one memory latency per
// record (6.0 us per chunk measured, against 4.3 us for eval_rows_kernel).
constexpr int EV_PER_LANE = KH_EVAL_CHUNK / 64;
static_assert(KH_EVAL_CHUNK % 64 == 0, "a chunk is whole rounds of the reducing wave");
__global__ __launch_bounds__(64) void eval_reduce_kernel(const double* __restrict__ lp, const double* __restrict__ lv,
                                                         const int32_t* __restrict__ tag, int count, double* __restrict__ part)
{
    const int lane = threadIdx.x;
    double a[EV_PER_LANE], b[EV_PER_LANE];
    int t[EV_PER_LANE];
#pragma unroll
    for (int j = 0; j < EV_PER_LANE; ++j) {
        const int i = lane + 64 * j;
        const bool on = i < count;
        a[j] = on ? lp[i] : 0.0;
        b[j] = on ? lv[i] : 0.0;
        t[j] = on ? tag[i] : 0;
    }
    double s = 0.0, q = 0.0;
    int agree = 0, with = 0;
#pragma unroll
    for (int j = 0; j < EV_PER_LANE; ++j) {
        if (lane + 64 * j < count) { s += a[j]; q += b[j]; }
        agree += t[j] & 1;
        with += t[j] >> 1 & 1;
    }
    s = wave_sum(s);
    q = wave_sum(q);
    agree = wave_sum(agree);
    with = wave_sum(with);
    if (lane == 0) {
        part[0] = s;
        part[1] = q;
        part[2] = (double)agree;
        part[3] = (double)with;
    }
}

namespace {

// where the per-record results of one chunk lie in EvalCache::rows
struct Rows {
    double *lp, *lv;
    int32_t* tag;
    explicit Rows(const DevMem& m) : lp(m.as<double>()), lv(lp + KH_EVAL_CHUNK), tag(reinterpret_cast<int32_t*>(lv + KH_EVAL_CHUNK)) {}
    static constexpr size_t bytes = (size_t)KH_EVAL_CHUNK * (8 + 8 + 4);
};

// Records first .. first + n - 1 (mod cap) of a record block in device memory, n <= cap, on the parameter set W; dmu held.
int eval_run(kh_engine* e, const Weights& W, hipStream_t st, const char* block, const RecordBlock& lay, int first, int cap, int n,
             kh_eval_result* out, double* rec_lp, double* rec_lv)
{
    EvalCache& ec = e->eval;
    const int nchunks = (n + KH_EVAL_CHUNK - 1) / KH_EVAL_CHUNK, rows_cap = std::min(n, KH_EVAL_CHUNK);
    const bool per_record = rec_lp || rec_lv;
    // page-locked results: flags | the chunks' sums | Lp[n] | Lv[n] (the last two only when the caller wants them)
    const size_t o_part = 16, o_lp = o_part + (size_t)nchunks * EV_PART * 8, o_lv = o_lp + (per_record ? (size_t)n * 8 : 0),
                 out_bytes = o_lv + (per_record ? (size_t)n * 8 : 0);
    if (ec.policy.ensure((size_t)rows_cap * KH_PSIZE * 4) || ec.vfull.ensure((size_t)rows_cap * KH_VALUE_WIDTH * 4) ||
        ec.rows.ensure(Rows::bytes) || ec.parts.ensure((size_t)nchunks * EV_PART * 8) || ec.flags.ensure(16) || ec.pin_out.ensure(out_bytes))
        return KH_ERR_HIP;
    const Rows rows(ec.rows);
    float *policy = ec.policy.as<float>(), *vfull = ec.vfull.as<float>();
    int* flags = ec.flags.as<int>();
    const kh_board* boards = reinterpret_cast<const kh_board*>(block + lay.boards);

    // KAMI_EVAL_TRACE=1: the call's stream work and, of it, the forward and the two loss kernels, by events on the stream
    const bool trace = getenv("KAMI_EVAL_TRACE") && atoi(getenv("KAMI_EVAL_TRACE")) != 0;
    std::vector<hipEvent_t> ev;
    if (trace) {
        ev.resize(2 + 2 * (size_t)nchunks);
        for (auto& x : ev) HIPCHK(hipEventCreate(&x));
        HIPCHK(hipEventRecord(ev[0], st));
    }
    HIPCHK(hipMemsetAsync(flags, 0, 16, st));
    for (int c = 0; c < nchunks; ++c) {
        const int i0 = c * KH_EVAL_CHUNK, m = std::min(KH_EVAL_CHUNK, n - i0);
        // the chunk's forward, cut where the block wraps: rows [0, m1) from slot s on, the rest from slot 0
        const int s = (int)(((int64_t)first + i0) % cap), m1 = std::min(m, cap - s);
        const int seg_slot[2] = { s, 0 }, seg_row[2] = { 0, m1 }, seg_n[2] = { m1, m - m1 };
        for (int g = 0; g < 2; ++g) {
            if (seg_n[g] <= 0) continue;
            hipStream_t used;
            int rc = encode_infer_on_device(e, W, boards + seg_slot[g], seg_n[g], policy + (size_t)seg_row[g] * KH_PSIZE,
                                            vfull + (size_t)seg_row[g] * KH_VALUE_WIDTH, st, &used);
            if (rc) return rc;
        }
        if (trace) HIPCHK(hipEventRecord(ev[2 + 2 * (size_t)c], st));
        for (int g = 0; g < 2; ++g) {
            if (seg_n[g] <= 0) continue;
            hipLaunchKernelGGL(eval_rows_kernel, dim3((seg_n[g] + EV_WAVES - 1) / EV_WAVES), dim3(64 * EV_WAVES), 0, st,
                               policy + (size_t)seg_row[g] * KH_PSIZE, vfull + (size_t)seg_row[g] * KH_VALUE_WIDTH,
                               reinterpret_cast<const float*>(block + lay.value), reinterpret_cast<const int32_t*>(block + lay.nact),
                               reinterpret_cast<const int16_t*>(block + lay.actions), reinterpret_cast<const float*>(block + lay.visits),
                               seg_slot[g], seg_n[g], rows.lp + seg_row[g], rows.lv + seg_row[g], rows.tag + seg_row[g], flags);
        }
        hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(64), 0, st, rows.lp, rows.lv, rows.tag, m,
                           ec.parts.as<double>() + (size_t)c * EV_PART);
        HIPCHK(hipGetLastError());
        if (trace) HIPCHK(hipEventRecord(ev[3 + 2 * (size_t)c], st));
        if (per_record) {
            HIPCHK(hipMemcpyAsync(ec.pin_out.at(o_lp + (size_t)i0 * 8), rows.lp, (size_t)m * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(ec.pin_out.at(o_lv + (size_t)i0 * 8), rows.lv, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipMemcpyAsync(ec.pin_out.at(o_part), ec.parts.p, (size_t)nchunks * EV_PART * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ec.pin_out.at(0), flags, 16, hipMemcpyDeviceToHost, st));
    if (trace) HIPCHK(hipEventRecord(ev[1], st));
    HIPCHK(hipStreamSynchronize(st));                         // the one synchronisation of the call
    if (trace) {
        float all = 0.0f, fwd = 0.0f, loss = 0.0f;
        HIPCHK(hipEventElapsedTime(&all, ev[0], ev[1]));
        for (int c = 0; c < nchunks; ++c) {
            float t = 0.0f;
            HIPCHK(hipEventElapsedTime(&t, c ? ev[1 + 2 * (size_t)c] : ev[0], ev[2 + 2 * (size_t)c]));       // (behind chunk c - 1's loss)
            fwd += t;
            HIPCHK(hipEventElapsedTime(&t, ev[2 + 2 * (size_t)c], ev[3 + 2 * (size_t)c]));
            loss += t;
        }
        for (auto& x : ev) (void)hipEventDestroy(x);
        fprintf(stderr, "kh_eval: %d records in %d chunks: %.3f ms on the stream, %.3f ms of it in the forward, %.3f ms in the loss kernels\n",
                n, nchunks, all, fwd, loss);
    }
    const int* fl = reinterpret_cast<const int*>(ec.pin_out.at(0));
    if (fl[0]) return fail(KH_ERR_NAN_POLICY, "inference policy output contains NaN");   // kh_infer's, in kh_infer's order
    if (fl[1]) return fail(KH_ERR_NAN_VALUE, "inference value output contains NaN");
    const double* part = reinterpret_cast<const double*>(ec.pin_out.at(o_part));
    double lp = 0.0, lv = 0.0;
    int64_t agree = 0, with = 0;
    for (int c = 0; c < nchunks; ++c) {
        lp += part[c * EV_PART];
        lv += part[c * EV_PART + 1];
        agree += (int64_t)part[c * EV_PART + 2];
        with += (int64_t)part[c * EV_PART + 3];
    }
    kh_eval_result res = {};
    res.records = n;
    res.policy_records = with;
    res.policy_loss = lp / (double)n;
    res.value_loss = lv / (double)n;
    res.top1 = with ? (double)agree / (double)with : 0.0;
    res.generation = W.generation;
    *out = res;
    if (rec_lp) memcpy(rec_lp, ec.pin_out.at(o_lp), (size_t)n * 8);
    if (rec_lv) memcpy(rec_lv, ec.pin_out.at(o_lv), (size_t)n * 8);
    return KH_OK;
}

// the stream of the device calls' slot (created on first use); dmu held
int eval_stream(kh_engine* e, int rows, hipStream_t* st)
{
    if (!e->devslot) e->devslot.reset(new Slot());
    int rc = slot_ensure(e, *e->devslot, rows, false);
    if (rc) return rc;
    *st = e->devslot->stream;
    return KH_OK;
}

}  // namespace
}  // namespace kh

using namespace kh;

extern "C" {

int kh_eval_records(kh_engine* e, const kh_record* rec, int n, kh_eval_result* out, double* record_policy_loss, double* record_value_loss)
{
    if (!e || !rec || !out) return fail(KH_ERR_INVALID, "null argument");
    if (n < 1) return fail(KH_ERR_INVALID, "kh_eval_records: n >= 1 required");
    int rc = check_records(e, "kh_eval_records");
    if (rc) return rc;
    if ((rc = records_check(rec, n, nullptr))) return rc;
    auto W = current_weights(e);                              // every chunk runs on this set
    if (!W) return fail(KH_ERR_NO_WEIGHTS, "kh_eval_records before kh_load_weights");
    if ((rc = set_device(e))) return rc;
    std::lock_guard<std::mutex> lk(e->dmu);
    hipStream_t st;
    if ((rc = eval_stream(e, std::min(n, KH_EVAL_CHUNK), &st))) return rc;
    EvalCache& ec = e->eval;
    const RecordBlock lay((size_t)n);
    if (ec.pin_rec.ensure(lay.bytes) || ec.rec.ensure(lay.bytes)) return KH_ERR_HIP;
    lay.pack(ec.pin_rec.at(0), rec, (size_t)n);
    HIPCHK(hipMemcpyAsync(ec.rec.p, ec.pin_rec.p, lay.bytes, hipMemcpyHostToDevice, st));
    return eval_run(e, *W, st, ec.rec.as<char>(), lay, 0, n, n, out, record_policy_loss, record_value_loss);
}

int kh_eval_replay(kh_engine* e, kh_replay* r, int first_slot, int n, kh_eval_result* out, double* record_policy_loss,
                   double* record_value_loss)
{
    if (!e || !r || !out) return fail(KH_ERR_INVALID, "null argument");
    int rc = check_records(e, "kh_eval_replay");
    if (rc) return rc;
    if (first_slot < 0 || first_slot >= r->capacity) return fail(KH_ERR_INVALID, "kh_eval_replay: slot %d outside [0, %d)", first_slot, r->capacity);
    if (n < 1 || n > r->capacity) return fail(KH_ERR_INVALID, "kh_eval_replay: n %d outside [1, %d]", n, r->capacity);
    if (r->device != e->cfg.device)
        return fail(KH_ERR_INVALID, "kh_eval_replay: the ring is on device %d, the engine on device %d", r->device, e->cfg.device);
    auto W = current_weights(e);
    if (!W) return fail(KH_ERR_NO_WEIGHTS, "kh_eval_replay before kh_load_weights");
    if ((rc = set_device(e))) return rc;
    std::lock_guard<std::mutex> ring(r->mu);                  // adds wait; taken before the engine's device-call lock
    std::lock_guard<std::mutex> lk(e->dmu);
    hipStream_t st;
    if ((rc = eval_stream(e, std::min(n, KH_EVAL_CHUNK), &st))) return rc;
    return eval_run(e, *W, st, r->mem.as<char>(), r->lay, first_slot, r->capacity, n, out, record_policy_loss, record_value_loss);
}

}  // extern "C"
