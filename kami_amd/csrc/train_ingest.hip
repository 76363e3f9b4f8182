// train_ingest.hip — compact replay records (kh_record, 664 bytes) as the trainer's input.
//
// kh_train takes dense fp32 rows (26 372 bytes per sample) and stages every batch through the host.  Here the call's
// records and its sample order go up once, and expand_records_kernel writes each batch straight into the buffers the
// recorded training step reads (TrainCache dx / dp / dv): planes through encode_square(), so they are the encoder's
// bits by construction; the 4 672-float visit row; the value.  The step itself — train_step, recorded as a graph — is
// kh_train's, untouched, which is what makes kh_train_records equal to kh_train on the expanded arrays bit for bit.
// kh_train_replay is the same call with a device replay ring (replay_ring.hip) as its record block: nothing but the
// sample order, composed with the ring's draws, goes up.
//
// One wavefront per row, lane = POV square (encode_f32_kernel's structure).  The wave owns 4 672 floats of LDS, used
// twice: as the [64][30] plane tile, then as the visit row, which is zeroed, scattered into and only then streamed
// out, with a barrier between each two of those — the zero fill and the scatter hit the same addresses, and nothing
// here depends on the order in which a wave's global stores land.
#include "replay_ring.h"
#include "encode_square.h"

#include <algorithm>
#include <cstring>

namespace kh {

constexpr int XR_WAVES = 2;                    // waves per workgroup: 2 x 18 688 B of LDS
constexpr int XR_TILE = 64 * KH_NFEATURES;     // floats of planes per position
static_assert(XR_TILE <= KH_PSIZE && XR_TILE % 4 == 0 && KH_PSIZE % 4 == 0, "one LDS row serves both outputs, in 16-byte pieces");

__global__ __launch_bounds__(64 * XR_WAVES) void expand_records_kernel(
    const kh_board* __restrict__ boards, const float* __restrict__ value, const int32_t* __restrict__ nact,
    const int16_t* __restrict__ actions, const float* __restrict__ visits, const int32_t* __restrict__ order,
    int base, int count, float* __restrict__ dx, float* __restrict__ dp, float* __restrict__ dv)
{
    using f4 = float __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float lds[XR_WAVES][KH_PSIZE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.x * XR_WAVES + wave;            // row of the batch, wave-uniform
    const bool on = r < count;
    int src = 0;                                           // record the row comes from
    if (on) src = __builtin_amdgcn_readfirstlane(order ? order[base + r] : base + r);
    float* buf = lds[wave];
    f4* buf4 = reinterpret_cast<f4*>(buf);

    if (on) {
        float v[KH_NFEATURES];
        encode_square(boards + src, lane, v);
        float2* dst = reinterpret_cast<float2*>(buf + lane * KH_NFEATURES);              // 120 B rows: 8-B aligned
#pragma unroll
        for (int i = 0; i < KH_NFEATURES / 2; ++i) dst[i] = make_float2(v[2 * i], v[2 * i + 1]);
    }
    __syncthreads();
    if (on) {
        f4* out = reinterpret_cast<f4*>(dx + (size_t)r * XR_TILE);
        for (int q = lane; q < XR_TILE / 4; q += 64) out[q] = buf4[q];
    }
    __syncthreads();                                       // the tile has been read: the row may take its place
    if (on) {
        const f4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (int q = lane; q < KH_PSIZE / 4; q += 64) buf4[q] = zero;
    }
    __syncthreads();                                       // zeros first ...
    if (on) {
        int n = nact[src];
        n = n < 0 ? 0 : (n > KH_MAX_RECORD_ACTIONS ? KH_MAX_RECORD_ACTIONS : n);
        const size_t row = (size_t)src * KH_MAX_RECORD_ACTIONS;
        for (int k = lane; k < n; k += 64) {
            const int a = actions[row + k];
            if ((unsigned)a < (unsigned)KH_PSIZE) buf[a] = visits[row + k];              // (the host has validated: never out of range)
        }
        if (lane == 0) dv[r] = value[src];
    }
    __syncthreads();                                       // ... then the shares, then the row as a whole
    if (on) {
        f4* out = reinterpret_cast<f4*>(dp + (size_t)r * KH_PSIZE);
        for (int q = lane; q < KH_PSIZE / 4; q += 64) out[q] = buf4[q];
    }
}

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

RecordBlock::RecordBlock(size_t n)
{
    boards = 0;
    value = up16(boards + n * sizeof(kh_board));
    nact = up16(value + n * 4);
    actions = up16(nact + n * 4);
    visits = up16(actions + n * KH_MAX_RECORD_ACTIONS * 2);
    bytes = up16(visits + n * KH_MAX_RECORD_ACTIONS * 4);
}

void RecordBlock::pack(char* dst, const kh_record* rec, size_t n) const
{
    kh_board* b = reinterpret_cast<kh_board*>(dst + boards);
    float* v = reinterpret_cast<float*>(dst + value);
    int32_t* na = reinterpret_cast<int32_t*>(dst + nact);
    int16_t* ac = reinterpret_cast<int16_t*>(dst + actions);
    float* vi = reinterpret_cast<float*>(dst + visits);
    for (size_t i = 0; i < n; ++i) {
        b[i] = rec[i].board;
        v[i] = rec[i].value;
        na[i] = rec[i].nact;
        memcpy(ac + i * KH_MAX_RECORD_ACTIONS, rec[i].actions, sizeof rec[i].actions);
        memcpy(vi + i * KH_MAX_RECORD_ACTIONS, rec[i].visits, sizeof rec[i].visits);
    }
}

void launch_expand_records(const char* d_block, const RecordBlock& lay, const int32_t* d_order, int base, int count,
                           float* dx, float* dp, float* dv, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(expand_records_kernel, dim3((count + XR_WAVES - 1) / XR_WAVES), dim3(64 * XR_WAVES), 0, s,
                       reinterpret_cast<const kh_board*>(d_block + lay.boards), reinterpret_cast<const float*>(d_block + lay.value),
                       reinterpret_cast<const int32_t*>(d_block + lay.nact), reinterpret_cast<const int16_t*>(d_block + lay.actions),
                       reinterpret_cast<const float*>(d_block + lay.visits), d_order, base, count, dx, dp, dv);
}

int record_fail(int rule, int record, int value, int entry)
{
    switch (rule) {
    case RECORD_BAD_NACT: return fail(KH_ERR_INVALID, "record %d: nact %d outside [0, %d]", record, value, KH_MAX_RECORD_ACTIONS);
    case RECORD_BAD_RANGE: return fail(KH_ERR_INVALID, "record %d: action %d (entry %d) outside [0, %d)", record, value, entry, KH_PSIZE);
    default: return fail(KH_ERR_INVALID, "record %d: action %d appears twice (entry %d); actions must be pairwise distinct", record, value, entry);
    }
}

int records_check(const kh_record* rec, int n, int* bad_index)
{
    if (bad_index) *bad_index = -1;
    if (n < 0 || (n > 0 && !rec)) return fail(KH_ERR_INVALID, "records: a buffer and n >= 0 required");
    uint64_t seen[(KH_PSIZE + 63) / 64] = { 0 };
    for (int i = 0; i < n; ++i) {
        const kh_record& r = rec[i];
        auto bad = [&]() { if (bad_index) *bad_index = i; };
        if (r.nact < 0 || r.nact > KH_MAX_RECORD_ACTIONS) {
            bad();
            return record_fail(RECORD_BAD_NACT, i, (int)r.nact, 0);
        }
        int rc = KH_OK, k = 0;
        for (; k < r.nact; ++k) {
            const int a = r.actions[k];
            if (a < 0 || a >= KH_PSIZE) {
                bad();
                rc = record_fail(RECORD_BAD_RANGE, i, a, k);
                break;
            }
            if (seen[a >> 6] >> (a & 63) & 1) {
                bad();
                rc = record_fail(RECORD_BAD_TWICE, i, a, k);
                break;
            }
            seen[a >> 6] |= (uint64_t)1 << (a & 63);
        }
        for (int j = 0; j < k; ++j) seen[r.actions[j] >> 6] = 0;
        if (rc) return rc;
    }
    return KH_OK;
}

constexpr int EXPAND_CHUNK = 512;        // records per pass of kh_expand_records: 13.5 MB of device scratch

}  // namespace kh

using namespace kh;

// A training call on records, behind its argument checks: kh_train_records on the call's own records (`rec`, uploaded in
// RecordBlock(n) layout), kh_train_replay on n draws from a ring (`ring`, its mutex held by the caller), whose storage
// is the record block as it lies — the draws are composed into the sample order, which is then all that goes up.
static int train_on_records(kh_engine* e, const char* who, const kh_record* rec, kh_replay* ring, int n, const kh_train_config* cfg,
                            float* first_loss, float* last_loss)
{
    int rc;
    TrainCall call;
    if ((rc = train_begin(e, cfg, who, call))) return rc;
    TrainCache& tc = *call.tc;
    hipStream_t st = call.st;
    const int B = cfg->batch, epochs = cfg->epochs;
    const int per_epoch = (n + B - 1) / B;
    const size_t nsteps = (size_t)epochs * per_epoch, slot = kh::train_result_floats(B);      // floats of one step's dloss block

    // records and order through one page-locked block, one copy each; the order is kh_train's (kh_train_order)
    const RecordBlock lay(ring ? (size_t)ring->capacity : (size_t)n);
    const size_t rec_bytes = ring ? 0 : lay.bytes, order_bytes = (size_t)epochs * n * 4;
    if (tc.pin_rec.ensure(rec_bytes + order_bytes) || tc.rec.ensure(rec_bytes) || tc.order.ensure(order_bytes) ||
        tc.pin_loss.ensure(nsteps * slot * 4))
        return KH_ERR_HIP;
    if (rec) lay.pack(tc.pin_rec.at(0), rec, (size_t)n);
    int32_t* order = reinterpret_cast<int32_t*>(tc.pin_rec.at(rec_bytes));
    if ((rc = kh_train_order(n, epochs, order))) return rc;
    if (ring) {
        // sample k of the call is the record in slot draw[k], as kh_replay_select would have returned it
        std::vector<int32_t> draw((size_t)n);
        for (int k = 0; k < n; ++k) draw[(size_t)k] = (int32_t)(ring->rng() % (uint64_t)ring->capacity);
        for (size_t i = 0; i < (size_t)epochs * n; ++i) order[i] = draw[(size_t)order[i]];
    } else
        HIPCHK(hipMemcpyAsync(tc.rec.p, tc.pin_rec.p, lay.bytes, hipMemcpyHostToDevice, st));
    const char* block = ring ? ring->mem.as<char>() : tc.rec.as<char>();
    HIPCHK(hipMemcpyAsync(tc.order.p, order, order_bytes, hipMemcpyHostToDevice, st));
    // kh_train zeroes its staging rows at the start of every call and a short batch keeps the rows behind its own:
    // the device rows live in the cache across calls, so they start from zero here
    HIPCHK(hipMemsetAsync(tc.dx.p, 0, (size_t)B * XR_TILE * 4, st));
    HIPCHK(hipMemsetAsync(tc.dp.p, 0, (size_t)B * KH_PSIZE * 4, st));
    HIPCHK(hipMemsetAsync(tc.dv.p, 0, (size_t)B * 4, st));
    float* slots = reinterpret_cast<float*>(tc.pin_loss.p);
    call.t_setup = std::chrono::steady_clock::now();
    size_t step = 0;
    for (int epoch = 0; epoch < epochs; ++epoch)
        for (int base = 0; base < n; base += B, ++step) {
            launch_expand_records(block, lay, tc.order.as<int32_t>() + (size_t)epoch * n, base, std::min(B, n - base),
                                  tc.dx.as<float>(), tc.dp.as<float>(), tc.dv.as<float>(), st);
            HIPCHK(hipGetLastError());
            if ((rc = train_launch_step(call))) return rc;
            HIPCHK(hipMemcpyAsync(slots + step * slot, tc.dloss.p, slot * 4, hipMemcpyDeviceToHost, st));
        }
    HIPCHK(hipStreamSynchronize(st));                         // the one synchronisation of the call
    // kh_train's bookkeeping over the steps in order: the first failing step decides status and message (nothing is
    // installed before the end of the call, so running the later steps changed nothing that is kept)
    float firstloss = 0.0f, lastloss = 0.0f;
    step = 0;
    for (int epoch = 0; epoch < epochs; ++epoch) {
        float avgloss = 0.0f;
        for (int b = 0; b < per_epoch; ++b, ++step) {
            float loss;
            if ((rc = train_step_result(call, slots + step * slot, cfg->detect_anomaly != 0, epoch, b, &loss))) return rc;
            avgloss += loss;
        }
        avgloss /= (float)per_epoch;
        if (!epoch) firstloss = avgloss;
        lastloss = avgloss;
    }
    call.t_steps = std::chrono::steady_clock::now();
    if ((rc = train_finish(e, call, n, epochs))) return rc;
    if (first_loss) *first_loss = firstloss;
    if (last_loss) *last_loss = lastloss;
    return KH_OK;
}

extern "C" {

int kh_records_validate(const kh_record* rec, int n, int* bad_index)
{
    return records_check(rec, n, bad_index);
}

int kh_expand_records(kh_engine* e, const kh_record* rec, int n, float* planes, float* obs_p, float* obs_v)
{
    if (!e || !rec) return fail(KH_ERR_INVALID, "null argument");
    if (n < 0) return fail(KH_ERR_INVALID, "negative record count");
    int rc = check_records(e, "kh_expand_records");
    if (rc) return rc;
    if ((rc = records_check(rec, n, nullptr))) return rc;
    if (n == 0) return KH_OK;
    if ((rc = set_device(e))) return rc;
    SlotLease lease(e);
    Slot& s = *lease.s;
    if (!s.stream) HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    hipStream_t st = s.stream;
    const RecordBlock lay(EXPAND_CHUNK);
    if (s.hin.ensure(lay.bytes) || s.pack_in.ensure(lay.bytes) || s.planes.ensure((size_t)EXPAND_CHUNK * XR_TILE * 4) ||
        s.policy.ensure((size_t)EXPAND_CHUNK * KH_PSIZE * 4) || s.pack_out.ensure((size_t)EXPAND_CHUNK * 4))
        return KH_ERR_HIP;
    for (int base = 0; base < n; base += EXPAND_CHUNK) {
        const int m = std::min(EXPAND_CHUNK, n - base);
        lay.pack(s.hin.at(0), rec + base, (size_t)m);
        HIPCHK(hipMemcpyAsync(s.pack_in.p, s.hin.p, lay.bytes, hipMemcpyHostToDevice, st));
        launch_expand_records(s.pack_in.as<char>(), lay, nullptr, 0, m, s.planes.as<float>(), s.policy.as<float>(), s.pack_out.as<float>(), st);
        HIPCHK(hipGetLastError());
        if (planes) HIPCHK(hipMemcpyAsync(planes + (size_t)base * XR_TILE, s.planes.p, (size_t)m * XR_TILE * 4, hipMemcpyDeviceToHost, st));
        if (obs_p) HIPCHK(hipMemcpyAsync(obs_p + (size_t)base * KH_PSIZE, s.policy.p, (size_t)m * KH_PSIZE * 4, hipMemcpyDeviceToHost, st));
        if (obs_v) HIPCHK(hipMemcpyAsync(obs_v + base, s.pack_out.p, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));                    // the staging block is packed again for the next chunk
    }
    return KH_OK;
}

int kh_train_records(kh_engine* e, const kh_record* rec, int n, const kh_train_config* cfg, float* first_loss, float* last_loss)
{
    if (!e || !rec || !cfg) return fail(KH_ERR_INVALID, "null argument");
    if (n < 1 || cfg->batch < 2 || cfg->epochs < 1) return fail(KH_ERR_INVALID, "trajectories >= 1, batch >= 2, epochs >= 1 required");
    int rc = check_records(e, "kh_train_records");
    if (rc) return rc;
    if ((rc = kh_train_config_check(cfg))) return rc;
    if ((rc = records_check(rec, n, nullptr))) return rc;
    return train_on_records(e, "kh_train_records", rec, nullptr, n, cfg, first_loss, last_loss);
}

int kh_train_replay(kh_engine* e, kh_replay* r, int n, const kh_train_config* cfg, float* first_loss, float* last_loss)
{
    if (!e || !r || !cfg) return fail(KH_ERR_INVALID, "null argument");
    if (n < 1 || cfg->batch < 2 || cfg->epochs < 1) return fail(KH_ERR_INVALID, "trajectories >= 1, batch >= 2, epochs >= 1 required");
    int rc = check_records(e, "kh_train_replay");
    if (rc) return rc;
    if ((rc = kh_train_config_check(cfg))) return rc;
    if (r->device != e->cfg.device)
        return fail(KH_ERR_INVALID, "kh_train_replay: the ring is on device %d, the engine on device %d", r->device, e->cfg.device);
    std::lock_guard<std::mutex> ring(r->mu);                  // adds wait; taken before the engine's trainer lock (train_begin)
    return train_on_records(e, "kh_train_replay", nullptr, r, n, cfg, first_loss, last_loss);
}

}  // extern "C"
