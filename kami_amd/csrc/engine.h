// engine.h — the engine's host-side state and the declarations its translation units share: kh_api.hip (C ABI, slots,
// forward wrappers, host and device I/O, kh_train, checkpoints), weights.hip (parameter sets; weights_pack.hip: their device packer), queue.hip (the
// coalescing queue), train_ingest.hip (kh_train_records, kh_expand_records) and eval.hip (kh_eval_*).  Not part of the public boundary (that
// is include/kami_hip.h).
#pragma once
#include "kh_internal.h"
#include "train_opt.h"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace kh {

extern thread_local std::string g_err;   // what kh_last_error() returns: the calling thread's last failure

int fail(int code, const char* fmt, ...);

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return fail(KH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                        __FILE__, __LINE__);                                                 \
    } while (0)

struct DevMem {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevMem() { if (p) (void)hipFree(p); }
    int ensure(size_t n)
    {
        if (n <= bytes) return KH_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        HIPCHK(hipMalloc(&p, n));
        bytes = n;
        return KH_OK;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// page-locked host staging: one DMA per direction instead of one driver-staged copy per argument
struct PinMem {
    void* p = nullptr;
    size_t bytes = 0;
    ~PinMem() { if (p) (void)hipHostFree(p); }
    int ensure(size_t n, bool exact = false)
    {
        if (n <= bytes) return KH_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        if (!exact) n += n / 2;                  // action counts vary from call to call (exact: a blob's size does not)
        HIPCHK(hipHostMalloc(&p, n, hipHostMallocDefault));
        bytes = n;
        return KH_OK;
    }
    char* at(size_t off) const { return static_cast<char*>(p) + off; }
};

// One immutable, device-resident parameter set.  kh_load_weights builds a new one and swaps
// the engine's shared_ptr; calls in flight keep the old set alive until they finish.
struct Weights {
    int generation = 0;
    int64_t bn_batches = 0;              // BatchNorm num_batches_tracked of the reference (kh_bn_batches): carried, never computed with
    std::vector<float> blob;             // host copy (kh_clone)
    DevMem simple;                       // fp32 [tap][ci][co] + scale/shift per layer
    std::vector<kh::SimpleLayer> layers; // stem, 2R tower convs, policyconv, policyconv2, valueconv
    const float *fcw = nullptr, *fcb = nullptr;
    // whole-network MFMA kernel (tower8_mfma.hip): packed fragment stream + folded parameters
    DevMem tw_stream, tw_par, tw_fc4;
    int tw_nchunks = 0, tw_npar = 0, tw_FP = 0;
    bool tw_ok = false;
    std::string tw_why;
    // per-layer MFMA path for wide nets (layers_mfma.hip)
    DevMem ly_w, ly_shift, ly_misc;      // ly_misc: vw[CP], fcw[256*64], fcb[256], fc4[16][256][4]
    DevMem ly_w4;                        // 3x3 layers once more, packed for conv4_mfma_kernel
    DevMem ly_w2b;                       // stem + tower packed for tower256_kernel (256-channel blocks)
    bool ly_w2b_ok = false;
    DevMem ly_wh;                        // policyconv + policyconv2 packed for policy_head4_kernel
    bool ly_wh_ok = false;
    std::vector<size_t> ly_w_off, ly_shift_off, ly_w4_off;
    int ly_FP = 0, ly_CP = 0;
    float ly_vshift = 0.0f;
    bool ly_ok = false;
};

// ------------------------------------------------------------------------------- slots
// Per-call workspace: stream + device scratch.  kh_infer may be called concurrently from many
// host threads on one engine (nn.cpp:166 takes a shared lock); each call owns one slot.
struct Slot {
    hipStream_t stream = nullptr;
    int cap = 0;                 // boards the scratch is sized for
    DevMem in, x, t, u, ph, logits, policy, v64, vfull, flags, boards, planes, offs, acts, priors, actin, xchg;
    DevMem pack_in, pack_out;    // legal-move host path: arguments / results packed for one copy each way
    PinMem hin, hout;
    hipStream_t stream2 = nullptr;   // registered caller buffers: chunks alternate between the two streams
    bool busy = false;
    bool flags_clean = false;    // device NaN flags known to be zero
    // device-pointer API: the scratch above is shared by every caller stream, so a call on another stream
    // than the previous one first waits for that call's last kernel (event recorded behind it)
    hipEvent_t scratch_done = nullptr;
    hipStream_t scratch_stream = nullptr;
    bool scratch_pending = false;
};

struct Queue;           // the submit / wait queue (queue.hip)

// kh_eval_* (eval.hip): the serving forward's outputs for one chunk of KH_EVAL_CHUNK positions, the chunk's per-record
// results and the call's per-chunk sums; kh_eval_records' record block.  Used under the engine's dmu.
struct EvalCache {
    DevMem policy, vfull, rows, parts, flags, rec;
    PinMem pin_rec, pin_out;
};

// The trainer's workspace, shared by kh_train (kh_api.hip) and kh_train_records (train_ingest.hip): both write a batch
// into dx / dp / dv and run the same recorded step on it, so alternating them on one engine re-records nothing.
struct TrainCache {
    DevMem params, grads, work, dx, dp, dv, dloss;
    DevMem vel, norm_part, frozen;              // optimizer options only: the velocity (blob-shaped, zeroed per call), the norm's
                                                // partial sums, the running-statistics slots' ranges (uploaded once: one shape per engine)
    std::vector<float> last_norms;              // kh_train_grad_norms: the last completed call's norms before clipping
    DevMem rec, order;                          // kh_train_records: the call's records (RecordBlock layout) and sample order
    PinMem pin, pin_params;                     // batch staging; the parameter blob on its way up (a pageable source made the
                                                // upload take 0.1 ms or 10-27 ms from call to call: the runtime pins it on the fly)
    PinMem pin_rec, pin_loss;                   // kh_train_records: records + order on their way up; one dloss slot per step
    std::weak_ptr<Weights> on_device;           // the weights whose blob `params` holds right now (the previous call's result):
                                                // training them again needs no upload at all
    hipStream_t st = nullptr;
    hipGraph_t g = nullptr;
    hipGraphExec_t x = nullptr;
    int B = 0;
    StepOpt opt{};
    bool valu = false, graph_tried = false;
    void drop_graph()
    {
        if (x) (void)hipGraphExecDestroy(x);
        if (g) (void)hipGraphDestroy(g);
        x = nullptr; g = nullptr; graph_tried = false;
    }
    ~TrainCache()
    {
        drop_graph();
        if (st) (void)hipStreamDestroy(st);
    }
};

}  // namespace kh

struct kh_engine {
    kh_config cfg;
    int num_cus = 256;
    bool f32_simple = false;     // KAMI_F32_SIMPLE=1: dtype f32 always runs forward_simple.hip
    int small_max = 128;         // kh_infer up to this batch AND up to 768 KB of planes takes the zero-copy path
                                 // (KAMI_SMALL_MAX; 0: never): measured 1.6x per thread at batch 16, even at 2 MB of planes
    std::mutex wmu;
    std::shared_ptr<kh::Weights> weights;
    std::mutex smu;
    std::condition_variable scv;
    std::vector<std::unique_ptr<kh::Slot>> slots;
    std::unique_ptr<kh::Slot> devslot;           // scratch for the device-pointer API
    std::mutex dmu;
    kh::EvalCache eval;                          // kh_eval_*'s scratch (under dmu)
    kh::Queue* co = nullptr;          // submit / wait queue (created on first use)
    std::atomic<kh::Queue*> co_ready{ nullptr };     // the same pointer once the dispatcher runs: submitters skip co_mu
    std::atomic<bool> has_weights{ false };
    std::mutex co_mu;
    std::atomic<int> small_calls{ 0 };       // synchronous small-batch calls currently inside the engine
    std::atomic<int> co_target{ 0 }, co_wait_us{ 0 }, co_callers{ 0 };
    // kh_train's workspace, staging, stream and recorded step: kept from call to call (selfplay.cpp:266 trains again and
    // again with the same batch size and learning rate; allocating 0.1-2 GB and instantiating a ~270-node graph per
    // call cost more than a dozen SGD steps)
    std::mutex train_mu;
    kh::TrainCache* train = nullptr;
    // kh_load_weights_device: one install at a time; the stream it packs on when the caller names none, the stream and
    // page-locked block the blob's host copy comes down through, the event that orders that copy behind the caller's work
    std::mutex ld_mu;
    kh::PinMem ld_pin;
    hipStream_t ld_stream = nullptr, ld_copy = nullptr;
    hipEvent_t ld_ready = nullptr;
    // caller buffers registered with kh_pin_buffer: [base, base + bytes)
    std::mutex pin_mu;
    std::vector<std::pair<const char*, size_t>> pinned;
};

namespace kh {

// a call's lease on one of the engine's workspace slots (waits for a free one once MAX_SLOTS exist)
constexpr int MAX_SLOTS = 32;
struct SlotLease {
    kh_engine* e;
    Slot* s = nullptr;
    explicit SlotLease(kh_engine* e_) : e(e_)
    {
        std::unique_lock<std::mutex> lk(e->smu);
        for (;;) {
            for (auto& p : e->slots)
                if (!p->busy) { s = p.get(); break; }
            if (!s && (int)e->slots.size() < MAX_SLOTS) {
                e->slots.emplace_back(new Slot());
                s = e->slots.back().get();
            }
            if (s) { s->busy = true; return; }
            e->scv.wait(lk);
        }
    }
    ~SlotLease()
    {
        { std::lock_guard<std::mutex> lk(e->smu); s->busy = false; }
        e->scv.notify_one();
    }
};

// ---- kh_api.hip
int set_device(kh_engine* e);
int slot_ensure(kh_engine* e, Slot& s, int batch, bool host_io);
std::shared_ptr<Weights> current_weights(kh_engine* e);

// The forward pass on device buffers, launched on `st`.  lg: the whole-network kernel's legal-move mode (TowerArgs::lg_*).
struct LegalDev { const int32_t* offsets; const int32_t* actions; float* priors; float* values; int* flags; };
int forward_tower(kh_engine* e, const Weights& W, Slot& s, hipStream_t st, const float* d_in, int B,
                  float* d_policy, float* d_vfull, float* d_logits_out, const kh_board* d_boards = nullptr,
                  const LegalDev* lg = nullptr);
int forward_dispatch(kh_engine* e, const Weights& W, Slot& s, hipStream_t st, const float* d_in, int B,
                     float* d_policy, float* d_vfull, float* d_logits_out);
bool fused_ingest(const kh_engine* e, const Weights& W);
// kh_encode_infer_device behind its argument checks, e->dmu held by the caller: the serving forward on `batch` compact
// boards in device memory (fused ingest where the engine has it, the encode kernel into scratch otherwise).  *st_out: the
// stream it went to (`stream`, or the engine's own for nullptr)
int encode_infer_on_device(kh_engine* e, const Weights& W, const kh_board* d_boards, int batch, float* d_policy, float* d_vfull,
                           void* stream, hipStream_t* st_out);

// One host-buffer inference call (kh_infer*, the queue's synchronous kinds): planes [batch][8][8][F] or compact records
// in; the outputs the caller wants (null: not wanted), `value` by value_mode, `legal` the priors of the legal actions.
struct LegalIO { const int32_t* offsets; const int32_t* actions; float* priors; };
struct HostCall {
    const float* input = nullptr;
    const kh_board* boards = nullptr;
    int batch = 0;
    float *policy = nullptr, *value = nullptr, *value_full = nullptr, *logits = nullptr;
    const LegalIO* legal = nullptr;
};
int infer_host(kh_engine* e, const HostCall& c);

int nan_status(Slot& s, const int* flags);                  // KH_ERR_NAN_* for the NaN flags a forward left
int check_offsets(const int32_t* offsets, int batch);       // action_offsets start at 0 and never decrease
int check_records(const kh_engine* e, const char* who);     // compact records need features == 30

// ---- kh_api.hip: the parts of a training call that do not depend on where the batches come from
struct TrainCall {
    std::shared_ptr<Weights> W;                                  // the set being trained
    std::unique_ptr<TrainNet, void (*)(TrainNet*)> net{ nullptr, train_layout_free };
    std::unique_lock<std::mutex> lock;                           // e->train_mu, held until the call returns
    TrainCache* tc = nullptr;
    hipStream_t st = nullptr;
    size_t nfl = 0;
    int B = 0;
    StepOpt opt{};
    std::vector<float> norms;                                    // max_grad_norm > 0: every step's norm before clipping so far
    std::chrono::steady_clock::time_point t_call, t_bufs, t_up, t_setup, t_steps;   // KAMI_TRAIN_TRACE
};
// weights, lock, workspace (drops the recorded step when what it holds changed), stream, parameters on the device
int train_begin(kh_engine* e, const kh_train_config* cfg, const char* who, TrainCall& c);
// one SGD step on dx / dp / dv -> dloss: the recorded graph (recorded at the first step) or plain launches
int train_launch_step(TrainCall& c);
// nn.cpp:337-341 and the loss of one step from its dloss block (train_result_floats(B)), as kh_train reports them; with
// max_grad_norm > 0 the step's gradient norm joins c.norms, and a norm that is not finite fails like a NaN loss
int train_step_result(TrainCall& c, const float* loss_rows, bool detect_anomaly, int epoch, int batch, float* loss);
// parameters back, installed as generation + 1 with the BatchNorm counter advanced
int train_finish(kh_engine* e, TrainCall& c, int trajectories, int epochs);

// ---- train_ingest.hip: compact records (kh_record) as the trainer's input
// Records re-laid as arrays in one block, every array 16-byte aligned (sizeof(kh_record) is not a multiple of 16, and
// encode_square() fetches a kh_board with 16-byte loads): kh_board[n], value[n], nact[n], actions[n][96], visits[n][96].
struct RecordBlock {
    size_t boards, value, nact, actions, visits, bytes;          // byte offsets
    explicit RecordBlock(size_t n);
    void pack(char* dst, const kh_record* rec, size_t n) const;
};
// rows [0, count) of dx / dp / dv from records order[base + r] (order == nullptr: records base + r)
void launch_expand_records(const char* d_block, const RecordBlock& lay, const int32_t* d_order, int base, int count,
                           float* dx, float* dp, float* dv, hipStream_t s);
int records_check(const kh_record* rec, int n, int* bad_index);

// ---- weights.hip: builds a parameter set from the blob and makes it the engine's current one
int load_weights_impl(kh_engine* e, const float* blob, size_t nfloats, int generation, int64_t bn_batches,
                      std::shared_ptr<Weights>* installed);
// the same from a blob in device memory, packed by the kernels of weights_pack.hip on `stream` (nullptr: the engine's own)
// behind what the caller queued there; returns with the set complete.  pin: page-locked staging of at least the blob's
// size for its host copy (nullptr: the engine's own)
int load_weights_device_impl(kh_engine* e, const float* d_blob, size_t nfloats, int generation, int64_t bn_batches,
                             hipStream_t stream, PinMem* pin, std::shared_ptr<Weights>* installed);

// ---- queue.hip: the ABI's queue entry points
int co_submit(kh_engine* e, int kind, const kh_board* boards, const float* planes, int batch, const int32_t* offsets,
              const int32_t* actions, float* priors, float* value, float* policy, int64_t* ticket);
int co_wait(kh_engine* e, int64_t ticket);
int co_try_wait(kh_engine* e, int64_t ticket, int* done);
int co_set_coalesce(kh_engine* e, int target_batch, int max_wait_us);
int co_set_callers(kh_engine* e, int callers);
int co_stats(kh_engine* e, int64_t* launches, int64_t* rows);
int co_encode_infer_legal(kh_engine* e, const kh_board* boards, int batch, const int32_t* action_offsets,
                          const int32_t* actions, float* priors, float* value);
void co_destroy(kh_engine* e);

}  // namespace kh
