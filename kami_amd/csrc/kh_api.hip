// kh_api.hip — the C ABI of libkamihip.so (include/kami_hip.h): engine object, workspace slots, forward wrappers,
// host-buffer and device-buffer entry points, kh_train's host loop and checkpoints.  Parameter sets are built in
// weights.hip, the coalescing queue lives in queue.hip, training from compact records in train_ingest.hip (engine.h:
// what they share).
//
// Boundary being replaced: class kami::NN (kami/nn/nn.h:40-73, kami/nn/nn.cpp:107-222) and
// Env::observe (kami/env.h:202-262).  There is no CPU fallback anywhere in this library:
// without a gfx950 device kh_create fails with KH_ERR_NO_DEVICE.
#include "engine.h"
#include "blob_layout.h"
#include "torch_archive.h"
#include "torch_archive_write.h"

#include <sched.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

namespace kh {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int set_device(kh_engine* e) { HIPCHK(hipSetDevice(e->cfg.device)); return KH_OK; }

int slot_ensure(kh_engine* e, Slot& s, int batch, bool host_io)
{
    if (!s.stream) HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    if (batch <= s.cap) return KH_OK;
    const size_t B = batch, C = e->cfg.filters, F = e->cfg.features;
    int rc = 0;
    if (host_io) {
        rc |= s.in.ensure(B * 64 * F * 4);
        rc |= s.policy.ensure(B * KH_PSIZE * 4);
        rc |= s.vfull.ensure(B * KH_VALUE_WIDTH * 4);
        rc |= s.boards.ensure(B * sizeof(kh_board));
        rc |= s.planes.ensure(B * 64 * KH_NFEATURES * 4);
    }
    rc |= s.x.ensure(B * 64 * C * 4);
    rc |= s.t.ensure(B * 64 * C * 4);
    rc |= s.u.ensure(B * 64 * C * 4);
    rc |= s.ph.ensure(B * 64 * KH_POLICY_MID * 4);
    rc |= s.logits.ensure(B * KH_PSIZE * 4);
    rc |= s.v64.ensure(B * 64 * 4);
    rc |= s.flags.ensure(16);
    if (rc) return KH_ERR_HIP;
    s.cap = batch;
    return KH_OK;
}

std::shared_ptr<Weights> current_weights(kh_engine* e)
{
    std::lock_guard<std::mutex> lk(e->wmu);
    return e->weights;
}

// ------------------------------------------------------------------------------- completion steps
// NaN flags are only ever OR-ed by the kernels: cleared on demand, not per launch (a memset node costs a launch
// boundary); whoever reads a raised one marks the slot dirty (nan_status).  sync: launches on other streams read them too.
int clean_flags(Slot& s, hipStream_t st, bool sync = false)
{
    if (s.flags_clean) return KH_OK;
    HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
    if (sync) HIPCHK(hipStreamSynchronize(st));
    s.flags_clean = true;
    return KH_OK;
}

int nan_status(Slot& s, const int* fl)
{
    if (fl[0] | fl[1]) s.flags_clean = false;
    if (fl[0]) return fail(KH_ERR_NAN_POLICY, "inference policy output contains NaN");   // nn.cpp:176-177
    if (fl[1]) return fail(KH_ERR_NAN_VALUE, "inference value output contains NaN");     // nn.cpp:179-180
    return KH_OK;
}

// completion of work whose results the kernels write into page-locked memory themselves: polled, not waited for
int poll_stream(hipStream_t st)
{
    for (int k = 0;; ++k) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) return KH_OK;
        if (q != hipErrorNotReady) return fail(KH_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(q));
        if ((k & 15) == 15) sched_yield();
    }
}

// The value per position: nn.cpp:186 hands back the first `batch` floats of the flattened [batch,256] tensor, the fixed
// mode the value column.  As the row stride of a kernel that writes them ...
int value_stride(const kh_engine* e) { return e->cfg.value_mode == KH_VALUE_REFERENCE_FLAT ? 1 : KH_VALUE_WIDTH; }

// ... and as a download of the [B][256] tensor
int copy_values(const kh_engine* e, float* value, const float* d_vfull, size_t B, hipStream_t st)
{
    if (e->cfg.value_mode == KH_VALUE_REFERENCE_FLAT) HIPCHK(hipMemcpyAsync(value, d_vfull, B * 4, hipMemcpyDeviceToHost, st));
    else HIPCHK(hipMemcpy2DAsync(value, 4, d_vfull, KH_VALUE_WIDTH * 4, 4, B, hipMemcpyDeviceToHost, st));
    return KH_OK;
}

int check_offsets(const int32_t* offsets, int batch)
{
    if (offsets[0] != 0) return fail(KH_ERR_INVALID, "action_offsets[0] must be 0");
    for (int i = 0; i < batch; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(KH_ERR_INVALID, "action_offsets must be non-decreasing");
    return KH_OK;
}

// who: the entry point named in the message (null: the queue's)
int check_records(const kh_engine* e, const char* who)
{
    if (e->cfg.features == KH_NFEATURES) return KH_OK;
    if (!who) return fail(KH_ERR_INVALID, "compact records need features == %d", KH_NFEATURES);
    return fail(KH_ERR_INVALID, "%s needs features == %d (Env::observe planes)", who, KH_NFEATURES);
}

// The forward pass on device buffers: exact-order fp32 path (forward_simple.hip).
int forward_simple(kh_engine* e, const Weights& W, Slot& s, hipStream_t st, const float* d_in, int B,
                   float* d_policy, float* d_vfull, float* d_logits_out)
{
    const int R = e->cfg.residuals;
    float *x = s.x.as<float>(), *t = s.t.as<float>(), *u = s.u.as<float>();
    int* flags = s.flags.as<int>();
    HIPCHK(hipMemsetAsync(flags, 0, 16, st));
    size_t li = 0;
    kh::launch_simple_conv(W.layers[li++], d_in, nullptr, x, B, st);            // nn.cpp:62-65
    for (int r = 0; r < R; ++r) {                                              // nn.cpp:26-34
        kh::launch_simple_conv(W.layers[li++], x, nullptr, t, B, st);
        kh::launch_simple_conv(W.layers[li++], t, x, u, B, st);
        float* tmp = x; x = u; u = tmp;
    }
    float* logits = d_logits_out ? d_logits_out : s.logits.as<float>();
    kh::launch_simple_conv(W.layers[li++], x, nullptr, s.ph.as<float>(), B, st);       // nn.cpp:72-74
    kh::launch_simple_conv(W.layers[li++], s.ph.as<float>(), nullptr, logits, B, st);  // nn.cpp:75-79
    kh::launch_softmax4672(logits, d_policy, B, flags, st);                            // nn.cpp:80
    kh::launch_simple_conv(W.layers[li++], x, nullptr, s.v64.as<float>(), B, st);      // nn.cpp:83-85
    kh::launch_value_fc(s.v64.as<float>(), W.fcw, W.fcb, d_vfull, B, flags, st);        // nn.cpp:86-88
    HIPCHK(hipGetLastError());
    return KH_OK;
}

// The throughput path: one persistent kernel for the whole forward pass (tower_mfma.hip, tower8_mfma.hip).

// the kernel's arguments for B boards of fp32 planes at d_in; outputs, flags and legal-move mode are the caller's to set
static kh::TowerArgs tower_args(const kh_engine* e, const Weights& W, const float* d_in, int B)
{
    kh::TowerArgs a;
    a.in = d_in; a.boards = nullptr; a.B = B; a.F = e->cfg.features; a.R = e->cfg.residuals;
    a.wstream = W.tw_stream.as<char>(); a.nchunks = W.tw_nchunks;
    a.params = W.tw_par.as<float>(); a.npar = W.tw_npar;
    a.fcw4 = W.tw_fc4.as<float>(); a.fcb = W.tw_fc4.as<float>() + (size_t)KH_VALUE_WIDTH * 64;
    return a;
}

int forward_tower(kh_engine* e, const Weights& W, Slot& s, hipStream_t st, const float* d_in, int B,
                  float* d_policy, float* d_vfull, float* d_logits_out, const kh_board* d_boards, const LegalDev* lg)
{
    if (!W.tw_ok) return fail(KH_ERR_INVALID, "bf16/f16 path unavailable for this configuration: %s", W.tw_why.c_str());
    if (!d_boards && (reinterpret_cast<uintptr_t>(d_in) & 15)) return fail(KH_ERR_INVALID, "input planes must be 16-byte aligned");
    if (int rc = clean_flags(s, st)) return rc;
    int* flags = s.flags.as<int>();
    kh::TowerArgs a = tower_args(e, W, d_in, B);
    a.boards = d_boards;
    a.policy = d_policy; a.vfull = d_vfull; a.logits = d_logits_out; a.flags = flags;
    if (lg) { a.lg_offsets = lg->offsets; a.lg_actions = lg->actions; a.lg_priors = lg->priors; a.lg_values = lg->values; a.lg_flags = lg->flags; }
    HIPCHK(kh::launch_tower(e->cfg.dtype, W.tw_FP, a, e->num_cus, st));
    return KH_OK;
}

// Wide nets in bf16 / f16: one MFMA launch per layer (layers_mfma.hip), then the shared softmax / FC kernels.
int forward_layers(kh_engine* e, const Weights& W, Slot& s, hipStream_t st, const float* d_in, int B,
                   float* d_policy, float* d_vfull, float* d_logits_out)
{
    const size_t nb = B, eb = e->cfg.dtype == KH_F32 ? 4 : 2;
    int rc = 0;
    rc |= s.actin.ensure(nb * 64 * W.ly_FP * eb);
    rc |= s.x.ensure(nb * 64 * W.ly_CP * eb);
    rc |= s.t.ensure(nb * 64 * W.ly_CP * eb);
    rc |= s.u.ensure(nb * 64 * W.ly_CP * eb);
    rc |= s.ph.ensure(nb * 64 * KH_POLICY_MID * eb);
    rc |= s.logits.ensure(nb * KH_PSIZE * 4);
    rc |= s.v64.ensure(nb * 64 * 4);
    rc |= s.flags.ensure(16);
    if (rc) return KH_ERR_HIP;
    if ((rc = clean_flags(s, st))) return rc;
    int* flags = s.flags.as<int>();
    kh::LayersArgs L;
    L.in = d_in; L.B = B; L.F = e->cfg.features; L.FP = W.ly_FP; L.CP = W.ly_CP; L.R = e->cfg.residuals;
    L.act_in = s.actin.as<unsigned short>();
    L.act[0] = s.x.as<unsigned short>(); L.act[1] = s.t.as<unsigned short>(); L.act[2] = s.u.as<unsigned short>();
    L.pmid = s.ph.as<unsigned short>();
    L.logits = d_logits_out ? d_logits_out : s.logits.as<float>();
    L.v64 = s.v64.as<float>();
    L.w = W.ly_w.as<unsigned short>(); L.w_off = W.ly_w_off.data();
    L.w4 = W.ly_w4.as<unsigned short>(); L.w4_off = W.ly_w4_off.data();
    L.shift = W.ly_shift.as<float>(); L.shift_off = W.ly_shift_off.data();
    L.vw = W.ly_misc.as<float>(); L.vshift = W.ly_vshift;
    L.wh = W.ly_wh_ok ? W.ly_wh.as<unsigned short>() : nullptr;
    L.w2b = W.ly_w2b_ok ? W.ly_w2b.as<unsigned short>() : nullptr;
    L.policy = d_policy; L.flags = flags; L.want_logits = d_logits_out != nullptr;
    L.fcw = W.ly_misc.as<float>() + W.ly_CP; L.fcb = L.fcw + (size_t)KH_VALUE_WIDTH * 64; L.vfull = d_vfull;
    L.fc4 = L.fcb + KH_VALUE_WIDTH;
    L.num_cus = e->num_cus;
    if (W.ly_CP == 256 && W.ly_w2b_ok && e->cfg.dtype != KH_F32 && 16 * (((B + 1) / 2 + 7) / 8) <= e->num_cus) {
        // tower2s_kernel's exchange area (two workgroups per board pair at batches that leave half the chip idle)
        const int pairs_cap = e->num_cus / 2;
        if (s.xchg.ensure(kh::layers_xchg_bytes(pairs_cap)) == KH_OK) {
            L.xflag = s.xchg.as<unsigned>();
            L.xbuf = reinterpret_cast<unsigned short*>(static_cast<char*>(s.xchg.p) + kh::layers_xflag_bytes(pairs_cap));
            L.x_pairs = pairs_cap;
        }
    }
    HIPCHK(kh::launch_layers(e->cfg.dtype, L, st));              // tower, policy head + softmax (nn.cpp:72-80), value head (nn.cpp:83-88)
    HIPCHK(hipGetLastError());
    return KH_OK;
}

int forward_dispatch(kh_engine* e, const Weights& W, Slot& s, hipStream_t st, const float* d_in, int B,
                     float* d_policy, float* d_vfull, float* d_logits_out)
{
    switch (e->cfg.dtype) {
    case KH_F32:
        // exact-f32 MFMA path (layers_mfma.hip) when the shape is covered; plain VALU kernels otherwise
        // (KAMI_F32_SIMPLE=1 forces the latter: it is the order-exact anchor used by the tests)
        if (W.ly_ok && !e->f32_simple) return forward_layers(e, W, s, st, d_in, B, d_policy, d_vfull, d_logits_out);
        return forward_simple(e, W, s, st, d_in, B, d_policy, d_vfull, d_logits_out);
    case KH_BF16:
    case KH_F16:
        if (!W.tw_ok && W.ly_ok) return forward_layers(e, W, s, st, d_in, B, d_policy, d_vfull, d_logits_out);
        return forward_tower(e, W, s, st, d_in, B, d_policy, d_vfull, d_logits_out);
    default: return fail(KH_ERR_INVALID, "bad dtype %d", e->cfg.dtype);
    }
}

int check_cfg(const kh_config* c)
{
    if (!c) return fail(KH_ERR_INVALID, "null config");
    if (c->width != KH_WIDTH || c->height != KH_HEIGHT)
        return fail(KH_ERR_INVALID, "only 8x8 boards are supported (got %dx%d)", c->width, c->height);
    if (c->psize != KH_PSIZE) return fail(KH_ERR_INVALID, "psize must be %d", KH_PSIZE);
    if (c->features < 1 || c->features > 4096) return fail(KH_ERR_INVALID, "bad features %d", c->features);
    if (c->filters < 1 || c->filters > 1024) return fail(KH_ERR_INVALID, "bad filters %d", c->filters);
    if (c->residuals < 0 || c->residuals > 256) return fail(KH_ERR_INVALID, "bad residuals %d", c->residuals);
    if (c->dtype != KH_F32 && c->dtype != KH_BF16 && c->dtype != KH_F16)
        return fail(KH_ERR_INVALID, "bad dtype %d", c->dtype);
    if (c->value_mode != KH_VALUE_REFERENCE_FLAT && c->value_mode != KH_VALUE_PER_SAMPLE0)
        return fail(KH_ERR_INVALID, "bad value_mode %d", c->value_mode);
    return KH_OK;
}

// Env::observe can run inside the forward kernel: bf16 / f16 tower kernel with the encoder's 30 planes
bool fused_ingest(const kh_engine* e, const Weights& W)
{
    return e->cfg.dtype != KH_F32 && W.tw_ok && W.tw_FP == 32 && e->cfg.features == KH_NFEATURES;
}


bool is_pinned(kh_engine* e, const void* p, size_t bytes)
{
    std::lock_guard<std::mutex> lk(e->pin_mu);
    const char* c = static_cast<const char*>(p);
    for (auto& r : e->pinned)
        if (c >= r.first && c + bytes <= r.first + r.second) return true;
    return false;
}

// kh_infer with REGISTERED caller buffers (kh_pin_buffer) on the whole-network kernel: the copies are plain DMA out of /
// into the caller's pages, so the call is cut into four chunks that alternate between two streams — chunk k + 1's upload
// runs under chunk k's kernel and policy download.  PCIe is what bounds this ABI (30 464 B in, 18 692 B out per
// evaluation at 119 planes); pageable buffers cost the runtime a pin / unpin of the caller's pages per call on top.
int infer_host_pinned(kh_engine* e, const Weights& W, Slot& s, const float* input, int batch, float* policy, float* value)
{
    const size_t F = e->cfg.features;
    if (!s.stream2) HIPCHK(hipStreamCreateWithFlags(&s.stream2, hipStreamNonBlocking));
    hipStream_t st[2] = { s.stream, s.stream2 };
    if (int rc = clean_flags(s, st[0], true)) return rc;
    int* flags = s.flags.as<int>();
    const int NCK = batch >= 256 ? 4 : (batch >= 64 ? 2 : 1);
    const int per = ((batch + NCK - 1) / NCK + 1) & ~1;            // whole board pairs per chunk
    float* d_in = s.in.as<float>();
    float* d_pol = s.policy.as<float>();
    float* d_vf = s.vfull.as<float>();
    for (int k = 0, lo = 0; lo < batch; ++k, lo += per) {
        const int n = std::min(per, batch - lo);
        hipStream_t q = st[k & 1];
        HIPCHK(hipMemcpyAsync(d_in + (size_t)lo * 64 * F, input + (size_t)lo * 64 * F, (size_t)n * 64 * F * 4, hipMemcpyHostToDevice, q));
        kh::TowerArgs a = tower_args(e, W, d_in + (size_t)lo * 64 * F, n);
        a.policy = d_pol + (size_t)lo * KH_PSIZE; a.vfull = d_vf + (size_t)lo * KH_VALUE_WIDTH; a.logits = nullptr; a.flags = flags;
        HIPCHK(kh::launch_tower(e->cfg.dtype, W.tw_FP, a, e->num_cus, q));
        HIPCHK(hipMemcpyAsync(policy + (size_t)lo * KH_PSIZE, d_pol + (size_t)lo * KH_PSIZE, (size_t)n * KH_PSIZE * 4, hipMemcpyDeviceToHost, q));
    }
    HIPCHK(hipStreamSynchronize(st[1]));
    // the values and the NaN flags
    if (int rc = copy_values(e, value, d_vf, batch, st[0])) return rc;
    int fl[4] = { 0, 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(fl, flags, 16, hipMemcpyDeviceToHost, st[0]));
    HIPCHK(hipStreamSynchronize(st[0]));
    return nan_status(s, fl);
}

// kh_infer at SMALL batches (kami's default selfplay_batch is 16): a call is latency, not bandwidth — four runtime
// copies out of / into pageable memory and their synchronisation cost more than the kernel.  So: the planes are copied by
// the CPU into the slot's page-locked block, the kernel reads them from there and writes the policy rows into the
// page-locked output block ITSELF (as the queue's launches do with records and priors), a second tiny launch puts the
// values and NaN flags behind them, completion is polled, and the CPU copies the rows out.  No copy engine, one wait.
int infer_host_small(kh_engine* e, const Weights& W, Slot& s, const float* input, int batch, float* policy, float* value)
{
    const size_t B = batch, F = e->cfg.features;
    const size_t in_bytes = B * 64 * F * 4, pol_bytes = B * KH_PSIZE * 4;
    const size_t o_val = (pol_bytes + 15) & ~(size_t)15, o_flags = o_val + ((B * 4 + 15) & ~(size_t)15);
    if (s.hin.ensure(in_bytes) || s.hout.ensure(o_flags + 16)) return KH_ERR_HIP;
    memcpy(s.hin.p, input, in_bytes);
    hipStream_t st = s.stream;
    int rc = forward_tower(e, W, s, st, static_cast<const float*>(s.hin.p), batch, reinterpret_cast<float*>(s.hout.at(0)), s.vfull.as<float>(), nullptr);
    if (rc) return rc;
    int* fl = reinterpret_cast<int*>(s.hout.at(o_flags));
    kh::launch_gather_legal(nullptr, nullptr, nullptr, nullptr, batch, st, s.vfull.as<float>(), value_stride(e), reinterpret_cast<float*>(s.hout.at(o_val)),
                            s.flags.as<int>(), fl);
    HIPCHK(hipGetLastError());
    if ((rc = poll_stream(st))) return rc;
    memcpy(policy, s.hout.at(0), pol_bytes);                        // nn.cpp:173,185
    memcpy(value, s.hout.at(o_val), B * 4);
    return nan_status(s, fl);
}

// Planes or records onto the device (records: encoded there, or read by the whole-network kernel itself) and the forward
// pass.  d_boards: the records once on the device.
int forward_from_host(kh_engine* e, const Weights& W, Slot& s, const HostCall& c, const kh_board* d_boards, float* d_logits)
{
    hipStream_t st = s.stream;
    const bool fused = c.boards && fused_ingest(e, W) && !c.logits;
    const float* d_in;
    if (c.boards) {
        if (!fused) kh::launch_encode_f32(d_boards, c.batch, s.planes.as<float>(), st);
        d_in = s.planes.as<float>();
    } else {
        HIPCHK(hipMemcpyAsync(s.in.p, c.input, (size_t)c.batch * 64 * e->cfg.features * 4, hipMemcpyHostToDevice, st));   // nn.cpp:160
        d_in = s.in.as<float>();
    }
    if (fused) return forward_tower(e, W, s, st, nullptr, c.batch, s.policy.as<float>(), s.vfull.as<float>(), nullptr, d_boards);
    return forward_dispatch(e, W, s, st, d_in, c.batch, s.policy.as<float>(), s.vfull.as<float>(), d_logits);
}

// The search's call (records or planes in, legal priors + one value per position out): everything but the planes
// travels as ONE page-locked block per direction — records | offsets | actions in, priors | values | NaN flags out.
struct LegalBlocks {
    int nact;
    size_t in_offs, in_acts, in_total, out_values, out_flags, out_total;
};

int stage_legal(Slot& s, const HostCall& c, LegalBlocks& L)
{
    auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t B = c.batch;
    L.nact = c.legal->offsets[c.batch];
    L.in_offs = c.boards ? up16(B * sizeof(kh_board)) : 0; L.in_acts = L.in_offs + up16((B + 1) * 4);
    L.in_total = L.in_acts + up16((size_t)L.nact * 4);
    L.out_values = up16((size_t)L.nact * 4); L.out_flags = L.out_values + up16(B * 4); L.out_total = L.out_flags + 16;
    if (s.hin.ensure(L.in_total) || s.hout.ensure(L.out_total)) return KH_ERR_HIP;
    if (s.pack_in.ensure(s.hin.bytes) || s.pack_out.ensure(s.hout.bytes)) return KH_ERR_HIP;
    if (c.boards) memcpy(s.hin.at(0), c.boards, B * sizeof(kh_board));
    memcpy(s.hin.at(L.in_offs), c.legal->offsets, (B + 1) * 4);
    memcpy(s.hin.at(L.in_acts), c.legal->actions, (size_t)L.nact * 4);
    return KH_OK;
}

// ONE launch, no copy engine: the kernel reads records / offsets / actions from the page-locked block and writes the
// legal priors, the values (column 0) and the NaN flags into the other one itself (tower8_kernel's legal-move mode; what
// the queue's launches do); completion is polled
int infer_legal_one_launch(kh_engine* e, const Weights& W, Slot& s, const HostCall& c)
{
    LegalBlocks L;
    int rc = stage_legal(s, c, L);
    if (rc) return rc;
    int* fl = reinterpret_cast<int*>(s.hout.at(L.out_flags));
    fl[0] = fl[1] = 0;
    const LegalDev lg{ reinterpret_cast<const int32_t*>(s.hin.at(L.in_offs)), reinterpret_cast<const int32_t*>(s.hin.at(L.in_acts)),
                       reinterpret_cast<float*>(s.hout.at(0)), reinterpret_cast<float*>(s.hout.at(L.out_values)), fl };
    if ((rc = forward_tower(e, W, s, s.stream, nullptr, c.batch, s.policy.as<float>(), s.vfull.as<float>(), nullptr,
                            reinterpret_cast<const kh_board*>(s.hin.at(0)), &lg)))
        return rc;
    if ((rc = poll_stream(s.stream))) return rc;
    memcpy(c.legal->priors, s.hout.at(0), (size_t)L.nact * 4);
    memcpy(c.value, s.hout.at(L.out_values), (size_t)c.batch * 4);
    return nan_status(s, fl);
}

// the packed blocks up, the forward pass, the gather kernel writes priors / values / flags into one block, that block down
int infer_legal_packed(kh_engine* e, const Weights& W, Slot& s, const HostCall& c)
{
    LegalBlocks L;
    int rc = stage_legal(s, c, L);
    if (rc) return rc;
    hipStream_t st = s.stream;
    HIPCHK(hipMemcpyAsync(s.pack_in.p, s.hin.p, L.in_total, hipMemcpyHostToDevice, st));
    const char* pin = s.pack_in.as<char>();
    char* pout = s.pack_out.as<char>();
    if ((rc = forward_from_host(e, W, s, c, reinterpret_cast<const kh_board*>(pin), nullptr))) return rc;
    kh::launch_gather_legal(s.policy.as<float>(), reinterpret_cast<const int32_t*>(pin + L.in_offs),
                            reinterpret_cast<const int32_t*>(pin + L.in_acts), reinterpret_cast<float*>(pout), c.batch, st,
                            s.vfull.as<float>(), value_stride(e), reinterpret_cast<float*>(pout + L.out_values), s.flags.as<int>(),
                            reinterpret_cast<int*>(pout + L.out_flags));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.hout.p, s.pack_out.p, L.out_total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(c.legal->priors, s.hout.at(0), (size_t)L.nact * 4);
    memcpy(c.value, s.hout.at(L.out_values), (size_t)c.batch * 4);
    return nan_status(s, reinterpret_cast<const int*>(s.hout.at(L.out_flags)));
}

// one copy per argument and per output (nn.cpp:160-186): logits, the whole value tensor, plain legal priors
int infer_staged(kh_engine* e, const Weights& W, Slot& s, const HostCall& c)
{
    const size_t B = c.batch;
    hipStream_t st = s.stream;
    if (c.boards) HIPCHK(hipMemcpyAsync(s.boards.p, c.boards, B * sizeof(kh_board), hipMemcpyHostToDevice, st));
    int rc = forward_from_host(e, W, s, c, s.boards.as<kh_board>(), c.logits ? s.logits.as<float>() : nullptr);
    if (rc) return rc;
    const int nact = c.legal ? c.legal->offsets[c.batch] : 0;
    if (nact > 0) {
        if (s.offs.ensure((B + 1) * 4) || s.acts.ensure((size_t)nact * 4) || s.priors.ensure((size_t)nact * 4)) return KH_ERR_HIP;
        HIPCHK(hipMemcpyAsync(s.offs.p, c.legal->offsets, (B + 1) * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s.acts.p, c.legal->actions, (size_t)nact * 4, hipMemcpyHostToDevice, st));
        kh::launch_gather_legal(s.policy.as<float>(), s.offs.as<int32_t>(), s.acts.as<int32_t>(), s.priors.as<float>(), c.batch, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.legal->priors, s.priors.p, (size_t)nact * 4, hipMemcpyDeviceToHost, st));
    }
    if (c.policy) HIPCHK(hipMemcpyAsync(c.policy, s.policy.p, B * KH_PSIZE * 4, hipMemcpyDeviceToHost, st));  // nn.cpp:173,185
    if (c.logits) HIPCHK(hipMemcpyAsync(c.logits, s.logits.p, B * KH_PSIZE * 4, hipMemcpyDeviceToHost, st));
    if (c.value_full) HIPCHK(hipMemcpyAsync(c.value_full, s.vfull.p, B * KH_VALUE_WIDTH * 4, hipMemcpyDeviceToHost, st));
    if (c.value && (rc = copy_values(e, c.value, s.vfull.as<float>(), B, st))) return rc;
    int flags[4] = { 0, 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(flags, s.flags.p, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return nan_status(s, flags);
}

// kh_infer*'s ways between host buffers and the device, in order of precedence
enum class HostIo {
    Registered,        // planes in, policy rows + values out, registered caller buffers (infer_host_pinned)
    SmallZeroCopy,     // the same from pageable buffers at small batches (infer_host_small)
    LegalOneLaunch,    // records in, legal priors + per-sample values out, encoder fused into the kernel
    LegalPacked,       // legal priors + values out otherwise
    Staged,            // everything else
};

HostIo choose_io(kh_engine* e, const Weights& W, const HostCall& c)
{
    const size_t B = c.batch, in_bytes = B * 64 * e->cfg.features * 4;
    const bool rows = c.input && c.policy && c.value && !c.legal && !c.logits && !c.value_full && e->cfg.dtype != KH_F32 && W.tw_ok;
    if (rows && (reinterpret_cast<uintptr_t>(c.input) & 15) == 0 && is_pinned(e, c.input, in_bytes) && is_pinned(e, c.policy, B * KH_PSIZE * 4))
        return HostIo::Registered;
    if (rows && c.batch <= e->small_max && in_bytes <= 768 * 1024) return HostIo::SmallZeroCopy;
    if (!c.legal || !c.value || c.policy || c.logits || c.value_full) return HostIo::Staged;
    if (c.boards && fused_ingest(e, W) && e->cfg.value_mode == KH_VALUE_PER_SAMPLE0) return HostIo::LegalOneLaunch;
    return HostIo::LegalPacked;
}

int infer_host(kh_engine* e, const HostCall& c)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    if (c.batch < 1) return fail(KH_ERR_INVALID, "batch must be >= 1 (got %d)", c.batch);
    if ((!c.input && !c.boards) || (!c.policy && !c.legal)) return fail(KH_ERR_INVALID, "null buffer");
    if (c.legal) {
        if (!c.legal->offsets || !c.legal->actions || !c.legal->priors) return fail(KH_ERR_INVALID, "null legal-move buffer");
        if (int rc = check_offsets(c.legal->offsets, c.batch)) return rc;
    }
    std::shared_ptr<Weights> W = current_weights(e);
    if (!W) return fail(KH_ERR_NO_WEIGHTS, "kh_infer before kh_load_weights");
    int rc = set_device(e);
    if (rc) return rc;
    SlotLease lease(e);
    Slot& s = *lease.s;
    if ((rc = slot_ensure(e, s, c.batch, true))) return rc;
    switch (choose_io(e, *W, c)) {
    case HostIo::Registered: return infer_host_pinned(e, *W, s, c.input, c.batch, c.policy, c.value);
    case HostIo::SmallZeroCopy: return infer_host_small(e, *W, s, c.input, c.batch, c.policy, c.value);
    case HostIo::LegalOneLaunch: return infer_legal_one_launch(e, *W, s, c);
    case HostIo::LegalPacked: return infer_legal_packed(e, *W, s, c);
    case HostIo::Staged: break;
    }
    return infer_staged(e, *W, s, c);
}

// ------------------------------------------------------------------------------- training calls
int train_begin(kh_engine* e, const kh_train_config* cfg, const char* who, TrainCall& c)
{
    c.t_call = std::chrono::steady_clock::now();
    c.W = current_weights(e);
    if (!c.W) return fail(KH_ERR_NO_WEIGHTS, "%s before kh_load_weights", who);
    int rc = set_device(e);
    if (rc) return rc;
    const int F = e->cfg.features, C = e->cfg.filters, R = e->cfg.residuals, B = cfg->batch;
    c.net.reset(kh::train_layout_new(F, C, R));
    c.nfl = c.W->blob.size();
    c.B = B;
    c.opt = kh::StepOpt{ cfg->lr, cfg->momentum, cfg->weight_decay, cfg->max_grad_norm, cfg->nesterov };
    const size_t nfl = c.nfl;
    c.lock = std::unique_lock<std::mutex>(e->train_mu);       // one trainer per engine at a time (the reference: exclusive lock, nn.cpp:226)
    if (!e->train) e->train = new TrainCache();
    TrainCache& tc = *e->train;
    c.tc = &tc;
    DevMem &params = tc.params, &grads = tc.grads, &work = tc.work, &dx = tc.dx, &dp = tc.dp, &dv = tc.dv, &dloss = tc.dloss;
    const bool valu_now = getenv("KAMI_TRAIN_VALU") && atoi(getenv("KAMI_TRAIN_VALU")) != 0;
    {
        const void* before[6] = { params.p, work.p, dx.p, dloss.p, tc.vel.p, tc.norm_part.p };
        if ((rc = params.ensure(nfl * 4)) || (rc = grads.ensure(nfl * 4)) || (rc = work.ensure(kh::train_workspace_floats(F, C, R, B) * 4)) ||
            (rc = dx.ensure((size_t)B * 64 * F * 4)) || (rc = dp.ensure((size_t)B * KH_PSIZE * 4)) || (rc = dv.ensure((size_t)B * 4)) ||
            (rc = dloss.ensure(kh::train_result_floats(B) * 4)))
            return rc;
        if (!c.opt.plain()) {
            if ((c.opt.momentum != 0.0f && (rc = tc.vel.ensure(nfl * 4))) ||
                (c.opt.max_grad_norm > 0.0f && (rc = tc.norm_part.ensure(kh::train_norm_parts(nfl) * sizeof(double)))))
                return rc;
            if (!tc.frozen.p) {
                const long long* ranges = nullptr;
                const size_t nr = kh::train_frozen_ranges(*c.net, &ranges);
                if ((rc = tc.frozen.ensure(nr * 2 * sizeof(long long)))) return rc;
                HIPCHK(hipMemcpy(tc.frozen.p, ranges, nr * 2 * sizeof(long long), hipMemcpyHostToDevice));
            }
        }
        // the recorded step holds buffer addresses, the batch size, the update rule's values and the kernel choice
        if (before[0] != params.p || before[1] != work.p || before[2] != dx.p || before[3] != dloss.p || before[4] != tc.vel.p ||
            before[5] != tc.norm_part.p || tc.B != B || !(tc.opt == c.opt) || tc.valu != valu_now)
            tc.drop_graph();
        if (before[0] != params.p) tc.on_device.reset();
        tc.B = B; tc.opt = c.opt; tc.valu = valu_now;
    }
    c.t_bufs = std::chrono::steady_clock::now();
    if (!tc.st) HIPCHK(hipStreamCreateWithFlags(&tc.st, hipStreamNonBlocking));
    c.st = tc.st;
    if (tc.on_device.lock() != c.W) {
        // through a page-locked block of the trainer's own (the blob is a std::vector)
        if (tc.pin_params.ensure(nfl * 4)) return KH_ERR_HIP;
        memcpy(tc.pin_params.p, c.W->blob.data(), nfl * 4);
        HIPCHK(hipMemcpyAsync(params.p, tc.pin_params.p, nfl * 4, hipMemcpyHostToDevice, c.st));
    }                                            // else: `params` still holds exactly these weights — the previous call trained them
    tc.on_device.reset();                        // (until this call has installed its result, `params` belongs to nobody)
    if (c.opt.momentum != 0.0f) HIPCHK(hipMemsetAsync(tc.vel.p, 0, nfl * 4, c.st));      // the velocity lives for one call
    c.t_up = std::chrono::steady_clock::now();
    HIPCHK(kh::conv_f32_raw_prepare());          // function attributes are not stream work: set them before any capture
    return KH_OK;
}

static const bool train_trace = getenv("KAMI_TRAIN_TRACE") != nullptr;

// A step is ~120 small launches on fixed buffers: recorded once as a graph, replayed per batch (with the
// tiled conv kernels the host's launch work, not the GPU, bounded a step).  Falls back to plain launches.
int train_launch_step(TrainCall& c)
{
    TrainCache& tc = *c.tc;
    const int B = c.B;
    hipStream_t st = c.st;
    const kh::StepBuffers sb{ tc.params.as<float>(), tc.grads.as<float>(), tc.work.as<float>() };
    const kh::OptBuffers ob{ tc.vel.as<float>(), tc.norm_part.as<double>(), tc.frozen.as<long long>() };
    float *dx = tc.dx.as<float>(), *dp = tc.dp.as<float>(), *dv = tc.dv.as<float>(), *dloss = tc.dloss.as<float>();
    // all options zero: the reference's step, the launches every earlier version recorded
    auto step = [&] {
        return c.opt.plain() ? kh::train_step(*c.net, sb, dx, dp, dv, B, c.opt.lr, dloss, st)
                             : kh::train_step_opt(*c.net, sb, ob, dx, dp, dv, B, c.opt, dloss, st);
    };
    static const bool no_graph = getenv("KAMI_TRAIN_NOGRAPH") != nullptr;
    if (!tc.graph_tried && no_graph) tc.graph_tried = true;
    if (!tc.graph_tried) {
        tc.graph_tried = true;
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const hipError_t ce = step();
            const hipError_t ee = hipStreamEndCapture(st, &tc.g);
            if (ce != hipSuccess || ee != hipSuccess || hipGraphInstantiate(&tc.x, tc.g, nullptr, nullptr, 0) != hipSuccess) {
                if (tc.x) { (void)hipGraphExecDestroy(tc.x); tc.x = nullptr; }
                (void)hipGetLastError();
            }
            if (train_trace) fprintf(stderr, "[kami train] step recorded as a graph: %s\n", tc.x ? "yes" : "NO (plain launches)");
        }
    }
    if (tc.x) HIPCHK(hipGraphLaunch(tc.x, st));
    else HIPCHK(step());
    return KH_OK;
}

int train_step_result(TrainCall& c, const float* loss_rows, bool detect_anomaly, int epoch, int batch, float* loss_out)
{
    const int B = c.B;
    if (detect_anomaly) {                                 // nn.cpp:337-341: the value output first, then the policy
        const int* nf = reinterpret_cast<const int*>(loss_rows + 2 * B);
        if (nf[1]) return fail(KH_ERR_NAN_VALUE, "forward value output contains NaN");
        if (nf[0]) return fail(KH_ERR_NAN_POLICY, "forward policy output contains NaN");
    }
    float lp = 0.0f, lv = 0.0f;
    for (int b = 0; b < B; ++b) { lp += loss_rows[b]; lv += loss_rows[B + b]; }
    const float loss = lp + lv / (float)(B * KH_VALUE_WIDTH);
    if (loss != loss) return fail(KH_ERR_NAN_POLICY, "training loss is NaN (epoch %d, batch %d)", epoch, batch);
    if (c.opt.max_grad_norm > 0.0f) {
        const float norm = loss_rows[2 * B + 2];
        if (!std::isfinite(norm)) return fail(KH_ERR_NAN_POLICY, "training gradient norm is not finite (epoch %d, batch %d)", epoch, batch);
        c.norms.push_back(norm);
    }
    *loss_out = loss;
    return KH_OK;
}

int train_finish(kh_engine* e, TrainCall& c, int trajectories, int epochs)
{
    TrainCache& tc = *c.tc;
    const size_t nfl = c.nfl;
    // the serving layouts are packed on the device, straight from `params` on the trainer's stream; the blob's host copy
    // comes down through pin_params meanwhile ("parameters back" is part of "weights installed" since)
    const auto t_read = std::chrono::steady_clock::now();
    std::shared_ptr<Weights> installed;
    // every training-mode forward (one per batch, the short last one included: nn.cpp:264-301) counts once in each
    // BatchNorm's num_batches_tracked
    const int64_t forwards = (int64_t)epochs * ((trajectories + c.B - 1) / c.B);
    const int lrc = load_weights_device_impl(e, tc.params.as<float>(), nfl, c.W->generation + 1, c.W->bn_batches + forwards, c.st,
                                             &tc.pin_params, &installed);  // nn.cpp:371 ++generation
    if (lrc == KH_OK) { tc.on_device = installed; tc.last_norms = std::move(c.norms); }
    if (train_trace) {
        auto ms = [](std::chrono::steady_clock::duration d) { return std::chrono::duration<double, std::milli>(d).count(); };
        fprintf(stderr, "[kami train] call: set-up %.2f ms (buffers %.2f, parameters up %.2f, staging %.2f), steps %.2f ms, parameters back %.2f ms, "
                "weights installed %.2f ms\n", ms(c.t_setup - c.t_call), ms(c.t_bufs - c.t_call), ms(c.t_up - c.t_bufs), ms(c.t_setup - c.t_up),
                ms(c.t_steps - c.t_setup), ms(t_read - c.t_steps), ms(std::chrono::steady_clock::now() - t_read));
    }
    return lrc;
}

}  // namespace kh

using namespace kh;

// =============================================================================== C ABI
extern "C" {

const char* kh_last_error(void) { return g_err.c_str(); }
const char* kh_version(void) { return "kamihip 0.1 gfx950"; }

int kh_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

size_t kh_weight_count(int F, int C, int R)
{
    return kh_blob::total(kh_blob::layout(F, C, R));
}

int kh_create(const kh_config* cfg, kh_engine** out)
{
    if (!out) return fail(KH_ERR_INVALID, "null out");
    *out = nullptr;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(KH_ERR_NO_DEVICE, "no HIP device visible; this engine has no CPU path");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(KH_ERR_INVALID, "device %d out of range (%d visible)", cfg->device, ndev);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(KH_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only",
                    cfg->device, prop.gcnArchName);
    kh_engine* e = new kh_engine();
    e->cfg = *cfg;
    e->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    e->f32_simple = getenv("KAMI_F32_SIMPLE") && atoi(getenv("KAMI_F32_SIMPLE")) != 0;
    if (getenv("KAMI_SMALL_MAX")) e->small_max = std::max(0, atoi(getenv("KAMI_SMALL_MAX")));
    *out = e;
    return KH_OK;
}

void kh_destroy(kh_engine* e)
{
    if (!e) return;
    co_destroy(e);
    (void)hipSetDevice(e->cfg.device);
    auto kill = [](Slot* s) {
        if (s && s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
        if (s && s->stream2) { (void)hipStreamSynchronize(s->stream2); (void)hipStreamDestroy(s->stream2); }
        if (s && s->scratch_done) (void)hipEventDestroy(s->scratch_done);
    };
    for (auto& s : e->slots) kill(s.get());
    kill(e->devslot.get());
    if (e->ld_stream) (void)hipStreamDestroy(e->ld_stream);
    if (e->ld_copy) (void)hipStreamDestroy(e->ld_copy);
    if (e->ld_ready) (void)hipEventDestroy(e->ld_ready);
    for (auto& r : e->pinned) (void)hipHostUnregister(const_cast<char*>(r.first));
    delete e->train;
    delete e;
}

int kh_load_weights(kh_engine* e, const float* blob, size_t nfloats, int generation)
{
    return load_weights_impl(e, blob, nfloats, generation, 0, nullptr);
}

int kh_load_weights_device(kh_engine* e, const float* d_blob, size_t nfloats, int generation, void* stream)
{
    return load_weights_device_impl(e, d_blob, nfloats, generation, 0, static_cast<hipStream_t>(stream), nullptr, nullptr);
}

int kh_train(kh_engine* e, const float* inputs, const float* obs_p, const float* obs_v, int trajectories,
             const kh_train_config* cfg, float* first_loss, float* last_loss)
{
    if (!e || !inputs || !obs_p || !obs_v || !cfg) return fail(KH_ERR_INVALID, "null argument");
    if (trajectories < 1 || cfg->batch < 2 || cfg->epochs < 1) return fail(KH_ERR_INVALID, "trajectories >= 1, batch >= 2, epochs >= 1 required");
    int rc = kh_train_config_check(cfg);
    if (rc) return rc;
    TrainCall call;
    if ((rc = train_begin(e, cfg, "kh_train", call))) return rc;
    TrainCache& tc = *call.tc;
    DevMem &dx = tc.dx, &dp = tc.dp, &dv = tc.dv, &dloss = tc.dloss;
    hipStream_t st = call.st;
    const int F = e->cfg.features, B = cfg->batch;

    // nn.cpp:245-262: one engine for the whole call, one shuffle per epoch; staging rows persist
    std::vector<int> picker((size_t)trajectories);
    for (int i = 0; i < trajectories; ++i) picker[i] = i;
    auto rng = std::default_random_engine{};
    const size_t in_row = (size_t)64 * F;
    // batch staging in page-locked memory (rows persist from batch to batch like the reference's stack buffers)
    PinMem& pin = tc.pin;
    const size_t n_in = (size_t)B * in_row, n_p = (size_t)B * KH_PSIZE;
    const size_t n_res = kh::train_result_floats(B);
    if (pin.ensure((n_in + n_p + (size_t)B + n_res) * 4)) return KH_ERR_HIP;
    float* next_input = reinterpret_cast<float*>(pin.p);
    float* next_policy = next_input + n_in;
    float* next_value = next_policy + n_p;
    float* loss_rows = next_value + B;
    memset(pin.p, 0, (n_in + n_p + (size_t)B + n_res) * 4);
    float firstloss = 0.0f, lastloss = 0.0f;
    call.t_setup = std::chrono::steady_clock::now();
    for (int epoch = 0; epoch < cfg->epochs; ++epoch) {
        std::shuffle(picker.begin(), picker.end(), rng);
        float avgloss = 0.0f;
        int nbatches = 0;
        for (int base = 0; base <= trajectories - 1;) {
            int i = 0;
            for (; i < B && i + base <= trajectories - 1; ++i) {
                const size_t src = (size_t)picker[base + i];
                memcpy(&next_input[(size_t)i * in_row], inputs + src * in_row, in_row * 4);
                memcpy(&next_policy[(size_t)i * KH_PSIZE], obs_p + src * KH_PSIZE, (size_t)KH_PSIZE * 4);
                next_value[i] = obs_v[src];
            }
            base += i;
            if (cfg->detect_anomaly) {                        // nn.cpp:329-333: isnan on the batch as it goes to the device
                for (size_t k = 0; k < n_in; ++k)
                    if (next_input[k] != next_input[k]) return fail(KH_ERR_INVALID, "training input ind %d contains NaN", nbatches);
            }
            HIPCHK(hipMemcpyAsync(dx.p, next_input, n_in * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(dp.p, next_policy, n_p * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(dv.p, next_value, (size_t)B * 4, hipMemcpyHostToDevice, st));
            if ((rc = train_launch_step(call))) return rc;
            HIPCHK(hipMemcpyAsync(loss_rows, dloss.p, n_res * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            float loss;
            if ((rc = train_step_result(call, loss_rows, cfg->detect_anomaly != 0, epoch, nbatches, &loss))) return rc;
            avgloss += loss;
            ++nbatches;
        }
        avgloss /= (float)nbatches;
        if (!epoch) firstloss = avgloss;
        lastloss = avgloss;
    }
    call.t_steps = std::chrono::steady_clock::now();
    if ((rc = train_finish(e, call, trajectories, cfg->epochs))) return rc;
    if (first_loss) *first_loss = firstloss;
    if (last_loss) *last_loss = lastloss;
    return KH_OK;
}

int kh_train_config_check(const kh_train_config* cfg)
{
    if (!cfg) return fail(KH_ERR_INVALID, "null kh_train_config");
    if (cfg->batch < 2) return fail(KH_ERR_INVALID, "batch %d: batch >= 2 required", (int)cfg->batch);
    if (cfg->epochs < 1) return fail(KH_ERR_INVALID, "epochs %d: epochs >= 1 required", (int)cfg->epochs);
    const struct { const char* name; float v; } reals[3] = { { "momentum", cfg->momentum }, { "weight_decay", cfg->weight_decay },
                                                             { "max_grad_norm", cfg->max_grad_norm } };
    for (const auto& r : reals) {
        if (!std::isfinite(r.v)) return fail(KH_ERR_INVALID, "%s is not finite", r.name);
        if (r.v < 0.0f) return fail(KH_ERR_INVALID, "%s %g: must not be negative", r.name, (double)r.v);
    }
    if (cfg->momentum >= 1.0f) return fail(KH_ERR_INVALID, "momentum %g outside [0, 1)", (double)cfg->momentum);
    if (cfg->nesterov != 0 && cfg->nesterov != 1) return fail(KH_ERR_INVALID, "nesterov %d: 0 or 1 required", (int)cfg->nesterov);
    if (cfg->nesterov && cfg->momentum == 0.0f) return fail(KH_ERR_INVALID, "nesterov requires momentum > 0");
    return KH_OK;
}

int kh_train_grad_norms(kh_engine* e, float* norms, int cap, int* steps)
{
    if (!e || !steps || cap < 0 || (cap > 0 && !norms)) return fail(KH_ERR_INVALID, "kh_train_grad_norms: an engine, steps and a buffer for cap norms required");
    std::lock_guard<std::mutex> lk(e->train_mu);
    const std::vector<float> none;
    const std::vector<float>& v = e->train ? e->train->last_norms : none;
    *steps = (int)v.size();
    for (int i = 0; i < cap && i < (int)v.size(); ++i) norms[i] = v[i];
    return KH_OK;
}

int kh_train_order(int trajectories, int epochs, int32_t* order)
{
    if (trajectories < 1 || epochs < 1 || !order) return fail(KH_ERR_INVALID, "trajectories >= 1, epochs >= 1 and a buffer required");
    std::vector<int> picker((size_t)trajectories);
    for (int i = 0; i < trajectories; ++i) picker[i] = i;
    auto rng = std::default_random_engine{};                  // exactly kh_train's
    for (int epoch = 0; epoch < epochs; ++epoch) {
        std::shuffle(picker.begin(), picker.end(), rng);
        for (int i = 0; i < trajectories; ++i) order[(size_t)epoch * trajectories + i] = picker[i];
    }
    return KH_OK;
}

int kh_train_conv_plan(int batch, int ci, int co, int* two_board_kernel, int* wgrad_ranges, int* boards_per_range)
{
    if (batch < 1 || ci < 1 || co < 1) return fail(KH_ERR_INVALID, "kh_train_conv_plan: batch, ci and co >= 1 required");
    const int ranges = kh::train_wgrad_splits(batch, ci, co);
    if (two_board_kernel) *two_board_kernel = kh::conv_f32_raw_two_board(batch, co) ? 1 : 0;
    if (wgrad_ranges) *wgrad_ranges = ranges;
    if (boards_per_range) *boards_per_range = (batch + ranges - 1) / ranges;
    return KH_OK;
}

int kh_checkpoint_read(const char* path, int* features, int* filters, int* residuals, int* generation,
                       float* blob, size_t cap, size_t* nfloats)
{
    return kh_checkpoint_read_ex(path, features, filters, residuals, generation, nullptr, blob, cap, nfloats);
}

// what a checkpoint file holds: a KAMW blob or the reference's libtorch archive, read and checked in one pass
struct CheckpointData {
    int F = 0, C = 0, R = 0, gen = 0;
    int64_t nbt = 0;                     // KAMW carries no counter
    std::vector<float> data;
};

static int read_checkpoint(const char* path, CheckpointData& out)
{
    if (!path) return fail(KH_ERR_INVALID, "null path");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(KH_ERR_INVALID, "cannot open %s", path);
    int32_t hdr[8] = { 0 };
    const size_t got = fread(hdr, 1, sizeof hdr, f);
    int &F = out.F, &C = out.C, &R = out.R, &gen = out.gen;
    int64_t& nbt = out.nbt;
    std::vector<float>& data = out.data;
    if (got == sizeof hdr && hdr[0] == 0x574d414b /* "KAMW" */) {
        F = hdr[1]; C = hdr[2]; R = hdr[3]; gen = hdr[4];
        if (F < 1 || F > 4096 || C < 1 || C > 1024 || R < 0 || R > 256) { fclose(f); return fail(KH_ERR_INVALID, "%s: bad header", path); }
        // the header's numbers come from the file: size the buffer only once the file is known to hold that many floats
        const size_t need = kh_weight_count(F, C, R);
        fseek(f, 0, SEEK_END);
        const long fsz = ftell(f);
        fseek(f, (long)sizeof hdr, SEEK_SET);
        if (fsz < 0 || ((size_t)fsz - sizeof hdr) / 4 < need) { fclose(f); return fail(KH_ERR_INVALID, "%s: truncated", path); }
        data.resize(need);
        const size_t n = fread(data.data(), 4, data.size(), f);
        fclose(f);
        if (n != data.size()) return fail(KH_ERR_INVALID, "%s: truncated", path);
    } else {
        fclose(f);
        if (got < 4 || memcmp(hdr, "PK\003\004", 4) != 0)
            return fail(KH_ERR_INVALID, "%s is neither a libtorch archive nor an engine weight blob", path);
        try {
            kh_archive::Checkpoint ck = kh_archive::read_checkpoint(path);
            auto w = ck.tensors.find("conv1.weight");
            auto g = ck.ints.find("generation");
            if (w == ck.tensors.end() || w->second.shape.size() != 4 || g == ck.ints.end())
                return fail(KH_ERR_INVALID, "%s: not a kami checkpoint (no conv1.weight / generation)", path);
            // the same bounds as the KAMW path, on numbers that come from the file; every tensor below must have EXACTLY
            // the shape libtorch gives it (nn.cpp:20-23,45-56) — an element count alone would take a transposed tensor
            const int64_t c64 = w->second.shape[0], f64 = w->second.shape[1];
            if (f64 < 1 || f64 > 4096 || c64 < 1 || c64 > 1024) return fail(KH_ERR_INVALID, "%s: conv1.weight has an impossible shape", path);
            if (g->second < INT32_MIN || g->second > INT32_MAX) return fail(KH_ERR_INVALID, "%s: generation out of range", path);
            C = (int)c64; F = (int)f64; gen = (int)g->second;
            nbt = ck.bn_batches;
            while (R <= 256 && ck.tensors.count("residual" + std::to_string(R) + ".conv1.weight")) ++R;
            if (R > 256) return fail(KH_ERR_INVALID, "%s: more than 256 residual blocks", path);
            const std::vector<kh_blob::Tensor> order = kh_blob::layout(F, C, R);
            if (order.size() != ck.tensors.size())
                return fail(KH_ERR_INVALID, "%s: %zu tensors, this network has %zu", path, ck.tensors.size(), order.size());
            for (auto& o : order) {
                auto t = ck.tensors.find(o.name);
                if (t == ck.tensors.end() || t->second.shape != o.shape)
                    return fail(KH_ERR_INVALID, "%s: tensor %s missing or of the wrong shape", path, o.name.c_str());
                data.insert(data.end(), t->second.data.begin(), t->second.data.end());
            }
        } catch (const std::exception& ex) {
            return fail(KH_ERR_INVALID, "%s: %s", path, ex.what());
        }
    }
    return KH_OK;
}

int kh_checkpoint_read_ex(const char* path, int* features, int* filters, int* residuals, int* generation, int64_t* bn_batches,
                          float* blob, size_t cap, size_t* nfloats)
{
    CheckpointData ck;
    if (int rc = read_checkpoint(path, ck)) return rc;
    if (features) *features = ck.F;
    if (filters) *filters = ck.C;
    if (residuals) *residuals = ck.R;
    if (generation) *generation = ck.gen;
    if (bn_batches) *bn_batches = ck.nbt;
    if (nfloats) *nfloats = ck.data.size();
    if (blob) {
        if (cap < ck.data.size()) return fail(KH_ERR_INVALID, "blob buffer holds %zu floats, the checkpoint has %zu", cap, ck.data.size());
        memcpy(blob, ck.data.data(), ck.data.size() * sizeof(float));
    }
    return KH_OK;
}

int kh_load_checkpoint(kh_engine* e, const char* path)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    CheckpointData ck;
    if (int rc = read_checkpoint(path, ck)) return rc;
    if (ck.F != e->cfg.features || ck.C != e->cfg.filters || ck.R != e->cfg.residuals)
        return fail(KH_ERR_INVALID, "%s holds a %d-plane %dx%d network, this engine is %d-plane %dx%d", path, ck.F, ck.R, ck.C,
                    e->cfg.features, e->cfg.residuals, e->cfg.filters);
    return load_weights_impl(e, ck.data.data(), ck.data.size(), ck.gen, ck.nbt, nullptr);
}


int kh_checkpoint_write(const char* path, int features, int filters, int residuals, int generation, int64_t bn_batches,
                        const float* blob, size_t nfloats)
{
    if (!path || !blob) return fail(KH_ERR_INVALID, "null argument");
    if (features < 1 || features > 4096 || filters < 1 || filters > 1024 || residuals < 0 || residuals > 256)
        return fail(KH_ERR_INVALID, "impossible network shape F=%d C=%d R=%d", features, filters, residuals);
    if (nfloats != kh_weight_count(features, filters, residuals))
        return fail(KH_ERR_INVALID, "weight blob has %zu floats, expected %zu for F=%d C=%d R=%d", nfloats,
                    kh_weight_count(features, filters, residuals), features, filters, residuals);
    if (bn_batches < 0) return fail(KH_ERR_INVALID, "negative BatchNorm batch count");
    try {
        kh_archive::write_checkpoint(path, residuals, generation, bn_batches, blob, kh_blob::layout(features, filters, residuals));
    } catch (const std::exception& ex) {
        return fail(KH_ERR_INVALID, "%s: %s", path, ex.what());
    }
    return KH_OK;
}

int kh_write_checkpoint(kh_engine* e, const char* path)
{
    if (!e || !path) return fail(KH_ERR_INVALID, "null argument");
    auto W = current_weights(e);                 // one parameter set: blob, generation and counter belong together
    if (!W) return fail(KH_ERR_NO_WEIGHTS, "no weights loaded");
    return kh_checkpoint_write(path, e->cfg.features, e->cfg.filters, e->cfg.residuals, W->generation, W->bn_batches,
                               W->blob.data(), W->blob.size());
}

int kh_get_weights(kh_engine* e, float* blob, size_t nfloats)
{
    if (!e || !blob) return fail(KH_ERR_INVALID, "null argument");
    auto W = current_weights(e);
    if (!W) return fail(KH_ERR_NO_WEIGHTS, "no weights loaded");
    if (nfloats != W->blob.size()) return fail(KH_ERR_INVALID, "blob has %zu floats, caller asked for %zu", W->blob.size(), nfloats);
    memcpy(blob, W->blob.data(), nfloats * sizeof(float));
    return KH_OK;
}

int kh_generation(kh_engine* e)
{
    if (!e) return -1;
    auto W = current_weights(e);
    return W ? W->generation : 0;
}

int kh_bn_batches(kh_engine* e, int64_t* count)
{
    if (!e || !count) return fail(KH_ERR_INVALID, "null argument");
    auto W = current_weights(e);
    *count = W ? W->bn_batches : 0;
    return KH_OK;
}

int kh_clone(kh_engine* src, kh_engine** out)
{
    if (!src || !out) return fail(KH_ERR_INVALID, "null argument");
    int rc = kh_create(&src->cfg, out);
    if (rc) return rc;
    auto W = current_weights(src);
    if (W && (rc = load_weights_impl(*out, W->blob.data(), W->blob.size(), W->generation, W->bn_batches, nullptr))) {
        kh_destroy(*out);
        *out = nullptr;
        return rc;
    }
    return KH_OK;
}

int kh_infer(kh_engine* e, const float* input, int batch, float* policy, float* value)
{
    if (!value) return fail(KH_ERR_INVALID, "null value buffer");
    // always the caller's private slot: a plane / full-policy call is 26-49 KB per position of PCIe traffic, which
    // concurrent callers' own streams overlap better than one merged launch does (measured: 4 threads x 16 positions
    // 0.44 M/s on private slots, 0.17 M/s merged) — kh_submit_infer stays for callers that want the queue anyway
    return infer_host(e, { .input = input, .batch = batch, .policy = policy, .value = value });
}

int kh_submit_infer(kh_engine* e, const float* input, int batch, float* policy, float* value, int64_t* ticket)
{
    return co_submit(e, 1, nullptr, input, batch, nullptr, nullptr, nullptr, value, policy, ticket);
}

int kh_submit_encode_infer_legal(kh_engine* e, const kh_board* boards, int batch, const int32_t* action_offsets,
                                 const int32_t* actions, float* priors, float* value, int64_t* ticket)
{
    return co_submit(e, 0, boards, nullptr, batch, action_offsets, actions, priors, value, nullptr, ticket);
}

int kh_wait(kh_engine* e, int64_t ticket) { return co_wait(e, ticket); }
int kh_try_wait(kh_engine* e, int64_t ticket, int* done) { return co_try_wait(e, ticket, done); }
int kh_set_coalesce(kh_engine* e, int target_batch, int max_wait_us) { return co_set_coalesce(e, target_batch, max_wait_us); }
int kh_set_coalesce_callers(kh_engine* e, int callers) { return co_set_callers(e, callers); }
int kh_coalesce_stats(kh_engine* e, int64_t* launches, int64_t* rows) { return co_stats(e, launches, rows); }

int kh_infer_full(kh_engine* e, const float* input, int batch, float* policy, float* value_full,
                  float* logits)
{
    return infer_host(e, { .input = input, .batch = batch, .policy = policy, .value_full = value_full, .logits = logits });
}

int kh_encode_infer(kh_engine* e, const kh_board* boards, int batch, float* policy, float* value)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    if (int rc = check_records(e, "kh_encode_infer")) return rc;
    if (!value || !boards) return fail(KH_ERR_INVALID, "null buffer");
    return infer_host(e, { .boards = boards, .batch = batch, .policy = policy, .value = value });
}

int kh_infer_legal(kh_engine* e, const float* input, int batch, const int32_t* action_offsets,
                   const int32_t* actions, float* priors, float* value)
{
    if (!value || !input) return fail(KH_ERR_INVALID, "null buffer");
    LegalIO l{ action_offsets, actions, priors };
    return infer_host(e, { .input = input, .batch = batch, .value = value, .legal = &l });
}

int kh_encode_infer_legal(kh_engine* e, const kh_board* boards, int batch, const int32_t* action_offsets,
                          const int32_t* actions, float* priors, float* value)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    if (int rc = check_records(e, "kh_encode_infer_legal")) return rc;
    if (!value || !boards) return fail(KH_ERR_INVALID, "null buffer");
    return co_encode_infer_legal(e, boards, batch, action_offsets, actions, priors, value);
}

int kh_encode(kh_engine* e, const kh_board* boards, int batch, float* planes)
{
    if (!e || !boards || !planes) return fail(KH_ERR_INVALID, "null argument");
    if (batch < 0) return fail(KH_ERR_INVALID, "negative batch");
    if (batch == 0) return KH_OK;
    int rc = set_device(e);
    if (rc) return rc;
    SlotLease lease(e);
    Slot& s = *lease.s;
    if (!s.stream) HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    const size_t B = batch;
    if (s.boards.ensure(B * sizeof(kh_board)) || s.planes.ensure(B * 64 * KH_NFEATURES * 4)) return KH_ERR_HIP;
    HIPCHK(hipMemcpyAsync(s.boards.p, boards, B * sizeof(kh_board), hipMemcpyHostToDevice, s.stream));
    kh::launch_encode_f32(s.boards.as<kh_board>(), batch, s.planes.as<float>(), s.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(planes, s.planes.p, B * 64 * KH_NFEATURES * 4, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    return KH_OK;
}

// st: the stream the call runs on (the caller's when given)
static int dev_slot(kh_engine* e, int batch, void* stream, Slot** out, hipStream_t* st_out)
{
    if (!e->devslot) e->devslot.reset(new Slot());
    Slot& s = *e->devslot;
    int rc = slot_ensure(e, s, batch, false);
    if (rc) return rc;
    *out = &s;
    // per-layer paths keep activations in the slot's scratch: order this call behind the previous one when it
    // runs on a different stream (same stream: stream order already does it)
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : s.stream;
    if (s.scratch_pending && s.scratch_stream != st) HIPCHK(hipStreamWaitEvent(st, s.scratch_done, 0));
    *st_out = st;
    return KH_OK;
}

// after a device-API forward: remember where the scratch was last used (only the per-layer paths use it; the
// whole-network kernel keeps its activations in LDS)
static int dev_slot_done(kh_engine* e, const Weights& W, Slot& s, hipStream_t st)
{
    const bool uses_scratch = e->cfg.dtype == KH_F32 || !W.tw_ok;
    if (!uses_scratch) return KH_OK;
    if (!s.scratch_done) HIPCHK(hipEventCreateWithFlags(&s.scratch_done, hipEventDisableTiming));
    HIPCHK(hipEventRecord(s.scratch_done, st));
    s.scratch_stream = st;
    s.scratch_pending = true;
    return KH_OK;
}

int kh_infer_device(kh_engine* e, const void* d_input, int batch, float* d_policy,
                    float* d_value_full, void* stream)
{
    if (!e || !d_input || !d_policy || !d_value_full) return fail(KH_ERR_INVALID, "null argument");
    if (batch < 1) return fail(KH_ERR_INVALID, "batch must be >= 1");
    auto W = current_weights(e);
    if (!W) return fail(KH_ERR_NO_WEIGHTS, "kh_infer_device before kh_load_weights");
    int rc = set_device(e);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(e->dmu);
    Slot* s;
    hipStream_t st;
    if ((rc = dev_slot(e, batch, stream, &s, &st))) return rc;
    if ((rc = forward_dispatch(e, *W, *s, st, static_cast<const float*>(d_input), batch, d_policy, d_value_full, nullptr))) return rc;
    return dev_slot_done(e, *W, *s, st);
}

int kh_encode_device(kh_engine* e, const kh_board* d_boards, int batch, float* d_planes, void* stream)
{
    if (!e || !d_boards || !d_planes) return fail(KH_ERR_INVALID, "null argument");
    if (batch < 1) return fail(KH_ERR_INVALID, "batch must be >= 1");
    int rc = set_device(e);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(e->dmu);
    if (!e->devslot) e->devslot.reset(new Slot());
    Slot& s = *e->devslot;
    if (!s.stream) HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    kh::launch_encode_f32(d_boards, batch, d_planes, stream ? static_cast<hipStream_t>(stream) : s.stream);
    HIPCHK(hipGetLastError());
    return KH_OK;
}

}  // extern "C"

namespace kh {
int encode_infer_on_device(kh_engine* e, const Weights& W, const kh_board* d_boards, int batch, float* d_policy, float* d_vfull,
                           void* stream, hipStream_t* st_out)
{
    Slot* s;
    hipStream_t st;
    int rc = dev_slot(e, batch, stream, &s, &st);
    if (rc) return rc;
    *st_out = st;
    if (fused_ingest(e, W)) return forward_tower(e, W, *s, st, nullptr, batch, d_policy, d_vfull, nullptr, d_boards);
    if (s->planes.ensure((size_t)batch * 64 * KH_NFEATURES * 4)) return KH_ERR_HIP;
    kh::launch_encode_f32(d_boards, batch, s->planes.as<float>(), st);
    if ((rc = forward_dispatch(e, W, *s, st, s->planes.as<float>(), batch, d_policy, d_vfull, nullptr))) return rc;
    return dev_slot_done(e, W, *s, st);
}
}  // namespace kh

extern "C" {

int kh_encode_infer_device(kh_engine* e, const kh_board* d_boards, int batch, float* d_policy,
                           float* d_value_full, void* stream)
{
    if (!e || !d_boards || !d_policy || !d_value_full) return fail(KH_ERR_INVALID, "null argument");
    if (batch < 1) return fail(KH_ERR_INVALID, "batch must be >= 1");
    int rc = check_records(e, "kh_encode_infer_device");
    if (rc) return rc;
    auto W = current_weights(e);
    if (!W) return fail(KH_ERR_NO_WEIGHTS, "kh_encode_infer_device before kh_load_weights");
    if ((rc = set_device(e))) return rc;
    std::lock_guard<std::mutex> lk(e->dmu);
    hipStream_t st;
    return kh::encode_infer_on_device(e, *W, d_boards, batch, d_policy, d_value_full, stream, &st);
}

static int time_loop(kh_engine* e, int iters, float* ms, int (*body)(void*), void* ctx)
{
    if (iters < 1 || !ms) return fail(KH_ERR_INVALID, "bad timing arguments");
    int rc = set_device(e);
    if (rc) return rc;
    if (!e->devslot) e->devslot.reset(new Slot());
    Slot& s = *e->devslot;
    if (!s.stream) HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    hipEvent_t t0, t1;
    HIPCHK(hipEventCreate(&t0));
    HIPCHK(hipEventCreate(&t1));
    if ((rc = body(ctx))) return rc;                       // warm-up (sizes scratch)
    HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipEventRecord(t0, s.stream));
    for (int i = 0; i < iters; ++i)
        if ((rc = body(ctx))) return rc;
    HIPCHK(hipEventRecord(t1, s.stream));
    HIPCHK(hipEventSynchronize(t1));
    float total = 0.f;
    HIPCHK(hipEventElapsedTime(&total, t0, t1));
    *ms = total / iters;
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    return KH_OK;
}

struct InferCtx { kh_engine* e; const void* in; int B; float *p, *v; };
struct EncCtx { kh_engine* e; const kh_board* b; int B; float* planes; };

int kh_time_infer_device(kh_engine* e, const void* d_input, int batch, float* d_policy,
                         float* d_value_full, int iters, float* ms_per_launch)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    InferCtx c{ e, d_input, batch, d_policy, d_value_full };
    return time_loop(e, iters, ms_per_launch,
                     [](void* p) { auto* c = static_cast<InferCtx*>(p); return kh_infer_device(c->e, c->in, c->B, c->p, c->v, nullptr); }, &c);
}

int kh_time_encode_device(kh_engine* e, const kh_board* d_boards, int batch, float* d_planes,
                          int iters, float* ms_per_launch)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    EncCtx c{ e, d_boards, batch, d_planes };
    return time_loop(e, iters, ms_per_launch,
                     [](void* p) { auto* c = static_cast<EncCtx*>(p); return kh_encode_device(c->e, c->b, c->B, c->planes, nullptr); }, &c);
}

int kh_pin_buffer(kh_engine* e, void* ptr, size_t bytes)
{
    if (!e || !ptr || !bytes) return fail(KH_ERR_INVALID, "null argument");
    int rc = set_device(e);
    if (rc) return rc;
    HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    std::lock_guard<std::mutex> lk(e->pin_mu);
    e->pinned.emplace_back(static_cast<const char*>(ptr), bytes);
    return KH_OK;
}

int kh_unpin_buffer(kh_engine* e, void* ptr)
{
    if (!e || !ptr) return fail(KH_ERR_INVALID, "null argument");
    {
        std::lock_guard<std::mutex> lk(e->pin_mu);
        auto it = std::find_if(e->pinned.begin(), e->pinned.end(), [&](const std::pair<const char*, size_t>& r) { return r.first == ptr; });
        if (it == e->pinned.end()) return fail(KH_ERR_INVALID, "buffer was not registered with kh_pin_buffer");
        e->pinned.erase(it);
    }
    int rc = set_device(e);
    if (rc) return rc;
    HIPCHK(hipHostUnregister(ptr));
    return KH_OK;
}

int kh_dev_alloc(kh_engine* e, size_t bytes, void** d_ptr)
{
    if (!e || !d_ptr) return fail(KH_ERR_INVALID, "null argument");
    int rc = set_device(e);
    if (rc) return rc;
    HIPCHK(hipMalloc(d_ptr, bytes));
    return KH_OK;
}
int kh_dev_free(kh_engine* e, void* d_ptr)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    int rc = set_device(e);
    if (rc) return rc;
    HIPCHK(hipFree(d_ptr));
    return KH_OK;
}
int kh_memcpy_h2d(kh_engine* e, void* d_dst, const void* h_src, size_t bytes)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    int rc = set_device(e);
    if (rc) return rc;
    HIPCHK(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return KH_OK;
}
int kh_memcpy_d2h(kh_engine* e, void* h_dst, const void* d_src, size_t bytes)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    int rc = set_device(e);
    if (rc) return rc;
    HIPCHK(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return KH_OK;
}
int kh_sync(kh_engine* e)
{
    if (!e) return fail(KH_ERR_INVALID, "null engine");
    int rc = set_device(e);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    return KH_OK;
}

}  // extern "C"
