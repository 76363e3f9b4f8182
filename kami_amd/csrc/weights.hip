// weights.hip — parameter sets: the canonical blob parsed (blob_layout.h), BatchNorm folded into the layers' epilogues,
// the weights packed into each kernel family's fragment order (forward_simple.hip, tower8_mfma.hip, layers_mfma.hip)
// and uploaded, and the result installed as the engine's current set (kh_load_weights, kh_train, checkpoints).
#include "engine.h"
#include "blob_layout.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>

namespace kh {
namespace {

// ------------------------------------------------------------------------------- weights
// Host view of the canonical blob (blob_layout.h).
struct ConvBN { const float *w, *b, *g, *be, *rm, *rv; };
struct HostNet {
    ConvBN stem;
    std::vector<ConvBN> res;
    ConvBN pconv;
    const float *p2w, *p2b;
    ConvBN vconv;
    const float *fcw, *fcb;
};

HostNet parse_blob(const float* blob, int F, int C, int R)
{
    const std::vector<kh_blob::Tensor> L = kh_blob::layout(F, C, R);
    size_t i = 0;
    auto take = [&] { return blob + L[i++].at; };
    auto take_convbn = [&](ConvBN& c) { c.w = take(); c.b = take(); c.g = take(); c.be = take(); c.rm = take(); c.rv = take(); };
    HostNet n;
    take_convbn(n.stem);
    n.res.resize(2 * R);
    for (auto& c : n.res) take_convbn(c);
    take_convbn(n.pconv);
    n.p2w = take();
    n.p2b = take();
    take_convbn(n.vconv);
    n.fcw = take();
    n.fcb = take();
    return n;
}

// Eval-mode BatchNorm folded to an epilogue (scale, shift):
//   bn(conv + bias) = conv * s + ((bias - mean) * s + beta),  s = gamma / sqrt(var + 1e-5)
void fold_bn(const ConvBN& c, int co, float* scale, float* shift)
{
    for (int i = 0; i < co; ++i) {
        const float s = c.g[i] / sqrtf(c.rv[i] + 1e-5f);
        scale[i] = s;
        shift[i] = (c.b[i] - c.rm[i]) * s + c.be[i];
    }
}

uint16_t f2bf16(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // keep NaN a NaN
    u += 0x7fffu + ((u >> 16) & 1u);                                            // round to nearest even
    return (uint16_t)(u >> 16);
}
uint16_t f2f16(float f)
{
    _Float16 h = (_Float16)f;
    uint16_t r;
    memcpy(&r, &h, 2);
    return r;
}

// Append one layer's MFMA A-operand fragments (v_mfma_f32_32x32x16: lane l = (r = l & 31, h = l >> 5)
// holds W[co = ms*32 + r][k = 8h + j], j = 0..7) in consumption order tap -> k-step -> ms, BN scale
// folded in before rounding, zero-padded to (MS*32, KS*16) and to a whole number of 8-fragment chunks.
// ci0: first input channel of this pass (the 33..128-plane stem runs as four 32-channel passes).
// centre_first: 3x3 taps in the order 4,0,1,2,3,5,6,7,8.  perm: the first `perm` k-steps of the
// stream take their activations from the consumer's packed output registers (tower_common.h,
// packed_fragments): slot (h, j) of k-step ks is input channel
// 32 (ks >> 1) + 8 (2 (ks & 1) + (j >> 2)) + 4 h + (j & 3) instead of 16 ks + 8 h + j.
void pack_layer(std::vector<uint16_t>& out, int dtype, const float* w, const float* scale, int Co, int Ci,
                int taps, int KS, int MS, int ci0 = 0, bool centre_first = false, int perm = 0, bool pad = true)
{
    int kstep = 0;
    for (int ti = 0; ti < taps; ++ti) {
        const int tap = !centre_first ? ti : (ti == 0 ? 4 : (ti <= 4 ? ti - 1 : ti));
        for (int ks = 0; ks < KS; ++ks, ++kstep)
            for (int ms = 0; ms < MS; ++ms)
                for (int l = 0; l < 64; ++l) {
                    const int r = l & 31, h = l >> 5;
                    for (int j = 0; j < 8; ++j) {
                        const int co = ms * 32 + r;
                        const int ci = ci0 + (kstep < perm ? 32 * (ks >> 1) + 8 * (2 * (ks & 1) + (j >> 2)) + 4 * h + (j & 3)
                                                           : ks * 16 + 8 * h + j);
                        float v = 0.0f;
                        if (co < Co && ci < Ci) v = w[((size_t)co * Ci + ci) * taps + tap] * (scale ? scale[co] : 1.0f);
                        out.push_back(dtype == KH_BF16 ? f2bf16(v) : f2f16(v));
                    }
                }
    }
    while (pad && out.size() % 4096) out.push_back(0);
}

// Fragments of one layer for layers_mfma.hip, BN scale folded in: 8 KB chunks of 64 input channels x 64
// output channels, [Co/64][Ci/64][tap][4][2][lane][8] — 64-channel slices of the reduction outermost, so that
// the kernel's variants (whole image staged at once, or in passes of 64 / 128 channels) all walk the same
// order and agree bit for bit.
void pack_layer_generic(uint16_t* o, int dtype, const float* w, const float* scale,
                        int Co, int Ci, int taps, int CoP, int CiP)
{
    // (runs at every weight install, the trainer's included: written by index into a slice sized CoP * CiP * taps)
    const bool bf = dtype == KH_BF16;
    for (int cb = 0; cb < CoP / 64; ++cb)
        for (int slice = 0; slice < CiP / 64; ++slice)
            for (int tap = 0; tap < taps; ++tap)
                for (int kk = 0; kk < 4; ++kk)
                    for (int ms = 0; ms < 2; ++ms)
                        for (int l = 0; l < 64; ++l) {
                            const int r = l & 31, h = l >> 5, ks = slice * 4 + kk;
                            const int co = cb * 64 + ms * 32 + r, ci0 = ks * 16 + 8 * h;
                            const float sc = scale ? (co < Co ? scale[co] : 0.0f) : 1.0f;
                            const float* src = w + ((size_t)co * Ci + ci0) * taps + tap;
                            for (int j = 0; j < 8; ++j) {
                                const float v = (co < Co && ci0 + j < Ci) ? src[(size_t)j * taps] * sc : 0.0f;
                                *o++ = bf ? f2bf16(v) : f2f16(v);
                            }
                        }
}

// The same fragments for conv4_mfma_kernel (four boards x 128 output channels per workgroup): 8 KB chunks of 32 input
// channels x 128 output channels, [Co/128][Ci/64][tap][half][ks2][ms 0..3][lane][8] — the reduction walks in the same
// order as above (64-channel slices, then taps, then k-steps), so both kernels produce the same bits.
void pack_layer_wide128(uint16_t* o, int dtype, const float* w, const float* scale,
                        int Co, int Ci, int taps, int CoP, int CiP, int CBC = 128)
{
    // CBC: output channels per block — 128 (conv4_mfma_kernel, tower128_kernel, policy_head4_kernel) or 256
    // (tower256_kernel: eight row tiles per k-step, one k-step per 8 KB chunk)
    const bool bf = dtype == KH_BF16;
    for (int cb = 0; cb < CoP / CBC; ++cb)
        for (int slice = 0; slice < CiP / 64; ++slice)
            for (int tap = 0; tap < taps; ++tap)
                for (int kk = 0; kk < 4; ++kk)                  // kk = 2 * half + ks2
                    for (int ms = 0; ms < CBC / 32; ++ms)
                        for (int l = 0; l < 64; ++l) {
                            const int r = l & 31, h = l >> 5, ks = slice * 4 + kk;
                            const int co = cb * CBC + ms * 32 + r, ci0 = ks * 16 + 8 * h;
                            const float sc = scale ? (co < Co ? scale[co] : 0.0f) : 1.0f;
                            const float* src = w + ((size_t)co * Ci + ci0) * taps + tap;
                            for (int j = 0; j < 8; ++j) {
                                const float v = (co < Co && ci0 + j < Ci) ? src[(size_t)j * taps] * sc : 0.0f;
                                *o++ = bf ? f2bf16(v) : f2f16(v);
                            }
                        }
}

// fp32 fragments for conv_f32_kernel: [Co/64][Ci slices of <= 128][tap][slice/8][2][lane][4]; lane (r, h) holds
// W[co = ms*32 + r][ci = 8j + 4h + 0..3]  (one slice up to 128 input channels: the image of a slice is what fits LDS)
void pack_layer_f32(float* o, const float* w, const float* scale, int Co, int Ci, int taps, int CoP, int CiP)
{
    for (int cb = 0; cb < CoP / 64; ++cb)
      for (int c_lo = 0; c_lo < CiP; c_lo += 128)
        for (int tap = 0; tap < taps; ++tap)
            for (int j = c_lo / 8; j < (c_lo + 128 < CiP ? c_lo + 128 : CiP) / 8; ++j)
                for (int ms = 0; ms < 2; ++ms)
                    for (int l = 0; l < 64; ++l) {
                        const int r = l & 31, h = l >> 5;
                        for (int i = 0; i < 4; ++i) {
                            const int co = cb * 64 + ms * 32 + r, ci = j * 8 + 4 * h + i;
                            *o++ = (co < Co && ci < Ci) ? w[((size_t)co * Ci + ci) * taps + tap] * (scale ? scale[co] : 1.0f) : 0.0f;
                        }
                    }
}

int build_layers(Weights& W, const HostNet& n, int dtype, int F, int C, int R)
{
    const bool f32 = dtype == KH_F32;
    // bf16/f16: input channels in multiples of 64 (an 8 KB weight chunk = 4 k-steps of one tap)
    const int FP = f32 ? (F + 7) / 8 * 8 : (F + 63) / 64 * 64, CP = (C + 63) / 64 * 64;
    // LDS image of two boards: 2 x 120 x (Ci * elem + 16) bytes must fit 160 KB
    if (CP > 256 || FP > 256) return KH_OK;      // not covered: ly_ok stays false
    // Every layer's fragments are packed by its own job into its own slice: the jobs run on a few host threads (this is
    // on the trainer's path too — kh_train installs its result here — and a 20x256 net is 48 M fragments' worth).
    std::vector<uint16_t> w, w4, wh, w2b;
    std::vector<float> wf;
    std::vector<float> shift;
    struct Job { int kind; size_t off; const float* wt; std::vector<float> sc; int Co, Ci, taps, CoP, CiP; };   // kind 0 generic, 1 wide128, 2 f32, 3 head
    std::vector<Job> jobs;
    size_t nw = 0, nw4 = 0, nwf = 0, nwh = 0, nw2b = 0;
    const bool want2b = !f32 && CP == 256 && FP == 128;      // tower256_kernel's shape
    std::vector<float> sc(256), sh(256);
    auto add = [&](const float* wt, const ConvBN* bn, const float* bias, int Co, int Ci, int taps, int CoP, int CiP) {
        W.ly_shift_off.push_back(shift.size());
        W.ly_w4_off.push_back((size_t)-1);
        if (bn) fold_bn(*bn, Co, sc.data(), sh.data());
        else for (int i = 0; i < Co; ++i) { sc[i] = 1.0f; sh[i] = bias[i]; }
        const std::vector<float> scv(sc.begin(), sc.begin() + Co);
        const size_t n = (size_t)CoP * CiP * taps;
        if (f32) { W.ly_w_off.push_back(nwf); jobs.push_back({ 2, nwf, wt, scv, Co, Ci, taps, CoP, CiP }); nwf += n; }
        else {
            W.ly_w_off.push_back(nw); jobs.push_back({ 0, nw, wt, scv, Co, Ci, taps, CoP, CiP }); nw += n;
            if (taps == 9 && CoP % 128 == 0 && (CiP == 128 || CiP == 256)) {     // conv4_mfma_kernel's shapes
                W.ly_w4_off.back() = nw4; jobs.push_back({ 1, nw4, wt, scv, Co, Ci, taps, CoP, CiP }); nw4 += n;
            }
            if (want2b && taps == 9) { jobs.push_back({ 4, nw2b, wt, scv, Co, Ci, taps, CoP, CiP }); nw2b += n; }
        }
        for (int i = 0; i < CoP; ++i) shift.push_back(i < Co ? sh[i] : 0.0f);
    };
    add(n.stem.w, &n.stem, nullptr, C, F, 9, CP, FP);
    for (int i = 0; i < 2 * R; ++i) add(n.res[i].w, &n.res[i], nullptr, C, C, 9, CP, CP);
    add(n.pconv.w, &n.pconv, nullptr, KH_POLICY_MID, C, 1, KH_POLICY_MID, CP);
    add(n.p2w, nullptr, n.p2b, KH_POLICY_PLANES, KH_POLICY_MID, 1, 128, KH_POLICY_MID);
    if (!f32 && (CP == 128 || CP == 256)) {          // policy_head4_kernel's shapes: policyconv then policyconv2
        fold_bn(n.pconv, KH_POLICY_MID, sc.data(), sh.data());
        jobs.push_back({ 3, nwh, n.pconv.w, std::vector<float>(sc.begin(), sc.begin() + KH_POLICY_MID), KH_POLICY_MID, C, 1, KH_POLICY_MID, CP });
        nwh += (size_t)KH_POLICY_MID * CP;
        jobs.push_back({ 3, nwh, n.p2w, std::vector<float>(), KH_POLICY_PLANES, KH_POLICY_MID, 1, 128, KH_POLICY_MID });
        nwh += (size_t)128 * KH_POLICY_MID;
    }
    w.resize(nw); w4.resize(nw4); wf.resize(nwf); wh.resize(nwh); w2b.resize(nw2b);
    {
        std::atomic<size_t> next{ 0 };
        auto run = [&]() {
            for (size_t j; (j = next.fetch_add(1)) < jobs.size();) {
                const Job& jb = jobs[j];
                const float* scp = jb.sc.empty() ? nullptr : jb.sc.data();
                if (jb.kind == 0) pack_layer_generic(w.data() + jb.off, dtype, jb.wt, scp, jb.Co, jb.Ci, jb.taps, jb.CoP, jb.CiP);
                else if (jb.kind == 1) pack_layer_wide128(w4.data() + jb.off, dtype, jb.wt, scp, jb.Co, jb.Ci, jb.taps, jb.CoP, jb.CiP);
                else if (jb.kind == 2) pack_layer_f32(wf.data() + jb.off, jb.wt, scp, jb.Co, jb.Ci, jb.taps, jb.CoP, jb.CiP);
                else if (jb.kind == 4) pack_layer_wide128(w2b.data() + jb.off, dtype, jb.wt, scp, jb.Co, jb.Ci, jb.taps, jb.CoP, jb.CiP, 256);
                else pack_layer_wide128(wh.data() + jb.off, dtype, jb.wt, scp, jb.Co, jb.Ci, jb.taps, jb.CoP, jb.CiP);
            }
        };
        const int nt = (int)std::min<size_t>(8, jobs.size());
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(run);
        run();
        for (auto& t : th) t.join();
    }
    std::vector<float> misc((size_t)CP + KH_VALUE_WIDTH * 64 + KH_VALUE_WIDTH + (size_t)KH_VALUE_WIDTH * 64, 0.0f);      // ... + fc4
    float vs, vsh;
    fold_bn(n.vconv, 1, &vs, &vsh);
    for (int i = 0; i < C; ++i) misc[i] = n.vconv.w[i] * vs;
    memcpy(misc.data() + CP, n.fcw, sizeof(float) * KH_VALUE_WIDTH * 64);
    memcpy(misc.data() + CP + (size_t)KH_VALUE_WIDTH * 64, n.fcb, sizeof(float) * KH_VALUE_WIDTH);
    {
        // valuefc.weight once more as [k / 4][output][4]: 64 lanes that take 64 consecutive outputs read 1 KB in one piece per
        // k-group (policy_head4_kernel / tower128_kernel's value FC; from the [256][64] rows every lane's 16 bytes were a
        // cache line of their own: 24 000 clocks of a 48 000-clock head)
        float* fc4 = misc.data() + CP + (size_t)KH_VALUE_WIDTH * 64 + KH_VALUE_WIDTH;
        for (int j = 0; j < KH_VALUE_WIDTH; ++j)
            for (int k = 0; k < 64; ++k) fc4[((size_t)(k / 4) * KH_VALUE_WIDTH + j) * 4 + (k & 3)] = n.fcw[(size_t)j * 64 + k];
    }
    W.ly_vshift = vsh; W.ly_FP = FP; W.ly_CP = CP;
    const void* wsrc = f32 ? (const void*)wf.data() : (const void*)w.data();
    const size_t wbytes = f32 ? wf.size() * 4 : w.size() * 2;
    if (W.ly_w.ensure(wbytes) || W.ly_shift.ensure(shift.size() * 4) || W.ly_misc.ensure(misc.size() * 4)) return KH_ERR_HIP;
    HIPCHK(hipMemcpy(W.ly_w.p, wsrc, wbytes, hipMemcpyHostToDevice));
    if (!w4.empty()) {
        if (W.ly_w4.ensure(w4.size() * 2)) return KH_ERR_HIP;
        HIPCHK(hipMemcpy(W.ly_w4.p, w4.data(), w4.size() * 2, hipMemcpyHostToDevice));
    }
    if (!w2b.empty()) {
        if (W.ly_w2b.ensure(w2b.size() * 2)) return KH_ERR_HIP;
        HIPCHK(hipMemcpy(W.ly_w2b.p, w2b.data(), w2b.size() * 2, hipMemcpyHostToDevice));
        W.ly_w2b_ok = true;
    }
    if (!wh.empty()) {
        if (W.ly_wh.ensure(wh.size() * 2)) return KH_ERR_HIP;
        HIPCHK(hipMemcpy(W.ly_wh.p, wh.data(), wh.size() * 2, hipMemcpyHostToDevice));
        W.ly_wh_ok = true;
    }
    HIPCHK(hipMemcpy(W.ly_shift.p, shift.data(), shift.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(W.ly_misc.p, misc.data(), misc.size() * 4, hipMemcpyHostToDevice));
    W.ly_ok = true;
    return KH_OK;
}

int build_tower(Weights& W, const HostNet& n, int dtype, int F, int C, int R)
{
    using namespace kh;
    if (C > TW_CP) { W.tw_why = "filters > 64 not supported by the MFMA tower kernel yet"; return KH_OK; }
    if (F > 128) { W.tw_why = "features > 128 not supported by the MFMA tower kernel yet"; return KH_OK; }
    const int FP = F <= 32 ? 32 : 128;
    if (tower_lds_bytes(FP, R) > 160 * 1024) { W.tw_why = "too many residual blocks for the LDS parameter area"; return KH_OK; }
    std::vector<float> sc(128), sh(128);
    std::vector<uint16_t> stream;
    std::vector<float> par((size_t)tower_par_copy_floats(R), 0.0f);
    fold_bn(n.stem, C, sc.data(), sh.data());
    if (FP == 128) {        // four 32-plane passes in one unpadded run of 72 k-steps: the later quarters of the planes are
                            // still being converted while the first passes run
        for (int q = 0; q < 4; ++q) pack_layer(stream, dtype, n.stem.w, sc.data(), C, F, 9, 2, 2, 32 * q, false, 0, false);
        if (stream.size() != (size_t)18 * 4096) return fail(KH_ERR_INVALID, "internal: stem stream size");
    } else {
        pack_layer(stream, dtype, n.stem.w, sc.data(), C, F, 9, FP / 16, 2);
    }
    memcpy(par.data(), sh.data(), sizeof(float) * C);
    for (int i = 0; i < 2 * R; ++i) {
        fold_bn(n.res[i], C, sc.data(), sh.data());
        pack_layer(stream, dtype, n.res[i].w, sc.data(), C, C, 9, TW_CP / 16, 2, 0, true, TW_CP / 16);
        memcpy(par.data() + (size_t)(1 + i) * TW_CP, sh.data(), sizeof(float) * C);
    }
    float* pshift1 = par.data() + (size_t)(1 + 2 * R) * TW_CP;
    fold_bn(n.pconv, KH_POLICY_MID, sc.data(), pshift1);
    pack_layer(stream, dtype, n.pconv.w, sc.data(), KH_POLICY_MID, C, 1, TW_CP / 16, 4, 0, false, TW_CP / 16);
    float* pbias2 = pshift1 + KH_POLICY_MID;
    memcpy(pbias2, n.p2b, sizeof(float) * KH_POLICY_PLANES);
    {
        // 73 planes on three 32-row tiles: a chunk holds 2 k-steps x 3 tiles = 6 fragments, padded to the ring's 8 KB
        std::vector<uint16_t> p2;
        pack_layer(p2, dtype, n.p2w, nullptr, KH_POLICY_PLANES, KH_POLICY_MID, 1, KH_POLICY_MID / 16, 3, 0, false, KH_POLICY_MID / 16, false);
        constexpr size_t FRAG = 512, CHUNK_FRAGS = 6;
        if (p2.size() != (size_t)(KH_POLICY_MID / 16) * 3 * FRAG) return fail(KH_ERR_INVALID, "internal: policyconv2 stream size");
        for (size_t c = 0; c < p2.size(); c += CHUNK_FRAGS * FRAG) {
            stream.insert(stream.end(), p2.begin() + c, p2.begin() + c + CHUNK_FRAGS * FRAG);
            stream.resize(stream.size() + (8 - CHUNK_FRAGS) * FRAG, 0);
        }
    }
    if (((stream.size() / 4096) & 1) != 0) stream.resize(stream.size() + 4096, 0);   // parity chunk (see gemm8_dummy)
    float* vw = pbias2 + 128;
    float vs, vsh;
    fold_bn(n.vconv, 1, &vs, &vsh);
    for (int i = 0; i < C; ++i) vw[i] = n.vconv.w[i] * vs;
    vw[TW_CP] = vsh;
    // valuefc.weight [256][64] -> [k/4][j][4] so that thread j reads coalesced float4
    std::vector<float> fc4((size_t)KH_VALUE_WIDTH * 64 + KH_VALUE_WIDTH);
    for (int j = 0; j < KH_VALUE_WIDTH; ++j)
        for (int k = 0; k < 64; ++k) fc4[((size_t)(k / 4) * KH_VALUE_WIDTH + j) * 4 + (k & 3)] = n.fcw[(size_t)j * 64 + k];
    memcpy(fc4.data() + (size_t)KH_VALUE_WIDTH * 64, n.fcb, sizeof(float) * KH_VALUE_WIDTH);

    W.tw_nchunks = (int)(stream.size() / 4096);
    W.tw_npar = (int)par.size();
    W.tw_FP = FP;
    int rc = 0;
    rc |= W.tw_stream.ensure(stream.size() * 2);
    rc |= W.tw_par.ensure(par.size() * 4);
    rc |= W.tw_fc4.ensure(fc4.size() * 4);
    if (rc) return KH_ERR_HIP;
    HIPCHK(hipMemcpy(W.tw_stream.p, stream.data(), stream.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(W.tw_par.p, par.data(), par.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(W.tw_fc4.p, fc4.data(), fc4.size() * 4, hipMemcpyHostToDevice));
    W.tw_ok = true;
    return KH_OK;
}

int build_simple(Weights& W, const HostNet& n, int F, int C, int R)
{
    struct Plan { const float* w; int Ci, Co, taps, relu; const ConvBN* bn; const float* bias; };
    std::vector<Plan> plan;
    plan.push_back({ n.stem.w, F, C, 9, 1, &n.stem, nullptr });
    for (int i = 0; i < 2 * R; ++i) plan.push_back({ n.res[i].w, C, C, 9, 1, &n.res[i], nullptr });
    plan.push_back({ n.pconv.w, C, KH_POLICY_MID, 1, 1, &n.pconv, nullptr });
    plan.push_back({ n.p2w, KH_POLICY_MID, KH_POLICY_PLANES, 1, 0, nullptr, n.p2b });
    plan.push_back({ n.vconv.w, C, 1, 1, 1, &n.vconv, nullptr });

    size_t total = 0;
    for (auto& p : plan) total += (size_t)p.taps * p.Ci * p.Co + 2 * (size_t)p.Co;
    total += (size_t)KH_VALUE_WIDTH * 64 + KH_VALUE_WIDTH;
    std::vector<float> host(total);
    int rc = W.simple.ensure(total * sizeof(float));
    if (rc) return rc;
    float* dbase = W.simple.as<float>();
    size_t off = 0;
    for (auto& p : plan) {
        kh::SimpleLayer L;
        L.Ci = p.Ci; L.Co = p.Co; L.taps = p.taps; L.relu = p.relu;
        float* wt = host.data() + off;
        // libtorch [Co][Ci][kh][kw] -> [tap][Ci][Co]
        for (int co = 0; co < p.Co; ++co)
            for (int ci = 0; ci < p.Ci; ++ci)
                for (int k = 0; k < p.taps; ++k)
                    wt[((size_t)k * p.Ci + ci) * p.Co + co] = p.w[((size_t)co * p.Ci + ci) * p.taps + k];
        L.wt = dbase + off;
        off += (size_t)p.taps * p.Ci * p.Co;
        float* sc = host.data() + off;
        float* sh = sc + p.Co;
        if (p.bn) fold_bn(*p.bn, p.Co, sc, sh);
        else for (int i = 0; i < p.Co; ++i) { sc[i] = 1.0f; sh[i] = p.bias[i]; }
        L.scale = dbase + off; L.shift = dbase + off + p.Co;
        off += 2 * (size_t)p.Co;
        W.layers.push_back(L);
    }
    memcpy(host.data() + off, n.fcw, sizeof(float) * KH_VALUE_WIDTH * 64);
    W.fcw = dbase + off; off += (size_t)KH_VALUE_WIDTH * 64;
    memcpy(host.data() + off, n.fcb, sizeof(float) * KH_VALUE_WIDTH);
    W.fcb = dbase + off; off += KH_VALUE_WIDTH;
    HIPCHK(hipMemcpy(dbase, host.data(), total * sizeof(float), hipMemcpyHostToDevice));
    return KH_OK;
}

}  // namespace

int load_weights_impl(kh_engine* e, const float* blob, size_t nfloats, int generation, int64_t bn_batches,
                      std::shared_ptr<Weights>* installed)
{
    if (!e || !blob) return fail(KH_ERR_INVALID, "null argument");
    const int F = e->cfg.features, C = e->cfg.filters, R = e->cfg.residuals;
    if (nfloats != kh_weight_count(F, C, R))
        return fail(KH_ERR_INVALID, "weight blob has %zu floats, expected %zu for F=%d C=%d R=%d",
                    nfloats, kh_weight_count(F, C, R), F, C, R);
    int rc = set_device(e);
    if (rc) return rc;
    auto W = std::make_shared<Weights>();
    W->generation = generation;
    W->bn_batches = bn_batches;
    W->blob.assign(blob, blob + nfloats);
    HostNet n = parse_blob(W->blob.data(), F, C, R);
    if (e->cfg.dtype == KH_F32) {
        if ((rc = build_simple(*W, n, F, C, R))) return rc;
        if (!e->f32_simple && (rc = build_layers(*W, n, KH_F32, F, C, R))) return rc;
    } else {
        if ((rc = build_tower(*W, n, e->cfg.dtype, F, C, R))) return rc;
        if (!W->tw_ok && (rc = build_layers(*W, n, e->cfg.dtype, F, C, R))) return rc;
    }
    std::lock_guard<std::mutex> lk(e->wmu);
    e->weights = W;                  // calls in flight keep their own reference
    e->has_weights.store(true, std::memory_order_release);
    if (installed) *installed = W;
    return KH_OK;
}

}  // namespace kh
