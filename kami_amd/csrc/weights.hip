// weights.hip — parameter sets: the canonical blob parsed (blob_layout.h), BatchNorm folded into the layers' epilogues,
// the weights packed into each kernel family's fragment order (forward_simple.hip, tower8_mfma.hip, layers_mfma.hip),
// and the result installed as the engine's current set.  What goes where is planned once (plan_set), as the jobs of
// weights_pack.h, and bound to one of two memories: a blob in host memory is packed by run_host's loops over that
// header's layout functions and uploaded (kh_load_weights, checkpoints, kh_clone), a blob in device memory by the kernels
// of weights_pack.hip over the same functions (kh_load_weights_device, kh_train's result).
#include "engine.h"
#include "blob_layout.h"
#include "weights_pack.h"

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

// ------------------------------------------------------------------------------- the plan
// What a parameter set's serving buffers hold, stated once: every buffer's size, every layer's place and layout in it
// and every folded parameter's, as jobs (weights_pack.h) over pointers into the blob.  The pointers are only offset here,
// never read, so the same plan describes a blob in host memory (run_host) and one in device memory (run_device).  The
// coverage decisions (tw_why, ly_ok, which extra layouts a shape gets) are made here.
enum Buf { B_TW_STREAM, B_TW_PAR, B_TW_FC4, B_LY_W, B_LY_W4, B_LY_W2B, B_LY_WH, B_LY_SHIFT, B_LY_MISC, B_SIMPLE, NBUF };

DevMem& buf_of(Weights& W, int b)
{
    DevMem* m[NBUF] = { &W.tw_stream, &W.tw_par, &W.tw_fc4, &W.ly_w, &W.ly_w4, &W.ly_w2b, &W.ly_wh, &W.ly_shift, &W.ly_misc, &W.simple };
    return *m[b];
}

struct SimpleOff { size_t wt, scale, shift; int Ci, Co, taps, relu; };
struct Plan {
    int dtype = KH_F32, fold_stride = 0;
    std::vector<FoldJob> folds;                          // stem, 2R tower convs, policyconv, policyconv2 (bias), valueconv
    std::vector<PackJob> packs;
    std::vector<CopyJob> copies;
    unsigned pack_blocks = 0, copy_blocks = 0;           // workgroups of the device packer's launches (bind)
    size_t bytes[NBUF] = {};
    bool threads = false;                                // run_host: pack on several host threads (the wide nets' volumes)
    std::vector<SimpleOff> simple;
    size_t simple_fcw = 0, simple_fcb = 0;
    int f_stem() const { return 0; }
    int f_res(int i) const { return 1 + i; }
    int f_pconv() const { return (int)folds.size() - 3; }
    int f_p2() const { return (int)folds.size() - 2; }
    int f_vconv() const { return (int)folds.size() - 1; }
    size_t fold_floats() const { return folds.size() * 2 * (size_t)fold_stride; }
    size_t fold_at(FoldRef r) const { return ((size_t)r.item * 2 + r.shift) * fold_stride; }
};

FoldJob fold_job(const ConvBN& c, int co, float* scale = nullptr, float* shift = nullptr)
{
    return { c.b, c.g, c.be, c.rm, c.rv, scale, shift, co };
}

void plan_folds(Plan& P, const HostNet& n, int C, int R)
{
    P.fold_stride = std::max(C, (int)KH_POLICY_MID);
    P.folds.push_back(fold_job(n.stem, C));
    for (int i = 0; i < 2 * R; ++i) P.folds.push_back(fold_job(n.res[i], C));
    P.folds.push_back(fold_job(n.pconv, KH_POLICY_MID));
    P.folds.push_back(fold_job(ConvBN{ nullptr, n.p2b, nullptr, nullptr, nullptr, nullptr }, KH_POLICY_PLANES));
    P.folds.push_back(fold_job(n.vconv, 1));
}

// a layer's fragments at byte `off` of `buf`, `bytes` long with their padding; the caller sets the layout's own fields
PackJob& pack_item(Plan& P, int buf, size_t off, size_t bytes, int kind, const float* w, int fold, int Co, int Ci, int taps)
{
    PackJob j{};
    j.w = w; j.fold = fold; j.buf = buf; j.off = off;
    j.groups = (unsigned)(bytes / 16);
    j.kind = kind; j.dtype = P.dtype; j.Co = Co; j.Ci = Ci; j.taps = taps;
    j.chunk_frags = 8;
    P.packs.push_back(j);
    P.bytes[buf] = std::max(P.bytes[buf], off + bytes);
    return P.packs.back();
}

void copy_item(Plan& P, int buf, size_t off, int kind, const float* src, FoldRef fsrc, int n, int npad, int scale_of = -1,
               int Co = 0, int Ci = 0, int taps = 0)
{
    P.copies.push_back({ src, fsrc, scale_of, buf, off, nullptr, nullptr, (unsigned)n, (unsigned)npad, 0, kind, Co, Ci, taps });
    P.bytes[buf] = std::max(P.bytes[buf], (off + npad) * sizeof(float));
}

void copy_fc4(Plan& P, int buf, size_t off, const float* fcw)
{
    copy_item(P, buf, off, CP_FC4, fcw, {}, KH_VALUE_WIDTH * 64, KH_VALUE_WIDTH * 64);
}

int plan_layers(Plan& P, Weights& W, const HostNet& n, int dtype, int F, int C, int R)
{
    const bool f32 = dtype == KH_F32;
    // bf16/f16: input channels in multiples of 64 (an 8 KB weight chunk = 4 k-steps of one tap)
    const int FP = f32 ? (F + 7) / 8 * 8 : (F + 63) / 64 * 64, CP = (C + 63) / 64 * 64;
    // LDS image of two boards: 2 x 120 x (Ci * elem + 16) bytes must fit 160 KB
    if (CP > 256 || FP > 256) return KH_OK;      // not covered: ly_ok stays false
    // Every layer's fragments are packed by its own job into its own slice (this is on the trainer's path too — kh_train
    // installs its result here — and a 20x256 net is 48 M fragments' worth).
    const size_t el = f32 ? 4 : 2;
    size_t nw = 0, nw4 = 0, nwh = 0, nw2b = 0, nshift = 0;
    const bool want2b = !f32 && CP == 256 && FP == 128;      // tower256_kernel's shape
    auto blocks = [&](int buf, size_t& at, int kind, const float* wt, int fold, int Co, int Ci, int taps, int CoP, int CiP, int CBC) {
        const size_t nel = (size_t)CoP * CiP * taps;
        PackJob& j = pack_item(P, buf, at * el, nel * el, kind, wt, fold, Co, Ci, taps);
        j.CiP = CiP; j.CBC = CBC;
        at += nel;
    };
    auto add = [&](const float* wt, int fold, int Co, int Ci, int taps, int CoP, int CiP) {
        W.ly_shift_off.push_back(nshift);
        W.ly_w4_off.push_back((size_t)-1);
        W.ly_w_off.push_back(nw);
        if (f32) blocks(B_LY_W, nw, PK_F32, wt, fold, Co, Ci, taps, CoP, CiP, 64);
        else {
            blocks(B_LY_W, nw, PK_BLOCKS, wt, fold, Co, Ci, taps, CoP, CiP, 64);
            if (taps == 9 && CoP % 128 == 0 && (CiP == 128 || CiP == 256)) {     // conv4_mfma_kernel's shapes
                W.ly_w4_off.back() = nw4;
                blocks(B_LY_W4, nw4, PK_BLOCKS, wt, fold, Co, Ci, taps, CoP, CiP, 128);
            }
            if (want2b && taps == 9) blocks(B_LY_W2B, nw2b, PK_BLOCKS, wt, fold, Co, Ci, taps, CoP, CiP, 256);
        }
        copy_item(P, B_LY_SHIFT, nshift, CP_COPY, nullptr, { fold, 1 }, Co, CoP);
        nshift += CoP;
    };
    add(n.stem.w, P.f_stem(), C, F, 9, CP, FP);
    for (int i = 0; i < 2 * R; ++i) add(n.res[i].w, P.f_res(i), C, C, 9, CP, CP);
    add(n.pconv.w, P.f_pconv(), KH_POLICY_MID, C, 1, KH_POLICY_MID, CP);
    add(n.p2w, P.f_p2(), KH_POLICY_PLANES, KH_POLICY_MID, 1, 128, KH_POLICY_MID);
    if (!f32 && (CP == 128 || CP == 256)) {          // policy_head4_kernel's shapes: policyconv then policyconv2
        blocks(B_LY_WH, nwh, PK_BLOCKS, n.pconv.w, P.f_pconv(), KH_POLICY_MID, C, 1, KH_POLICY_MID, CP, 128);
        blocks(B_LY_WH, nwh, PK_BLOCKS, n.p2w, -1, KH_POLICY_PLANES, KH_POLICY_MID, 1, 128, KH_POLICY_MID, 128);
        W.ly_wh_ok = true;
    }
    W.ly_w2b_ok = nw2b != 0;
    // ly_misc: vw[CP], fcw[256*64], fcb[256], fc4[16][256][4]
    size_t m = 0;
    copy_item(P, B_LY_MISC, m, CP_MULS, n.vconv.w, {}, C, CP, P.f_vconv());
    m += CP;
    copy_item(P, B_LY_MISC, m, CP_COPY, n.fcw, {}, KH_VALUE_WIDTH * 64, KH_VALUE_WIDTH * 64);
    m += (size_t)KH_VALUE_WIDTH * 64;
    copy_item(P, B_LY_MISC, m, CP_COPY, n.fcb, {}, KH_VALUE_WIDTH, KH_VALUE_WIDTH);
    m += KH_VALUE_WIDTH;
    copy_fc4(P, B_LY_MISC, m, n.fcw);
    W.ly_FP = FP; W.ly_CP = CP;
    W.ly_ok = true;
    P.threads = true;
    return KH_OK;
}

int plan_tower(Plan& P, Weights& W, const HostNet& n, int F, int C, int R)
{
    if (C > TW_CP) { W.tw_why = "filters > 64 not supported by the MFMA tower kernel yet"; return KH_OK; }
    if (F > 128) { W.tw_why = "features > 128 not supported by the MFMA tower kernel yet"; return KH_OK; }
    const int FP = F <= 32 ? 32 : 128;
    if (tower_lds_bytes(FP, R) > 160 * 1024) { W.tw_why = "too many residual blocks for the LDS parameter area"; return KH_OK; }
    constexpr size_t FRAG = 512;                 // 16-bit values of one fragment; an 8 KB chunk of the ring holds 8
    size_t at = 0;                               // values of the stream so far
    // chunk_frags < 8: every chunk takes that many fragments of the layer and is zero-padded to 8; pad: the layer is
    // zero-padded to a whole number of chunks
    auto stream = [&](const float* w, int fold, int Co, int Ci, int taps, int KS, int MS, int ci0, bool centre_first, int perm,
                      int chunk_frags, bool pad) {
        const size_t frags = (size_t)taps * KS * MS;
        const size_t out = chunk_frags < 8 ? frags / chunk_frags * 8 : (pad ? (frags + 7) / 8 * 8 : frags);
        PackJob& j = pack_item(P, B_TW_STREAM, at * 2, out * FRAG * 2, PK_STREAM, w, fold, Co, Ci, taps);
        j.KS = KS; j.MS = MS; j.ci0 = ci0; j.centre_first = centre_first; j.perm = perm; j.chunk_frags = chunk_frags;
        at += out * FRAG;
    };
    if (FP == 128) {        // four 32-plane passes in one unpadded run of 72 k-steps: the later quarters of the planes are
                            // still being converted while the first passes run
        for (int q = 0; q < 4; ++q) stream(n.stem.w, P.f_stem(), C, F, 9, 2, 2, 32 * q, false, 0, 8, false);
        if (at != (size_t)18 * 4096) return fail(KH_ERR_INVALID, "internal: stem stream size");
    } else {
        stream(n.stem.w, P.f_stem(), C, F, 9, FP / 16, 2, 0, false, 0, 8, true);
    }
    for (int i = 0; i < 2 * R; ++i) stream(n.res[i].w, P.f_res(i), C, C, 9, TW_CP / 16, 2, 0, true, TW_CP / 16, 8, true);
    stream(n.pconv.w, P.f_pconv(), KH_POLICY_MID, C, 1, TW_CP / 16, 4, 0, false, TW_CP / 16, 8, true);
    // 73 planes on three 32-row tiles: a chunk holds 2 k-steps x 3 tiles = 6 fragments, padded to the ring's 8 KB
    static_assert((KH_POLICY_MID / 16 * 3) % 6 == 0, "policyconv2 fills whole chunks of 6 fragments");
    stream(n.p2w, -1, KH_POLICY_PLANES, KH_POLICY_MID, 1, KH_POLICY_MID / 16, 3, 0, false, KH_POLICY_MID / 16, 6, false);
    if (at % 4096) return fail(KH_ERR_INVALID, "internal: weight stream is not whole chunks");
    if (((at / 4096) & 1) != 0) stream(nullptr, -1, 0, 0, 1, 1, 8, 0, false, 0, 8, true);   // parity chunk (see gemm8_dummy): zeros

    // tw_par: shifts of the 1 + 2R 3x3 layers [TW_CP each], policyconv shift [128], policyconv2 bias [128], valueconv
    // weight * scale [TW_CP], valueconv shift [4]
    size_t p = 0;
    copy_item(P, B_TW_PAR, p, CP_COPY, nullptr, { P.f_stem(), 1 }, C, TW_CP);
    p += TW_CP;
    for (int i = 0; i < 2 * R; ++i, p += TW_CP) copy_item(P, B_TW_PAR, p, CP_COPY, nullptr, { P.f_res(i), 1 }, C, TW_CP);
    copy_item(P, B_TW_PAR, p, CP_COPY, nullptr, { P.f_pconv(), 1 }, KH_POLICY_MID, 128);
    p += 128;
    copy_item(P, B_TW_PAR, p, CP_COPY, n.p2b, {}, KH_POLICY_PLANES, 128);
    p += 128;
    copy_item(P, B_TW_PAR, p, CP_MULS, n.vconv.w, {}, C, TW_CP, P.f_vconv());
    p += TW_CP;
    copy_item(P, B_TW_PAR, p, CP_COPY, nullptr, { P.f_vconv(), 1 }, 1, 4);
    p += 4;
    if (p != (size_t)tower_par_copy_floats(R)) return fail(KH_ERR_INVALID, "internal: tower parameter block size");
    copy_fc4(P, B_TW_FC4, 0, n.fcw);
    copy_item(P, B_TW_FC4, (size_t)KH_VALUE_WIDTH * 64, CP_COPY, n.fcb, {}, KH_VALUE_WIDTH, KH_VALUE_WIDTH);

    W.tw_nchunks = (int)(at / 4096);
    W.tw_npar = (int)p;
    W.tw_FP = FP;
    W.tw_ok = true;
    return KH_OK;
}

void plan_simple(Plan& P, const HostNet& n, int F, int C, int R)
{
    struct L { const float* w; int Ci, Co, taps, relu, fold; };
    std::vector<L> layers;
    layers.push_back({ n.stem.w, F, C, 9, 1, P.f_stem() });
    for (int i = 0; i < 2 * R; ++i) layers.push_back({ n.res[i].w, C, C, 9, 1, P.f_res(i) });
    layers.push_back({ n.pconv.w, C, KH_POLICY_MID, 1, 1, P.f_pconv() });
    layers.push_back({ n.p2w, KH_POLICY_MID, KH_POLICY_PLANES, 1, 0, P.f_p2() });
    layers.push_back({ n.vconv.w, C, 1, 1, 1, P.f_vconv() });
    size_t off = 0;
    for (const L& l : layers) {
        const int nw = l.taps * l.Ci * l.Co;
        // libtorch [Co][Ci][kh][kw] -> [tap][Ci][Co]
        copy_item(P, B_SIMPLE, off, CP_TRANSPOSE, l.w, {}, nw, nw, -1, l.Co, l.Ci, l.taps);
        copy_item(P, B_SIMPLE, off + nw, CP_COPY, nullptr, { l.fold, 0 }, l.Co, l.Co);
        copy_item(P, B_SIMPLE, off + nw + l.Co, CP_COPY, nullptr, { l.fold, 1 }, l.Co, l.Co);
        P.simple.push_back({ off, off + nw, off + nw + l.Co, l.Ci, l.Co, l.taps, l.relu });
        off += (size_t)nw + 2 * (size_t)l.Co;
    }
    copy_item(P, B_SIMPLE, off, CP_COPY, n.fcw, {}, KH_VALUE_WIDTH * 64, KH_VALUE_WIDTH * 64);
    P.simple_fcw = off; off += (size_t)KH_VALUE_WIDTH * 64;
    copy_item(P, B_SIMPLE, off, CP_COPY, n.fcb, {}, KH_VALUE_WIDTH, KH_VALUE_WIDTH);
    P.simple_fcb = off;
}

// the buffers of a set, by the engine's dtype and shape: the fp32 reference layers, the whole-network kernel's stream where
// it covers the shape, the per-layer kernels' fragments where it does not
int plan_set(const kh_engine* e, Plan& P, Weights& W, const HostNet& n)
{
    const int F = e->cfg.features, C = e->cfg.filters, R = e->cfg.residuals;
    int rc = KH_OK;
    P.dtype = e->cfg.dtype;
    plan_folds(P, n, C, R);
    if (e->cfg.dtype == KH_F32) {
        plan_simple(P, n, F, C, R);
        if (!e->f32_simple) rc = plan_layers(P, W, n, KH_F32, F, C, R);
    } else {
        if ((rc = plan_tower(P, W, n, F, C, R))) return rc;
        if (!W.tw_ok) rc = plan_layers(P, W, n, e->cfg.dtype, F, C, R);
    }
    // 64 lanes decode a fragment together (pack_decode): the padding rules above make every job whole fragments
    for (const PackJob& j : P.packs)
        if (!rc && j.groups % 64) rc = fail(KH_ERR_INVALID, "internal: a pack job of %u groups is not whole fragments", j.groups);
    return rc;
}

int alloc_buffers(Weights& W, const Plan& P)
{
    for (int b = 0; b < NBUF; ++b)
        if (P.bytes[b] && buf_of(W, b).ensure(P.bytes[b])) return KH_ERR_HIP;
    const float* dbase = W.simple.as<float>();
    for (const SimpleOff& s : P.simple) {
        kh::SimpleLayer L;
        L.wt = dbase + s.wt; L.scale = dbase + s.scale; L.shift = dbase + s.shift;
        L.Ci = s.Ci; L.Co = s.Co; L.taps = s.taps; L.relu = s.relu;
        W.layers.push_back(L);
    }
    if (!P.simple.empty()) { W.fcw = dbase + P.simple_fcw; W.fcb = dbase + P.simple_fcb; }
    return KH_OK;
}

// ------------------------------------------------------------------------------- the two packers
// Turns every job's (buffer, offset) and FoldRef into pointers against one memory — the folded arrays at `fold`, the
// buffers at `base` — and numbers the workgroups of the device packer's launches.  Job order is kept: find_job
// (weights_pack.hip) searches by block0.
void bind(Plan& P, float* fold, char* const base[NBUF])
{
    auto at = [&](FoldRef r) { return fold + P.fold_at(r); };
    for (size_t i = 0; i < P.folds.size(); ++i) { P.folds[i].scale = at({ (int)i, 0 }); P.folds[i].shift = at({ (int)i, 1 }); }
    for (PackJob& j : P.packs) {
        j.scale = j.fold < 0 ? nullptr : at({ j.fold, 0 });
        j.dst = base[j.buf] + j.off;
        j.block0 = P.pack_blocks;
        P.pack_blocks += (j.groups + PACK_THREADS - 1) / PACK_THREADS;
    }
    for (CopyJob& j : P.copies) {
        if (j.fsrc.item >= 0) j.src = at(j.fsrc);
        j.s = j.scale_of < 0 ? nullptr : at({ j.scale_of, 0 });
        j.dst = reinterpret_cast<float*>(base[j.buf]) + j.off;
        j.block0 = P.copy_blocks;
        P.copy_blocks += (j.npad + PACK_THREADS - 1) / PACK_THREADS;
    }
}

// one pack job on the host: a fragment decoded once, its 64 lanes emitted  (the job by value: no store aliases it)
void pack_job_host(const PackJob jb)
{
    for (unsigned frag = 0; frag < jb.groups / 64; ++frag) {
        const PackFrag f = pack_decode(jb, frag);
        if (jb.kind == PK_F32)
            for (int l = 0; l < 64; ++l) static_cast<float4*>(jb.dst)[frag * 64 + l] = pack_emit32(jb, f, l);
        else
            for (int l = 0; l < 64; ++l) static_cast<uint4*>(jb.dst)[frag * 64 + l] = pack_emit16(jb, f, l);
    }
}

// one copy job: a row decoded once, its elements emitted
void copy_job_host(const CopyJob jb)
{
    const unsigned len = copy_row_len(jb);
    for (unsigned i0 = 0; i0 < jb.npad; i0 += len) {
        const float* row = copy_decode(jb, i0 / len);
        for (unsigned x = 0; x < len; ++x) jb.dst[i0 + x] = copy_emit(jb, row, i0, x);
    }
}

int run_host(Weights& W, Plan& P)
{
    std::vector<float> fold(P.fold_floats());
    std::vector<char> host[NBUF];
    char* base[NBUF];
    for (int b = 0; b < NBUF; ++b) { host[b].assign(P.bytes[b], 0); base[b] = host[b].data(); }
    bind(P, fold.data(), base);
    for (const FoldJob& j : P.folds)
        for (int i = 0; i < j.co; ++i) fold_channel(j, i);
    {
        // the jobs run on a few host threads (a 20x256 net is 48 M fragments' worth)
        std::atomic<size_t> next{ 0 };
        auto run = [&]() {
            for (size_t j; (j = next.fetch_add(1)) < P.packs.size();) pack_job_host(P.packs[j]);
        };
        const int nt = P.threads ? (int)std::min<size_t>(8, P.packs.size()) : 1;
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(run);
        run();
        for (auto& t : th) t.join();
    }
    for (const CopyJob& j : P.copies) copy_job_host(j);
    int rc = alloc_buffers(W, P);
    if (rc) return rc;
    for (int b = 0; b < NBUF; ++b)
        if (P.bytes[b]) HIPCHK(hipMemcpy(buf_of(W, b).p, host[b].data(), P.bytes[b], hipMemcpyHostToDevice));
    return KH_OK;
}

// The jobs as tables in device memory and three launches on `st` (fold, pack, copy).  `scratch` (the folded arrays and
// the tables) and `tables` (their host source) must live until the stream has run them.
int run_device(Weights& W, Plan& P, hipStream_t st, DevMem& scratch, std::vector<char>& tables)
{
    int rc = alloc_buffers(W, P);
    if (rc) return rc;
    const size_t fold_bytes = (P.fold_floats() * 4 + 15) / 16 * 16;
    const size_t nf = P.folds.size() * sizeof(FoldJob), np = P.packs.size() * sizeof(PackJob), nc = P.copies.size() * sizeof(CopyJob);
    const size_t at_f = 0, at_p = (at_f + nf + 15) / 16 * 16, at_c = (at_p + np + 15) / 16 * 16;
    if (scratch.ensure(fold_bytes + at_c + nc)) return KH_ERR_HIP;
    char* base[NBUF];
    for (int b = 0; b < NBUF; ++b) base[b] = buf_of(W, b).as<char>();
    bind(P, scratch.as<float>(), base);
    tables.assign(at_c + nc, 0);
    memcpy(tables.data() + at_f, P.folds.data(), nf);
    memcpy(tables.data() + at_p, P.packs.data(), np);
    memcpy(tables.data() + at_c, P.copies.data(), nc);
    char* d_tab = scratch.as<char>() + fold_bytes;
    HIPCHK(hipMemcpyAsync(d_tab, tables.data(), tables.size(), hipMemcpyHostToDevice, st));
    HIPCHK(launch_fold(reinterpret_cast<const FoldJob*>(d_tab + at_f), (int)P.folds.size(), st));
    HIPCHK(launch_pack(reinterpret_cast<const PackJob*>(d_tab + at_p), (int)P.packs.size(), P.pack_blocks, st));
    HIPCHK(launch_copy(reinterpret_cast<const CopyJob*>(d_tab + at_c), (int)P.copies.size(), P.copy_blocks, st));
    return KH_OK;
}

void install(kh_engine* e, const std::shared_ptr<Weights>& W, std::shared_ptr<Weights>* installed)
{
    std::lock_guard<std::mutex> lk(e->wmu);
    e->weights = W;                  // calls in flight keep their own reference
    e->has_weights.store(true, std::memory_order_release);
    if (installed) *installed = W;
}

// Weights::ly_vshift travels as a kernel argument: the folded valueconv shift, from the host copy of the blob
void set_vshift(Weights& W, const HostNet& host)
{
    float vs;
    fold_channel(fold_job(host.vconv, 1, &vs, &W.ly_vshift), 0);
}

// what both ways of installing begin with: the blob's size checked, the engine's device current, a new set
int begin_install(kh_engine* e, const float* blob, size_t nfloats, int generation, int64_t bn_batches, std::shared_ptr<Weights>& W)
{
    if (!e || !blob) return fail(KH_ERR_INVALID, "null argument");
    const int F = e->cfg.features, C = e->cfg.filters, R = e->cfg.residuals;
    if (nfloats != kh_weight_count(F, C, R))
        return fail(KH_ERR_INVALID, "weight blob has %zu floats, expected %zu for F=%d C=%d R=%d",
                    nfloats, kh_weight_count(F, C, R), F, C, R);
    int rc = set_device(e);
    if (rc) return rc;
    W = std::make_shared<Weights>();
    W->generation = generation;
    W->bn_batches = bn_batches;
    return KH_OK;
}

}  // namespace

int load_weights_impl(kh_engine* e, const float* blob, size_t nfloats, int generation, int64_t bn_batches,
                      std::shared_ptr<Weights>* installed)
{
    std::shared_ptr<Weights> W;
    int rc = begin_install(e, blob, nfloats, generation, bn_batches, W);
    if (rc) return rc;
    const int F = e->cfg.features, C = e->cfg.filters, R = e->cfg.residuals;
    W->blob.assign(blob, blob + nfloats);
    const HostNet n = parse_blob(W->blob.data(), F, C, R);
    Plan P;
    if ((rc = plan_set(e, P, *W, n)) || (rc = run_host(*W, P))) return rc;
    set_vshift(*W, n);
    install(e, W, installed);
    return KH_OK;
}

int load_weights_device_impl(kh_engine* e, const float* d_blob, size_t nfloats, int generation, int64_t bn_batches,
                             hipStream_t stream, PinMem* pin, std::shared_ptr<Weights>* installed)
{
    std::shared_ptr<Weights> W;
    int rc = begin_install(e, d_blob, nfloats, generation, bn_batches, W);
    if (rc) return rc;
    const int F = e->cfg.features, C = e->cfg.filters, R = e->cfg.residuals;
    {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, d_blob) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != e->cfg.device) {
            (void)hipGetLastError();
            return fail(KH_ERR_INVALID, "d_blob is not device memory of device %d", e->cfg.device);
        }
        void* base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, const_cast<float*>(d_blob)) != hipSuccess) (void)hipGetLastError();
        else if (reinterpret_cast<const char*>(d_blob) + nfloats * 4 > static_cast<const char*>(base) + size)
            return fail(KH_ERR_INVALID, "d_blob: %zu floats do not fit its allocation", nfloats);
    }
    std::lock_guard<std::mutex> ld(e->ld_mu);         // one device install at a time: they share the staging below
    if (!pin) pin = &e->ld_pin;
    if (pin->ensure(nfloats * 4, true)) return KH_ERR_HIP;
    if (!e->ld_stream) HIPCHK(hipStreamCreateWithFlags(&e->ld_stream, hipStreamNonBlocking));
    if (!e->ld_copy) HIPCHK(hipStreamCreateWithFlags(&e->ld_copy, hipStreamNonBlocking));
    if (!e->ld_ready) HIPCHK(hipEventCreateWithFlags(&e->ld_ready, hipEventDisableTiming));
    hipStream_t st = stream ? stream : e->ld_stream;
    // the host copy (kh_get_weights, kh_clone, checkpoints, the trainer's next upload) comes down on a stream of its own,
    // behind what the caller queued on `st`, while the kernels pack
    HIPCHK(hipEventRecord(e->ld_ready, st));
    HIPCHK(hipStreamWaitEvent(e->ld_copy, e->ld_ready, 0));
    HIPCHK(hipMemcpyAsync(pin->p, d_blob, nfloats * 4, hipMemcpyDeviceToHost, e->ld_copy));
    Plan P;
    DevMem scratch;
    std::vector<char> tables;
    rc = plan_set(e, P, *W, parse_blob(d_blob, F, C, R));
    if (!rc) rc = run_device(*W, P, st, scratch, tables);
    // whatever happened, nothing of this call is left running on either stream when it returns
    const hipError_t ce = hipStreamSynchronize(e->ld_copy);
    if (!rc && ce == hipSuccess) {
        W->blob.assign(static_cast<const float*>(pin->p), static_cast<const float*>(pin->p) + nfloats);
        set_vshift(*W, parse_blob(W->blob.data(), F, C, R));
    }
    const hipError_t se = hipStreamSynchronize(st);
    if (rc) return rc;
    HIPCHK(ce);
    HIPCHK(se);
    install(e, W, installed);
    return KH_OK;
}

}  // namespace kh
