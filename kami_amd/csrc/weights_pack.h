// weights_pack.h — a parameter set's serving layouts, each written once.  The jobs below describe what goes where
// (weights.hip plans them); the __host__ __device__ functions are every layout's index map, BatchNorm fold and rounding.
// The host packer (weights.hip, run_host) and the device packer (weights_pack.hip) are loops and kernels over these same
// functions, so they write the same bits by construction; what is left to differ is how each side's compiler rounds
// (tests/test_gpu_weights_device.py).  A pack or a copy is split into what a fragment or a row shares (decoded once on the
// host, by every thread on the device) and one element of it; the functions are forced inline because the host loops'
// speed depends on it (out of line, a job's fields are reloaded and the fragment re-read for every lane).
#pragma once
#include "kh_internal.h"

namespace kh {

__host__ __device__ inline uint16_t f2bf16(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // keep NaN a NaN
    u += 0x7fffu + ((u >> 16) & 1u);                                            // round to nearest even
    return (uint16_t)(u >> 16);
}
__host__ __device__ inline uint16_t f2f16(float f)
{
    _Float16 h = (_Float16)f;
    uint16_t r;
    __builtin_memcpy(&r, &h, 2);
    return r;
}

// A job names its destination as (buffer, offset) and a folded input as a FoldRef; bind (weights.hip) turns both into
// pointers, against host staging or against device memory.  Pointers into the blob are only offset while planning.
struct FoldRef { int item = -1, shift = 0; };            // a folded layer's scale (shift = 0) or shift (1) array

// Eval-mode BatchNorm of one layer folded to an epilogue (scale[co], shift[co]):
//   bn(conv + bias) = conv * s + ((bias - mean) * s + beta),  s = gamma / sqrt(var + 1e-5)
// g == nullptr: a plain conv, scale 1, shift = b.
struct FoldJob {
    const float *b, *g, *be, *rm, *rv;
    float *scale, *shift;    // bound
    int co;
};
// channel i; the subtract, the multiply and the add are three roundings (no contraction: see weights_pack.hip)
__host__ __device__ __forceinline__ void fold_channel(const FoldJob& jb, int i)
{
    if (!jb.g) { jb.scale[i] = 1.0f; jb.shift[i] = jb.b[i]; return; }
    const float s = jb.g[i] / sqrtf(jb.rv[i] + 1e-5f);
    const float d = jb.b[i] - jb.rm[i];
    const float p = d * s;
    jb.scale[i] = s;
    jb.shift[i] = p + jb.be[i];
}

// One layer in one layout of MFMA A-operand fragments (v_mfma_f32_32x32x16: lane l = (r = l & 31, h = l >> 5) holds
// W[co = row tile + r][k = 8h + j], j = 0..7), BN scale folded in before the one rounding, rows >= Co and channels >= Ci
// zero.  A fragment is 64 lanes x one 16-byte group (eight 16-bit values or four floats); every job is whole fragments.
//   PK_STREAM  tower8_mfma.hip's ring — what the comments of tower_mfma.hip and tower_common.h call pack_layer:
//              fragments [tap][ks][ms] of (MS*32, KS*16), eight per 8 KB chunk of which the first `chunk_frags` are taken
//              from the layer and the rest, like every fragment past the layer's last, are zero.  ci0: first input channel
//              of this pass (the 33..128-plane stem runs as four 32-channel passes).  centre_first: 3x3 taps in the order
//              4,0,1,2,3,5,6,7,8.  perm: the first `perm` k-steps take their activations from the consumer's packed output
//              registers (tower_common.h, packed_fragments), which permutes their input channels.
//   PK_BLOCKS  layers_mfma.hip: [Co/CBC][CiP/64][tap][kk 0..3][ms < CBC/32][lane][8] — 64-channel slices of the reduction
//              outermost, then taps, then k-steps, so every kernel variant walks the same order and agrees bit for bit.
//              CBC: output channels per block, 64 (8 KB chunks of 64 x 64), 128 (conv4_mfma_kernel, tower128_kernel,
//              policy_head4_kernel: 32 x 128) or 256 (tower256_kernel: one k-step of eight row tiles per chunk).
//   PK_F32     conv_f32_kernel: [Co/64][Ci slices of <= 128][tap][j][ms 0..1][lane][4]; the lane holds
//              W[co][ci = 8j + 4h + 0..3]  (a slice is what fits LDS as an image).
enum { PK_STREAM = 0, PK_BLOCKS = 1, PK_F32 = 2 };
struct PackJob {
    const float* w;          // [Co][Ci][taps]
    int fold;                // the layer whose scale is folded in (-1: none)
    int buf; size_t off;     // destination: buffer and byte offset
    const float* scale;      // bound; nullptr: 1
    void* dst;               // bound
    unsigned groups;         // 16-byte groups this job writes, padding included
    unsigned block0;         // bound: first workgroup of this job in the launch
    int kind, dtype, Co, Ci, taps;
    int KS, MS, ci0, centre_first, perm, chunk_frags;    // PK_STREAM
    int CiP, CBC;                                        // PK_BLOCKS, PK_F32
};

// what the 64 lanes of one fragment share
struct PackFrag {
    int tap, ks, co0;        // ks: k-step of 16 input channels (PK_F32: j, 8 input channels); co0: first row of the tile
    bool live, permuted;     // !live: padding, all zero
};
__host__ __device__ __forceinline__ PackFrag pack_decode(const PackJob& jb, unsigned frag)
{
    PackFrag f{ 0, 0, 0, true, false };
    if (jb.kind == PK_STREAM) {
        const unsigned chunk = frag >> 3, fi = frag & 7;
        const unsigned sf = chunk * jb.chunk_frags + fi;
        f.live = (int)fi < jb.chunk_frags && sf < (unsigned)(jb.taps * jb.KS * jb.MS);
        const int ti = sf / (jb.KS * jb.MS), ms = sf % jb.MS;
        f.ks = (sf / jb.MS) % jb.KS;
        f.tap = !jb.centre_first ? ti : (ti == 0 ? 4 : (ti <= 4 ? ti - 1 : ti));
        f.permuted = ti * jb.KS + f.ks < jb.perm;
        f.co0 = ms * 32;
    } else if (jb.kind == PK_BLOCKS) {
        const int M = jb.CBC / 32, slices = jb.CiP / 64;
        unsigned t = frag;
        const int ms = t % M; t /= M;
        const int kk = t & 3; t >>= 2;
        f.tap = t % jb.taps; t /= jb.taps;
        const int slice = t % slices, cb = t / slices;
        f.ks = slice * 4 + kk;
        f.co0 = cb * jb.CBC + ms * 32;
    } else {
        const unsigned per_cb = (unsigned)jb.taps * (jb.CiP / 8) * 2, full = (unsigned)jb.taps * 16 * 2;
        const int cb = frag / per_cb;
        unsigned t = frag % per_cb;
        const int slice = t / full;
        t -= slice * full;
        const int len8 = (jb.CiP - 128 * slice < 128 ? jb.CiP - 128 * slice : 128) / 8;
        f.tap = t / (len8 * 2);
        t %= len8 * 2;
        f.ks = slice * 16 + (t >> 1);
        f.co0 = cb * 64 + (t & 1) * 32;
    }
    return f;
}

// A lane's row of the layer: tap `tap` of W[co][0 .. Ci), times the channel's scale; a row past the layer's last is zero.
struct PackRow { const float* w; float sc; int Ci, stride; };
__host__ __device__ __forceinline__ PackRow pack_row(const PackJob& jb, bool live, int co, int tap)
{
    if (!live || co >= jb.Co) return { jb.w, 0.0f, 0, 0 };
    return { jb.w + (size_t)co * jb.Ci * jb.taps + tap, jb.scale ? jb.scale[co] : 1.0f, jb.Ci, jb.taps };
}
__host__ __device__ __forceinline__ float pack_value(const PackRow& r, int ci)
{
    return ci < r.Ci ? r.w[(size_t)ci * r.stride] * r.sc : 0.0f;
}
// the lane's group of a 16-bit layout
__host__ __device__ __forceinline__ uint4 pack_emit16(const PackJob& jb, const PackFrag& f, int lane)
{
    const int h = lane >> 5;
    const PackRow r = pack_row(jb, f.live, f.co0 + (lane & 31), f.tap);
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = jb.ci0 + (f.permuted ? 32 * (f.ks >> 1) + 8 * (2 * (f.ks & 1) + (j >> 2)) + 4 * h + (j & 3)
                                            : f.ks * 16 + 8 * h + j);
        const float v = pack_value(r, ci);
        o[j] = jb.dtype == KH_BF16 ? f2bf16(v) : f2f16(v);
    }
    uint4 q;
    q.x = o[0] | o[1] << 16;
    q.y = o[2] | o[3] << 16;
    q.z = o[4] | o[5] << 16;
    q.w = o[6] | o[7] << 16;
    return q;
}
// the lane's group of PK_F32
__host__ __device__ __forceinline__ float4 pack_emit32(const PackJob& jb, const PackFrag& f, int lane)
{
    const int ci = f.ks * 8 + 4 * (lane >> 5);
    const PackRow r = pack_row(jb, true, f.co0 + (lane & 31), f.tap);
    float4 v;
    v.x = pack_value(r, ci + 0);
    v.y = pack_value(r, ci + 1);
    v.z = pack_value(r, ci + 2);
    v.w = pack_value(r, ci + 3);
    return v;
}

// Folded parameters and re-laid fp32 tensors, a float at a time.  A job is rows of copy_row_len elements that share
// their place in the source (copy_decode); copy_emit reads one of them.
//   CP_COPY dst[i] = src[i]    CP_MULS dst[i] = src[i] * s[0]    (one row)
//   CP_FC4  valuefc.weight [256][64] -> [k/4][j][4]: thread j reads coalesced float4 (tower8_kernel; policy_head4_kernel /
//           tower128_kernel's value FC, where from the [256][64] rows every lane's 16 bytes were a cache line of their own)
//   CP_TRANSPOSE  libtorch [Co][Ci][taps] -> [taps][Ci][Co]; a row is one (tap, ci)
enum { CP_COPY = 0, CP_MULS = 1, CP_FC4 = 2, CP_TRANSPOSE = 3 };
struct CopyJob {
    const float* src;        // blob floats; bound to the folded array when fsrc names one
    FoldRef fsrc;
    int scale_of;            // CP_MULS: the layer whose scale[0] multiplies (-1: none)
    int buf; size_t off;     // destination: buffer and float offset
    const float* s;          // bound
    float* dst;              // bound
    unsigned n, npad;        // dst[n .. npad) = 0
    unsigned block0;         // bound
    int kind, Co, Ci, taps;
};
__host__ __device__ __forceinline__ unsigned copy_row_len(const CopyJob& jb)
{
    return jb.kind == CP_TRANSPOSE ? jb.Co : jb.kind == CP_FC4 ? 4 * KH_VALUE_WIDTH : jb.npad;
}
__host__ __device__ __forceinline__ const float* copy_decode(const CopyJob& jb, unsigned row)
{
    if (jb.kind == CP_TRANSPOSE) return jb.src + (row % jb.Ci) * (size_t)jb.taps + row / jb.Ci;
    return jb.src + (jb.kind == CP_FC4 ? 4 * row : 0);
}
// element x of the row that starts at dst[i0]
__host__ __device__ __forceinline__ float copy_emit(const CopyJob& jb, const float* row, unsigned i0, unsigned x)
{
    if (i0 + x >= jb.n) return 0.0f;
    if (jb.kind == CP_COPY) return row[x];
    if (jb.kind == CP_MULS) return row[x] * jb.s[0];
    if (jb.kind == CP_FC4) return row[(size_t)(x >> 2) * 64 + (x & 3)];
    return row[(size_t)x * jb.Ci * jb.taps];
}

constexpr int PACK_THREADS = 256;

// the three launches of one device install, in this order on `s`; the tables are device memory, sorted by block0
hipError_t launch_fold(const FoldJob* d_jobs, int njobs, hipStream_t s);
hipError_t launch_pack(const PackJob* d_jobs, int njobs, unsigned blocks, hipStream_t s);
hipError_t launch_copy(const CopyJob* d_jobs, int njobs, unsigned blocks, hipStream_t s);

}  // namespace kh
