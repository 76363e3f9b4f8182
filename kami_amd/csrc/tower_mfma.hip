// tower_mfma.hip — the throughput path for nets of up to 64 filters: the WHOLE network forward (kami/nn/nn.cpp:59-91) as
// ONE persistent gfx950 kernel, tower8_kernel in tower8_mfma.hip (launcher: launch_tower there).  bf16 or f16 operands,
// fp32 accumulation on the matrix cores (v_mfma_f32_32x32x16_{bf16,f16}).  This file is the overview of that path and
// its LDS budget; geometry and the device helpers are in tower_common.h.
//
// Why one kernel: at batch 512 the 6x64 net is only ~35 GFLOP — ~14 us at the MFMA peak — so a launch per layer (13 conv
// layers + heads, ~1.5 us per dependent boundary) would cost more than the arithmetic.  Instead one workgroup owns TW_NB
// boards for the whole forward pass:
//
//   HBM  --fp32 planes-->  LDS S (T = bf16/f16, 10x12 zero-haloed pixel grid per board)
//   stem 3x3 conv S -> X, then per residual block  X -conv1-> T,  T -conv2(+X)-> X   (all in LDS)
//   heads: value 1x1 + FC + tanh (VALU), policy 1x1 -> P (registers), policy 1x1 -> logits L, softmax -> HBM
//
// Activations never leave the CU.  Each 3x3 conv is an implicit GEMM  D[co][pixel] = sum_k W[co][k] * X[k][pixel],
// k = (tap, ci): weights are the MFMA A operand, pre-packed on the host in exact fragment order (pack_layer in
// kh_api.hip); activations are the B operand, read straight from the pixel-major LDS image (one ds_read_b128 per lane
// per 16-channel k-step, tap shifts are immediates).  Output channels land 4-consecutive per lane, so the epilogue
// (ReLU, +skip, convert) writes 8-byte packed groups back to LDS.  BatchNorm (eval) is folded: scale into the weights
// before rounding, shift into the accumulator's initial value.
//
// LDS layout (byte offsets, tower_common.h):  [0, LDS_X) the weight ring, RING_D slots of 8 KB  |  [LDS_X, LDS_ST) X,
// TW_NB images of XSTR = 2*64 + 16 bytes per pixel  |  [LDS_ST, +st_size(FP)) S (the input planes, FP padded channels),
// later T  |  then the parameter block (tower_par_floats: folded shifts, policy bias, value conv, scratch).  The logits
// L start at LDS_X and run on into S.
//
// Weights (~1 MB for 6x64, L2 resident) stream through the ring by LDS-DMA (global_load_lds_dwordx4) as a cyclic
// sequence of 8 KB chunks, one workgroup barrier per chunk, so the prefetch runs across layer and board-group boundaries.
// The stream's order is the kernel's walk: the stem (F <= 32: padded to 32 planes; 33..128: four unpadded passes of 32
// planes, 18 chunks), the 2R 3x3 layers centre tap first, policyconv, policyconv2, and a zero chunk when the count is odd.
//
// LDS bank conflicts: pixel stride = 2*C + 16 bytes and row pitch 12, with the lane->pixel map PIXMAP chosen so that
// every 16-lane group of a ds_read_b128 touches 16 distinct 16-byte slots for every tap (MI355X_MICROARCH.md §LDS:
// groups {0-3,12-15,20-27}, {4-11,16-19,28-31}).
#include "tower_common.h"

namespace kh {

int tower_lds_bytes(int FP, int R)
{
    return LDS_ST + st_size(FP) + tower_par_floats(R) * 4;
}

}  // namespace kh
