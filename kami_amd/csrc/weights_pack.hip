// weights_pack.hip — the device packer: three kernels that run a parameter set's jobs (weights_pack.h) on a canonical
// fp32 blob in device memory.  The layouts, the fold and the roundings are weights_pack.h's functions, the ones the host
// packer loops over; here a thread folds one channel, or decodes its fragment and stores its lane's 16-byte group whole,
// or writes one float.  Padding (rows >= Co, channels >= Ci, empty fragments, the parity chunk) is written as zeros,
// never assumed.
//
// This file is compiled with -ffp-contract=off (kami_amd/build.py): the host folds BatchNorm with a subtract, a
// multiply and an add, and a fused multiply-add here would change the last bit of a shift.  `/` and sqrtf are
// correctly rounded in device code.
#include "weights_pack.h"

namespace kh {
namespace {

__global__ void __launch_bounds__(PACK_THREADS) fold_kernel(const FoldJob* __restrict__ jobs)
{
    const FoldJob jb = jobs[blockIdx.x];
    for (int i = threadIdx.x; i < jb.co; i += PACK_THREADS) fold_channel(jb, i);
}

// the job whose block range holds `block`: jobs are sorted by block0
template <class J> __device__ inline int find_job(const J* jobs, int njobs, unsigned block)
{
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(PACK_THREADS) pack_kernel(const PackJob* __restrict__ jobs, int njobs)
{
    const PackJob& jb = jobs[find_job(jobs, njobs, blockIdx.x)];
    const unsigned g = (blockIdx.x - jb.block0) * PACK_THREADS + threadIdx.x;
    if (g >= jb.groups) return;
    const PackFrag f = pack_decode(jb, g >> 6);
    if (jb.kind == PK_F32) static_cast<float4*>(jb.dst)[g] = pack_emit32(jb, f, g & 63);
    else static_cast<uint4*>(jb.dst)[g] = pack_emit16(jb, f, g & 63);
}

__global__ void __launch_bounds__(PACK_THREADS) copy_kernel(const CopyJob* __restrict__ jobs, int njobs)
{
    const CopyJob& jb = jobs[find_job(jobs, njobs, blockIdx.x)];
    const unsigned i = (blockIdx.x - jb.block0) * PACK_THREADS + threadIdx.x;
    if (i >= jb.npad) return;
    const unsigned len = copy_row_len(jb), row = i / len;
    jb.dst[i] = copy_emit(jb, copy_decode(jb, row), row * len, i - row * len);
}

}  // namespace

hipError_t launch_fold(const FoldJob* d_jobs, int njobs, hipStream_t s)
{
    if (njobs > 0) hipLaunchKernelGGL(fold_kernel, dim3(njobs), dim3(PACK_THREADS), 0, s, d_jobs);
    return hipGetLastError();
}
hipError_t launch_pack(const PackJob* d_jobs, int njobs, unsigned blocks, hipStream_t s)
{
    if (blocks > 0) hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(PACK_THREADS), 0, s, d_jobs, njobs);
    return hipGetLastError();
}
hipError_t launch_copy(const CopyJob* d_jobs, int njobs, unsigned blocks, hipStream_t s)
{
    if (blocks > 0) hipLaunchKernelGGL(copy_kernel, dim3(blocks), dim3(PACK_THREADS), 0, s, d_jobs, njobs);
    return hipGetLastError();
}

}  // namespace kh
