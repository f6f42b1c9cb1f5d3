// gather.hip -- row gather / scatter-add over the neighbor table (NeuralPoints.forward's index_select and its backward) and the flags of the
// point rows a table touches.
#include "mlp_common.h"

namespace {
constexpr int TPB = 256;

__global__ __launch_bounds__(TPB) void k_gather_rows(const float *__restrict__ src, int n_src, int width, const int *__restrict__ idx,
                                                     long long n_idx, float *__restrict__ dst) {
    const long long total = n_idx * width;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += (long long)gridDim.x * TPB) {
        const long long i = e / width;
        const int c = (int)(e - i * width);
        int p = idx[i];
        p = p < 0 ? 0 : (p >= n_src ? n_src - 1 : p);         // torch.clamp(sample_pidx, min=0)  neural_points.py:708
        dst[e] = src[(long long)p * width + c];
    }
}
// width a multiple of 4 with width / 4 a power of two <= 64 (the embedding: 32 floats = 8 lanes x 16 bytes per row): a group of W4 lanes copies one
// row with 16-byte accesses, no per-element division.  (Round 3's 4.2 TB/s for this kernel came from the loop vectoriser, which the library has
// had switched off since round 4 -- the packed-fp32 fault, csrc/Makefile --: the scalar form above fell to 3.1 TB/s; profiles/r0[345]_microbench.json.)
template <int W4>
__global__ __launch_bounds__(TPB) void k_gather_rows_v4(const float4 *__restrict__ src, int n_src, const int *__restrict__ idx, long long n_idx, float4 *__restrict__ dst) {
    const int c = threadIdx.x & (W4 - 1);
    for (long long i = ((long long)blockIdx.x * TPB + threadIdx.x) / W4; i < n_idx; i += (long long)gridDim.x * (TPB / W4)) {
        int p = idx[i];
        p = p < 0 ? 0 : (p >= n_src ? n_src - 1 : p);
        const float4 v = src[(long long)p * W4 + c];
        pn_f4 t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<pn_f4 *>(dst + i * W4 + c));
    }
}
// -1 slots were gathered from point 0 (A.9 of SURVEY.md: the reference lets point 0 collect gradient from every
// empty slot).  Those are the vast majority of the slots, all hitting ONE row: they are summed per block in LDS
// first and leave as one atomic per column per block; real indices go straight to global atomics.
__global__ __launch_bounds__(TPB) void k_scatter_add_rows(const float *__restrict__ grad_rows, const int *__restrict__ idx, long long n_idx,
                                                          int width, float *__restrict__ grad_src, int n_src) {
    __shared__ float row0[64];
    const bool use_lds = width <= 64;
    if (use_lds && threadIdx.x < 64) row0[threadIdx.x] = 0.f;
    __syncthreads();
    const long long total = n_idx * width;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += (long long)gridDim.x * TPB) {
        const long long i = e / width;
        const int c = (int)(e - i * width);
        int p = idx[i];
        const float g = grad_rows[e];
        if (p <= 0 && use_lds) { atomicAdd(&row0[c], g); continue; }
        p = p < 0 ? 0 : (p >= n_src ? n_src - 1 : p);
        atomicAdd(&grad_src[(long long)p * width + c], g);
    }
    __syncthreads();
    if (use_lds && threadIdx.x < width && row0[threadIdx.x] != 0.f) atomicAdd(&grad_src[threadIdx.x], row0[threadIdx.x]);
}

// flags[p] = 1 for every point p that occurs in the neighbor table, flags[0] = 1 if any slot is empty (empty slots read point 0 like the
// reference, neural_points.py:709, and the zero-one regulariser differentiates through that read): the rows a rank's point gradients can be
// non-zero in -- what a data-parallel caller exchanges instead of the dense [N, 39] gradient (pointnerf_amd/dist.py).  Plain stores of the
// same value race benignly; the table is read as int4 where it can be.
__global__ __launch_bounds__(256) void k_touched_flags(const int *__restrict__ pidx, long long n, int n_points, int *__restrict__ flags) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int p = pidx[i];
        if (p >= 0 && p < n_points) flags[p] = 1;
        else if (p < 0) flags[0] = 1;
    }
}
}  // namespace

extern "C" int pnerf_gather_rows(const float *d_src, int n_src, int width, const int32_t *d_idx, int64_t n_idx, float *d_dst, void *stream) {
    if (n_idx == 0) return 0;                      // nothing to gather (a chunk of rays that hit nothing): pointers may be null
    if (!d_src || !d_idx || !d_dst || n_src <= 0 || width <= 0 || n_idx < 0) return PNERF_E_INVAL;
    long long total = n_idx * width;
    int grid = (int)((total + TPB - 1) / TPB < 16384 ? (total + TPB - 1) / TPB : 16384);
    PnProfScope prof(PNK_GATHER, (hipStream_t)stream);
    const bool al = ((uintptr_t)d_src % 16 == 0) && ((uintptr_t)d_dst % 16 == 0);
    const long long rows_per_block = TPB / (width / 4 > 0 ? width / 4 : 1);
    const int gridv = (int)((n_idx + rows_per_block - 1) / rows_per_block < 16384 ? (n_idx + rows_per_block - 1) / rows_per_block : 16384);
    if (al && width == 32) hipLaunchKernelGGL(k_gather_rows_v4<8>, dim3(gridv), dim3(TPB), 0, (hipStream_t)stream, (const float4 *)d_src, n_src, d_idx, (long long)n_idx, (float4 *)d_dst);
    else if (al && width == 4) hipLaunchKernelGGL(k_gather_rows_v4<1>, dim3(gridv), dim3(TPB), 0, (hipStream_t)stream, (const float4 *)d_src, n_src, d_idx, (long long)n_idx, (float4 *)d_dst);
    else hipLaunchKernelGGL(k_gather_rows, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, d_src, n_src, width, d_idx, (long long)n_idx, d_dst);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_scatter_add_rows(const float *d_grad_rows, const int32_t *d_idx, int64_t n_idx, int width, float *d_grad_src, int n_src, void *stream) {
    if (n_idx == 0) return 0;
    if (!d_grad_rows || !d_idx || !d_grad_src || n_src <= 0 || width <= 0 || n_idx < 0) return PNERF_E_INVAL;
    long long total = n_idx * width;
    int grid = (int)((total + TPB - 1) / TPB < 4096 ? (total + TPB - 1) / TPB : 4096);
    PnProfScope prof(PNK_GATHER, (hipStream_t)stream);
    hipLaunchKernelGGL(k_scatter_add_rows, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, d_grad_rows, d_idx, (long long)n_idx, width, d_grad_src, n_src);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_touched_flags(const int32_t *d_pidx, int64_t n, int32_t n_points, int32_t *d_flags, void *stream) {
    if (n < 0 || n_points < 0 || (n > 0 && !d_pidx) || (n_points > 0 && !d_flags)) return PNERF_E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n_points == 0) return 0;
    if (hipMemsetAsync(d_flags, 0, (size_t)n_points * sizeof(int32_t), s) != hipSuccess) return PNERF_E_LAUNCH;
    if (n == 0) return 0;
    const long long blocks = (n + 255) / 256;
    PnProfScope prof(PNK_GATHER, s);
    hipLaunchKernelGGL(k_touched_flags, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, d_pidx, (long long)n, n_points, d_flags);
    PN_CHECK_LAUNCH();
    return 0;
}
