// cloudinit.hip -- from a point cloud the user already has (COLMAP, a sensor, both merged) to per-view groups of neural-point positions:
// the reference's `--load_points 1/2/3` route (run/train_ft.py:642-735) between "a cloud" and the per-view query_embedding loop.  Replaces
//   nearest_view                                                   run/train_ft.py:39-48     (k_nearest_view)
//   construct_vox_points_ind x 2 + the occupancy mask              run/train_ft.py:657-669, models/mvs/mvs_utils.py:520-534
//                                                                                            (k_occ_set / k_occ_test)
//   the crop to opt.ranges                                         run/train_ft.py:675-680   (k_crop_flag)
//   torch.unique(cam_ind) + one boolean index per view             run/train_ft.py:707-710   (k_group_rank / k_group_place / k_group_offsets)
// k_nearest_view: the reference scores N x M (point, camera) pairs in 10 000-point slices that each materialise [10000, M, 3] temporaries;
// here one thread owns a point and the loop over the cameras runs inside it.  The camera records (position + centre ray, 6 floats) are
// staged through LDS NV_CHUNK at a time (any M), every lane reads the same record (a broadcast); 12 B read and 4 B written per point.
// Bit-reproducible: no atomics, no temporaries.  One division (of the dot product) where the reference divides the three components, and
// norm * 0.005f for norm / 200: tests/cloudinit_case.py holds the result to the float64 argmin on every point whose runner-up is farther
// than the reference's own fp32 deviation allows.
// Occupancy merge: a res^3-bit bitmap set from cloud A (atomic OR on words: the result does not depend on the order), tested by cloud B.
// Merge and crop end in scan.hip's compaction (ascending index = the order of the reference's boolean indexing) and a row gather.
// Grouping: a stable counting sort without an atomic.  A block ranks GB_CHUNK points among the earlier points OF ITS OWN CHUNK with the
// same view (the chunk's views sit in LDS, every lane reads the same word), the last point of a view in the chunk writes the chunk's count
// of that view into a [M, blocks] table, one exclusive scan over the table (view-major) gives every (view, block) its first position.
// fp32, no FMA contraction (built with -ffp-contract=off): the cell arithmetic rounds as the reference's does.
#include "pn_common.h"

namespace {
constexpr int NV_TPB = 256;
constexpr int NV_CHUNK = 256;          // camera records per LDS stage (8 KB)

__global__ __launch_bounds__(NV_TPB) void k_nearest_view(const float *__restrict__ xyz, long long n, const float *__restrict__ campos,
                                                         const float *__restrict__ camdir, int M, int *__restrict__ cam_ind) {
    __shared__ float4 rec[2 * NV_CHUNK];
    const long long i = (long long)blockIdx.x * NV_TPB + threadIdx.x;
    const bool live = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) { px = xyz[3 * i]; py = xyz[3 * i + 1]; pz = xyz[3 * i + 2]; }
    float best = __int_as_float(0x7f800000);
    int arg = 0;
    for (int base = 0; base < M; base += NV_CHUNK) {
        const int cnt = min(NV_CHUNK, M - base);
        __syncthreads();
        for (int c = threadIdx.x; c < cnt; c += NV_TPB) {
            const float *cp = campos + 3 * (long long)(base + c), *cd = camdir + 3 * (long long)(base + c);
            rec[2 * c] = make_float4(cp[0], cp[1], cp[2], 0.f);
            rec[2 * c + 1] = make_float4(cd[0], cd[1], cd[2], 0.f);
        }
        __syncthreads();
        if (live)
            for (int c = 0; c < cnt; ++c) {
                const float4 a = rec[2 * c], r = rec[2 * c + 1];
                const float dx = px - a.x, dy = py - a.y, dz = pz - a.z;                                    // :43
                const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz);                                     // :44
                const float dot = (dx * r.x + dy * r.y) + dz * r.z;                                         // :45-46, divided once
                const float s = nrm * 0.005f + (1.1f - dot / (nrm + 1e-6f));                                // :46
                if (s < best) { best = s; arg = base + c; }                                                 // :47 ties: the lowest camera (a NaN score never wins)
            }
    }
    if (live) cam_ind[i] = arg;
}

// ---- occupancy merge and crop ----------------------------------------------------------------------------------------------------------
struct OccArgs { float mn[3], va[3], vb[3]; int res; };

__device__ __forceinline__ long long occ_key(const float *__restrict__ p, const float *mn, const float *vs, int res) {
    const int cx = pn_cell(p[0], mn[0], vs[0]), cy = pn_cell(p[1], mn[1], vs[1]), cz = pn_cell(p[2], mn[2], vs[2]);
    if (cx < 0 || cy < 0 || cz < 0 || cx >= res || cy >= res || cz >= res) return -1;
    return ((long long)cx * res + cy) * res + cz;
}

__global__ void k_occ_set(const float *__restrict__ a_xyz, long long na, OccArgs g, unsigned *__restrict__ bits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= na) return;
    const long long k = occ_key(a_xyz + 3 * i, g.mn, g.va, g.res);
    if (k >= 0) atomicOr(&bits[k >> 5], 1u << (k & 31));
}

__global__ void k_occ_test(const float *__restrict__ b_xyz, long long nb, OccArgs g, const unsigned *__restrict__ bits, int *__restrict__ flags,
                           unsigned char *__restrict__ mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const long long k = occ_key(b_xyz + 3 * i, g.mn, g.vb, g.res);
    const int keep = (k < 0 || !((bits[k >> 5] >> (k & 31)) & 1u)) ? 1 : 0;                               // a cell outside the grid holds no point of A
    flags[i] = keep;
    mask[i] = (unsigned char)keep;
}

struct CropArgs { float r[6]; };
__global__ void k_crop_flag(const float *__restrict__ xyz, long long n, CropArgs g, int *__restrict__ flags, unsigned char *__restrict__ mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int keep = 1;
    for (int j = 0; j < 3; ++j) keep &= (xyz[3 * i + j] >= g.r[j] && xyz[3 * i + j] <= g.r[3 + j]) ? 1 : 0;      // :677-679 (NaN fails)
    flags[i] = keep;
    mask[i] = (unsigned char)keep;
}

__global__ void k_take_rows(const float *__restrict__ src, const int *__restrict__ list, const int *__restrict__ count, long long n,
                            float *__restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n || t >= *count) return;
    const long long i = list[t];
    out[3 * t] = src[3 * i]; out[3 * t + 1] = src[3 * i + 1]; out[3 * t + 2] = src[3 * i + 2];
}

constexpr long long SEL_MAX = 0x7fffff00LL;      // rows whose indices and counts fit scan.hip's int32
struct SelLayout { size_t flags, list, scan, bits, total; };
SelLayout sel_layout(long long n, long long cells) {
    PnCarver cv(nullptr);
    SelLayout L;
    const size_t m = (size_t)(n > 0 ? n : 1);
    L.flags = cv.off; cv.take<int>(m);
    L.list = cv.off; cv.take<int>(m);
    L.scan = cv.off; cv.take<int>(pn_scan_scratch_ints(n));
    L.bits = cv.off; cv.take<unsigned>((size_t)((cells + 31) / 32));
    L.total = cv.off;
    return L;
}
// flags -> ascending list -> rows
int sel_finish(const float *src, long long n, const SelLayout &L, char *ws, float *out, int *d_count, hipStream_t s) {
    int *flags = (int *)(ws + L.flags), *list = (int *)(ws + L.list), *scan = (int *)(ws + L.scan);
    const int rc = pn_compact_gt0_i32(flags, n, list, d_count, scan, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_take_rows, dim3(pn_cdiv(n, 256)), dim3(256), 0, s, src, list, d_count, n, out);
    PN_CHECK_LAUNCH();
    return 0;
}

// ---- grouping ----------------------------------------------------------------------------------------------------------------------------
constexpr int GB_TPB = 256, GB_EPT = 4, GB_CHUNK = GB_TPB * GB_EPT;

__global__ __launch_bounds__(GB_TPB) void k_group_rank(const int *__restrict__ cam_ind, long long n, int M, int nblk, int *__restrict__ rank,
                                                       int *__restrict__ hist) {
    __shared__ int lv[GB_CHUNK];
    const long long base = (long long)blockIdx.x * GB_CHUNK;
    const int cnt = (int)min((long long)GB_CHUNK, n - base);
    int my[GB_EPT], r[GB_EPT], c[GB_EPT];
#pragma unroll
    for (int k = 0; k < GB_EPT; ++k) {
        const int q = k * GB_TPB + threadIdx.x;
        int v = -1;
        if (q < cnt) {
            v = cam_ind[base + q];
            if (v < 0 || v >= M) v = -1;                      // not a view: left out (the caller sees offsets[M] < n)
        }
        lv[q] = v; my[k] = v; r[k] = 0; c[k] = 0;
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
        const int w = lv[j];
#pragma unroll
        for (int k = 0; k < GB_EPT; ++k) {
            const int eq = w == my[k] ? 1 : 0;
            c[k] += eq;
            r[k] += eq & (j < k * GB_TPB + (int)threadIdx.x ? 1 : 0);
        }
    }
#pragma unroll
    for (int k = 0; k < GB_EPT; ++k) {
        if (my[k] < 0) continue;
        rank[base + k * GB_TPB + threadIdx.x] = r[k];
        if (r[k] == c[k] - 1) hist[(long long)my[k] * nblk + blockIdx.x] = c[k];      // the chunk's last point of this view: one writer
    }
}

__global__ void k_group_place(const int *__restrict__ cam_ind, long long n, int M, int nblk, const int *__restrict__ rank,
                              const int *__restrict__ start, long long *__restrict__ order) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = cam_ind[i];
    if (v < 0 || v >= M) return;
    order[(long long)start[(long long)v * nblk + i / GB_CHUNK] + rank[i]] = i;
}

__global__ void k_group_offsets(const int *__restrict__ start, int M, int nblk, long long *__restrict__ offsets) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v <= M) offsets[v] = start[(long long)v * nblk];        // start[M * nblk] = the scan's total
}

struct GroupLayout { size_t hist, start, rank, scan, total; long long cells; int nblk; };
GroupLayout group_layout(long long n, int M) {
    PnCarver cv(nullptr);
    GroupLayout L;
    L.nblk = pn_cdiv(n > 0 ? n : 1, GB_CHUNK);
    L.cells = (long long)M * L.nblk;
    L.hist = cv.off; cv.take<int>((size_t)L.cells + 1);
    L.start = cv.off; cv.take<int>((size_t)L.cells + 2);
    L.rank = cv.off; cv.take<int>((size_t)(n > 0 ? n : 1));
    L.scan = cv.off; cv.take<int>(pn_scan_scratch_ints(L.cells));
    L.total = cv.off;
    return L;
}
bool group_fits(long long n, int M) { return n >= 0 && M >= 1 && n <= SEL_MAX && (long long)M * pn_cdiv(n > 0 ? n : 1, GB_CHUNK) <= SEL_MAX; }
}  // namespace

extern "C" int pnerf_nearest_view(const float *d_xyz, int64_t n, const float *d_campos, const float *d_camdir, int M, int32_t *d_cam_ind,
                                  void *stream) {
    if (M < 1 || n < 0) return PNERF_E_INVAL;
    if (n == 0) return 0;
    if (!d_xyz || !d_campos || !d_camdir || !d_cam_ind) return PNERF_E_INVAL;
    if (n / NV_TPB >= 0x7fffffffLL) return PNERF_E_UNSUP;
    hipLaunchKernelGGL(k_nearest_view, dim3(pn_cdiv(n, NV_TPB)), dim3(NV_TPB), 0, (hipStream_t)stream, d_xyz, (long long)n, d_campos, d_camdir, M,
                       d_cam_ind);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t pnerf_occupancy_merge_workspace_bytes(int64_t nb, int res) {
    if (nb < 0 || nb > SEL_MAX || res < 1 || (long long)res * res * res > SEL_MAX) return 0;
    return sel_layout(nb, (long long)res * res * res).total;
}

extern "C" int pnerf_occupancy_merge(const float *d_a_xyz, int64_t na, const float *d_b_xyz, int64_t nb, const float *space_min3_host,
                                     const float *vox_size_a3_host, const float *vox_size_b3_host, int res, float *d_kept_xyz, int32_t *d_count,
                                     uint8_t *d_mask, void *d_ws, size_t ws_bytes, void *stream) {
    if (na < 0 || nb < 0 || res < 1 || !space_min3_host || !vox_size_a3_host || !vox_size_b3_host || !d_count) return PNERF_E_INVAL;
    if (nb > SEL_MAX || (long long)res * res * res > SEL_MAX || na / 256 >= 0x7fffffffLL) return PNERF_E_UNSUP;
    hipStream_t s = (hipStream_t)stream;
    if (nb == 0) return hipMemsetAsync(d_count, 0, sizeof(int), s) == hipSuccess ? 0 : PNERF_E_LAUNCH;
    if ((na > 0 && !d_a_xyz) || !d_b_xyz || !d_kept_xyz || !d_mask || !d_ws) return PNERF_E_INVAL;
    const long long cells = (long long)res * res * res;
    const SelLayout L = sel_layout(nb, cells);
    if (ws_bytes < L.total) return PNERF_E_WS;
    OccArgs g;
    for (int j = 0; j < 3; ++j) { g.mn[j] = space_min3_host[j]; g.va[j] = vox_size_a3_host[j]; g.vb[j] = vox_size_b3_host[j]; }
    g.res = res;
    char *ws = (char *)d_ws;
    unsigned *bits = (unsigned *)(ws + L.bits);
    if (hipMemsetAsync(bits, 0, (size_t)((cells + 31) / 32) * 4, s) != hipSuccess) return PNERF_E_LAUNCH;
    if (na > 0) hipLaunchKernelGGL(k_occ_set, dim3(pn_cdiv(na, 256)), dim3(256), 0, s, d_a_xyz, (long long)na, g, bits);
    hipLaunchKernelGGL(k_occ_test, dim3(pn_cdiv(nb, 256)), dim3(256), 0, s, d_b_xyz, (long long)nb, g, bits, (int *)(ws + L.flags), d_mask);
    return sel_finish(d_b_xyz, nb, L, ws, d_kept_xyz, d_count, s);
}

extern "C" size_t pnerf_crop_ranges_workspace_bytes(int64_t n) {
    if (n < 0 || n > SEL_MAX) return 0;
    return sel_layout(n, 0).total;
}

extern "C" int pnerf_crop_ranges(const float *d_xyz, int64_t n, const float *ranges6_host, float *d_kept_xyz, int32_t *d_count, uint8_t *d_mask,
                                 void *d_ws, size_t ws_bytes, void *stream) {
    if (n < 0 || !ranges6_host || !d_count) return PNERF_E_INVAL;
    if (n > SEL_MAX) return PNERF_E_UNSUP;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return hipMemsetAsync(d_count, 0, sizeof(int), s) == hipSuccess ? 0 : PNERF_E_LAUNCH;
    if (!d_xyz || !d_kept_xyz || !d_mask || !d_ws) return PNERF_E_INVAL;
    const SelLayout L = sel_layout(n, 0);
    if (ws_bytes < L.total) return PNERF_E_WS;
    CropArgs g;
    for (int j = 0; j < 6; ++j) g.r[j] = ranges6_host[j];
    char *ws = (char *)d_ws;
    hipLaunchKernelGGL(k_crop_flag, dim3(pn_cdiv(n, 256)), dim3(256), 0, s, d_xyz, (long long)n, g, (int *)(ws + L.flags), d_mask);
    return sel_finish(d_xyz, n, L, ws, d_kept_xyz, d_count, s);
}

extern "C" size_t pnerf_group_by_view_workspace_bytes(int64_t n, int M) {
    if (!group_fits(n, M)) return 0;
    return group_layout(n, M).total;
}

extern "C" int pnerf_group_by_view(const int32_t *d_cam_ind, int64_t n, int M, int64_t *d_order, int64_t *d_offsets, void *d_ws, size_t ws_bytes,
                                   void *stream) {
    if (n < 0 || M < 1 || !d_offsets) return PNERF_E_INVAL;
    if (!group_fits(n, M)) return PNERF_E_UNSUP;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return hipMemsetAsync(d_offsets, 0, (size_t)(M + 1) * sizeof(int64_t), s) == hipSuccess ? 0 : PNERF_E_LAUNCH;
    if (!d_cam_ind || !d_order || !d_ws) return PNERF_E_INVAL;
    const GroupLayout L = group_layout(n, M);
    if (ws_bytes < L.total) return PNERF_E_WS;
    char *ws = (char *)d_ws;
    int *hist = (int *)(ws + L.hist), *start = (int *)(ws + L.start), *rank = (int *)(ws + L.rank), *scan = (int *)(ws + L.scan);
    if (hipMemsetAsync(hist, 0, (size_t)(L.cells + 1) * 4, s) != hipSuccess) return PNERF_E_LAUNCH;
    if (hipMemsetAsync(d_order, 0xff, (size_t)n * sizeof(int64_t), s) != hipSuccess) return PNERF_E_LAUNCH;      // -1 where nothing is placed
    hipLaunchKernelGGL(k_group_rank, dim3(L.nblk), dim3(GB_TPB), 0, s, d_cam_ind, (long long)n, M, L.nblk, rank, hist);
    const int rc = pn_exclusive_scan_i32(hist, start, L.cells, scan, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_group_place, dim3(pn_cdiv(n, 256)), dim3(256), 0, s, d_cam_ind, (long long)n, M, L.nblk, rank, start, (long long *)d_order);
    hipLaunchKernelGGL(k_group_offsets, dim3(pn_cdiv(M + 1, 256)), dim3(256), 0, s, start, M, L.nblk, (long long *)d_offsets);
    PN_CHECK_LAUNCH();
    return 0;
}
