// loss.hip -- the two terms of the training loss that run on the renderer's dense results: the zero-one regulariser on the confidences of
// the hit rays' neighbor slots and the colour term over the dense ray colours.  Each has a forward that leaves per-block partial sums (the
// caller adds them: deterministic) and a backward.
#include "pn_ray.h"

namespace {
constexpr int TPB = 256;

// ---- the zero-one regulariser on the confidences of the hit rays' neighbor slots, fused --------------------------------------------
// Reference: conf_coefficient = gradient_clamp(points_conf[clamp(sample_pidx, min=0)], 1e-4, 1) (point_aggregators.py:722-724, 812) and
// loss_zero_one = mean(log(v) + log(1 - v)), v = clamp(conf_coefficient, eps, 1 - eps) (base_rendering_model.py:630-641): a gather, two
// clamps, two logs, a reduction and their autograd mirror over [R'', SR, K] elements (84 M at configs[3]) -- ~20 element-wise passes
// in ATen.  Here: one pass that sums the terms per block (the caller adds the per-block partials: deterministic), one pass that
// adds  g * (1 / v - 1 / (1 - v)) [eps <= c' <= 1 - eps]  into the confidence gradient, with the point-0 flood of the empty slots
//  reduced per block first.
// One forward and one backward kernel over rows x slots elements of the index table, a workgroup per row at a time.  The rays form: rows = R,
// slots = SR * K, hit = the per-ray hit flags (only rays that hit the cloud count: the reference forms conf_coefficient for the R'' hit rays
// only; no [R'', SR, K] copy of the table is ever made).  The flat form: rows of TPB elements, hit = NULL, `total` cuts the last row short.
__global__ __launch_bounds__(TPB) void k_zero_one_forward(const float *__restrict__ conf, int n, const int *__restrict__ idx, const int *__restrict__ hit, long long rows, int slots,
                                                          long long total, float eps, float *__restrict__ partial) {
    __shared__ float red[TPB / 64];
    float acc = 0.f;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        if (hit && hit[r] <= 0) continue;
        const int *row = idx + r * slots;
        const int m = (int)(total - r * slots < slots ? total - r * slots : slots);
        for (int e = threadIdx.x; e < m; e += TPB) acc += PnZeroOne(conf[pn_zero_one_point(row[e], n)], eps).value();
    }
    acc = pn_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < TPB / 64; ++w) t += red[w];
        partial[blockIdx.x] = t;
    }
}
__global__ __launch_bounds__(TPB) void k_zero_one_backward(const float *__restrict__ conf, int n, const int *__restrict__ idx, const int *__restrict__ hit, long long rows, int slots,
                                                           long long total, float eps, const float *__restrict__ gscale, float *__restrict__ grad_conf) {
    __shared__ float row0;
    if (threadIdx.x == 0) row0 = 0.f;
    __syncthreads();
    const float gs = gscale[0];
    float mine0 = 0.f;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        if (hit && hit[r] <= 0) continue;
        const int *row = idx + r * slots;
        const int m = (int)(total - r * slots < slots ? total - r * slots : slots);
        for (int e = threadIdx.x; e < m; e += TPB) {
            const int p = pn_zero_one_point(row[e], n);
            const PnZeroOne z(conf[p], eps);
            if (!z.inside()) continue;
            if (p == 0) mine0 += z.grad(gs);
            else atomicAdd(&grad_conf[p], z.grad(gs));
        }
    }
    mine0 = pn_wave_sum(mine0);
    if ((threadIdx.x & 63) == 0 && mine0 != 0.f) atomicAdd(&row0, mine0);
    __syncthreads();
    if (threadIdx.x == 0 && row0 != 0.f) atomicAdd(&grad_conf[0], row0);
}

// colour term of the training loss over the DENSE ray colours with the rays' hit flags (models/base_rendering_model.py:543-551:
// ray_masked_coarse_raycolor = sum over the hit rays' (colour - gt)^2, the caller divides by its global element count): no compaction of the
// hit rays (argsort + index_selects) on the way to a scalar.  partial[b] = block sums; backward writes d colour for EVERY ray (0 for a miss),
// which is what the renderer's backward reads.
__global__ __launch_bounds__(256) void k_color_loss_forward_rays(const float *__restrict__ col, const float *__restrict__ gt, const int *__restrict__ hit, int R,
                                                                 float *__restrict__ partial) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < R; r += gridDim.x * 256)
        if (hit[r] > 0) {
            const float dx = col[3 * r] - gt[3 * r], dy = col[3 * r + 1] - gt[3 * r + 1], dz = col[3 * r + 2] - gt[3 * r + 2];
            acc += (dx * dx + dy * dy) + dz * dz;
        }
    acc = pn_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_color_loss_backward_rays(const float *__restrict__ col, const float *__restrict__ gt, const int *__restrict__ hit, int R,
                                                                  const float *__restrict__ gscale, float *__restrict__ gcol) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float g = hit[r] > 0 ? 2.f * gscale[0] : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) gcol[3 * r + c] = g == 0.f ? 0.f : g * (col[3 * r + c] - gt[3 * r + c]);
}

// depth and mask supervision over the DENSE per-ray geometry of a render (the two loops of models/base_rendering_model.py:610-626:
// l2loss(coarse_depth * gt_mask, gt_depth * gt_mask) and l2loss(coarse_is_background * (1 - gt_mask), 1 - gt_mask), as numerators -- the
// caller divides by its global ray count).  Per ray, with m = gt_mask, d = depth_sum / (acc + 1e-6) (models/neural_points_volumetric_model.py:321)
// and T = the background transmittance; a ray that missed has d = 0 and T = 1, as fill_invalid leaves them:
//   depth term = (m (d - gt_depth))^2        bg term = ((1 - m) (T - 1))^2
// partial[b] = block sums of the depth terms, partial[gridDim.x + b] = of the bg terms.  PnGeomRay is the one statement of both passes.
struct PnGeomRay {
    float inv, d, ed, eb, m, w;           // 1 / (acc + 1e-6), depth, m (d - gt), (1 - m) (T - 1), m, 1 - m
    __device__ __forceinline__ PnGeomRay(bool hit, float depth_sum, float acc, float T, float gt, float mask) {
        inv = 1.f / (acc + 1e-6f);
        d = hit ? depth_sum * inv : 0.f;
        m = mask; w = 1.f - mask;
        ed = m * (d - gt);
        eb = w * ((hit ? T : 1.f) - 1.f);
    }
};
__global__ __launch_bounds__(256) void k_geometry_loss_forward_rays(const float *__restrict__ depth_sum, const float *__restrict__ acc, const float *__restrict__ bg_trans,
                                                                    const int *__restrict__ hit, const float *__restrict__ gt_depth, const float *__restrict__ gt_mask,
                                                                    int R, float *__restrict__ partial) {
    __shared__ float red[2][4];
    float sd = 0.f, sb = 0.f;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < R; r += gridDim.x * 256) {
        const bool h = hit[r] > 0;
        const PnGeomRay g(h, h ? depth_sum[r] : 0.f, h ? acc[r] : 0.f, h ? bg_trans[r] : 1.f, gt_depth[r], gt_mask[r]);
        sd += g.ed * g.ed;
        sb += g.eb * g.eb;
    }
    sd = pn_wave_sum(sd); sb = pn_wave_sum(sb);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sd; red[1][threadIdx.x >> 6] = sb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partial[gridDim.x + blockIdx.x] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}
// grad_geom [R,3] = (d / d depth_sum, d / d acc, d / d T) of gscale[0] * (depth numerator) + gscale[1] * (bg numerator); zeros on a miss.
// The 1 / (acc + 1e-6) of a hit but almost transparent ray is the reference's formula and is kept.
__global__ __launch_bounds__(256) void k_geometry_loss_backward_rays(const float *__restrict__ depth_sum, const float *__restrict__ acc, const float *__restrict__ bg_trans,
                                                                     const int *__restrict__ hit, const float *__restrict__ gt_depth, const float *__restrict__ gt_mask,
                                                                     int R, const float *__restrict__ gscale, float *__restrict__ grad_geom) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float g_ds = 0.f, g_acc = 0.f, g_T = 0.f;
    if (hit[r] > 0) {
        const PnGeomRay g(true, depth_sum[r], acc[r], bg_trans[r], gt_depth[r], gt_mask[r]);
        g_ds = (2.f * gscale[0]) * (g.m * g.ed) * g.inv;                  // 2 m^2 (d - gt) / (acc + 1e-6)
        g_acc = -g_ds * g.d;
        g_T = (2.f * gscale[1]) * (g.w * g.eb);                           // 2 (1 - m)^2 (T - 1)
    }
    grad_geom[3 * r] = g_ds; grad_geom[3 * r + 1] = g_acc; grad_geom[3 * r + 2] = g_T;
}
}  // namespace
extern "C" int pnerf_geometry_loss_forward_rays(const float *d_depth_sum, const float *d_acc, const float *d_bg_trans, const int32_t *d_ray_hit,
                                                const float *d_gt_depth, const float *d_gt_mask, int R, float *d_partial, void *stream) {
    if (!d_depth_sum || !d_acc || !d_bg_trans || !d_ray_hit || !d_gt_depth || !d_gt_mask || !d_partial || R < 0) return PNERF_E_INVAL;
    PnProfScope prof(PNK_GATHER, (hipStream_t)stream);
    hipLaunchKernelGGL(k_geometry_loss_forward_rays, dim3(pnerf_color_loss_blocks(R)), dim3(256), 0, (hipStream_t)stream, d_depth_sum, d_acc, d_bg_trans, d_ray_hit,
                       d_gt_depth, d_gt_mask, R, d_partial);
    PN_CHECK_LAUNCH();
    return 0;
}
extern "C" int pnerf_geometry_loss_backward_rays(const float *d_depth_sum, const float *d_acc, const float *d_bg_trans, const int32_t *d_ray_hit,
                                                 const float *d_gt_depth, const float *d_gt_mask, int R, const float *d_gscale2, float *d_grad_geom, void *stream) {
    if (R == 0) return 0;
    if (!d_depth_sum || !d_acc || !d_bg_trans || !d_ray_hit || !d_gt_depth || !d_gt_mask || !d_gscale2 || !d_grad_geom || R < 0) return PNERF_E_INVAL;
    PnProfScope prof(PNK_GATHER, (hipStream_t)stream);
    hipLaunchKernelGGL(k_geometry_loss_backward_rays, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_depth_sum, d_acc, d_bg_trans, d_ray_hit,
                       d_gt_depth, d_gt_mask, R, d_gscale2, d_grad_geom);
    PN_CHECK_LAUNCH();
    return 0;
}
extern "C" int pnerf_color_loss_blocks(int R) {
    const int b = (R + 255) / 256;
    return b < 1 ? 1 : (b > 1024 ? 1024 : b);
}
extern "C" int pnerf_color_loss_forward_rays(const float *d_ray_color, const float *d_gt, const int32_t *d_ray_hit, int R, float *d_partial, void *stream) {
    if (!d_ray_color || !d_gt || !d_ray_hit || !d_partial || R < 0) return PNERF_E_INVAL;
    PnProfScope prof(PNK_GATHER, (hipStream_t)stream);
    hipLaunchKernelGGL(k_color_loss_forward_rays, dim3(pnerf_color_loss_blocks(R)), dim3(256), 0, (hipStream_t)stream, d_ray_color, d_gt, d_ray_hit, R, d_partial);
    PN_CHECK_LAUNCH();
    return 0;
}
extern "C" int pnerf_color_loss_backward_rays(const float *d_ray_color, const float *d_gt, const int32_t *d_ray_hit, int R, const float *d_gscale,
                                              float *d_grad_ray_color, void *stream) {
    if (R == 0) return 0;
    if (!d_ray_color || !d_gt || !d_ray_hit || !d_gscale || !d_grad_ray_color || R < 0) return PNERF_E_INVAL;
    PnProfScope prof(PNK_GATHER, (hipStream_t)stream);
    hipLaunchKernelGGL(k_color_loss_backward_rays, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_ray_color, d_gt, d_ray_hit, R, d_gscale, d_grad_ray_color);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_zero_one_blocks(int64_t n_idx) {
    const long long b = (n_idx + TPB - 1) / TPB;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
// both passes of both forms: rows x slots elements of d_idx (`total` of them exist), d_hit optional; the caller has checked its arguments
static int pn_zero_one_launch(const float *d_conf, int n_points, const int32_t *d_idx, const int32_t *d_hit, long long rows, int slots, long long total, float eps,
                              float *d_partial, const float *d_gscale, float *d_grad_conf, void *stream) {
    const dim3 grid(pnerf_zero_one_blocks(rows * TPB));
    PnProfScope prof(PNK_GATHER, (hipStream_t)stream);
    if (d_partial) hipLaunchKernelGGL(k_zero_one_forward, grid, dim3(TPB), 0, (hipStream_t)stream, d_conf, n_points, d_idx, d_hit, rows, slots, total, eps, d_partial);
    else hipLaunchKernelGGL(k_zero_one_backward, grid, dim3(TPB), 0, (hipStream_t)stream, d_conf, n_points, d_idx, d_hit, rows, slots, total, eps, d_gscale, d_grad_conf);
    PN_CHECK_LAUNCH();
    return 0;
}
extern "C" int pnerf_zero_one_forward_rays(const float *d_conf, int n_points, const int32_t *d_idx, const int32_t *d_ray_hit, int R, int slots_per_ray, float eps,
                                           float *d_partial, void *stream) {
    if (!d_conf || !d_partial || !d_idx || !d_ray_hit || n_points <= 0 || R < 0 || slots_per_ray <= 0) return PNERF_E_INVAL;
    return pn_zero_one_launch(d_conf, n_points, d_idx, d_ray_hit, R, slots_per_ray, (long long)R * slots_per_ray, eps, d_partial, nullptr, nullptr, stream);
}
extern "C" int pnerf_zero_one_backward_rays(const float *d_conf, int n_points, const int32_t *d_idx, const int32_t *d_ray_hit, int R, int slots_per_ray, float eps,
                                            const float *d_gscale, float *d_grad_conf, void *stream) {
    if (R == 0) return 0;
    if (!d_conf || !d_idx || !d_ray_hit || !d_gscale || !d_grad_conf || n_points <= 0 || R < 0 || slots_per_ray <= 0) return PNERF_E_INVAL;
    return pn_zero_one_launch(d_conf, n_points, d_idx, d_ray_hit, R, slots_per_ray, (long long)R * slots_per_ray, eps, nullptr, d_gscale, d_grad_conf, stream);
}
extern "C" int pnerf_zero_one_forward(const float *d_conf, int n_points, const int32_t *d_idx, int64_t n_idx, float eps, float *d_partial, void *stream) {
    if (!d_conf || !d_partial || n_points <= 0 || n_idx < 0 || (n_idx > 0 && !d_idx)) return PNERF_E_INVAL;
    return pn_zero_one_launch(d_conf, n_points, d_idx, nullptr, (n_idx + TPB - 1) / TPB, TPB, n_idx, eps, d_partial, nullptr, nullptr, stream);
}
extern "C" int pnerf_zero_one_backward(const float *d_conf, int n_points, const int32_t *d_idx, int64_t n_idx, float eps, const float *d_gscale,
                                       float *d_grad_conf, void *stream) {
    if (n_idx == 0) return 0;
    if (!d_conf || !d_idx || !d_gscale || !d_grad_conf || n_points <= 0 || n_idx < 0) return PNERF_E_INVAL;
    return pn_zero_one_launch(d_conf, n_points, d_idx, nullptr, (n_idx + TPB - 1) / TPB, TPB, n_idx, eps, nullptr, d_gscale, d_grad_conf, stream);
}
