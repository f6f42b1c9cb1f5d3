// raygeom.hip -- per-ray depth and opacity maps of a render-only pass, on the renderer's DENSE per-ray results.
//
// k_ray_geometry: what `is_compute_depth` of the reference was meant to hand out (models/neural_points_volumetric_model.py:318-322:
// depth = sum_s blend_weight_s ray_ts_s / (sum_s blend_weight_s + 1e-6); `ray_ts` is undefined there, so the option raises in the reference
// and stays refused here).  The substitute for ray_ts is the camera-z depth of a sample, the quantity the ray march's ray-dist block
// already uses (raydir is not normalised, so z IS the ray parameter up to the pixel's constant); blend weight, opacity and transmittance
// are ray_march's (models/rendering/diff_ray_marching.py:508-554) as k_raymarch_forward (render.hip) forms them: opacity and blend_w are
// READ BACK from the renderer's outputs, not recomputed, and the inclusive transmittance T_s = prod_{j <= s} (1 - op_j + 1e-10) is a
// wave-inclusive product per 64-slot chunk times the product carried over the chunks in front (PnTransmittance, pn_ray.h).  Per ray:
//   acc = sum_s bw_s      depth_sum = sum_s bw_s z_s (valid slots only)      depth = depth_sum / (acc + 1e-6)
//   median_slot = the lowest valid slot with T_s < 0.5 (-1: none),   median_depth = z there (0: none)
// A ray that missed the cloud gets zeros and -1; its rows are not read.
//
// Shape: one 64-lane wavefront per ray (like k_raymarch_forward / k_probe_rays), four rays per workgroup, no LDS, no atomics.  The lanes
// stride over SR in chunks of 64 and keep per-lane partial sums over the chunks; lanes at or beyond SR carry neutral elements (u = 1,
// bw = 0).  The sums meet in the xor butterfly of pn_wave_sum (pn_ray.h), so the accumulation order is a function of SR alone and two calls
// give the same bits.  The pass is HBM-bound: 24 bytes per slot (sample_loc, sample_nn, opacity, blend_w) against the ray march's ~44.
// The wave scans, the perspective depth and the transmittance step are pn_ray.h's, the ones the ray march itself runs.
//
// k_geometry_canvas: the per-pixel fill of the three maps for one chunk of rays (one thread per ray), instead of three index-puts.
#include "pn_ray.h"

namespace {
constexpr int PN_RG_TPB = 256;       // k_ray_geometry: 4 rays per workgroup
constexpr int PN_GC_TPB = 256;

struct RgArgs {
    pnerf_camera cam;
    const float *sample_loc, *opacity, *blend_w;
    const int *nn, *hit;
    int R, SR;
};
struct RgOut {
    float *acc, *depth_sum, *depth, *median_depth;
    int *median_slot;
};

__global__ __launch_bounds__(PN_RG_TPB) void k_ray_geometry(RgArgs a, RgOut o) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (PN_RG_TPB / 64) + (threadIdx.x >> 6);
    if (r >= a.R) return;
    if (a.hit[r] <= 0) {                                                 // (wave-uniform)  a miss: zeros, no crossing; the rows are not read
        if (lane == 0) { o.acc[r] = 0.f; o.depth_sum[r] = 0.f; o.depth[r] = 0.f; o.median_depth[r] = 0.f; o.median_slot[r] = -1; }
        return;
    }
    const int SR = a.SR;
    const long long row = r * SR;
    PnTransmittance tr;
    float sum_w = 0.f, sum_wz = 0.f, mz = 0.f;
    int ms = -1;
    for (int base = 0; base < SR; base += 64) {
        const int s = base + lane;
        const bool in = s < SR;
        const bool valid = in && a.nn[row + s] > 0;                      // ray_valid = any_K(mask)  point_aggregators.py:741
        const float z = valid ? pn_pers_z(a.cam, a.sample_loc + (row + s) * 3) : 0.f;       // an empty slot's position is never read
        const float op = in ? a.opacity[row + s] : 0.f;
        const float bw = in ? a.blend_w[row + s] : 0.f;                  // (0 on the empty slots: the renderer wrote it)
        sum_w += bw;
        sum_wz += bw * z;
        float Tx;
        const float Tin = tr.step(op, in, lane, Tx);                     // transmittance BEHIND slot s  (diff_ray_marching.py:533)
        const unsigned long long below = __ballot(valid && Tin < 0.5f);
        if (ms < 0 && below != 0ull) {                                   // (wave-uniform)  the first crossing: the lowest lane of the lowest chunk
            const int first = __ffsll((long long)below) - 1;
            ms = base + first;
            mz = __shfl(z, first, 64);
        }
    }
    sum_w = pn_wave_sum(sum_w);
    sum_wz = pn_wave_sum(sum_wz);
    if (lane == 0) {
        o.acc[r] = sum_w;
        o.depth_sum[r] = sum_wz;
        o.depth[r] = sum_wz / (sum_w + 1e-6f);                           // neural_points_volumetric_model.py:321
        o.median_depth[r] = mz;
        o.median_slot[r] = ms;
    }
}

// One thread per ray of a chunk: the ray's three values go to pixel (px, py) of the [H, W] canvases; a ray that missed writes 0.  A pixel
// outside the image writes nothing and sets *flag to PNERF_E_INVAL (every thread that sets it stores the same word: no atomic).
__global__ __launch_bounds__(PN_GC_TPB) void k_geometry_canvas(const int *__restrict__ pixel_idx, const signed char *__restrict__ ray_mask,
                                                               const float *__restrict__ depth, const float *__restrict__ median_depth,
                                                               const float *__restrict__ acc, long long n, int H, int W,
                                                               float *__restrict__ depth_canvas, float *__restrict__ median_canvas,
                                                               float *__restrict__ acc_canvas, int *__restrict__ flag) {
    const long long i = (long long)blockIdx.x * PN_GC_TPB + threadIdx.x;
    if (i >= n) return;
    const int px = pixel_idx[2 * i], py = pixel_idx[2 * i + 1];
    if (px < 0 || px >= W || py < 0 || py >= H) { *flag = PNERF_E_INVAL; return; }
    const bool hit = !ray_mask || ray_mask[i] > 0;
    const long long j = (long long)py * W + px;
    depth_canvas[j] = hit ? depth[i] : 0.f;
    median_canvas[j] = hit ? median_depth[i] : 0.f;
    acc_canvas[j] = hit ? acc[i] : 0.f;
}
}  // namespace

extern "C" int pnerf_ray_geometry(const pnerf_camera *cam, const float *d_sample_loc, const int32_t *d_sample_nn, const int32_t *d_ray_hit,
                                  const float *d_opacity, const float *d_blend_w, int R, int SR, float *d_acc, float *d_depth_sum,
                                  float *d_depth, float *d_median_depth, int32_t *d_median_slot, void *stream) {
    if (!cam || R < 0 || SR < 1) return PNERF_E_INVAL;
    if (R == 0) return 0;
    if (!d_sample_loc || !d_sample_nn || !d_ray_hit || !d_opacity || !d_blend_w || !d_acc || !d_depth_sum || !d_depth || !d_median_depth ||
        !d_median_slot) return PNERF_E_INVAL;
    RgArgs a = {*cam, d_sample_loc, d_opacity, d_blend_w, d_sample_nn, d_ray_hit, R, SR};
    RgOut o = {d_acc, d_depth_sum, d_depth, d_median_depth, d_median_slot};
    hipLaunchKernelGGL(k_ray_geometry, dim3(pn_cdiv(R, PN_RG_TPB / 64)), dim3(PN_RG_TPB), 0, (hipStream_t)stream, a, o);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_geometry_canvas(const int32_t *d_pixel_idx, const int8_t *d_ray_mask, const float *d_depth, const float *d_median_depth,
                                     const float *d_acc, int n_rays, int H, int W, float *d_depth_canvas, float *d_median_canvas,
                                     float *d_acc_canvas, int32_t *d_flag, void *stream) {
    if (n_rays < 0 || H <= 0 || W <= 0) return PNERF_E_INVAL;
    if (n_rays == 0) return 0;
    if (!d_pixel_idx || !d_depth || !d_median_depth || !d_acc || !d_depth_canvas || !d_median_canvas || !d_acc_canvas || !d_flag)
        return PNERF_E_INVAL;
    hipLaunchKernelGGL(k_geometry_canvas, dim3(pn_cdiv(n_rays, PN_GC_TPB)), dim3(PN_GC_TPB), 0, (hipStream_t)stream, (const int *)d_pixel_idx,
                       (const signed char *)d_ray_mask, d_depth, d_median_depth, d_acc, (long long)n_rays, H, W, d_depth_canvas, d_median_canvas,
                       d_acc_canvas, (int *)d_flag);
    PN_CHECK_LAUNCH();
    return 0;
}
