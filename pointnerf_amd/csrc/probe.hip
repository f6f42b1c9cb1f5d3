// probe.hip -- the probe pass of the point-growing step on the renderer's DENSE per-ray results.
//
// k_probe_rays restates the `opt.prob == 1` block of NeuralPointsRayMarching.forward (models/neural_points_volumetric_model.py:331-352):
// per ray the sample of largest opacity, its world location, the distance from there to the nearest of its K neighbor points and the
// weight x confidence averages of the neighbors' colour / direction / confidence / embedding.  The reference forms them from [R'', SR, K]
// copies of the hit rays' tensors with a dozen gathers and reductions; everything needed already lies dense over the R submitted rays
// after pnerf_render_forward (opacity, weight, sample_loc, sample_pidx, ray_hit), and only ONE sample per ray and its K point rows are
// touched.  A ray that missed the cloud gets zeros in all seven outputs -- fill_invalid's `prob == 1` zero fill (:121-122 "unmask") -- so
// the outputs are full-size and nothing is compacted or scattered afterwards.
//
// Shape: one 64-lane wavefront per ray (like k_raymarch_forward), four rays per workgroup, no LDS, no atomics.  The lanes stride over the
// ray's SR opacities in chunks of 64; the (value, index) pairs meet in PnWaveArgmax (pn_ray.h), whose order relation -- larger value
// first, then the smaller index -- is total, so every lane ends with the same pair whatever the tree and the result is the LOWEST index
// among the maxima.  Lane k < K then owns neighbor slot k (point index, weight, distance); in the averages lane c owns an output column (0..31 the
// embedding: a point row is one coalesced 128-byte read of 32 lanes; 32..34 colour, 35..37 direction, 38 confidence) and the K slots
// arrive by lane broadcast.  The pass is latency- and HBM-bound: SR opacities plus K point rows per hit ray.
//
// k_probe_hole_mask restates the candidate rule of probe_hole (run/train_ft.py:489-500, with bloat_inds :532-540) per pixel of a view.
#include "pn_ray.h"

namespace {
constexpr int PN_PR_TPB = 256;       // k_probe_rays: 4 rays per workgroup
constexpr int PN_PR_EMB = 32;        // floats of an embedding row (the only feature width of this library: pnerf_mlp_layout)
constexpr int PN_HM_TPB = 256;

struct PnProbeOut {
    float *max_opacity, *loc3, *far_dist, *avg_color3, *avg_dir3, *avg_conf, *avg_emb32;
};

// what the kernel reads of pnerf_points (the probe outputs do not depend on per-point frames)
struct PrPoints { const float *xyz, *embedding, *conf, *dir, *color; int32_t n, feat_dim; };
__global__ __launch_bounds__(PN_PR_TPB) void k_probe_rays(PrPoints pts, const float *__restrict__ opacity, const float *__restrict__ weight,
                                                          const float *__restrict__ sample_loc, const int *__restrict__ sample_pidx,
                                                          const int *__restrict__ ray_hit, int R, int SR, int K, PnProbeOut o) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (PN_PR_TPB / 64) + (threadIdx.x >> 6);
    if (r >= R) return;
    // the lane's output element: 0..31 embedding, 32..34 colour, 35..37 direction, 38 confidence, 40..42 location, 43 opacity, 44 distance
    float *dst = nullptr;
    if (lane < PN_PR_EMB) dst = o.avg_emb32 + r * PN_PR_EMB + lane;
    else if (lane < 35) dst = o.avg_color3 + r * 3 + (lane - 32);
    else if (lane < 38) dst = o.avg_dir3 + r * 3 + (lane - 35);
    else if (lane == 38) dst = o.avg_conf + r;
    else if (lane >= 40 && lane < 43) dst = o.loc3 + r * 3 + (lane - 40);
    else if (lane == 43) dst = o.max_opacity + r;
    else if (lane == 44) dst = o.far_dist + r;
    if (ray_hit[r] <= 0) {                                   // (wave-uniform)  :121-122: the missed rays' probe outputs are zero
        if (dst) *dst = 0.f;
        return;
    }
    // ---- s* = the lowest index among the maxima of opacity[r, 0 .. SR-1]   (torch.max(dim=-1), :331)
    const float *op = opacity + r * SR;
    PnWaveArgmax best;
    for (int s = lane; s < SR; s += 64) best.take(op[s], s);
    best.meet();
    const int ss = best.i < SR ? best.i : 0;                         // (a row of NaN compares false everywhere: stay inside the row)
    const long long smp = r * SR + ss;
    const float mx = op[ss];
    const float lx = sample_loc[smp * 3], ly = sample_loc[smp * 3 + 1], lz = sample_loc[smp * 3 + 2];       // :333-334
    // ---- lane k < K: neighbor slot k of the sample
    int p = 0;
    float w = 0.f, dist = INFINITY;
    if (lane < K) {
        p = pn_zero_one_point(sample_pidx[smp * K + lane], pts.n);                          // an empty slot (-1) reads point 0  neural_points.py:708
        w = weight[smp * K + lane] * fminf(fmaxf(pts.conf[p], 1e-4f), 1.f);                 // weight * gradient_clamp(conf)  :336, point_aggregators.py:722-724
        const float dx = pts.xyz[3 * (long long)p] - lx, dy = pts.xyz[3 * (long long)p + 1] - ly, dz = pts.xyz[3 * (long long)p + 2] - lz;
        dist = sqrtf(dx * dx + dy * dy + dz * dz);                                          // :341-342 (point 0 of the empty slots included)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dist = fminf(dist, __shfl_xor(dist, off, 64));
    // ---- lane c: column c of sum_k w_k row_k   :344-352
    const float *col = nullptr;
    int stride = 0;
    if (lane < PN_PR_EMB) { col = pts.embedding + lane; stride = PN_PR_EMB; }
    else if (lane < 35) { col = pts.color + (lane - 32); stride = 3; }
    else if (lane < 38) { col = pts.dir + (lane - 35); stride = 3; }
    else if (lane == 38) { col = pts.conf; stride = 1; }
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const float wk = __shfl(w, k, 64);
        const int pk = __shfl(p, k, 64);
        if (col) acc += wk * col[(long long)pk * stride];
    }
    if (lane == 40) acc = lx; else if (lane == 41) acc = ly; else if (lane == 42) acc = lz;
    else if (lane == 43) acc = mx; else if (lane == 44) acc = dist;
    if (dst) *dst = acc;
}

// One thread per pixel of the [H, W] view.  flag = hit && near && max_opacity > opacity_thresh, near = a missed pixel whose ground truth
// is not background (|gt - bg| > 0.002) in the 3 x 3 neighborhood (bloat_inds clamps the neighbors of a border pixel onto border pixels,
// which adds nothing a zero-padded 3 x 3 maximum does not have) or -- far_thresh > 0 -- a well-rendered hit far from every neural point.
__device__ __forceinline__ float pn_hm_norm3(const float *a, float bx, float by, float bz) {
    const float dx = a[0] - bx, dy = a[1] - by, dz = a[2] - bz;
    return sqrtf(dx * dx + dy * dy + dz * dz);
}
__global__ __launch_bounds__(PN_HM_TPB) void k_probe_hole_mask(const signed char *__restrict__ ray_mask, const float *__restrict__ max_opacity,
                                                               const float *__restrict__ far_dist, const float *__restrict__ raycolor,
                                                               const float *__restrict__ gt, const unsigned char *__restrict__ edge, float bgx,
                                                               float bgy, float bgz, int H, int W, float opacity_thresh, float far_thresh,
                                                               int *__restrict__ flags) {
    const long long i = (long long)blockIdx.x * PN_HM_TPB + threadIdx.x;
    if (i >= (long long)H * W) return;
    int flag = 0;
    if (ray_mask[i] > 0 && max_opacity[i] > opacity_thresh) {
        const int y = (int)(i / W), x = (int)(i - (long long)y * W);
        bool near = false;
        for (int yy = max(y - 1, 0); yy <= min(y + 1, H - 1); ++yy)
            for (int xx = max(x - 1, 0); xx <= min(x + 1, W - 1); ++xx) {
                const long long j = (long long)yy * W + xx;
                near = near || (!(ray_mask[j] > 0) && edge[j] != 0 && pn_hm_norm3(gt + 3 * j, bgx, bgy, bgz) > 0.002f);       // :489-492
            }
        if (far_thresh > 0.f)                                                                                                  // :494-498
            near = near || (far_dist[i] > far_thresh && pn_hm_norm3(gt + 3 * i, raycolor[3 * i], raycolor[3 * i + 1], raycolor[3 * i + 2]) < 0.1f);
        flag = near ? 1 : 0;
    }
    flags[i] = flag;
}
}  // namespace

extern "C" int pnerf_probe_rays(const pnerf_points *pts, const float *d_opacity, const float *d_weight, const float *d_sample_loc,
                                const int32_t *d_sample_pidx, const int32_t *d_ray_hit, int R, int SR, int K, float *d_max_opacity,
                                float *d_loc3, float *d_far_dist, float *d_avg_color3, float *d_avg_dir3, float *d_avg_conf, float *d_avg_emb32,
                                void *stream) {
    if (!pts || R < 0 || SR <= 0 || K < 1 || K > PNERF_MAX_K) return PNERF_E_INVAL;
    if (R == 0) return 0;
    if (!pts->xyz || !pts->embedding || !pts->conf || !pts->dir || !pts->color || pts->n <= 0) return PNERF_E_INVAL;
    if (!d_opacity || !d_weight || !d_sample_loc || !d_sample_pidx || !d_ray_hit || !d_max_opacity || !d_loc3 || !d_far_dist || !d_avg_color3 ||
        !d_avg_dir3 || !d_avg_conf || !d_avg_emb32) return PNERF_E_INVAL;
    if (pts->feat_dim != PN_PR_EMB) return PNERF_E_UNSUP;
    PnProbeOut o = {d_max_opacity, d_loc3, d_far_dist, d_avg_color3, d_avg_dir3, d_avg_conf, d_avg_emb32};
    hipLaunchKernelGGL(k_probe_rays, dim3(pn_cdiv(R, PN_PR_TPB / 64)), dim3(PN_PR_TPB), 0, (hipStream_t)stream, PrPoints{pts->xyz, pts->embedding, pts->conf, pts->dir, pts->color, pts->n, pts->feat_dim}, d_opacity, d_weight,
                       d_sample_loc, d_sample_pidx, d_ray_hit, R, SR, K, o);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_probe_hole_mask(const int8_t *d_ray_mask, const float *d_max_opacity, const float *d_far_dist, const float *d_raycolor,
                                     const float *d_gt, const uint8_t *d_edge, const float *bg3_host, int H, int W, float opacity_thresh,
                                     float far_thresh, int32_t *d_flags, void *stream) {
    if (!d_ray_mask || !d_max_opacity || !d_far_dist || !d_raycolor || !d_gt || !d_edge || !bg3_host || !d_flags || H <= 0 || W <= 0)
        return PNERF_E_INVAL;
    const long long n = (long long)H * W;
    if ((n + PN_HM_TPB - 1) / PN_HM_TPB > 0x7fffffffLL) return PNERF_E_UNSUP;
    hipLaunchKernelGGL(k_probe_hole_mask, dim3((unsigned)((n + PN_HM_TPB - 1) / PN_HM_TPB)), dim3(PN_HM_TPB), 0, (hipStream_t)stream,
                       (const signed char *)d_ray_mask, d_max_opacity, d_far_dist, d_raycolor, d_gt, d_edge, bg3_host[0], bg3_host[1], bg3_host[2],
                       H, W, opacity_thresh, far_thresh, d_flags);
    PN_CHECK_LAUNCH();
    return 0;
}
