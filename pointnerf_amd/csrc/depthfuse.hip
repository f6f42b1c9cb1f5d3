// depthfuse.hip -- from one depth map per view to the raw point cloud that pointinit.hip voxelises: the multi-view consistency filter and
// the visual hull of the reference's initialisation (run/train_ft.py:96-146).  Replaces
//   reproject_with_depth_gpu / check_geometric_consistency_gpu   models/mvs/filter_utils.py:157-218   (k_geo_consistency)
//   filter_by_masks_gpu, reassign_conf, range_mask_torch         models/mvs/filter_utils.py:222-297, 146-154   (k_fuse_flag / k_fuse_write)
//   alpha_masking                                                models/mvs/mvs_utils.py:573-607      (k_alpha_hull)
// The reference checks every view against every other view with ~40 element-wise launches and as many [H,W] temporaries per pair; here the
// loop over the source views runs inside the thread: one launch for all V (V - 1) pairs, no temporaries, no atomics.
// k_geo_consistency: one thread per reference pixel, the reference view is blockIdx.y (the pair table of (r, s) is wave-uniform: it comes
// through the constant cache), a wave is an 8 x 8 pixel tile (neighbouring pixels project to neighbouring texels of the source map: the four
// gathers of a bilinear sample touch a few lines), a workgroup four tiles side by side.  HBM: the V maps are read once by their own view and
// gathered (L2-resident at these sizes) by the others; 8 B written per pixel.  The pair tables fold the intrinsics into E_s E_r^-1
// (host, float64, rounded once): 2 x (9 + 3) multiply-adds per direction instead of four 3 x 3 / 4 x 4 products.
// Selection: flags -> scan.hip's compaction (ascending index = view-major, row-major = the order of the reference's boolean indexing) ->
// one thread per kept pixel.  Bit-reproducible.  fp32, no FMA contraction (built with -ffp-contract=off): the tests are threshold decisions.
#include "pn_common.h"

namespace {
constexpr int DF_PAIR = PNERF_DF_PAIR_FLOATS;

// F.grid_sample(bilinear, padding_mode='border', align_corners=True) of one [H,W] map at the PIXEL position (x, y): the reference's
// normalisation x * 2 / (W - 1) - 1 (:182) and grid_sample's inverse of it cancel.  NaN clamps to 0 (the caller's own arithmetic on x, y
// keeps the NaN and fails the comparisons); the corner weights are torch's (x_se - x, x - x_nw).
__device__ __forceinline__ float df_sample(const float *__restrict__ img, int H, int W, float x, float y) {
    const float xc = fminf(fmaxf(x, 0.f), (float)(W - 1)), yc = fminf(fmaxf(y, 0.f), (float)(H - 1));
    const float xw = floorf(xc), yn = floorf(yc);
    const int ix = (int)xw, iy = (int)yn;
    const int ix1 = ix + 1 < W ? ix + 1 : ix, iy1 = iy + 1 < H ? iy + 1 : iy;       // (the clamped corner carries weight 0)
    const float w = xc - xw, e = (xw + 1.f) - xc, n = yc - yn, s = (yn + 1.f) - yc;
    const float nw = img[(long long)iy * W + ix], ne = img[(long long)iy * W + ix1];
    const float sw = img[(long long)iy1 * W + ix], se = img[(long long)iy1 * W + ix1];
    return ((nw * (e * s) + ne * (w * s)) + sw * (e * n)) + se * (w * n);
}

// pair table of (reference r, source s), DF_PAIR floats:
//   [0..8]   A = K_s R_sr K_r^-1     [9..11]  b = K_s t_sr      (E_s E_r^-1 = [R_sr t_sr]):   K_s xyz_src = d_ref A [x y 1]^T + b
//   [12..20] B = K_r R_rs K_s^-1     [21..23] c = K_r t_rs      (E_r E_s^-1 = [R_rs t_rs]):   K_r xyz_rep = d_src B [x_src y_src 1]^T + c
//   [24..26] D = row 2 of R_rs K_s^-1, [27] e = t_rs[2]:         depth_reprojected = d_src D [x_src y_src 1]^T + e
__global__ __launch_bounds__(256) void k_geo_consistency(const float *__restrict__ depth, const float *__restrict__ pairs, int V, int H, int W,
                                                         int tiles_x, int *__restrict__ geo_mask_sum, float *__restrict__ depth_avg) {
    const int r = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const int px = bx * 32 + wave * 8 + (lane & 7), py = by * 8 + (lane >> 3);
    if (px >= W || py >= H) return;
    const long long HW = (long long)H * W, pix = (long long)py * W + px;
    const float d_ref = depth[r * HW + pix];
    const float xf = (float)px, yf = (float)py;
    float sum = 0.f;
    int cnt = 0;
    for (int s = 0; s < V; ++s) {
        if (s == r) continue;
        const float *__restrict__ T = pairs + ((long long)r * V + s) * DF_PAIR;
        const float X = ((T[0] * xf + T[1] * yf) + T[2]) * d_ref + T[9];
        const float Y = ((T[3] * xf + T[4] * yf) + T[5]) * d_ref + T[10];
        const float Z = ((T[6] * xf + T[7] * yf) + T[8]) * d_ref + T[11];
        const float x_src = X / Z, y_src = Y / Z;                                                           // :172
        const float d_src = df_sample(depth + s * HW, H, W, x_src, y_src);                                  // :182
        const float Xr = ((T[12] * x_src + T[13] * y_src) + T[14]) * d_src + T[21];
        const float Yr = ((T[15] * x_src + T[16] * y_src) + T[17]) * d_src + T[22];
        const float Zr = ((T[18] * x_src + T[19] * y_src) + T[20]) * d_src + T[23];
        const float d_rep = ((T[24] * x_src + T[25] * y_src) + T[26]) * d_src + T[27];                      // :193
        const float dx = Xr / Zr - xf, dy = Yr / Zr - yf;                                                   // :195
        const float dist = sqrtf(dx * dx + dy * dy);                                                        // :209
        const float rel = fabsf(d_rep - d_ref) / d_ref;                                                     // :212-213
        if (dist < 1.f && rel < 0.01f) { ++cnt; sum += d_rep; }                                             // :215-216, :256-257 (NaN / inf fail)
    }
    geo_mask_sum[r * HW + pix] = cnt;
    depth_avg[r * HW + pix] = (sum + d_ref) / (float)(cnt + 1);                                             // :259
}

struct FuseArgs {
    const int *geo; const float *avg, *cam, *conf; const unsigned char *pmask; const float *inv_ext;
    long long HW, n;
    float thresh; int cnsst, use_geo, has_factor, has_ranges;
    float factor[10], ranges[6];
};

// the kept-or-dropped decision of pixel i and, for a kept one, what is written for it
__device__ __forceinline__ bool fuse_point(const FuseArgs &a, long long i, float cam3[3], float world3[3], float &conf, int &view) {
    const float c = a.conf[i];
    const int g = a.geo[i];
    if (!(c > a.thresh) || !a.pmask[i] || (a.use_geo && g < a.cnsst)) return false;                         // :261-263
    view = (int)(i / a.HW);
    cam3[0] = a.cam[3 * i]; cam3[1] = a.cam[3 * i + 1]; cam3[2] = a.avg[i];                                 // :264-265 (x, y are not rescaled)
    const float *M = a.inv_ext + 16 * view;                                                                 // :282 [xyz 1] @ inv(E)^T
    for (int j = 0; j < 3; ++j) world3[j] = ((cam3[0] * M[4 * j] + cam3[1] * M[4 * j + 1]) + cam3[2] * M[4 * j + 2]) + M[4 * j + 3];
    if (a.has_ranges)                                                                                       // :146-154
        for (int j = 0; j < 3; ++j)
            if (!(world3[j] >= a.ranges[j] && world3[j] <= a.ranges[3 + j])) return false;
    conf = c;
    if (a.has_factor) {                                                                                     // :294-297, the host's table of 1 - 1 / 1.14869^k
        int k = g - a.cnsst + 1;
        k = k < 1 ? 1 : (k > 10 ? 10 : k);
        conf = c * a.factor[k - 1];
    }
    return true;
}

__global__ void k_fuse_flag(FuseArgs a, int *__restrict__ flags) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    float cam3[3], world3[3], conf; int view;
    flags[i] = fuse_point(a, i, cam3, world3, conf, view) ? 1 : 0;
}

__global__ void k_fuse_write(FuseArgs a, const int *__restrict__ list, const int *__restrict__ count, float *__restrict__ xyz_cam,
                             float *__restrict__ xyz_world, float *__restrict__ conf_out, int *__restrict__ view_id) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n || t >= *count) return;
    float cam3[3], world3[3], conf = 0.f; int view = 0;
    fuse_point(a, list[t], cam3, world3, conf, view);
    for (int j = 0; j < 3; ++j) { xyz_cam[3 * t + j] = cam3[j]; xyz_world[3 * t + j] = world3[j]; }
    conf_out[t] = conf;
    view_id[t] = view;
}

// one thread per point, the views inside: AND over the views of (alpha at the floored, clamped pixel (+ 1 outside the image) > 0.1) [and near / far]
__global__ void k_alpha_hull(const float *__restrict__ pts, long long n, const float *__restrict__ alphas, const float *__restrict__ w2c,
                             const float *__restrict__ intr, int V, int H, int W, int use_range, int has_nf, float near_m1, float far,
                             unsigned char *__restrict__ mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    bool keep = true;
    for (int v = 0; v < V; ++v) {
        const float *M = w2c + 16 * v, *K = intr + 9 * v;
        float c[3], q[3];
        for (int j = 0; j < 3; ++j) c[j] = ((x * M[4 * j] + y * M[4 * j + 1]) + z * M[4 * j + 2]) + M[4 * j + 3];          // :581
        for (int j = 0; j < 3; ++j) q[j] = (c[0] * K[3 * j] + c[1] * K[3 * j + 1]) + c[2] * K[3 * j + 2];                  // :585
        const float fx = floorf(q[0] / q[2] + 0.0f), fy = floorf(q[1] / q[2] + 0.0f);                                      // :586
        const bool inside = fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H;                                      // :590-591
        const int ix = fx >= (float)(W - 1) ? W - 1 : (fx > 0.f ? (int)fx : 0);                                            // :593-594 (NaN -> 0)
        const int iy = fy >= (float)(H - 1) ? H - 1 : (fy > 0.f ? (int)fy : 0);
        float m = alphas[((long long)v * H + iy) * W + ix];                                                                // :595
        if (use_range && !inside) m = m + 1.f;                                                                             // :596-597
        bool ok = m > 0.1f;                                                                                                // :598
        if (has_nf) ok = ok && c[2] >= near_m1 && c[2] <= far;                                                             // :584, :600
        keep = keep && ok;
    }
    mask[i] = keep ? 1 : 0;
}

struct FuseLayout { size_t flags, list, scan, total; };
FuseLayout fuse_layout(long long n) {
    PnCarver cv(nullptr);
    FuseLayout L;
    L.flags = cv.off; cv.take<int>((size_t)n);
    L.list = cv.off; cv.take<int>((size_t)n);
    L.scan = cv.off; cv.take<int>(pn_scan_scratch_ints(n));
    L.total = cv.off;
    return L;
}
// all views one size, at least 2 x 2 (the bilinear sample divides by nothing, but the reference's normalisation does: W - 1, H - 1)
int df_shape(const int32_t *view_hw_host, int V, int &H, int &W) {
    if (!view_hw_host || V < 1) return PNERF_E_INVAL;
    H = view_hw_host[0]; W = view_hw_host[1];
    if (H < 2 || W < 2) return PNERF_E_INVAL;
    for (int v = 1; v < V; ++v)
        if (view_hw_host[2 * v] != H || view_hw_host[2 * v + 1] != W) return PNERF_E_UNSUP;
    if (V > 65535 || (long long)V * H * W > 0x7fffff00LL) return PNERF_E_UNSUP;
    return 0;
}
}  // namespace

extern "C" int pnerf_depth_consistency(const float *d_depth, const int32_t *view_hw_host, int V, const float *d_pairs, int32_t *d_geo_mask_sum,
                                       float *d_depth_avg, void *stream) {
    int H = 0, W = 0;
    const int rc = df_shape(view_hw_host, V, H, W);
    if (rc) return rc;
    if (!d_depth || !d_pairs || !d_geo_mask_sum || !d_depth_avg) return PNERF_E_INVAL;
    const int tiles_x = pn_cdiv(W, 32), tiles_y = pn_cdiv(H, 8);
    hipLaunchKernelGGL(k_geo_consistency, dim3(tiles_x * tiles_y, V), dim3(256), 0, (hipStream_t)stream, d_depth, d_pairs, V, H, W, tiles_x,
                       d_geo_mask_sum, d_depth_avg);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t pnerf_depth_fuse_select_workspace_bytes(int V, int H, int W) {
    if (V < 1 || H < 2 || W < 2 || (long long)V * H * W > 0x7fffff00LL) return 0;
    return fuse_layout((long long)V * H * W).total;
}

extern "C" int pnerf_depth_fuse_select(const int32_t *d_geo_mask_sum, const float *d_depth_avg, const float *d_cam_xyz, const float *d_confidence,
                                       const uint8_t *d_points_mask, const float *d_inv_ext, int V, int H, int W, float depth_conf_thresh,
                                       int geo_cnsst_num, const float *conf_factor10_host, const float *ranges6_host, float *d_xyz_cam,
                                       float *d_xyz_world, float *d_conf_out, int32_t *d_view_id, int32_t *d_count, void *d_ws, size_t ws_bytes,
                                       void *stream) {
    if (V < 1 || H < 2 || W < 2) return PNERF_E_INVAL;
    if (!d_geo_mask_sum || !d_depth_avg || !d_cam_xyz || !d_confidence || !d_points_mask || !d_inv_ext || !d_xyz_cam || !d_xyz_world ||
        !d_conf_out || !d_view_id || !d_count || !d_ws) return PNERF_E_INVAL;
    if ((long long)V * H * W > 0x7fffff00LL) return PNERF_E_UNSUP;
    FuseArgs a;
    a.HW = (long long)H * W; a.n = a.HW * V;
    const FuseLayout L = fuse_layout(a.n);
    if (ws_bytes < L.total) return PNERF_E_WS;
    a.geo = d_geo_mask_sum; a.avg = d_depth_avg; a.cam = d_cam_xyz; a.conf = d_confidence; a.pmask = d_points_mask; a.inv_ext = d_inv_ext;
    a.thresh = depth_conf_thresh; a.cnsst = geo_cnsst_num; a.use_geo = V > 1 ? 1 : 0;                       // :263 (one view: no geometric clause)
    a.has_factor = conf_factor10_host ? 1 : 0; a.has_ranges = ranges6_host ? 1 : 0;
    for (int k = 0; k < 10; ++k) a.factor[k] = conf_factor10_host ? conf_factor10_host[k] : 1.f;
    for (int k = 0; k < 6; ++k) a.ranges[k] = ranges6_host ? ranges6_host[k] : 0.f;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)d_ws;
    int *flags = (int *)(ws + L.flags), *list = (int *)(ws + L.list), *scan = (int *)(ws + L.scan);
    const int nb = pn_cdiv(a.n, 256);
    hipLaunchKernelGGL(k_fuse_flag, dim3(nb), dim3(256), 0, s, a, flags);
    const int rc = pn_compact_gt0_i32(flags, a.n, list, d_count, scan, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_fuse_write, dim3(nb), dim3(256), 0, s, a, list, d_count, d_xyz_cam, d_xyz_world, d_conf_out, d_view_id);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_alpha_hull(const float *d_points, int64_t n_points, const float *d_alphas, const float *d_w2c, const float *d_intrinsics, int V,
                                int H, int W, int use_range_mask, const float *near_far2_host, uint8_t *d_mask, void *stream) {
    if (V < 1 || H < 1 || W < 1 || n_points < 0) return PNERF_E_INVAL;
    if (n_points == 0) return 0;
    if (!d_points || !d_alphas || !d_w2c || !d_intrinsics || !d_mask) return PNERF_E_INVAL;
    if (n_points / 256 >= 0x7fffffffLL || (long long)V * H * W > 0x7fffff00LL) return PNERF_E_UNSUP;
    hipLaunchKernelGGL(k_alpha_hull, dim3(pn_cdiv(n_points, 256)), dim3(256), 0, (hipStream_t)stream, d_points, (long long)n_points, d_alphas, d_w2c,
                       d_intrinsics, V, H, W, use_range_mask ? 1 : 0, near_far2_host ? 1 : 0, near_far2_host ? near_far2_host[0] : 0.f,
                       near_far2_host ? near_far2_host[1] : 0.f, d_mask);
    PN_CHECK_LAUNCH();
    return 0;
}
