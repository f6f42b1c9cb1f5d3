// mvsdepth.hip -- from images to one depth map per view: the two fused stages of the pretrained MVSNet that every per-scene script of the
// reference runs first (manual_depth_view=1), and the tail of gen_points that turns a depth map into camera-space candidates.  Replaces
//   homo_warping + the variance lines            models/depth_estimators/module.py:36-70, mvsnet.py:110-122      (k_cost_volume)
//   softmax, two depth_regression, pad + avg_pool3d + gather   mvsnet.py:127-136, module.py:73-78                (k_depth_regress)
//   F.interpolate(nearest), gau_single_sampler, depth2point, ndc_2_cam   models/mvs/mvs_points_model.py:329-337, 152-157, 171-182,
//                                                                        models/mvs/mvs_utils.py:92-98           (k_depth_to_points)
// The reference materialises one warped volume [B,32,D,h,w] per source view and runs a dozen element-wise passes over them; here the loop
// over the views runs inside the thread and the variance volume is written once.
// k_cost_volume: the feature maps are first transposed to channels-last (k_channels_last: a few MB, once per call), so that a bilinear tap
// is 64 contiguous bytes per lane (16 channels).  One thread per output voxel (b, d, pixel) and channel half; lanes run along the flattened
// pixel index of one (b, c, d) plane, so every store of one channel is one contiguous segment of the output.  Offsets into the volume are
// 64-bit.  No atomics, no temporaries: bit-reproducible.
// k_depth_regress: one thread per pixel, lanes along the flattened pixel index; ONE pass over the D logits with a running maximum (online
// softmax: the three sums are rescaled when the maximum moves) plus four re-reads for the confidence window; the probability volume is
// written by a second pass only when it is asked for.
// fp32, no FMA contraction (built with -ffp-contract=off): the arithmetic rounds like the reference's separate tensor operations.
#include "pn_common.h"

namespace {
constexpr int MV_C = 32;          // feature channels of MVSNet's FeatureNet (mvsnet.py:21)
constexpr int MV_CG = 16;         // channels per thread

// [n, 32, hw] -> [n, hw, 32]: a 32 x 64 tile through LDS, both sides coalesced
__global__ __launch_bounds__(256) void k_channels_last(const float *__restrict__ src, float *__restrict__ dst, long long hw) {
    __shared__ float tile[64][MV_C + 1];
    const long long n = blockIdx.y, p0 = (long long)blockIdx.x * 64;
    const float *__restrict__ s = src + n * MV_C * hw;
    float *__restrict__ d = dst + n * MV_C * hw;
    const int t = threadIdx.x;
    for (int i = 0; i < 8; ++i) {
        const int c = (t >> 6) + 4 * i, p = t & 63;
        if (p0 + p < hw) tile[p][c] = s[(long long)c * hw + p0 + p];
    }
    __syncthreads();
    for (int i = 0; i < 8; ++i) {
        const int p = (t >> 5) + 8 * i, c = t & 31;
        if (p0 + p < hw) d[(p0 + p) * MV_C + c] = tile[p][c];
    }
}

// grid_sample's un-normalisation of one coordinate (ATen grid_sampler_unnormalize)
__device__ __forceinline__ float mv_unnormalize(float g, int size, int align_corners) {
    return align_corners ? ((g + 1.f) / 2.f) * (float)(size - 1) : ((g + 1.f) * (float)size - 1.f) / 2.f;
}

__global__ __launch_bounds__(256) void k_cost_volume(const float *__restrict__ feats_cl, long long feat_set_stride, const float *__restrict__ proj,
                                                     const float *__restrict__ depth_values, int V, int D, int h, int w, int align_corners,
                                                     float *__restrict__ volume) {
    const long long hw = (long long)h * w;
    const long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= hw) return;
    const int d = blockIdx.y >> 1, cg = (blockIdx.y & 1) * MV_CG, b = blockIdx.z;
    const int y = (int)(pix / w), x = (int)(pix - (long long)y * w);
    const float xf = (float)x, yf = (float)y;
    const float depth = depth_values[(long long)b * D + d];
    const float half_w = (float)(w - 1) / 2.f, half_h = (float)(h - 1) / 2.f;                              // module.py:61-62
    float sum[MV_CG], sq[MV_CG];
    for (int c = 0; c < MV_CG; ++c) { sum[c] = 0.f; sq[c] = 0.f; }
    for (int v = 0; v < V; ++v) {
        const float *__restrict__ P = proj + ((long long)b * V + v) * 12;                                   // [3,4]: rot | trans, wave-uniform
        const float X = (((P[0] * xf + P[1] * yf) + P[2]) * depth) + P[3];                                  // :56-59
        const float Y = (((P[4] * xf + P[5] * yf) + P[6]) * depth) + P[7];
        const float Z = (((P[8] * xf + P[9] * yf) + P[10]) * depth) + P[11];
        const float gx = (X / Z) / half_w - 1.f, gy = (Y / Z) / half_h - 1.f;                               // :60-62
        const float ix = mv_unnormalize(gx, w, align_corners), iy = mv_unnormalize(gy, h, align_corners);
        // a position with no tap inside the map (NaN and infinities included: every comparison fails) contributes exactly zero; inside this
        // test ix in (-1, w) and iy in (-1, h), so the conversions below are defined
        if (!(ix > -1.f && ix < (float)w && iy > -1.f && iy < (float)h)) continue;
        const float x0f = floorf(ix), y0f = floorf(iy);
        const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
        const float wx1 = ix - x0f, wx0 = (x0f + 1.f) - ix, wy1 = iy - y0f, wy0 = (y0f + 1.f) - iy;        // torch's corner weights
        const float wnw = wx0 * wy0, wne = wx1 * wy0, wsw = wx0 * wy1, wse = wx1 * wy1;
        const bool okx0 = x0 >= 0 && x0 < w, okx1 = x1 >= 0 && x1 < w, oky0 = y0 >= 0 && y0 < h, oky1 = y1 >= 0 && y1 < h;
        const float *__restrict__ F = feats_cl + (long long)b * feat_set_stride + (long long)v * hw * MV_C + cg;
        float s[MV_CG];
        for (int c = 0; c < MV_CG; ++c) s[c] = 0.f;
        if (okx0 && oky0) {
            const float4 *__restrict__ q = (const float4 *)(F + ((long long)y0 * w + x0) * MV_C);
            for (int k = 0; k < MV_CG / 4; ++k) { const float4 t = q[k]; s[4 * k] += t.x * wnw; s[4 * k + 1] += t.y * wnw; s[4 * k + 2] += t.z * wnw; s[4 * k + 3] += t.w * wnw; }
        }
        if (okx1 && oky0) {
            const float4 *__restrict__ q = (const float4 *)(F + ((long long)y0 * w + x1) * MV_C);
            for (int k = 0; k < MV_CG / 4; ++k) { const float4 t = q[k]; s[4 * k] += t.x * wne; s[4 * k + 1] += t.y * wne; s[4 * k + 2] += t.z * wne; s[4 * k + 3] += t.w * wne; }
        }
        if (okx0 && oky1) {
            const float4 *__restrict__ q = (const float4 *)(F + ((long long)y1 * w + x0) * MV_C);
            for (int k = 0; k < MV_CG / 4; ++k) { const float4 t = q[k]; s[4 * k] += t.x * wsw; s[4 * k + 1] += t.y * wsw; s[4 * k + 2] += t.z * wsw; s[4 * k + 3] += t.w * wsw; }
        }
        if (okx1 && oky1) {
            const float4 *__restrict__ q = (const float4 *)(F + ((long long)y1 * w + x1) * MV_C);
            for (int k = 0; k < MV_CG / 4; ++k) { const float4 t = q[k]; s[4 * k] += t.x * wse; s[4 * k + 1] += t.y * wse; s[4 * k + 2] += t.z * wse; s[4 * k + 3] += t.w * wse; }
        }
        for (int c = 0; c < MV_CG; ++c) { sum[c] += s[c]; sq[c] += s[c] * s[c]; }                          // mvsnet.py:119-120
    }
    const float nv = (float)V;
    float *__restrict__ out = volume + (((long long)b * MV_C + cg) * D + d) * hw + pix;
    for (int c = 0; c < MV_CG; ++c) {
        const float m = sum[c] / nv;
        out[(long long)c * D * hw] = sq[c] / nv - m * m;                                                    // :122
    }
}

__global__ __launch_bounds__(256) void k_depth_regress(const float *__restrict__ cost, const float *__restrict__ depth_values, int D, long long hw,
                                                       float *__restrict__ depth, float *__restrict__ conf, float *__restrict__ prob) {
    const long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= hw) return;
    const int b = blockIdx.y;
    const float *__restrict__ L = cost + (long long)b * D * hw + pix;
    const float *__restrict__ dv = depth_values + (long long)b * D;
    // the running maximum starts at -FLT_MAX: a logit of -inf adds exp(-inf) = 0, +inf or NaN make the sums NaN, as softmax does
    float m = -3.402823466e38f, S = 0.f, Sd = 0.f, Si = 0.f;
    for (int d = 0; d < D; ++d) {
        const float l = L[(long long)d * hw];
        if (l > m) {                                                     // the maximum moves: rescale what is summed so far
            const float r = expf(m - l);
            S = S * r; Sd = Sd * r; Si = Si * r;
            m = l;
        }
        const float e = expf(l - m);
        S += e; Sd += e * dv[d]; Si += e * (float)d;
    }
    depth[(long long)b * hw + pix] = Sd / S;                             // depth_regression (module.py:73-78)
    const float fi = Si / S;                                             // mvsnet.py:135, .long() truncates
    int idx = fi >= (float)(D - 1) ? D - 1 : (fi > 0.f ? (int)fi : 0);   // clamped before the conversion; NaN -> 0
    float c4 = 0.f;                                                      // :134, :136: p[idx-1] + p[idx] + p[idx+1] + p[idx+2], zeros outside
    for (int j = idx - 1; j <= idx + 2; ++j)
        if (j >= 0 && j < D) c4 += expf(L[(long long)j * hw] - m) / S;
    conf[(long long)b * hw + pix] = c4;
    if (prob) {
        float *__restrict__ Pv = prob + (long long)b * D * hw + pix;
        for (int d = 0; d < D; ++d) Pv[(long long)d * hw] = expf(L[(long long)d * hw] - m) / S;
    }
}

// F.interpolate(mode='nearest')'s source index (ATen nearest_neighbor_compute_source_index; scale = (float)in / out, formed by the host)
__device__ __forceinline__ int mv_nearest(int dst, float scale, int in_size) {
    const int s = (int)floorf((float)dst * scale);
    return s < in_size - 1 ? s : in_size - 1;
}

struct D2PArgs { float near, far, scale_y, scale_x, M[9]; int h, w, H, W; };

__global__ __launch_bounds__(256) void k_depth_to_points(const float *__restrict__ depth_lr, const float *__restrict__ conf_lr, D2PArgs a,
                                                         float *__restrict__ cam_xyz, float *__restrict__ conf, unsigned char *__restrict__ mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)a.H * a.W) return;
    const int Y = (int)(i / a.W), X = (int)(i - (long long)Y * a.W);
    const long long src = (long long)mv_nearest(Y, a.scale_y, a.h) * a.w + mv_nearest(X, a.scale_x, a.w);  // mvs_points_model.py:329-331
    const float d = depth_lr[src];
    conf[i] = conf_lr[src];
    mask[i] = (d >= a.near && d <= a.far) ? 1 : 0;                                                        // :154
    const float range = a.far - a.near;
    float ndc = (d - a.near) / range;                                                                     // :155
    ndc = ndc < 0.f ? 0.f : (ndc > 1.f ? 1.f : ndc);                                                      // :168 (NaN stays NaN)
    const float cz = ndc * range + a.near;                                                                // mvs_utils.py:94
    const float cx = (((float)X / (float)(a.W - 1)) * (float)(a.W - 1)) * cz;                             // :174, mvs_utils.py:95
    const float cy = (((float)Y / (float)(a.H - 1)) * (float)(a.H - 1)) * cz;
    for (int j = 0; j < 3; ++j) cam_xyz[3 * i + j] = (cx * a.M[j] + cy * a.M[3 + j]) + cz * a.M[6 + j];   // mvs_utils.py:97: row @ inv(K^T)
}

int mv_volume_shape(int B, int V, int C, int D, int h, int w) {
    if (B < 1 || V < 1 || D < 1 || h < 2 || w < 2 || C < 1) return PNERF_E_INVAL;
    if (C != MV_C) return PNERF_E_UNSUP;
    if (B > 65535 || 2 * (long long)D > 65535 || (long long)h * w > 0x7fffff00LL) return PNERF_E_UNSUP;
    return 0;
}
}  // namespace

extern "C" size_t pnerf_mvs_cost_volume_workspace_bytes(int n_feat_sets, int V, int h, int w) {
    if (n_feat_sets < 1 || mv_volume_shape(1, V, MV_C, 1, h, w) || n_feat_sets > 65535) return 0;
    return pn_align((size_t)n_feat_sets * V * MV_C * h * w * sizeof(float));
}

extern "C" int pnerf_mvs_cost_volume(const float *d_feats, int n_feat_sets, const float *d_proj, const float *d_depth_values, int B, int V, int C,
                                     int D, int h, int w, int align_corners, float *d_volume, void *d_ws, size_t ws_bytes, void *stream) {
    const int rc = mv_volume_shape(B, V, C, D, h, w);
    if (rc) return rc;
    if (n_feat_sets != 1 && n_feat_sets != B) return PNERF_E_INVAL;
    if (!d_feats || !d_proj || !d_depth_values || !d_volume || !d_ws) return PNERF_E_INVAL;
    if (ws_bytes < pnerf_mvs_cost_volume_workspace_bytes(n_feat_sets, V, h, w)) return PNERF_E_WS;
    hipStream_t s = (hipStream_t)stream;
    const long long hw = (long long)h * w;
    float *cl = (float *)d_ws;
    if ((long long)n_feat_sets * V > 65535) return PNERF_E_UNSUP;
    hipLaunchKernelGGL(k_channels_last, dim3(pn_cdiv(hw, 64), n_feat_sets * V), dim3(256), 0, s, d_feats, cl, hw);
    hipLaunchKernelGGL(k_cost_volume, dim3(pn_cdiv(hw, 256), 2 * D, B), dim3(256), 0, s, (const float *)cl,
                       n_feat_sets == 1 ? 0LL : (long long)V * hw * MV_C, d_proj, d_depth_values, V, D, h, w, align_corners ? 1 : 0, d_volume);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_mvs_depth_regress(const float *d_cost_reg, const float *d_depth_values, int B, int D, int h, int w, float *d_depth,
                                       float *d_confidence, float *d_prob_volume, void *stream) {
    if (B < 1 || D < 1 || h < 1 || w < 1) return PNERF_E_INVAL;
    if (!d_cost_reg || !d_depth_values || !d_depth || !d_confidence) return PNERF_E_INVAL;
    if (B > 65535 || (long long)h * w > 0x7fffff00LL) return PNERF_E_UNSUP;
    const long long hw = (long long)h * w;
    hipLaunchKernelGGL(k_depth_regress, dim3(pn_cdiv(hw, 256), B), dim3(256), 0, (hipStream_t)stream, d_cost_reg, d_depth_values, D, hw, d_depth,
                       d_confidence, d_prob_volume);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_depth_to_cam_points(const float *d_depth_lr, const float *d_conf_lr, int h, int w, int H, int W, float near, float far,
                                         const float *inv_kt9_host, float *d_cam_xyz, float *d_confidence, uint8_t *d_mask, void *stream) {
    if (h < 1 || w < 1 || H < 2 || W < 2) return PNERF_E_INVAL;
    if (!d_depth_lr || !d_conf_lr || !inv_kt9_host || !d_cam_xyz || !d_confidence || !d_mask) return PNERF_E_INVAL;
    if ((long long)H * W > 0x7fffff00LL / 3 || (long long)h * w > 0x7fffff00LL) return PNERF_E_UNSUP;
    D2PArgs a;
    a.near = near; a.far = far; a.h = h; a.w = w; a.H = H; a.W = W;
    a.scale_y = (float)h / (float)H; a.scale_x = (float)w / (float)W;
    for (int k = 0; k < 9; ++k) a.M[k] = inv_kt9_host[k];
    hipLaunchKernelGGL(k_depth_to_points, dim3(pn_cdiv((long long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, d_depth_lr, d_conf_lr, a, d_cam_xyz,
                       d_confidence, d_mask);
    PN_CHECK_LAUNCH();
    return 0;
}
