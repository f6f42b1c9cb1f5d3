// metrics.hip -- the image scores of the reference's evaluation (run/evaluate.py:55-61,76 report_metrics: PSNR / SSIM / RMSE over the
// 8-bit PNGs that utils/visualizer.py:58-59 wrote) on the device: one pass over a rendered image and its ground truth gives the sum of
// squared differences and, per colour channel, the sum of the SSIM map over the valid window positions.
//
// SSIM restates skimage's structural_similarity(gt, img, win_size=win, multichannel=True) in its uniform-filter form (what the
// reference's call resolves to): five window means per position, sample covariance (NP / (NP - 1)), and
//   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  C1 = (0.01 R)^2, C2 = (0.03 R)^2.
// skimage filters with reflected borders and crops (win - 1) / 2 pixels before averaging: only windows fully inside the image
// contribute, so there is no border handling here.
//
// Arithmetic: float64 from the float32 (optionally 8-bit quantised) pixels -- the pass is memory-light (2 x 7.7 MB for 800^2) and fp64
// removes the cancellation in uxx - ux^2 on flat backgrounds.  No FMA contraction (the pragma below): for identical images numerator and
// denominator of S are then the same roundings and S is exactly 1.  No float atomics: one partial per tile and quantity, added by a
// single workgroup in a fixed order, so two calls on the same inputs give the same bits.
//
// Shape: one 256-thread workgroup per PN_IM_T x PN_IM_T tile of window positions.  The tile plus its win - 1 halo of both images (all
// three channels, interleaved as in memory) is staged through LDS; then per channel a horizontal pass of running sums (each item: one
// row, PN_IM_SEG consecutive positions: one full window, then add the entering and drop the leaving pixel) writes five float64 planes
// [S][T], and a vertical pass of running sums over those planes ends in the SSIM formula.
#include "pn_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int PN_IM_T = 16;        // tile edge in window positions (tests/test_gpu_image_metrics.py places image edges around it)
constexpr int PN_IM_SEG = 4;       // positions per running-sum item, both passes
constexpr int PN_IM_TPB = 256;
constexpr int PN_IM_WIN_MAX = 25;  // LDS of the tile: (5 S T + 16) * 8 + 6 S^2 * 4 bytes, S = T + win - 1: 64 128 bytes at win = 25

static inline size_t pn_im_lds_bytes(int win) {
    const size_t S = PN_IM_T + win - 1;
    return (5 * S * PN_IM_T + 16) * sizeof(double) + 6 * S * S * sizeof(float);
}

// what the reference's PNG round trip does to a pixel (utils/visualizer.py:58-59 writes uint8(clip(x, 0, 1) * 255): truncation;
// run/evaluate.py:55 reads it back as float32 / 255).  A NaN pixel becomes 0.
__device__ __forceinline__ float pn_im_pixel(float v, int quantize8) {
    if (!quantize8) return v;
    const float c = fminf(fmaxf(v, 0.f), 1.f) * 255.f;
    return (float)(int)c / 255.f;
}

// sum of v[0..3] over the workgroup in a fixed order (xor butterfly inside each wave, then the four waves in index order): thread q < 4
// RETURNS the total of quantity q (the other threads return 0; v[] is left holding the wave's sums).  red: 16 doubles of LDS.
__device__ __forceinline__ double pn_im_block_sum4(double v[4], double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off, 64);
    if (lane == 0)
        for (int q = 0; q < 4; ++q) red[wave * 4 + q] = v[q];
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x < 4)
        for (int w = 0; w < PN_IM_TPB / 64; ++w) tot += red[w * 4 + threadIdx.x];
    return tot;
}

__global__ __launch_bounds__(PN_IM_TPB) void k_image_metrics(const float *__restrict__ img, const float *__restrict__ gt, int H, int W, int win,
                                                             double C1, double C2, int quantize8, double *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) double pn_im_lds[];
    constexpr int T = PN_IM_T, SEG = PN_IM_SEG;
    const int S = T + win - 1, S3 = S * 3;
    double *hs = pn_im_lds;                              // [5][S][T]
    double *red = hs + 5 * S * T;                        // [16]
    float *px = (float *)(red + 16);                     // [S][S][3] img
    float *py = px + S * S3;                             // [S][S][3] gt
    const int OH = H - win + 1, OW = W - win + 1;
    const int y0 = blockIdx.y * T, x0 = blockIdx.x * T;
    const bool last_y = blockIdx.y == gridDim.y - 1, last_x = blockIdx.x == gridDim.x - 1;
    const int tid = threadIdx.x;

    // ---- stage the tile and its halo (zeros outside the image: only masked positions read them); the squared differences of the pixels
    // this tile owns (its first T rows / columns, and the halo too on the last tile row / column: every pixel of the image exactly once)
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                // sse, ssim sum of channels 0..2
    for (int i = tid; i < S * S3; i += PN_IM_TPB) {
        const int r = i / S3, k = i - r * S3, col = k / 3;
        const int gy = y0 + r, gx = x0 + col;
        float a = 0.f, b = 0.f;
        if (gy < H && gx < W) {
            const size_t g = ((size_t)gy * W + x0) * 3 + k;
            a = pn_im_pixel(img[g], quantize8);
            b = pn_im_pixel(gt[g], quantize8);
            if ((r < T || last_y) && (col < T || last_x)) {
                const double d = (double)a - (double)b;
                acc[0] += d * d;
            }
        }
        px[i] = a;
        py[i] = b;
    }
    __syncthreads();

    const double NP = (double)(win * win), cov = NP / (NP - 1.0);
    const int plane = S * T;
    for (int c = 0; c < 3; ++c) {
        double ssum = 0.0;
        // ---- horizontal: hs[q][r][j] = sum over the win pixels right of column j of row r (q: x, y, xx, yy, xy)
        for (int item = tid; item < S * (T / SEG); item += PN_IM_TPB) {
            const int r = item / (T / SEG), j0 = (item - r * (T / SEG)) * SEG;
            const float *rx = px + r * S3 + c, *ry = py + r * S3 + c;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
            for (int j = j0; j < j0 + win; ++j) {
                const double x = (double)rx[3 * j], y = (double)ry[3 * j];
                sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
            }
            double *o = hs + r * T + j0;
            for (int s = 0;; ++s) {
                o[s] = sx; o[plane + s] = sy; o[2 * plane + s] = sxx; o[3 * plane + s] = syy; o[4 * plane + s] = sxy;
                if (s == SEG - 1) break;
                const double xn = (double)rx[3 * (j0 + s + win)], yn = (double)ry[3 * (j0 + s + win)];
                const double xo = (double)rx[3 * (j0 + s)], yo = (double)ry[3 * (j0 + s)];
                sx += xn; sy += yn; sxx += xn * xn; syy += yn * yn; sxy += xn * yn;
                sx -= xo; sy -= yo; sxx -= xo * xo; syy -= yo * yo; sxy -= xo * yo;
            }
        }
        __syncthreads();
        // ---- vertical: window sums of position (i, j) = sum over rows i .. i + win - 1 of hs[.][.][j]; then the formula
        for (int item = tid; item < T * (T / SEG); item += PN_IM_TPB) {
            const int j = item % T, i0 = (item / T) * SEG;
            const double *p = hs + j;
            double sm[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (int i = i0; i < i0 + win; ++i)
                for (int q = 0; q < 5; ++q) sm[q] += p[q * plane + i * T];
            for (int s = 0;; ++s) {
                if (y0 + i0 + s < OH && x0 + j < OW) {
                    const double ux = sm[0] / NP, uy = sm[1] / NP, uxx = sm[2] / NP, uyy = sm[3] / NP, uxy = sm[4] / NP;
                    const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
                    const double num = (2.0 * (ux * uy) + C1) * (2.0 * vxy + C2);
                    const double den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
                    ssum += num / den;
                }
                if (s == SEG - 1) break;
                for (int q = 0; q < 5; ++q) {
                    sm[q] += p[q * plane + (i0 + s + win) * T];
                    sm[q] -= p[q * plane + (i0 + s) * T];
                }
            }
        }
        if (c == 0) acc[1] = ssum; else if (c == 1) acc[2] = ssum; else acc[3] = ssum;      // (constant indices: acc stays in registers)
        __syncthreads();
    }

    const double tot = pn_im_block_sum4(acc, red);
    const int ntiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
    if (tid < 4) partial[(size_t)tid * ntiles + tile] = tot;
}

// one workgroup: out4[q] = sum of partial[q][0 .. ntiles) (thread t adds tiles t, t + 256, ... in ascending order, then the fixed
// workgroup order of pn_im_block_sum4)
__global__ __launch_bounds__(PN_IM_TPB) void k_image_metrics_sum(const double *__restrict__ partial, int ntiles, double *__restrict__ out4) {
    __shared__ double red[16];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < ntiles; i += PN_IM_TPB)
        for (int q = 0; q < 4; ++q) acc[q] += partial[(size_t)q * ntiles + i];
    const double tot = pn_im_block_sum4(acc, red);
    if (threadIdx.x < 4) out4[threadIdx.x] = tot;
}

static inline bool pn_im_args_ok(int H, int W, int win) { return win >= 3 && (win & 1) && H >= win && W >= win; }
// tiles of window positions along x and y; false where the grid or the tile count would not fit (65 535 tile rows, 2^31 - 1 tiles)
static inline bool pn_im_tiles(int H, int W, int win, int &ntx, int &nty) {
    ntx = pn_cdiv(W - win + 1, PN_IM_T); nty = pn_cdiv(H - win + 1, PN_IM_T);
    return nty <= 65535 && (long long)ntx * nty <= 0x7fffffffLL;
}
}  // namespace

extern "C" size_t pnerf_image_metrics_workspace_bytes(int H, int W, int win) {
    if (!pn_im_args_ok(H, W, win)) return 0;
    int ntx, nty;
    if (!pn_im_tiles(H, W, win, ntx, nty)) return 0;
    return pn_align((size_t)ntx * nty * 4 * sizeof(double));
}

extern "C" int pnerf_image_metrics(const float *d_img, const float *d_gt, int H, int W, int win, double data_range, int quantize8,
                                   double *d_out4, void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_img || !d_gt || !d_out4 || !d_ws || !pn_im_args_ok(H, W, win) || !(data_range > 0.0)) return PNERF_E_INVAL;
    if (win > PN_IM_WIN_MAX) return PNERF_E_UNSUP;
    int ntx, nty;
    if (!pn_im_tiles(H, W, win, ntx, nty)) return PNERF_E_UNSUP;
    if (ws_bytes < pnerf_image_metrics_workspace_bytes(H, W, win)) return PNERF_E_WS;
    const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_image_metrics, dim3(ntx, nty), dim3(PN_IM_TPB), pn_im_lds_bytes(win), s, d_img, d_gt, H, W, win, C1, C2,
                       quantize8 ? 1 : 0, (double *)d_ws);
    hipLaunchKernelGGL(k_image_metrics_sum, dim3(1), dim3(PN_IM_TPB), 0, s, (const double *)d_ws, ntx * nty, d_out4);
    PN_CHECK_LAUNCH();
    return 0;
}
