// mlp_common.h -- layout of the aggregator / colour MLP parameters and the saved-activation area.  Every GEMM of the forward and
// of the dgrad chain runs on the f16 matrix pipe with two-plane operands: f16x3.h.
#pragma once
#include "pn_common.h"
#include <type_traits>
#include <utility>

// ---- architecture (reference viewmlp_init, models/aggregators/point_aggregators.py:276-348, lego flags)
#define PN_F      32                 // point_features_dim
#define PN_IN1    284                // 32 + 2*3*32 + 2*5*6
#define PN_IN1P   288                // padded to a multiple of 8 (zero columns)
#define PN_H      256                // shading_feature_num
#define PN_IN3    263                // 256 + colour 3 + (dir - view) 3 + dir.view 1
#define PN_INC    280                // 256 + view PE 24
#define PN_HC     128
#define PN_TILE   64                 // neighbor rows per aggregator tile (2 MFMA row tiles).  Measured: 32-row tiles are 10 % slower (twice the weight-fragment traffic per MFMA)
#define PN_MT     (PN_TILE / 32)
// Organisation of an aggregator workgroup (forward and backward tile kernels): 4 waves, each 2 feature blocks x 2 row blocks of the 64-row tile,
// two workgroups per CU, 4 threads per tile row in the row-wise phases.  It is the only one: an 8-wave organisation (one feature block per wave,
// roles split between waves 0..3 and 4..7) was built in round 4 and measured slower in the real kernels, forward 12.78 -> 14.56 ms, backward
// 13.85 -> 14.82 ms (profiles/r04_orgB_vs_orgA.txt); its source was last present in commit 0554797.
#define PN_NTHR   256                // threads of an aggregator workgroup
#define PN_NW     4                  // its waves
#define PN_NFB    2                  // 32-feature blocks per wave in the 256-wide GEMMs
static_assert(PN_NTHR == 64 * PN_NW && PN_NW == 4 && PN_NW * PN_NFB == 8, "the tile kernels are written for 4 waves x 2 of the 8 feature blocks each");
#define PN_TPR    (PN_NTHR / PN_TILE)     // threads per tile row in the row-wise phases
#define PN_EPT    (PN_F / PN_TPR)         // embedding dims per thread of a row (feature build, embedding gradient)
#define PN_CTILE  64                 // valid samples per colour-MLP tile

// flat parameter vector (state_dict order, torch [out,in] row-major)
enum : int {
    PO_W1 = 0, PO_B1 = PO_W1 + PN_H * PN_IN1, PO_W2 = PO_B1 + PN_H, PO_B2 = PO_W2 + PN_H * PN_H,
    PO_W3 = PO_B2 + PN_H, PO_B3 = PO_W3 + PN_H * PN_IN3, PO_W4 = PO_B3 + PN_H, PO_B4 = PO_W4 + PN_H * PN_H,
    PO_W5 = PO_B4 + PN_H, PO_B5 = PO_W5 + PN_H, PO_WC1 = PO_B5 + 1, PO_BC1 = PO_WC1 + PN_HC * PN_INC,
    PO_WC2 = PO_BC1 + PN_HC, PO_BC2 = PO_WC2 + PN_HC * PN_HC, PO_WC3 = PO_BC2 + PN_HC, PO_BC3 = PO_WC3 + PN_HC * PN_HC,
    PO_WC4 = PO_BC3 + PN_HC, PO_BC4 = PO_WC4 + 3 * PN_HC, PO_TOTAL = PO_BC4 + 3
};
static_assert(PO_TOTAL == 341764, "parameter count of the lego-script aggregator");

typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef float pn_f4 __attribute__((ext_vector_type(4)));
typedef float pn_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float pn_lrelu_grad(float post) { return post > 0.f ? 1.f : 0.01f; }

template <int... I, class F> __device__ __forceinline__ void pn_static_for_impl(std::integer_sequence<int, I...>, F &&f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> __device__ __forceinline__ void pn_static_for(F &&f) { pn_static_for_impl(std::make_integer_sequence<int, N>{}, f); }

// ---- small device helpers of the tile and colour kernels (aggregate.hip, backward.hip)
// v @ M (transpose = false: out_j = sum_i v_i M[i][j]) or v @ M^T (true: out_j = sum_i v_i M[j][i]), M row-major 3 x 3
__device__ __forceinline__ void rot3(const float *M, float x, float y, float z, bool transpose, float &ox, float &oy, float &oz) {
    if (!transpose) { ox = x * M[0] + y * M[3] + z * M[6]; oy = x * M[1] + y * M[4] + z * M[7]; oz = x * M[2] + y * M[5] + z * M[8]; }
    else { ox = x * M[0] + y * M[1] + z * M[2]; oy = x * M[3] + y * M[4] + z * M[5]; oz = x * M[6] + y * M[7] + z * M[8]; }
}
template <int N> __device__ __forceinline__ float group_sum(float v) {      // sum over N adjacent lanes (N = 4 or 8)
#pragma unroll
    for (int off = 1; off < N; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <int AF> __device__ __forceinline__ void pn_acc_zero(f32x16 (&acc)[AF][2]) {
#pragma unroll
    for (int i = 0; i < AF; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}
// softplus(x) = log(1 + e^x) (raw2out_density, networks.py:262-267) on the hardware exponential / logarithm: absolute error <= 2e-7 for
// x <= 20 (log of 1 + e^x, e^x >= 0: the argument is >= 1, v_log_f32 / v_exp_f32 are good to an ulp), the identity above; and its derivative
__device__ __forceinline__ float pn_softplus(float x) {
#ifdef PN_EMU
    return x > 20.f ? x : log1pf(expf(x));
#else
    return x > 20.f ? x : __logf(1.0f + __expf(x));
#endif
}
__device__ __forceinline__ float pn_sigmoid(float x) {
#ifdef PN_EMU
    return x > 20.f ? 1.f : 1.0f / (1.0f + expf(-x));
#else
    return x > 20.f ? 1.f : __builtin_amdgcn_rcpf(1.0f + __expf(-x));
#endif
}

// ---- saved-activation area (training) -------------------------------------------------------
struct PnSaved {
    // per neighbor row (rows = row tiles * 64):
    uint4 *x0k, *h1k, *h2k, *h3k;       // k-major [rows / 8][NF] inputs of the four layers (NF = 288, 256, 288, 256) as ONE f16 plane (round to nearest):
                                        // what the weight-gradient GEMM streams (x0k on the fused path: only X0's last 64 columns, [rows / 8][64] --
                                        // k_wgrad_x0 rebuilds the other 224)
    uint4 *dy1k, *dy2k, *dy3k, *dy4k;   // k-major [rows / 8][256] output gradients of the four layers (ONE f16 plane, round to nearest), SCALED by the backward's power-of-two scale
    uint4 *h4r;                         // row-major [2][rows][32] last activation, both planes (alpha head / K-weighted sums of the backward)
    float *arow;                        // per row: pre-activation of the alpha head
    int4 *rmeta;                        // per row: {sample id or -1, point id or -1, bits(normalised weight), bits(final weight)}
    unsigned *lmask;                    // [row tiles][3 layers h1..h3][8 feature blocks][64 lanes]: LeakyReLU sign bits in the accumulator layout
    unsigned *gscale;                   // [PN_GS_WORDS]: [0] bits of max |d decoded| over the valid samples (the backward derives its scale from it);
                                        // [PN_GS_CLAIM + class] the backward's tile claim counters
    // per valid sample (padded to colour tiles * 64)
    float *fs, *dfs, *c3;               // fp32 rows: aggregated feature [256] and its gradient, last colour post-activation [128]
    uint4 *xck, *c1k, *c2k;             // k-major [samples / 8][288 | 128 | 128] inputs of the three colour layers ([f | view encoding | 0], c1, c2), one plane
    uint4 *dc1k, *dc2k, *dc3k;          // k-major [samples / 8][128] their output gradients (one plane, scaled)
    unsigned *cmask;                    // [colour tiles][2 layers c1, c2][256]: LeakyReLU sign bits in the accumulator layout
    // two-plane weight-gradient mode only (pnerf_set_wgrad_planes(2); null otherwise): the RESIDUAL plane of every array above that the
    // weight-gradient GEMMs stream (value = plane + residual to 22 bits), same layouts; x0k then always holds all 288 columns
    uint4 *x0m, *h1m, *h2m, *h3m, *dy1m, *dy2m, *dy3m, *dy4m;
    uint4 *xcm, *c1m, *c2m, *dc1m, *dc2m, *dc3m;
    int wg2;                            // 1 in that mode
    // sample classes (aggregate.hip: pn_classify): the valid samples re-listed class by class, and where each class lives
    int *cls_list;                      // [samples] sample ids, class 0 first
    int *cls_info;                      // PN_CI_* words
    int *cls_tmp;                       // scratch of the partition: flags [samples] + positions [samples] + scan scratch
    long long rows, samples;
};
// cls_info words: per class c (< PN_NCLS): number of samples, first position in cls_list, first tile; then totals
enum : int { PN_NCLS = 3, PN_CI_COUNT = 0, PN_CI_VBASE = 4, PN_CI_TBASE = 8, PN_CI_TILES = 12, PN_CI_CTILES = 13 /* colour tiles of the step */,
              PN_CI_CLAIM = 16 /* the forward's tile claim counters, one per class */, PN_CI_WORDS = 20 };
// ---- dynamic tile claim of the two tile kernels.  A launch keeps its grid of resident workgroups and its tile index space; a workgroup's first
// PN_CLAIM_STATIC_* tiles are blockIdx.x + j * gridDim.x (as many as its loop looks ahead: it starts without waiting for anything), every later
// one comes from a returning atomicAdd on the launch's counter, issued by one lane a tile ahead of its use and handed to the other waves through
// one LDS word behind barriers the loop has anyway.  Claims ascend, so the chip still works on one moving window of the saved area; a claim at or
// beyond the tile count ends the workgroup.  Counters are zero at launch: the forward's (cls_info) by the classification's memset, the backward's
// (gscale words PN_GS_CLAIM ..) by the memset of its launcher.  With one tile per claim every tile iteration claims once: a launch leaves
// its counter at the number of tiles it ran, the same number every time (the saved area stays bit-reproducible).
// (k_agg_backward with xyz_grad and f16 cross terms or two planes keeps the static dealing: backward.hip.)
#ifndef PN_CLAIM_TILES
#define PN_CLAIM_TILES 1                       // consecutive tiles per claim.  Only 1 is shipped and tested; 2 and 4 were built for one A/B (no better: profiles/dynamic_tiles.json)
#endif
enum : int { PN_CLAIM_STATIC_FWD = 4, PN_CLAIM_STATIC_BWD = 2, PN_GS_CLAIM = 4, PN_GS_WORDS = 8 };
// tile index of claim sequence number m (0, 1, ...) of a workgroup whose latest claimed value is v
__device__ __forceinline__ int pn_claim_tile(int nstatic, int grid, int v, int m) { return nstatic * grid + v * PN_CLAIM_TILES + m % PN_CLAIM_TILES; }
// the grid of the tile and colour kernels: `dflt` resident workgroups (a multiple of the CU count), or pnerf_debug_set_tile_grid's cap
int pn_tile_grid(long long tiles, long long dflt);
int pn_class_slots(int K, int kc[3]);
int pn_classify(const PnSaved &sv, const int32_t *d_valid_list, const int32_t *d_counters, const int32_t *d_pidx, int K, long long n_valid, bool train, bool save_x0, hipStream_t s);
// the layout of the saved area (aggregate.hip): one walk serves the byte count (null base) and the pointers; s.rows / s.samples are set either way
size_t pn_saved_walk(void *base, long long n_valid, int K, PnSaved &s);
void pn_cls_walk(PnCarver &cv, PnSaved &s);
size_t pn_saved_bytes(long long n_valid, int K);
PnSaved pn_saved_carve(void *base, long long n_valid, int K);
// the launchers behind the four render entry points (render.hip validates, then calls): the aggregator + colour MLP forward (aggregate.hip)
// and their backward with the weight-gradient GEMMs (backward.hip; d_partials holds pn_wgrad_partials_bytes())
int pn_agg_forward_launch(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step &st, float *d_decoded, float *d_weight,
                          const PnSaved &sv, bool train, bool save_x0, hipStream_t s);
int pn_agg_backward_launch(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step &st, const float *d_decoded, const float *d_weight,
                           const float *d_grad_decoded, const PnSaved &sv, float *d_grad_params, const pnerf_point_grads *pg,
                           float *d_partials, bool x0_saved, hipStream_t s);
size_t pn_wgrad_partials_bytes();
// the process-wide arithmetic settings (aggregate.hip; include/pnerf.h: pnerf_set_* / pnerf_get_arithmetic).  A launcher takes ONE copy.
struct PnArith {
    int products;                       // 3 (default) or 2: MFMA products per multiply-add of the inference forward
    int wgrad_planes;                   // 1 (default: one f16 plane per weight-gradient operand) or 2 (both operands as two planes, three products)
    int cross_terms;                    // 8 (default: mixq.h, e4m3 cross terms in the aggregator's tile GEMMs) or 16 (f16x3.h's three f16 products)
    int mix_where;                      // as stored: bit 0 / 1 / 2 = inference forward / training forward / backward
    int mix_mask() const { return cross_terms == 8 ? mix_where : 0; }       // which tile kernels run the mixed format now
};
PnArith pn_arith();

__host__ __device__ inline int pn_tile_samples(int K) { return PN_TILE / K; }
// row / K for a tile row (row < 64, K <= 64) without an integer division (a runtime division is ~35 instructions, and the tile kernels
// did one per row they touch): kinv = ceil(2^16 / K), row / K = (row * kinv) >> 16 exactly for row * K < 2^16
__device__ __forceinline__ unsigned pn_kinv(int K) { return (65536u + (unsigned)K - 1u) / (unsigned)K; }
__device__ __forceinline__ int pn_row_div(int row, unsigned kinv) { return (int)(((unsigned)row * kinv) >> 16); }


// ---- dev-only phase timeline (build with EXTRA_DEFS=-DPN_PHASE_TRACE into tools/_build; tools/gpu_phase_trace.py reads it) ----------
// thread 0 of the first PN_TR_WGS workgroups stamps s_memrealtime (100 MHz) at the phase boundaries of PN_TR_ITERS tile iterations
#ifdef PN_PHASE_TRACE
#define PN_TR_WGS   512
#define PN_TR_IT0   20
#define PN_TR_ITERS 6
#define PN_TR_SLOTS 24
#define PN_TR_DECL(name) __device__ unsigned long long name[PN_TR_WGS * PN_TR_ITERS * PN_TR_SLOTS]
#define PN_TR(buf, ph)                                                                                              \
    do {                                                                                                            \
        if (tid == 0 && blockIdx.x < PN_TR_WGS && titer >= PN_TR_IT0 && titer < PN_TR_IT0 + PN_TR_ITERS)           \
            buf[((size_t)blockIdx.x * PN_TR_ITERS + (titer - PN_TR_IT0)) * PN_TR_SLOTS + (ph)] = wall_clock64();    \
    } while (0)
#define PN_TR_HWID(buf)                                                                                             \
    do {                                                                                                            \
        if (tid == 0 && blockIdx.x < PN_TR_WGS && titer >= PN_TR_IT0 && titer < PN_TR_IT0 + PN_TR_ITERS)           \
            buf[((size_t)blockIdx.x * PN_TR_ITERS + (titer - PN_TR_IT0)) * PN_TR_SLOTS + PN_TR_SLOTS - 1] =         \
                (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |                                    \
                ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);                             \
    } while (0)
#define PN_TR_ITER_DECL int titer = -1
#define PN_TR_ITER_NEXT ++titer
// the life of a workgroup in the launch of the K-rows class (tools/gpu_finish_trace.py): [0] top of its first tile, [1] end of its last
// tile (every tile overwrites it), [2] tiles it ran
#define PN_TR_SPAN_DECL(name) __device__ unsigned long long name[PN_TR_WGS * 4]
#define PN_TR_SPAN(buf, cls, end)                                                                                   \
    do {                                                                                                            \
        if (tid == 0 && (cls) == 0 && blockIdx.x < PN_TR_WGS && ((end) || titer == 0)) {                            \
            buf[(size_t)blockIdx.x * 4 + (end)] = wall_clock64();                                                   \
            if (end) buf[(size_t)blockIdx.x * 4 + 2] = (unsigned long long)(titer + 1);                             \
        }                                                                                                           \
    } while (0)
#else
#define PN_TR(buf, ph)
#define PN_TR_HWID(buf)
#define PN_TR_ITER_DECL
#define PN_TR_ITER_NEXT
#define PN_TR_SPAN(buf, cls, end)
#endif
