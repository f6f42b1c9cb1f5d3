// aggregate.hip -- per-sample feature aggregator (forward): gather + feature build + MFMA MLP chain +
// K-weighted reduction, then the colour MLP, for the lego-script architecture.
//
// Replaces NeuralPoints.forward's index_select gathers (models/neural_points/neural_points.py:706-717),
// PointAggregator.forward / viewmlp (models/aggregators/point_aggregators.py:727-814, 488-644) and
// positional_encoding (models/helpers/networks.py:175-190).  The reference runs this as ~60 ATen kernels
// that move every [Nv,256] activation through HBM between layers and compact/scatter rows by boolean
// masks; here a workgroup keeps a 64-row tile (TS samples x K neighbor slots) in LDS across the whole chain:
//   gather (embedding 128 B + xyz/dir/colour/conf) -> X0[64x288] in LDS (sin/cos PE computed in place)
//   -> 284->256->256 -> (+7) ->256->256 on the f16 matrix pipe with two-plane operands (f16x3.h: fp32-accurate, 5.3x the
//   fp32 MFMA rate), weights streamed from an L2-resident fragment-ordered image -> alpha head + K-weighted sums
//   (sigma, f[256]) -> f to HBM -> colour kernel: 64 samples per tile, 280->128->128->128->3 on the same two-plane GEMMs.
// Two workgroups (4 waves each) share a CU: the second one hides the first one's latencies (its VALU / LDS work does not run under
// the first one's MFMAs: tools/gemm_probe.hip).  In training mode the operands of the weight-gradient GEMMs are written once, already
// split into their f16 planes and transposed to the k-major order that kernel streams.
#include "mixq.h"
#include <stdlib.h>

// ------------------------------------------------------------------------------ layout / packing
extern "C" int pnerf_mlp_layout(int feat_dim, int64_t *offsets) {
    if (feat_dim != PN_F || !offsets) return PNERF_E_UNSUP;
    const int64_t o[PNERF_MLP_NTENSORS + 1] = {PO_W1, PO_B1, PO_W2, PO_B2, PO_W3, PO_B3, PO_W4, PO_B4, PO_W5, PO_B5,
                                               PO_WC1, PO_BC1, PO_WC2, PO_BC2, PO_WC3, PO_BC3, PO_WC4, PO_BC4, PO_TOTAL};
    for (int i = 0; i <= PNERF_MLP_NTENSORS; ++i) offsets[i] = o[i];
    return 0;
}
extern "C" size_t pnerf_mlp_packed_bytes(void) { return (size_t)PKC_END; }

namespace {
// two-plane f16 images of the aggregator and colour layers (f16x3.h): forward W[m][k] (trans = 0: m = output unit, k = input column)
// and dgrad W^T[m][k] (trans = 1: m = input column, k = output unit)
// cm1 / ck1 (dgrad images only; 0 = none): first unit + 1 of the column scales (mixq.h: PN_CS_*) of the image's m / k index -- the image then holds
// W^T[m][k] c[m] / c[k]; m beyond the layer's units (the extras of layer 3) has no scale
struct PackHDesc { int src, ld, trans, Mreal, Kreal, NCH, MB, dst, cm1, ck1; };
__device__ __forceinline__ float pn_pack_scale(const char *packed, int cm1, int ck1, int m, int k) {
    float f = 1.f;
    if (cm1 && m < (cm1 - 1 < PN_CS_C1 ? PN_H : PN_HC)) f = pn_col_scale(packed, cm1 - 1)[m];
    if (ck1) f *= pn_col_scale_inv(packed, ck1 - 1)[k];
    return f;
}
// the column scales of the seven hidden layers (mixq.h): one workgroup per layer, a thread per unit
struct ColScaleDesc { int first, units, n_cons; struct { int src, ld, rows; } cons[2]; };
struct ColScaleTable { ColScaleDesc d[7]; };
__global__ __launch_bounds__(256) void k_pack_colscale(ColScaleTable t, const float *__restrict__ params, char *__restrict__ packed) {
    __shared__ unsigned red[256];
    const ColScaleDesc d = t.d[blockIdx.x];
    const int j = threadIdx.x;
    float mx = 0.f;
    if (j < d.units)
        for (int c = 0; c < d.n_cons; ++c)
            for (int r = 0; r < d.cons[c].rows; ++r) mx = fmaxf(mx, fabsf(params[d.cons[c].src + r * d.cons[c].ld + j]));
    const unsigned mb = __float_as_uint(mx);
    const bool ok = mb >= 0x00800000u && mb < 0x7f800000u;          // (a zero / subnormal / non-finite column takes no scale and sets no reference)
    red[j] = ok ? mb : 0u;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (j < off) red[j] = red[j] > red[j + off] ? red[j] : red[j + off];
        __syncthreads();
    }
    if (j >= d.units) return;
    int e = ok ? (int)(red[0] >> 23) - (int)(mb >> 23) : 0;           // binades below the layer's largest column
    e = e > PN_CS_MAXE ? PN_CS_MAXE : e;
    float *cs = reinterpret_cast<float *>(packed + PKC_SCALE);
    cs[d.first + j] = __uint_as_float((unsigned)(127 + e) << 23);
    cs[PN_CS_UNITS + d.first + j] = __uint_as_float((unsigned)(127 - e) << 23);
}
struct PackHTable { PackHDesc d[15]; };
__global__ __launch_bounds__(256) void k_pack_h(PackHTable t, const float *__restrict__ params, char *__restrict__ packed) {
    const PackHDesc d = t.d[blockIdx.y];
    const int total = d.NCH * d.MB * 64;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int lane = e & 63, mb = (e >> 6) % d.MB, c = (e >> 6) / d.MB;
        const int m = 32 * mb + (lane & 31), k0 = 16 * c + 8 * (lane >> 5);
        unsigned h[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int k = k0 + 2 * j + i;
                v[i] = 0.f;
                if (m < d.Mreal && k < d.Kreal) v[i] = d.trans ? params[d.src + k * d.ld + m] * pn_pack_scale(packed, d.cm1, d.ck1, m, k) : params[d.src + m * d.ld + k];
            }
            // weights: high plane rounded to NEAREST (v_cvt_pk_f16_f32), residual as always -- h + m is the same 22-bit number for the
            // three-product GEMMs, and h alone is the unbiased best single f16 of the weight, which is what the two-product inference
            // option multiplies with (a round-toward-zero plane shrinks every weight by 2^-12 on average: measured 7e-4 on RGB after
            // seven layers); |w| <= 65504 is checked on the host (PointAggregator.check_range), the clamp here is that bound
            pn_split2_sat(v[0], v[1], h[j], lo[j]);
        }
        uint4 *o = reinterpret_cast<uint4 *>(packed + d.dst) + ((size_t)(c * d.MB + mb) * 2) * 64 + lane;
        o[0] = make_uint4(h[0], h[1], h[2], h[3]);
        o[64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }
}

// mixed-format images of the eight aggregator GEMMs (mixq.h): per (superchunk, feature block, lane) four f16 h fragments, two e4m3 fragments
// [q8(wm 2^11 / 2^e) x 8 | q8(wh / 2^e) x 8] per 8-column group with the lane's block scale e, then the classic two-plane tail chunks
struct PackMDesc { int src, ld, trans, Mreal, Kreal, NT, MB, dst, cm1, ck1; };
struct PackMTable { PackMDesc d[9]; };
__global__ __launch_bounds__(256) void k_pack_mix(PackMTable t, const float *__restrict__ params, char *__restrict__ packed) {
    pn_mode_saturate();
    const PackMDesc d = t.d[blockIdx.y];
    auto W = [&](int m, int k) -> float {
        return (m < d.Mreal && k < d.Kreal) ? (d.trans ? params[d.src + k * d.ld + m] * pn_pack_scale(packed, d.cm1, d.ck1, m, k) : params[d.src + m * d.ld + k]) : 0.f;
    };
    uint4 *img = reinterpret_cast<uint4 *>(packed + d.dst);
    unsigned *sc = reinterpret_cast<unsigned *>(img + PN_MIMG_U4(d.NT, d.MB));
    const int nsup = PN_MIX_NS * d.MB * 64, ntail = d.NT * d.MB * 64;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < nsup + ntail; e += gridDim.x * 256) {
        if (e < nsup) {
            const int lane = e & 63, mb = (e >> 6) % d.MB, s = (e >> 6) / d.MB, m = 32 * mb + (lane & 31), hf = lane >> 5;
            uint4 *o = img + ((size_t)(s * d.MB + mb) * 8) * 64 + lane;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k0 = 64 * s + 16 * r + 8 * hf;
                unsigned h[4], lo[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) pn_split2_rne(W(m, k0 + 2 * j), W(m, k0 + 2 * j + 1), h[j], lo[j]);
                o[r * 64] = make_uint4(h[0], h[1], h[2], h[3]);
            }
            unsigned scw = 0u;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // the lane's 16 columns (two 8-column groups), and the largest slot over ALL 32 columns of the fragment (both lane halves): the
                // instruction's scale blocks are registers 0..3 of BOTH halves (scaled by lanes 0..31's byte) and registers 4..7 of both (lanes 32..63's),
                // not "a lane's 32 slots" -- measured, tools/gpu_mix_diag.py; one exponent per (row, fragment) is right under either reading
                float wh[16], wm[16], mx = 0.f;
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const float w = W(m, 64 * s + 32 * j + i);
#ifdef PN_EMU
                    const float wc = fmaxf(fminf(w, 65504.f), -65504.f);
#else
                    const float wc = w;
#endif
                    const float h = (float)(_Float16)wc;
                    mx = fmaxf(mx, fmaxf(fabsf(h), fabsf(w - h) * 2048.f));
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float w = W(m, 8 * (8 * s + 4 * j + 2 * hf + (i >> 3)) + (i & 7));
#ifdef PN_EMU
                    const float wc = fmaxf(fminf(w, 65504.f), -65504.f);
#else
                    const float wc = w;
#endif
                    wh[i] = (float)(_Float16)wc; wm[i] = w - wh[i];
                }
                int ex = 0;
                const float fr = frexpf(mx, &ex);
                int be = mx > 0.f ? (fr > 0.875f ? ex - 8 : ex - 9) : 0;            // the largest slot / 2^be lies in (224, 448]
                be = be < -100 ? -100 : (be > 100 ? 100 : be);
                const float sh = __uint_as_float((unsigned)(be + 127) << 23), sm = __uint_as_float((unsigned)(be + 127 - 11) << 23);
                scw |= (unsigned)(be + 127) << (8 * j);
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    unsigned q[4];
#pragma unroll
                    for (int w4 = 0; w4 < 4; ++w4) {
                        const float *src = (w4 < 2 ? wm : wh) + 8 * tt + 4 * (w4 & 1);
                        const float scl = w4 < 2 ? sm : sh;
                        pn_s2 r = {0, 0};
                        r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, src[0], src[1], scl, false);
                        r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, src[2], src[3], scl, true);
                        q[w4] = __builtin_bit_cast(unsigned, r);
                    }
                    o[(4 + 2 * j + tt) * 64] = make_uint4(q[0], q[1], q[2], q[3]);
                }
            }
            sc[(size_t)(s * d.MB + mb) * 64 + lane] = scw;
        } else {
            const int e2 = e - nsup, lane = e2 & 63, mb = (e2 >> 6) % d.MB, tc = (e2 >> 6) / d.MB, m = 32 * mb + (lane & 31);
            const int k0 = 256 + 16 * tc + 8 * (lane >> 5);
            unsigned h[4], lo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) pn_split2_sat(W(m, k0 + 2 * j), W(m, k0 + 2 * j + 1), h[j], lo[j]);
            uint4 *o = img + (size_t)PN_MIX_NS * d.MB * 8 * 64 + ((size_t)(tc * d.MB + mb) * 2) * 64 + lane;
            o[0] = make_uint4(h[0], h[1], h[2], h[3]);
            o[64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        }
    }
}
}  // namespace

extern "C" int pnerf_mlp_pack(const float *d_params, void *d_packed, void *stream) {
    if (!d_params || !d_packed) return PNERF_E_INVAL;
    PackHTable th = {{
        {PO_W1, PN_IN1, 0, PN_H, PN_IN1, 18, 8, PKH_F1},
        {PO_W2, PN_H, 0, PN_H, PN_H, 16, 8, PKH_F2},
        {PO_W3, PN_IN3, 0, PN_H, PN_IN3, 17, 8, PKH_F3},
        {PO_W4, PN_H, 0, PN_H, PN_H, 16, 8, PKH_F4},
        {PO_W4, PN_H, 1, PN_H, PN_H, 16, 8, PKH_D4, PN_CS_L3 + 1, PN_CS_L4 + 1},
        {PO_W3, PN_IN3, 1, PN_IN3, PN_H, 16, 9, PKH_D3, PN_CS_L2 + 1, PN_CS_L3 + 1},
        {PO_W2, PN_H, 1, PN_H, PN_H, 16, 8, PKH_D2, PN_CS_L1 + 1, PN_CS_L2 + 1},
        {PO_W1, PN_IN1, 1, 32 * PN_MB_D1, PN_H, 16, PN_MB_D1, PKH_D1, 0, PN_CS_L1 + 1},
        // colour MLP: forward W[m][k], dgrad W^T[m][k] (first 256 input columns of layer 1: the view encoding has no gradient)
        {PO_WC1, PN_INC, 0, PN_HC, PN_INC, 18, 4, PKH_FC1},
        {PO_WC2, PN_HC, 0, PN_HC, PN_HC, 8, 4, PKH_FC2},
        {PO_WC3, PN_HC, 0, PN_HC, PN_HC, 8, 4, PKH_FC3},
        {PO_WC3, PN_HC, 1, PN_HC, PN_HC, 8, 4, PKH_DC3, PN_CS_C2 + 1, PN_CS_C3 + 1},
        {PO_WC2, PN_HC, 1, PN_HC, PN_HC, 8, 4, PKH_DC2, PN_CS_C1 + 1, PN_CS_C2 + 1},
        {PO_WC1, PN_INC, 1, PN_H, PN_HC, 8, 8, PKH_DC1, PN_CS_L4 + 1, PN_CS_C1 + 1},          // (d f leaves x the h4 units' scales: b_front)
        // xyz_grad: d X0 columns 224 .. 287 (W1^T rows 224 .. 283, the distance encoding; rows 284 .. 287 zero)
        {PO_W1 + 32 * PN_MB_D1, PN_IN1, 1, PN_IN1 - 32 * PN_MB_D1, PN_H, 16, 2, PKH_D1T, 0, PN_CS_L1 + 1},
    }};
    // the hidden units' column scales first (mixq.h): from the columns of every consumer's weight; the dgrad images below are built with them
    const ColScaleTable tc = {{
        {PN_CS_L1, PN_H, 1, {{PO_W2, PN_H, PN_H}}},
        {PN_CS_L2, PN_H, 1, {{PO_W3, PN_IN3, PN_H}}},
        {PN_CS_L3, PN_H, 1, {{PO_W4, PN_H, PN_H}}},
        {PN_CS_L4, PN_H, 2, {{PO_W5, PN_H, 1}, {PO_WC1, PN_INC, PN_HC}}},
        {PN_CS_C1, PN_HC, 1, {{PO_WC2, PN_HC, PN_HC}}},
        {PN_CS_C2, PN_HC, 1, {{PO_WC3, PN_HC, PN_HC}}},
        {PN_CS_C3, PN_HC, 1, {{PO_WC4, PN_HC, 3}}},
    }};
    PnProfScope prof(PNK_PACK, (hipStream_t)stream);
    hipLaunchKernelGGL(k_pack_colscale, dim3(7), dim3(256), 0, (hipStream_t)stream, tc, d_params, (char *)d_packed);
    hipLaunchKernelGGL(k_pack_h, dim3(40, 15), dim3(256), 0, (hipStream_t)stream, th, d_params, (char *)d_packed);
    PackMTable tm = {{
        {PO_W1, PN_IN1, 0, PN_H, PN_IN1, 2, 8, PKM_F1},
        {PO_W2, PN_H, 0, PN_H, PN_H, 0, 8, PKM_F2},
        {PO_W3, PN_IN3, 0, PN_H, PN_IN3, 1, 8, PKM_F3},
        {PO_W4, PN_H, 0, PN_H, PN_H, 0, 8, PKM_F4},
        {PO_W4, PN_H, 1, PN_H, PN_H, 0, 8, PKM_D4, PN_CS_L3 + 1, PN_CS_L4 + 1},
        {PO_W3, PN_IN3, 1, PN_IN3, PN_H, 0, 9, PKM_D3, PN_CS_L2 + 1, PN_CS_L3 + 1},
        {PO_W2, PN_H, 1, PN_H, PN_H, 0, 8, PKM_D2, PN_CS_L1 + 1, PN_CS_L2 + 1},
        {PO_W1, PN_IN1, 1, 32 * PN_MB_D1, PN_H, 0, PN_MB_D1, PKM_D1, 0, PN_CS_L1 + 1},
        {PO_W1 + 32 * PN_MB_D1, PN_IN1, 1, PN_IN1 - 32 * PN_MB_D1, PN_H, 0, 2, PKM_D1T, 0, PN_CS_L1 + 1},
    }};
    hipLaunchKernelGGL(k_pack_mix, dim3(12, 9), dim3(256), 0, (hipStream_t)stream, tm, d_params, (char *)d_packed);
    PN_CHECK_LAUNCH();
    return 0;
}

namespace {
// ---- debug: one mixed tile GEMM D[64][256] = X[64][K] W[256][K]^T through the tile's LDS format and a packed image (tests: against float64 on the
// device, against the numpy restatement of the format on the host emulator)
template <int NT>
__global__ __launch_bounds__(256) void k_debug_mix_gemm(const float *__restrict__ x, const char *__restrict__ img, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_d[];
    pn_mode_saturate();
    constexpr int K = 256 + 16 * NT;
    char *X = smem_d;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int e = tid; e < PN_TILE * (K / 4); e += 256) {
        const int row = e / (K / 4), col = 4 * (e % (K / 4));
        const float4 v = *reinterpret_cast<const float4 *>(x + row * K + col);
        if (col < 256) pn_xq_store4(X, row, col, v.x, v.y, v.z, v.w);
        else pn_xt_store4(X, row, col, v.x, v.y, v.z, v.w);
    }
    __syncthreads();
    f32x16 acc[2][2];
    pn_acc_zero(acc);
    pn_gemm_mix<PN_MIX_NS, NT, 8, 2>(X, img, 2 * wave, lane, acc);
#pragma unroll
    for (int fb = 0; fb < 2; ++fb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) out[(32 * rb + (lane & 31)) * PN_H + pn_d_feat(2 * wave + fb, g, lane) + i] = acc[fb][rb][4 * g + i];
}
}  // namespace

extern "C" int pnerf_debug_mix_gemm(const float *d_w, int K, const float *d_x, void *d_img, float *d_out, void *stream) {
    if (!d_w || !d_x || !d_img || !d_out || (K != 256 && K != 272 && K != 288)) return PNERF_E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    const int NT = (K - 256) / 16;
    PackMTable tm = {{{0, K, 0, PN_H, K, NT, 8, 0}}};
    hipLaunchKernelGGL(k_pack_mix, dim3(12, 1), dim3(256), 0, s, tm, d_w, (char *)d_img);
    const void *fn = NT == 0 ? (const void *)k_debug_mix_gemm<0> : NT == 1 ? (const void *)k_debug_mix_gemm<1> : (const void *)k_debug_mix_gemm<2>;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, PN_XBYTES) != hipSuccess) return PNERF_E_LAUNCH;
    if (NT == 0) hipLaunchKernelGGL(k_debug_mix_gemm<0>, dim3(1), dim3(256), PN_XBYTES, s, d_x, (const char *)d_img, d_out);
    else if (NT == 1) hipLaunchKernelGGL(k_debug_mix_gemm<1>, dim3(1), dim3(256), PN_XBYTES, s, d_x, (const char *)d_img, d_out);
    else hipLaunchKernelGGL(k_debug_mix_gemm<2>, dim3(1), dim3(256), PN_XBYTES, s, d_x, (const char *)d_img, d_out);
    PN_CHECK_LAUNCH();
    return 0;
}

namespace {
__global__ __launch_bounds__(64) void k_debug_mfma_f16(const uint4 *__restrict__ a, const uint4 *__restrict__ b, float *__restrict__ d) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(pn_h8, a[threadIdx.x]), __builtin_bit_cast(pn_h8, b[threadIdx.x]), acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) d[threadIdx.x * 16 + r] = acc[r];
}
}  // namespace
namespace {
__global__ __launch_bounds__(256) void k_debug_split(const float *__restrict__ x, long long n, unsigned *__restrict__ h, unsigned *__restrict__ m, int sat) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; 2 * i < n; i += (long long)gridDim.x * 256) {
        unsigned hh, mm;
        if (sat) pn_split2_sat(x[2 * i], x[2 * i + 1], hh, mm);
        else pn_split2(x[2 * i], x[2 * i + 1], hh, mm);
        h[i] = hh; m[i] = mm;
    }
}
}  // namespace
extern "C" int pnerf_debug_split(const float *d_x, int64_t n, void *d_h, void *d_m, int sat, void *stream) {
    if (!d_x || !d_h || !d_m || n < 0 || (n & 1)) return PNERF_E_INVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_debug_split, dim3(64), dim3(256), 0, (hipStream_t)stream, d_x, (long long)n, (unsigned *)d_h, (unsigned *)d_m, sat);
    PN_CHECK_LAUNCH();
    return 0;
}

namespace {
template <int NF> __global__ __launch_bounds__(256) void k_debug_pe(const float *__restrict__ x, long long n, float *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float s[NF], c[NF];
        pn_pe_octaves<NF>(x[i], s, c);
#pragma unroll
        for (int f = 0; f < NF; ++f) { out[(i * NF + f) * 2] = s[f]; out[(i * NF + f) * 2 + 1] = c[f]; }
    }
}
}  // namespace
extern "C" int pnerf_debug_pe(const float *d_x, int64_t n, int nfreq, float *d_out, void *stream) {
    if (!d_x || !d_out || n < 0 || nfreq < 1 || nfreq > 5) return PNERF_E_INVAL;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    switch (nfreq) {
        case 1: hipLaunchKernelGGL(k_debug_pe<1>, dim3(64), dim3(256), 0, s, d_x, (long long)n, d_out); break;
        case 2: hipLaunchKernelGGL(k_debug_pe<2>, dim3(64), dim3(256), 0, s, d_x, (long long)n, d_out); break;
        case 3: hipLaunchKernelGGL(k_debug_pe<3>, dim3(64), dim3(256), 0, s, d_x, (long long)n, d_out); break;
        case 4: hipLaunchKernelGGL(k_debug_pe<4>, dim3(64), dim3(256), 0, s, d_x, (long long)n, d_out); break;
        default: hipLaunchKernelGGL(k_debug_pe<5>, dim3(64), dim3(256), 0, s, d_x, (long long)n, d_out); break;
    }
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_debug_mfma_f16(const void *d_a, const void *d_b, float *d_out, void *stream) {
    if (!d_a || !d_b || !d_out) return PNERF_E_INVAL;
    hipLaunchKernelGGL(k_debug_mfma_f16, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint4 *)d_a, (const uint4 *)d_b, d_out);
    PN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------ saved activations
// THE layout of the saved area: which arrays, in which order, how many elements each.  A carver without a base only counts (pn_saved_bytes), one
// with a base hands out the pointers (pn_saved_carve): the two cannot disagree.  Returns the bytes.
size_t pn_saved_walk(void *base, long long n_valid, int K, PnSaved &s) {
    const int TS = pn_tile_samples(K);
    // + PN_NCLS tiles of rounding (each class ends in a partial tile) + PN_NCLS gap tiles (every class owns a padding tile) + 1
    const long long tiles = (n_valid + TS - 1) / TS + 2 * PN_NCLS + 1;
    s.rows = tiles * PN_TILE;
    s.samples = ((tiles * TS + PN_CTILE - 1) / PN_CTILE + 1) * PN_CTILE;
    PnCarver cv(base);
    const size_t rg = (size_t)s.rows / 8, rgc = (size_t)s.samples / 8;
    // the k-major planes the weight-gradient GEMMs stream: the residual planes (two-plane mode only) repeat the layout of the first ones
    auto planes = [&](uint4 *&x0, uint4 *&h2, uint4 *&h1, uint4 *&h3, uint4 *&dy1, uint4 *&dy2, uint4 *&dy3, uint4 *&dy4) {
        x0 = cv.take<uint4>(rg * PN_NF1); h2 = cv.take<uint4>(rg * PN_NF1);
        h1 = cv.take<uint4>(rg * PN_H); h3 = cv.take<uint4>(rg * PN_H);
        dy1 = cv.take<uint4>(rg * PN_H); dy2 = cv.take<uint4>(rg * PN_H);
        dy3 = cv.take<uint4>(rg * PN_H); dy4 = cv.take<uint4>(rg * PN_H);
    };
    auto cplanes = [&](uint4 *&xc, uint4 *&c1, uint4 *&c2, uint4 *&dc1, uint4 *&dc2, uint4 *&dc3) {
        xc = cv.take<uint4>(rgc * PN_NF1); c1 = cv.take<uint4>(rgc * PN_HC); c2 = cv.take<uint4>(rgc * PN_HC);
        dc1 = cv.take<uint4>(rgc * PN_HC); dc2 = cv.take<uint4>(rgc * PN_HC); dc3 = cv.take<uint4>(rgc * PN_HC);
    };
    planes(s.x0k, s.h2k, s.h1k, s.h3k, s.dy1k, s.dy2k, s.dy3k, s.dy4k);
    s.h4r = cv.take<uint4>((size_t)s.rows * 32 * 2);
    s.arow = cv.take<float>((size_t)s.rows); s.rmeta = cv.take<int4>((size_t)s.rows);
    s.lmask = cv.take<unsigned>((size_t)tiles * 3 * 512);
    s.gscale = cv.take<unsigned>(PN_GS_WORDS);
    s.fs = cv.take<float>((size_t)s.samples * PN_H); s.dfs = cv.take<float>((size_t)s.samples * PN_H);
    s.c3 = cv.take<float>((size_t)s.samples * PN_HC);
    cplanes(s.xck, s.c1k, s.c2k, s.dc1k, s.dc2k, s.dc3k);
    s.cmask = cv.take<unsigned>((size_t)s.samples / PN_CTILE * 2 * 256);
    s.wg2 = pn_arith().wgrad_planes == 2 ? 1 : 0;
    s.x0m = s.h1m = s.h2m = s.h3m = s.dy1m = s.dy2m = s.dy3m = s.dy4m = nullptr;
    s.xcm = s.c1m = s.c2m = s.dc1m = s.dc2m = s.dc3m = nullptr;
    if (s.wg2) {
        planes(s.x0m, s.h2m, s.h1m, s.h3m, s.dy1m, s.dy2m, s.dy3m, s.dy4m);
        cplanes(s.xcm, s.c1m, s.c2m, s.dc1m, s.dc2m, s.dc3m);
    }
    pn_cls_walk(cv, s);
    return cv.off;
}
// the class partition's arrays for s.samples samples (the tail of the saved area, and of the inference workspace: render.hip)
void pn_cls_walk(PnCarver &cv, PnSaved &s) {
    s.cls_list = cv.take<int>((size_t)s.samples);
    s.cls_info = cv.take<int>(PN_CI_WORDS);
    s.cls_tmp = cv.take<int>((size_t)2 * s.samples + pn_scan_scratch_ints(s.samples) + 8);
}
size_t pn_saved_bytes(long long n_valid, int K) { PnSaved s; return pn_saved_walk(nullptr, n_valid, K, s); }
PnSaved pn_saved_carve(void *base, long long n_valid, int K) { PnSaved s; pn_saved_walk(base, n_valid, K, s); return s; }

extern "C" size_t pnerf_agg_saved_bytes(int64_t n_valid_samples, int K) {
    if (K <= 0 || K > PNERF_MAX_K || n_valid_samples < 0) return 0;
    return pn_saved_bytes(n_valid_samples, K);
}

// ------------------------------------------------------------------------------ forward kernels
namespace {
struct FwdArgs {
    pnerf_camera cam;
    const float *xyz, *emb, *conf, *dir, *color;
    const float *params;
    const float4 *packed;
    const float *raydir, *sample_loc;
    const float *xyz_pers, *loc_pers;   // optional: perspective coords supplied by the caller (stand-alone aggregator)
    const int *pidx, *valid_list, *counters;
    const int *cls_list, *cls_info;     // sample classes (pn_classify); cls = the class this launch processes
    int cls, Kstride;                   // K = neighbor slots PROCESSED per sample of this class, Kstride = slots per sample in pidx / weight
    int save_x0;                        // training: also save the X0 planes (only the stand-alone aggregator, whose perspective coordinates come
                                        // from the caller; the fused path's weight-gradient GEMM rebuilds X0 from the gather: k_wgrad_x0)
    int R, SR, K, TS;
    long long cap_samples;      // capacity (in valid samples) of fs / saved buffers
    float *decoded, *weight;
    PnSaved sv;                 // fs always valid; the rest only when TRAIN
};
// the argument of the FRAMES instances (per-point Rw2c frames, pnerf_points.frames [N,9]); every other instance keeps FwdArgs as it is
struct FwdArgsF : FwdArgs { const float *frames; };
template <bool FRAMES> struct FwdArgsOf { using type = FwdArgs; };
template <> struct FwdArgsOf<true> { using type = FwdArgsF; };

// ------------------------------------------------------------------------------ sample classes
// 6 % of the neighbor rows of valid samples are empty slots (a sample near the surface's edge has 1..K-1 neighbors); the
// reference drops them by boolean masking (point_aggregators.py:523-538).  Tiles need whole samples of equal row count, so the
// valid samples are partitioned by the position of their LAST occupied slot into up to three classes that are processed with
// K, K/2 and K/4 rows per sample (K % 4 == 0; the query fills slots front to back, and for a caller-supplied mask the last
// occupied slot is what counts).  The partition is stable (ascending sample id inside a class): results are identical to the
// one-class launch, rows processed drop from 7.49 M to 7.1 M at the bench configuration.  Every class owns a run of tiles
// followed by one padding tile (the partner slot of an odd tile count works on it).
namespace {
struct ClsArgs { const int *valid_list, *counters, *pidx; int K, n, ncls; int kc[PN_NCLS], ts[PN_NCLS]; };

__global__ void k_cls_flags(ClsArgs c, int which, int *__restrict__ flags) {
    const int vs = blockIdx.x * blockDim.x + threadIdx.x;
    if (vs >= c.n) return;
    const int Ns = c.counters[0] < c.n ? c.counters[0] : c.n;
    int f = 0;
    if (vs < Ns) {
        const long long si = c.valid_list[vs];
        int hv = 0;
        for (int k = 0; k < c.K; ++k)
            if (c.pidx[si * c.K + k] >= 0) hv = k + 1;
        int cl = 0;
        for (int j = 1; j < c.ncls; ++j)
            if (hv <= c.kc[j]) cl = j;
        f = cl == which;
    }
    flags[vs] = f;
}

__global__ void k_cls_gather(ClsArgs c, int which, const int *__restrict__ pos, const int *__restrict__ count, int *__restrict__ cls_list,
                             int *__restrict__ info) {
    const int n = *count, base = info[PN_CI_VBASE + which];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) cls_list[base + i] = c.valid_list[pos[i]];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int tiles = (n + c.ts[which] - 1) / c.ts[which], tb = info[PN_CI_TBASE + which];
        info[PN_CI_COUNT + which] = n;
        if (which + 1 < PN_NCLS) { info[PN_CI_VBASE + which + 1] = base + n; info[PN_CI_TBASE + which + 1] = tb + tiles + 1; }
        info[PN_CI_TILES] = tb + tiles + 1;
    }
}

// the padding tile of every class: zero rows in everything the weight-gradient GEMMs read
__global__ void k_cls_zero_gaps(PnSaved sv, int ncls, int save_x0) {
    const int c = blockIdx.y;
    if (c >= ncls) return;
    // x0k holds EITHER the whole X0 (288-column layout: the stand-alone aggregator) OR its last 64 columns (64-column layout: the fused
    // path) -- the two layouts overlap, only the one in use may be zeroed
    if ((blockIdx.x == 0 && !save_x0) || (blockIdx.x == 8 && save_x0)) return;
    const long long gap = (c + 1 < PN_NCLS ? sv.cls_info[PN_CI_TBASE + c + 1] : sv.cls_info[PN_CI_TILES]) - 1;
    uint4 *arrs[9] = {sv.x0k, sv.h2k, sv.h1k, sv.h3k, sv.dy1k, sv.dy2k, sv.dy3k, sv.dy4k, sv.x0k};
    uint4 *arrm[9] = {sv.x0m, sv.h2m, sv.h1m, sv.h3m, sv.dy1m, sv.dy2m, sv.dy3m, sv.dy4m, nullptr};
    const int which = blockIdx.x;                      // 8 arrays (one k-major plane each) + x0k in its 64-column layout (the fused path: k_wgrad_x0)
    const int nf = which == 8 ? 64 : which < 2 ? PN_NF1 : PN_H;
    uint4 *p = arrs[which] + gap * 8 * nf;
    for (int i = threadIdx.x; i < 8 * nf; i += blockDim.x) p[i] = make_uint4(0u, 0u, 0u, 0u);
    if (sv.wg2 && arrm[which]) {                       // two-plane weight-gradient mode: the residual planes too
        uint4 *pm = arrm[which] + gap * 8 * nf;
        for (int i = threadIdx.x; i < 8 * nf; i += blockDim.x) pm[i] = make_uint4(0u, 0u, 0u, 0u);
    }
}
}  // namespace

}  // namespace

// class c processes kc[c] slots per sample
int pn_class_slots(int K, int kc[PN_NCLS]) {
    if (K % 4 == 0) { kc[0] = K; kc[1] = K / 2; kc[2] = K / 4; return 3; }
    kc[0] = K; kc[1] = kc[2] = 0;
    return 1;
}

int pn_classify(const PnSaved &sv, const int32_t *d_valid_list, const int32_t *d_counters, const int32_t *d_pidx, int K, long long n_valid,
                bool train, bool save_x0, hipStream_t s) {
    ClsArgs c;
    c.valid_list = d_valid_list; c.counters = d_counters; c.pidx = d_pidx; c.K = K; c.n = (int)n_valid;
    c.ncls = pn_class_slots(K, c.kc);
    for (int j = 0; j < PN_NCLS; ++j) c.ts[j] = c.kc[j] > 0 ? pn_tile_samples(c.kc[j]) : 1;
    if (hipMemsetAsync(sv.cls_info, 0, PN_CI_WORDS * sizeof(int), s) != hipSuccess) return PNERF_E_LAUNCH;
    if (n_valid <= 0) return 0;
    int *flags = sv.cls_tmp, *pos = flags + n_valid, *cnt = pos + n_valid, *scratch = cnt + 8;
    PnProfScope prof(PNK_COMPACT, s);
    for (int j = 0; j < c.ncls; ++j) {
        hipLaunchKernelGGL(k_cls_flags, dim3(pn_cdiv(n_valid, 256)), dim3(256), 0, s, c, j, flags);
        int rc = pn_compact_gt0_i32(flags, n_valid, pos, cnt, scratch, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cls_gather, dim3(256), dim3(256), 0, s, c, j, pos, cnt, sv.cls_list, sv.cls_info);
    }
    if (train) hipLaunchKernelGGL(k_cls_zero_gaps, dim3(9, c.ncls), dim3(256), 0, s, sv, c.ncls, save_x0 ? 1 : 0);
    PN_CHECK_LAUNCH();
    return 0;
}


namespace {

// ------------------------------------------------------------------------------ aggregator forward
// LDS of a workgroup (80 896 bytes: two workgroups per CU):
//   X     [2][64][PN_XRS]   the activation tile, two f16 planes (f16x3.h): X0 -> h1 -> [h2 | extras] -> h3 -> h4
//   exb   [64][8] f32       layer-3 extras of the tile's rows until they move next to h2
//   w5s   [256] f32         alpha head weights
//   rowf  wraw, wrow, wnrm [64] f32, sidx [64] int
constexpr int FL_EX = PN_XBYTES, FL_W5 = FL_EX + PN_TILE * 8 * 4, FL_ROW = FL_W5 + PN_H * 4, FL_CLAIM = FL_ROW + 4 * PN_TILE * 4 /* the claimed tile: one word */, FL_BYTES = FL_CLAIM + 16;
static_assert(2 * FL_BYTES <= 160 * 1024, "two forward workgroups must fit the 160 KB LDS");

struct FGather {               // what a thread holds of one tile row (4 threads per row, q = thread in row)
    float4 e0, e1;             // its 8 embedding dims
    float px, py, pz, lx, ly, lz, cf;
    float ppx, ppy, ppz, lpx, lpy, lpz;   // optional caller-supplied perspective coordinates
    float dxv, dyv, dzv, cx, cy, cz, rx, ry, rz;   // q == 0 only (FRAMES: direction and ray of every thread of the row)
    float fx, fy, fz, gx, gy, gz;                  // FRAMES only: row min(q, 2) of the frame of the row's point / of the sample's slot-0 point
};

// sample id of row `row` of tile `tile` (or -1)
__device__ __forceinline__ int f_sample_of(const FwdArgs &a, long long tile, int row, int Ns, unsigned kinv) {
    const int ls = pn_row_div(row, kinv);
    const long long vs = tile * a.TS + ls;
    return (ls < a.TS && vs < Ns) ? a.valid_list[vs] : -1;
}

template <bool PERS, bool FRAMES = false>
__device__ __forceinline__ void f_gather(const FwdArgs &a, FGather &G, int si_, int p_, int q, const float *frames = nullptr) {
    const int p = p_ > 0 ? p_ : 0, si = si_ > 0 ? si_ : 0;     // empty slots / rows read point 0 / sample 0 like the reference (neural_points.py:709); their weight is 0
    const float *ep = a.emb + (long long)p * PN_F + PN_EPT * q;
    G.e0 = *reinterpret_cast<const float4 *>(ep); G.e1 = *reinterpret_cast<const float4 *>(ep + 4);
    G.px = a.xyz[3 * p]; G.py = a.xyz[3 * p + 1]; G.pz = a.xyz[3 * p + 2];
    G.lx = a.sample_loc[(long long)si * 3]; G.ly = a.sample_loc[(long long)si * 3 + 1]; G.lz = a.sample_loc[(long long)si * 3 + 2];
    if (PERS) {
        G.ppx = a.xyz_pers[3 * p]; G.ppy = a.xyz_pers[3 * p + 1]; G.ppz = a.xyz_pers[3 * p + 2];
        G.lpx = a.loc_pers[(long long)si * 3]; G.lpy = a.loc_pers[(long long)si * 3 + 1]; G.lpz = a.loc_pers[(long long)si * 3 + 2];
    }
    G.cf = a.conf[p];
    if (FRAMES) {
        // per-point frames: thread q of the row (q < 3) forms component q of F[p] (xyz - loc), of F[p] dir and of F[slot 0] raydir, so it holds
        // ROW q of the two frames (3 + 3 floats, not 9 + 9) and the row's direction and ray; thread 3 repeats row 2 (its results are not used).
        // The slot-0 point of the sample comes through the neighbor table itself: empty -> point 0, like every empty slot
        const int r = si / a.SR, fr = q < 3 ? q : 2;
        const int ps_ = a.pidx[(long long)si * a.Kstride], ps = ps_ > 0 ? ps_ : 0;
        const float *fp = frames + (long long)p * 9 + 3 * fr, *gp = frames + (long long)ps * 9 + 3 * fr;
        G.fx = fp[0]; G.fy = fp[1]; G.fz = fp[2];
        G.gx = gp[0]; G.gy = gp[1]; G.gz = gp[2];
        G.dxv = a.dir[3 * p]; G.dyv = a.dir[3 * p + 1]; G.dzv = a.dir[3 * p + 2];
        G.rx = a.raydir[3 * r]; G.ry = a.raydir[3 * r + 1]; G.rz = a.raydir[3 * r + 2];
        if (q == 0) { G.cx = a.color[3 * p]; G.cy = a.color[3 * p + 1]; G.cz = a.color[3 * p + 2]; }
    } else if (q == 0) {
        const int r = si / a.SR;
        G.dxv = a.dir[3 * p]; G.dyv = a.dir[3 * p + 1]; G.dzv = a.dir[3 * p + 2];
        G.cx = a.color[3 * p]; G.cy = a.color[3 * p + 1]; G.cz = a.color[3 * p + 2];
        G.rx = a.raydir[3 * r]; G.ry = a.raydir[3 * r + 1]; G.rz = a.raydir[3 * r + 2];
    }
}

// X0 row of the tile: [e(32) | PE3(e) (192) | PE5(dists) (60) | 1 | 0 0 0], the row's raw weight and layer-3 extras
// (point_aggregators.py:773-784, :425-428, :506, :566; networks.py:175-190)
// MIX: the tile in the mixed format of mixq.h (columns < 256: h plane + e4m3 units; from 256 on the two f16 planes, h to nearest); else
// f16x3.h's two planes with h rounded to NEAREST (inference and training alike; the training forward's k-major copy-outs then read the h plane only)
// FRAMES: per-point Rw2c (scene editing, point_aggregators.py:492-496,506,526,566): the first three distance components and the stored
// direction are rotated by the frame of the ROW's point, the view direction by the frame of the sample's SLOT-0 point -- also inside the
// extras (q - v, q.v) of every row of the sample, which so mix two frames exactly as the reference does
template <bool PERS, bool MIX = false, bool FRAMES = false>
__device__ __forceinline__ void f_build(const FwdArgs &a, const FGather &G, char *X, float *exb, float *wraw, int *sidx, int si, int p, int row, int q) {
    const float dwx = G.px - G.lx, dwy = G.py - G.ly, dwz = G.pz - G.lz;
    float ppx, ppy, pcz, spx, spy, scz;
    if (PERS) {
        ppx = G.ppx; ppy = G.ppy; pcz = G.ppz; spx = G.lpx; spy = G.lpy; scz = G.lpz;
    } else {
        float pcx, pcy, scx, scy;
        if (FRAMES) {
            // hipcc contracts a sum of three products into a multiply and two FMAs in an order that depends on the code around it (in the uniform
            // instance the first of the two rot3 below starts from the x product, the second from the y product), and each order rounds
            // differently.  The FRAMES instances spell out the order the uniform fused-path instance has -- here, at the row weight and at q.v
            // below -- so that identity frames reproduce the uniform render bit for bit (tests/test_gpu_editing.py)
            const float *M = a.cam.camrot;
            const float x = G.px - a.cam.campos[0], y = G.py - a.cam.campos[1], z = G.pz - a.cam.campos[2];
            const float u = G.lx - a.cam.campos[0], v = G.ly - a.cam.campos[1], w = G.lz - a.cam.campos[2];
            pcx = __builtin_fmaf(z, M[6], __builtin_fmaf(y, M[3], x * M[0]));
            pcy = __builtin_fmaf(z, M[7], __builtin_fmaf(y, M[4], x * M[1]));
            pcz = __builtin_fmaf(z, M[8], __builtin_fmaf(y, M[5], x * M[2]));
            scx = __builtin_fmaf(w, M[6], __builtin_fmaf(u, M[0], v * M[3]));
            scy = __builtin_fmaf(w, M[7], __builtin_fmaf(u, M[1], v * M[4]));
            scz = __builtin_fmaf(w, M[8], __builtin_fmaf(u, M[2], v * M[5]));
        } else {
        rot3(a.cam.camrot, G.px - a.cam.campos[0], G.py - a.cam.campos[1], G.pz - a.cam.campos[2], false, pcx, pcy, pcz);
        rot3(a.cam.camrot, G.lx - a.cam.campos[0], G.ly - a.cam.campos[1], G.lz - a.cam.campos[2], false, scx, scy, scz);
        }
        ppx = pcx / pcz; ppy = pcy / pcz; spx = scx / scz; spy = scy / scz;
    }
    float d0, d1, d2;
    if (FRAMES) d0 = d1 = d2 = dwx * G.fx + dwy * G.fy + dwz * G.fz;        // the thread's own component (q < 3)
    else rot3(a.cam.rw2c, dwx, dwy, dwz, true, d0, d1, d2);
    const float d3 = ppx * pcz - spx * scz, d4 = ppy * pcz - spy * scz, d5 = pcz - scz;
    const float da = q == 0 ? d0 : q == 1 ? d1 : q == 2 ? d2 : d3;
    const float db = q == 0 ? d4 : d5;
    // the thread's 8 embedding dims and their 3 octaves
    const float e[8] = {G.e0.x, G.e0.y, G.e0.z, G.e0.w, G.e1.x, G.e1.y, G.e1.z, G.e1.w};
    if (MIX) {
        pn_xq_store4(X, row, PN_EPT * q, e[0], e[1], e[2], e[3]);
        pn_xq_store4(X, row, PN_EPT * q + 4, e[4], e[5], e[6], e[7]);
        // two dims = 12 consecutive columns (a multiple of four from column 32 + 48 q on): three 4-column stores
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
            const int col = PN_F + (PN_EPT * q + i) * 6;
            float s0[3], c0[3], s1[3], c1[3];
            pn_pe_octaves<3>(e[i], s0, c0);
            pn_pe_octaves<3>(e[i + 1], s1, c1);
            pn_xq_store4(X, row, col, s0[0], c0[0], s0[1], c0[1]);
            pn_xq_store4(X, row, col + 4, s0[2], c0[2], s1[0], c1[0]);
            pn_xq_store4(X, row, col + 8, s1[1], c1[1], s1[2], c1[2]);
        }
    } else {
    pn_xt_store4(X, row, PN_EPT * q, e[0], e[1], e[2], e[3]); pn_xt_store4(X, row, PN_EPT * q + 4, e[4], e[5], e[6], e[7]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int dd = PN_EPT * q + i;
        float s[3], c[3];
        pn_pe_octaves<3>(e[i], s, c);
        pn_xt_store2(X, row, PN_F + dd * 6, s[0], c[0]);
        pn_xt_store2(X, row, PN_F + dd * 6 + 2, s[1], c[1]);
        pn_xt_store2(X, row, PN_F + dd * 6 + 4, s[2], c[2]);
    }
    }
    // PE5 of distance components q and q + 4
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int comp = q + 4 * j;
        if (comp < 6) {
            float s[5], c[5];
            pn_pe_octaves<5>(j == 0 ? da : db, s, c);
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                if (MIX) pn_xa_store2(X, row, PN_F * 7 + (comp * 5 + f) * 2, s[f], c[f]);
                else pn_xt_store2(X, row, PN_F * 7 + (comp * 5 + f) * 2, s[f], c[f]);
            }
        }
    }
    if (q == 3) pn_xt_store4(X, row, PN_ONES1, 1.f, 0.f, 0.f, 0.f);
    float fvx = 0.f, fvy = 0.f, fvz = 0.f, fqx = 0.f, fqy = 0.f, fqz = 0.f;
    if (FRAMES) {          // components q of the rotated view and point directions -> thread 0 of the row (lanes l, l + 1, l + 2 hold q = 0, 1, 2)
        fvx = G.rx * G.gx + G.ry * G.gy + G.rz * G.gz;
        fqx = G.dxv * G.fx + G.dyv * G.fy + G.dzv * G.fz;
        fvy = __shfl_down(fvx, 1, 64); fvz = __shfl_down(fvx, 2, 64);
        fqy = __shfl_down(fqx, 1, 64); fqz = __shfl_down(fqx, 2, 64);
    }
    if (q == 0) {
        float vx, vy, vz, qx, qy, qz;
        if (FRAMES) { vx = fvx; vy = fvy; vz = fvz; qx = fqx; qy = fqy; qz = fqz; }
        else {
        rot3(a.cam.rw2c, G.rx, G.ry, G.rz, true, vx, vy, vz);
        rot3(a.cam.rw2c, G.dxv, G.dyv, G.dzv, true, qx, qy, qz);
        }
        float *ex = exb + row * 8;
        *reinterpret_cast<float4 *>(ex) = make_float4(G.cx, G.cy, G.cz, qx - vx);
        if (FRAMES) {          // (the same sums in the uniform instance's order of products: see above)
            *reinterpret_cast<float4 *>(ex + 4) = make_float4(qy - vy, qz - vz, __builtin_fmaf(qz, vz, __builtin_fmaf(qx, vx, qy * vy)), 1.f);
            wraw[row] = p >= 0 ? 1.0f / fmaxf(sqrtf(__builtin_fmaf(dwz, dwz, __builtin_fmaf(dwx, dwx, dwy * dwy))), 1e-6f) : 0.f;
        } else {
        *reinterpret_cast<float4 *>(ex + 4) = make_float4(qy - vy, qz - vz, qx * vx + qy * vy + qz * vz, 1.f);
        wraw[row] = p >= 0 ? 1.0f / fmaxf(sqrtf(dwx * dwx + dwy * dwy + dwz * dwz), 1e-6f) : 0.f;
        }
        sidx[row] = si;
    }
}

// epilogue of a layer: accumulators + bias, LeakyReLU, sign bits, both planes -> the tile (columns 0..255).
// Sign word: one v_alignbit_b32 per element shifts the element's sign bit into a 32-bit accumulator (MSB first), element
// e = ((fb * 2 + rb) * 4 + g) * 4 + i of a lane -> bit 31 - (e & 31) of half e >> 5; bit set = negative = slope 0.01 in the backward
// The bias is the accumulators' INITIAL value (D = W X^T + b: a lane's element (fb, rb, g, i) belongs to feature pn_d_feat(..) + i, the
// same for both row blocks): requested before the tile's copy-out, in the accumulators when the GEMM starts -- the epilogue then holds
// no global data at all (round 2 loaded it behind the GEMM, and behind the next tile's gather in the in-order vmcnt queue).
__device__ __forceinline__ void f_acc_bias(const float *__restrict__ bias, int wave, int lane, f32x16 (&acc)[PN_NFB][2]) {
#pragma unroll
    for (int fb = 0; fb < PN_NFB; ++fb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b = *reinterpret_cast<const float4 *>(bias + pn_d_feat(PN_NFB * wave + fb, g, lane));
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) { acc[fb][rb][4 * g] = b.x; acc[fb][rb][4 * g + 1] = b.y; acc[fb][rb][4 * g + 2] = b.z; acc[fb][rb][4 * g + 3] = b.w; }
        }
}
// epilogue of a layer: LeakyReLU of the accumulators (bias included), sign bits, both planes -> the tile (columns 0..255).
// Sign word: one v_alignbit_b32 per element shifts the element's sign bit into a 32-bit accumulator (MSB first), element
// e = (rb * 4 + g) * 4 + i of a lane's feature block -> bit 31 - e of the block's word; bit set = negative = slope 0.01 in the backward.
// mw[fb] = the word of the wave's feature block fb (global block PN_NFB * wave + fb): stored as lmask[tile][layer][block][lane].
template <bool BITS, bool MIX = false, bool HR = false>
__device__ __forceinline__ void f_epilogue(const f32x16 (&acc)[PN_NFB][2], char *X, int wave, int lane, unsigned (&mw)[PN_NFB]) {
#pragma unroll
    for (int fb = 0; fb < PN_NFB; ++fb) mw[fb] = 0u;
#pragma unroll
    for (int fb = 0; fb < PN_NFB; ++fb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int f0 = pn_d_feat(PN_NFB * wave + fb, g, lane);
                float v[4] = {acc[fb][rb][4 * g], acc[fb][rb][4 * g + 1], acc[fb][rb][4 * g + 2], acc[fb][rb][4 * g + 3]};
                if (BITS) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) mw[fb] = __builtin_amdgcn_alignbit(mw[fb], __float_as_uint(v[i]), 31);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.01f * v[i]);
                if (MIX) pn_xq_store4(X, 32 * rb + (lane & 31), f0, v[0], v[1], v[2], v[3]);
                else if (HR) pn_xt_store4(X, 32 * rb + (lane & 31), f0, v[0], v[1], v[2], v[3]);
                else pn_x_store4<false>(X, 32 * rb + (lane & 31), f0, v[0], v[1], v[2], v[3]);
            }
}
// the sign words of a layer -> lmask[gtile][layer][block][lane]
__device__ __forceinline__ void f_store_masks(unsigned *__restrict__ lmask, long long gtile, int layer, int wave, int lane, const unsigned (&mw)[PN_NFB]) {
#pragma unroll
    for (int fb = 0; fb < PN_NFB; ++fb) lmask[((gtile * 3 + layer) * 8 + PN_NFB * wave + fb) * 64 + lane] = mw[fb];
}

// ---- the tile's tail in ONE pass over the h4 tile, for K in {1, 2, 4, 8} (the rows of a sample then never straddle a thread's 8 rows):
// thread -> columns 8 (tid & 31) .. + 7 of rows 8 (tid >> 5) .. + 7.  Per row: both planes read once (ds_read_b128), streamed to HBM as
// the backward's h4 (training), dotted with the alpha head's weights and added, weighted, to the thread's per-sample sums f.  The rows'
// alpha dot products are then reduced over the 32 lanes that share the rows by a transposing butterfly (8 -> 4 -> 2 -> 1 values per
// lane: 7 + 2 shuffles instead of 8 x 5), softplus runs once per row, sigma is summed over a sample's rows by log2(KC) more shuffles.
// Round 2 made three passes (alpha head, h4 copy, K-sums: 64 LDS reads per thread and two barriers); this is 16 reads and no barrier.
// KC = 0 (round 5): any other K (12 / 6 / 3 of the Barn configuration, ...): the per-ROW half of the pass -- both planes read once, streamed
// out as the backward's h4, the alpha head's dot product, butterfly, softplus -- with the rows' weighted alpha left in `wraw` for the K-sums
// pass that follows behind one barrier (a sample's rows then straddle the threads' 8-row strips).  The three-pass form it replaces read the
// tile three times with two barriers.
template <int KC, bool TRAIN>
__device__ __forceinline__ void f_tail(const FwdArgs &a, const char *X, const float *w5s, const float *wrow, const int *sidx, float b5,
                                       long long tile, long long gtile, int tid, float *wraw = nullptr) {
    constexpr int NS = KC == 0 ? 1 : 8 / (KC == 0 ? 1 : KC);                      // samples per thread
    const int lane = tid & 63, cg = tid & 31, r0 = 8 * (tid >> 5);
    const float4 wa = *reinterpret_cast<const float4 *>(w5s + 8 * cg), wb = *reinterpret_cast<const float4 *>(w5s + 8 * cg + 4);
    float pa[8];
    float4 fa[NS], fb[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) fa[j] = fb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = r0 + i;
        const uint4 h = *reinterpret_cast<const uint4 *>(X + r * PN_XRS + cg * 16);
        const uint4 m = *reinterpret_cast<const uint4 *>(X + PN_XPLANE + r * PN_XRS + cg * 16);
        if (TRAIN) {
            pn_f4 th = {__uint_as_float(h.x), __uint_as_float(h.y), __uint_as_float(h.z), __uint_as_float(h.w)};
            pn_f4 tm = {__uint_as_float(m.x), __uint_as_float(m.y), __uint_as_float(m.z), __uint_as_float(m.w)};
            PN_STREAM_STORE(th, reinterpret_cast<pn_f4 *>(a.sv.h4r + (gtile * PN_TILE + r) * 32 + cg));
            PN_STREAM_STORE(tm, reinterpret_cast<pn_f4 *>(a.sv.h4r + (a.sv.rows + gtile * PN_TILE + r) * 32 + cg));
        }
        float s = 0.f;
        s = pn_fma2_lo(h.x, m.x, wa.x, s); s = pn_fma2_hi(h.x, m.x, wa.y, s); s = pn_fma2_lo(h.y, m.y, wa.z, s); s = pn_fma2_hi(h.y, m.y, wa.w, s);
        s = pn_fma2_lo(h.z, m.z, wb.x, s); s = pn_fma2_hi(h.z, m.z, wb.y, s); s = pn_fma2_lo(h.w, m.w, wb.z, s); s = pn_fma2_hi(h.w, m.w, wb.w, s);
        pa[i] = s;
        if (KC != 0) {
            const float w = wrow[r];
            float4 &f0 = fa[i / (KC == 0 ? 1 : KC)], &f1 = fb[i / (KC == 0 ? 1 : KC)];
            f0.x = pn_fma2_lo(h.x, m.x, w, f0.x); f0.y = pn_fma2_hi(h.x, m.x, w, f0.y); f0.z = pn_fma2_lo(h.y, m.y, w, f0.z); f0.w = pn_fma2_hi(h.y, m.y, w, f0.w);
            f1.x = pn_fma2_lo(h.z, m.z, w, f1.x); f1.y = pn_fma2_hi(h.z, m.z, w, f1.y); f1.z = pn_fma2_lo(h.w, m.w, w, f1.z); f1.w = pn_fma2_hi(h.w, m.w, w, f1.w);
        }
    }
    // f rows of the thread's samples (class-ordered list: the colour MLP reads them in that order)
#pragma unroll
    for (int j = 0; j < (KC == 0 ? 0 : NS); ++j) {
        const long long vs = tile * (PN_TILE / (KC == 0 ? 1 : KC)) + (r0 / (KC == 0 ? 1 : KC)) + j;
        if (vs < a.cap_samples) {
            *reinterpret_cast<float4 *>(a.sv.fs + vs * PN_H + 8 * cg) = fa[j];
            *reinterpret_cast<float4 *>(a.sv.fs + vs * PN_H + 8 * cg + 4) = fb[j];
        }
    }
    // transposing butterfly over the 32 lanes of the row set: after the three halving steps a lane holds ONE row's partial sum,
    // row index i = 4 b4 + 2 b3 + b2 (bits of the lane), then two full steps over bits 1, 0
    {
        const bool b4 = lane & 16, b3 = lane & 8, b2 = lane & 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float send = b4 ? pa[j] : pa[j + 4], keep = b4 ? pa[j + 4] : pa[j]; pa[j] = keep + __shfl_xor(send, 16, 64); }
#pragma unroll
        for (int j = 0; j < 2; ++j) { const float send = b3 ? pa[j] : pa[j + 2], keep = b3 ? pa[j + 2] : pa[j]; pa[j] = keep + __shfl_xor(send, 8, 64); }
        { const float send = b2 ? pa[0] : pa[1], keep = b2 ? pa[1] : pa[0]; pa[0] = keep + __shfl_xor(send, 4, 64); }
        pa[0] += __shfl_xor(pa[0], 2, 64);
        pa[0] += __shfl_xor(pa[0], 1, 64);
        const int i = ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1), r = r0 + i;
        const float x = pa[0] + b5 - 1.0f;
        float sg = pn_softplus(x) * wrow[r];
        if (TRAIN && (lane & 3) == 0) a.sv.arow[gtile * PN_TILE + r] = x;
        if (KC == 0) {              // the row's share of sigma: summed per sample by the K-sums pass
            if ((lane & 3) == 0) wraw[r] = sg;
            return;
        }
        // sigma of a sample = sum over its KC rows: rows i differ in the low log2(KC) bits of i = lane bits 2 .. (b2 is i's bit 0)
        if (KC >= 2) sg += __shfl_xor(sg, 4, 64);
        if (KC >= 4) sg += __shfl_xor(sg, 8, 64);
        if (KC >= 8) sg += __shfl_xor(sg, 16, 64);
        if ((lane & 3) == 0 && (i % (KC == 0 ? 1 : KC)) == 0) {
            const int si = sidx[r];
            if (si >= 0) a.decoded[(long long)si * 4] = sg;
        }
    }
}

#ifdef PN_PHASE_TRACE
PN_TR_DECL(pn_trace_fwd);
PN_TR_SPAN_DECL(pn_span_fwd);
#endif
// WG2: the two-plane weight-gradient mode (pnerf_set_wgrad_planes(2)): every saved GEMM operand also leaves its residual plane, X0 whole
// NP = 4: the mixed format of mixq.h (f16 h.h + e4m3 cross terms: the default since round 6); NP = 3 / 2: f16x3.h's three / two f16 products
// FRAMES: per-point Rw2c frames (a.frames; inference only, f16 cross terms and three products)
template <bool TRAIN, bool PERS, int NP, bool WG2 = false, bool FRAMES = false>
__global__ __launch_bounds__(PN_NTHR, PN_NW / 2) void k_agg_forward(typename FwdArgsOf<FRAMES>::type a) {
    constexpr bool MIX = NP == 4;
    static_assert(!FRAMES || (!TRAIN && NP == 3), "per-point frames: the default inference arithmetic only");
    // Store forms of the tile: the feature build and the epilogues of layers 1-3 write "nearest" planes (MIX: the mixed format; else f16x3 planes with
    // h rounded to nearest, HR: inference and training alike, the same bits); the layer-4 epilogue writes f16x3.h's classic split (f_epilogue<false>),
    // which is what f_tail and the backward's h4 read
    constexpr bool HR = !MIX;
    constexpr bool HC = TRAIN && !WG2;              // the k-major copy-outs read the h plane alone
    static_assert(!(MIX && WG2), "the two-plane weight-gradient mode keeps f16x3.h's arithmetic everywhere");
    pn_mode_saturate();
    extern __shared__ __attribute__((aligned(16))) char smem_f[];
    char *X = smem_f;
    float *exb = reinterpret_cast<float *>(smem_f + FL_EX), *w5s = reinterpret_cast<float *>(smem_f + FL_W5);
    float *wraw = reinterpret_cast<float *>(smem_f + FL_ROW), *wrow = wraw + PN_TILE, *wnrm = wrow + PN_TILE;
    int *sidx = reinterpret_cast<int *>(wnrm + PN_TILE);
    const float *frames = nullptr;
    if constexpr (FRAMES) frames = a.frames;
    const int tid0 = threadIdx.x;
    const int K = a.K, TS = a.TS;
    const unsigned kinv = pn_kinv(K);
    // this launch processes one sample class: its list, its run of tiles, its range of per-sample rows
    const int Ns = a.cls_info[PN_CI_COUNT + a.cls];
    const long long vb = a.cls_info[PN_CI_VBASE + a.cls], tb = a.cls_info[PN_CI_TBASE + a.cls];
    a.valid_list = a.cls_list + vb; a.cap_samples = Ns;
    a.sv.fs += vb * PN_H;
    const long long ntiles = ((long long)Ns + TS - 1) / TS;
    const float *P = a.params;
    const char *img = reinterpret_cast<const char *>(a.packed);
    if (tid0 < PN_H) w5s[tid0] = P[PO_W5 + tid0];
    const float b5 = P[PO_B5];
    // tiles of a workgroup: blockIdx.x + j * gridDim.x for j < PN_CLAIM_STATIC_FWD (what the index pipeline below looks ahead), then whatever it
    // claims (mlp_common.h: dynamic tile claim) -- in ascending order, so the chip still works on one moving window of the saved area (one
    // contiguous run of tiles per workgroup measured the same, 12.85 against 12.90 ms).  t0 .. t2: this tile and the next two, uniform
    const int tile_last = (int)ntiles, grid = gridDim.x;
    int t0 = blockIdx.x, t1 = t0 + grid, t2 = t1 + grid;
    if (t0 >= tile_last) return;
    int *claim_ctr = a.sv.cls_info + PN_CI_CLAIM + a.cls, *claim_w = reinterpret_cast<int *>(smem_f + FL_CLAIM);
    int nclaim = 0;                                    // claim sequence number of the tile the NEXT iteration learns (its t3)

    // index pipeline of this thread's row (4 threads per tile row): (si0, p0) current tile, (si1, p1) next, si2 the one after
    long long tile = t0;
    int si0, si1, si2, p0, p1;
    FGather G;
    {
        const int row = tid0 / PN_TPR, q = tid0 % PN_TPR, k = row - pn_row_div(row, kinv) * K;
        si0 = f_sample_of(a, tile, row, Ns, kinv); si1 = t1 < tile_last ? f_sample_of(a, t1, row, Ns, kinv) : -1;
        si2 = t2 < tile_last ? f_sample_of(a, t2, row, Ns, kinv) : -1;
        p0 = si0 >= 0 ? a.pidx[(long long)si0 * a.Kstride + k] : -1;
        p1 = si1 >= 0 ? a.pidx[(long long)si1 * a.Kstride + k] : -1;
        f_gather<PERS, FRAMES>(a, G, si0, p0, q, frames);
    }

    f32x16 acc[PN_NFB][2];
    PN_TR_ITER_DECL;
    for (bool first = true; t0 < tile_last; first = false) {
        PN_TR_ITER_NEXT;
        tile = t0;
        // thread-index-derived offsets are recomputed per tile: hoisted out of the loop they become hundreds of loop-carried
        // registers (every LDS / bias / image address of every unrolled store) and spill
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int row = tid / PN_TPR, q = tid % PN_TPR, k = row - pn_row_div(row, kinv) * K;
        const long long gtile = tb + tile;               // tile index inside the saved area
        PN_LDS_BARRIER();                                 // the previous tile's readers are done with X and the row arrays
        PN_TR(pn_trace_fwd, 0); PN_TR_HWID(pn_trace_fwd); PN_TR_SPAN(pn_span_fwd, a.cls, 0);
        f_build<PERS, MIX, FRAMES>(a, G, X, exb, wraw, sidx, si0, p0, row, q);
        // Round 4: what the next GEMM needs from GLOBAL memory -- its bias (the accumulators' initial value) and its first weight-fragment
        // chunks -- is requested in front of the barrier that precedes it, not behind: neither depends on LDS, and the L2 round trip
        // (0.6 .. 1.1 us per layer in profiles/r03_phase_trace.json: the "acc = bias" phases) passes under the barrier wait.
        f_acc_bias(P + PO_B1, wave, lane, acc);
        PnTileW<MIX, 2, 8, NP> W1;
        W1.prefetch(img, PKH_F1, PKM_F1, PN_NFB * wave, lane);
        PN_LDS_BARRIER();
        if (q == 0) {      // weights of the row: normalise over the K slots, multiply by the clamped confidence (:801-811)
            const int ls = pn_row_div(row, kinv);
            float wn = 0.f, w = 0.f;
            if (si0 >= 0) {
                float sum = 0.f;
                for (int kk = 0; kk < K; ++kk) sum += wraw[ls * K + kk];
                wn = wraw[row] / fmaxf(sum, 1e-8f);
                w = wn * fminf(fmaxf(G.cf, 1e-4f), 1.0f);
                a.weight[(long long)si0 * a.Kstride + k] = wn;
            }
            wnrm[row] = wn; wrow[row] = w;
            if (TRAIN) a.sv.rmeta[gtile * PN_TILE + row] = make_int4(si0, si0 >= 0 ? p0 : -1, __float_as_int(wn), __float_as_int(w));
        }
        unsigned mask[PN_NFB];
        PN_TR(pn_trace_fwd, 1);
        // ---- layer 1: 288 -> 256.  Training: the layer's input tile is copied out (k-major planes for the weight-gradient GEMM) BEHIND the
        // layer's GEMM, not in front of it: vmcnt counts loads and stores of a wave in ONE in-order queue, so a GEMM that starts right
        // behind 20 stores waits for their acknowledgements from HBM before its first weight fragment counts as arrived (round 2 order:
        // every GEMM phase carried 1 .. 3 us of that).  Behind the GEMM the stores have the epilogue and two barriers to drain.
        PN_TR(pn_trace_fwd, 2);
        W1.run(X, lane, acc);
        if (TRAIN) {           // (behind the GEMM: see above)
            if (HC) {         // the tile's h plane IS the nearest f16: the k-major plane is its transpose
                if (a.save_x0) pn_copy_out_kmajor_h<PN_NF1>(X, a.sv.x0k, gtile * 8, tid);
                else pn_copy_out_kmajor_cols64_h<224>(X, a.sv.x0k, gtile * 8, tid);
            } else if (WG2) pn_copy_out_kmajor<PN_NF1, true>(X, a.sv.x0k, gtile * 8, tid, a.sv.x0m);
            else if (a.save_x0) pn_copy_out_kmajor<PN_NF1, false>(X, a.sv.x0k, gtile * 8, tid);
            else pn_copy_out_kmajor_cols64<224>(X, a.sv.x0k, gtile * 8, tid);       // the fused path: only the last 64 columns (k_wgrad_x0)
        }
        PN_LDS_BARRIER();
        PN_TR(pn_trace_fwd, 3);
        f_epilogue<TRAIN, MIX, HR>(acc, X, wave, lane, mask);
        if (TRAIN) f_store_masks(a.sv.lmask, gtile, 0, wave, lane, mask);
        f_acc_bias(P + PO_B2, wave, lane, acc);
        PnTileW<MIX, 0, 8, NP> W2;
        W2.prefetch(img, PKH_F2, PKM_F2, PN_NFB * wave, lane);
        PN_LDS_BARRIER();
        PN_TR(pn_trace_fwd, 4);
        // ---- layer 2: 256 -> 256
        PN_TR(pn_trace_fwd, 5);
        W2.run(X, lane, acc);
        if (TRAIN) {      // (behind the GEMM: see below)
            if (HC) pn_copy_out_kmajor_h<PN_H>(X, a.sv.h1k, gtile * 8, tid);
            else pn_copy_out_kmajor<PN_H, WG2>(X, a.sv.h1k, gtile * 8, tid, a.sv.h1m);
        }
        PN_LDS_BARRIER();
        PN_TR(pn_trace_fwd, 6);
        f_epilogue<TRAIN, MIX, HR>(acc, X, wave, lane, mask);
        if (TRAIN) f_store_masks(a.sv.lmask, gtile, 1, wave, lane, mask);
        if (tid < PN_TILE) {     // the row's extras next to h2: columns 256..262, the ones column, zeros up to 271
            const float4 u = *reinterpret_cast<const float4 *>(exb + tid * 8), v = *reinterpret_cast<const float4 *>(exb + tid * 8 + 4);
            pn_xt_store4(X, tid, PN_H, u.x, u.y, u.z, u.w);
            pn_xt_store4(X, tid, PN_H + 4, v.x, v.y, v.z, v.w);
            pn_xt_store4(X, tid, PN_H + 8, 0.f, 0.f, 0.f, 0.f);
            pn_xt_store4(X, tid, PN_H + 12, 0.f, 0.f, 0.f, 0.f);
        }
        f_acc_bias(P + PO_B3, wave, lane, acc);
        PnTileW<MIX, 1, 8, NP> W3;
        W3.prefetch(img, PKH_F3, PKM_F3, PN_NFB * wave, lane);
        PN_LDS_BARRIER();
        PN_TR(pn_trace_fwd, 7);
        // ---- layer 3: 256 + 7 -> 256
        PN_TR(pn_trace_fwd, 8);
        W3.run(X, lane, acc);
        if (TRAIN) {      // (behind the GEMM: see below)
            if (HC) pn_copy_out_kmajor_h<PN_NF1>(X, a.sv.h2k, gtile * 8, tid);
            else pn_copy_out_kmajor<PN_NF1, WG2>(X, a.sv.h2k, gtile * 8, tid, a.sv.h2m);
        }
        PN_LDS_BARRIER();
        PN_TR(pn_trace_fwd, 9);
        f_epilogue<TRAIN, MIX, HR>(acc, X, wave, lane, mask);
        if (TRAIN) f_store_masks(a.sv.lmask, gtile, 2, wave, lane, mask);
        f_acc_bias(P + PO_B4, wave, lane, acc);
        PnTileW<MIX, 0, 8, NP> W4;
        W4.prefetch(img, PKH_F4, PKM_F4, PN_NFB * wave, lane);
        PN_LDS_BARRIER();
        PN_TR(pn_trace_fwd, 10);
        // ---- layer 4: 256 -> 256
        PN_TR(pn_trace_fwd, 11);
        W4.run(X, lane, acc);
        if (TRAIN) {
            if (HC) pn_copy_out_kmajor_h<PN_H>(X, a.sv.h3k, gtile * 8, tid);
            else pn_copy_out_kmajor<PN_H, WG2>(X, a.sv.h3k, gtile * 8, tid, a.sv.h3m);
        }
        PN_TR(pn_trace_fwd, 12);
        // the next tile's point data and the indices of the two after it: requested here, consumed at the top of the next
        // iteration -- their HBM latency passes under the element-wise tail of this tile (nothing of this tile waits for memory any more)
        // the tile three ahead: static in the first iteration, else the claim the previous iteration left in LDS (barriers lie between its write
        // at the end of that iteration, this read, and the next write).  This iteration's own claim is requested here, in front of the loads below,
        // and lands in LDS at the end of the iteration: its round trip passes under the layer-4 epilogue and the tail
        const int t3 = first ? t2 + grid : pn_claim_tile(PN_CLAIM_STATIC_FWD, grid, __builtin_amdgcn_readfirstlane(*claim_w), nclaim - 1);
        const bool claims = nclaim % PN_CLAIM_TILES == 0;
        int claimed = 0;
        if (tid == 0 && claims) claimed = atomicAdd(claim_ctr, 1);
        const int si_next = si1, p_next = p1;
        if (t1 < tile_last) f_gather<PERS, FRAMES>(a, G, si1, p1, q, frames);
        const int p2 = si2 >= 0 ? a.pidx[(long long)si2 * a.Kstride + k] : -1;
        const int si3 = t3 < tile_last ? f_sample_of(a, t3, row, Ns, kinv) : -1;
        PN_LDS_BARRIER();
        PN_TR(pn_trace_fwd, 13);
        f_epilogue<false>(acc, X, wave, lane, mask);
        PN_LDS_BARRIER();
        PN_TR(pn_trace_fwd, 14);
        if (K == 8 || K == 4 || K == 2 || K == 1) {
            // ---- alpha head + h4 copy + K-weighted sums + sigma in one pass (f_tail)
            if (K == 8) f_tail<8, TRAIN>(a, X, w5s, wrow, sidx, b5, tile, gtile, tid);
            else if (K == 4) f_tail<4, TRAIN>(a, X, w5s, wrow, sidx, b5, tile, gtile, tid);
            else if (K == 2) f_tail<2, TRAIN>(a, X, w5s, wrow, sidx, b5, tile, gtile, tid);
            else f_tail<1, TRAIN>(a, X, w5s, wrow, sidx, b5, tile, gtile, tid);
            PN_TR(pn_trace_fwd, 15);
        } else {
        // ---- (any other K: two passes) the per-row half in f_tail's mapping (alpha head 256 -> 1, softplus(x - 1), raw2out_density :262-265; h4 planes
        // streamed out for the backward), then the K-weighted sums
        f_tail<0, TRAIN>(a, X, w5s, wrow, sidx, b5, tile, gtile, tid, wraw);
        PN_LDS_BARRIER();
        PN_TR(pn_trace_fwd, 15);
        // ---- K-weighted sums -> f[256] per sample (HBM), sigma
        for (int e = tid; e < TS * 32; e += PN_NTHR) {          // item = (sample, 8 columns): 16-byte reads of both planes, K rows
            const int ls = e >> 5, cg = e & 31;
            float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
            for (int kk = 0; kk < K; ++kk) {
                const int r = ls * K + kk;
                const uint4 h = *reinterpret_cast<const uint4 *>(X + r * PN_XRS + cg * 16);
                const uint4 m = *reinterpret_cast<const uint4 *>(X + PN_XPLANE + r * PN_XRS + cg * 16);
                const float w = wrow[r];
                f0.x = pn_fma2_lo(h.x, m.x, w, f0.x); f0.y = pn_fma2_hi(h.x, m.x, w, f0.y); f0.z = pn_fma2_lo(h.y, m.y, w, f0.z); f0.w = pn_fma2_hi(h.y, m.y, w, f0.w);
                f1.x = pn_fma2_lo(h.z, m.z, w, f1.x); f1.y = pn_fma2_hi(h.z, m.z, w, f1.y); f1.z = pn_fma2_lo(h.w, m.w, w, f1.z); f1.w = pn_fma2_hi(h.w, m.w, w, f1.w);
            }
            const long long vs = tile * TS + ls;
            if (vs < a.cap_samples) {
                *reinterpret_cast<float4 *>(a.sv.fs + vs * PN_H + 8 * cg) = f0;
                *reinterpret_cast<float4 *>(a.sv.fs + vs * PN_H + 8 * cg + 4) = f1;
            }
        }
        if (tid < TS) {
            const int si = sidx[tid * K];
            if (si >= 0) {
                float sg = 0.f;
                for (int kk = 0; kk < K; ++kk) sg += wraw[tid * K + kk];
                a.decoded[(long long)si * 4] = sg;
            }
        }
        }
        si0 = si_next; p0 = p_next; si1 = si2; p1 = p2; si2 = si3;
        if (tid == 0 && claims) *claim_w = claimed;
        t0 = t1; t1 = t2; t2 = t3; ++nclaim;
        PN_TR(pn_trace_fwd, 16); PN_TR_SPAN(pn_span_fwd, a.cls, 1);
    }
}

// ------------------------------------------------------------------------------ colour MLP forward
// 64 valid samples per tile: [f (256) | view-direction encoding (24) | 0 (8)] -> 128 -> 128 -> 128 -> 3, the three 128-wide layers as
// two-plane f16 GEMMs (f16x3.h: one 32-feature block per wave, 18 / 8 / 8 chunks), the 3-wide output layer and the sigmoid on the
// VALU.  One activation tile in LDS, reused layer after layer; the post-activations the backward needs (LeakyReLU masks, the fp32
// weight-gradient GEMMs of these three layers) leave from the accumulator registers as fp32 rows.
constexpr int CL_W4 = PN_XBYTES, CL_BYTES = CL_W4 + 3 * PN_HC * 4;
static_assert(2 * CL_BYTES <= 160 * 1024, "two colour workgroups must fit the 160 KB LDS");

__device__ __forceinline__ void c_load_bias(const float *__restrict__ bias, int wave, int lane, float4 (&b)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {         // (scalar loads: the colour tensors sit at odd float offsets of the parameter vector)
        const float *p = bias + pn_d_feat(wave, g, lane);
        b[g] = make_float4(p[0], p[1], p[2], p[3]);
    }
}
// bias + LeakyReLU of the wave's feature block, two planes into the tile.  Training: SAVE32 -> the fp32 rows to `save` (the last layer:
// the backward needs its values); else the sign bits of the lane's 32 pre-activations (rb, g, i order, first element in bit 31)
template <bool TRAIN, bool SAVE32>
__device__ __forceinline__ unsigned c_epilogue(const f32x16 (&acc)[2][2], const float4 (&bias)[4], char *X, int wave, int lane, float *__restrict__ save, long long grow0) {
    unsigned mw = 0u;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int f0 = pn_d_feat(wave, g, lane), row = 32 * rb + (lane & 31);
            const float4 b = bias[g];
            float v[4] = {acc[0][rb][4 * g] + b.x, acc[0][rb][4 * g + 1] + b.y, acc[0][rb][4 * g + 2] + b.z, acc[0][rb][4 * g + 3] + b.w};
            if (TRAIN && !SAVE32) {
#pragma unroll
                for (int i = 0; i < 4; ++i) mw = __builtin_amdgcn_alignbit(mw, __float_as_uint(v[i]), 31);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.01f * v[i]);
            if (TRAIN && SAVE32) {
                pn_f4 t = {v[0], v[1], v[2], v[3]};
                PN_REG_STORE(t, reinterpret_cast<pn_f4 *>(save + (grow0 + row) * PN_HC + f0));
            }
            pn_x_store4<false>(X, row, f0, v[0], v[1], v[2], v[3]);
        }
    return mw;
}

// FRAMES: the view direction is rotated by the frame of the sample's slot-0 point (a.frames) instead of cam.rw2c
template <bool TRAIN, int NP, bool WG2 = false, bool FRAMES = false>
__global__ __launch_bounds__(256, 2) void k_color_forward(typename FwdArgsOf<FRAMES>::type a) {
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    char *X = smem_c;
    float *w4s = reinterpret_cast<float *>(smem_c + CL_W4);       // [3][128] output layer
    const int Ns = a.counters[0] < a.cap_samples ? a.counters[0] : (int)a.cap_samples;
    const float *P = a.params;
    const char *img = reinterpret_cast<const char *>(a.packed);
    for (int i = threadIdx.x; i < 3 * PN_HC; i += 256) w4s[i] = P[PO_WC4 + i];
    const float b40 = P[PO_BC4], b41 = P[PO_BC4 + 1], b42 = P[PO_BC4 + 2];

    f32x16 acc[2][2];
    for (long long tile = blockIdx.x; tile * PN_CTILE < Ns; tile += gridDim.x) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), row = tid >> 2, q = tid & 3;
        const long long grow0 = tile * PN_CTILE, vs = grow0 + row;
        const int si = vs < Ns ? a.valid_list[vs] : -1;
        // (round 4: the first weight-fragment chunks of a GEMM -- here 7 of a layer's 8 or 18 -- are requested in front of the barrier that
        //  precedes it; a colour tile has 3.5 us of MFMA work in ~25 us, the L2 round trips at the start of its three GEMMs were exposed)
        PnGemmW<18, 4, 1, 7, NP> WC1;
        WC1.prefetch(reinterpret_cast<const uint4 *>(img + PKH_FC1), wave, lane);
        PN_LDS_BARRIER();                                 // the previous tile's readers are done with X
        if (si >= 0) {
            // the row's four threads take interleaved 16-byte pieces (piece 4 c + q): a wave's load instruction reads whole 64-byte segments of
            // 16 rows, its LDS stores land on 8 consecutive banks per row (round 4; one contiguous quarter row per thread touched 64 different
            // segments per instruction and put threads 0 / 2 and 1 / 3 of a row on the same banks: half of this kernel's LDS cycles were conflicts)
            const float4 *f = reinterpret_cast<const float4 *>(a.sv.fs + vs * PN_H);
            float4 fv[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) fv[c] = f[4 * c + q];
#pragma unroll
            for (int c = 0; c < 16; ++c) pn_x_store4<false>(X, row, 16 * c + 4 * q, fv[c].x, fv[c].y, fv[c].z, fv[c].w);
            {   // positional_encoding(viewdirs, 4, ori=True)[..., 3:] = [sin(v_d 2^f) (d-major) | cos(...)]   networks.py:185-187
                // thread q < 3 of the row: direction component q, its four frequencies (columns 256 + 4 q .. and 268 + 4 q ..)
                const int r = si / a.SR;
                float v[3], sn[4], cs[4];
                if constexpr (FRAMES) {
                    const int ps_ = a.pidx[(long long)si * a.Kstride], ps = ps_ > 0 ? ps_ : 0;
                    const float *fp = a.frames + (long long)ps * 9;
                    const float fm[9] = {fp[0], fp[1], fp[2], fp[3], fp[4], fp[5], fp[6], fp[7], fp[8]};
                    rot3(fm, a.raydir[3 * r], a.raydir[3 * r + 1], a.raydir[3 * r + 2], true, v[0], v[1], v[2]);
                } else
                rot3(a.cam.rw2c, a.raydir[3 * r], a.raydir[3 * r + 1], a.raydir[3 * r + 2], true, v[0], v[1], v[2]);
                const float vq = q == 0 ? v[0] : (q == 1 ? v[1] : v[2]);
                pn_pe_octaves<4>(vq, sn, cs);
                if (q < 3) {
                    pn_x_store4<false>(X, row, PN_H + 4 * q, sn[0], sn[1], sn[2], sn[3]);
                    pn_x_store4<false>(X, row, PN_H + 12 + 4 * q, cs[0], cs[1], cs[2], cs[3]);
                } else {
                    pn_x_store4<false>(X, row, PN_H + 24, 0.f, 0.f, 0.f, 0.f);
                    pn_x_store4<false>(X, row, PN_H + 28, 0.f, 0.f, 0.f, 0.f);
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 18; ++c) pn_x_store4<false>(X, row, 16 * c + 4 * q, 0.f, 0.f, 0.f, 0.f);
        }
        PN_LDS_BARRIER();
        float4 bias[4];
        // ---- layer 1: 280 (288) -> 128.  Training: every layer's input tile leaves k-major for the weight-gradient GEMM
        if (TRAIN) pn_copy_out_kmajor<PN_NF1, WG2>(X, a.sv.xck, tile * 8, tid, a.sv.xcm);
        pn_acc_zero(acc);
        pn_gemm_f16x3_run<18, 4, 1, 7, NP>(X, WC1, lane, acc);
        c_load_bias(P + PO_BC1, wave, lane, bias);
        PN_LDS_BARRIER();                                 // every wave is done reading the input tile
        unsigned mw = c_epilogue<TRAIN, false>(acc, bias, X, wave, lane, nullptr, grow0);
        if (TRAIN) a.sv.cmask[(tile * 2 + 0) * 256 + tid] = mw;
        PnGemmW<8, 4, 1, 7, NP> WC2;
        WC2.prefetch(reinterpret_cast<const uint4 *>(img + PKH_FC2), wave, lane);
        PN_LDS_BARRIER();
        // ---- layer 2
        if (TRAIN) pn_copy_out_kmajor<PN_HC, WG2>(X, a.sv.c1k, tile * 8, tid, a.sv.c1m);
        pn_acc_zero(acc);
        pn_gemm_f16x3_run<8, 4, 1, 7, NP>(X, WC2, lane, acc);
        c_load_bias(P + PO_BC2, wave, lane, bias);
        PN_LDS_BARRIER();
        mw = c_epilogue<TRAIN, false>(acc, bias, X, wave, lane, nullptr, grow0);
        if (TRAIN) a.sv.cmask[(tile * 2 + 1) * 256 + tid] = mw;
        PnGemmW<8, 4, 1, 7, NP> WC3;
        WC3.prefetch(reinterpret_cast<const uint4 *>(img + PKH_FC3), wave, lane);
        PN_LDS_BARRIER();
        // ---- layer 3
        if (TRAIN) pn_copy_out_kmajor<PN_HC, WG2>(X, a.sv.c2k, tile * 8, tid, a.sv.c2m);
        pn_acc_zero(acc);
        pn_gemm_f16x3_run<8, 4, 1, 7, NP>(X, WC3, lane, acc);
        c_load_bias(P + PO_BC3, wave, lane, bias);
        PN_LDS_BARRIER();
        c_epilogue<TRAIN, true>(acc, bias, X, wave, lane, a.sv.c3, grow0);
        PN_LDS_BARRIER();
        // ---- output layer 128 -> 3 and the colour activation: 4 threads per row, 32 columns each
        {
            float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c0 = q * 32 + 8 * j;
                o0 = pn_x_dot8(X, row, c0, *reinterpret_cast<const float4 *>(w4s + c0), *reinterpret_cast<const float4 *>(w4s + c0 + 4), o0);
                o1 = pn_x_dot8(X, row, c0, *reinterpret_cast<const float4 *>(w4s + PN_HC + c0), *reinterpret_cast<const float4 *>(w4s + PN_HC + c0 + 4), o1);
                o2 = pn_x_dot8(X, row, c0, *reinterpret_cast<const float4 *>(w4s + 2 * PN_HC + c0), *reinterpret_cast<const float4 *>(w4s + 2 * PN_HC + c0 + 4), o2);
            }
            o0 = group_sum<4>(o0); o1 = group_sum<4>(o1); o2 = group_sum<4>(o2);
            if (q == 0 && si >= 0) {
                float *o = a.decoded + (long long)si * 4;
                o[1] = 1.0f / (1.0f + expf(-(o0 + b40))) * 1.002f - 0.001f;                                     // raw2out_color :269-273
                o[2] = 1.0f / (1.0f + expf(-(o1 + b41))) * 1.002f - 0.001f;
                o[3] = 1.0f / (1.0f + expf(-(o2 + b42))) * 1.002f - 0.001f;
            }
        }
    }
}
}  // namespace

// ------------------------------------------------------------------------------ arithmetic settings (include/pnerf.h: pnerf_set_*)
// One record, process-wide.  products: per multiply-add of the INFERENCE forward (training always runs three; f16x3.h NP).  wgrad_planes: per
// operand of the weight-gradient GEMMs.  cross_terms: 8 = e4m3 (mixq.h; the default) or 16 = f16 (f16x3.h's three f16 products, the round-2..5
// arithmetic) in the aggregator's tile GEMMs, forward and input-gradient chain.  mix_where: which tile kernels run the mixed format when the cross
// terms are e4m3, bit 0 = inference forward, bit 1 = training forward, bit 2 = backward (the input-gradient chain).  Default 4: the forward keeps
// f16 cross terms -- with e4m3 ones its sigma / RGB are 1e-5 .. 6e-5 from the fp32 oracle instead of 1e-6 (inside the 1e-4 bar), but
// pre-activations within that distance of zero take the other LeakyReLU branch than the oracle's, and the gradient tests against the oracle see
// those flips (profiles/r06_cross_terms_ab.json)
#ifndef PN_MIX_DEFAULT_MASK
#define PN_MIX_DEFAULT_MASK 4
#endif
static PnArith &pn_arith_record() {
    static PnArith a = [] {
        const char *e = getenv("PNERF_MIX_MASK");          // (dev A/B)
        return PnArith{3, 1, 8, e ? atoi(e) & 7 : PN_MIX_DEFAULT_MASK};
    }();
    return a;
}
PnArith pn_arith() { return pn_arith_record(); }
// every setter: the previous value, or PNERF_E_INVAL (< 0) and nothing changed
static int pn_arith_set(int PnArith::*field, int v, bool valid) {
    if (!valid) return PNERF_E_INVAL;
    const int old = pn_arith_record().*field;
    pn_arith_record().*field = v;
    return old;
}
extern "C" int pnerf_set_inference_products(int n) { return pn_arith_set(&PnArith::products, n, n == 2 || n == 3); }
extern "C" int pnerf_set_wgrad_planes(int n) { return pn_arith_set(&PnArith::wgrad_planes, n, n == 1 || n == 2); }
extern "C" int pnerf_set_cross_terms(int bits) { return pn_arith_set(&PnArith::cross_terms, bits, bits == 8 || bits == 16); }
extern "C" int pnerf_set_cross_terms_where(int mask) { return pn_arith_set(&PnArith::mix_where, mask, mask >= 0 && mask <= 7); }
// the grid of the tile and colour kernels (tests: a handful of workgroups reaches every edge of the tile claim with a handful of tiles)
static int pn_tile_grid_cap = 0;
int pn_tile_grid(long long tiles, long long dflt) { return pn_capped_grid(tiles, pn_tile_grid_cap > 0 && pn_tile_grid_cap < dflt ? pn_tile_grid_cap : dflt); }
extern "C" int pnerf_debug_set_tile_grid(int max_workgroups) {
    if (max_workgroups < 0) return PNERF_E_INVAL;
    const int old = pn_tile_grid_cap;
    pn_tile_grid_cap = max_workgroups;
    return old;
}
extern "C" int pnerf_get_arithmetic(int32_t out[4]) {
    if (!out) return PNERF_E_INVAL;
    const PnArith a = pn_arith();
    out[0] = a.products; out[1] = a.wgrad_planes; out[2] = a.cross_terms; out[3] = a.mix_where;
    return 0;
}

// shared with render.hip
int pn_agg_forward_launch(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step &st, float *d_decoded, float *d_weight,
                          const PnSaved &sv, bool train, bool save_x0, hipStream_t s) {
    const int K = st.K;
    const long long cap_samples = st.n_valid_max;
    const PnArith ar = pn_arith();                     // one snapshot: every selection below reads it
    FwdArgs a;
    const bool wg2 = train && sv.wg2;                  // two-plane weight-gradient mode: residual planes, X0 saved whole
    if (wg2) save_x0 = true;
    a.save_x0 = save_x0 ? 1 : 0;
    a.cam = *cam;
    a.xyz = pts->xyz; a.emb = pts->embedding; a.conf = pts->conf; a.dir = pts->dir; a.color = pts->color;
    a.params = st.params; a.packed = (const float4 *)st.packed_mlp;
    a.raydir = st.raydir; a.sample_loc = st.sample_loc; a.xyz_pers = st.xyz_pers; a.loc_pers = st.loc_pers; a.pidx = st.sample_pidx; a.valid_list = st.valid_list; a.counters = st.counters;
    a.R = st.R; a.SR = st.SR; a.K = K; a.TS = pn_tile_samples(K);
    a.cap_samples = cap_samples;
    a.decoded = d_decoded; a.weight = d_weight; a.sv = sv;
    const bool frames = pts->frames != nullptr;
    if (frames && train) return PNERF_E_INVAL;            // per-point frames are render-only (include/pnerf.h: pnerf_points.frames)
    const int ncu = pn_cu_count();
    if (!ncu) return PNERF_E_LAUNCH;
    const int grid_c = pn_tile_grid((cap_samples + PN_CTILE - 1) / PN_CTILE, 2LL * ncu);       // two workgroups per CU
    const size_t lds_a = FL_BYTES, lds_c = CL_BYTES;
    const bool pers = st.xyz_pers != nullptr;
    const bool np2 = !train && ar.products == 2;      // inference with the weights' high plane only (f16x3.h: NP)
    const bool mix = !wg2 && !np2 && (ar.mix_mask() & (train ? 2 : 1));      // mixq.h: f16 h.h + e4m3 cross terms
    if (frames && (np2 || mix)) return PNERF_E_UNSUP;     // the FRAMES instances exist for the default inference arithmetic only
    // the one place that names the kernel instances: the selection serves both the LDS attribute and the launch
    using FwdKernel = void (*)(FwdArgs);
    using FwdKernelF = void (*)(FwdArgsF);            // per-point frames: their own argument and instances
    const FwdKernelF kfnf = pers ? k_agg_forward<false, true, 3, false, true> : k_agg_forward<false, false, 3, false, true>;
    const FwdKernelF cfnf = k_color_forward<false, 3, false, true>;
    const FwdKernel kfn = wg2   ? (pers ? k_agg_forward<true, true, 3, true> : k_agg_forward<true, false, 3, true>)
                        : mix   ? (train ? (pers ? k_agg_forward<true, true, 4> : k_agg_forward<true, false, 4>)
                                         : (pers ? k_agg_forward<false, true, 4> : k_agg_forward<false, false, 4>))
                        : train ? (pers ? k_agg_forward<true, true, 3> : k_agg_forward<true, false, 3>)
                        : np2   ? (pers ? k_agg_forward<false, true, 2> : k_agg_forward<false, false, 2>)
                                : (pers ? k_agg_forward<false, true, 3> : k_agg_forward<false, false, 3>);
    const FwdKernel cfn = wg2 ? k_color_forward<true, 3, true> : train ? k_color_forward<true, 3> : np2 ? k_color_forward<false, 2> : k_color_forward<false, 3>;
    if (hipFuncSetAttribute(frames ? reinterpret_cast<const void *>(kfnf) : reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a) != hipSuccess) return PNERF_E_LAUNCH;
    if (hipFuncSetAttribute(frames ? reinterpret_cast<const void *>(cfnf) : reinterpret_cast<const void *>(cfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c) != hipSuccess) return PNERF_E_LAUNCH;
    int rc = pn_classify(sv, st.valid_list, st.counters, st.sample_pidx, K, cap_samples, train, save_x0, s);
    if (rc) return rc;
    a.cls_list = sv.cls_list; a.cls_info = sv.cls_info; a.Kstride = K;
    int kc[PN_NCLS];
    const int ncls = pn_class_slots(K, kc);
    {
        PnProfScope prof(PNK_AGG_FWD, s);
        for (int j = 0; j < ncls; ++j) {            // class sizes are only known on the device: the grid covers the worst case, surplus workgroups return at once
            a.cls = j; a.K = kc[j]; a.TS = pn_tile_samples(kc[j]);
            const int grid_a = pn_tile_grid((cap_samples + a.TS - 1) / a.TS, 2LL * ncu);     // two workgroups per CU
            if (frames) { FwdArgsF af; static_cast<FwdArgs &>(af) = a; af.frames = pts->frames; hipLaunchKernelGGL(kfnf, dim3(grid_a), dim3(PN_NTHR), lds_a, s, af); }
            else hipLaunchKernelGGL(kfn, dim3(grid_a), dim3(PN_NTHR), lds_a, s, a);
        }
    }
    a.K = K; a.TS = pn_tile_samples(K); a.valid_list = sv.cls_list;      // the colour MLP walks the class-ordered list: f rows are in that order
    {
        PnProfScope prof(PNK_COLOR_FWD, s);
        if (frames) { FwdArgsF af; static_cast<FwdArgs &>(af) = a; af.frames = pts->frames; hipLaunchKernelGGL(cfnf, dim3(grid_c), dim3(256), lds_c, s, af); }
        else hipLaunchKernelGGL(cfn, dim3(grid_c), dim3(256), lds_c, s, a);
    }
    PN_CHECK_LAUNCH();
    return 0;
}

#ifdef PN_PHASE_TRACE
extern "C" int pnerf_debug_trace_fwd(void *host, size_t bytes) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(pn_trace_fwd), bytes < sizeof(pn_trace_fwd) ? bytes : sizeof(pn_trace_fwd)) == hipSuccess ? 0 : -1;
}
extern "C" int pnerf_debug_span_fwd(void *host, size_t bytes) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(pn_span_fwd), bytes < sizeof(pn_span_fwd) ? bytes : sizeof(pn_span_fwd)) == hipSuccess ? 0 : -1;
}
#endif
