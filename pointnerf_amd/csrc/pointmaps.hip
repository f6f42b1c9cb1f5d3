// pointmaps.hip -- point attribute maps, picking and image-to-point lifting of a render-only pass, on the renderer's DENSE per-ray results
// (DESIGN.md 4.8).  No reference counterpart: the reference never connects a pixel back to the points that produced it.
//
// One linear operator and its adjoint on blend_w [R,SR], weight [R,SR,K], sample_pidx [R,SR,K], ray_hit [R].  For ray r, slot s, neighbor k:
//   p = sample_pidx[r,s,k],   g[r,s,k] = blend_w[r,s] * weight[r,s,k] (ONE fp32 multiply) if 0 <= p < n_points, else 0.
// An index outside [0, n_points) -- the empty slot -1 included, which here does NOT read point 0 -- contributes nothing and is never
// dereferenced.  `weight` is the renderer's normalised distance weight (sum_k g = blend_w on a valid sample); the confidence factor of the
// density is deliberately NOT part of g.  A ray with ray_hit <= 0 produces zeros / -1 and none of its rows are read.
//
// k_ray_attributes (A and the pick):  attr_sum[r,c] = sum_{s,k} g attr[p,c];  top_flat = the LOWEST flat index s*K + k among the maxima of
// g[r,:,:] -- the largest single (sample, slot) entry, not a per-point sum over the ray's samples -- top_point = sample_pidx there,
// top_contrib = g there; -1 / -1 / 0 where the largest g is not > 0.  fp32 accumulation in an order that is a function of (SR, K, C) alone,
// no atomics: two calls give the same bits.
// k_lift_to_points (A^T):  point_sum[p,c] += g m[r] values[r,c],  point_mass[p] += g m[r]  over every entry that addresses p, with fp32
// atomicAdd on global memory (the kind of the backward's point gradients): the sums depend on arrival order and are NOT bit-reproducible.
//
// Shape: one 64-lane wavefront per ray, four rays per workgroup (k_probe_rays' shape), no LDS.  The pick strides the lanes over the ray's
// SR*K entries in chunks of 64 (coalesced weight / sample_pidx, blend_w per sample); the (value, flat index) pairs meet in one xor butterfly
// whose order -- larger value, then smaller index -- is total.  The sums come in two instances: C <= 4 is entry-parallel (each lane owns
// entries, keeps the column sums in registers, a point row is one 4..16-byte read per lane, butterfly sums at the end); the general C <= 256
// is column-parallel in passes of 64 columns (lane c owns a column, the K slots of a sample arrive by lane broadcast, a point row is one
// coalesced read).  A sample with blend_w == 0 (an empty slot, a sample a cut render left unshaded, a miss) is skipped before its rows are
// read.  The butterfly sum and the order of the pick are pn_ray.h's (pn_wave_sum, PnWaveArgmax); the pick carries the point index as a
// third word through its butterfly (re-reading sample_pidx at the winner instead measured 2-3 % slower: profiles/HISTORY.md).
#include "pn_ray.h"

namespace {
constexpr int PN_PM_TPB = 256;       // 4 rays per workgroup
constexpr int PN_PM_CMAX = 256;      // k_ray_attributes: columns of the attribute table
constexpr int PN_PM_LIFT_CMAX = 8;   // k_lift_to_points: columns of the per-ray values

struct PmIn {
    const float *blend_w, *weight;
    const int *pidx, *hit;
    int R, SR, K, n_points;
};
struct PmOut {
    float *attr_sum, *top_contrib;
    int *top_point, *top_flat;
};

// g of the flat entry e = s*K + k of the ray whose first sample is `row`, and its point index (-1 where the entry contributes nothing)
__device__ __forceinline__ float pm_entry(const PmIn &a, long long row, int e, int &p) {
    p = -1;
    const float bw = a.blend_w[row + e / a.K];
    if (bw == 0.f) return 0.f;                                           // weight / sample_pidx of an unshaded sample are not read
    const int q = a.pidx[row * a.K + e];
    if ((unsigned)q >= (unsigned)a.n_points) return 0.f;                 // the empty slot -1 and anything beyond the table
    p = q;
    return bw * a.weight[row * a.K + e];
}

// PnWaveArgmax on (g, flat index) with the entry's point as payload
struct PmPick {
    PnWaveArgmax b;
    int p = -1;
    __device__ __forceinline__ void take(float ov, int oe, int op) {
        if (b.loses_to(ov, oe)) { b.v = ov; b.i = oe; p = op; }
    }
    __device__ __forceinline__ void meet() {                             // every lane ends with the same triple: the order is total
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(b.v, off, 64);
            const int oe = __shfl_xor(b.i, off, 64), op = __shfl_xor(p, off, 64);
            take(ov, oe, op);
        }
    }
    __device__ __forceinline__ void store(const PmOut &o, long long r) const {
        const bool any = b.v > 0.f;                                      // a hit ray whose largest g is not > 0: -1, -1, 0
        o.top_point[r] = any ? p : -1;
        o.top_flat[r] = any ? b.i : -1;
        o.top_contrib[r] = any ? b.v : 0.f;
    }
};

__device__ __forceinline__ void pm_store_miss(const PmOut &o, long long r, int C, int lane) {
    for (int c = lane; c < C; c += 64) o.attr_sum[r * C + c] = 0.f;
    if (lane == 0) { o.top_point[r] = -1; o.top_flat[r] = -1; o.top_contrib[r] = 0.f; }
}

// C <= 4 (C == 0: the pick alone).  VEC: the table's rows are read as one float2 / float4 (the launcher checks the alignment).
template <int C, bool VEC>
__global__ __launch_bounds__(PN_PM_TPB) void k_ray_attributes(PmIn a, const float *__restrict__ attr, PmOut o) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (PN_PM_TPB / 64) + (threadIdx.x >> 6);
    if (r >= a.R) return;
    if (a.hit[r] <= 0) { pm_store_miss(o, r, C, lane); return; }         // (wave-uniform)
    const long long row = r * a.SR;
    const int n = a.SR * a.K;
    float acc[C > 0 ? C : 1] = {};
    PmPick best;
    for (int base = 0; base < n; base += 64) {
        const int e = base + lane;
        if (e >= n) continue;
        int p;
        const float g = pm_entry(a, row, e, p);
        best.take(g, e, p);
        if constexpr (C > 0) {
            if (g != 0.f) {
                const float *src = attr + (long long)p * C;
                float x[C];
                if constexpr (VEC && C == 4) { const float4 t = *reinterpret_cast<const float4 *>(src); x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w; }
                else if constexpr (VEC && C == 2) { const float2 t = *reinterpret_cast<const float2 *>(src); x[0] = t.x; x[1] = t.y; }
                else {
#pragma unroll
                    for (int c = 0; c < C; ++c) x[c] = src[c];
                }
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += g * x[c];
            }
        }
    }
    best.meet();
    if constexpr (C > 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = pn_wave_sum(acc[c]);
    }
    if (lane == 0) {
        best.store(o, r);
        if constexpr (C > 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) o.attr_sum[r * C + c] = acc[c];
        }
    }
}

// 4 < C <= 256: lane c owns columns c, c + 64, c + 128, c + 192; the samples with blend_w != 0 are walked in order, their K slots by broadcast
__global__ __launch_bounds__(PN_PM_TPB) void k_ray_attributes_wide(PmIn a, const float *__restrict__ attr, int C, PmOut o) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (PN_PM_TPB / 64) + (threadIdx.x >> 6);
    if (r >= a.R) return;
    if (a.hit[r] <= 0) { pm_store_miss(o, r, C, lane); return; }         // (wave-uniform)
    const long long row = r * a.SR;
    const int n = a.SR * a.K;
    PmPick best;
    for (int e = lane; e < n; e += 64) {
        int p;
        const float g = pm_entry(a, row, e, p);
        best.take(g, e, p);
    }
    best.meet();
    float acc[PN_PM_CMAX / 64] = {};
    for (int base = 0; base < a.SR; base += 64) {
        const float bwl = base + lane < a.SR ? a.blend_w[row + base + lane] : 0.f;
        unsigned long long todo = __ballot(bwl != 0.f);
        while (todo) {                                                   // (wave-uniform)  an unshaded sample costs nothing
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const float bw = __shfl(bwl, j, 64);
            const long long ent = (row + base + j) * a.K;
            float g = 0.f;
            int p = -1;
            if (lane < a.K) {
                const int q = a.pidx[ent + lane];
                if ((unsigned)q < (unsigned)a.n_points) { p = q; g = bw * a.weight[ent + lane]; }
            }
            for (int k = 0; k < a.K; ++k) {
                const float gk = __shfl(g, k, 64);
                const int pk = __shfl(p, k, 64);
                if (gk == 0.f) continue;                                 // (wave-uniform)
                const float *src = attr + (long long)pk * C + lane;
#pragma unroll
                for (int q = 0; q < PN_PM_CMAX / 64; ++q)
                    if (q * 64 + lane < C) acc[q] += gk * src[q * 64];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < PN_PM_CMAX / 64; ++q)
        if (q * 64 + lane < C) o.attr_sum[r * C + q * 64 + lane] = acc[q];
    if (lane == 0) best.store(o, r);
}

struct PmLift {
    const float *values, *factor;
    float *point_sum, *point_mass;
    int C;
};

__global__ __launch_bounds__(PN_PM_TPB) void k_lift_to_points(PmIn a, PmLift l) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (PN_PM_TPB / 64) + (threadIdx.x >> 6);
    if (r >= a.R || a.hit[r] <= 0) return;                               // (wave-uniform)  a miss adds nothing
    const float m = l.factor ? l.factor[r] : 1.f;
    if (m == 0.f) return;                                                // (wave-uniform)  a pixel outside the painted region
    float v[PN_PM_LIFT_CMAX];
#pragma unroll
    for (int c = 0; c < PN_PM_LIFT_CMAX; ++c) v[c] = c < l.C ? l.values[r * l.C + c] : 0.f;
    const long long row = r * a.SR;
    const int n = a.SR * a.K;
    for (int e = lane; e < n; e += 64) {
        int p;
        const float gm = pm_entry(a, row, e, p) * m;
        if (gm == 0.f) continue;
        atomicAdd(l.point_mass + p, gm);
        float *dst = l.point_sum + (long long)p * l.C;
#pragma unroll
        for (int c = 0; c < PN_PM_LIFT_CMAX; ++c)
            if (c < l.C) atomicAdd(dst + c, gm * v[c]);
    }
}

inline bool pm_aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
}  // namespace

extern "C" int pnerf_ray_attributes(const float *d_attr, int32_t n_points, int C, const float *d_blend_w, const float *d_weight,
                                    const int32_t *d_sample_pidx, const int32_t *d_ray_hit, int R, int SR, int K, float *d_attr_sum,
                                    int32_t *d_top_point, int32_t *d_top_flat, float *d_top_contrib, void *stream) {
    if (R < 0 || SR <= 0 || K < 1 || K > PNERF_MAX_K || n_points <= 0 || C < 0) return PNERF_E_INVAL;
    if (C > PN_PM_CMAX || (long long)SR * K > 0x7fffffffLL) return PNERF_E_UNSUP;
    if (R == 0) return 0;
    if (!d_blend_w || !d_weight || !d_sample_pidx || !d_ray_hit || !d_top_point || !d_top_flat || !d_top_contrib) return PNERF_E_INVAL;
    if (C > 0 && (!d_attr || !d_attr_sum)) return PNERF_E_INVAL;
    const PmIn a = {d_blend_w, d_weight, d_sample_pidx, d_ray_hit, R, SR, K, n_points};
    const PmOut o = {d_attr_sum, d_top_contrib, d_top_point, d_top_flat};
    const dim3 grid(pn_cdiv(R, PN_PM_TPB / 64)), block(PN_PM_TPB);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 0: hipLaunchKernelGGL((k_ray_attributes<0, false>), grid, block, 0, s, a, d_attr, o); break;
    case 1: hipLaunchKernelGGL((k_ray_attributes<1, false>), grid, block, 0, s, a, d_attr, o); break;
    case 2:
        if (pm_aligned(d_attr, 8)) hipLaunchKernelGGL((k_ray_attributes<2, true>), grid, block, 0, s, a, d_attr, o);
        else hipLaunchKernelGGL((k_ray_attributes<2, false>), grid, block, 0, s, a, d_attr, o);
        break;
    case 3: hipLaunchKernelGGL((k_ray_attributes<3, false>), grid, block, 0, s, a, d_attr, o); break;
    case 4:
        if (pm_aligned(d_attr, 16)) hipLaunchKernelGGL((k_ray_attributes<4, true>), grid, block, 0, s, a, d_attr, o);
        else hipLaunchKernelGGL((k_ray_attributes<4, false>), grid, block, 0, s, a, d_attr, o);
        break;
    default: hipLaunchKernelGGL(k_ray_attributes_wide, grid, block, 0, s, a, d_attr, C, o); break;
    }
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_lift_to_points(const float *d_values, int C, const float *d_ray_factor, const float *d_blend_w, const float *d_weight,
                                    const int32_t *d_sample_pidx, const int32_t *d_ray_hit, int R, int SR, int K, int32_t n_points,
                                    float *d_point_sum, float *d_point_mass, void *stream) {
    if (R < 0 || SR <= 0 || K < 1 || K > PNERF_MAX_K || n_points <= 0 || C < 0) return PNERF_E_INVAL;
    if (C > PN_PM_LIFT_CMAX || (long long)SR * K > 0x7fffffffLL) return PNERF_E_UNSUP;
    if (R == 0) return 0;
    if (!d_blend_w || !d_weight || !d_sample_pidx || !d_ray_hit || !d_point_mass) return PNERF_E_INVAL;
    if (C > 0 && (!d_values || !d_point_sum)) return PNERF_E_INVAL;
    const PmIn a = {d_blend_w, d_weight, d_sample_pidx, d_ray_hit, R, SR, K, n_points};
    const PmLift l = {d_values, d_ray_factor, d_point_sum, d_point_mass, C};
    hipLaunchKernelGGL(k_lift_to_points, dim3(pn_cdiv(R, PN_PM_TPB / 64)), dim3(PN_PM_TPB), 0, (hipStream_t)stream, a, l);
    PN_CHECK_LAUNCH();
    return 0;
}
