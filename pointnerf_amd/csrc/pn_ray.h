// pn_ray.h -- the vocabulary of the wave-per-ray kernels (render.hip, raygeom.hip, pointmaps.hip, probe.hip): one 64-lane wavefront per ray,
// the lanes striding over the ray's SR slots in chunks of 64.  THE definition of the wave scans, of the reference's ray-dist rule and of the
// transmittance step: the cut render's promise that an uncut ray matches pnerf_render_forward bit for bit, and the "two calls give the same
// bits" of the per-ray maps, rest on every kernel taking them from here.  The operation order of each helper is part of that contract.
#pragma once
#include "pn_common.h"

// xor butterfly, offsets 32 -> 1: every lane ends with the sum of the 64 lanes, in an order that depends on nothing but the lane number
__device__ __forceinline__ float pn_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int pn_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// inclusive scans over the lanes (lane l ends with the combination of lanes 0 .. l)
__device__ __forceinline__ float pn_wave_incl_max(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { float y = __shfl_up(v, off, 64); if (lane >= off) v = fmaxf(v, y); }
    return v;
}
template <class F> __device__ __forceinline__ F pn_wave_incl_prod(F v, int lane) {                   // F = float, or double (the ray-march backward)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { F y = __shfl_up(v, off, 64); if (lane >= off) v *= y; }
    return v;
}
__device__ __forceinline__ float pn_wave_incl_sum(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { float y = __shfl_up(v, off, 64); if (lane >= off) v += y; }
    return v;
}
// back to front, over the maps x -> a x + b: lane l ends with f_l o f_(l+1) o ... o f_63, the map that carries a value from behind lane 63
// to in front of lane l (a = 1, b = 0 is the neutral element)
__device__ __forceinline__ void pn_wave_rincl_affine(double &a, double &b, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double oa = __shfl_down(a, off, 64), ob = __shfl_down(b, off, 64);
        if (lane + off < 64) { b = a * ob + b; a *= oa; }
    }
}

// perspective depth of a world position: ((p - campos) @ camrot)[2]   (point_query.py:101-108)
__device__ __forceinline__ float pn_pers_z(const pnerf_camera &c, const float *p) {
    return (p[0] - c.campos[0]) * c.camrot[2] + (p[1] - c.campos[1]) * c.camrot[5] + (p[2] - c.campos[2]) * c.camrot[8];
}

// The ray_dist block of NeuralPointsRayMarching.forward (models/neural_points_volumetric_model.py:271-279) for one 64-slot chunk of a ray:
// lane `lane` holds slot s of the ray whose SR slots start at element `row` of sample_loc [.,3] / nn.  Slots at or beyond s_end (<= SR)
// carry neutral elements and are not read (s_end = SR: the whole ray; the cut render advances through one stage's slots).  `cm_prev` is the
// running cummax of the perspective depth in front of the chunk and is advanced; delta = the slot's ray_dist, 0 on an empty slot.
__device__ __forceinline__ void pn_chunk_raydist(const pnerf_camera &cam, const float *sample_loc, const int *nn, long long row, int s, int s_end, int SR, int lane,
                                                 float &cm_prev, float &delta, bool &valid) {
    const bool in = s < s_end;
    float z = -INFINITY, znext = -INFINITY;
    if (in) z = pn_pers_z(cam, sample_loc + (row + s) * 3);
    const int next_end = s_end < SR ? s_end + 1 : SR;                // s + 1 < next_end  <=>  in && s + 1 < SR   (s_end <= SR)
    if (s + 1 < next_end) znext = pn_pers_z(cam, sample_loc + (row + s + 1) * 3);
    const float cm = fmaxf(pn_wave_incl_max(z, lane), cm_prev);      // torch.cummax(sample_loc[...,2])  :271
    const float vs = cam.vsize_z;
    float d = (s + 1 < SR) ? fmaxf(cm, znext) - cm : vs;             // cm[s+1] - cm[s]; last = vsize[2]   :272
    bool m = d < 1e-8f;
    if (cam.raydist_mode_unit > 0) m = m || (d > 2.f * vs);          // :274-276
    if (m) d = vs;                                                   // :278
    valid = in && nn[row + s] > 0;                                   // ray_valid = any_K(mask)  point_aggregators.py:741
    delta = valid ? d : 0.f;                                         // :279
    cm_prev = __shfl(cm, 63, 64);
}

// ray_march's transmittance (models/rendering/diff_ray_marching.py:533-539) across the chunks of a ray: u = 1 - op + 1e-10 per slot (1 on a
// lane outside the ray), T in front of a slot = the product of u over the slots in front of it.  F = float: the forward's T, bit for bit, in
// every kernel that thresholds or stores it; F = double: the same fp32 factors u multiplied without a rounding of their own (the backward).
template <class F> struct PnTransmittanceT {
    F T_carry = 1;                   // the product over the chunks in front; after the last chunk: the ray's background transmittance
    static __device__ __forceinline__ float u_of(float op, bool in) { return in ? (1.f - op + 1e-10f) : 1.f; }       // :533
    // one chunk: Tx = the transmittance IN FRONT of the lane's slot (exclusive product by lane shift), returns the one BEHIND it (inclusive)
    __device__ __forceinline__ F step(float op, bool in, int lane, F &Tx) {
        const F incl = pn_wave_incl_prod((F)u_of(op, in), lane);
        Tx = __shfl_up(incl, 1, 64);
        if (lane == 0) Tx = 1;
        Tx *= T_carry;
        const F Tin = incl * T_carry;
        T_carry *= __shfl(incl, 63, 64);
        return Tin;
    }
};
using PnTransmittance = PnTransmittanceT<float>;

// (largest value, lowest index) over a wave.  The order -- larger value first, then the smaller index -- is total, so after meet() every lane
// holds the same pair whatever the tree; a NaN compares false everywhere and is never taken.
struct PnWaveArgmax {
    float v = -INFINITY;
    int i = 0x7fffffff;
    __device__ __forceinline__ bool loses_to(float ov, int oi) const { return ov > v || (ov == v && oi < i); }       // THE order
    __device__ __forceinline__ void take(float ov, int oi) {
        if (loses_to(ov, oi)) { v = ov; i = oi; }
    }
    __device__ __forceinline__ void meet() {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(v, off, 64);
            const int oi = __shfl_xor(i, off, 64);
            take(ov, oi);
        }
    }
};
