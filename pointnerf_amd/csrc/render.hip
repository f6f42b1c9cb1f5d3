// render.hip -- ray-dist + alpha-composite volume renderer (forward and backward), the cut render, and the C-ABI entry points of the
// fused render path.
//
// Replaces the ray_dist block of NeuralPointsRayMarching.forward
// (models/neural_points_volumetric_model.py:271-279) and ray_march
// (models/rendering/diff_ray_marching.py:508-554; radiance_render / alpha_blend / no_tone_map,
// models/rendering/diff_render_func.py:36-62).  One 64-lane wavefront per ray: the cummax over the
// perspective depth and the exclusive transmittance product are wave scans (pn_ray.h), no intermediate
// [R,SR] tensors of the reference (sigma, opacity, cumprod, blend weight, ...) are materialised except
// the ones the caller asks for.
#include "mlp_common.h"
#include "pn_ray.h"

namespace {
constexpr int TPB = 256;

struct RmArgs {
    pnerf_camera cam;
    const float *sample_loc, *decoded;
    const int *nn;
    const float *ray_dist;            // stand-alone ray_march(): distances and validity supplied by the caller
    const unsigned char *valid8;
    int R, SR;
};
// the GEOM instance of k_raymarch_backward: per-ray gradients of depth_sum, acc and the background transmittance, and the
// slots' depths when the caller supplies them (the stand-alone form; NULL: pn_pers_z of the sample positions)
struct RmGeomArgs : RmArgs {
    const float *grad_geom;           // [R,3] = (g_ds, g_acc, g_T)
    const float *z;                   // [R,SR] or NULL
};
template <bool GEOM> struct RmArgsOf { using T = RmArgs; };
template <> struct RmArgsOf<true> { using T = RmGeomArgs; };

// Per-sample quantities of one 64-sample chunk of a ray.  `cm_prev` is the running cummax before the
// chunk.  Returns delta (ray_dist), valid flag, and updates cm_prev.
__device__ __forceinline__ void chunk_raydist(const RmArgs &a, int r, int s, int lane, float &cm_prev, float &delta, bool &valid) {
    const int SR = a.SR;
    const long long row = (long long)r * SR;
    if (a.ray_dist) {
        valid = s < SR && a.valid8[row + s] != 0;
        delta = s < SR ? a.ray_dist[row + s] : 0.f;
        return;
    }
    pn_chunk_raydist(a.cam, a.sample_loc, a.nn, row, s, SR, SR, lane, cm_prev, delta, valid);
}

__global__ __launch_bounds__(TPB) void k_raymarch_forward(RmArgs a, float *__restrict__ ray_color, float *__restrict__ opacity_out,
                                                          float *__restrict__ bg_trans, float *__restrict__ blend_w,
                                                          float *__restrict__ acc_trans) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int SR = a.SR;
    float cm_prev = -INFINITY;
    PnTransmittance tr;
    float cr = 0.f, cg = 0.f, cb = 0.f;
    for (int base = 0; base < SR; base += 64) {
        const int s = base + lane;
        float delta; bool valid;
        chunk_raydist(a, r, s, lane, cm_prev, delta, valid);
        float sigma = 0.f, rr = 0.f, gg = 0.f, bb = 0.f;
        if (s < SR) {
            const float4 f = *reinterpret_cast<const float4 *>(a.decoded + ((long long)r * SR + s) * 4);
            sigma = valid ? f.x : 0.f; rr = f.y; gg = f.z; bb = f.w;
        }
        const float op = 1.f - expf(-sigma * delta);                    // diff_ray_marching.py:530
        float Tx;
        tr.step(op, s < SR, lane, Tx);
        const float bw = op * Tx;                                       // alpha_blend
        if (s < SR) {
            opacity_out[(long long)r * SR + s] = op;
            blend_w[(long long)r * SR + s] = bw;
            if (acc_trans) acc_trans[(long long)r * SR + s] = Tx;
        }
        cr += bw * rr; cg += bw * gg; cb += bw * bb;
    }
    const float T_end = tr.T_carry;
    cr = pn_wave_sum(cr); cg = pn_wave_sum(cg); cb = pn_wave_sum(cb);
    if (lane == 0) {
        if (a.cam.has_bg) { cr += a.cam.bg[0] * T_end; cg += a.cam.bg[1] * T_end; cb += a.cam.bg[2] * T_end; }   // :543-545
        ray_color[3 * r] = cr; ray_color[3 * r + 1] = cg; ray_color[3 * r + 2] = cb;
        bg_trans[r] = T_end;
    }
}

// Backward: dL/d(ray_color) -> dL/d(decoded) = (d sigma, d r, d g, d b) per sample.
//   color = sum_s bw_s rgb_s + bg T_end ;  bw_s = op_s T_s ; T_s = prod_{j<s} u_j ; u = 1 - op + eps ; op = 1 - exp(-sigma delta)
//   d color / d op_s = T_s rgb_s - (sum_{j>s} bw_j rgb_j + T_end bg) / u_s
// With c_j = g . rgb_j and T_(s+1) = T_s u_s the bracket is T_(s+1) S_s, where S_s is what the ray shows BEHIND slot s, seen from there:
//   S_(SR-1) = g . bg ;  S_(j-1) = op_j c_j + u_j S_j        so        d (g . color) / d op_s = T_s (c_s - S_s).
// S is built back to front from the slots behind s alone, by a scan over the maps S -> u_j S + op_j c_j (pn_wave_rincl_affine).  The bracket
// is never formed as (total - prefix) and nothing is divided by u_s: behind an opaque slot the true bracket is tiny against the ray's total,
// the difference would keep the rounding residue of the whole ray, and 1 / u_s ~ 1e6 .. 1e10 would blow it up to the size of the ray's own
// d sigma.  Nor are T_s c_s and the bracket rounded apart before they cancel: the rounding of T_s multiplies the whole difference.
// Pass 1 leaves the map of chunk i in lane i (one lane per 64-slot chunk: SR <= RM_BWD_MAX_SR) and applies those back to front to g . bg, which
// gives S behind every chunk; pass 2 runs the transmittance front to back and S back to front within the chunk.
// delta, op = 1 - expf(-sigma delta) and u are the forward's own fp32 values (chunk_raydist, PnTransmittance::u_of): the gradient is the one of
// the function the forward evaluates.  What is BUILT from them -- c, the maps, S, T -- is carried in double and rounded once per output, so the
// order of the wave scans (a tree per lane, whose roundings neighbouring lanes do not share) costs nothing: measured per ray against float64,
// d sigma and d rgb are as close as the fp32 autograd of the same formula or closer where the device's expf is not what limits them
// (tests/raymarch_case.py; figures in DESIGN.md 4.9).
// GEOM: the ray's depth_sum = sum_s bw_s z_s, acc = sum_s bw_s and background transmittance T_end are further channels of
// the same recurrence -- with their per-ray gradients (g_ds, g_acc, g_T),  c_s += g_ds z_s + g_acc  and  S_bg += g_T  -- one fused
// multiply-add per slot and one per ray, in double like c and S themselves; d rgb has no new term.  z_s is the perspective depth of the
// sample (or the caller's array), 0 on a slot that is not valid: an empty slot's position is not read, and its op is 0.  With all three
// gradients zero the additions are exact and the outputs are the GEOM = false instance's.
constexpr int RM_BWD_MAX_SR = 64 * 64;
template <bool GEOM> __device__ __forceinline__ double geom_channel(const typename RmArgsOf<GEOM>::T &a, long long slot, bool valid, double c, double g_ds, double g_acc) {
    if constexpr (GEOM) {
        const float z = !valid ? 0.f : (a.z ? a.z[slot] : pn_pers_z(a.cam, a.sample_loc + slot * 3));
        return c + (g_ds * (double)z + g_acc);
    } else {
        return c;
    }
}
template <bool GEOM>
__global__ __launch_bounds__(TPB) void k_raymarch_backward(typename RmArgsOf<GEOM>::T a, const float *__restrict__ grad_color, float *__restrict__ grad_decoded) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int SR = a.SR;
    const float g0 = grad_color[3 * r], g1 = grad_color[3 * r + 1], g2 = grad_color[3 * r + 2];
    double g_ds = 0., g_acc = 0., g_T = 0.;
    if constexpr (GEOM) { g_ds = a.grad_geom[3 * r]; g_acc = a.grad_geom[3 * r + 1]; g_T = a.grad_geom[3 * r + 2]; }
    // pass 1: in lane i the map of chunk i >= 1, S behind the chunk -> S in front of it (nothing lies in front of chunk 0: its map is not needed)
    float cm_prev = -INFINITY;
    double ca = 1., cb = 0.;
    for (int base = 0; base < SR; base += 64) {
        const int s = base + lane;
        float delta; bool valid;
        chunk_raydist(a, r, s, lane, cm_prev, delta, valid);              // chunk 0 too: it carries the depth cummax through the ray
        if (base == 0) continue;
        float sigma = 0.f;
        double c = 0.;
        if (s < SR) {
            const float4 f = *reinterpret_cast<const float4 *>(a.decoded + ((long long)r * SR + s) * 4);
            sigma = valid ? f.x : 0.f; c = (double)g0 * f.y + (double)g1 * f.z + (double)g2 * f.w;
            c = geom_channel<GEOM>(a, (long long)r * SR + s, valid, c, g_ds, g_acc);
        }
        const float op = 1.f - expf(-sigma * delta);
        double ma = PnTransmittance::u_of(op, s < SR), mb = op * c;       // a lane outside the ray: u = 1, op c = 0
        pn_wave_rincl_affine(ma, mb, lane);
        ma = __shfl(ma, 0, 64); mb = __shfl(mb, 0, 64);
        if (lane == (base >> 6)) { ca = ma; cb = mb; }
    }
    // lane i: S BEHIND chunk i -- the background behind the last chunk, then chunk by chunk towards the front
    double S_bg = a.cam.has_bg ? (double)g0 * a.cam.bg[0] + (double)g1 * a.cam.bg[1] + (double)g2 * a.cam.bg[2] : 0.;
    if constexpr (GEOM) S_bg += g_T;                                      // T_end multiplies the background colour: its gradient joins g . bg
    double behind = S_bg, S_front = S_bg;
    for (int i = (SR - 1) >> 6; i >= 1; --i) {
        S_front = __shfl(ca, i, 64) * S_front + __shfl(cb, i, 64);        // in front of chunk i = behind chunk i - 1
        if (lane == i - 1) behind = S_front;
    }
    // pass 2: per-sample gradients
    cm_prev = -INFINITY;
    PnTransmittanceT<double> tr;
    for (int base = 0; base < SR; base += 64) {
        const int s = base + lane;
        float delta; bool valid;
        chunk_raydist(a, r, s, lane, cm_prev, delta, valid);
        float sigma = 0.f;
        double c = 0.;
        if (s < SR) {
            const float4 f = *reinterpret_cast<const float4 *>(a.decoded + ((long long)r * SR + s) * 4);
            sigma = valid ? f.x : 0.f; c = (double)g0 * f.y + (double)g1 * f.z + (double)g2 * f.w;
            c = geom_channel<GEOM>(a, (long long)r * SR + s, valid, c, g_ds, g_acc);
        }
        const float e = expf(-sigma * delta);
        const float op = 1.f - e;
        const float u = PnTransmittance::u_of(op, s < SR);
        double Tx;
        tr.step(op, s < SR, lane, Tx);
        double ma = u, mb = op * c;
        pn_wave_rincl_affine(ma, mb, lane);
        const double S_end = __shfl(behind, base >> 6, 64);               // S behind the chunk
        double S = __shfl_down(ma * S_end + mb, 1, 64);                   // S behind slot s = in front of slot s + 1
        if (lane == 63) S = S_end;
        const float dop = (float)(Tx * (c - S));
        if (s < SR) {
            const double bw = op * Tx;
            float4 o;
            o.x = valid ? dop * delta * e : 0.f;                          // d op / d sigma = delta exp(-sigma delta)
            o.y = (float)(bw * g0); o.z = (float)(bw * g1); o.w = (float)(bw * g2);
            *reinterpret_cast<float4 *>(grad_decoded + ((long long)r * SR + s) * 4) = o;
        }
    }
}

// ---- early ray termination of a render-only pass ("cut render", include/pnerf.h: pnerf_render_forward_cut) -------------------------
// The reference has no counterpart for the cut itself; what is thresholded is ray_march's transmittance (models/rendering/
// diff_ray_marching.py:508-554) as k_raymarch_forward forms it: the ray-dist deltas of pn_chunk_raydist and the transmittance step of
// PnTransmittance (pn_ray.h), the very code the ray march runs, so an uncut ray matches pnerf_render_forward bit for bit.  A ray is
// shaded front to back in stages of B slots; the step of stage j advances the ray's transmittance through the slots of stage j - 1 (their
// sigma is in `decoded` by then; unshaded samples hold 0), drops the ray once T < cutoff, and
// flags the slots of stage j with a neighbor of the rays still alive.  One wavefront per ray.  Per-ray state between stages: the running
// T, the running cummax of the perspective depth in front of the next slot to advance through (the ray-dist delta needs it), and
//   alive: 1 = still shaded, 0 = a miss or ended with nothing left to shade, 2 = ended with at least one valid sample unshaded
// so a stage reads only its own B slots of sample_loc / decoded (a ray that ends reads the rest of its neighbor counts once).
struct CutArgs {
    pnerf_camera cam;
    const float *sample_loc, *decoded;
    const int *nn, *hit;
    int R, SR, B, stage;
    float cutoff;
};
__global__ __launch_bounds__(TPB) void k_cut_stage(CutArgs a, float *__restrict__ T_st, float *__restrict__ cm_st, int *__restrict__ alive_st,
                                                   int *__restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int SR = a.SR;
    const long long row = (long long)r * SR;
    int alive;
    PnTransmittance tr;
    float cm_prev = -INFINITY;
    if (a.stage == 0) alive = (!a.hit || a.hit[r] > 0) ? 1 : 0;      // (no hit flags: a ray without a valid sample flags nothing and keeps T = 1)
    else {
        alive = alive_st[r]; tr.T_carry = T_st[r]; cm_prev = cm_st[r];
        if (alive == 1) {
            const int s0 = (a.stage - 1) * a.B, s1 = s0 + a.B;             // the previous stage's slots (s1 < SR: this stage exists)
            for (int base = s0; base < s1; base += 64) {                   // B need not divide 64: lanes beyond s1 carry neutral elements
                const int s = base + lane;
                float delta, Tx; bool valid;
                pn_chunk_raydist(a.cam, a.sample_loc, a.nn, row, s, s1, SR, lane, cm_prev, delta, valid);
                const float sigma = valid ? a.decoded[(row + s) * 4] : 0.f;
                tr.step(1.f - expf(-sigma * delta), s < s1, lane, Tx);
            }
            if (!(tr.T_carry >= a.cutoff)) {                               // the ray ends here: does that leave a valid sample unshaded?
                int left = 0;
                for (int base = s1; base < SR; base += 64) {
                    const int s = base + lane;
                    if (s < SR && a.nn[row + s] > 0) left = 1;
                }
                alive = __ballot(left) != 0ull ? 2 : 0;
            }
        }
    }
    if (lane == 0) { T_st[r] = tr.T_carry; cm_st[r] = cm_prev; alive_st[r] = alive; }
    const int f0 = a.stage * a.B, f1 = f0 + a.B;
    for (int base = 0; base < SR; base += 64) {                            // the whole row: the compaction reads every flag
        const int s = base + lane;
        if (s < SR) flags[row + s] = (alive == 1 && s >= f0 && s < f1 && a.nn[row + s] > 0) ? 1 : 0;
    }
}
// totals of a cut render, without atomics: out[0] = samples shaded (the stages' list lengths added), out[1] = rays that ended with a
// valid sample unshaded (alive == 2), out[2] = out[3] = 0.  One workgroup.
__global__ __launch_bounds__(1024) void k_cut_totals(const int *__restrict__ stage_counters, int n_stages, const int *__restrict__ alive_st, int R,
                                                     int *__restrict__ out) {
    __shared__ int red[16];
    int n = 0;
    for (int r = threadIdx.x; r < R; r += 1024) n += alive_st[r] == 2 ? 1 : 0;
    n = pn_wave_sum(n);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int cut = 0, shaded = 0;
        for (int w = 0; w < 16; ++w) cut += red[w];
        for (int j = 0; j < n_stages; ++j) shaded += stage_counters[8 * j];
        out[0] = shaded; out[1] = cut; out[2] = 0; out[3] = 0;
    }
}
}  // namespace

// the argument of the two ray-march kernels, in its two forms: ray distances and validity from the camera, the samples' positions and their
// neighbor counts (the fused path), or supplied by the caller with the background colour (the stand-alone ray_march())
static RmArgs rm_args(const pnerf_camera &cam, const float *sample_loc, const int32_t *nn, const float *decoded, int R, int SR) {
    RmArgs ra = {};
    ra.cam = cam; ra.sample_loc = sample_loc; ra.nn = nn; ra.decoded = decoded; ra.R = R; ra.SR = SR;
    return ra;
}
static RmArgs rm_args(const float *ray_dist, const uint8_t *valid8, const float *bg3_host, const float *decoded, int R, int SR) {
    RmArgs ra = {};
    ra.ray_dist = ray_dist; ra.valid8 = valid8; ra.decoded = decoded; ra.R = R; ra.SR = SR;
    ra.cam.has_bg = bg3_host ? 1 : 0;
    if (bg3_host) { ra.cam.bg[0] = bg3_host[0]; ra.cam.bg[1] = bg3_host[1]; ra.cam.bg[2] = bg3_host[2]; }
    return ra;
}

// the inference workspace: [fs | class partition | room for the weight-gradient partials]; training: the caller passes a pnerf_agg_saved_bytes()
// area instead.  Like pn_saved_walk: counts without a base, hands out sv.fs and the class arrays with one.
static size_t agg_workspace_walk(void *base, long long n_valid_max, int K, PnSaved &sv) {
    PnSaved dims;
    pn_saved_walk(nullptr, n_valid_max, K, dims);
    sv = PnSaved();
    sv.rows = dims.rows; sv.samples = dims.samples;      // the row and sample counts of that capacity; everything else null / 0
    PnCarver cv(base);
    sv.fs = cv.take<float>((size_t)sv.samples * PN_H);
    pn_cls_walk(cv, sv);
    return cv.off + pn_wgrad_partials_bytes();
}
extern "C" size_t pnerf_agg_workspace_bytes(int64_t n_valid_max, int K) {
    if (K <= 0 || K > PNERF_MAX_K || n_valid_max < 0) return 0;
    PnSaved sv;
    return agg_workspace_walk(nullptr, n_valid_max, K, sv);
}

// THE validation of the four render entry points, in the order that decides between two codes.  ST_RENDER: the render pair, which reads
// st->sample_nn and projects from cam (it refuses st->xyz_pers / st->loc_pers; the pnerf_agg_* pair takes both or neither); ST_SAVING: a training
// forward or a backward (per-point frames are render-only: include/pnerf.h, pnerf_points.frames); call_ptrs: the results or gradients of this
// call are all there
enum : unsigned { ST_RENDER = 1, ST_SAVING = 2 };
static int check_step(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *st, unsigned kind, bool call_ptrs) {
    const bool render = kind & ST_RENDER;
    if (!cam || !pts || !st || st->R < 0 || st->SR <= 0 || st->K <= 0 || st->K > PNERF_MAX_K) return PNERF_E_INVAL;
    if (pts->feat_dim != PN_F) return PNERF_E_UNSUP;
    if (!pts->xyz || !pts->embedding || !pts->conf || !pts->dir || !pts->color) return PNERF_E_UNSUP;
    if (!st->packed_mlp || !st->params || !st->raydir || !st->sample_loc || !st->sample_pidx || (render && !st->sample_nn) || !st->valid_list || !st->counters) return PNERF_E_INVAL;
    if (!call_ptrs) return PNERF_E_INVAL;
    if (render ? (st->xyz_pers || st->loc_pers) : (st->xyz_pers == nullptr) != (st->loc_pers == nullptr)) return PNERF_E_INVAL;
    if (pts->frames && (kind & ST_SAVING)) return PNERF_E_INVAL;
    return 0;
}

// where a forward works, after check_step: the saved area (training) or the inference workspace
static int agg_scratch(const pnerf_step &st, void *d_saved, void *d_ws, size_t ws_bytes, PnSaved &sv) {
    if (d_saved) sv = pn_saved_carve(d_saved, st.n_valid_max, st.K);
    else if (!d_ws || ws_bytes < pnerf_agg_workspace_bytes(st.n_valid_max, st.K)) return PNERF_E_WS;
    else agg_workspace_walk(d_ws, st.n_valid_max, st.K, sv);
    return 0;
}
// decoded / weight are zero wherever no sample is shaded
static int zero_outputs(const pnerf_step &st, float *d_decoded, float *d_weight, hipStream_t s) {
    if (hipMemsetAsync(d_decoded, 0, (size_t)st.R * st.SR * 4 * sizeof(float), s) != hipSuccess) return PNERF_E_LAUNCH;
    if (hipMemsetAsync(d_weight, 0, (size_t)st.R * st.SR * st.K * sizeof(float), s) != hipSuccess) return PNERF_E_LAUNCH;
    return 0;
}
// the aggregator + colour MLP of both forwards, after check_step: works in the saved area (training) or in the inference workspace
static int agg_forward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step &st, float *d_decoded, float *d_weight,
                       void *d_saved, void *d_ws, size_t ws_bytes, bool save_x0, hipStream_t s) {
    if (st.R == 0) return 0;
    PnSaved sv;
    int rc = agg_scratch(st, d_saved, d_ws, ws_bytes, sv);
    if (rc || (rc = zero_outputs(st, d_decoded, d_weight, s)) != 0) return rc;
    if (st.n_valid_max == 0) return 0;
    return pn_agg_forward_launch(cam, pts, st, d_decoded, d_weight, sv, d_saved != nullptr, save_x0, s);
}

static int raymarch_launch(const pnerf_camera *cam, const pnerf_step *st, const float *d_decoded, float *d_ray_color, float *d_opacity, float *d_bg_trans,
                           float *d_blend_w, hipStream_t s) {
    { PnProfScope prof(PNK_RAYMARCH_FWD, s);
    hipLaunchKernelGGL(k_raymarch_forward, dim3(pn_cdiv(st->R, TPB / 64)), dim3(TPB), 0, s, rm_args(*cam, st->sample_loc, st->sample_nn, d_decoded, st->R, st->SR),
                       d_ray_color, d_opacity, d_bg_trans, d_blend_w, (float *)nullptr); }
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_render_forward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *st,
                                    float *d_decoded, float *d_weight, float *d_ray_color, float *d_opacity,
                                    float *d_bg_trans, float *d_blend_w,
                                    void *d_saved, void *d_ws, size_t ws_bytes, void *stream) {
    int rc = check_step(cam, pts, st, ST_RENDER | (d_saved ? ST_SAVING : 0), d_decoded && d_weight && d_ray_color && d_opacity && d_bg_trans && d_blend_w);
    if (rc || st->R == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = agg_forward(cam, pts, *st, d_decoded, d_weight, d_saved, d_ws, ws_bytes, /*save_x0=*/false, s)) != 0) return rc;
    return raymarch_launch(cam, st, d_decoded, d_ray_color, d_opacity, d_bg_trans, d_blend_w, s);
}

// ---- the cut render (include/pnerf.h) ---------------------------------------------------------------------------------------------
namespace {
// the cut workspace: per-ray state, the stage's flags and work list, 8 counter words per stage (at most SR stages), scan scratch
struct CutWs { float *T, *cm; int *alive, *flags, *list, *counters, *scan; };
size_t cut_ws_walk(void *base, int R, int SR, CutWs &w) {
    const size_t n = (size_t)(R > 0 ? R : 0) * SR;
    PnCarver cv(base);
    w.T = cv.take<float>(R); w.cm = cv.take<float>(R); w.alive = cv.take<int>(R);
    w.flags = cv.take<int>(n); w.list = cv.take<int>(n > 0 ? n : 1); w.counters = cv.take<int>((size_t)8 * SR);
    w.scan = cv.take<int>(pn_scan_scratch_ints((long long)n));
    return cv.off;
}
// the step of stage `stage` and the compaction of its flags: list = ascending r * SR + s, counters[0] = its length (counters[1..7] = 0)
int cut_stage_launch(const pnerf_camera &cam, const float *sample_loc, const int *nn, const int *hit, const float *decoded, int R, int SR, float cutoff,
                     int B, int stage, float *T, float *cm, int *alive, int *flags, int *list, int *counters, int *scan, hipStream_t s) {
    CutArgs a;
    a.cam = cam; a.sample_loc = sample_loc; a.decoded = decoded; a.nn = nn; a.hit = hit; a.R = R; a.SR = SR; a.B = B; a.stage = stage; a.cutoff = cutoff;
    if (hipMemsetAsync(counters, 0, 8 * sizeof(int), s) != hipSuccess) return PNERF_E_LAUNCH;
    PnProfScope prof(PNK_COMPACT, s);
    hipLaunchKernelGGL(k_cut_stage, dim3(pn_cdiv(R, TPB / 64)), dim3(TPB), 0, s, a, T, cm, alive, flags);
    PN_CHECK_LAUNCH();
    return pn_compact_gt0_i32(flags, (long long)R * SR, list, counters, scan, s);
}
}  // namespace

extern "C" size_t pnerf_render_cut_workspace_bytes(int R, int SR) {
    if (R < 0 || SR <= 0) return 0;
    CutWs w;
    return cut_ws_walk(nullptr, R, SR, w);
}

extern "C" int pnerf_cut_stage(const pnerf_camera *cam, const float *d_sample_loc, const int32_t *d_sample_nn, const int32_t *d_ray_hit,
                               const float *d_decoded, int R, int SR, float cutoff, int stage_samples, int stage,
                               float *d_trans, float *d_depth_max, int32_t *d_alive, int32_t *d_flags, int32_t *d_list, int32_t *d_counters,
                               void *d_ws, size_t ws_bytes, void *stream) {
    if (!cam || !d_sample_loc || !d_sample_nn || !d_ray_hit || !d_decoded || !d_trans || !d_depth_max || !d_alive || !d_flags || !d_list || !d_counters || !d_ws)
        return PNERF_E_INVAL;
    if (R < 0 || SR <= 0 || !(cutoff > 0.f && cutoff < 1.f) || stage_samples < 1 || stage < 0) return PNERF_E_INVAL;
    const int B = stage_samples < SR ? stage_samples : SR;
    if ((long long)stage * B >= SR) return PNERF_E_INVAL;
    if (ws_bytes < pnerf_compact_workspace_bytes((int64_t)R * SR)) return PNERF_E_WS;
    if (R == 0) return hipMemsetAsync(d_counters, 0, 8 * sizeof(int), (hipStream_t)stream) == hipSuccess ? 0 : PNERF_E_LAUNCH;
    return cut_stage_launch(*cam, d_sample_loc, d_sample_nn, d_ray_hit, d_decoded, R, SR, cutoff, B, stage, d_trans, d_depth_max, d_alive, d_flags, d_list,
                            d_counters, (int *)d_ws, (hipStream_t)stream);
}

extern "C" int pnerf_render_forward_cut(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *st, float cutoff, int stage_samples,
                                        float *d_decoded, float *d_weight, float *d_ray_color, float *d_opacity, float *d_bg_trans, float *d_blend_w,
                                        int32_t *d_cut_counters, void *d_ws, size_t ws_bytes, void *d_cut_ws, size_t cut_ws_bytes, void *stream) {
    if (!(cutoff >= 0.f && cutoff < 1.f) || stage_samples < 1) return PNERF_E_INVAL;
    int rc = check_step(cam, pts, st, ST_RENDER, d_decoded && d_weight && d_ray_color && d_opacity && d_bg_trans && d_blend_w && d_cut_counters);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_cut_counters, 0, 4 * sizeof(int), s) != hipSuccess) return PNERF_E_LAUNCH;
    if (st->R == 0) return 0;
    if (cutoff == 0.f) {                       // no cut: the body of pnerf_render_forward; every valid sample is shaded
        if ((rc = agg_forward(cam, pts, *st, d_decoded, d_weight, nullptr, d_ws, ws_bytes, /*save_x0=*/false, s)) != 0) return rc;
        if (hipMemcpyAsync(d_cut_counters, st->counters, sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess) return PNERF_E_LAUNCH;
        return raymarch_launch(cam, st, d_decoded, d_ray_color, d_opacity, d_bg_trans, d_blend_w, s);
    }
    const int R = st->R, SR = st->SR;
    PnSaved sv;
    if ((rc = agg_scratch(*st, nullptr, d_ws, ws_bytes, sv)) != 0) return rc;
    if (!d_cut_ws || cut_ws_bytes < pnerf_render_cut_workspace_bytes(R, SR)) return PNERF_E_WS;
    CutWs w;
    cut_ws_walk(d_cut_ws, R, SR, w);
    if ((rc = zero_outputs(*st, d_decoded, d_weight, s)) != 0) return rc;
    const int B = stage_samples < SR ? stage_samples : SR, n_stages = pn_cdiv(SR, B);
    pnerf_step stage_step = *st;               // the same launches as pnerf_render_forward's, on the stage's list and count
    stage_step.valid_list = w.list;
    for (int j = 0; j < n_stages; ++j) {
        stage_step.counters = w.counters + 8 * j;
        if ((rc = cut_stage_launch(*cam, st->sample_loc, st->sample_nn, /*hit=*/nullptr, d_decoded, R, SR, cutoff, B, j, w.T, w.cm, w.alive, w.flags, w.list,
                                   w.counters + 8 * j, w.scan, s)) != 0) return rc;
        if (st->n_valid_max > 0 && (rc = pn_agg_forward_launch(cam, pts, stage_step, d_decoded, d_weight, sv, /*train=*/false, /*save_x0=*/false, s)) != 0) return rc;
    }
    { PnProfScope prof(PNK_COMPACT, s);
    hipLaunchKernelGGL(k_cut_totals, dim3(1), dim3(1024), 0, s, w.counters, n_stages, w.alive, R, d_cut_counters); }
    PN_CHECK_LAUNCH();
    return raymarch_launch(cam, st, d_decoded, d_ray_color, d_opacity, d_bg_trans, d_blend_w, s);
}

// the ray-march backward in its two instances: the existing one, or GEOM when the caller has per-ray geometry gradients
static void raymarch_backward_launch(const RmArgs &ra, const float *d_grad_ray_color, const float *d_grad_geom, const float *d_z, float *d_grad_decoded, hipStream_t s) {
    const dim3 grid(pn_cdiv(ra.R, TPB / 64));
    if (!d_grad_geom) {
        hipLaunchKernelGGL(k_raymarch_backward<false>, grid, dim3(TPB), 0, s, ra, d_grad_ray_color, d_grad_decoded);
        return;
    }
    RmGeomArgs ga;
    static_cast<RmArgs &>(ga) = ra;
    ga.grad_geom = d_grad_geom; ga.z = d_z;
    hipLaunchKernelGGL(k_raymarch_backward<true>, grid, dim3(TPB), 0, s, ga, d_grad_ray_color, d_grad_decoded);
}

// both forms of the fused backward; d_grad_geom == NULL: the existing route and the existing instance
static int render_backward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *st,
                           const float *d_decoded, const float *d_weight, const float *d_grad_ray_color, const float *d_grad_geom,
                           void *d_saved, float *d_grad_params, const pnerf_point_grads *pg,
                           void *d_ws, size_t ws_bytes, void *stream) {
    int rc = check_step(cam, pts, st, ST_RENDER | ST_SAVING, d_decoded && d_weight && d_grad_ray_color && d_saved && d_grad_params && pg && d_ws);
    if (rc) return rc;
    const int R = st->R, SR = st->SR;
    const size_t gd_bytes = pn_align((size_t)R * SR * 4 * sizeof(float));
    if (SR > RM_BWD_MAX_SR) return PNERF_E_UNSUP;
    if (ws_bytes < gd_bytes + pn_wgrad_partials_bytes()) return PNERF_E_WS;
    if (R == 0 || st->n_valid_max == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    float *grad_decoded = (float *)d_ws;
    float *partials = (float *)((char *)d_ws + gd_bytes);
    { PnProfScope prof(PNK_RAYMARCH_BWD, s);
    raymarch_backward_launch(rm_args(*cam, st->sample_loc, st->sample_nn, d_decoded, R, SR), d_grad_ray_color, d_grad_geom, /*z=*/nullptr, grad_decoded, s); }
    PN_CHECK_LAUNCH();
    return pn_agg_backward_launch(cam, pts, *st, d_decoded, d_weight, grad_decoded, pn_saved_carve(d_saved, st->n_valid_max, st->K), d_grad_params, pg,
                                  partials, /*x0_saved=*/false, s);
}
extern "C" int pnerf_render_backward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *st,
                                     const float *d_decoded, const float *d_weight, const float *d_grad_ray_color,
                                     void *d_saved, float *d_grad_params, const pnerf_point_grads *pg,
                                     void *d_ws, size_t ws_bytes, void *stream) {
    return render_backward(cam, pts, st, d_decoded, d_weight, d_grad_ray_color, nullptr, d_saved, d_grad_params, pg, d_ws, ws_bytes, stream);
}
extern "C" int pnerf_render_backward_geom(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *st,
                                          const float *d_decoded, const float *d_weight, const float *d_grad_ray_color, const float *d_grad_geom,
                                          void *d_saved, float *d_grad_params, const pnerf_point_grads *pg,
                                          void *d_ws, size_t ws_bytes, void *stream) {
    return render_backward(cam, pts, st, d_decoded, d_weight, d_grad_ray_color, d_grad_geom, d_saved, d_grad_params, pg, d_ws, ws_bytes, stream);
}

extern "C" size_t pnerf_render_backward_workspace_bytes(int R, int SR) {
    return pn_align((size_t)R * SR * 4 * sizeof(float)) + pn_wgrad_partials_bytes();
}

// ================================ stand-alone (level-1) entry points ================================

extern "C" size_t pnerf_compact_workspace_bytes(int64_t n) { return pn_align(pn_scan_scratch_ints(n) * sizeof(int)); }

// d_list = ascending indices i with d_nn[i] > 0, d_counters[0] = their number (builds the aggregator's work list from
// a caller-supplied validity array: PointAggregator.forward's ray_valid = any_K(sample_pnt_mask), point_aggregators.py:741)
extern "C" int pnerf_compact_valid(const int32_t *d_nn, int64_t n, int32_t *d_list, int32_t *d_counters, void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_nn || !d_list || !d_counters || !d_ws || n < 0) return PNERF_E_INVAL;
    if (ws_bytes < pnerf_compact_workspace_bytes(n)) return PNERF_E_WS;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_counters, 0, 8 * sizeof(int), s) != hipSuccess) return PNERF_E_LAUNCH;
    if (n == 0) return 0;
    PnProfScope prof(PNK_COMPACT, s);
    return pn_compact_gt0_i32(d_nn, n, d_list, d_counters, (int *)d_ws, s);
}

extern "C" int pnerf_agg_forward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *st, float *d_decoded, float *d_weight,
                                 void *d_saved, void *d_ws, size_t ws_bytes, void *stream) {
    const int rc = check_step(cam, pts, st, d_saved ? ST_SAVING : 0, d_decoded && d_weight);
    return rc ? rc : agg_forward(cam, pts, *st, d_decoded, d_weight, d_saved, d_ws, ws_bytes, /*save_x0=*/d_saved != nullptr, (hipStream_t)stream);
}

extern "C" int pnerf_agg_backward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *st,
                                  const float *d_decoded, const float *d_weight, const float *d_grad_decoded,
                                  void *d_saved, float *d_grad_params, const pnerf_point_grads *pg, void *d_ws, size_t ws_bytes, void *stream) {
    int rc = check_step(cam, pts, st, ST_SAVING, d_decoded && d_weight && d_grad_decoded && d_saved && d_grad_params && pg && d_ws);
    if (rc) return rc;
    if (ws_bytes < pn_wgrad_partials_bytes()) return PNERF_E_WS;
    if (st->R == 0 || st->n_valid_max == 0) return 0;
    return pn_agg_backward_launch(cam, pts, *st, d_decoded, d_weight, d_grad_decoded, pn_saved_carve(d_saved, st->n_valid_max, st->K), d_grad_params, pg,
                                  (float *)d_ws, /*x0_saved=*/true, (hipStream_t)stream);
}

// ray_march(ray_dist, ray_valid, ray_features, radiance, alpha, bg_color)   models/rendering/diff_ray_marching.py:508-554
extern "C" int pnerf_raymarch_forward(const float *d_ray_dist, const uint8_t *d_ray_valid, const float *d_features, const float *bg3_host,
                                      int R, int SR, float *d_ray_color, float *d_opacity, float *d_acc_trans, float *d_blend_w,
                                      float *d_bg_trans, void *stream) {
    if (!d_ray_dist || !d_ray_valid || !d_features || !d_ray_color || !d_opacity || !d_acc_trans || !d_blend_w || !d_bg_trans || R < 0 || SR <= 0) return PNERF_E_INVAL;
    if (R == 0) return 0;
    const RmArgs ra = rm_args(d_ray_dist, d_ray_valid, bg3_host, d_features, R, SR);
    hipStream_t s = (hipStream_t)stream;
    PnProfScope prof(PNK_RAYMARCH_FWD, s);
    hipLaunchKernelGGL(k_raymarch_forward, dim3(pn_cdiv(R, TPB / 64)), dim3(TPB), 0, s, ra, d_ray_color, d_opacity, d_bg_trans, d_blend_w, d_acc_trans);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_raymarch_backward(const float *d_ray_dist, const uint8_t *d_ray_valid, const float *d_features, const float *bg3_host,
                                       int R, int SR, const float *d_grad_ray_color, float *d_grad_features, void *stream) {
    if (!d_ray_dist || !d_ray_valid || !d_features || !d_grad_ray_color || !d_grad_features || R < 0 || SR <= 0) return PNERF_E_INVAL;
    if (SR > RM_BWD_MAX_SR) return PNERF_E_UNSUP;
    if (R == 0) return 0;
    const RmArgs ra = rm_args(d_ray_dist, d_ray_valid, bg3_host, d_features, R, SR);
    hipStream_t s = (hipStream_t)stream;
    PnProfScope prof(PNK_RAYMARCH_BWD, s);
    raymarch_backward_launch(ra, d_grad_ray_color, nullptr, nullptr, d_grad_features, s);
    PN_CHECK_LAUNCH();
    return 0;
}

extern "C" int pnerf_raymarch_backward_geom(const float *d_ray_dist, const uint8_t *d_ray_valid, const float *d_features, const float *d_z, const float *bg3_host,
                                            int R, int SR, const float *d_grad_ray_color, const float *d_grad_geom, float *d_grad_features, void *stream) {
    if (!d_ray_dist || !d_ray_valid || !d_features || !d_z || !d_grad_ray_color || !d_grad_geom || !d_grad_features || R < 0 || SR <= 0) return PNERF_E_INVAL;
    if (SR > RM_BWD_MAX_SR) return PNERF_E_UNSUP;
    if (R == 0) return 0;
    const RmArgs ra = rm_args(d_ray_dist, d_ray_valid, bg3_host, d_features, R, SR);
    hipStream_t s = (hipStream_t)stream;
    PnProfScope prof(PNK_RAYMARCH_BWD, s);
    raymarch_backward_launch(ra, d_grad_ray_color, d_grad_geom, d_z, d_grad_features, s);
    PN_CHECK_LAUNCH();
    return 0;
}
