/*
 * pnerf.h -- C ABI of libpnerf_hip.so, the MI355X (gfx950) implementation of the Point-NeRF
 * render/optimise hot path.
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory owned by the caller (contiguous, 16-byte aligned);
 *     the library never allocates or frees device memory: sizes of scratch areas are returned by
 *     the *_bytes() queries and the caller (torch's caching allocator in the Python host) provides
 *     them;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it (no host
 *     synchronisation) unless its comment says "synchronous";
 *   - return value: 0 = ok, <0 = PNERF_E_* (nothing was enqueued);
 *   - not thread-safe per stream, re-entrant across streams.
 *
 * Each entry point cites the reference interface it replaces (paths under /root/reference).
 */
#ifndef PNERF_H
#define PNERF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNERF_E_INVAL   (-1)   /* bad argument (null pointer, K/SR/P out of range, ...) */
#define PNERF_E_WS      (-2)   /* workspace too small */
#define PNERF_E_LAUNCH  (-3)   /* hipGetLastError() != hipSuccess after a launch */
#define PNERF_E_UNSUP   (-4)   /* configuration not supported by this build */

#define PNERF_MAX_K 16

/* Grid description: what lighting_fast_querier.get_hyperparameters computes per call
 * (models/neural_points/point_query.py:47-71) plus the querier constants of :35-42. */
typedef struct pnerf_grid_params {
    float ranges[6];       /* padded min xyz [0..2] / max xyz [3..5]  (ranges_tensor) */
    float vsize[3];        /* scaled voxel size = vsize * vscale       (scaled_vsize)  */
    int32_t vdim[3];       /* grid dimensions                          (scaled_vdim)   */
    int32_t kernel_size[3];/* neighbor search window (layers = (ks[0]+1)/2) */
    int32_t query_size[3]; /* occupancy dilation window */
    int32_t P;             /* max points per voxel */
    int32_t max_o;         /* max occupied voxels (overflow is reported, see pnerf_grid_info) */
    float radius;          /* radius_limit (0 disables the radius test) */
} pnerf_grid_params;

/* info words written by pnerf_grid_build at the start of the grid workspace */
enum { PNERF_GI_N_IN_GRID = 0, PNERF_GI_N_OCC = 1, PNERF_GI_MAX_CNT = 2, PNERF_GI_CELL0 = 3,
       PNERF_GI_FIRST_IDX = 4, PNERF_GI_OSTART_OFF = 5 /* internal: where the cell offsets sit in the workspace */, PNERF_GI_LEN = 8 };

/* ---- library ---------------------------------------------------------------------------- */
int pnerf_version(void);                 /* 1000*major + minor */
const char *pnerf_arch(void);            /* "gfx950" */

/* ---- voxel grid (replaces claim_occ / map_coor2occ / fill_occ2pnts and their ~140 MB of
 * per-call tables: models/neural_points/cuda/query_worldcoords.cu:18-162, host :308-365).
 * Deterministic by construction: points of a cell are stored in ascending point index (the
 * reference's canonical serial order), the dilated occupancy is a bit field.  The grid is a
 * function of (xyz, params) only and is meant to be cached across calls by the host. */
size_t pnerf_grid_workspace_bytes(const pnerf_grid_params *gp, int n_points);
int pnerf_grid_build(const pnerf_grid_params *gp, const float *d_xyz, int n_points,
                     void *d_grid_ws, size_t ws_bytes, void *stream);
/* synchronous: copies the PNERF_GI_* words to host_info[PNERF_GI_LEN] (stream is synchronised) */
int pnerf_grid_info(const void *d_grid_ws, int32_t *host_info, void *stream);
/* Elementwise minimum and maximum over the points: d_out6 = {min x, min y, min z, max x, max y, max z} (device, 6 floats), what
 * lighting_fast_querier.get_hyperparameters (models/neural_points/point_query.py:51-52) takes with torch.min / torch.max before it clamps to
 * opt.ranges and pads: one HBM pass, asynchronous on `stream`.  Comparisons are exact (no arithmetic on the values); NaN coordinates are not
 * ordered (the reference's reductions would propagate them). */
int pnerf_points_minmax(const float *d_xyz, int64_t n_points, float *d_out6, void *stream);

/* ---- query (replaces mask_raypos / get_shadingloc / query_neigh_along_ray_layered and the ATen
 * glue between them: query_worldcoords.cu:165-302, host :367-431; entry point
 * woord_query_grid_point_index, query_worldcoords.cpp:34-82).
 *
 * Ray samples come either from d_raypos [R,D,3] (the native op's own input) or -- fused, never
 * materialised -- from campos + raydir * mid[d] with the D mid-point depths d_mid computed by the
 * host exactly as near_far_linear_ray_generation does (models/rendering/diff_ray_marching.py:369-392).
 * If jitter > 0 (training: point_query.py:81 uses 0.3) d_mid holds the D un-jittered segment lengths and every segment is
 * scaled by 1 + jitter (U - 0.5) in-kernel, U = pnerf_debug_uniform(seed, ray * D + d); the end points are the SEQUENTIAL fp32
 * running sum (torch.cumsum of the reference's CPU path), so the samples are bit-defined; near/far are then required.
 *
 * Outputs are DENSE OVER ALL R RAYS (no host sync, no compaction):
 *   d_sample_loc  [R,SR,3] f32   world position of the first <=SR occupied samples, 0 elsewhere
 *   d_sample_pidx [R,SR,K] i32   neighbor point indices in the reference's slot order, -1 padded
 *   d_sample_nn   [R,SR]   i32   number of valid neighbors of each sample (0 for empty slots)
 *   d_ray_hit     [R]      i32   1 if the ray has at least one sample with a neighbor
 *   d_valid_list  [R*SR]   i32   ascending list of r*SR+s with nn>0 (the aggregator's work list)
 *   d_counters    [8]      i32   [0]=#valid samples (len of d_valid_list) [1]=#rays hit
 *                                [2]=#selected samples [3]=#valid neighbor slots
 * The reference's [R'',...] outputs are row gathers of these by d_ray_hit (done by the host). */
size_t pnerf_query_workspace_bytes(int R, int SR);
int pnerf_query(const pnerf_grid_params *gp, const void *d_grid_ws,
                const float *d_raypos,                       /* [R,D,3] or NULL */
                const float *campos3_host, const float *d_raydir, const float *d_mid,   /* used if d_raypos==NULL */
                float near_depth, float far_depth, float jitter, uint64_t seed,
                int R, int D, int SR, int K,
                float *d_sample_loc, int32_t *d_sample_pidx, int32_t *d_sample_nn,
                int32_t *d_ray_hit, int32_t *d_valid_list, int32_t *d_counters,
                void *d_query_ws, size_t ws_bytes, void *stream);

/* ---- per-neighbor gather (NeuralPoints.forward's index_select block,
 * models/neural_points/neural_points.py:706-717) and its backward scatter-add.  Row i of each
 * output holds point max(idx[i],0): -1 slots read point 0 exactly as the reference does. */
int pnerf_gather_rows(const float *d_src, int n_src, int width, const int32_t *d_idx, int64_t n_idx,
                      float *d_dst, void *stream);
int pnerf_scatter_add_rows(const float *d_grad_rows, const int32_t *d_idx, int64_t n_idx, int width,
                           float *d_grad_src, int n_src, void *stream);

/* ---- the zero-one regulariser on the neighbor slots' confidences, fused (gather + gradient_clamp of
 * models/aggregators/point_aggregators.py:722-724,812 + loss_zero_one of models/base_rendering_model.py:630-641 + their backward).
 * forward: d_partial[b], b < pnerf_zero_one_blocks(n_idx), = per-block sums of log(v) + log(1 - v) over the n_idx slots
 * (v = clamp(clamp(conf[max(idx, 0)], 1e-4, 1), eps, 1 - eps)); the caller adds them and divides by its (global) element count.
 * backward: d_grad_conf[max(idx, 0)] += d_gscale[0] * (1 / v - 1 / (1 - v)) where the clamp to [eps, 1 - eps] was inactive. */
int pnerf_zero_one_blocks(int64_t n_idx);
int pnerf_zero_one_forward(const float *d_conf, int n_points, const int32_t *d_idx, int64_t n_idx, float eps,
                           float *d_partial, void *stream);
int pnerf_zero_one_backward(const float *d_conf, int n_points, const int32_t *d_idx, int64_t n_idx, float eps,
                            const float *d_gscale, float *d_grad_conf, void *stream);
/* the same over the DENSE neighbor table d_idx [R][slots_per_ray] of a query, restricted to the rays with d_ray_hit[r] > 0 (the reference's
 * conf_coefficient exists for the hit rays only): no [R'', SR, K] copy of the table is made.  d_partial holds pnerf_zero_one_blocks(R * 256)
 * floats; the caller divides by (hit rays) x slots_per_ray.  (One kernel pair serves both forms: the flat list is rows of 256 slots without hit flags.) */
int pnerf_zero_one_forward_rays(const float *d_conf, int n_points, const int32_t *d_idx, const int32_t *d_ray_hit, int R, int slots_per_ray, float eps,
                                float *d_partial, void *stream);
int pnerf_zero_one_backward_rays(const float *d_conf, int n_points, const int32_t *d_idx, const int32_t *d_ray_hit, int R, int slots_per_ray, float eps,
                                 const float *d_gscale, float *d_grad_conf, void *stream);
/* the colour term of the training loss (models/base_rendering_model.py:543-551 "ray_masked_coarse_raycolor": sum over the rays that hit of
 * (colour - gt)^2; the caller divides by its global element count) over the DENSE ray colours d_ray_color [R,3] / d_gt [R,3] with the rays' hit
 * flags -- the hit rays are not compacted on the way to a scalar.  forward: d_partial[b], b < pnerf_color_loss_blocks(R), block sums.
 * backward: d_grad_ray_color [R,3] = 2 d_gscale[0] (colour - gt) for a hit ray, 0 for a miss (every element is written). */
int pnerf_color_loss_blocks(int R);
int pnerf_color_loss_forward_rays(const float *d_ray_color, const float *d_gt, const int32_t *d_ray_hit, int R, float *d_partial, void *stream);
int pnerf_color_loss_backward_rays(const float *d_ray_color, const float *d_gt, const int32_t *d_ray_hit, int R, const float *d_gscale,
                                   float *d_grad_ray_color, void *stream);

/* the depth and the background (mask) terms of the training loss (models/base_rendering_model.py:610-626: l2loss(coarse_depth * gt_mask,
 * gt_depth * gt_mask) and l2loss(coarse_is_background * (1 - gt_mask), 1 - gt_mask); the caller divides by its global ray count) over the DENSE
 * per-ray results of a render: d_depth_sum / d_acc [R] as pnerf_ray_geometry wrote them, d_bg_trans [R] as pnerf_render_forward did, the rays'
 * hit flags, d_gt_depth / d_gt_mask [R].  Per ray, m = gt_mask, d = depth_sum / (acc + 1e-6f) (models/neural_points_volumetric_model.py:321;
 * the 1 / (acc + 1e-6) of a hit but almost transparent ray is the reference's formula and is kept), T = bg_trans; a ray with d_ray_hit <= 0
 * counts with d = 0 and T = 1 (fill_invalid's values) and its rows are not read.
 * forward: d_partial [2 * pnerf_color_loss_blocks(R)]: the block sums of (m (d - gt_depth))^2, then those of ((1 - m) (T - 1))^2.
 * backward: d_grad_geom [R,3] = the gradient of d_gscale2[0] * (depth numerator) + d_gscale2[1] * (bg numerator) with respect to
 * (depth_sum, acc, T): g_ds = 2 m^2 (d - gt) / (acc + 1e-6), g_acc = -g_ds d, g_T = 2 (1 - m)^2 (T - 1); zeros for a miss (every element is
 * written): the d_grad_geom of pnerf_render_backward_geom. */
int pnerf_geometry_loss_forward_rays(const float *d_depth_sum, const float *d_acc, const float *d_bg_trans, const int32_t *d_ray_hit,
                                     const float *d_gt_depth, const float *d_gt_mask, int R, float *d_partial, void *stream);
int pnerf_geometry_loss_backward_rays(const float *d_depth_sum, const float *d_acc, const float *d_bg_trans, const int32_t *d_ray_hit,
                                      const float *d_gt_depth, const float *d_gt_mask, int R, const float *d_gscale2, float *d_grad_geom, void *stream);

/* ---- aggregator MLP + renderer (PointAggregator.forward/viewmlp,
 * models/aggregators/point_aggregators.py:488-644,727-814; ray-dist,
 * models/neural_points_volumetric_model.py:271-279; ray_march,
 * models/rendering/diff_ray_marching.py:508-554).  Lego-script architecture only:
 * 284->256->256, (+7)->256->256, alpha 256->1, colour 280->128->128->128->3, LeakyReLU(0.01),
 * linear distance kernel, agg_dist_pers=20, agg_intrp_order=2.                                   */

/* Offsets (in floats) of each tensor inside the flat MLP parameter / gradient vector, in the
 * reference's state_dict order: block1.0.{weight,bias}, block1.2.*, block3.0.*, block3.2.*,
 * alpha_branch.0.*, color_branch.{0,2,4,6}.* ; every weight is [out,in] row-major (torch layout). */
#define PNERF_MLP_NTENSORS 18
int pnerf_mlp_layout(int feat_dim, int64_t *offsets /*[PNERF_MLP_NTENSORS+1]*/);
size_t pnerf_mlp_packed_bytes(void);
/* repack the flat parameter vector into MFMA fragment order: 14 two-plane f16 images (forward W and dgrad W^T of the four aggregator and three colour
 * layers, csrc/f16x3.h) and the 8 mixed-format images of the aggregator layers (f16 h fragments + e4m3 cross-term fragments with block exponents,
 * csrc/mixq.h).  Called once per optimisation step (the weights change); ~20 us. */
int pnerf_mlp_pack(const float *d_params, void *d_packed, void *stream);

typedef struct pnerf_camera {
    float campos[3];
    float camrot[9];       /* c2w rotation, row-major */
    float rw2c[9];         /* NeuralPoints.Rw2c when it is ONE [3,3] frame, row-major (identity in every training script): rotates the first
                            * three distance components, the points' stored directions and the view direction (v -> rw2c v).  A cloud
                            * with one frame PER POINT (scene editing) passes pnerf_points.frames instead; rw2c is then not read */
    float vsize_z;         /* unscaled opt.vsize[2] (ray-dist clamp) */
    int32_t raydist_mode_unit;
    float bg[3];           /* background colour */
    int32_t has_bg;
} pnerf_camera;

typedef struct pnerf_points {        /* the neural point cloud, all [N,*] row-major f32 */
    const float *xyz;                /* [N,3]  */
    const float *embedding;          /* [N,F]  */
    const float *conf;               /* [N,1]  */
    const float *dir;                /* [N,3]  */
    const float *color;              /* [N,3]  */
    int32_t n, feat_dim;
    const float *frames;             /* optional [N,9] (NULL: cam.rw2c for every point): NeuralPoints.Rw2c [N,3,3] of a composed scene
                                      * (run/editing.py; models/aggregators/point_aggregators.py:492-496,506,526,566), row-major as in the
                                      * checkpoint.  A neighbor row of point p uses F[p] for its distance components and stored direction;
                                      * the view direction of a sample uses the frame of the sample's slot-0 point (empty: point 0) -- also in
                                      * the rows' (dir - view, dir . view) extras.  RENDER-ONLY: with d_saved != NULL (a training forward) or in
                                      * pnerf_render_backward / pnerf_agg_backward -> PNERF_E_INVAL; served by the default inference arithmetic
                                      * only: pnerf_set_inference_products(2) or bit 0 of pnerf_set_cross_terms_where -> PNERF_E_UNSUP.
                                      * pnerf_agg_forward: indexed like the other pseudo-point arrays, by the slot number */
} pnerf_points;

typedef struct pnerf_point_grads {   /* gradient accumulators (added to, never zeroed) */
    float *embedding, *conf, *dir, *color;
    void *ready_event;               /* optional hipEvent_t (NULL: none): recorded on the call's stream as soon as the four point
                                      * gradients are complete, i.e. BEFORE the weight-gradient GEMMs of the same call are
                                      * enqueued -- a data-parallel caller starts the all-reduce of the (large) point
                                      * gradients on another stream behind this event and overlaps it with those GEMMs */
    const float *zero_one_gscale;    /* optional (NULL: none; pnerf_render_backward only): the conf gradient of the zero-one regulariser on the
                                      * hit rays' conf_coefficient (pnerf_zero_one_backward_rays: += d_gscale[0] (1 / v - 1 / (1 - v)) per neighbor slot,
                                      * empty slots on point 0) is added BY THIS CALL -- the term of a slot rides on the conf atomic the backward issues
                                      * for that neighbor row anyway, the empty slots of the hit rays are one closed-form addition to point 0
                                      * ((#rays hit x SR x K - #valid neighbor slots) identical terms): the regulariser's own pass of ~7 M atomics on
                                      * the same addresses is not run */
    float zero_one_eps;              /* its clamp bound (opt.zero_epsilon) */
    float *xyz;                      /* optional [N,3] (NULL: none; pnerf_render_backward only): d xyz of the point positions (xyz_grad), through
                                      * the distance encoding and the inverse-distance weights of every neighbor row that names the point */
} pnerf_point_grads;

/* One render step's inputs: what the four entry points below (pnerf_render_forward / _backward, pnerf_agg_forward / _backward) all read.  The
 * forward and the backward of a step get the same record. */
typedef struct pnerf_step {
    const float *raydir;             /* [R,3]     all four */
    const float *sample_loc;         /* [R,SR,3]  all four: world position of the samples (pnerf_query's d_sample_loc) */
    const int32_t *sample_pidx;      /* [R,SR,K]  all four: neighbor point indices, -1 padded */
    const int32_t *sample_nn;        /* [R,SR]    pnerf_render_forward / _backward only (NULL for the pnerf_agg_* pair): valid neighbors per sample */
    const int32_t *valid_list;       /* all four: ascending list of r*SR+s with nn>0 (the aggregator's work list) */
    const int32_t *counters;         /* [8]       all four: [0]=#valid samples (len of valid_list) ... as pnerf_query writes them */
    const float *xyz_pers;           /* [N,3]     read by pnerf_agg_forward only, both or neither: the caller's perspective coordinates */
    const float *loc_pers;           /* [R,SR,3]  (sampled_xyz_pers, sample_loc); both NULL = project from cam.  Enforced: one without the other, or
                                      * either one given to pnerf_render_forward / _backward (which project from cam) -> PNERF_E_INVAL */
    const float *params;             /* all four: the flat MLP parameter vector (pnerf_mlp_layout order) */
    const void *packed_mlp;          /* all four: its packed image (pnerf_mlp_pack) */
    int32_t R, SR, K;
    int64_t n_valid_max;             /* all four: capacity in valid samples (>= counters[0], which the host reads once per call to size its
                                      * buffers); the backward of a step must get the n_valid_max of its forward */
} pnerf_step;

/* bytes of saved activations per valid neighbor row / per valid sample (training forward) */
size_t pnerf_agg_saved_bytes(int64_t n_valid_samples, int K);
size_t pnerf_agg_workspace_bytes(int64_t n_valid_max, int K);   /* inference scratch for n_valid_max valid samples */
size_t pnerf_render_backward_workspace_bytes(int R, int SR);

/* Forward: for every valid sample in step->valid_list computes (sigma, r, g, b) into
 * d_decoded [R,SR,4] (zero elsewhere), d_weight [R,SR,K] (normalised distance weights, before
 * confidence), then ray-dist + alpha compositing into d_ray_color [R,3], d_opacity [R,SR],
 * d_bg_trans [R], d_blend_w [R,SR].  Inference: d_saved == NULL and d_ws holds
 * pnerf_agg_workspace_bytes(n_valid_max, K).  Training: d_saved holds pnerf_agg_saved_bytes(n_valid_max, K)
 * and keeps the activations needed by pnerf_render_backward (which must get the same n_valid_max). */
int pnerf_render_forward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *step,
                         float *d_decoded, float *d_weight, float *d_ray_color, float *d_opacity,
                         float *d_bg_trans, float *d_blend_w,
                         void *d_saved, void *d_ws, size_t ws_bytes, void *stream);

/* ---- early ray termination of a RENDER-ONLY pass (the "cut render").  The reference has no counterpart for the cut itself: it shades
 * every valid sample of every hit ray; what is thresholded here is the transmittance of its ray_march
 * (models/rendering/diff_ray_marching.py:508-554).  With cutoff c in (0, 1) and a stage width of B = min(stage_samples, SR) slots a ray is
 * shaded front to back in ceil(SR / B) stages, stage j = slots [jB, min((j+1)B, SR)) (the query packs a ray's samples from slot 0 upwards in
 * depth order):
 *   T_r(s) = the exclusive transmittance in front of slot s exactly as pnerf_render_forward's ray march forms it (the same ray-dist
 *            deltas, u = 1 - op + 1e-10, the product over the slots < s), on the d_decoded values written so far: unshaded samples
 *            count as sigma = 0;
 *   ray r is alive at stage 0 (a ray without a valid sample has nothing to shade); alive at stage j >= 1 if alive at j - 1 and T_r(jB) >= c;
 *   stage j shades the samples with a neighbor of the alive rays in its slots: the launches of pnerf_render_forward on the stage's own
 *            work list and count (no host read between stages; whatever inference arithmetic is selected; per-point frames as there);
 *   after the last stage pnerf_render_forward's ray march runs once over the dense d_decoded.
 * Unshaded samples therefore have d_decoded = d_weight = d_opacity = d_blend_w = 0, and d_bg_trans of a ray that was cut is its
 * transmittance AT TERMINATION (< c), not the value of the full render.  Error bound: decoded RGB lies in [-0.001, 1.001] (sigmoid * 1.002
 * - 0.001) and the background in [0, 1]; what is dropped is, up to the 1e-10 terms, a convex combination of such values times T_cut < c, so
 * every channel of d_ray_color differs from pnerf_render_forward's by less than 1.002 c.  No atomics: two calls give the same bits.
 *
 * d_cut_counters [4] i32: [0] = samples shaded, [1] = rays that ended with at least one valid sample unshaded, [2] = [3] = 0.
 * d_ws as pnerf_render_forward's inference workspace (pnerf_agg_workspace_bytes(step->n_valid_max, K): reused stage after stage);
 * d_cut_ws holds pnerf_render_cut_workspace_bytes(R, SR).  Inference only (no saved area).  PNERF_E_INVAL: cutoff outside [0, 1),
 * stage_samples < 1, a null pointer, and everything pnerf_render_forward refuses (the same PNERF_E_UNSUP cases too);
 * cutoff == 0 runs the body of pnerf_render_forward (d_cut_ws is not used; [0] = step->counters[0]). */
size_t pnerf_render_cut_workspace_bytes(int R, int SR);
int pnerf_render_forward_cut(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *step, float cutoff, int stage_samples,
                             float *d_decoded, float *d_weight, float *d_ray_color, float *d_opacity, float *d_bg_trans, float *d_blend_w,
                             int32_t *d_cut_counters, void *d_ws, size_t ws_bytes, void *d_cut_ws, size_t cut_ws_bytes, void *stream);
/* ONE stage of the cut render on caller-supplied dense arrays (d_sample_loc [R,SR,3], d_sample_nn [R,SR], d_ray_hit [R], d_decoded [R,SR,4]
 * as written by the stages before): the step of stage `stage` (advance T through the slots of stage - 1, decide alive, flag the stage's
 * slots) and the compaction of the flags.  The transmittance is ray_march's, models/rendering/diff_ray_marching.py:508-554; the cut has no
 * reference counterpart.  Per-ray state, written by stage 0 and updated by every later one (call the stages in order):
 *   d_trans [R] f32      T in front of slot stage * B (frozen once the ray has ended)
 *   d_depth_max [R] f32  running maximum of the perspective depth over the slots < (stage - 1) * B + B (-inf at stage 0)
 *   d_alive [R] i32      1 = alive; 0 = missed the cloud, or ended with nothing left to shade; 2 = ended with a valid sample unshaded
 * Outputs: d_flags [R,SR] i32 0/1 (every element written), d_list [max(R*SR,1)] the ascending r * SR + s of the flags, d_counters [8] with
 * [0] = its length (the words the aggregator launches read).  d_ws holds pnerf_compact_workspace_bytes(R * SR).  cutoff in (0, 1);
 * PNERF_E_INVAL also for stage * B >= SR. */
int pnerf_cut_stage(const pnerf_camera *cam, const float *d_sample_loc, const int32_t *d_sample_nn, const int32_t *d_ray_hit,
                    const float *d_decoded, int R, int SR, float cutoff, int stage_samples, int stage,
                    float *d_trans, float *d_depth_max, int32_t *d_alive, int32_t *d_flags, int32_t *d_list, int32_t *d_counters,
                    void *d_ws, size_t ws_bytes, void *stream);

/* Arithmetic of the INFERENCE forward (d_saved == NULL; pnerf_render_forward and pnerf_agg_forward): every fp32 GEMM operand is two f16
 * planes and a multiply-add is 3 MFMA products (default: fp32-class accuracy, sigma / RGB ~1e-6 from an fp32 evaluation) or 2 (the
 * weights' residual plane dropped: a third of the matrix work and half of the weight stream less; measured: rendered ray colour 1e-6 ..
 * 2e-5 from fp32, inside the 1e-4 bar, but per-sample sigma / RGB 2e-4 .. 4e-4, outside it -- which is why it is an OPTION for previews
 * and evaluation loops and not the default; nothing differentiates through it).  Training forwards always run 3.  Returns the
 * previous setting, or PNERF_E_INVAL for n not in {2, 3}.  Process-wide. */
int pnerf_set_inference_products(int n);

/* Arithmetic of the WEIGHT-GRADIENT GEMMs of the training backward (dW = dY^T X summed over all neighbor rows / samples of the step; the
 * reference: cuBLAS SGEMMs under loss.backward(), models/mvs_points_volumetric_model.py:98-118).  1 (default): each operand is streamed as
 * ONE f16 plane rounded to nearest, one MFMA product (11-bit significands, fp32 accumulation; the rounding errors are unbiased and add up
 * like a random walk over the rows: DESIGN.md 4.1).  2: both operands as TWO f16 planes (22 bits), three products -- the arithmetic of the
 * forward and of the input-gradient chain, i.e. fp32-class weight gradients; the forward then saves, and the weight-gradient GEMMs stream,
 * twice the bytes (pnerf_agg_saved_bytes grows accordingly: size the arena AFTER choosing the mode, and keep the mode fixed between a
 * training forward and its backward).  Returns the previous setting, or PNERF_E_INVAL for n not in {1, 2}.  Process-wide. */
int pnerf_set_wgrad_planes(int n);
/* Arithmetic of the CROSS TERMS of the aggregator's tile GEMMs (the four 256-wide nn.Linear layers of
 * models/aggregators/point_aggregators.py:286-344, forward and input-gradient chain).  Every fp32 operand is h + m (two f16 numbers, 22 bits) and
 * a product is h*h + (h*m + m*h): the leading term always runs on f16 factors; the two cross terms, 2^-11 of the result, run on
 * 8 (default, csrc/mixq.h): e4m3 factors on v_mfma_scale_f32_32x32x64_f8f6f4 (weights with per-lane block scales), 2 instead of 3 matrix-pipe
 *    passes per multiply-add, 1.3e-6 rms of sum |terms| per 256-term dot product (tests/test_gpu_mix.py);
 * 16 (csrc/f16x3.h, the arithmetic of rounds 2-5): f16 factors, 3e-8 rms.
 * The two-plane weight-gradient mode (pnerf_set_wgrad_planes(2)) and the two-product inference option always use 16.  Returns the previous
 * setting, or PNERF_E_INVAL.  Process-wide; may change between a training forward and its backward (the saved activations do not depend on it). */
int pnerf_set_cross_terms(int bits);
/* WHICH tile kernels use the e4m3 cross terms while pnerf_set_cross_terms is 8: bit 0 = the inference forward, bit 1 = the training forward,
 * bit 2 = the backward's input-gradient chain.  Default 4 (backward only): gradients stay inside every bar of the oracle comparison (the
 * LeakyReLU masks come from an fp32-class forward), the step is 8 % faster.  With the forward bits set sigma / RGB are 1e-5 .. 6e-5 from the
 * oracle (bar 1e-4; f16 cross terms: 1e-6) and the step is 15 % faster, but pre-activations that close to zero take the other LeakyReLU branch
 * than the fp32 oracle's, which the gradient comparisons against the oracle see (bench.py reports that variant).  Returns the previous mask, or
 * PNERF_E_INVAL.  Process-wide. */
int pnerf_set_cross_terms_where(int mask);
/* The four settings above as they are now, without changing them: out = {inference products, weight-gradient planes, cross-term bits, the
 * cross-term mask AS STORED} (the mask takes effect only while the cross-term bits are 8).  0, or PNERF_E_INVAL for a null pointer. */
int pnerf_get_arithmetic(int32_t out[4]);
/* Tests only: caps the grid of the aggregator's tile kernels and of the colour kernels at max_workgroups (0, the default: as many workgroups
 * as stay resident, two or three per CU).  Which workgroup runs a tile does not change a forward's results and changes gradients only by the
 * order of their atomic additions; a small grid reaches the edges of the kernels' tile claim with a handful of tiles.  Returns the previous
 * cap, or PNERF_E_INVAL for a negative one.  Process-wide and unsynchronised: every launcher reads it, so it must not be changed while another
 * thread may be inside a pnerf_render_* / pnerf_agg_* call. */
int pnerf_debug_set_tile_grid(int max_workgroups);

/* Backward of pnerf_render_forward for dL/d(ray_color) = d_grad_ray_color [R,3]:
 * accumulates dL/d(MLP params) into d_grad_params (flat, pnerf_mlp_layout order) and
 * dL/d(point tensors) into pg.  d_decoded / d_weight: the forward's results;
 * d_ws holds pnerf_render_backward_workspace_bytes(R, SR). */
int pnerf_render_backward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *step,
                          const float *d_decoded, const float *d_weight, const float *d_grad_ray_color,
                          void *d_saved, float *d_grad_params, const pnerf_point_grads *pg,
                          void *d_ws, size_t ws_bytes, void *stream);
/* The same backward for a loss that also reads the ray's geometry (the depth and bg loss items of models/base_rendering_model.py:610-626 on
 * the depth of models/neural_points_volumetric_model.py:318-322 and on ray_march's background transmittance, models/rendering/
 * diff_ray_marching.py:533-545): d_grad_geom [R,3] = per ray the gradients (g_ds, g_acc, g_T) with respect to pnerf_ray_geometry's
 * d_depth_sum = sum_s bw_s z_s and d_acc = sum_s bw_s and to pnerf_render_forward's d_bg_trans.  They enter the ray march's backward as
 * further channels of the colour recurrence (per slot c_s += g_ds z_s + g_acc, per ray g . bg += g_T; z_s = the camera-z depth of the
 * sample, 0 on an empty slot, whose position is not read), so d sigma arrives at the aggregator's backward with the three terms in it;
 * sample positions do not depend on the point positions: d xyz has no new term.  d_grad_geom == NULL: pnerf_render_backward, launch for
 * launch.  Everything else -- checks, workspace, return codes -- as pnerf_render_backward. */
int pnerf_render_backward_geom(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *step,
                               const float *d_decoded, const float *d_weight, const float *d_grad_ray_color, const float *d_grad_geom,
                               void *d_saved, float *d_grad_params, const pnerf_point_grads *pg,
                               void *d_ws, size_t ws_bytes, void *stream);

/* ---- stand-alone (level-1) forms of the same kernels, for callers that use the reference's modules one by one ---- */

/* work list from a caller-supplied per-sample neighbor count (ray_valid = any_K(sample_pnt_mask),
 * models/aggregators/point_aggregators.py:741): d_list = ascending i with d_nn[i] > 0, d_counters[0] = count */
size_t pnerf_compact_workspace_bytes(int64_t n);
/* d_flags [n_points] int32 := 1 for every point index that occurs in d_pidx [n] (>= 0), 0 elsewhere; d_flags[0] := 1 as well if any entry
 * is negative (an empty neighbor slot reads point 0: models/neural_points/neural_points.py:709).  The rows of the per-point gradients a
 * rank can have touched: the sparse gradient exchange of the data-parallel step (no reference counterpart: its DataParallel is batch 1,
 * models/neural_points_volumetric_model.py:165-168). */
int pnerf_touched_flags(const int32_t *d_pidx, int64_t n, int32_t n_points, int32_t *d_flags, void *stream);
int pnerf_compact_valid(const int32_t *d_nn, int64_t n, int32_t *d_list, int32_t *d_counters, void *d_ws, size_t ws_bytes, void *stream);

/* PointAggregator.forward (point_aggregators.py:727-814) on its own: -> d_decoded [R,SR,4], d_weight [R,SR,K].
 * Scratch/saved sizing as pnerf_render_forward. */
int pnerf_agg_forward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *step, float *d_decoded, float *d_weight,
                      void *d_saved, void *d_ws, size_t ws_bytes, void *stream);
/* its backward for dL/d(decoded) = d_grad_decoded [R,SR,4]; d_ws holds pnerf_render_backward_workspace_bytes(0, 1) */
int pnerf_agg_backward(const pnerf_camera *cam, const pnerf_points *pts, const pnerf_step *step,
                       const float *d_decoded, const float *d_weight, const float *d_grad_decoded,
                       void *d_saved, float *d_grad_params, const pnerf_point_grads *pg, void *d_ws, size_t ws_bytes, void *stream);

/* ray_march(ray_dist, ray_valid, ray_features, radiance, alpha, bg) (models/rendering/diff_ray_marching.py:508-554):
 * d_ray_dist [R,SR] f32, d_ray_valid [R,SR] u8, d_features [R,SR,4] (sigma,r,g,b), bg3_host NULL = no background.
 * PNERF_E_INVAL: a null pointer other than bg3_host, R < 0, SR <= 0.  R == 0: nothing is enqueued.  The backward keeps one lane per
 * 64-slot chunk of a ray: SR > 4096 -> PNERF_E_UNSUP, from pnerf_raymarch_backward and from pnerf_render_backward (the reference's
 * largest SR is 400). */
int pnerf_raymarch_forward(const float *d_ray_dist, const uint8_t *d_ray_valid, const float *d_features, const float *bg3_host,
                           int R, int SR, float *d_ray_color, float *d_opacity, float *d_acc_trans, float *d_blend_w,
                           float *d_bg_trans, void *stream);
int pnerf_raymarch_backward(const float *d_ray_dist, const uint8_t *d_ray_valid, const float *d_features, const float *bg3_host,
                            int R, int SR, const float *d_grad_ray_color, float *d_grad_features, void *stream);
/* ray_march's backward for a loss on (ray colour, depth_sum = sum_s blend_weight_s z_s, acc = sum_s blend_weight_s, background transmittance)
 * (models/rendering/diff_ray_marching.py:508-554; the depth of models/neural_points_volumetric_model.py:318-322): pnerf_raymarch_backward
 * plus d_z [R,SR] f32, the slots' depths (read on valid slots only), and d_grad_geom [R,3] = (g_ds, g_acc, g_T) per ray.  d sigma gets all
 * four terms, d rgb is pnerf_raymarch_backward's; with d_grad_geom all zeros so is d sigma.  Checks and return codes as
 * pnerf_raymarch_backward: PNERF_E_INVAL for a null pointer other than bg3_host, R < 0, SR <= 0; PNERF_E_UNSUP for SR > 4096; R == 0:
 * nothing is enqueued. */
int pnerf_raymarch_backward_geom(const float *d_ray_dist, const uint8_t *d_ray_valid, const float *d_features, const float *d_z, const float *bg3_host,
                                 int R, int SR, const float *d_grad_ray_color, const float *d_grad_geom, float *d_grad_features, void *stream);

/* ---- parameter update: one Adam step of one tensor in one pass (the reference steps two torch.optim.Adam instances,
 * models/mvs_points_volumetric_model.py:80-91 and :98-118; lr / plr, betas (0.9, 0.999), eps 1e-8, no weight decay).
 * All four arrays hold n floats (16-byte aligned arrays take the float4 path); step counts from 1 (the value torch keeps in state['step']). */
int pnerf_adam_step(float *d_param, const float *d_grad, float *d_exp_avg, float *d_exp_avg_sq, int64_t n,
                    double lr, double beta1, double beta2, double eps, int64_t step, void *stream);
/* the same update for a list of tensors in ONE launch (per 24 tensors): each entry carries its own size, learning rate and step count,
 * so both of the reference's optimizers (MLP: 18 tensors at lr, points: 4 tensors at plr) are one call.  `tensors` is a HOST array. */
typedef struct pnerf_adam_tensor {
    float *param; const float *grad; float *exp_avg; float *exp_avg_sq;
    int64_t n; double lr; int64_t step;
} pnerf_adam_tensor;
int pnerf_adam_step_multi(const pnerf_adam_tensor *tensors, int count, double beta1, double beta2, double eps, void *stream);

/* ---- point initialisation: voxel down-sampling of a raw cloud (models/mvs/mvs_utils.py:537-561 construct_vox_points_closest,
 * called at run/train_ft.py:138-139).  Voxel of a point = floor((p - space_min) / vox_size) per axis (fp32), points outside
 * [0, r) are dropped and counted.  Outputs for the M occupied voxels in ascending (x, y, z) order (torch.unique(dim=0) order):
 * d_centroid [M,3] mean of the members (summed in point order), d_grid_idx [M,3], d_min_idx [M] = member closest to the centroid
 * (ties: lowest index).  All outputs are sized for n_points voxels; d_counts[0] = M, d_counts[1] = points outside. */
size_t pnerf_voxel_downsample_workspace_bytes(int64_t n_points, int rx, int ry, int rz);
int pnerf_voxel_downsample(const float *d_xyz, int64_t n_points, const float *space_min3_host, const float *vox_size3_host,
                           int rx, int ry, int rz, float *d_centroid, int32_t *d_grid_idx, int64_t *d_min_idx, int32_t *d_counts,
                           void *d_ws, size_t ws_bytes, void *stream);

/* ---- point initialisation: appearance of candidate points from GIVEN 2-D maps (MvsPointsModel.extract_2d
 * models/mvs/mvs_points_model.py:198-218 = homo_warp_nongrid / homo_warp_nongrid_occ models/mvs/mvs_utils.py:299-315,333-369 +
 * extract_from_2d_grid :411-421; called from query_embedding :233-238).  The maps (the source images and the feature pyramid of the
 * reference's FeatureNet) are INPUTS: the 2-D network itself is outside the hot-path scope.
 * d_cam_xyz [n,3]: the points in the frame of the camera `cam_vid`.  A view = (c2w of cam_vid, w2c of the view, the view's 3x3 intrinsic,
 * all row-major; has_w2c = 0 for the view that IS cam_vid: no transform, :302-305).  Pixel = ((p / p.z) @ K^T).xy; in-image test
 * 0 <= pixel <= (WD-1, HD-1) (depth_occ == 0) or on ceil(pixel) (depth_occ != 0), then for depth_occ != 0 the z-buffer test
 * z <= min(z over the in-image points of the same ceil-pixel) + tolerate.  Every map [C,H,W] of a view is sampled at the pixel scaled to
 * [-1,1] by (WD-1, HD-1) (bilinear, zeros outside, align_corners) into columns [out_col, out_col + C) of d_feats [n,feat_cols] or, with
 * is_color, of d_colors [n,color_cols]; rows of points that fail a view's test are zero in that view's columns.  d_mask [n_views,n]
 * (optional): the views' final masks. */
#define PNERF_EX2D_MAX_VIEWS 8
#define PNERF_EX2D_MAX_MAPS 32
typedef struct pnerf_view_desc {
    float c2w[16];          /* c2ws[:, cam_vid] */
    float w2c[16];          /* w2cs[:, vid] */
    float intrinsic[9];     /* intrinsics[:, vid] */
    int32_t has_w2c;
} pnerf_view_desc;
typedef struct pnerf_map_desc {
    const float *d_map;     /* [C,H,W] device: img_feats[lid][vid] */
    int32_t view;           /* index into the views array */
    int32_t C, H, W;
    int32_t out_col;        /* first column in d_feats (d_colors when is_color) */
    int32_t is_color;       /* layer 0 of the reference's pyramid = the image itself (:209-210) */
    int32_t first_of_view;  /* set by the library */
} pnerf_map_desc;
size_t pnerf_extract_2d_workspace_bytes(int64_t n_points, int n_views, int HD, int WD, int depth_occ);
int pnerf_extract_2d(const float *d_cam_xyz, int64_t n_points, const pnerf_view_desc *views, int n_views, const pnerf_map_desc *maps,
                     int n_maps, int HD, int WD, int depth_occ, float tolerate, float *d_feats, int feat_cols, float *d_colors,
                     int color_cols, uint8_t *d_mask, void *d_ws, size_t ws_bytes, void *stream);
/* the "dir" block of query_embedding (models/mvs/mvs_points_model.py:239-251): d_dirs [n, n_views, 3] = unit(p - cam_pos_cam[v]) (norm + 1e-6)
 * @ rot1^T (@ rot2^T when rot2 != NULL); cam_pos_cam_host [n_views,3] = the views' centres in cam_vid's frame, rot1 = c2ws[cam_vid][:3,:3],
 * rot2 = c2ws[ref_vid][:3,:3] unless pointdir_w. */
int pnerf_point_dirs(const float *d_cam_xyz, int64_t n_points, const float *cam_pos_cam_host, int n_views, const float *rot1_host9,
                     const float *rot2_host9, float *d_dirs, void *stream);

/* ---- point initialisation: from one depth map per view to the raw cloud (run/train_ft.py:96-146), csrc/depthfuse.hip.
 *
 * pnerf_depth_consistency: the geometric part of filter_by_masks_gpu (models/mvs/filter_utils.py:222-259 = the loop over
 * check_geometric_consistency_gpu :203-218 / reproject_with_depth_gpu :157-199) for ALL pairs of views in one launch.  d_depth [V,H,W] f32;
 * view_hw_host [V,2] i32 = every view's (H, W): the reference assumes one size, a view of another size -> PNERF_E_UNSUP.  d_pairs
 * [V,V,PNERF_DF_PAIR_FLOATS] f32, entry (r, s) for reference view r and source view s (the diagonal is not read), with
 * E_s E_r^-1 = [R_sr t_sr], E_r E_s^-1 = [R_rs t_rs] formed in float64 and rounded once:
 *   [0..8] K_s R_sr K_r^-1, [9..11] K_s t_sr, [12..20] K_r R_rs K_s^-1, [21..23] K_r t_rs, [24..26] row 2 of R_rs K_s^-1, [27] t_rs[2], rest 0.
 * Per reference pixel (x, y) with d = d_depth[r,y,x] and every s != r: (X, Y, Z) = d [0..8] (x, y, 1) + [9..11]; (x_s, y_s) = (X / Z, Y / Z);
 * d_s = the bilinear sample of view s there, coordinates clamped to the image (grid_sample align_corners, border: an out-of-image projection
 * is not rejected by itself); (X', Y', Z') = d_s [12..20] (x_s, y_s, 1) + [21..23]; d' = d_s [24..26] (x_s, y_s, 1) + [27]; the pair passes if
 * |(X' / Z', Y' / Z') - (x, y)| < 1 and |d' - d| / d < 0.01 (d == 0, NaN, inf fail).  d_geo_mask_sum [V,H,W] i32 = the number of passing s;
 * d_depth_avg [V,H,W] f32 = (sum of the passing d' in ascending s + d) / (count + 1).  No atomics: two calls give the same bits.
 * PNERF_E_INVAL: V < 1, H or W < 2, a null pointer; PNERF_E_UNSUP: views of different size, V > 65535, more than 2^31 - 257 pixels. */
#define PNERF_DF_PAIR_FLOATS 32
int pnerf_depth_consistency(const float *d_depth, const int32_t *view_hw_host, int V, const float *d_pairs, int32_t *d_geo_mask_sum,
                            float *d_depth_avg, void *stream);
/* pnerf_depth_fuse_select: the selection of filter_by_masks_gpu (models/mvs/filter_utils.py:259-291 with reassign_conf :294-297 and
 * range_mask_torch :146-154) on the dense maps above.  A pixel is kept if d_confidence [V,H,W] > depth_conf_thresh, d_points_mask [V,H,W] u8
 * != 0, (V > 1 only) d_geo_mask_sum >= geo_cnsst_num, and (ranges6_host != NULL) its world position lies in [ranges[0..2], ranges[3..5]].
 * Kept pixels are written in ascending (view, row, column) -- the order of the reference's boolean indexing, view after view:
 *   d_xyz_cam [n,3] = (d_cam_xyz[v,y,x,0], d_cam_xyz[v,y,x,1], d_depth_avg[v,y,x]) (x, y as given, not rescaled to the averaged depth),
 *   d_xyz_world [n,3] = [xyz_cam 1] @ d_inv_ext[v]^T (d_inv_ext [V,16]: the inverse extrinsics, row-major; k ascending, no FMA),
 *   d_conf_out [n] = the confidence, times conf_factor10_host[clamp(geo_mask_sum - geo_cnsst_num + 1, 1, 10) - 1] when that table is given
 *   (the host's 1 - 1 / 1.14869^k, k = 1..10: reassign_conf), d_view_id [n] i32 = v; *d_count = n (device).  All outputs are sized for
 *   V*H*W rows.  d_ws holds pnerf_depth_fuse_select_workspace_bytes(V, H, W) (0 for invalid sizes).  No atomics.
 * PNERF_E_INVAL: V < 1, H or W < 2, a null pointer other than the two host tables; PNERF_E_WS; PNERF_E_UNSUP: more than 2^31 - 257 pixels. */
size_t pnerf_depth_fuse_select_workspace_bytes(int V, int H, int W);
int pnerf_depth_fuse_select(const int32_t *d_geo_mask_sum, const float *d_depth_avg, const float *d_cam_xyz, const float *d_confidence,
                            const uint8_t *d_points_mask, const float *d_inv_ext, int V, int H, int W, float depth_conf_thresh,
                            int geo_cnsst_num, const float *conf_factor10_host, const float *ranges6_host, float *d_xyz_cam,
                            float *d_xyz_world, float *d_conf_out, int32_t *d_view_id, int32_t *d_count, void *d_ws, size_t ws_bytes,
                            void *stream);
/* pnerf_alpha_hull: the visual hull of alpha_masking (models/mvs/mvs_utils.py:573-607).  d_points [n,3] world positions, d_alphas [V,H,W] f32,
 * d_w2c [V,16], d_intrinsics [V,9] row-major.  Per view: c = [p 1] @ w2c^T, q = c @ K^T, pixel = floor(q.xy / q.z) clamped to the image
 * (NaN -> 0); m = alpha there, + 1 if use_range_mask != 0 and the unclamped pixel is outside the image (opt.alpha_range > 0 or
 * opt.inall_img == 0: such a view does not carve); the view passes if m > 0.1 and (near_far2_host != NULL) near_far2_host[0] <= c.z <=
 * near_far2_host[1] (the caller passes near - 1 and far).  d_mask [n] u8 = 1 where every view passes.
 * PNERF_E_INVAL: V, H or W < 1, n < 0, a null pointer other than near_far2_host while n > 0.  n == 0: nothing is enqueued. */
int pnerf_alpha_hull(const float *d_points, int64_t n_points, const float *d_alphas, const float *d_w2c, const float *d_intrinsics, int V,
                     int H, int W, int use_range_mask, const float *near_far2_host, uint8_t *d_mask, void *stream);

/* ---- point initialisation: from a cloud the user already has to per-view groups (run/train_ft.py:642-735, `--load_points 1/2/3`),
 * csrc/cloudinit.hip.
 *
 * pnerf_nearest_view: nearest_view (run/train_ft.py:39-48) without its 10 000-point slices and [10000,M,3] temporaries.  d_xyz [n,3],
 * d_campos [M,3] (camera centres), d_camdir [M,3] (centre rays) f32.  Per point p and camera (c, r): d = p - c,
 * s = |d| / 200 + (1.1 - dot(d, r) / (|d| + 1e-6)); d_cam_ind [n] i32 = the camera of the smallest s, ties to the lowest index (torch.argmin);
 * a NaN score never wins.  One thread per point, the cameras staged through LDS: any M.  The dot product is divided once (the reference
 * divides the three components) and |d| / 200 is |d| * 0.005f: the result is the float64 argmin wherever the runner-up is farther than the
 * reference's own fp32 rounding reaches (tests/cloudinit_case.py).  No atomics: two calls give the same bits.
 * PNERF_E_INVAL: M < 1, n < 0, a null pointer while n > 0.  n == 0: nothing is enqueued. */
int pnerf_nearest_view(const float *d_xyz, int64_t n, const float *d_campos, const float *d_camdir, int M, int32_t *d_cam_ind, void *stream);
/* pnerf_occupancy_merge: the `load_points == 3` merge (run/train_ft.py:657-669 over construct_vox_points_ind, models/mvs/mvs_utils.py:520-534):
 * the rows of cloud B [nb,3] whose cell holds no point of cloud A [na,3].  Cells are floor((x - space_min) / vox) per axis in fp32 (IEEE
 * divide), A's with vox_size_a3_host (the reference's scalar edge / res, :531 after :525) and B's with vox_size_b3_host ((space_max -
 * space_min) / res per axis, :530-531: the two can differ in the last bit); a cell outside [0, res)^3 holds no point of A, so such a row of B
 * is kept.  d_mask [nb] u8 = 1 where kept, d_kept_xyz [nb rows allocated] = the kept rows in their original order (the order of the
 * reference's boolean indexing), *d_count (device) = their number.  A res^3-bit map is set from A with an atomic OR (order-independent:
 * two calls give the same bits).  d_ws holds pnerf_occupancy_merge_workspace_bytes(nb, res): 0 when nb > 2^31 - 257 or res^3 bits exceed
 * that 32-bit addressing.  PNERF_E_INVAL: na or nb < 0, res < 1, a null pointer (d_a_xyz may be null when na == 0); PNERF_E_WS; PNERF_E_UNSUP
 * as for the workspace.  nb == 0: *d_count = 0, nothing else is touched. */
size_t pnerf_occupancy_merge_workspace_bytes(int64_t nb, int res);
int pnerf_occupancy_merge(const float *d_a_xyz, int64_t na, const float *d_b_xyz, int64_t nb, const float *space_min3_host,
                          const float *vox_size_a3_host, const float *vox_size_b3_host, int res, float *d_kept_xyz, int32_t *d_count,
                          uint8_t *d_mask, void *d_ws, size_t ws_bytes, void *stream);
/* pnerf_crop_ranges: the crop to opt.ranges (run/train_ft.py:675-680): the rows with ranges6_host[0..2] <= p <= ranges6_host[3..5] (NaN
 * fails), outputs and errors as pnerf_occupancy_merge. */
size_t pnerf_crop_ranges_workspace_bytes(int64_t n);
int pnerf_crop_ranges(const float *d_xyz, int64_t n, const float *ranges6_host, float *d_kept_xyz, int32_t *d_count, uint8_t *d_mask, void *d_ws,
                      size_t ws_bytes, void *stream);
/* pnerf_group_by_view: torch.unique(cam_ind) and the per-view boolean indexing of run/train_ft.py:707-710 as one stable counting sort.
 * d_cam_ind [n] i32 in [0, M).  d_order [n] i64 = the permutation that lists the points by ascending view, original order inside a view;
 * d_offsets [M+1] i64: view v owns d_order[d_offsets[v] .. d_offsets[v+1]).  An entry outside [0, M) is left out: d_offsets[M] < n and the
 * tail of d_order is -1.  No atomic decides a position (ranks inside 1024-point chunks, one scan over the [M, chunks] counts): two calls give
 * the same bits.  d_ws holds pnerf_group_by_view_workspace_bytes(n, M): 0 when n > 2^31 - 257 or M * ceil(n / 1024) exceeds it.
 * PNERF_E_INVAL: n < 0, M < 1, a null pointer; PNERF_E_WS; PNERF_E_UNSUP as for the workspace.  n == 0: d_offsets = 0. */
size_t pnerf_group_by_view_workspace_bytes(int64_t n, int M);
int pnerf_group_by_view(const int32_t *d_cam_ind, int64_t n, int M, int64_t *d_order, int64_t *d_offsets, void *d_ws, size_t ws_bytes,
                        void *stream);

/* ---- point initialisation: from images to one depth map per view (the pretrained MVSNet of every per-scene script, manual_depth_view=1),
 * csrc/mvsdepth.hip.  The 2-D and 3-D convolutions stay with the host framework; these are the stages between and behind them.
 *
 * pnerf_mvs_cost_volume: homo_warping (models/depth_estimators/module.py:36-70) for all views and the variance of mvsnet.py:110-122 in one
 * pass, no warped volume.  d_feats [n_feat_sets, V, 32, h, w] f32 (n_feat_sets == B, or 1: every batch item reads the same maps, as
 * gen_points' expanded images give, models/mvs/mvs_points_model.py:306); d_proj [B, V, 3, 4] f32 = rot | trans of proj[:, :3]; d_depth_values
 * [B, D].  d_volume [B, 32, D, h, w] f32 (the layout CostRegNet.conv0 takes) = sum_v s^2 / V - (sum_v s / V)^2, v ascending, s the
 * bilinear zero-padded sample of view v at  p = rot (x, y, 1) depth + trans,  g = (p.x / p.z) / ((w - 1) / 2) - 1 (y with h), un-normalised
 * as F.grid_sample does: align_corners == 0 (the reference's call under torch >= 1.3): ((g + 1) size - 1) / 2; != 0: (g + 1) / 2 (size - 1).
 * A position without a tap inside the map -- NaN, infinite, far outside: planes at or behind a source camera -- contributes exactly 0;
 * every tap is bounds-checked after the conversion, nothing outside a map is read.  The maps are transposed to channels-last in d_ws
 * (pnerf_mvs_cost_volume_workspace_bytes(n_feat_sets, V, h, w); 0 for invalid sizes).  fp32, no atomics: two calls give the same bits.
 * PNERF_E_INVAL: B, V or D < 1, h or w < 2, n_feat_sets not 1 or B, a null pointer; PNERF_E_UNSUP: C != 32, B or 2 D or n_feat_sets V >
 * 65535, more than 2^31 - 257 pixels per map; PNERF_E_WS. */
size_t pnerf_mvs_cost_volume_workspace_bytes(int n_feat_sets, int V, int h, int w);
int pnerf_mvs_cost_volume(const float *d_feats, int n_feat_sets, const float *d_proj, const float *d_depth_values, int B, int V, int C, int D,
                          int h, int w, int align_corners, float *d_volume, void *d_ws, size_t ws_bytes, void *stream);
/* pnerf_mvs_depth_regress: mvsnet.py:127-136 (F.softmax over D, depth_regression module.py:73-78 twice, F.pad (1, 2) + avg_pool3d(4) * 4 +
 * gather) per pixel in one pass over the logits plus four re-reads.  d_cost_reg [B, D, h, w] f32 (the regulariser's logits), d_depth_values
 * [B, D].  With p = softmax over D:  d_depth [B, h, w] = sum p depth_values;  idx = trunc(sum p d) clamped to [0, D - 1] (NaN -> 0);
 * d_confidence [B, h, w] = p[idx - 1] + p[idx] + p[idx + 1] + p[idx + 2], zeros outside [0, D - 1];  d_prob_volume [B, D, h, w] = p when not
 * NULL (a second pass; nothing is staged otherwise).  A NaN or +inf logit gives NaN outputs at its pixel and indexes nothing out of range.
 * PNERF_E_INVAL: B, D, h or w < 1, a null pointer other than d_prob_volume; PNERF_E_UNSUP: B > 65535, more than 2^31 - 257 pixels. */
int pnerf_mvs_depth_regress(const float *d_cost_reg, const float *d_depth_values, int B, int D, int h, int w, float *d_depth,
                            float *d_confidence, float *d_prob_volume, void *stream);
/* pnerf_depth_to_cam_points: the tail of gen_points for one view (models/mvs/mvs_points_model.py:329-337, gau_single_sampler :152-157 with
 * manual_std_depth = 0, depth2point :171-182, ndc_2_cam models/mvs/mvs_utils.py:92-98).  d_depth_lr / d_conf_lr [h, w] f32.  Per output
 * pixel (X, Y) of [H, W]: the source pixel of F.interpolate(mode='nearest') (min(floor(dst * ((float)in / out)), in - 1) per axis);
 * d_confidence [H, W] = the confidence there; d = the depth there; d_mask [H, W] u8 = near <= d <= far; ndc = clamp((d - near) / (far - near),
 * 0, 1) (the mask does not undo the clamp); z = ndc (far - near) + near; d_cam_xyz [H, W, 3] = ((X / (W - 1)) (W - 1) z, (Y / (H - 1)) (H - 1)
 * z, z) @ inv_kt9_host, the host's row-major inverse of the transposed intrinsics.
 * PNERF_E_INVAL: h or w < 1, H or W < 2, a null pointer; PNERF_E_UNSUP: more than (2^31 - 257) / 3 output pixels. */
int pnerf_depth_to_cam_points(const float *d_depth_lr, const float *d_conf_lr, int h, int w, int H, int W, float near, float far,
                              const float *inv_kt9_host, float *d_cam_xyz, float *d_confidence, uint8_t *d_mask, void *stream);

/* ---- evaluation scores of a rendered image against its ground truth (run/evaluate.py:55-61,76 report_metrics: compare_psnr,
 * compare_ssim(gt, img, 11, multichannel=True) and mean_squared_error over the PNGs that utils/visualizer.py:58-59 wrote).
 * d_img / d_gt [H,W,3] f32.  quantize8 != 0 first maps every pixel of both images through that PNG round trip,
 * q = (float)(uint8)(clip(x, 0, 1) * 255.f) / 255.f (the conversion truncates; the division is fp32).  d_out4 (4 doubles):
 *   [0]     sum of squared differences over all H*W*3 elements      (mse = [0] / (H*W*3); psnr = 10 log10(1 / mse); rmse = sqrt(mse))
 *   [1..3]  per channel, the sum over the (H-win+1) x (W-win+1) windows fully inside the image of skimage's SSIM map in its uniform-filter
 *           form (window means, covariance scaled by NP/(NP-1), C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2); skimage's reflected
 *           border is cropped before its mean, so  ssim = ([1] + [2] + [3]) / (3 (H-win+1)(W-win+1)).  The reference's call passes float
 *           images and no data_range to skimage <= 0.18, which makes data_range = 2 (while its PSNR takes 1).
 * All arithmetic is fp64 on the fp32 pixels; no atomics: two calls on the same inputs give the same bits.  PNERF_E_INVAL: null pointer,
 * win even or < 3, H < win or W < win (skimage raises there), data_range <= 0; PNERF_E_WS: workspace too small; PNERF_E_UNSUP: win > 25
 * (the tile and its halo no longer fit the LDS) or an image of more than 65 535 x 16 window rows / 2^31 - 1 tiles of 16 x 16 windows. */
size_t pnerf_image_metrics_workspace_bytes(int H, int W, int win);     /* run/evaluate.py:55-61,76; utils/visualizer.py:58-59; 0 for invalid or unsupported sizes */
int pnerf_image_metrics(const float *d_img, const float *d_gt, int H, int W, int win, double data_range, int quantize8, double *d_out4,
                        void *d_ws, size_t ws_bytes, void *stream);

/* ---- the probe pass of the point-growing step (run/train_ft.py:417-530 probe_hole) on the renderer's dense results.
 *
 * pnerf_probe_rays: the `opt.prob == 1` outputs of NeuralPointsRayMarching.forward (models/neural_points_volumetric_model.py:331-352) for
 * all R submitted rays from the DENSE tensors of pnerf_query / pnerf_render_forward (d_opacity [R,SR], d_weight [R,SR,K], d_sample_loc
 * [R,SR,3], d_sample_pidx [R,SR,K], d_ray_hit [R]); no [R'',SR,K] copy is read or written.  For a ray with d_ray_hit[r] > 0, with s* the
 * LOWEST sample index among the maxima of d_opacity[r, 0 .. SR-1] and p_k = max(d_sample_pidx[r, s*, k], 0) (an empty slot reads point 0,
 * models/neural_points/neural_points.py:708), w_k = d_weight[r, s*, k] * min(max(conf[p_k], 1e-4), 1)
 * (gradient_clamp, models/aggregators/point_aggregators.py:722-724):
 *   d_max_opacity [R]    ray_max_shading_opacity = d_opacity[r, s*]        d_loc3 [R,3]   ray_max_sample_loc_w = d_sample_loc[r, s*, :]
 *   d_far_dist    [R]    ray_max_far_dist = min_k |xyz[p_k] - loc| over ALL K slots (point 0 of the empty ones included, as in the reference)
 *   d_avg_color3 [R,3], d_avg_dir3 [R,3], d_avg_conf [R], d_avg_emb32 [R,32]    shading_avg_* = sum_k w_k row_k, fp32
 * A ray with d_ray_hit[r] <= 0 gets zeros in all seven (fill_invalid's zero fill, :121-122); its input rows are not read.
 * PNERF_E_INVAL: K outside 1..PNERF_MAX_K, SR <= 0, R < 0, a null pointer; PNERF_E_UNSUP: pts->feat_dim != 32.  R == 0: nothing is enqueued. */
int pnerf_probe_rays(const pnerf_points *pts, const float *d_opacity, const float *d_weight, const float *d_sample_loc,
                     const int32_t *d_sample_pidx, const int32_t *d_ray_hit, int R, int SR, int K, float *d_max_opacity, float *d_loc3,
                     float *d_far_dist, float *d_avg_color3, float *d_avg_dir3, float *d_avg_conf, float *d_avg_emb32, void *stream);
/* pnerf_probe_hole_mask: the candidate rule of probe_hole per pixel of an [H,W] view (run/train_ft.py:489-500 with bloat_inds :532-540):
 *   hit = d_ray_mask > 0;  miss = !hit && |d_gt - bg| > 0.002 && d_edge;  near = any miss in the 3 x 3 neighborhood clamped to the image;
 *   far_thresh > 0: near |= hit && d_far_dist > far_thresh && |d_gt - d_raycolor| < 0.1;   d_flags = hit && near && d_max_opacity > opacity_thresh
 * d_ray_mask [H,W] i8, d_max_opacity / d_far_dist [H,W] f32, d_raycolor / d_gt [H,W,3] f32, d_edge [H,W] u8 (pixels the view has rays
 * for), bg3_host: 3 floats on the host, d_flags [H,W] i32 0/1 -- the input of pnerf_compact_valid, which turns it into the ascending
 * row-major candidate list with its count on the device.  The norms are sqrtf of the fp32 sum of squares.  PNERF_E_INVAL: H or W <= 0,
 * a null pointer. */
int pnerf_probe_hole_mask(const int8_t *d_ray_mask, const float *d_max_opacity, const float *d_far_dist, const float *d_raycolor,
                          const float *d_gt, const uint8_t *d_edge, const float *bg3_host, int H, int W, float opacity_thresh,
                          float far_thresh, int32_t *d_flags, void *stream);

/* ---- per-ray depth and opacity maps of a render-only pass, on the renderer's dense results.
 *
 * pnerf_ray_geometry: the depth the reference's `is_compute_depth` was meant to return (models/neural_points_volumetric_model.py:318-322:
 * sum_s blend_weight ray_ts / (sum_s blend_weight + 1e-6); `ray_ts` is undefined there), with the camera-z depth of a sample in the place
 * of ray_ts, plus the accumulated opacity and the median depth, from the DENSE tensors of pnerf_query / pnerf_render_forward (d_sample_loc
 * [R,SR,3], d_sample_nn [R,SR], d_ray_hit [R], d_opacity [R,SR], d_blend_w [R,SR]; opacity, blend weight and transmittance are ray_march's,
 * models/rendering/diff_ray_marching.py:508-554, read back and not recomputed).  For a ray with d_ray_hit[r] > 0, over the slots s < SR:
 *   z_s = ((d_sample_loc[r,s] - cam->campos) @ cam->camrot)[2],  valid_s = d_sample_nn[r,s] > 0,
 *   T_s = prod_{j <= s} (1 - d_opacity[r,j] + 1e-10f)  (a wave-inclusive product per 64 slots times the product carried in front, as the ray march);
 *   d_acc [R] = sum_s d_blend_w[r,s]      d_depth_sum [R] = sum over the valid s of d_blend_w[r,s] z_s (an empty slot's position is not read)
 *   d_depth [R] = d_depth_sum / (d_acc + 1e-6f)
 *   d_median_slot [R] i32 = the lowest valid s with T_s < 0.5, or -1;   d_median_depth [R] = z there, or 0
 * A ray with d_ray_hit[r] <= 0 gets zeros and -1; its rows are not read.  The sums are per-lane partial sums over the 64-slot chunks met in
 * one xor butterfly; no atomics: two calls give the same bits.  Of `cam` only campos and camrot are read.
 * PNERF_E_INVAL: R < 0, SR < 1, a null pointer (cam always; the arrays while R > 0).  R == 0: nothing is enqueued. */
int pnerf_ray_geometry(const pnerf_camera *cam, const float *d_sample_loc, const int32_t *d_sample_nn, const int32_t *d_ray_hit,
                       const float *d_opacity, const float *d_blend_w, int R, int SR, float *d_acc, float *d_depth_sum, float *d_depth,
                       float *d_median_depth, int32_t *d_median_slot, void *stream);
/* pnerf_geometry_canvas: the per-pixel fill of the three maps for one chunk of n_rays rays (no reference counterpart; the reference's test
 * loop scatters its visuals by pixel_idx, run/train_ft.py:316-320): ray i goes to pixel (px, py) = d_pixel_idx[i] ([n_rays,2] i32) of the
 * three [H,W] canvases, canvas[py * W + px] = d_depth / d_median_depth / d_acc [i], or 0 where d_ray_mask[i] <= 0 ([n_rays] i8; NULL: every
 * ray counts as a hit).  No other pixel is touched.  A pixel outside the image writes nothing and stores PNERF_E_INVAL in *d_flag (i32 on
 * the device; zero it once, before the first chunk of an image, and read it with the canvases: the call itself never reads it, so the
 * chunks of an image are enqueued without a host read in between).  PNERF_E_INVAL from the call: n_rays < 0, H or W <= 0, a null pointer
 * other than d_ray_mask while n_rays > 0. */
int pnerf_geometry_canvas(const int32_t *d_pixel_idx, const int8_t *d_ray_mask, const float *d_depth, const float *d_median_depth,
                          const float *d_acc, int n_rays, int H, int W, float *d_depth_canvas, float *d_median_canvas, float *d_acc_canvas,
                          int32_t *d_flag, void *stream);

/* ---- point attribute maps, picking and image-to-point lifting of a render-only pass, on the renderer's dense results (no reference
 * counterpart).  One linear operator A and its adjoint on d_blend_w [R,SR], d_weight [R,SR,K], d_sample_pidx [R,SR,K], d_ray_hit [R] as
 * pnerf_query / pnerf_render_forward (or _cut) left them.  For ray r, slot s < SR, neighbor slot k < K:
 *   p = d_sample_pidx[r,s,k];   g[r,s,k] = d_blend_w[r,s] * d_weight[r,s,k] (one fp32 multiply) if 0 <= p < n_points, else 0.
 * An index outside [0, n_points) -- the empty slot -1 included, which here does NOT read point 0 -- contributes nothing and is never
 * dereferenced; the weight and index rows of a sample with d_blend_w == 0 are not read.  d_weight is the normalised distance weight (it sums
 * to 1 over the occupied slots of a valid sample: sum_k g = d_blend_w); the confidence factor of the density is NOT part of g.  A ray with
 * d_ray_hit[r] <= 0 produces zeros / -1 (pnerf_ray_attributes) or adds nothing (pnerf_lift_to_points); none of its rows are read.
 *
 * pnerf_ray_attributes (A and the pick), d_attr [n_points,C] f32:
 *   d_attr_sum [R,C] = sum_{s,k} g[r,s,k] d_attr[p,c], fp32, in an order that depends on (SR, K, C) only;
 *   d_top_flat [R] i32 = the LOWEST flat index s*K + k among the maxima of g[r,:,:] -- the largest single (sample, slot) entry, not a
 *   per-point sum over the ray's samples --, d_top_point [R] i32 = d_sample_pidx there, d_top_contrib [R] = g there; a hit ray whose
 *   largest g is not > 0 gets -1, -1, 0.  No atomics: two calls give the same bits.  C == 0 runs the pick only.
 * pnerf_lift_to_points (A^T), d_values [R,C] f32, d_ray_factor [R] f32 (NULL: 1):
 *   d_point_sum [n_points,C] += g[r,s,k] m[r] d_values[r,c],   d_point_mass [n_points] += g[r,s,k] m[r]   over every entry that addresses p.
 *   The call ADDS into the caller's accumulators (several views add up; the caller zeroes them) with fp32 atomicAdd on global memory, the
 *   kind of the backward's point gradients: the sums depend on the order of arrival and are NOT bit-reproducible.
 * PNERF_E_INVAL: K outside 1..PNERF_MAX_K, SR <= 0, R < 0, n_points <= 0, C < 0, a null pointer (while R > 0; d_ray_factor may be null);
 * PNERF_E_UNSUP: C > 256 (attributes), C > 8 (lifting).  R == 0: nothing is enqueued.  No allocation, no host read. */
int pnerf_ray_attributes(const float *d_attr, int32_t n_points, int C,
        const float *d_blend_w, const float *d_weight, const int32_t *d_sample_pidx, const int32_t *d_ray_hit,
        int R, int SR, int K,
        float *d_attr_sum /*[R,C]; may be NULL iff C == 0*/, int32_t *d_top_point, int32_t *d_top_flat, float *d_top_contrib /*[R] each*/,
        void *stream);
int pnerf_lift_to_points(const float *d_values /*[R,C] or NULL iff C == 0*/, int C, const float *d_ray_factor /*[R] or NULL*/,
        const float *d_blend_w, const float *d_weight, const int32_t *d_sample_pidx, const int32_t *d_ray_hit,
        int R, int SR, int K, int32_t n_points,
        float *d_point_sum /*[n_points,C] or NULL iff C == 0*/, float *d_point_mass /*[n_points]*/, void *stream);

/* ---- diagnostics: ONE v_mfma_f32_32x32x16_f16, D = A B with caller-built fragments: d_a / d_b [64 lanes][8] f16 (lane l holds
 * A[l & 31][8 (l >> 5) .. + 7] resp. B[8 (l >> 5) .. + 7][l & 31]), d_out [64 lanes][16] f32 (register r of lane l =
 * D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31]).  The tests pin with it the fragment layout and the un-flushed handling of f16
 * subnormal inputs that the two-plane GEMMs of the aggregator (csrc/f16x3.h) rely on. */
int pnerf_debug_mfma_f16(const void *d_a, const void *d_b, float *d_out, void *stream);
/* ONE tile GEMM in the mixed format of csrc/mixq.h (f16 h.h + e4m3 cross terms): d_out [64][256] = d_x [64][K] d_w[256][K]^T, K in {256, 272, 288}
 * (columns >= 256 run the classic three f16 products), through the tile's LDS format and a packed weight image written to d_img
 * (>= pnerf_mlp_packed_bytes()).  Tests measure it against float64 on the device and against the numpy restatement of the format on the host
 * emulator.  The arithmetic stands behind the nn.Linear layers of models/aggregators/point_aggregators.py:286-344. */
int pnerf_debug_mix_gemm(const float *d_w, int K, const float *d_x, void *d_img, float *d_out, void *stream);
/* measurement aid of bench.py (roofline.peak_measured of the matrix-pipe entries; no reference counterpart): `iters` x 32 register-resident
 * v_mfma_f32_32x32x16_f16 per wave on 2 x 256-thread workgroups per CU, operands all zero (mode 0), one constant (1) or pseudo-random f16 in
 * +-[0.5, 1) (2: they toggle like a GEMM's fragments).  Asynchronous on `stream`; the caller times it with events.  *flop_out = the flops the
 * launch executes; d_scratch: >= 256 floats of device memory (never written in practice). */
int pnerf_debug_mfma_rate(int mode, int iters, float *d_scratch, double *flop_out, void *stream);
/* the counter-based uniforms of the jittered ray sampling (pnerf_query with jitter > 0 draws U[r * D + d] = uniform(seed, r * D + d)):
 * d_out[i] = uniform(seed, first + i) in [0, 1).  With these the jittered samples are a deterministic function of the inputs and
 * equal the reference's near_far_linear_ray_generation (diff_ray_marching.py:369-385, CPU) fed the same numbers, bit for bit. */
int pnerf_debug_uniform(uint64_t seed, uint64_t first, int64_t n, float *d_out, void *stream);
/* the two-plane split of csrc/f16x3.h on n floats (n even): d_h / d_m [n] f16 (high plane: round toward zero; residual plane: round to
 * nearest of x - h); sat != 0 clamps to the f16 range first (the gradient form).  Tests compare it bit for bit with the numpy restatement. */
int pnerf_debug_split(const float *d_x, int64_t n, void *d_h, void *d_m, int sat, void *stream);
/* the positional encoding the aggregator kernels evaluate (csrc/f16x3.h pn_pe_octaves; reference models/helpers/networks.py:175-190):
 * d_out[i][f] = {sin(x_i 2^f), cos(x_i 2^f)}, f < nfreq <= 5, d_out [n][nfreq][2] f32.  Tests measure it against float64 for |x| up to
 * thousands (trained embeddings are not confined to the initialisation's (-0.5, 0.5)). */
int pnerf_debug_pe(const float *d_x, int64_t n, int nfreq, float *d_out, void *stream);

/* ---- per-kernel timing (HIP events recorded on the launch stream; off by default) --------------- */
int pnerf_prof_enable(int on);
int pnerf_prof_kernel_count(void);
const char *pnerf_prof_kernel_name(int id);
/* synchronous: device is synchronised; totals of every launch recorded since the last collect */
int pnerf_prof_collect(double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* PNERF_H */
