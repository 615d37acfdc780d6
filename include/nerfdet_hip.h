/*
 * nerfdet_hip.h -- C ABI of libnerfdet_hip.so: the MI355X (gfx950) implementation of the
 * NeRF-Det volumetric hot path.
 *
 * The reference has no FFI layer on this path (it is pure PyTorch Python); the drop-in boundary
 * is the set of module-level Python callables listed in SURVEY.md section 8(b).  Every entry
 * point below states which reference callable (file:line under the reference tree) it replaces.
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the parameter name ends in _host;
 *   - fp32 everywhere on the data path, int64 for counts / indices (as the reference);
 *   - caller allocates every output; the library allocates nothing and keeps no state
 *     between calls (re-entrant; one process per GPU);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); work is only enqueued,
 *     never synchronised;
 *   - return value: 0 on success, negative NDET_E_* otherwise; ndet_last_error() gives a
 *     thread-local message.  The Python mirror turns these into the exceptions the reference
 *     raises (AssertionError / ValueError).
 */
#ifndef NERFDET_HIP_H
#define NERFDET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDET_OK 0
#define NDET_E_INVALID (-1)     /* bad argument (null pointer, non-positive size) */
#define NDET_E_UNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define NDET_E_LAUNCH (-3)      /* hipLaunch / runtime failure */

#define NDET_LAYOUT_CN 0 /* (C, N): the reference's (C,X,Y,Z) contiguous layout */
#define NDET_LAYOUT_NC 1 /* (N, C): channels-last (NDHWC), the native layout of this library */

int ndet_version(void);
const char* ndet_last_error(void);

/* A2. Voxel lower-corner lattice. Replaces get_points(), mmdet3d/models/detectors/nerfdet.py:380-390.
 * points: (3, nx*ny*nz) fp32, z fastest.  voxel_size_host/origin_host: 3 floats each, HOST memory.
 * Same fp32 operation order as the reference: idx*vs + (origin - n/2*vs), un-fused. */
int ndet_get_points(float* points, int nx, int ny, int nz, const float* voxel_size_host,
                    const float* origin_host, void* stream);

/* Layout helper: (n, c, hw) -> (n, hw, c).  The reference keeps feature maps NCHW; the fused kernels
 * want one pixel's channels contiguous (SURVEY.md section 7 "Layout").  No reference counterpart. */
int ndet_nchw_to_nhwc(const float* src, float* dst, int n, int c, int hw, void* stream);

/* Measurement aid: dst[i] = src[i], one non-temporal 16-byte access per thread.  Its rate (2 * 4 * n_floats / time) is the
 * empirical HBM ceiling bench.py prices the gather kernels against, next to the 8 TB/s specification (SURVEY.md 8d "the builder must
 * also report an empirical copy-kernel ceiling"; the reference's harness has no counterpart, tools/benchmark.py:63-89 times the model only).
 * Pointers 16-byte aligned, n_floats % 4 == 0. */
int ndet_hbm_copy(const float* src, float* dst, int64_t n_floats, void* stream);

/* A3 (exact API form). Replaces backproject(), nerfdet.py:393-420 (depth=None).
 * features: element (v,c,y,x) at v*sv + c*sc + y*sy + x*sx (floats) -- any layout.
 * points (3,N); projection (n_views,3,4).  Outputs the reference's materialised tensors:
 * volume (n_views, C, N) fp32 (zero where invalid) and valid (n_views, N) uint8 0/1. */
int ndet_backproject(const float* features, int n_views, int C, int h, int w,
                     int64_t sv, int64_t sc, int64_t sy, int64_t sx,
                     const float* points, int N, const float* projection,
                     float* volume, uint8_t* valid, void* stream);

/* A3+A4 (+A6 gating) fused -- the inference hot kernel.  Replaces backproject() followed by the view
 * aggregation of nerfdet.py:171-176 and, when alpha != NULL, the gating of nerfdet.py:259-261, without
 * materialising the (n_views,C,N) volume.
 * features_nhwc: element (v,y,x,c) at v*view_pitch + y*row_pitch + x*C + c (floats); C % 4 == 0, C <= 1024.
 * alpha: NULL or (N) fp32.  out: mean (or alpha*mean) in `out_layout`; count: (N) int64 view count. */
int ndet_backproject_aggregate(const float* features_nhwc, int n_views, int C, int h, int w,
                               int64_t view_pitch, int64_t row_pitch,
                               const float* points, int N, const float* projection,
                               const float* alpha, float* out, int out_layout, int64_t* count,
                               void* stream);

/* A5. Per-voxel NeRF conditioning vector.  Replaces nerfdet.py:234-253 (image mode) with the algebraic
 * identity mapping(volume)[v] == mapped_map[v,y,x] where the view sees the voxel and == bias where it
 * does not.
 * mapped_nhwc: Linear(C->cm)(features), element (v,y,x,c) at v*mview_pitch + y*mrow_pitch + x*cm + c; cm <= 61.
 * bias: (cm) the Linear's bias.  rgb: de-normalised images, element (v,c,y,x) at v*rsv + c*rsc + y*rsy + x
 * (3 channels, H x W).  projection: stride-4 matrices (validity + count), rgb_projection: stride-1 matrices.
 * global_feat: (N, 2*(3+cm)) fp32, channels INTERLEAVED [mean_0,cov_0,mean_1,cov_1,...] with channel order
 * [rgb0,rgb1,rgb2,m0..m(cm-1)] -- the effective layout of the reference's cat(dim=1)+view (nerfdet.py:251-253). */
int ndet_density_features(const float* mapped_nhwc, int n_views, int cm, int h, int w,
                          int64_t mview_pitch, int64_t mrow_pitch, const float* bias,
                          const float* rgb, int H, int W, int64_t rsv, int64_t rsc, int64_t rsy,
                          const float* points, int N, const float* projection, const float* rgb_projection,
                          float* global_feat, void* stream);

/* A5, packed form (the inference path's kernel): same statement, inputs and output layout as ndet_density_features --
 * nerfdet.py:234-253 -- for cm % 4 == 0 and n_views <= 128: channel quads per lane, 64/(cm/4+1) voxels per wavefront, both
 * projections of a (voxel, view) pair evaluated once, only the views that see the voxel are walked, and the variance uses the
 * shifted one-pass form (equal to the reference's two-pass sum up to fp32 rounding, not bit-equal). */
int ndet_density_features_packed(const float* mapped_nhwc, int n_views, int cm, int h, int w,
                                 int64_t mview_pitch, int64_t mrow_pitch, const float* bias,
                                 const float* rgb, int H, int W, int64_t rsv, int64_t rsc, int64_t rsy,
                                 const float* points, int N, const float* projection,
                                 const float* rgb_projection, float* global_feat, void* stream);

/* ---- depth-gated backprojection (RGB-D scenes): nerfdet.py:404-411 ----
 * With a per-view depth map D, the reference's backproject() counts view v as seeing voxel n only where the ordinary test holds
 * (pixel in bounds after round(), z > 0) AND  D'[v,y,x] - voxel_size[2] < z < D'[v,y,x] + voxel_size[2]  (both strict), with
 * z = the third row of P.[p;1] (the `d` of every projection here) and D' = F.interpolate(D, (h, w), bilinear, align_corners=False)
 * resized to the map the projection indexes.  The arithmetic follows PyTorch's promotion: dtype 0 (float32 D): D' - band in
 * float32 with band rounded to float32; dtype 1 (float64 D): in float64, z widened exactly.  Everything downstream of the
 * validity (counts, means, the bias fill of unseen views, variance, gradients) is the ungated statement over the gated mask.
 *
 * NdetDepthGate, one block per call (same style as NdetConvArgs):
 *   size            sizeof(NdetDepthGate); any other value is rejected (NDET_E_INVALID).
 *   dtype           0 = float32, 1 = float64 (element type of depth_f / depth_r).
 *   n_views         views of both maps; must equal the call's n_views.
 *   depth_f, h, w   D resized to the projection's map (the feature map, or the image for ndet_backproject_gated on images);
 *                   element (v,y,x) at v*f_view_pitch + y*f_row_pitch + x (elements); h, w must equal the call's.
 *   depth_r, H, W   D resized to the full-resolution image (the stride-1 projection of the density features); read by
 *                   ndet_density_features*_gated only, NULL / 0 elsewhere.
 *   band            voxel_size[2]: finite, > 0.
 */
typedef struct NdetDepthGate {
    int32_t size;
    int32_t dtype;
    int32_t n_views;
    int32_t h, w;
    int32_t H, W;
    const void* depth_f;
    int64_t f_view_pitch, f_row_pitch;
    const void* depth_r;
    int64_t r_view_pitch, r_row_pitch;
    double band;
} NdetDepthGate;

/* D' of nerfdet.py:405 for one scene in one launch: depth (n_views, Hd, Wd), element (v,y,x) at v*sv + y*sy + x, of `dtype`
 * (0 float32, 1 float64) -> out_f (n_views, h, w) and, when out_r != NULL, out_r (n_views, H, W), both contiguous, same dtype.
 * F.interpolate(mode="bilinear", align_corners=False) in the map's dtype: src = max((dst + 0.5) * (in / out) - 0.5, 0),
 * i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1, out = ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11) for an
 * output with H + W > 128, ((ly0 lx0) v00 + (ly0 lx1) v01 + (ly1 lx0) v10) + (ly1 lx1) v11 (left to right) for a smaller one -- the two
 * paths of PyTorch's CPU kernel, bit-equal to it at integer ratios; at other ratios within a few ulp. */
int ndet_depth_resize(const void* depth, int dtype, int n_views, int Hd, int Wd, int64_t sv, int64_t sy,
                      void* out_f, int h, int w, void* out_r, int H, int W, void* stream);

/* ndet_backproject with the depth gate of nerfdet.py:404-411 (gate->depth_f at the features' h x w). */
int ndet_backproject_gated(const float* features, int n_views, int C, int h, int w,
                           int64_t sv, int64_t sc, int64_t sy, int64_t sx,
                           const float* points, int N, const float* projection,
                           float* volume, uint8_t* valid, const NdetDepthGate* gate, void* stream);

/* ndet_backproject_aggregate with the depth gate of nerfdet.py:404-411 (gate->depth_f at the features' h x w): gated-out views
 * are dropped before the row gather. */
int ndet_backproject_aggregate_gated(const float* features_nhwc, int n_views, int C, int h, int w,
                                     int64_t view_pitch, int64_t row_pitch,
                                     const float* points, int N, const float* projection,
                                     const float* alpha, float* out, int out_layout, int64_t* count,
                                     const NdetDepthGate* gate, void* stream);

/* ndet_density_features with the depth gate of nerfdet.py:404-411 on both projections: the stride-4 one against gate->depth_f
 * (h x w), the stride-1 one against gate->depth_r (H x W), as the reference's two backproject() calls (nerfdet.py:164-169, 204-210). */
int ndet_density_features_gated(const float* mapped_nhwc, int n_views, int cm, int h, int w,
                                int64_t mview_pitch, int64_t mrow_pitch, const float* bias,
                                const float* rgb, int H, int W, int64_t rsv, int64_t rsc, int64_t rsy,
                                const float* points, int N, const float* projection, const float* rgb_projection,
                                float* global_feat, const NdetDepthGate* gate, void* stream);

/* ndet_density_features_packed with the depth gate of nerfdet.py:404-411, maps as in ndet_density_features_gated. */
int ndet_density_features_packed_gated(const float* mapped_nhwc, int n_views, int cm, int h, int w,
                                       int64_t mview_pitch, int64_t mrow_pitch, const float* bias,
                                       const float* rgb, int H, int W, int64_t rsv, int64_t rsc, int64_t rsy,
                                       const float* points, int N, const float* projection,
                                       const float* rgb_projection, float* global_feat, const NdetDepthGate* gate, void* stream);

/* Streaming scenes: one scene's views arrive in chunks (nerf-det_amd/streaming.py).  The state holds what K1 and K2 keep of the views
 * seen so far; the finishes turn it into K2's conditioning rows and K1's gated volume at any time and leave it unchanged.
 *
 * NdetSceneAccum, one block per call (same style as NdetConvArgs / NdetDepthGate):
 *   size          sizeof(NdetSceneAccum); any other value is rejected (NDET_E_INVALID).
 *   N, C, cm      voxels, feature channels (multiple of 4, <= 1024), mapped channels (multiple of 4, <= 128).
 *   n_views       views accumulated so far (the scene's total); read by the finishes only.
 *   k1_sum        (N, k1_pitch) fp32: per voxel the running sum of the C-float feature rows of the views that see it, in ascending
 *                 view order; k1_pitch >= C, a multiple of 4, 16-byte aligned rows.
 *   k1_count      (N) int32: views that see the voxel (the stride-4 projection, depth-gated when the chunks were).
 *   k2_sum        (N, k2_pitch) fp32, k2_pitch >= 3 (cm + 4), a multiple of 4: three segments of cm + 4 floats, each laid out
 *                 [r, g, b, 0, mapped channel 0 .. cm-1]: sum_seen v, sum_seen (v - fill)^2, sum_seen (v - fill), where fill is the
 *                 Linear's bias (mapped channels) or 0 (colour) and "seen" is the stride-4 map for mapped channels, the image for colour.
 *   k2_count      (N, 2) int32: views that see the voxel in the stride-4 map / in the stride-1 image.
 * A zeroed state is an empty scene.  Pitches must fit int32. */
typedef struct NdetSceneAccum {
    int32_t size;
    int32_t N, C, cm;
    int32_t n_views;
    float* k1_sum;
    int64_t k1_pitch;
    int32_t* k1_count;
    float* k2_sum;
    int64_t k2_pitch;
    int32_t* k2_count;
} NdetSceneAccum;

/* Add one chunk of n_views views (any number; K2 runs in launches of at most 128) to the state: K1's running sums and count of
 * nerfdet.py:164-176 without the division, K2's shifted sums and counts of nerfdet.py:234-253 without the finish.  Inputs as in
 * ndet_backproject_aggregate (features, h x w, pitches) and ndet_density_features_packed (mapped map at the same h x w, bias, rgb,
 * projections) for the chunk's views; points (3, N).  gate: NULL, or the depth gate of nerfdet.py:404-411 for the chunk's views
 * (maps at h x w and H x W).  Feeding a scene's views in any chunking leaves the same K1 sums and the same counts as one chunk. */
int ndet_scene_accumulate(const NdetSceneAccum* s, const float* features_nhwc, int n_views, int h, int w,
                          int64_t view_pitch, int64_t row_pitch, const float* mapped_nhwc, int64_t mview_pitch,
                          int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv, int64_t rsc,
                          int64_t rsy, const float* points, const float* projection, const float* rgb_projection,
                          const NdetDepthGate* gate, void* stream);

/* K2's finish over the state's s->n_views views (nerfdet.py:234-253): global_feat (N, 2 (3 + cm)) rows [mean_c, cov_c] with the packed
 * kernel's expressions (mean not zeroed at cnt 0, variance 1e6 at cnt 0, cov = exp(-var)).  bias: the Linear's bias, the state's pivot.
 * For a state filled by one chunk of <= 128 views the rows equal ndet_density_features_packed's bit for bit. */
int ndet_scene_density_finish(const NdetSceneAccum* s, const float* bias, float* global_feat, void* stream);

/* K1's epilogue over the state (nerfdet.py:175-176, 259-261): out (N, C) channels-last = alpha * sum / (count + 1e-8), 0 where count
 * is 0 (alpha NULL: no gating), count (N) int64.  Equals ndet_backproject_aggregate over all the state's views bit for bit. */
int ndet_scene_volume_finish(const NdetSceneAccum* s, const float* alpha, float* out, int64_t* count, void* stream);

/* Sliding windows: one state per chunk, finished over several states at once, so that a chunk is forgotten by leaving its state out.
 * segs: HOST array of n_segs blocks, oldest first, 1 <= n_segs <= NDET_RING_MAX; every block valid as above, all with the same N, C
 * and cm; the blocks' n_views must add up to an int32.  Per voxel the segments' sums (fp32) and counts (int32) are added in array order,
 * starting from the oldest segment's values (not from zero), and the total is finished with the single-state expressions: n_segs == 1
 * gives the single-state function's output bit for bit.  A segment's row is not read where its own count for the voxel is 0 (a state
 * filled by ndet_scene_accumulate holds an all-zero row there); the states are only read. */
#define NDET_RING_MAX 64

/* ndet_scene_density_finish over a ring of states (nerfdet.py:234-253): global_feat (N, 2 (3 + cm)), n_views the segments' total. */
int ndet_scene_density_finish_ring(const NdetSceneAccum* segs, int n_segs, const float* bias, float* global_feat, void* stream);

/* ndet_scene_volume_finish over a ring of states (nerfdet.py:175-176, 259-261): out (N, C) channels-last, count (N) int64. */
int ndet_scene_volume_finish_ring(const NdetSceneAccum* segs, int n_segs, const float* alpha, float* out, int64_t* count, void* stream);

/* Scene groups: many streamed scenes served by one call (nerf-det_amd/streaming.py, SceneGroup).  Every scene keeps a state of its own, laid
 * out as an NdetSceneAccum's tensors; one accumulate folds one chunk of k views per listed scene into that scene's state, one finish
 * finishes the listed scenes' states, with grid.y = listed scene.  Nothing a scene receives depends on the other scenes of the call:
 *   - for the same feature rows, mapped rows, images, points, projections and gate, a scene's four state tensors after
 *     ndet_scene_accumulate_group hold the bits ndet_scene_accumulate leaves in them for that scene alone (sums and counts), for any
 *     number of scenes, any subset and any order of the listed scenes;
 *   - the grouped finishes write, per listed scene, the single-state finishes' rows, volume and counts bit for bit.
 *
 * NdetSceneSlot: one 64-byte row per scene of the group, a table in DEVICE memory (built once per group; the host cannot read it, so
 * the caller answers for its pointers: the alignments of NdetSceneAccum, allocations of N rows at the group's pitches, points (3, N)).
 * NdetSceneGroup: what the group's scenes share, one HOST block per call (size = sizeof(NdetSceneGroup)): the table and its n_slots
 *   (1 .. NDET_GROUP_MAX), N, C, cm and the two state pitches, under NdetSceneAccum's rules.
 * NdetGroupSel: the scenes one call serves, a HOST block (size = sizeof(NdetGroupSel)) that rides by value in the kernel arguments:
 *   n          listed scenes, 1 .. NDET_GROUP_MAX; grid.y of every launch.
 *   slot[i]    table row of listed scene i: 0 <= slot[i] < n_slots, all distinct (two blocks never share a state).
 *   n_views[i] the scene's view total: for the accumulate the views held before the call (n_views[i] + k must fit int32), for the
 *              finishes the views held (>= 0; the divisor-side n_views of nerfdet.py:234-253).
 * Entries beyond n are not read. */
#define NDET_GROUP_MAX 64
typedef struct NdetSceneSlot {
    float* k1_sum;
    int32_t* k1_count;
    float* k2_sum;
    int32_t* k2_count;
    const float* points;
    int64_t reserved[3];
} NdetSceneSlot;

typedef struct NdetSceneGroup {
    int32_t size;
    int32_t n_slots;
    int32_t N, C, cm;
    int32_t reserved;
    int64_t k1_pitch, k2_pitch;
    const NdetSceneSlot* table;
} NdetSceneGroup;

typedef struct NdetGroupSel {
    int32_t size;
    int32_t n;
    int32_t slot[NDET_GROUP_MAX];
    int32_t n_views[NDET_GROUP_MAX];
} NdetGroupSel;

/* The host-side checks every group entry point makes before it launches anything, on their own (nerfdet.py:164-176, 234-253 are what the
 * blocks feed): the NdetSceneGroup's fields as ndet_scene_accumulate checks an NdetSceneAccum's, the selection as described above.
 * k > 0: also the accumulate's check that n_views[i] + k fits int32; k = 0: the finishes' checks.  NDET_OK, NDET_E_INVALID or
 * NDET_E_UNSUPPORTED (message set); nothing is launched and no device memory is read. */
int ndet_scene_group_check(const NdetSceneGroup* g, const NdetGroupSel* sel, int k);

/* ndet_scene_accumulate for sel->n scenes in two launches (K1's running sums and count of nerfdet.py:164-176, K2's shifted sums and
 * counts of nerfdet.py:234-253): every listed scene brings k views, 1 <= k <= 128.  features / mapped / rgb / projection /
 * rgb_projection and the gate's maps hold n * k views, scene-major in the listed order (listed scene i owns views i k .. (i + 1) k - 1),
 * with the pitches and alignments of ndet_scene_accumulate; k views of the mapped map and of the images must each stay below 2^31
 * floats.  gate: NULL, or one depth gate over the n * k views (gate->n_views = n * k): it gates every scene of the call.  The states and
 * points come from the table rows sel->slot[i].  A scene's state ends up bit-equal to ndet_scene_accumulate on that scene alone. */
int ndet_scene_accumulate_group(const NdetSceneGroup* g, const NdetGroupSel* sel, int k, const float* features_nhwc, int h, int w,
                                int64_t view_pitch, int64_t row_pitch, const float* mapped_nhwc, int64_t mview_pitch,
                                int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv, int64_t rsc,
                                int64_t rsy, const float* projection, const float* rgb_projection, const NdetDepthGate* gate,
                                void* stream);

/* ndet_scene_density_finish for the listed scenes in one launch (nerfdet.py:234-253): global_feat (n N, 2 (3 + cm)), listed scene i's
 * voxel v in row i N + v, finished over sel->n_views[i] views; bit for bit the single-state finish's rows.  The states are only read. */
int ndet_scene_density_finish_group(const NdetSceneGroup* g, const NdetGroupSel* sel, const float* bias, float* global_feat, void* stream);

/* ndet_scene_volume_finish for the listed scenes in one launch (nerfdet.py:175-176, 259-261): out (n, N, C) channels-last, count (n, N)
 * int64, alpha NULL or (n N) indexed as global_feat's rows; bit for bit the single-state finish's outputs.  The states are only read. */
int ndet_scene_volume_finish_group(const NdetSceneGroup* g, const NdetGroupSel* sel, const float* alpha, float* out, int64_t* count,
                                   void* stream);

/* Windowed groups: every scene of a group keeps a sliding window of chunks, one state per chunk (nerf-det_amd/streaming.py,
 * SceneGroup(window=S)), and the listed scenes' windows are finished by one launch, grid.y = listed scene, each scene over its own
 * number of segments.  The accumulate side is ndet_scene_accumulate_group, unchanged: a call's chunks go into empty states listed by a
 * per-call table of n rows.
 *
 * The states of all the scenes form a pool: one NdetSceneSlot row per state in a DEVICE table (a row carries its scene's points), described
 * by an NdetSceneGroup block with n_slots in 1 .. NDET_GROUP_POOL_MAX (up to NDET_RING_MAX + 1 states for each of NDET_GROUP_MAX scenes: a
 * sliding window of S chunks owns S + 1 states).  The block's other fields are checked as ndet_scene_group_check checks them; the four
 * entry points above keep refusing n_slots > NDET_GROUP_MAX.
 * NdetGroupRingSel: the scenes one ring finish serves, a HOST block (size = sizeof(NdetGroupRingSel)) that rides by value in the kernel
 * arguments:
 *   n          listed scenes, 1 .. NDET_GROUP_MAX; grid.y of the launch.
 *   n_segs[i]  segments of listed scene i, 1 .. NDET_RING_MAX.
 *   n_views[i] the scene's view total over its segments (>= 0; the divisor-side n_views of nerfdet.py:234-253).
 * The segment lists: (n, NDET_RING_MAX) int32 pool rows, row i listed scene i's segments oldest first; entries beyond n_segs[i] are never
 * read.  Up to 16 KiB, too large for the kernel arguments, so the list is passed twice: segs_host (HOST memory, read by the checks only) and
 * segs_dev (DEVICE memory holding the same values, read by the kernel; the caller uploads it on the call's stream).  No pool row may be
 * listed twice in one call.  The entry points copy nothing and do not wait for the device.
 * Per voxel a scene's segments are added in list order starting from the oldest segment's values, as ndet_scene_*_finish_ring add them:
 * listed scene i's outputs are bit for bit those functions' outputs over its segments' states (so one segment gives the single-state
 * finish's).  The states are only read. */
#define NDET_GROUP_POOL_MAX (NDET_GROUP_MAX * (NDET_RING_MAX + 1))
typedef struct NdetGroupRingSel {
    int32_t size;
    int32_t n;
    int32_t n_segs[NDET_GROUP_MAX];
    int32_t n_views[NDET_GROUP_MAX];
} NdetGroupRingSel;

/* The host-side checks both grouped ring finishes make before they launch anything, on their own (nerfdet.py:164-176, 234-253 are what
 * the blocks feed): the pool block, the selection, every listed pool row inside the table and listed once.  NDET_OK, NDET_E_INVALID or NDET_E_UNSUPPORTED (message set); nothing is launched
 * and no device memory is read. */
int ndet_scene_group_ring_check(const NdetSceneGroup* pool, const NdetGroupRingSel* sel, const int32_t* segs_host);

/* ndet_scene_density_finish_ring for the listed scenes in one launch (nerfdet.py:234-253): global_feat (n N, 2 (3 + cm)), listed scene
 * i's voxel v in row i N + v, finished over sel->n_views[i] views. */
int ndet_scene_density_finish_group_ring(const NdetSceneGroup* pool, const NdetGroupRingSel* sel, const int32_t* segs_host,
                                         const int32_t* segs_dev, const float* bias, float* global_feat, void* stream);

/* ndet_scene_volume_finish_ring for the listed scenes in one launch (nerfdet.py:175-176, 259-261): out (n, N, C) channels-last, count
 * (n, N) int64, alpha NULL or (n N) indexed as global_feat's rows. */
int ndet_scene_volume_finish_group_ring(const NdetSceneGroup* pool, const NdetGroupRingSel* sel, const int32_t* segs_host,
                                        const int32_t* segs_dev, const float* alpha, float* out, int64_t* count, void* stream);

/* A6 (gating only, unfused form). volume = (1-exp(-density)) * mean, 0 where count==0; nerfdet.py:257-261.
 * mean/out in `layout` with C channels. */
int ndet_alpha_gate(const float* mean, const float* density, const int64_t* count, float* out,
                    int C, int N, int layout, void* stream);

/* alpha = 1 - exp(-relu(raw_sigma)) for N voxels (nerf_mlp.py:227 + nerfdet.py:257). */
int ndet_sigma_to_alpha(const float* raw_sigma, float* alpha, int N, void* stream);

/* A6 input assembly: rows [posenc(xyz) (63) | global (F) | zero padding] for the sigma-MLP, nerf_mlp.py:181-197,140.
 * points (3,N) SoA; out (N, out_stride), out_stride >= 63+F (a multiple of 32 when the rows feed the MFMA kernel). */
int ndet_posenc_concat(const float* points, const float* global_feat, int N, int F, int out_stride, float* out,
                       void* stream);

/* A6 tail. sigma = w . [h | x] + b on the re-joined trunk output without materialising the concat (nerf_mlp.py:86,143),
 * alpha = 1 - exp(-relu(sigma)) (nerf_mlp.py:227, nerfdet.py:257).  h (N,Ch); x (N, x_stride) of which the first Cx columns
 * are used; w (Ch+Cx); bias: DEVICE scalar; raw_sigma (N) or NULL; alpha (N). */
int ndet_sigma_head(const float* h, int Ch, const float* x, int Cx, int x_stride, const float* w, const float* bias,
                    int N, float* raw_sigma, float* alpha, void* stream);

/* A15. Greedy class-aware axis-aligned 3D NMS. Replaces aligned_3d_nms(),
 * mmdet3d/core/post_processing/box3d_nms.py:91-138 (pinned by the reference's tests/test_nms.py:5-58).
 * boxes (n,6) x1,y1,z1,x2,y2,z2; scores (n); classes (n) int64; n <= 4096.
 * keep: (n) int64, receives the picked ORIGINAL indices in pick order (highest score first);
 * n_keep: (1) int64 device scalar.  workspace: ndet_nms_workspace_bytes(n) bytes of device memory.
 * Score ties (undefined in the reference: torch.argsort is unstable) are taken higher index first. */
int64_t ndet_nms_workspace_bytes(int n);
int ndet_aligned_3d_nms(const float* boxes, const float* scores, const int64_t* classes, int n, float thresh,
                        int64_t* keep, int64_t* n_keep, void* workspace, void* stream);

/* A14 decode. One pass per head level over the fused head convolution output raw (N, 7 + n_cls) =
 * [centerness logit | 6 reg | n_cls class logits]: best class score = max_k sigmoid(cls_k)*sigmoid(centerness)*valid, its label,
 * and the decoded box (x1,y1,z1,x2,y2,z2) = voxel corner -/+ exp(scale*reg).  Replaces the elementwise chain of
 * mmdet3d/models/dense_heads/imvoxel_head_v2.py:262-271 + :447 + :547-555 (top-k, thresholding and NMS follow).
 * valid (N) uint8; scale: DEVICE pointer to the level's learnable scalar; voxel_size_host already multiplied by 2^level. */
int ndet_head_decode(const float* raw, int n_cls, const uint8_t* valid, const float* scale, int nx, int ny, int nz,
                     const float* voxel_size_host, const float* origin_host, float* best, int64_t* label, float* boxes,
                     void* stream);

/* ndet_level_valid + ndet_head_decode for up to four head levels in ONE launch (imvoxel_head_v2.py:262-271,442-449,547-555; the tail of the
 * one-scene loop is a chain of tiny dependent kernels).  HOST arrays of per-level DEVICE pointers (raw, scale, best, label, boxes), HOST dims
 * (3 ints per level), integer down-scale factors against the (X, Y, Z) float validity volume `valid` (1 or even, dims * factor == X, Y, Z), HOST
 * voxel sizes (3 floats per level, already times 2^level) and origin.  Same arithmetic, level by level, as the two separate calls. */
int ndet_head_decode_levels(int n_levels, const float* const* raw_host, const float* const* scale_host, const int* dims_host,
                            const int* factor_host, const float* voxel_size_host, const float* origin_host, int n_cls, const float* valid, int X,
                            int Y, int Z, float* const* best_host, int64_t* const* label_host, float* const* boxes_host, void* stream);

/* valid mask of an FPN level: F.interpolate(valid, size, mode='trilinear').round().bool() of
 * mmdet3d/models/dense_heads/imvoxel_head_v2.py:442-449 for the integer down-scale `factor` (1 or even) of the level:
 * valid (X,Y,Z) float view counts -> out (X/f,Y/f,Z/f) uint8. */
int ndet_level_valid(const float* valid, int X, int Y, int Z, int factor, uint8_t* out, void* stream);

/* `scores > score_thr` over the concatenated levels (imvoxel_head_v2.py:533-545) as one order-preserving compaction:
 * best/label/boxes are HOST arrays of n_levels device pointers (per-level outputs of ndet_head_decode), n the level sizes;
 * survivors go to out_* in level-then-voxel order, counts (device, n_levels + 1 ints) = per level, then the total. */
int ndet_select_candidates(int n_levels, const float* const* best, const int64_t* const* label, const float* const* boxes,
                           const int* n, float score_thr, float* out_best, int64_t* out_label, float* out_boxes, int* counts,
                           void* stream);

/* The same compaction with the per-level top-``nms_pre`` cut of dense_heads/imvoxel_head_v2.py:272-276 decided on the device (radix
 * select over the score bits): the kept set per level is what ``topk(nms_pre)`` followed by ``scores > score_thr`` keeps.
 * counts (n_levels + 2 ints): per level after the cut, total, survivors before the cut. */
int ndet_select_candidates_topk(int n_levels, const float* const* best, const int64_t* const* label, const float* const* boxes,
                                const int* n, float score_thr, int nms_pre, float* out_best, int64_t* out_label, float* out_boxes,
                                int* counts, void* stream);

/* picked candidates -> detections in pick order: (centre, size) boxes, scores, labels (imvoxel_head_v2.py:546-555). */
int ndet_gather_detections(const int64_t* keep, int n_keep, const float* boxes, const float* scores, const int64_t* labels,
                           float* out_boxes, float* out_scores, int64_t* out_labels, void* stream);

/* The tail of get_bboxes without a host round trip (dense_heads/imvoxel_head_v2.py:216-285,528-555 + core/bbox/transforms.py:49-67):
 * greedy NMS (core/post_processing/box3d_nms.py:91-138) over the candidates ndet_select_candidates compacted -- their count is read
 * on the device from counts[n_levels] -- and the picks packed for ONE device-to-host copy: out_packed = {n_keep, n_candidates,
 * status, range guard} followed by up to k_cap rows [x, y, z_bottom, dx, dy, dz, 0, score, label]; range_guard (may be null): the scene's guard word
 * of ndet_conv_split / ndet_conv_chain (NdetConvArgs::guard), whose bit 0 is copied into the header so that it reaches the host with the picks.  status != 0 (more than n_cap <= 4096
 * candidates, a level with more than nms_pre survivors, more picks than rows): the caller repeats the scene on the synchronous
 * path.  workspace: ndet_nms_workspace_bytes(n_cap). */
int ndet_nms_pack_detections(const float* cand_boxes, const float* cand_scores, const int64_t* cand_labels, const int* counts,
                             int n_levels, int nms_pre, int n_cap, float thresh, int64_t* keep, int64_t* n_keep, void* workspace,
                             float* out_packed, int k_cap, const unsigned* range_guard, void* stream);

/* A9. Samples along rays. Replaces sample_along_camera_ray(), mmdet3d/models/model_utils/render_ray.py:145-189
 * (inv_uniform=False).  ray_o, ray_d (R,3); t_rand NULL (det=True) or (R,S) uniforms in [0,1) -- the stream the
 * reference draws with torch.rand_like, injectable for parity.  Outputs pts (R,S,3), z_vals (R,S). */
int ndet_sample_along_rays(const float* ray_o, const float* ray_d, int R, int S, float near, float far,
                           const float* t_rand, float* pts, float* z_vals, void* stream);

/* A7+A8 fused. Replaces Projector.compute() (model_utils/projection.py:91-151, grid_sample=True) followed by
 * compute_mask_points() (render_ray.py:71-93) and the concat / pixel mask of render_ray.py:301-303, without
 * materialising the (R,S,n_views,3+d) tensor.
 * pts (P,3) sample points; KE (n_views,3,4) = rows 0..2 of K(4x4) @ E(4x4) per view (render_ray.py:48-69 cameras);
 * img_h,img_w: cameras[:, :2]; rgb: source images, element (v,c,y,x) at v*rsv + c*rsc + y*rsy + x, H x W;
 * feat_nhwc: mapped features, element (v,y,x,c) at v*fview_pitch + y*frow_pitch + x*d + c, hf x wf, d <= 61.
 * global_feat (P, 2*(3+d)) = [mean(3+d) | exp(-var)(3+d)]; pixel_mask (P) uint8 = (views seeing the point > 1);
 * view_count (P) int32 or NULL. */
int ndet_ray_view_stats(const float* pts, int n_points, const float* KE, int n_views, float img_h, float img_w,
                        const float* rgb, int H, int W, int64_t rsv, int64_t rsc, int64_t rsy,
                        const float* feat_nhwc, int d, int hf, int wf, int64_t fview_pitch, int64_t frow_pitch,
                        float* global_feat, uint8_t* pixel_mask, int* view_count, void* stream);

/* Source images as (n_views,H,W,4) fp32 (4th component 0) for the packed sampler below: one image pixel = one 16-byte load.
 * rgb: element (v,c,y,x) at v*rsv + c*rsc + y*rsy + x -- the (n_v,3,H,W) ``denorm_images`` the reference permutes to
 * (1,n_v,H,W,3) before Projector.compute (model_utils/render_ray.py:296-299).  Once per scene. */
int ndet_pack_rgb_nhwc4(const float* rgb, int n_views, int H, int W, int64_t rsv, int64_t rsc, int64_t rsy, float* out_nhwc4,
                        void* stream);

/* A7+A8 fused, packed form (the training / render_testing hot kernel): same outputs as ndet_ray_view_stats -- Projector.compute()
 * (model_utils/projection.py:91-151) + compute_mask_points() (render_ray.py:71-93) + the concat / pixel mask of render_ray.py:301-303 --
 * for d % 4 == 0 and n_views <= 128.  rgb_nhwc4 from ndet_pack_rgb_nhwc4.  Each (sample, view) is projected once; views without a
 * bilinear tap inside a map are counted, not gathered (they sample exactly 0); the variance uses the shifted one-pass form
 * (equal to the reference's two-pass sum up to fp32 rounding, not bit-equal). */
int ndet_ray_view_stats_packed(const float* pts, int n_points, const float* KE, int n_views, float img_h, float img_w,
                               const float* rgb_nhwc4, int H, int W, const float* feat_nhwc, int d, int hf, int wf,
                               int64_t fview_pitch, int64_t frow_pitch, float* global_feat, uint8_t* pixel_mask, int* view_count,
                               void* stream);

/* A view bank: the source views of a streamed scene (nerf-det_amd/streaming.py), kept per chunk in separate allocations.  One
 * NdetBankView per source view, oldest first, in DEVICE memory:
 *   feat   (hf, wf, d) mapped map of the view, dense, 16-byte aligned.
 *   rgb4   (H, W, 4) image of the view as ndet_pack_rgb_nhwc4 writes it, 16-byte aligned.
 *   ke     rows 0..2 of K(4x4) @ E(4x4) of the view (render_ray.py:48-69 cameras).
 * The map and image sizes are the call's, the same for every view. */
typedef struct NdetBankView {
    const float* feat;
    const float* rgb4;
    float ke[12];
} NdetBankView;

/* A7+A8 fused over a view bank: the outputs of ndet_ray_view_stats_packed -- Projector.compute() (model_utils/projection.py:91-151) +
 * compute_mask_points() (render_ray.py:71-93) + the concat / pixel mask of render_ray.py:299-303 -- for any number of views, each behind
 * its own pointers.  d % 4 == 0, d <= 128; views_dev 8-byte aligned.  The views are taken in rounds of 64 in ascending order with the
 * statistics carried from round to round; with more than one round a first pass counts the views seeing each sample (the masked mean's
 * weight needs the count over all views).  For at most 128 views the outputs equal ndet_ray_view_stats_packed's bit for bit. */
int ndet_ray_view_stats_bank(const float* pts, int n_points, const NdetBankView* views_dev, int n_views, float img_h, float img_w, int H,
                             int W, int d, int hf, int wf, float* global_feat, uint8_t* pixel_mask, int* view_count, void* stream);

/* The view banks one grouped sampler call serves, a HOST block (size = sizeof(NdetBankGroupSel)) that rides by value in the kernel
 * arguments (1032 bytes; with the library's prefix over n_points 1288 of the 4096 a launch may carry):
 *   n          listed scenes, 1 .. NDET_GROUP_MAX; grid.y of the launch.
 *   views[i]   listed scene i's DEVICE table of NdetBankView rows, oldest view first, 8-byte aligned.
 *   n_views[i] its rows, >= 1.
 *   n_points[i] its sample points, >= 1: rows [sum_{j<i} n_points[j], + n_points[i]) of the call's point array and of every output. */
typedef struct NdetBankGroupSel {
    int32_t size;
    int32_t n;
    const NdetBankView* views[NDET_GROUP_MAX];
    int32_t n_views[NDET_GROUP_MAX];
    int32_t n_points[NDET_GROUP_MAX];
} NdetBankGroupSel;

/* ndet_ray_view_stats_bank for several view banks in one launch -- Projector.compute() (model_utils/projection.py:91-151) +
 * compute_mask_points() (render_ray.py:71-93) + the concat / pixel mask of render_ray.py:299-303 per listed scene.  pts
 * (sum n_points, 3), global_feat (sum n_points, 2*(3+d)), pixel_mask and view_count (sum n_points; view_count may be NULL): listed scene
 * i's rows follow scene i-1's.  The map, image and camera sizes are the call's, shared by every scene; d % 4 == 0, d <= 128; fewer than
 * 2^31 points in all.  Every check runs on the host before the launch and reads no device memory.  Listed scene i's output rows are
 * ndet_ray_view_stats_bank's over views[i] and its points bit for bit, whatever the other scenes, the subset or its order. */
int ndet_ray_view_stats_bank_group(const float* pts, const NdetBankGroupSel* sel, float img_h, float img_w, int H, int W, int d, int hf,
                                   int wf, float* global_feat, uint8_t* pixel_mask, int* view_count, void* stream);

/* ---- empty-space skipping for renders from a streamed scene (nerf-det_amd/streaming.py, skip_empty=; the reference renders every sample).
 * Every entry point checks its arguments on the host before any HIP call: a null pointer, a non-positive size, dilate outside 0 .. 2, a
 * non-finite threshold or lattice origin, a voxel size that is not positive and finite and an unknown `outside` are NDET_E_INVALID; 2^31
 * points or voxels or more, a misaligned pointer and more than 2^24 workgroups are NDET_E_UNSUPPORTED.  Plain vector stores, no global
 * atomics: every output is the same bytes on every call.
 *
 * ndet_occupancy_bits: the alpha of the voxel lattice (1 - exp(-relu(sigma)), nerfdet.py:255-257 -- the density volume a detect() computes;
 * k_composite applies the same expression to a sample, render_ray.py:196-247) as a dilated bit grid.  alpha (N) float32 and count (N)
 * int64 (the `valid` of ndet_scene_volume_finish) in the lattice's flat order n = (ix ny + iy) nz + iz, N = nx ny nz.  Voxel n is SOLID iff
 * !(alpha[n] <= threshold) || count[n] == 0: a NaN alpha is solid, and so is a voxel no view saw.  Bit n (word n >> 5, bit n & 31 of
 * uint32 bits[(N + 31) / 32]; the last word's spare bits are 0) is set iff any voxel within Chebyshev distance `dilate` of n, inside the
 * grid, is solid.  One thread per voxel, a wave's ballot is two whole words. */
int ndet_occupancy_bits(const float* alpha, const int64_t* count, int nx, int ny, int nz, float threshold, int dilate, uint32_t* bits,
                        void* stream);

#define NDET_OUTSIDE_KEEP 0 /* a point outside the lattice is kept */
#define NDET_OUTSIDE_CULL 1 /* ... is culled */

/* Ordered compaction of n_points sample points (n_points, 3) against the bits of ndet_occupancy_bits (sample_along_camera_ray's points,
 * render_ray.py:145-189).  The lattice: n_voxels[3], p0[3] its first point, vs[3] the voxel size, HOST arrays.  Per axis, in float32 and
 * this statement order,   q = (x - p0) / vs;   i = (int)floorf(q + 0.5f)   -- the nearest lattice point.  A point is INSIDE iff all
 * three i lie in [0, n_voxels) and its three coordinates are finite; an inside point is kept iff its bit is set, any other point iff
 * outside == NDET_OUTSIDE_KEEP.  The points go in blocks of 512 consecutive points, a wave each:
 *   ndet_cull_blocks  the number of blocks of n_points points (0 for n_points <= 0);
 *   ndet_cull_count   block_count[b] = kept points of block b (ndet_cull_blocks(n_points) ints);
 *   ndet_cull_write   with block_first the EXCLUSIVE prefix sum of block_count: idx (M) int32, the kept flat point indices in ascending
 *                     order, and pts_kept (M, 3) their points; M = the sum of block_count, which the caller reads back (one read).
 * The bits are staged in LDS when they fit 64 KiB, else read from global memory.  Order inside a block comes from wave ballots and prefix
 * popcounts. */
int64_t ndet_cull_blocks(int64_t n_points);
int ndet_cull_count(const float* pts, int64_t n_points, const uint32_t* bits, const int* n_voxels, const float* p0, const float* vs,
                    int outside, int* block_count, void* stream);
int ndet_cull_write(const float* pts, int64_t n_points, const uint32_t* bits, const int* n_voxels, const float* p0, const float* vs,
                    int outside, const int* block_first, int* idx, float* pts_kept, void* stream);

/* The count pass of ndet_ray_view_stats_bank alone: pixel_mask (n_points) = view_count > 1 and view_count (n_points) int32, the number of
 * views of the bank whose image holds the sample (Projector.compute()'s mask, model_utils/projection.py:91-151, summed as in
 * render_ray.py:299-303) -- ndet_ray_view_stats_bank's two outputs bit for bit, through the same projection, with no gathers. */
int ndet_ray_view_count_bank(const float* pts, int64_t n_points, const NdetBankView* views_dev, int n_views, float img_h, float img_w,
                             uint8_t* pixel_mask, int* view_count, void* stream);

/* ---- early ray termination for renders from a streamed scene (nerf-det_amd/streaming.py, early_stop=; the reference composites every
 * sample).  A pass of R rays x S samples is walked front to back in segments of consecutive columns [s0, s1); a ray whose transmittance
 * at a segment's first column is below eps is left out from there on, its raw rows stay zero, and a zero row is an exact no-op in
 * ndet_composite.  Every entry point checks its arguments on the host before any HIP call: a null pointer, a non-positive R or S,
 * s0 < 0, s1 > S, s1 < s0 (s1 <= s0 for the front pair), an eps that is NaN or outside [0, 1) and the lattice's knobs as
 * ndet_cull_count rejects them are NDET_E_INVALID; a segment of more than 32 columns, R S of 2^31 or more, 2^31 voxels or more, a
 * misaligned pointer (raw: 16 bytes, the rest 4) and more than 2^24 workgroups are NDET_E_UNSUPPORTED.  Plain vector stores, no atomics:
 * every output is the same bytes on every call.
 *
 * ndet_ray_advance: T[r] <- T[r] * prod_{s = s0}^{s1 - 1} ((1.0f - a_s) + 1e-10f), a_s = 1.0f - expf(-raw[r, s, 3]), s ascending, in
 * ndet_composite's statements (raw2outputs' cumprod(1 - alpha + 1e-10), render_ray.py:196-247): advanced from 1 over columns [0, b),
 * T[r] is ndet_composite's transparency[r, b] bit for bit.  raw (R S, 4), T (R) updated in place; one lane per ray, one store per ray;
 * s0 == s1 launches nothing. */
int ndet_ray_advance(const float* raw, float* T, int R, int S, int s0, int s1, void* stream);

/* Ordered compaction of the LIVE rays' samples of the segment [s0, s1), 1 <= w = s1 - s0 <= 32, of pts (R S, 3), optionally through the
 * occupancy grid of ndet_occupancy_bits in the same launch (the samples whose weights raw2outputs would compute, render_ray.py:196-247).
 * The virtual point n = r w + c stands for the flat sample f = r S + s0 + c.  It is KEPT iff !(T[r] < eps) -- a float32 compare: a NaN
 * transmittance keeps the ray -- and, if bits is not NULL, ndet_cull_count would keep pts[f] (the same float32 statements: nearest
 * lattice point, finite test, `outside` rule).  With bits == NULL the arguments n_voxels, p0, vs and outside are ignored and may be NULL.
 * The nominal width of a segment is the least of 4, 8, 16, 32 that holds w; a wave step covers 64 / nominal consecutive rays, lanes over
 * (ray, column), and a wave owns one block of 512 / nominal consecutive rays:
 *   ndet_front_blocks  the number of blocks of R rays at width w (0 for R <= 0 or w outside 1 .. 32);
 *   ndet_front_count   block_count[b] = kept virtual points of block b (ndet_front_blocks(R, w) ints);
 *   ndet_front_write   with block_first the EXCLUSIVE prefix sum of block_count: idx (M) int32, the kept f in ascending order, and
 *                      pts_kept (M, 3) their points; M = the sum of block_count, which the caller reads back (one read).
 * The bits are staged in LDS when they fit 64 KiB, else read from global memory.  Order inside a block comes from wave ballots and prefix
 * popcounts; T must not change between the two launches. */
int64_t ndet_front_blocks(int64_t R, int w);
int ndet_front_count(const float* pts, int R, int S, int s0, int s1, const float* T, float eps, const uint32_t* bits, const int* n_voxels,
                     const float* p0, const float* vs, int outside, int* block_count, void* stream);
int ndet_front_write(const float* pts, int R, int S, int s0, int s1, const float* T, float eps, const uint32_t* bits, const int* n_voxels,
                     const float* p0, const float* vs, int outside, const int* block_first, int* idx, float* pts_kept, void* stream);

/* ---- space carving from depth frames (nerf-det_amd/streaming.py, begin_scene(carve=); the reference has no counterpart).
 * A FINE lattice of (nx, ny, nz) voxels, n = (ix ny + iy) nz + iz, refines the detection lattice by refine = 1, 2 or 4 per axis (the same
 * box, the same centre).  Every entry point checks its arguments on the host before any HIP call: a null pointer, a non-positive size,
 * min_free < 1, dilate outside 0 .. 2, a band that is not finite and positive, a depth dtype other than 0 / 1, pitches smaller than the
 * map, refine other than 1 / 2 / 4 (with coarse_bits: fine sizes that are no multiples of it) and fewer than 1 or more than
 * NDET_RING_MAX segments are NDET_E_INVALID; 2^31 voxels or more, more than 2^24 workgroups and a misaligned pointer are
 * NDET_E_UNSUPPORTED.  Plain vector stores, no atomics: the same bytes on every call.
 *
 * ndet_carve_accumulate: adds the evidence of a chunk's k >= 1 views to counts (N) uint32, one word per fine voxel: the FREE count in bits
 * 0-15, the HIT count in bits 16-31, each saturating at 65535 (integer adds: any chunking of the same views leaves the same bytes).
 * points (3, nx, ny, nz) the fine lattice (ndet_get_points), proj (k, 3, 4) the chunk's stride-1 projections (DEVICE), depth the chunk's
 * image-resolution depth maps, element (v, y, x) at v view_pitch + y row_pitch + x, dtype 0 = float32 / 1 = float64, H x W the image.
 * View v and voxel n: the point goes through the projection of ndet_density_features' RGB gather (k-ordered FMA chain, round-half-even
 * pixel, in-image and z > 0); a rejected point is no evidence.  Else d = depth[v, y, x]; !(d > 0) -- a hole, a negative, a NaN -- is no
 * evidence.  Else, in the map's dtype (z widened exactly for float64; band rounded to float32 for float32):
 *     FREE  iff !(z > d - band)               in front of the surface by at least the band;
 *     HIT   iff  z > d - band && z < d + band the depth gate's own test (NdetDepthGate, nerfdet.py:404-411);
 *     else behind the surface: no evidence.
 * One thread per voxel, the views' loop inside it, one read-modify-write of the voxel's word per launch. */
int ndet_carve_accumulate(const float* points, int nx, int ny, int nz, const float* proj, int k, const void* depth, int dtype,
                          int64_t view_pitch, int64_t row_pitch, int H, int W, double band, uint32_t* counts, void* stream);

/* ndet_carve_bits: n_segs (1 .. NDET_RING_MAX) counter buffers, a HOST array of device pointers, -> bits[(N + 31) / 32] in
 * ndet_occupancy_bits' format (the last word's spare bits are 0), for ndet_cull_* and ndet_front_* to leave samples out of a render
 * (the reference composites every sample, render_ray.py:196-247).  Per fine voxel free and hit are summed over the segments in 32 bits.
 * The voxel is EMPTY iff free >= min_free && hit == 0, else SOLID (unseen, behind a surface or on one).  With coarse_bits -- an UNDILATED
 * grid of ndet_occupancy_bits on the parent lattice (nx, ny, nz) / refine -- a voxel is solid iff it is carve-solid AND bit
 * ((ix / refine) (ny / refine) + iy / refine) (nz / refine) + iz / refine is set.  Bit n is set iff a voxel within Chebyshev distance
 * dilate of n, inside the grid, is solid.  scratch: NULL, or (N + 31) / 32 words of the caller's; with scratch and dilate > 0 a first
 * launch writes the undilated grid there and a second dilates from those bits (the segments are read once a voxel), else every thread
 * sums the segments over its whole neighbourhood.  Both forms give the same bytes. */
int ndet_carve_bits(const uint32_t* const* segments, int n_segs, int min_free, int dilate, int nx, int ny, int nz,
                    const uint32_t* coarse_bits, int refine, uint32_t* scratch, uint32_t* bits, void* stream);

/* ---- points out: a voxel-downsampled point cloud of a streamed RGB-D scene (nerf-det_amd/streaming.py, begin_scene(cloud=); DESIGN.md
 * 22; the reference has no counterpart).  The FINE lattice is the carve's: (nx, ny, nz) voxels, n = (ix ny + iy) nz + iz, first point p0,
 * voxel size vs (HOST float[3] each).  A voxel's record is 8 uint32 words, 32 bytes: n, sum qx, sum qy, sum qz, sum b, sum g, sum r and
 * one spare word that is never written.  Every entry point checks its arguments on the host before any HIP call: a null pointer, a
 * non-positive size, a depth dtype other than 0 / 1, pitches smaller than the map or the planes, a voxel size that is not finite and
 * positive, an origin that is not finite, a NaN max_depth, min_points < 1 and fewer than 1 or more than NDET_RING_MAX segments are
 * NDET_E_INVALID; 2^31 voxels or points or more, 2^24 workgroups or more, k H W >= 2^24 pixels in one launch, a misaligned pointer and
 * more than 32767 boxes are NDET_E_UNSUPPORTED.
 *
 * ndet_cloud_accumulate: adds the k >= 1 views of a chunk to sums (N, 8).  depth: the chunk's image-resolution maps, element (v, y, x) at
 * v view_pitch + y row_pitch + x, dtype 0 = float32 / 1 = float64; rgb: the B, G, R float planes in [0, 1], element (v, c, y, x) at
 * v rgb_view_pitch + c rgb_plane_pitch + y rgb_row_pitch + x; intrinsic_rows (2,3), camrotc2w (k,3,3), cam_lightpos (k,3) DEVICE, as
 * ndet_camera_rays takes them.  Pixel (v, xi, yi), d = (float) the map's value, contributes iff d > 0, d is finite and (max_depth <= 0 or
 * d <= max_depth).  Its point is the camera centre plus d times ndet_camera_rays' direction of the pixel (get_dtu_raydir,
 * mmdet3d/datasets/pipelines/data_augment_utils.py:410-424; the reference itself uses a depth map only in the gate of
 * nerfdet.py:404-411), in ndet_label_frames' float32
 * statements (pt_j = fmaf(d, dir_j, centre_j)).  Per axis, in float32, t = (x - p0) / vs + 0.5f, i = floorf(t), frac = t - i -- the
 * voxel whose bit ndet_cull_* reads for the point; a point with an index out of range or a coordinate that is not finite is dropped;
 * q = min((int)(frac * 256.0f), 255).  A colour byte is ndet_pack_frames' (x 255 rounded half up, saturated, NaN -> 0).  The voxel's
 * record takes n += 1, the three q and the three bytes, by integer atomics: any chunking and any arrival order leave the same bytes; a
 * sum of bytes stays exact below 2^24 contributions, which the caller keeps track of.  One thread per pixel.  merge != 0: a wave sums
 * the values of its lanes that share a voxel before it touches memory; merge == 0: every lane adds its own.  The same bytes. */
int ndet_cloud_accumulate(const void* depth, int dtype, int64_t view_pitch, int64_t row_pitch, const float* rgb, int64_t rgb_view_pitch,
                          int64_t rgb_plane_pitch, int64_t rgb_row_pitch, const float* intrinsic_rows, const float* camrotc2w,
                          const float* cam_lightpos, int k, int H, int W, const float* p0, const float* vs, int nx, int ny, int nz,
                          float max_depth, int merge, uint32_t* sums, void* stream);

/* ndet_cloud_count / ndet_cloud_write: ordered compaction of n_segs (1 .. NDET_RING_MAX) record buffers, a HOST array of device pointers,
 * over the fine lattice (ndet_get_points' of nerfdet.py:380-390, refined; the reference's only 3-D output is its list of boxes).
 * Per fine voxel every field is summed over the segments in 64 bits; the voxel is emitted iff n >= min_points.  ndet_cloud_count writes
 * block_count[ndet_cloud_blocks(N)], the emitted voxels of every 512 consecutive ones; the caller turns them into exclusive prefix sums
 * (block_first) and M, their total.  ndet_cloud_write then writes, for the emitted voxels in ascending flat index:
 *     xyz (M,3)   per axis (float)((double)p0 + (double)vs * ((double)i - 0.5 + ((double)sum_q + 0.5 n) / (256.0 n)));
 *     bgr (M,3)   per channel (2 sum_c + n) / (2 n) in integers;
 *     count (M)   n, saturated to int32;  voxel (M)  the flat index.
 * No atomics: the same bytes on every call. */
int64_t ndet_cloud_blocks(int64_t n_voxels);
int ndet_cloud_count(const uint32_t* const* segments, int n_segs, int nx, int ny, int nz, const float* p0, const float* vs, int min_points,
                     int* block_count, void* stream);
int ndet_cloud_write(const uint32_t* const* segments, int n_segs, int nx, int ny, int nz, const float* p0, const float* vs, int min_points,
                     const int* block_first, float* xyz, uint8_t* bgr, int* count, int* voxel, void* stream);

/* ndet_label_points: labels[p] = the highest index among the n <= 32767 box_frames rows (centre, half extents, cos yaw, sin yaw) that hold
 * point p of points (n_points, 3), -1 for none: ndet_label_frames' test -- the inverse of the corners' yaw,
 * mmdet3d/core/bbox/structures/depth_box3d.py:46-84 -- on a point that the caller has already. */
int ndet_label_points(const float* points, int64_t n_points, const float* box_frames, int n, int16_t* labels, void* stream);

/* A7 exact API form. Replaces Projector.compute(), projection.py:91-151: rgb_feat (P, n_views, 3+d) and
 * mask (P, n_views) fp32 0/1, materialised like the reference. Same inputs as ndet_ray_view_stats. */
int ndet_project_sample(const float* pts, int n_points, const float* KE, int n_views, float img_h, float img_w,
                        const float* rgb, int H, int W, int64_t rsv, int64_t rsc, int64_t rsy,
                        const float* feat_nhwc, int d, int hf, int wf, int64_t fview_pitch, int64_t frow_pitch,
                        float* rgb_feat, float* mask, void* stream);

/* A11. Alpha compositing. Replaces raw2outputs(), render_ray.py:196-247.
 * raw (R,S,4) = [rgb, sigma]; z_vals (R,S); pixel_mask (R,S) uint8 or NULL; zminmax: DEVICE pointer to
 * {z_vals.min(), z_vals.max()} (the depth clamp is global, render_ray.py:236).
 * Outputs rgb_map (R,3), depth_map (R), weights/alpha/transparency (R,S), ray_mask (R) uint8 (NULL if no pixel_mask). */
int ndet_composite(const float* raw, const float* z_vals, const uint8_t* pixel_mask, int R, int S, int white_bkgd,
                   const float* zminmax, float* rgb_map, float* depth_map, float* weights, uint8_t* ray_mask,
                   float* alpha, float* transparency, void* stream);

/* Hierarchical sampling, exact API form.  Replaces sample_pdf(), mmdet3d/models/model_utils/render_ray.py:96-142, with the uniforms
 * supplied: bins (R, M+1), weights (R, M; NOT modified -- the reference adds 1e-5 in place), u: n_out values per ray at rows
 * u_row_stride floats apart -- n_out, or 0 when every ray shares one row (det=True: torch.linspace(0, 1, n_out); else the
 * torch.rand draw) -- samples (R, n_out).  Per ray, every operation rounded on its own: w = weights + 1e-5, pdf = w / sum(w),
 * cdf = [0, cumsum(pdf)], above = #{i < M : u >= cdf[i]}, below = max(above - 1, 0), denom = cdf[above] - cdf[below] (1 where
 * < 1e-5), sample = bins[below] + (u - cdf[below]) / denom * (bins[above] - bins[below]), then kept inside [bins[0], bins[M]]: the
 * reference's float32 result overshoots bins[M] at u = 1.0 when its rounded cdf ends below 1.  The order of the sum and of the running
 * sum is the kernel's own (csrc/importance_kernels.hip), fixed; results repeat bit for bit, torch's differ in the last bits of the cdf.
 * Refused on the host before any launch, reading no device memory: a null pointer, R < 1, M < 1, n_out < 1, u_row_stride neither 0
 * nor n_out (NDET_E_INVALID); M > 254, n_out > 256, R * (M + 1 + n_out) >= 2^31 (NDET_E_UNSUPPORTED). */
int ndet_sample_pdf(const float* bins, const float* weights, int R, int M, const float* u, int u_row_stride, int n_out, float* samples,
                    void* stream);

/* Hierarchical sampling, fused: the fine pass's sample set of render_ray.py:343-356 (inv_uniform=False) in one launch.  z_vals and
 * weights (R, S) of the coarse pass, ray_o and ray_d (R, 3), u as ndet_sample_pdf takes it (n_imp values a ray).  Per ray: bins =
 * .5 * (z[1:] + z[:-1]), the weights weights[:, 1:-1] (M = S - 2), the draw of ndet_sample_pdf (same device code, same bits) ->
 * z_samples_out (R, n_imp; may be NULL); z_out (R, S + n_imp) ascending, as a multiset sort(cat(z_vals, samples)) (equal depths in
 * any order, no NaN); pts_out (R, S + n_imp, 3) = z * ray_d + ray_o, a multiply then an add.
 * Refused on the host before any launch, reading no device memory: a null pointer (z_samples_out excepted), R < 1, S < 3, n_imp < 1,
 * u_row_stride neither 0 nor n_imp (NDET_E_INVALID); S > 256, n_imp > 256, R * (S + n_imp) >= 2^31 (NDET_E_UNSUPPORTED). */
int ndet_importance_merge(const float* z_vals, const float* weights, const float* ray_o, const float* ray_d, int R, int S, const float* u,
                          int u_row_stride, int n_imp, float* z_out, float* pts_out, float* z_samples_out, void* stream);

/* A13/A14. 3D convolution, channels-last, fp32 on the matrix cores, fused epilogue.  Replaces nn.Conv3d /
 * nn.ConvTranspose3d(2,2) + BatchNorm3d(eval) + ReLU (+ residual add) of mmdet3d/models/necks/imvoxelnet.py:8-67,
 * 233-260 and the head convs of mmdet3d/models/dense_heads/imvoxel_head_v2.py:45-49,442-449.
 * in (D,H,W,Cin) fp32, Cin % 32 == 0; w_packed (taps, Cout, Cin) with tap = (kd*k + kh)*k + kw
 * [transposed: (8, Cout, Cin), tap = kd*4 + kh*2 + kw, out voxel = 2*in + (kd,kh,kw)];
 * out (OD,OH,OW,Cout), O = (I + 2*(k/2) - k)/stride + 1 [transposed: 2*I].  ksize 3 or 1, stride 1 or 2.
 * Epilogue: v = acc*scale[co] + shift[co] (if scale != NULL); relu == 2: max(v,0); v += residual (if != NULL);
 * relu == 1: max(v,0).  splits > 1: split-K over blockIdx.z into `workspace` (ndet_conv3d_workspace_bytes) and a
 * fixed-order reduction (bitwise reproducible).  tile: 0 auto, 64 or 128. */
int64_t ndet_conv3d_workspace_bytes(int D, int H, int W, int Cin, int Cout, int ksize, int stride, int splits);
int ndet_conv3d_ndhwc(const float* in, const float* w_packed, float* out, int D, int H, int W, int Cin, int Cout,
                      int ksize, int stride, int transposed, const float* scale, const float* shift,
                      const float* residual, int relu, int splits, int tile, void* workspace, void* stream);

/* Generic form of the same kernel: per-axis kernel / stride / zero-pad (3 ints each, HOST memory, order D,H,W).
 * A batch of 2D feature maps (N,H,W,C) is the case D = N, kernel[0] = 1, pad[0] = 0 -- used for the ResNet/FPN convolutions
 * (conv + eval-BatchNorm + ReLU + residual in one pass; third-party mmdet ResNet/FPN, SURVEY.md appendix C, called at
 * mmdet3d/models/detectors/nerfdet.py:140-142).  w_packed (kd*kh*kw, Cout, Cin).  residual_up2 != 0: `residual` is the
 * coarser (OD, ceil(OH/2), ceil(OW/2), Cout) map and is added at (d, h>>1, w>>1) -- FPN's nearest-x2 top-down add fused
 * into the lateral convolution (not combinable with split-K).  Other arguments as ndet_conv3d_ndhwc;
 * split-K workspace = splits * OD*OH*OW*Cout * 4 bytes. */
int ndet_conv_ndhwc(const float* in, const float* w_packed, float* out, int D, int H, int W, int Cin, int Cout,
                    const int* kernel_host, const int* stride_host, const int* pad_host, const float* scale,
                    const float* shift, const float* residual, int residual_up2, int relu, int splits, int tile,
                    void* workspace, void* stream);

/* Packed fp32 weights (taps, Cout, Cin) -> three bf16 planes tiled per 32-channel K step, (taps, Cin/32, 3, Cout, 32), with
 * w = p0 + p1 + p2 exactly (p0 = bf16(w), p1 = bf16(w - p0), p2 = bf16(w - p0 - p1), round-to-nearest-even).  Prepares the
 * weights of ndet_conv_split with arith 0 / 2 (the conv weights of necks/imvoxelnet.py:36-67, dense_heads/imvoxel_head_v2.py:45-49). */
int ndet_split_weights_bf16x3(const float* w_packed, int taps, int Cout, int Cin, uint16_t* planes, void* stream);

/* The same planes straight from a torch-layout weight (Cout, Cin, taps) -- training re-packs every step.  adjoint = 0: the layer's
 * own weight, planes (taps, Cin/32, 3, Cout, 32).  adjoint = 1: the weight of the layer's data gradient (autograd of the
 * convolutions of mmdet3d/models/necks/imvoxelnet.py:22-67,233-260), W'[t][ci][co] = W[co][ci][taps-1-t], planes
 * (taps, ceil32(Cout)/32, 3, Cin, 32) with the padded input channels zero. */
int ndet_split_weights_bf16x3_torch(const float* w_torch, int taps, int Cout, int Cin, int adjoint, uint16_t* planes, void* stream);

/* A6 fused: [posenc(points) | global_feat] -> 4 x (Linear 256 + ReLU) -> sigma layer over [h | input] -> alpha = 1 - exp(-relu(sigma)), one launch,
 * the 256-wide activations never leave the CU.  Replaces VanillaNeRFRadianceField.query_density (mmdet3d/models/model_utils/nerf_mlp.py:224-227;
 * NerfMLP.query_density :138-144, MLP.forward :80-90 with skip_layer = 3, SinusoidalEncoder.forward :181-197) and the alpha line of
 * detectors/nerfdet.py:254-257 for the shipped architecture (net_depth 4, net_width 256).  points (3, N); global_feat (N, F) or null with F = 0;
 * K0 = 63 + F rounded up to a multiple of 32 (<= 256) = the padded input width the first layer's planes were built for.
 * w_planes_host / w_inv_scale_host / bias_host: HOST arrays of 4 entries -- device pointers to the fp16-pair planes of each hidden layer
 * (ndet_split_weights_f16x2 of the (1, 256, K) packed weight, K = K0 for layer 0 and 256 after it), 1 / their scales, device pointers to the
 * biases (256).  w_sigma (256 + 63 + F) over [h | input], b_sigma (1).  Arithmetic: fp16-pair products, fp32 accumulate, the activation scale
 * taken PER ROW (a row's error is 2^-22 of its own magnitude -- the rows of voxels no view sees hold ~1e9, nerfdet.py:236-243).
 * Outputs: alpha (N); raw_sigma (N, before the ReLU) and h_out (N, 256, the trunk output) may be null. */
int ndet_point_mlp_alpha(const float* points, const float* global_feat, int N, int F, int K0, int hidden, const uint16_t* const* w_planes_host,
                         const float* w_inv_scale_host, const float* const* bias_host, const float* w_sigma, const float* b_sigma,
                         float* raw_sigma, float* alpha, float* h_out, void* stream);

/* fp16-PAIR arithmetic of the same convolutions (arith = 1 below): every fp32 operand, pre-scaled by a power of two so that the tensor's
 * largest magnitude sits in [2^14, 2^15), is written as hi + lo with hi = fp16(x), lo = fp16(x - hi) (2 x 11 significand bits + sign:
 * |x - hi - lo| <= 2^-23 |x| for every element above ~2^-16 of the tensor's maximum), and a*b is accumulated in fp32 as the THREE products
 * hi_a hi_b + hi_a lo_b + lo_a hi_b (each exact in fp32; the dropped lo_a lo_b is <= 2^-22 |ab|) -- half the MFMA work of the six-product
 * bf16x3 scheme, with a measured error against fp64 at or below bf16x3's on every layer shape (three accumulator roundings per K step
 * instead of six; tests/test_conv3d_gpu.py).  Weights: ndet_split_weights_f16x2 builds the planes (taps, Cin/32, 2, Cout, 32) of
 * w * scale once per model (scale = a power of two, chosen by the caller from max |w|); activations: the kernels derive their scale on
 * the device from `in_amax` (max |in|, written by the previous layer's epilogue through its `out_amax`, or by ndet_amax_f32) and undo both
 * scales in the epilogue -- nothing is synchronised with the host.  Same reference modules as ndet_conv_split
 * (mmdet3d/models/necks/imvoxelnet.py:36-67,233-260). */
int ndet_split_weights_f16x2(const float* w_packed, int taps, int Cout, int Cin, float scale, uint16_t* planes, void* stream);

/* max |x| over n floats, atomically maxed (as uint bits) into *slot, which the caller zeroed: the `in_amax` of a fp16-pair convolution
 * whose input no convolution kernel wrote (the voxel volume of nerfdet.py:363-420, the MLP inputs of nerf_mlp.py:200-245). */
int ndet_amax_f32(const float* x, int64_t n, float* slot, void* stream);

/* Floats per amax slot (8 per-XCD sub-slots x 32 floats = 1 KiB): the host allocates slots of exactly this size (nerfdet_amd/conv3d.py asserts it
 * at load time; a narrower slot would make the kernels' sub-slot atomics run into the neighbouring tensor's slot).  Serves the same convolutions as ndet_amax_f32 (mmdet3d/models/necks/imvoxelnet.py:36-67); the reference
 * itself has no counterpart. */
int ndet_amax_slot_floats(void);

/* Measurement knobs of the convolution launchers, set explicitly by profiling scripts (tools/layer_times.py) -- never read from the environment, so
 * a production process cannot pick them up by accident.  "nt_bytes": outputs of at least this many bytes are written with non-temporal stores
 * (default 32 MiB); "order2": 1 / 0 = deal the column tiles of a row tile to one XCD or keep grid order (neither changes a result bit);
 * "deterministic_scatter": 1 = the backward kernels' gradient scatter on 64-bit fixed-point integer atomics (the caller then passes zeroed int64
 * buffers in place of the float ones: order-independent sums, for reproducibility tests; nerfdet_amd/autograd.py::set_deterministic; the
 * grad_bias of ndet_density_features_bwd[_gated] is then 2 * cm int64: units of 2^-40 in [0, cm), units of 2^-8 in [cm, 2 cm));
 * "wgrad_wide": 0 = ndet_wgrad_split (arith 1) keeps its 128 x 128 tile where it would take 128 x 256 (same sums in another association);
 * "wgrad_xcd": 0 = the weight-gradient kernel's workgroups in grid order instead of one K split per XCD at a time (no result bit changes).
 * HOST string.  No reference counterpart (the reference's harness, tools/benchmark.py:63-89, times the model only). */
int ndet_measurement_knob(const char* name_host, int64_t value);

/* The split-family convolutions on the bf16 / fp16 matrix cores (csrc/conv_split_kernels.hip), every argument in one block: the same contract
 * as ndet_conv_ndhwc / the transposed form of ndet_conv3d_ndhwc, replacing the same reference modules -- nn.Conv3d / nn.ConvTranspose3d +
 * BatchNorm3d + ReLU (+ residual) of mmdet3d/models/necks/imvoxelnet.py:36-67,233-260, dense_heads/imvoxel_head_v2.py:45-49 and the mmdet
 * ResNet/FPN convolutions behind detectors/nerfdet.py:140.  `a` is a HOST pointer, read during the call only; a zero / null field switches its
 * feature off.
 *   size          sizeof(NdetConvArgs), set by the caller; any other value is rejected (NDET_E_INVALID): the caller's layout differs from this one.
 *   in, out       (D,H,W,Cin) fp32 channels-last (2D: D = batch, kernel[0] = 1) -> (OD,OH,OW,Cout) [transposed: (2D,2H,2W,Cout)]; `in` 16-byte aligned.
 *   w_planes      the packed (taps, Cout, Cin) weight as tiled planes (taps, Cin/32, P, Cout, 32), 16-byte aligned: ndet_split_weights_bf16x3
 *                 (arith 0 / 2, P = 3), ndet_split_weights_f16x2 or ndet_split_weights_train (arith 1, P = 2).  Cin % 32 == 0.
 *   kernel, stride, pad   per axis (D, H, W).  transposed = 1: k2 s2 ConvTranspose3d (kernel / stride 2, pad 0; 8 taps).
 *   scale, shift  (Cout) folded BatchNorm / bias, both or neither.  relu: 0 none, 1 after the residual add, 2 before it.
 *   residual      (OD,OH,OW,Cout); residual_up2 = 1: a (OD, ceil(OH/2), ceil(OW/2), Cout) map added at (d, h/2, w/2) -- the FPN's nearest x2
 *                 upsample-add (not with split-K).
 *   splits        split-K over blockIdx.z into `workspace` (splits * M * Cout floats), reduced in a fixed order.
 *   tile          a workgroup's tile: 0 auto, or an id of the table CONV_TILES (csrc/conv_split_kernels.hip; read it with ndet_conv_tile_info).  Four
 *                 families: the unified tiles, LDS-staged epilogue or -- NDET_TILE_DIRECT -- storing straight from the accumulators (splits == 1, not
 *                 transposed, Cout % 32 == 0, output < 4 GB); the wave-specialised 128 x 256 tile; its persistent forms (plain convolutions,
 *                 Cout % 16 == 0, <= 32 taps); the halo-stationary 128-voxel patches (stride 1, odd kernel, same padding, more than one tap).  The
 *                 staged and direct forms of a unified tile, and the one-shot and persistent forms of the wave-specialised tile, give bit-identical
 *                 results (tests/test_conv3d_gpu.py).
 *   arith         0 = bf16x3: every fp32 operand as the exact sum of three bf16 terms, the six products of order <= 2 accumulated in fp32 (error at
 *                 the level of an fp32 FMA chain).  1 = fp16 pair (three products; see ndet_split_weights_f16x2).  2 = bf16: both operands rounded
 *                 to bf16, one product, fp32 accumulate and fp32 activations in HBM -- the "bf16" arithmetic BASELINE.json's configs 3 and 5
 *                 name (what torch.autocast(bfloat16) would run the layers in).
 *   in_amax       arith 1 only, and required there: the input's amax slot (ndet_amax_f32, or the out_amax of the launch that wrote it).
 *   w_inv_scale   arith 1 without w_amax: 1 / the scale ndet_split_weights_f16x2 was given (> 0).  Ignored otherwise.
 *   w_amax        the TRAINING form (arith 1, not transposed, no residual_up2; forward and data gradient of the convolutions above and of
 *                 dense_heads/imvoxel_head_v2.py:444-449, detectors/nerfdet.py:140-142): the weight planes were scaled ON THE DEVICE by the
 *                 power of two of this slot -- by ndet_split_weights_train (the optimizer moves the weights every step), or, for the
 *                 weight-gradient GEMM over ndet_wgrad_rows' tap copies, dy's planes from ndet_wgrad_dy_planes_f16x2 -- so 1 / scale is read
 *                 from the same slot and w_inv_scale is ignored; guard_l1 is then the contraction length taps * Cin (||w||_1 <= K max|w|).
 *   out_amax      any arith: max |out| is maxed into this zeroed slot -- the next layer's in_amax.
 *   guard         the RANGE GUARD of arith 1 (ignored otherwise; with it guard_l1 >= 0 and guard_tol > 0).  The activation scale of that arithmetic
 *                 is per tensor, so beside its fp32-class relative error an output carries an absolute floor of at most
 *                     2^-39 max|in| * guard_l1,    guard_l1 = max_j |scale_j| (sum_k |w_jk| + max|w| #{k: 0 < |w_jk| < 2^-16 max|w|})    (host, per pack)
 *                 whatever the distribution inside the tensor (csrc/conv_common.hpp::conv_guard_check).  max|in| is known on the device at kernel
 *                 entry, and so is the smallest maximum any workgroup tile of the input committed (word 1 of the amax sub-slots): when the floor
 *                 exceeds guard_tol AND that tile minimum lies below 2^-16 of max|in| (a part of the tensor really is outside the fp16-pair window;
 *                 a uniformly large tensor is not), the launch ORs 1 into *guard (device word, zeroed by the caller per scene).  The caller reads
 *                 the word with the detections (ndet_nms_pack_detections) and repeats such a scene on bf16x3.  The tensor that first needed it:
 *                 the sigma-MLP rows of detectors/nerfdet.py:236-243.
 *   keep_partials 1 (weight-gradient GEMMs; no affine / residual / ReLU / out_amax, not transposed): a split-K launch leaves its partial sums in
 *                 the workspace for ndet_wgrad_to_torch instead of running the reduction pass; `out` is then not written.
 *   map_w, map_b, map_out   a chained 32-channel projection of every output row in the same launch: map_out (M, 32) = out_row . map_w + map_b,
 *                 map_w (Cout, 32) and map_b (32) with the convolution's own affine folded in by the caller (map_w[c][j] = scale_c Wm[j][c],
 *                 map_b[j] = sum_c shift_c Wm[j][c] + bm[j]); fp32 FMAs; all three 16-byte aligned.  The detector's feature mapping
 *                 (detectors/nerfdet.py:194-197: self.mapping on every FPN level-0 pixel) behind the FPN output convolution: the 276 MB feature
 *                 map is not read back by a launch of its own.  Only the tiles flagged NDET_TILE_OWNS_ROWS (the 256-column halo tiles) take it:
 *                 Cout = 256, no split-K, residual, ReLU or transposition. */
typedef struct NdetConvArgs {
    int32_t size;
    const float* in;
    const uint16_t* w_planes;
    float* out;
    int D, H, W, Cin, Cout;
    int kernel[3], stride[3], pad[3];
    int transposed;
    const float* scale;
    const float* shift;
    const float* residual;
    int residual_up2, relu, splits, tile, arith;
    const float* in_amax;
    float w_inv_scale;
    const float* w_amax;
    float* out_amax;
    void* workspace;
    unsigned* guard;
    float guard_l1, guard_tol;
    int keep_partials;
    const float* map_w;
    const float* map_b;
    float* map_out;
} NdetConvArgs;
int ndet_conv_split(const NdetConvArgs* a, void* stream);

/* ndet_conv_split over a BATCH of volumes in one launch: in (batch, D, H, W, Cin) -> out (batch, OD, OH, OW, Cout), both contiguous; a->D / H / W are
 * ONE volume's extents.  The GEMM has batch * OD * OH * OW rows; a row's taps are bounded by its own volume (nothing is read across a volume's
 * first or last slice), the weights, the affine, the residual (same shape as out), split-K (workspace: splits * batch * M * Cout floats), in_amax /
 * out_amax (one slot each for the whole batch: the fp16-pair scale is shared by its volumes) and the guard work on the rows of all volumes as they
 * do on one volume's.  The layers of mmdet3d/models/necks/imvoxelnet.py:36-67,233-260 and dense_heads/imvoxel_head_v2.py:45-49 for several scenes
 * at once (the reference runs them on a batch axis of nn.Conv3d).  Every tile but the persistent ones (129256 / 129257 / 129064) has a batched
 * instantiation of its kernel beside the plain one.  batch == 1 is ndet_conv_split, launch for launch.  Refused before any HIP call: batch < 1
 * (NDET_E_INVALID); batch > 1 with w_amax, keep_partials, residual_up2, map_* or a persistent tile, batch * OD * OH * OW >= 2^31, and the tile
 * families' operand limits taken over the whole batch (NDET_E_UNSUPPORTED). */
int ndet_conv_split_batch(const NdetConvArgs* a, int batch, void* stream);

/* TEST SUPPORT, not part of the drop-in surface (no caller in the package).  What a halo tile (3128 / 3256 / 3257 / 3258) would launch on a stride-1 same-padded convolution over one D x H x W volume (a batch tiles every
 * volume this way): patch[3] = the 128-voxel output patch (TD, TH, TW) its launcher picks, *looped = 1 when the depth taps are looped outside the
 * staged halo image, 0 when they lie inside it.  No HIP call: for tests that must know which of the two forms a shape exercises.  Part of the
 * launcher of the convolutions of mmdet3d/models/necks/imvoxelnet.py:36-67; the reference has no counterpart.  NDET_E_INVALID for another tile. */
int ndet_conv_halo_patch(int tile, int D, int H, int W, const int* kernel, int* patch, int* looped);

/* TEST SUPPORT, not part of the drop-in surface (no caller in the package).  Taps per barrier interval of the halo tiles' K walk: tile 3128 in
 * arith 1 / 2 multiplies the three taps of a group between two barriers when the staged image's taps come in threes (3x3, 3x3x3 in both depth
 * forms, 3x1x3); every other launch, one.  mode: 1 = every later launch of this process takes the one-tap walk (the same build's reference for
 * the three-tap one: the two are bit-identical by construction), 0 = automatic again (the default), -1 = leave the switch as it is.  With taps or
 * lds_bytes non-null, also what a launch of `tile` in `arith` (as NdetConvArgs::arith) over an image of `taps_per_image` taps would take under the
 * switch as it then stands: *taps = 3 or 1, *lds_bytes = the dynamic LDS of its K walk (split image + weight stages).  No HIP call.  Part of the
 * launcher of the convolutions of mmdet3d/models/necks/imvoxelnet.py:36-67; the reference has no counterpart.  NDET_E_INVALID for a mode outside
 * -1 .. 1 and, when a query is asked, for a tile that is not a halo tile, arith outside 0 .. 2 or taps_per_image < 1 (the switch is then left). */
int ndet_conv_halo_taps(int mode, int tile, int arith, int taps_per_image, int* taps, int* lds_bytes);

#define NDET_TILE_DIRECT 1    /* epilogue straight from the accumulators: final values only */
#define NDET_TILE_OWNS_ROWS 2 /* one tile holds all 256 channels of its rows: the chained projection (map_out) is allowed */
#define NDET_TILE_ORDER2 4    /* may be dealt in the activation-stationary workgroup order */
/* One row of the tile table behind NdetConvArgs::tile: rows x output channels of a workgroup's tile and its NDET_TILE_* flags; NDET_E_INVALID for an
 * id the table does not hold (0 = auto included).  No HIP call.  For the host's copy of the table (nerfdet_amd/conv_tiles.py), which tests hold
 * against this one; part of the launcher of the convolutions of mmdet3d/models/necks/imvoxelnet.py:36-67, the reference has no counterpart. */
int ndet_conv_tile_info(int tile, int* rows, int* cols, int* flags);

/* Convolution + chained 1x1 convolution in one launch: out = act3(bn3(W3 . relu(bn1(conv(in)))) + residual), the intermediate (Cmid = 64 or
 * 128 channels, ALL of them in one 128-row tile) never leaves the CU.  Replaces the conv2 -> bn2 -> relu -> conv3 -> bn3 -> (+identity) ->
 * relu tail of the ResNet bottlenecks the detector runs as `self.backbone(img)` in mmdet3d/models/detectors/nerfdet.py:140 (mmdet's
 * resnet.py Bottleneck.forward; third-party, restated): in stages 1 / 2 the intermediate is 61 / 31 MB per block at 50 views 240x320.
 * in (D,H,W,Cin) fp32 channels-last (2D: D = batch, kernel[0] = 1); w_planes / w3_planes: the planes of the (taps, Cmid, Cin) and (1, Cout, Cmid)
 * packed weights for `arith` (numbered as NdetConvArgs::arith; w1_inv_scale / w3_inv_scale belong to w_planes / w3_planes, 1 for arith 0 / 2);
 * scale1/shift1, scale3/shift3: folded BatchNorm (null = identity); residual (M, Cout) or null; relu3: 0 none, 1 after the residual add, 2
 * before it; in_amax / out_amax as in NdetConvArgs.  Cin % 32 == 0, Cout % 64 == 0.  The bf16x3 form is the same arithmetic as the two
 * ndet_conv_split launches it replaces except that the intermediate is not rounded through memory (it is the same fp32 value); in the
 * fp16-pair arithmetic the intermediate's scale is the workgroup's own maximum: it never exists as a whole tensor.  guard (arith 1, may be
 * null): the range guard of NdetConvArgs -- guard_l1 belongs to w_planes and max|in|, guard_l1_3 to w3_planes and the chained product
 * (reserved: its operand is scaled by each workgroup's own maximum, which needs no check). */
int ndet_conv_chain(const float* in, const uint16_t* w_planes, int D, int H, int W, int Cin, int Cmid, const int* kernel,
                    const int* stride, const int* pad, const float* scale1, const float* shift1, const uint16_t* w3_planes,
                    int Cout, const float* scale3, const float* shift3, const float* residual, int relu3, float* out,
                    int arith, const float* in_amax, float w1_inv_scale, float w3_inv_scale, float* out_amax, float guard_l1,
                    float guard_l1_3, float guard_tol, unsigned* guard, void* stream);

/* A whole ResNet bottleneck of stage 1 in one launch, fp16-pair arithmetic: out = relu(bn3(W3 . relu(bn2(conv3x3(relu(bn1(W1 . x)))))) + identity),
 * identity = x (Cin == Cout) or, with wd_planes, bnD(WD . x) (the first block of the stage; Cin = 64) -- mmdet's Bottleneck.forward (style 'pytorch',
 * stride 1) behind mmdet3d/models/detectors/nerfdet.py:140.  x (N, H, W, Cin) channels-last, out (N, H, W, Cout); the intermediate has 64 channels
 * (w1 (1, Cin/32, 2, 64, 32), w2 (9, 2, 2, 64, 32), w3 (1, 2, 2, Cout, 32), wd (1, Cin/32, 2, Cout, 32): ndet_split_weights_f16x2 planes with their
 * inverse scales; scale* / shift*: folded eval-mode BatchNorm).  A workgroup owns a 4 x 16 patch of one map from x to out: conv1 is evaluated on
 * the patch plus its one-pixel halo into LDS, conv2's taps multiply out of that image, conv3 follows as in ndet_conv_chain; the scales of
 * the two intermediates are the workgroup's own maxima.  in_amax: x's slot; out_amax (may be null): max |out|.  guard (may be null): the range
 * guard word (see NdetConvArgs::guard), guard_l1_host = 4 HOST floats (w1, w2, w3, wd). */
int ndet_bottleneck_f16x2(const float* x, int N, int H, int W, int Cin, int Cout, const uint16_t* w1_planes, float w1_inv_scale, const float* scale1,
                          const float* shift1, const uint16_t* w2_planes, float w2_inv_scale, const float* scale2, const float* shift2,
                          const uint16_t* w3_planes, float w3_inv_scale, const float* scale3, const float* shift3, const uint16_t* wd_planes,
                          float wd_inv_scale, const float* scale_d, const float* shift_d, const float* in_amax, float* out_amax, float* out,
                          const float* guard_l1_host, float guard_tol, unsigned* guard, void* stream);

/* ResNet stem tail in one pass: BatchNorm(eval) as per-channel scale/shift + ReLU + MaxPool(3, stride 2, pad 1) on the
 * channels-last stem output x (N,H,W,C), C % 4 == 0 -> out (N, (H-1)/2+1, (W-1)/2+1, C).  Third-party mmdet ResNet stem
 * (SURVEY.md appendix C), called at mmdet3d/models/detectors/nerfdet.py:140. */
int ndet_bn_relu_maxpool_nhwc(const float* x, const float* scale, const float* shift, int N, int H, int W, int C,
                              float* out, void* stream);

/* ResNet stem in ONE launch: Conv2d(3, 64, 7, stride 2, pad 3, no bias) + BatchNorm(eval, as per-channel scale/shift) + ReLU +
 * MaxPool(3, stride 2, pad 1) -- conv1 / bn1 / relu / maxpool of the third-party mmdet ResNet called at
 * mmdet3d/models/detectors/nerfdet.py:140.  images: N views of 3 x H x W fp32 with the given ELEMENT strides (NCHW or channels-last);
 * w_planes: ndet_stem_pack_weights of the (64,3,7,7) weight; out (N, PH, PW, 64) channels-last, PH = ((H-1)/2+1 - 1)/2 + 1.
 * Arithmetic of ndet_conv_split with arith 0 (fp32 operands as exact sums of three bf16 terms, six MFMA products). */
int ndet_stem_pack_weights(const float* w_64x3x7x7, uint16_t* planes /* (3, 64, 176) */, void* stream);
/* ... and its fp16-pair form (two fp16 planes of w * scale, scale a power of two chosen by the caller from max |w|): ndet_stem_conv_bn_relu_maxpool
 * with w_inv_scale = 1 / scale then issues three fp16 MFMA products per multiply, the image patch scaled by the power of two of its own maximum
 * inside the kernel (same conv1 / bn1 / relu / maxpool of mmdet's ResNet behind mmdet3d/models/detectors/nerfdet.py:140). */
int ndet_stem_pack_weights_f16x2(const float* w_64x3x7x7, float scale, uint16_t* planes /* (2, 64, 176) */, void* stream);

/* The launch itself (see above; conv1 / bn1 / relu / maxpool behind mmdet3d/models/detectors/nerfdet.py:140).  w_inv_scale: 0 for the bf16x3 planes of
 * ndet_stem_pack_weights, else 1 / scale of ndet_stem_pack_weights_f16x2.  out_amax (may be null): max |out|
 * into a zeroed amax slot -- the first bottleneck's fp16-pair scale without another pass over the 61 MB. */
int ndet_stem_conv_bn_relu_maxpool(const float* images, int N, int H, int W, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                                   int64_t stride_x, const uint16_t* w_planes, float w_inv_scale, const float* scale, const float* shift, float* out, float* out_amax,
                                   void* stream);

/* ---- input contract: what the data pipeline hands to nerfdet.forward_*, from decoded,
 * resized and padded uint8 BGR frames (n_frames,H,W,3) resident on the device.  mean_rgb / std_rgb are HOST arrays of 3
 * doubles (the config's img_norm_cfg); the image arithmetic is float32 with stdinv = float(1 / std), as mmcv does it.
 *
 * ndet_normalize_views: for each selected frame ids[v]: img (n_sel,3,H,W) = mmcv.imnormalize(to_rgb=True), and
 * denorm (n_sel,3,H,W) = imdenormalize(img, to_bgr=True).astype(uint8) / 255 -- the round trip of
 * mmdet3d/datasets/pipelines/multi_view.py:107-110, channel-first as formating.py:44-52,80-85 stacks them. */
int ndet_normalize_views(const uint8_t* frames_bgr, const int* ids, int n_sel, int H, int W, const double* mean_rgb,
                         const double* std_rgb, float* img, float* denorm, void* stream);

/* ndet_target_rays: the NeRF targets of multi_view.py:117-155 for frames target_ids[t]: rays on the pixel grid
 * [margin, W-margin) x [margin, H-margin), row-major; raydirs (n_t,R,3) = get_dtu_raydir
 * (data_augment_utils.py:410-424) with intrinsic_rows = rows 0,1 of intrinsic[:2]/ratio as a device (2,3) array and
 * camrotc2w (n_frames,3,3); lightpos (n_t,R,3) = cam_lightpos[frame] repeated (formating.py:70-75); gt_images
 * (n_t,R,3) = the de-normalised BGR frame / 255 at the ray's pixel (multi_view.py:147-150). */
int ndet_target_rays(const uint8_t* frames_bgr, const int* target_ids, int n_targets, int H, int W, int margin,
                     const float* intrinsic_rows, const float* camrotc2w, const float* cam_lightpos, const double* mean_rgb,
                     const double* std_rgb, float* raydirs, float* lightpos, float* gt_images, void* stream);

/* ndet_resize_normalize_views: the same contract from frames at CAPTURE resolution, frames_bgr (n_frames,Hs,Ws,3) uint8 BGR -- the
 * configs' Resize(keep_ratio) -> Normalize -> Pad (configs/nerfdet/nerfdet_res101_2x_low_res.py:95-97, applied per view by
 * mmdet3d/datasets/pipelines/multi_view.py:90-110) in one launch.  For each selected frame ids[v] (ids == NULL: frames 0 .. n_sel-1):
 *   content [0,Hr) x [0,Wr) of the H x W outputs: the byte of nerfdet_amd.datasets.imresize_linear(frame, (Wr, Hr)) bit for bit
 *     (cv2.INTER_LINEAR: two taps per axis at float32(float64((d + 0.5) * (src / dst) - 0.5)), clamped at the borders, 11-bit
 *     fixed-point weights, two-stage rounding; Hr == Hs && Wr == Ws is a copy; upscaling is allowed), then ndet_normalize_views'
 *     float32 arithmetic on that byte: img RGB planes, denorm BGR planes;
 *   pad, the rest: img = 0.0f (Pad follows Normalize), denorm = (float)(unsigned char)(int)mean_c / 255.0f, resized_bgr = 0.
 * img, denorm (n_sel,3,H,W); resized_bgr NULL or (n_sel,H,W,3) uint8.  Every element of every output is written.  Frame offsets are
 * 64-bit.  Refused before any device work: a null pointer other than ids / resized_bgr, a non-positive size, std <= 0, Hr > H or
 * Wr > W (NDET_E_INVALID); Hs * Ws * 3 >= 2^31 or H * W * 3 >= 2^31 (NDET_E_UNSUPPORTED). */
int ndet_resize_normalize_views(const uint8_t* frames_bgr, const int* ids, int n_sel, int Hs, int Ws, int Hr, int Wr, int H, int W,
                                const double* mean_rgb, const double* std_rgb, float* img, float* denorm, uint8_t* resized_bgr,
                                void* stream);

/* ---- NV12 surfaces: what a hardware video decoder leaves in device memory and a hardware encoder takes.  A surface batch is
 * surfaces (n, rows, pitch) uint8: the Y plane in rows [0,Hs), the interleaved U,V plane (U first) in rows [uv_row, uv_row + Hs/2),
 * columns [0,Ws) of each row used; tight: pitch = Ws, uv_row = Hs, rows = Hs * 3 / 2.  The colour definition is
 * nerfdet_amd.datasets.nv12_to_bgr / bgr_to_nv12 (BT.601 limited range in 20-bit fixed point, nearest chroma on ingest, the rounded
 * 2 x 2 mean on egress), bit for bit.
 *
 * ndet_resize_normalize_views_nv12: ndet_resize_normalize_views' contract -- the configs' Resize(keep_ratio) -> Normalize -> Pad
 * (configs/nerfdet/nerfdet_res101_2x_low_res.py:95-97, applied per view by mmdet3d/datasets/pipelines/multi_view.py:90-110) -- reading
 * surfaces: img, denorm and resized_bgr are what ndet_resize_normalize_views writes for nv12_to_bgr of each selected surface, bit for
 * bit; ids, the pad and mean / std as there.  Each of the four taps converts its own source pixel, Y at (y, x) and the UV pair at
 * (y >> 1, x >> 1), before the 2^11 fixed-point blend.  Frame offsets are 64-bit, offsets inside a surface 32-bit.  Refused before any
 * device work: a null pointer other than ids / resized_bgr, a non-positive size, std <= 0, Hr > H or Wr > W, odd Hs or Ws, pitch < Ws,
 * uv_row < Hs, rows < uv_row + Hs/2 (NDET_E_INVALID); rows * pitch >= 2^31, H * W * 3 >= 2^31, 2^31 workgroups or more, an odd pitch
 * or an odd base address -- the UV pair is one 16-bit load -- (NDET_E_UNSUPPORTED). */
int ndet_resize_normalize_views_nv12(const uint8_t* surfaces, const int* ids, int n_sel, int Hs, int Ws, int pitch, int uv_row, int rows,
                                     int Hr, int Wr, int H, int W, const double* mean_rgb, const double* std_rgb, float* img, float* denorm,
                                     uint8_t* resized_bgr, void* stream);

/* ndet_nv12_to_bgr: frames_bgr (n_sel,Hs,Ws,3) uint8 = nv12_to_bgr of each selected surface ids[v] (ids == NULL: 0 .. n_sel-1) at full
 * size, for what needs capture-size BGR (drawing onto camera frames; the frames are those the configs' LoadImageFromFile hands to
 * mmdet3d/datasets/pipelines/multi_view.py:90).  One thread per 2 x 2 block; every output byte is written.  Refusals as above, and
 * Hs * Ws * 3 >= 2^31 (NDET_E_UNSUPPORTED). */
int ndet_nv12_to_bgr(const uint8_t* surfaces, const int* ids, int n_sel, int Hs, int Ws, int pitch, int uv_row, int rows,
                     uint8_t* frames_bgr, void* stream);

/* ndet_bgr_to_nv12: tight surfaces (n, He * 3 / 2, We) = bgr_to_nv12 of frames_bgr (n,H,W,3) of ANY size: He = H + H % 2,
 * We = W + W % 2, surface pixel (r, c) reads frame[min(r, H-1), min(c, W-1)] -- the inverse direction of the same contract
 * (multi_view.py:107-110 keeps BGR bytes; an encoder takes NV12).  One thread per 2 x 2 block writes four Y bytes and one UV pair; every
 * output byte is written.  Refused before any device work: a null pointer, a non-positive size (NDET_E_INVALID); H * W * 3 >= 2^31
 * (NDET_E_UNSUPPORTED). */
int ndet_bgr_to_nv12(const uint8_t* frames_bgr, int n, int H, int W, uint8_t* surfaces, void* stream);

/* ---- depth frames: the loader's `depth`, `gt_depths` and `depth_rays` from the sensor's frames, frames_mm (n_frames,Hd,Wd) uint16
 * millimetres resident on the device.
 *
 * ndet_depth_frames: for each selected frame ids[v] (ids == NULL: frames 0 .. n_sel-1) the map
 * nerfdet_amd.datasets.imresize_linear(frame / 1000, (w, h)) in float64, bit for bit -- mmcv.imresize of the float64 metres, as
 * mmdet3d/datasets/pipelines/multi_view.py:98-105 resizes a selected view's depth to the meta's img_shape and multi_view.py:156-166 a
 * target view's to gt_rgb_shape, the PADDED image size -- of which only the crop [margin, h-margin) x [margin, w-margin) is computed
 * and stored: out (n_sel, h-2*margin, w-2*margin) float64, every element written.  Each tap is double(u16) / 1000.0; positions
 * float32(float64((d + 0.5) * (src / dst) - 0.5)), floor, both border clamps; weight f float32 widened to float64, 1 - f formed in
 * float64; a * (1 - fx) + b * fx per source row, then h0 * (1 - fy) + h1 * fy; every product and sum rounded on its own (no FMA);
 * h == Hd && w == Wd is the copy frame / 1000.  Frame offsets are 64-bit, offsets inside a frame or a map 32-bit.  Refused before any
 * device work: a null pointer other than ids, a non-positive size, margin < 0 or a margin that leaves no pixel (NDET_E_INVALID);
 * Hd * Wd >= 2^31 or (h-2*margin) * (w-2*margin) >= 2^31 (NDET_E_UNSUPPORTED). */
int ndet_depth_frames(const uint16_t* frames_mm, const int* ids, int n_sel, int Hd, int Wd, int h, int w, int margin, double* out,
                      void* stream);

/* ndet_positive_indices: the rays WITH depth of the training-time ray draw, render_ray.py:386-404 (torch.nonzero(gt_depth > 0)) and
 * nerfdet_amd/datasets.py:293 (np.flatnonzero on the loader's side): indices[0 .. K) = the i with x[i] > 0 in ascending order, int64,
 * and count[0] = K, for x (n) float64 on the device; NaN, zeros of either sign and negative values are left out; indices[K .. n) is
 * not written.  ONE kernel launch behind a memset node that zeroes the workspace (ndet_positive_indices_workspace_bytes(n) bytes
 * of device memory, 16-byte aligned, contents irrelevant on entry): a single-pass scan over tiles of 256 elements; no atomic decides
 * where an index goes, so two calls on the same x write the same bytes.  Waits inside the kernel are bounded: should one run out,
 * count[0] = -1 and indices is unspecified.  indices holds n elements; count is a device int64.  Refused before any device work: a
 * null pointer, n <= 0, a misaligned workspace (NDET_E_INVALID); n >= 2^31 (NDET_E_UNSUPPORTED). */
int ndet_positive_indices(const double* x, int64_t n, int64_t* indices, int64_t* count, void* workspace, void* stream);

/* ---- frames out: a pose in, uint8 BGR and uint16 millimetre frames out, and a render compared with a held-out frame on the device.
 * Every entry point checks its arguments on the host before any HIP call: a null pointer (other than the optional ones named below) or
 * a non-positive size is NDET_E_INVALID, 2^31 elements or more and a misaligned pointer are NDET_E_UNSUPPORTED.
 *
 * ndet_camera_rays: get_dtu_raydir (mmdet3d/datasets/pipelines/data_augment_utils.py:410-424, un-normalised, as multi_view.py:117-155
 * calls it) for n_cams cameras that share intrinsic_rows, a device (2,3) array (rows 0,1 of the intrinsics at the image grid's scale),
 * with camrotc2w (n_cams,3,3) and cam_lightpos (n_cams,3) on the device.  Output pixel (i, j) of camera c looks through image pixel
 * px = x0 + j * stride, py = y0 + i * stride: x = ((float)px + 0.5f - k[2]) / k[0], y = ((float)py + 0.5f - k[5]) / k[4],
 * ray_d[c][i * w + j][r] = fmaf(y, R[r][1], x * R[r][0]) + R[r][2] -- ndet_target_rays' arithmetic in its operation order, bit for bit --
 * and ray_o the camera centre repeated (formating.py:70-75); both (n_cams, h * w, 3) float32.  No frame and no image bound: a pose may
 * look anywhere.  stride >= 1, x0, y0 >= 0, n_cams, h, w >= 1 (else NDET_E_INVALID); n_cams * h * w * 3 >= 2^31 or a pixel coordinate
 * of 2^31 or more: NDET_E_UNSUPPORTED. */
int ndet_camera_rays(const float* intrinsic_rows, const float* camrotc2w, const float* cam_lightpos, int n_cams, int x0, int y0, int stride,
                     int h, int w, float* ray_o, float* ray_d, void* stream);

/* ndet_pack_frames: a render as the formats the input side takes (the reference writes np.uint8(img * 255.0),
 * mmdet3d/models/model_utils/save_rendered_img.py:68).  rgb (R,3) float32, depth (R) float32 metres, mask (R) bool or NULL (all true) ->
 * bgr_u8 (R,3) uint8, depth_mm (R) uint16.  Byte, in float32: v = x * 255.0f; NaN and v < 0 give 0, v > 255 gives 255, else
 * (uint8)(int)(v + 0.5f).  The channel order is kept: composited from a view bank the three columns are B, G, R already.  Depth:
 * d = depth * 1000.0f; NaN and d < 0 give 0, d > 65535 gives 65535, else (uint16)(int)(d + 0.5f); 0 where mask is false -- a depth of 0
 * is a hole, as in the sensor's frames.  R * 3 >= 2^31: NDET_E_UNSUPPORTED. */
int ndet_pack_frames(const float* rgb, const float* depth, const uint8_t* mask, int64_t R, uint8_t* bgr_u8, uint16_t* depth_mm, void* stream);

/* ndet_frame_errors: frames a against frames b, as integer sums per frame (the reference's compute_psnr and depth error,
 * mmdet3d/models/model_utils/save_rendered_img.py:10-19,55, on the bytes).  a, b (n, px, 3) uint8; da, db (n, px) uint16 millimetres, db may
 * be NULL; out (n,4) int64 on the device: sse = sum (a - b)^2 over the three bytes of every pixel with da != 0; n_px, the number of those
 * pixels; sad_mm = sum |da - db| over the pixels with da != 0 && db != 0; n_depth, their number (both 0 without db).  A memset node in
 * front of the launch zeroes out; a wave reduction and one 64-bit vector atomic add per workgroup and sum follow -- integers, so exact and the
 * same bytes in any order.  n * px * 3 >= 2^31: NDET_E_UNSUPPORTED. */
int ndet_frame_errors(const uint8_t* a, const uint8_t* b, const uint16_t* da, const uint16_t* db, int n, int64_t px, int64_t* out,
                      void* stream);

/* ndet_frame_ssim: the structural similarity of frames a (a render) and b (held-out frames), as integer sums per frame and channel (the
 * reference's compute_ssim, mmdet3d/models/model_utils/save_rendered_img.py:21-36,51-78 -> skimage.metrics.structural_similarity of
 * scikit-image 0.18.1 with multichannel=True: 7 x 7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03, data range 2 on float images,
 * the mean over the window-valid interior).  a, b (n, h, w, 3) contiguous, uint8 (kind 0) or float32 (kind 1); depth_a (n, h, w) uint16 or
 * NULL; out (n,4) int64 on the device: Q_0, Q_1, Q_2, n_w.  Per frame and channel the windows are the (h-6)(w-6) valid 7 x 7 windows; a
 * window COUNTS iff all its 49 pixels have depth_a != 0 (every window without depth_a).  For a counting window, with Sx, Sy, Sxx, Syy, Sxy
 * the sums over its 49 pixels of one channel (kind 0: exact integers of the bytes),
 *     C1 = (0.01*2*255)^2 * 49^2, C2 = (0.03*2*255)^2 * 49*48      (kind 1: without the 255 factors), float64
 *     A1 = (double)(2 Sx Sy) + C1                A2 = (double)(2 (49 Sxy - Sx Sy)) + C2
 *     B1 = (double)(Sx^2 + Sy^2) + C1            B2 = (double)(49 Sxx - Sx^2 + 49 Syy - Sy^2) + C2
 *     s = (A1 A2) / (B1 B2)  in IEEE float64, one rounding per operation;    q = llrint(s * 2^40), ties to even
 * and Q_c = sum of q over the counting windows of channel c, n_w their number: SSIM_c = Q_c / (2^40 n_w).  Integer sums, so kind 0 gives
 * the same bytes for any tile shape and atomic order.  Kind 1 forms every window's sums in float64 in one fixed order (each row's 7 terms
 * left to right, then the 7 row sums top to bottom; a product of two float32 is exact): the same bytes call to call and at any place in
 * the batch.  A memset node in front of the launch zeroes out.  n < 1, h or w below 7, a kind other than 0 and 1: NDET_E_INVALID;
 * (h-6)(w-6) >= 2^22 (keeps |Q_c| < 2^62), n * h * w * 3 >= 2^31, a misaligned depth_a or out, misaligned float32 frames:
 * NDET_E_UNSUPPORTED. */
int ndet_frame_ssim(const void* a, const void* b, const uint16_t* depth_a, int kind, int n, int h, int w, int64_t* out, void* stream);

/* ---- detections out: the 3D boxes of a detection result in a camera's image -- projected, drawn onto a frame, matched to a depth frame.
 * Every entry point checks its arguments on the host before any HIP call: a null pointer, a non-positive size, stride < 1, a negative
 * offset, near <= 0 and a thickness other than 1, 3, 5 are NDET_E_INVALID; 2^31 elements or more, a misaligned pointer and more boxes than
 * an int16 label holds are NDET_E_UNSUPPORTED.  Plain vector stores, no global atomics; nothing is read back.
 *
 * ndet_project_boxes: the corners of n boxes, (n,8,3) float32 in the order of DepthInstance3DBoxes.corners
 * (mmdet3d/core/bbox/structures/depth_box3d.py:46-84), through k world-to-camera matrices world2cam (k,3,4) and the intrinsic rows (2,3) of
 * ndet_camera_rays (the skew entry is ignored, as there) onto ndet_camera_rays' grid: output pixel (i, j) is image pixel
 * (y0 + i * stride, x0 + j * stride), an image pixel px covers [px, px + 1) and has its centre at px + 0.5.  One thread per (pose, box),
 * float32 in this statement order (the library is built with -ffp-contract=off, every fused step is an fmaf):
 *   camera point   q_r = fmaf(E[r][2], Z, fmaf(E[r][1], Y, E[r][0] * X)) + E[r][3]  for the rows r = 0, 1, 2 of the pose's matrix E;
 *   the 12 edges   (0,1) (1,2) (2,3) (3,0), (4,5) (5,6) (6,7) (7,4), (0,4) (1,5) (2,6) (3,7) as corner pairs.  An end survives iff
 *       z >= near (a NaN fails).  An edge whose ends both fail is dropped; if exactly one fails it moves to the near plane: with a the
 *       surviving and b the failing end t = (near - z_a) / (z_b - z_a), x = fmaf(t, x_b - x_a, x_a), y likewise, z = near;
 *   pixel          u = fmaf(k[0], x / z, k[2]), v = fmaf(k[4], y / z, k[5]); xo = (u - ((float)x0 + 0.5f)) / (float)stride + 0.5f, yo likewise
 *       with y0.  A NaN in any of an edge's four coordinates drops the edge; else each is clamped to [-2^20, 2^20] (which only keeps
 *       ndet_draw_boxes' integers in range: a line that leaves that square is bent at its border) and (int)floorf is taken.
 * Outputs: edges (k,n,12,4) int32 = x_a, y_a, x_b, y_b per edge in the edge's own corner order, zeros for a dropped edge; edge_mask (k,n)
 * int32, bit e set iff edge e survives; rect (k,n,4) int32 = inclusive xmin, ymin, xmax, ymax of the surviving edges' ends intersected with
 * [0,w) x [0,h), four -1 when nothing survives or nothing is left; zrange (k,n,2) float32 = the least and the largest camera z of the eight
 * unclipped corners (a NaN z is passed over unless all are).  edges and rect must be 16-byte aligned. */
int ndet_project_boxes(const float* intrinsic_rows, const float* world2cam, const float* corners, int k, int n, int x0, int y0, int stride, int h,
                       int w, float near_m, int32_t* edges, int32_t* edge_mask, int32_t* rect, float* zrange, void* stream);

/* ndet_draw_boxes: the wireframes of ndet_project_boxes' edges onto frames -- the reference draws its results nowhere; the boxes are the
 * result's, mmdet3d/models/dense_heads/imvoxel_head_v2.py:544.  frames_in (k,h,w,3) uint8 is only read; frames_out, a buffer that does
 * not overlap it, gets every pixel: the input bytes, or -- where an edge covers the pixel -- colours[b] (n,3) uint8 of the HIGHEST box index
 * b with a covering edge (hand the boxes over by ascending score and the best detection wins).  A gather per pixel: one workgroup per
 * 16 x 16 tile scans the frame's 12 n edges in batches of 256, keeps in LDS those that can reach the tile, and each thread tests its pixel.
 * Coverage is integer-exact, thickness t in {1, 3, 5}, r = (t - 1) / 2; for an edge with a = x_b - x_a, b = y_b - y_a:
 *   x-major, |a| >= |b| and a != 0: with the ends swapped so that a > 0, for x_a <= x <= x_b the line passes
 *       yl = y_a + floor((2 b (x - x_a) + a) / (2 a))  (floor division in int64) and covers (x, y) iff |y - yl| <= r;
 *   y-major, |b| > |a|: the same with x and y exchanged;  a = b = 0: the pixels x = x_a, |y - y_a| <= r.
 * Edges whose bit in edge_mask (k,n) is clear paint nothing. */
int ndet_draw_boxes(const uint8_t* frames_in, const int32_t* edges, const int32_t* edge_mask, const uint8_t* colours, int k, int h, int w, int n,
                    int thickness, uint8_t* frames_out, void* stream);

/* ndet_project_boxes_w: ndet_project_boxes -- the same arguments, checks and statement order, its four outputs bit for bit (the corners
 * are DepthInstance3DBoxes.corners, mmdet3d/core/bbox/structures/depth_box3d.py:46-84) -- plus edge_w (k,n,12,2) float32 for
 * ndet_draw_overlay's depth test: for a surviving edge, in the edge's own corner order, 1.0f / z of either end AFTER the near clip (a
 * clipped end has z = near); two zeros for a dropped edge.  edge_w must be 8-byte aligned (NDET_E_UNSUPPORTED), a null edge_w is
 * NDET_E_INVALID. */
int ndet_project_boxes_w(const float* intrinsic_rows, const float* world2cam, const float* corners, int k, int n, int x0, int y0, int stride, int h,
                         int w, float near_m, int32_t* edges, int32_t* edge_mask, int32_t* rect, float* zrange, float* edge_w, void* stream);

/* ndet_draw_overlay: ndet_draw_boxes with an optional depth test of the edges and optional text plates, one launch, new frames (the
 * boxes are the result's, mmdet3d/models/dense_heads/imvoxel_head_v2.py:544; the reference draws nothing).  frames_in, edges, edge_mask,
 * colours, thickness and frames_out are ndet_draw_boxes', with its line rule.  Two optional argument groups, each whole or all null:
 * depth_mm (k,h,w) uint16 millimetres + edge_w (k,n,12,2) of ndet_project_boxes_w;  rect (k,n,4) of ndet_project_boxes + text (n,32) uint8
 * codes + text_len (n) int32 + font (96,7) uint8.  With both groups null the output is ndet_draw_boxes' bit for bit.
 *   Edge depth at a covered pixel: where the line rule swaps an edge's ends, their w swap with them.  With P the pixel's major-axis
 *       coordinate, p0 and p1 the ends' and a = p1 - p0 > 0:  s = (float)(P - p0) / (float)a,  w_p = fmaf(s, w_1 - w_0, w_0);  a = 0 (a
 *       point edge): w_p = w_0, the first end in corner order;  e_mm = (1.0f / w_p) * 1000.0f.  Every pixel a thick line covers uses
 *       its own P and its own millimetres.  1/z is linear on the screen, but s comes from integer cells: it is off by up to a pixel's
 *       worth along the edge, and more at an end bent by ndet_project_boxes' 2^20 clamp -- bias_mm is there to absorb that.
 *   Hidden: a covered pixel of an edge is hidden iff mm != 0 && (float)mm + bias_mm < e_mm.  A hole hides nothing; 65535 is a value
 *       like any other.  Without depth_mm nothing is hidden.
 *   Winner without a plate: bv = the highest box index with a visible covering edge, bh = the highest with a hidden one.  bv >= 0: the
 *       pixel is colours[bv] (a visible edge beats a hidden one of any index); else occluded == 1 (dim) and bh >= 0: each channel is
 *       (3 * in + colours[bh][c] + 2) >> 2; else the input byte (occluded == 0: hide).
 *   Plates: box b of pose p has one iff rect[p][b].x >= 0 and len = clamp(text_len[b], 0, 32) > 0.  With S = text_scale in {1, 2, 3}:
 *       pw = S (6 len + 1), ph = 9 S, px0 = min(xmin, max(w - pw, 0)), py0 = max(ymin - ph, 0), clipped to the frame.  For a pixel inside
 *       u = (x - px0) / S, v = (y - py0) / S, c = u - 1, r = v - 1, g = c / 6, gc = c - 6 g; it is ink iff c >= 0 && 0 <= r <= 6 &&
 *       gc < 5 && g < len and bit (4 - gc) of font[glyph][r] is set, glyph = code - 32 for 32 <= code <= 127 (code = text[b][g]), else 95.
 *       A pixel under any plate takes the plate of the HIGHEST box index, ahead of every edge and never depth-tested: colours[b], or
 *       for ink black where (29 B + 150 G + 77 R + 128) >> 8 >= 128 of that colour, else white.
 * One workgroup per 16 x 16 tile; plates and edges are staged through LDS 256 at a time, the font once.  On the host, before any HIP call:
 * ndet_draw_boxes' refusals, an incomplete group, occluded not 0 or 1, bias_mm negative, NaN or infinite, text_scale outside 1..3 with
 * plates: NDET_E_INVALID; 2^31 elements, 2^24 workgroups, a misaligned edge_w (8 bytes), rect (16), depth_mm (2), text_len (4):
 * NDET_E_UNSUPPORTED. */
int ndet_draw_overlay(const uint8_t* frames_in, const int32_t* edges, const int32_t* edge_mask, const uint8_t* colours, const uint16_t* depth_mm,
                      const float* edge_w, float bias_mm, int occluded, const int32_t* rect, const uint8_t* text, const int32_t* text_len,
                      const uint8_t* font, int text_scale, int k, int h, int w, int n, int thickness, uint8_t* frames_out, void* stream);

/* ndet_label_frames: which detection each pixel of a depth frame belongs to.  depth_mm (k,h,w) uint16 millimetres (0: a hole) on
 * ndet_camera_rays' grid x0, y0, stride with its intrinsic_rows (2,3), camrotc2w (k,3,3) and cam_lightpos (k,3); box_frames (n,8) float32 =
 * centre (3), half extents (3), cos yaw, sin yaw, n <= 32767.  A pixel with mm != 0 looks along d, ndet_camera_rays' expression statement
 * for statement (get_dtu_raydir, mmdet3d/datasets/pipelines/data_augment_utils.py:410-424); its point is z = (float)mm / 1000.0f,
 * p_j = fmaf(z, d_j, lpos_j); in a box's frame, with (dx, dy, dz) = p - centre, lx = fmaf(dx, cos, -(dy * sin)), ly = fmaf(dx, sin, dy * cos)
 * -- the inverse of the corners' yaw; the box holds the point iff |lx| <= hx && |ly| <= hy && |dz| <= hz.  labels (k,h,w) int16: the
 * highest index among the boxes that hold the point, -1 for none and for mm = 0.  One thread per pixel, the boxes staged through LDS 256 at
 * a time. */
int ndet_label_frames(const uint16_t* depth_mm, const float* intrinsic_rows, const float* camrotc2w, const float* cam_lightpos,
                      const float* box_frames, int k, int h, int w, int n, int x0, int y0, int stride, int16_t* labels, void* stream);

/* Workspace of ndet_positive_indices for n elements (render_ray.py:386-404), in bytes; 0 for an n the entry point refuses. */
int64_t ndet_positive_indices_workspace_bytes(int64_t n);

/* Weight-gradient staging for the training-time convolutions (autograd of nn.Conv3d / nn.Conv2d in
 * mmdet3d/models/necks/imvoxelnet.py:22-67,233-260 and of the third-party ResNet/FPN layers): channels-last x (D,H,W,C) -> rows
 * out[t - t0][c][j] = x[stride * o(j) + tap(t) - pad][c] over the flattened OUTPUT grid of the (kernel, stride, pad) convolution, taps
 * t0 .. t0+n_taps-1; every element of out (n_taps, C, lrow) is written (zeros where the tap reads padding and for j past the grid;
 * lrow >= OD*OH*OW).  With these rows (and dY staged by the same call with a 1x1x1 kernel) the weight gradient is one GEMM over j on
 * ndet_conv_split, for any stride (nerfdet_amd/conv_train.py). */
int ndet_wgrad_rows(const float* x_ndhwc, int D, int H, int W, int C, const int* kernel, const int* stride, const int* pad, int t0,
                    int n_taps, int lrow, float* out, void* stream);

/* Weight gradient of a convolution as ONE implicit GEMM (autograd of nn.Conv3d / nn.Conv2d in
 * mmdet3d/models/necks/imvoxelnet.py:22-67,233-260 and of the ResNet / FPN layers): dw_rows[(t, ci)][co] = sum over output voxels j of
 * x[stride * o(j) + tap(t) - pad][ci] * dy[j][co].  x (D,H,W,Cin) channels-last fp32 is read in place (transposed on its way into
 * LDS); dy arrives as the bf16 planes of its channel-major rows: ndet_wgrad_rows(dy, 1x1x1) -> (Cout, lrow), then
 * ndet_split_weights_bf16x3 on that (1, Cout, lrow) "weight".  dw_rows (taps * Cin, Cout) row-major; Cin % 64 == 0, lrow % 32 == 0;
 * splits > 1: workspace of splits * taps * Cin * Cout floats, reduced in a fixed order (keep_partials = 1: left there for ndet_wgrad_to_torch,
 * dw_rows not written).  arith as NdetConvArgs::arith: 0 six products, 2 one (bf16); 1 fp16 pairs -- dy_planes from ndet_wgrad_dy_planes_f16x2
 * (two planes per K step, scaled by the slot dy_amax), x split in the kernel under the scale of the slot x_amax, three products, the sums
 * multiplied by the inverse of both scales; the two slots are required with arith 1 and null otherwise. */
int ndet_wgrad_split(const float* x_ndhwc, int D, int H, int W, int Cin, const int* kernel, const int* stride, const int* pad,
                     const uint16_t* dy_planes, int Cout, int lrow, int splits, int arith, const float* x_amax, const float* dy_amax,
                     void* workspace, float* dw_rows, int keep_partials, void* stream);

/* dY of a convolution (L output voxels x Cout, channels-last fp32) -> the bf16 planes of its channel-major rows in the layout of
 * ndet_split_weights_bf16x3 for a (1, Cout, lrow) "weight": (lrow/32, 3, Cout, 32), zeros past L -- the "weight" operand of the
 * weight-gradient GEMMs (ndet_wgrad_split, or ndet_conv_split on ndet_wgrad_rows' tap copies) in one pass; autograd of nn.Conv3d /
 * nn.Conv2d in mmdet3d/models/necks/imvoxelnet.py:22-67,233-260 and of the ResNet / FPN layers. */
int ndet_wgrad_dy_planes(const float* dy_rows_by_voxel, int L, int Cout, int lrow, uint16_t* planes, void* stream);

/* fp16-pair form of the call above (the training step on the three-product arithmetic): dy's planes are (lrow/32, 2, Cout, 32), two fp16
 * halves of dy * 2^k with 2^k taken ON THE DEVICE from dy's amax slot (ndet_amax_f32; largest magnitude in [2^14, 2^15)) -- the operand of
 * ndet_wgrad_split with arith 1.  Same reference: autograd of nn.Conv3d / nn.Conv2d in mmdet3d/models/necks/imvoxelnet.py:22-67,233-260 and of
 * the ResNet / FPN layers. */
int ndet_wgrad_dy_planes_f16x2(const float* dy_rows_by_voxel, int L, int Cout, int lrow, const float* dy_amax, uint16_t* planes, void* stream);

/* Both weight packs of one training step in ONE pass over a torch-layout weight (Cout, Cin, taps <= 27): planes = the layer's own
 * (taps, Cin/32, P, Cout, 32), planes_adjoint (may be null) = its data gradient's (taps, ceil32(Cout)/32, P, Cin, 32), W'[t][ci][co] = W[co][ci][taps-1-t]
 * (see ndet_split_weights_bf16x3_torch).  arith 0: P = 3 bf16 planes (w_amax null).  arith 1: P = 2 fp16 planes of w * 2^k, 2^k derived on the
 * device from the weight's amax slot w_amax (ndet_amax_f32) -- the optimizer moves the weights every step
 * (config nerfdet_res50_2x_low_res.py:167-172, AdamW), and no maximum has to reach the host for it.  A workgroup moves a 32 x 32 (co, ci) block with
 * all its taps through LDS: coalesced reads of the torch layout, every (tap, plane) of either pack written as one 2 KB piece. */
int ndet_split_weights_train(const float* w_torch, int taps, int Cout, int Cin, int arith, const float* w_amax, uint16_t* planes,
                             uint16_t* planes_adjoint, void* stream);

/* BatchNorm on BATCH statistics over channels-last rows (N x C fp32, C / 4 a divisor of 1024), with the ReLU and the residual add that follow it in
 * BasicBlock3dV2 / the up and out blocks of FastIndoorImVoxelNeck folded in (mmdet3d/models/necks/imvoxelnet.py:22-67,233-260; training mode of
 * nn.BatchNorm3d): y = relu?((x - mean) / sqrt(var + eps) * gamma + beta (+ residual)), mean / biased var over the N rows; running_mean /
 * running_var (may be null) updated with `momentum` (unbiased variance), save_mean / save_invstd kept for the backward.  y_amax (may be null): a
 * zeroed amax slot that receives max |y|.  workspace: ndet_bn_workspace_floats(N, C) floats.  Three launches (partial sums, finish, apply); the
 * variance is one pass of sums about a pivot per workgroup (the median of three rows of its slice: no single row decides the conditioning),
 * left as the slice's (mean, M2) and joined by the pairwise (n, mean, M2) formula; every sum is added in a fixed order.  The backward:
 * dx = gamma invstd (g - mean(g) - xhat mean(g xhat)) with g = dy [y > 0] when relu (y = the forward's output), d_residual (may be null) = g,
 * dgamma = sum g xhat, dbeta = sum g; dx_amax as y_amax. */
int64_t ndet_bn_workspace_floats(int64_t N, int C);
int ndet_bn_train_forward(const float* x, int64_t N, int C, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, const float* residual, int relu, float* y, float* save_mean, float* save_invstd, float* y_amax,
                          float* workspace, void* stream);
int ndet_bn_train_backward(const float* dy, const float* x, const float* y, int64_t N, int C, const float* gamma, const float* save_mean,
                           const float* save_invstd, int relu, float* dx, float* d_residual, float* dgamma, float* dbeta, float* dx_amax,
                           float* workspace, void* stream);

/* The weight gradient in torch's layout: dw_rows ((tap, ci) rows x Cout floats, what ndet_wgrad_split and the staged GEMM write) ->
 * dw_torch (Cout, Cin, taps), the layout autograd hands to the optimizer for nn.Conv3d / nn.Conv2d.weight
 * (mmdet3d/models/necks/imvoxelnet.py:22-67,233-260).  32 x 32 x taps blocks through LDS, coalesced on both sides; taps <= 27, Cin % 32 == 0.
 * splits > 1: dw_rows is the split-K WORKSPACE of a launch made with keep_partials = 1 (ndet_conv_split, ndet_wgrad_split) -- `splits`
 * partial sums taps * Cin * Cout floats apart, added here in index order (what the separate reduction pass would have done, bit for bit). */
int ndet_wgrad_to_torch(const float* dw_rows, int splits, int taps, int Cout, int Cin, float* dw_torch, void* stream);

/* Backward of the fused epilogue y = relu(conv * scale + shift (+ identity)) -- convolution + frozen eval-mode BatchNorm + ReLU (+ the
 * bottleneck's identity) of the trainable ResNet stages (mmdet Bottleneck.forward behind mmdet3d/models/detectors/nerfdet.py:140;
 * config: norm_eval=True, norm_cfg.requires_grad=False): d_identity = dy [y > 0] (null = not wanted), d_conv = d_identity * scale[c],
 * one pass over `rows` channels-last rows of C floats (C % 4 == 0).  relu = 0: no mask (y may be null). */
int ndet_relu_affine_bwd(const float* dy, const float* y, const float* scale, int64_t rows, int C, int relu, float* d_identity,
                         float* d_conv, void* stream);
/* ndet_relu_affine_bwd that also leaves max |d_conv| in the zeroed 1 KiB amax slot d_conv_amax (see ndet_amax_f32): d_conv is the operand of the
 * layer's data and weight gradients, whose fp16-pair launches take their scale from that slot.  Same reference: mmdet Bottleneck.forward behind
 * mmdet3d/models/detectors/nerfdet.py:140 under norm_eval=True. */
int ndet_relu_affine_bwd_amax(const float* dy, const float* y, const float* scale, int64_t rows, int C, int relu, float* d_identity,
                              float* d_conv, float* d_conv_amax, void* stream);

/* ---- backward passes (training).  The reference obtains these from autograd over its materialised tensors; each
 * entry point names the forward statement it differentiates.  Scatter targets must be zero-initialised by the caller;
 * accumulation uses float atomics (order not fixed). ---- */

/* d(features) of the view mean, mmdet3d/models/detectors/nerfdet.py:164-176: grad_features[v,y,x,:] += grad_mean[n,:] /
 * (count_n + 1e-8) for every view v that sees voxel n.  grad_mean in `grad_layout`; grad_features_nhwc as features_nhwc. */
int ndet_backproject_aggregate_bwd(const float* grad_mean, int grad_layout, int n_views, int C, int h, int w,
                                   int64_t view_pitch, int64_t row_pitch, const float* points, int N,
                                   const float* projection, float* grad_features_nhwc, void* stream);

/* d(mapped features), d(bias) of ndet_density_features, nerfdet.py:234-253 (the RGB volume carries no gradient). */
int ndet_density_features_bwd(const float* grad_global_feat, const float* mapped_nhwc, int n_views, int cm, int h, int w,
                              int64_t mview_pitch, int64_t mrow_pitch, const float* bias, const float* points, int N,
                              const float* projection, float* grad_mapped_nhwc, float* grad_bias, void* stream);

/* ndet_backproject_aggregate_bwd over the depth-gated validity of nerfdet.py:404-411 (gate->depth_f at h x w). */
int ndet_backproject_aggregate_bwd_gated(const float* grad_mean, int grad_layout, int n_views, int C, int h, int w,
                                         int64_t view_pitch, int64_t row_pitch, const float* points, int N,
                                         const float* projection, float* grad_features_nhwc, const NdetDepthGate* gate,
                                         void* stream);

/* ndet_density_features_bwd over the depth-gated stride-4 validity of nerfdet.py:404-411 (gate->depth_f at h x w). */
int ndet_density_features_bwd_gated(const float* grad_global_feat, const float* mapped_nhwc, int n_views, int cm, int h, int w,
                                    int64_t mview_pitch, int64_t mrow_pitch, const float* bias, const float* points, int N,
                                    const float* projection, float* grad_mapped_nhwc, float* grad_bias,
                                    const NdetDepthGate* gate, void* stream);

/* d(mapped features) of ndet_ray_view_stats: F.grid_sample backward (projection.py:127) through the masked statistics of
 * render_ray.py:83-88.  Sample points and images carry no gradient. */
int ndet_ray_view_stats_bwd(const float* grad_global_feat, const float* pts, int n_points, const float* KE, int n_views,
                            float img_h, float img_w, const float* feat_nhwc, int d, int hf, int wf,
                            int64_t fview_pitch, int64_t frow_pitch, float* grad_feat_nhwc, void* stream);

/* Packed form of ndet_ray_view_stats_bwd (d % 4 == 0, n_views <= 128): F.grid_sample backward (projection.py:127) through the
 * masked statistics of render_ray.py:83-88; grad_feat_nhwc shares feat_nhwc's pitches and must be zero-initialised. */
int ndet_ray_view_stats_packed_bwd(const float* grad_global_feat, const float* pts, int n_points, const float* KE, int n_views,
                                   float img_h, float img_w, const float* feat_nhwc, int d, int hf, int wf, int64_t fview_pitch,
                                   int64_t frow_pitch, float* grad_feat_nhwc, void* stream);

/* d(raw) of ndet_composite (render_ray.py:196-236) from d(rgb_map) (R,3) and d(depth_map) (R) or NULL.
 * transparency: the forward's (R,S) output. */
int ndet_composite_bwd(const float* raw, const float* z_vals, const float* transparency, int R, int S, int white_bkgd,
                       const float* zminmax, const float* grad_rgb, const float* grad_depth, float* grad_raw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFDET_HIP_H */
