// Shared host/device helpers for libnerfdet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/nerfdet_hip.h"

#define NDET_WAVE 64

// ---- host-side error plumbing ------------------------------------------------------------
void ndet_set_error(const char* fmt, ...);

#define NDET_REQUIRE(cond, code, ...)  \
    do {                               \
        if (!(cond)) {                 \
            ndet_set_error(__VA_ARGS__); \
            return (code);             \
        }                              \
    } while (0)

// ... and for a check that has set the message itself: its error code is the caller's
#define NDET_TRY(call)                    \
    do {                                  \
        const int rc__ = (call);          \
        if (rc__ != NDET_OK) return rc__; \
    } while (0)

#define NDET_CHECK_LAUNCH(name)                                                      \
    do {                                                                             \
        hipError_t e__ = hipGetLastError();                                          \
        if (e__ != hipSuccess) {                                                     \
            ndet_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));   \
            return NDET_E_LAUNCH;                                                    \
        }                                                                            \
    } while (0)

// Raise `kernel`'s dynamic-LDS limit to `bytes`.  The limit is a per-device attribute of the kernel: the runtime is asked once per (kernel,
// current device) -- again only for a larger size -- and its answer, a refusal included, is what every later call returns; a call that
// finds its answer costs one hipGetDevice.  What a refusal means is the caller's business (volume_kernels.hip).
hipError_t ndet_lds_limit(const void* kernel, size_t bytes);

// ... for the launchers to which a refusal is an error (`fn` = the entry point's name, in scope)
#define NDET_RAISE_LDS(kernel, bytes)                                                                                     \
    do {                                                                                                                  \
        const hipError_t e__ = ndet_lds_limit((const void*)(kernel), (bytes));                                            \
        NDET_REQUIRE(e__ == hipSuccess, NDET_E_LAUNCH, "%s: cannot raise the LDS limit: %s", fn, hipGetErrorString(e__)); \
    } while (0)

// ---- device helpers ----------------------------------------------------------------------

// Maximum / minimum / ReLU that carry a NaN, as torch.relu, max_pool, clamp and threshold_backward do ("Non-finite values"):
// IEEE 754-2019 maximum / minimum, one v_maximum3_f32 / v_minimum3_f32 each; for operands that are not NaN the bits of fmaxf / fminf
// (-0 < +0 included).  fmaxf / fminf return the operand that is NOT a NaN: they stay where a max |x| is built, which is by contract
// the maximum over the elements that are not NaN, and nowhere else on a value the reference passes through a maximum.
__device__ __forceinline__ float ndet_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float ndet_min(float a, float b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ float ndet_relu(float v) { return __builtin_elementwise_maximum(v, 0.0f); }
__device__ __forceinline__ float4 ndet_relu4(float4 v) { return make_float4(ndet_relu(v.x), ndet_relu(v.y), ndet_relu(v.z), ndet_relu(v.w)); }
// threshold_backward: the gradient passes unless y <= 0, so it passes where y is NaN
__device__ __forceinline__ float ndet_relu_mask(float y, float g) { return !(y <= 0.0f) ? g : 0.0f; }
__device__ __forceinline__ float4 ndet_relu_mask4(float4 y, float4 g) {
    return make_float4(ndet_relu_mask(y.x, g.x), ndet_relu_mask(y.y, g.y), ndet_relu_mask(y.z, g.z), ndet_relu_mask(y.w, g.w));
}

// Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share one).  Give each XCD a
// contiguous slab of tiles so neighbouring voxel tiles (which hit the same feature pixels)
// share an L2.  Bijective for any n (cdna guide, "XCD swizzle must be bijective").  Speed only.
__device__ __forceinline__ int ndet_xcd_remap(int b, int n) {
    const int q = n >> 3, r = n & 7, x = b & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (b >> 3);
}

// One voxel -> one view, the arithmetic of nerfdet.py:398-403.
//   torch.bmm(P, [p;1]) on the CPU reference evaluates each row as a k-ordered FMA chain
//   acc = p0*x; acc = fma(p1,y,acc); acc = fma(p2,z,acc); acc = acc + p3   (measured: 0 of
//   3.84 M elements differ from MKL sgemm at the cfg2 shapes) -- the same chain is used here,
//   the file is compiled with -ffp-contract=off so nothing else fuses.
//   `/` is IEEE correctly-rounded (hipcc default), rintf = round-half-even = torch.round.
//   Validity is evaluated on the rounded *float* coordinate: equivalent to the reference's
//   int64 cast + compare for every finite value, and NaN / inf / |x| >= 2^63 come out invalid
//   on both sides (x86 cvttss2si yields INT64_MIN there).
__device__ __forceinline__ bool ndet_project_z(const float* __restrict__ P, float px, float py, float pz,
                                               int w, int h, int& xi, int& yi, float& z) {
    float u = P[0] * px;
    u = fmaf(P[1], py, u);
    u = fmaf(P[2], pz, u);
    u = u + P[3];
    float v = P[4] * px;
    v = fmaf(P[5], py, v);
    v = fmaf(P[6], pz, v);
    v = v + P[7];
    float d = P[8] * px;
    d = fmaf(P[9], py, d);
    d = fmaf(P[10], pz, d);
    d = d + P[11];
    const float fx = rintf(u / d);
    const float fy = rintf(v / d);
    const bool ok = (fx >= 0.0f) && (fy >= 0.0f) && (fx < (float)w) && (fy < (float)h) && (d > 0.0f);
    xi = ok ? (int)fx : 0;
    yi = ok ? (int)fy : 0;
    z = d;
    return ok;
}

__device__ __forceinline__ bool ndet_project(const float* __restrict__ P, float px, float py, float pz,
                                             int w, int h, int& xi, int& yi) {
    float z;
    return ndet_project_z(P, px, py, pz, w, h, xi, yi, z);
}

// One sample point -> one source view of the ray branch (projection.py:42-64 + :37-40 + :24-35), for the forward samplers
// (ray_kernels.hip, ray_stats_kernels.hip) and the sampler's backward (backward_kernels.hip).  KE = rows 0..2 of K @ E, in memory or
// in registers; the same k-ordered FMA chain as ndet_project_z.
struct NdetRayHit {
    float nx, ny;  // normalised coordinates in [-1, 1] (projection.py:37-40)
    bool mask;     // in-image and in front (projection.py:149-150)
};

__device__ __forceinline__ NdetRayHit ndet_ray_project(const float* KE, float x, float y, float z, float h, float w) {
    float q0 = KE[0] * x;
    q0 = fmaf(KE[1], y, q0);
    q0 = fmaf(KE[2], z, q0);
    q0 = q0 + KE[3];
    float q1 = KE[4] * x;
    q1 = fmaf(KE[5], y, q1);
    q1 = fmaf(KE[6], z, q1);
    q1 = q1 + KE[7];
    float q2 = KE[8] * x;
    q2 = fmaf(KE[9], y, q2);
    q2 = fmaf(KE[10], z, q2);
    q2 = q2 + KE[11];
    const float den = fmaxf(q2, 1e-8f);                       // torch.clamp(min=1e-8)
    float px = q0 / den, py = q1 / den;
    px = fminf(fmaxf(px, -1e6f), 1e6f);                       // torch.clamp(-1e6, 1e6)
    py = fminf(fmaxf(py, -1e6f), 1e6f);
    NdetRayHit r;
    r.mask = (px <= w - 1.0f) && (px >= 0.0f) && (py <= h - 1.0f) && (py >= 0.0f) && (q2 > 0.0f);
    r.nx = (2.0f * px) / (w - 1.0f) - 1.0f;
    r.ny = (2.0f * py) / (h - 1.0f) - 1.0f;
    return r;
}

// Pixel (px, py) of a camera -> its ray direction, get_dtu_raydir un-normalised (data_augment_utils.py:410-424): kn = rows 0, 1 of the
// intrinsics (2,3), R = the camera-to-world rotation (3,3).  One operation order for every kernel that casts a ray or lifts a pixel.
__device__ __forceinline__ void ndet_pixel_dir(const float* __restrict__ kn, const float* __restrict__ R, int px, int py, float (&dir)[3]) {
    const float x = ((float)px + 0.5f - kn[2]) / kn[0];
    const float y = ((float)py + 0.5f - kn[5]) / kn[4];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float d = x * R[j * 3 + 0];
        d = fmaf(y, R[j * 3 + 1], d);
        d = d + R[j * 3 + 2];
        dir[j] = d;
    }
}

// ... and one axis of the world point at depth z along it
__device__ __forceinline__ float ndet_ray_point(float z, float dir, float centre) { return fmaf(z, dir, centre); }

// Which box holds a point: the highest index among the n boxes (centre, half extents, cos yaw, sin yaw: 8 floats) that hold (x, y, z),
// -1 for none; a NaN fails every test.  The boxes pass through LDS in batches, so all 256 threads of the workgroup call, `on` or not.
#define NDET_BOX_BATCH 256
__device__ __forceinline__ int ndet_box_of_point(const float* __restrict__ boxes, int n, bool on, float x, float y, float z) {
    __shared__ float s_box[NDET_BOX_BATCH * 8];
    int best = -1;
    for (int base = 0; base < n; base += NDET_BOX_BATCH) {
        const int here = min(NDET_BOX_BATCH, n - base);
        __syncthreads();
        for (int j = threadIdx.x; j < here * 8; j += 256) s_box[j] = boxes[(int64_t)base * 8 + j];
        __syncthreads();
        if (on) {
            for (int j = 0; j < here; ++j) {
                const float* B = s_box + j * 8;
                const float dx = x - B[0], dy = y - B[1], dz = z - B[2];
                const float lx = fmaf(dx, B[6], -(dy * B[7]));
                const float ly = fmaf(dx, B[7], dy * B[6]);
                if (fabsf(lx) <= B[3] && fabsf(ly) <= B[4] && fabsf(dz) <= B[5]) best = base + j;
            }
        }
    }
    return best;
}

// Depth gate of nerfdet.py:404-411 (include/nerfdet_hip.h, NdetDepthGate): one resized map, kernel-argument form.  The kernels
// take it under a compile-time flag; their ungated instantiations never read it.
struct NdetGateMap {
    const void* map;      // (n_views, h, w) float or double, element (v,y,x) at v*view_pitch + y*row_pitch + x
    int64_t view_pitch;
    int row_pitch;
    int f64;              // 0: float32 map, 1: float64 map
    double band;          // voxel_size[2]
};

// View v sees the voxel at pixel (xi, yi) with camera depth z iff  D'[v,y,x] - band < z < D'[v,y,x] + band  (strict), evaluated
// as PyTorch evaluates `z > depth - voxel_size[-1]` on the reference's tensors: in float32 with band rounded to float32 for a
// float32 map, in float64 (z widened exactly) for a float64 one.  Call only where ndet_project accepted the pixel.
__device__ __forceinline__ bool ndet_depth_band(const NdetGateMap& g, int v, int xi, int yi, float z) {
    const int64_t o = (int64_t)v * g.view_pitch + (int64_t)yi * g.row_pitch + xi;
    if (g.f64) {
        const double dv = static_cast<const double*>(g.map)[o];
        const double zz = (double)z;
        return (zz > dv - g.band) && (zz < dv + g.band);
    }
    const float dv = static_cast<const float*>(g.map)[o];
    const float b = (float)g.band;
    return (z > dv - b) && (z < dv + b);
}

// Host side: validate a caller's NdetDepthGate against the call (n_views, the projection's map h x w, and when need_r the image's
// H x W) and turn its maps into kernel arguments.  Returns NDET_OK or the error code (message set).
int ndet_gate_prepare(const NdetDepthGate* g, const char* fn, int n_views, int h, int w, int H, int W, bool need_r,
                      NdetGateMap* gf, NdetGateMap* gr);

// The gate with its map moved on by v0 views: what a launch (or a group kernel's block) over views v0 .. of the call indexes from 0.
__host__ __device__ __forceinline__ NdetGateMap ndet_gate_from_view(const NdetGateMap& g, int64_t v0) {
    NdetGateMap o = g;
    o.map = static_cast<const char*>(g.map) + (size_t)v0 * g.view_pitch * (g.f64 ? sizeof(double) : sizeof(float));
    return o;
}

// Host side: launch(std::true_type / std::false_type) by a run-time flag, for kernels that take the flag as a template argument.
template <class F>
static inline void ndet_by_flag(bool flag, F&& launch) {
    if (flag) launch(std::true_type{});
    else launch(std::false_type{});
}

// Streaming scenes (include/nerfdet_hip.h, NdetSceneAccum): launchers of K2's accumulate (<= 128 views) and finish kernels
// (density_kernels.hip), called by the entry points in volume_kernels.hip once every argument has been checked.
void ndet_scene_k2_accumulate_launch(const NdetSceneAccum* s, const float* mapped, int n_views, int h, int w, int mview_pitch, int mrow_pitch,
                                     const float* bias, const float* rgb, int H, int W, int rsv, int rsc, int rsy, const float* points,
                                     const float* proj, const float* rgb_proj, bool gated, const NdetGateMap& gf, const NdetGateMap& gr,
                                     hipStream_t stream);
void ndet_scene_k2_finish_launch(const NdetSceneAccum* s, const float* bias, float* global_feat, hipStream_t stream);

// Ring finishes (include/nerfdet_hip.h, ndet_scene_*_finish_ring): the segments' sum and count tensors of one kernel (K1's or K2's), oldest
// first, riding in the kernel-argument block (1.25 KiB); entries beyond n_segs are null and never read.
struct NdetRingArgs {
    const float* sum[NDET_RING_MAX];
    const int* count[NDET_RING_MAX];
    int pitch[NDET_RING_MAX];
};
#define NDET_RING_BATCH 4   // segments whose loads a thread issues before it adds them (in array order)

// Where a ring walk (k1_ring_sum in volume_kernels.hip, k2_ring_sums in density_kernels.hip) finds segment j: in the kernel-argument
// block, or -- the grouped ring finishes -- in the workgroup's LDS arrays of resolved pointers, every state at the pool's pitch.
struct NdetRingArgSegs {
    const NdetRingArgs& r;
    __device__ __forceinline__ const float* sum(int j) const { return r.sum[j]; }
    __device__ __forceinline__ const int* count(int j) const { return r.count[j]; }
    __device__ __forceinline__ int pitch(int j) const { return r.pitch[j]; }
};
struct NdetRingLdsSegs {
    const float* const (&s_sum)[NDET_RING_MAX];
    const int* const (&s_count)[NDET_RING_MAX];
    int pool_pitch;
    __device__ __forceinline__ const float* sum(int j) const { return s_sum[j]; }
    __device__ __forceinline__ const int* count(int j) const { return s_count[j]; }
    __device__ __forceinline__ int pitch(int) const { return pool_pitch; }
};
void ndet_scene_k2_finish_ring_launch(const NdetSceneAccum* segs, int n_segs, int n_views, const float* bias, float* global_feat,
                                      hipStream_t stream);

// Scene groups (include/nerfdet_hip.h, ndet_scene_*_group): launchers of K2's grouped accumulate (k <= 128 views per scene, grid.y = listed
// scene) and finish kernels (density_kernels.hip), called by the entry points in volume_kernels.hip once every argument has been checked.
void ndet_scene_k2_accumulate_group_launch(const NdetSceneGroup* g, const NdetGroupSel* sel, int k, const float* mapped, int h, int w,
                                           int mview_pitch, int mrow_pitch, const float* bias, const float* rgb, int H, int W, int rsv, int rsc,
                                           int rsy, const float* proj, const float* rgb_proj, bool gated, const NdetGateMap& gf,
                                           const NdetGateMap& gr, hipStream_t stream);
void ndet_scene_k2_finish_group_launch(const NdetSceneGroup* g, const NdetGroupSel* sel, const float* bias, float* global_feat,
                                       hipStream_t stream);

// Windowed groups (include/nerfdet_hip.h, ndet_scene_*_finish_group_ring): launcher of K2's grouped ring finish (density_kernels.hip);
// segs_dev is the DEVICE copy of the (n, NDET_RING_MAX) segment lists, the host copy having been checked by the entry point.
void ndet_scene_k2_finish_group_ring_launch(const NdetSceneGroup* pool, const NdetGroupRingSel* sel, const int32_t* segs_dev, const float* bias,
                                            float* global_feat, hipStream_t stream);

// Gradient scatter of the backward kernels.  Default: float atomics (global_atomic_add_f32) -- fast, but the ORDER of the adds, and with it the last
// bits of every sum, changes from run to run.  Deterministic mode (tests: ndet_measurement_knob("deterministic_scatter", 1); the caller then hands
// a zeroed buffer of int64 in place of the float buffer): every contribution is rounded to a multiple of 2^-40 and added as a 64-bit INTEGER --
// integer addition is associative, so the sum is the same whatever the order (range +-8.4e6, resolution 9e-13; the caller converts back).
extern int g_ndet_deterministic_scatter;      // host side, set by ndet_measurement_knob, read by the backward launchers
__device__ __forceinline__ void ndet_scatter_add(float* buf, int64_t idx, float v, int det) {
    if (det) atomicAdd(reinterpret_cast<unsigned long long*>(buf) + idx, (unsigned long long)(long long)llrintf(v * 0x1p40f));
    else unsafeAtomicAdd(buf + idx, v);
}

__device__ __forceinline__ float4 ndet_add4(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
