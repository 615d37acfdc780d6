// Voxel-grid side of the NeRF-Det hot path on gfx950: lattice, projection + nearest gather,
// multi-view aggregation, density conditioning features, alpha gating.
// SURVEY.md section 8a rows A2-A6.  Compiled with -ffp-contract=off: every fused multiply-add in
// here is an explicit fmaf().
#include "ndet_common.hpp"

#include <stdarg.h>

#include <map>
#include <mutex>
#include <utility>

// ------------------------------------------------------------------------------------------
// error plumbing (host)
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void ndet_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

hipError_t ndet_lds_limit(const void* kernel, size_t bytes) {
    struct Raised { size_t bytes; hipError_t err; };
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, Raised> seen;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    const auto it = seen.find({kernel, dev});
    if (it != seen.end() && it->second.bytes >= bytes) return it->second.err;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    seen[{kernel, dev}] = {bytes, e};
    return e;
}

int g_ndet_deterministic_scatter = 0;     // ndet_common.hpp::ndet_scatter_add
extern "C" int ndet_version(void) { return 110; }
extern "C" const char* ndet_last_error(void) { return g_err; }

#define VOX_PER_TILE 16  // one workgroup = 4 waves x 4 voxels = 16 consecutive voxels (one z column at Z=16)
// K2 gathers one float per lane and view (a 140-byte row): a batch is cheap in registers and the kernel is latency bound, so it
// keeps many more views in flight than K1's 1-KiB rows allow
#ifndef K2_BATCH
#define K2_BATCH 4
#endif
#ifndef GATHER_BATCH
#define GATHER_BATCH 4  // independent 1-KiB row loads a wave keeps in flight per voxel (tools/tune_k1.py: 4 beats 8/12/16)
#endif
#ifndef K1_MIN_WAVES
#define K1_MIN_WAVES 6  // __launch_bounds__ 2nd argument (waves per SIMD) for K1; tuned with tools/tune_k1.py
#endif

// ------------------------------------------------------------------------------------------
// A2  get_points  (nerfdet.py:380-390)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_get_points(float* __restrict__ pts, int nx, int ny, int nz,
                                                    float vx, float vy, float vz, float ox, float oy, float oz) {
    const int N = nx * ny * nz;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int iz = n % nz;
    const int iy = (n / nz) % ny;
    const int ix = n / (nz * ny);
    // idx * voxel_size, rounded, then + shifted origin, rounded (two torch ops in the reference)
    pts[n] = (float)ix * vx + ox;
    pts[N + n] = (float)iy * vy + oy;
    pts[2 * N + n] = (float)iz * vz + oz;
}

extern "C" int ndet_get_points(float* points, int nx, int ny, int nz, const float* vs, const float* org, void* stream) {
    NDET_REQUIRE(points && vs && org, NDET_E_INVALID, "ndet_get_points: null pointer");
    NDET_REQUIRE(nx > 0 && ny > 0 && nz > 0, NDET_E_INVALID, "ndet_get_points: n_voxels must be positive");
    // new_origin = origin - n_voxels / 2. * voxel_size   (fp32, un-fused; nerfdet.py:388)
    volatile float hx = (float)nx / 2.0f, hy = (float)ny / 2.0f, hz = (float)nz / 2.0f;
    volatile float mx = hx * vs[0], my = hy * vs[1], mz = hz * vs[2];
    const float ox = org[0] - mx, oy = org[1] - my, oz = org[2] - mz;
    const int N = nx * ny * nz;
    hipLaunchKernelGGL(k_get_points, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, points, nx, ny, nz,
                       vs[0], vs[1], vs[2], ox, oy, oz);
    NDET_CHECK_LAUNCH("ndet_get_points");
    return NDET_OK;
}

// ------------------------------------------------------------------------------------------
// layout helper: (n, c, hw) -> (n, hw, c)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nchw_to_nhwc(const float* __restrict__ src, float* __restrict__ dst, int c, int hw) {
    __shared__ float tile[32][33];
    const int img = blockIdx.z;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const float* s = src + (int64_t)img * c * hw;
    float* d = dst + (int64_t)img * c * hw;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int cc = c0 + ty + k, pp = p0 + tx;
        tile[ty + k][tx] = (cc < c && pp < hw) ? s[(int64_t)cc * hw + pp] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int pp = p0 + ty + k, cc = c0 + tx;
        if (pp < hw && cc < c) d[(int64_t)pp * c + cc] = tile[tx][ty + k];
    }
}

extern "C" int ndet_nchw_to_nhwc(const float* src, float* dst, int n, int c, int hw, void* stream) {
    NDET_REQUIRE(src && dst, NDET_E_INVALID, "ndet_nchw_to_nhwc: null pointer");
    NDET_REQUIRE(n > 0 && c > 0 && hw > 0, NDET_E_INVALID, "ndet_nchw_to_nhwc: sizes must be positive");
    NDET_REQUIRE(n <= 65535 && (c + 31) / 32 <= 65535, NDET_E_UNSUPPORTED, "ndet_nchw_to_nhwc: grid too large");
    dim3 grid((hw + 31) / 32, (c + 31) / 32, n);
    hipLaunchKernelGGL(k_nchw_to_nhwc, grid, dim3(256), 0, (hipStream_t)stream, src, dst, c, hw);
    NDET_CHECK_LAUNCH("ndet_nchw_to_nhwc");
    return NDET_OK;
}

// ------------------------------------------------------------------------------------------
// measurement aid: the float4 copy whose rate is the empirical HBM ceiling the gather kernels are priced against
// ------------------------------------------------------------------------------------------
typedef float ndet_f4v __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_copy_float4(const ndet_f4v* __restrict__ src, ndet_f4v* __restrict__ dst, int64_t n4) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

extern "C" int ndet_hbm_copy(const float* src, float* dst, int64_t n_floats, void* stream) {
    NDET_REQUIRE(src && dst, NDET_E_INVALID, "ndet_hbm_copy: null pointer");
    NDET_REQUIRE(n_floats > 0 && n_floats % 4 == 0, NDET_E_INVALID, "ndet_hbm_copy: the length must be a positive multiple of 4 floats");
    NDET_REQUIRE(((uintptr_t)src | (uintptr_t)dst) % 16 == 0, NDET_E_INVALID, "ndet_hbm_copy: pointers must be 16-byte aligned");
    const int64_t n4 = n_floats / 4;
    // one 16-byte element per thread, non-temporal: the best of the shapes swept on MI355X (grid-stride with 1/2/4/8 elements per thread,
    // 1 024 ... n4/256 workgroups, temporal / non-temporal: 5.4 - 6.66 TB/s on 1 GiB buffers)
    const int64_t blocks = (n4 + 255) / 256;
    NDET_REQUIRE(blocks <= 0x7fffffff, NDET_E_UNSUPPORTED, "ndet_hbm_copy: at most 2^39 floats per launch");
    const int grid = (int)blocks;
    hipLaunchKernelGGL(k_copy_float4, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const ndet_f4v*)src, (ndet_f4v*)dst, n4);
    NDET_CHECK_LAUNCH("ndet_hbm_copy");
    return NDET_OK;
}

// ------------------------------------------------------------------------------------------
// Depth gate (nerfdet.py:404-411): argument checks and the resize of the depth maps
// ------------------------------------------------------------------------------------------
int ndet_gate_prepare(const NdetDepthGate* g, const char* fn, int n_views, int h, int w, int H, int W, bool need_r,
                      NdetGateMap* gf, NdetGateMap* gr) {
    NDET_REQUIRE(g, NDET_E_INVALID, "%s: null depth gate", fn);
    NDET_REQUIRE(g->size == (int32_t)sizeof(NdetDepthGate), NDET_E_INVALID, "%s: NdetDepthGate.size %d != %d (caller built against another layout)",
                 fn, g->size, (int)sizeof(NdetDepthGate));
    NDET_REQUIRE(g->dtype == 0 || g->dtype == 1, NDET_E_INVALID, "%s: depth dtype %d (0 = float32, 1 = float64)", fn, g->dtype);
    NDET_REQUIRE(g->band > 0.0 && g->band < 1e300, NDET_E_INVALID, "%s: band %g must be finite and > 0", fn, g->band);
    NDET_REQUIRE(g->n_views == n_views, NDET_E_INVALID, "%s: depth maps for %d views, call has %d", fn, g->n_views, n_views);
    NDET_REQUIRE(g->depth_f && g->h == h && g->w == w, NDET_E_INVALID, "%s: depth_f must be a %dx%d map (got %p, %dx%d)", fn, h, w,
                 g->depth_f, g->h, g->w);
    NDET_REQUIRE(g->f_row_pitch >= w && g->f_view_pitch >= (int64_t)h * g->f_row_pitch && g->f_row_pitch < ((int64_t)1 << 31),
                 NDET_E_INVALID, "%s: depth_f pitches smaller than the map", fn);
    const size_t es = g->dtype ? sizeof(double) : sizeof(float);
    NDET_REQUIRE(((uintptr_t)g->depth_f % es) == 0, NDET_E_INVALID, "%s: depth_f misaligned for its dtype", fn);
    gf->map = g->depth_f; gf->view_pitch = g->f_view_pitch; gf->row_pitch = (int)g->f_row_pitch; gf->f64 = g->dtype; gf->band = g->band;
    if (need_r) {
        NDET_REQUIRE(g->depth_r && g->H == H && g->W == W, NDET_E_INVALID, "%s: depth_r must be a %dx%d map (got %p, %dx%d)", fn, H, W,
                     g->depth_r, g->H, g->W);
        NDET_REQUIRE(g->r_row_pitch >= W && g->r_view_pitch >= (int64_t)H * g->r_row_pitch && g->r_row_pitch < ((int64_t)1 << 31),
                     NDET_E_INVALID, "%s: depth_r pitches smaller than the map", fn);
        NDET_REQUIRE(((uintptr_t)g->depth_r % es) == 0, NDET_E_INVALID, "%s: depth_r misaligned for its dtype", fn);
        gr->map = g->depth_r; gr->view_pitch = g->r_view_pitch; gr->row_pitch = (int)g->r_row_pitch; gr->f64 = g->dtype; gr->band = g->band;
    } else if (gr) {
        *gr = *gf;
    }
    return NDET_OK;
}

// F.interpolate(bilinear, align_corners=False) in T, PyTorch's CPU kernel's source-index form (bit-equal at integer ratios).
// One thread per output pixel; the launch covers the feature-sized maps of all views, then the image-sized ones.
template <typename T>
__device__ __forceinline__ void resize_axis(int dst, int in, T scale, int& i0, int& i1, T& l0, T& l1) {
    T src = ((T)dst + (T)0.5) * scale - (T)0.5;
    if (src < (T)0) src = (T)0;
    i0 = (int)src;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    l1 = src - (T)i0;
    l0 = (T)1 - l1;
}

template <typename T>
__global__ __launch_bounds__(256) void k_depth_resize(const T* __restrict__ src, int n_views, int Hd, int Wd, int64_t sv, int64_t sy,
                                                      T* __restrict__ out_f, int h, int w, T* __restrict__ out_r, int H, int W) {
    const int64_t nf = (int64_t)n_views * h * w;
    const int64_t nr = out_r ? (int64_t)n_views * H * W : 0;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf + nr) return;
    const bool f = i < nf;
    const int64_t k = f ? i : i - nf;
    const int oh = f ? h : H, ow = f ? w : W;
    T* out = f ? out_f : out_r;
    const int x = (int)(k % ow), y = (int)((k / ow) % oh), v = (int)(k / ((int64_t)ow * oh));
    const T sh = (T)Hd / (T)oh, sw = (T)Wd / (T)ow;
    int y0, y1, x0, x1;
    T ly0, ly1, lx0, lx1;
    resize_axis<T>(y, Hd, sh, y0, y1, ly0, ly1);
    resize_axis<T>(x, Wd, sw, x0, x1, lx0, lx1);
    const T* b = src + (int64_t)v * sv;
    const T v00 = b[(int64_t)y0 * sy + x0], v01 = b[(int64_t)y0 * sy + x1];
    const T v10 = b[(int64_t)y1 * sy + x0], v11 = b[(int64_t)y1 * sy + x1];
    // PyTorch's CPU kernel takes one of two paths by the OUTPUT size (H + W <= 128: the per-tap weight products summed left to right;
    // larger: the nested form); each is followed here so that both the small test scenes and the shipped sizes come out bit-equal
    if (oh + ow <= 128)
        out[k] = (((ly0 * lx0) * v00 + (ly0 * lx1) * v01) + (ly1 * lx0) * v10) + (ly1 * lx1) * v11;
    else
        out[k] = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
}

extern "C" int ndet_depth_resize(const void* depth, int dtype, int n_views, int Hd, int Wd, int64_t sv, int64_t sy,
                                 void* out_f, int h, int w, void* out_r, int H, int W, void* stream) {
    const char* fn = "ndet_depth_resize";
    NDET_REQUIRE(depth && out_f, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(dtype == 0 || dtype == 1, NDET_E_INVALID, "%s: dtype %d (0 = float32, 1 = float64)", fn, dtype);
    NDET_REQUIRE(n_views > 0 && Hd > 0 && Wd > 0 && h > 0 && w > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(!out_r || (H > 0 && W > 0), NDET_E_INVALID, "%s: image-sized map of %dx%d", fn, H, W);
    NDET_REQUIRE(sy >= Wd && sv >= (int64_t)Hd * sy, NDET_E_INVALID, "%s: pitches smaller than the depth map", fn);
    const int64_t total = (int64_t)n_views * h * w + (out_r ? (int64_t)n_views * H * W : 0);
    const int64_t blocks = (total + 255) / 256;
    NDET_REQUIRE(blocks < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: too many pixels", fn);
    if (dtype == 0)
        hipLaunchKernelGGL(k_depth_resize<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)depth, n_views, Hd, Wd,
                           sv, sy, (float*)out_f, h, w, (float*)out_r, H, W);
    else
        hipLaunchKernelGGL(k_depth_resize<double>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const double*)depth, n_views, Hd,
                           Wd, sv, sy, (double*)out_f, h, w, (double*)out_r, H, W);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ------------------------------------------------------------------------------------------
// A3  backproject, materialising form (exact reference API; not the hot path)
// ------------------------------------------------------------------------------------------
template <bool DG>
__global__ __launch_bounds__(256) void k_backproject(const float* __restrict__ feat, int C, int h, int w,
                                                     int64_t sv, int64_t sc, int64_t sy, int64_t sx,
                                                     const float* __restrict__ points, int N,
                                                     const float* __restrict__ proj, float* __restrict__ volume,
                                                     uint8_t* __restrict__ valid, NdetGateMap gate) {
    const int v = blockIdx.y;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int xi, yi;
    float z;
    bool ok = ndet_project_z(proj + v * 12, points[n], points[N + n], points[2 * N + n], w, h, xi, yi, z);
    if (DG) ok = ok && ndet_depth_band(gate, v, xi, yi, z);
    valid[(int64_t)v * N + n] = ok ? 1 : 0;
    const float* src = feat + v * sv + yi * sy + xi * sx;
    float* dst = volume + (int64_t)v * C * N + n;
    int c = 0;
    for (; c + 4 <= C; c += 4) {
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
        if (ok) {
            t0 = src[(c + 0) * sc];
            t1 = src[(c + 1) * sc];
            t2 = src[(c + 2) * sc];
            t3 = src[(c + 3) * sc];
        }
        dst[(int64_t)(c + 0) * N] = t0;
        dst[(int64_t)(c + 1) * N] = t1;
        dst[(int64_t)(c + 2) * N] = t2;
        dst[(int64_t)(c + 3) * N] = t3;
    }
    for (; c < C; ++c) dst[(int64_t)c * N] = ok ? src[c * sc] : 0.f;
}

static int backproject_impl(const char* fn, const float* features, int n_views, int C, int h, int w, int64_t sv, int64_t sc,
                            int64_t sy, int64_t sx, const float* points, int N, const float* projection,
                            float* volume, uint8_t* valid, const NdetDepthGate* gate, void* stream) {
    NDET_REQUIRE(features && points && projection && volume && valid, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_views > 0 && C > 0 && h > 0 && w > 0 && N > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(n_views <= 65535, NDET_E_UNSUPPORTED, "%s: more than 65535 views", fn);
    NdetGateMap gm = {};
    if (gate) {
        const int rc = ndet_gate_prepare(gate, fn, n_views, h, w, 0, 0, false, &gm, nullptr);
        if (rc != NDET_OK) return rc;
    }
    dim3 grid((N + 255) / 256, n_views);
    if (gate)
        hipLaunchKernelGGL(k_backproject<true>, grid, dim3(256), 0, (hipStream_t)stream, features, C, h, w, sv, sc, sy, sx, points,
                           N, projection, volume, valid, gm);
    else
        hipLaunchKernelGGL(k_backproject<false>, grid, dim3(256), 0, (hipStream_t)stream, features, C, h, w, sv, sc, sy, sx, points,
                           N, projection, volume, valid, gm);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_backproject(const float* features, int n_views, int C, int h, int w, int64_t sv, int64_t sc,
                                int64_t sy, int64_t sx, const float* points, int N, const float* projection,
                                float* volume, uint8_t* valid, void* stream) {
    return backproject_impl("ndet_backproject", features, n_views, C, h, w, sv, sc, sy, sx, points, N, projection, volume, valid,
                            nullptr, stream);
}

extern "C" int ndet_backproject_gated(const float* features, int n_views, int C, int h, int w, int64_t sv, int64_t sc,
                                      int64_t sy, int64_t sx, const float* points, int N, const float* projection,
                                      float* volume, uint8_t* valid, const NdetDepthGate* gate, void* stream) {
    NDET_REQUIRE(gate, NDET_E_INVALID, "ndet_backproject_gated: null depth gate");
    return backproject_impl("ndet_backproject_gated", features, n_views, C, h, w, sv, sc, sy, sx, points, N, projection, volume, valid,
                            gate, stream);
}

// ------------------------------------------------------------------------------------------
// K1  fused backproject + view mean / count (+ alpha gating)   A3 + A4 (+ A6 gating)
//
// One wavefront per voxel, lanes over channels: with channels-last features one pixel's C floats
// are one contiguous row (1 KiB at C=256 = 64 lanes x float4), so a voxel-view gather is a single
// fully coalesced wave load.  The projection of the voxel into the views is computed with lanes
// over VIEWS (64 views per round), the valid views become a ballot mask, and the wave then walks
// the set bits with scalar code: only views that see the voxel cost a load, and the per-view pixel
// offset comes out of the lane that computed it with v_readlane.  GATHER_BATCH independent row
// loads are kept in flight.  The sum runs in ascending view order.
// Nothing of size (n_views, C, N) is ever written: reads = feature rows actually hit,
// writes = (C + 2) * N * 4 bytes.
// ------------------------------------------------------------------------------------------
// K1's view walk for the wave's voxels, phases A and B of k_backproject_aggregate below: adds the feature row of every view that sees a voxel
// to acc, in ascending view order, and the number of those views to cnt.  Used by the streaming accumulate kernels (k1_accumulate_body),
// which start from the scene's running sums instead of zero.  The one-shot kernel keeps its own copy of the walk: inlined through this
// helper it compiles to other register allocations (at NCHUNK = 2, 114 spilled VGPRs instead of 24).
constexpr int K1_VPW = VOX_PER_TILE / 4;  // voxels per wave, processed together
template <int NCHUNK, bool DG>
__device__ __forceinline__ void k1_walk(const float* __restrict__ feat, int n_views, int C, int h, int w, int64_t view_pitch, int row_pitch,
                                        const float* __restrict__ proj, const float (&px)[K1_VPW], const float (&py)[K1_VPW],
                                        const float (&pz)[K1_VPW], const bool (&live)[K1_VPW], float4 (&acc)[K1_VPW][NCHUNK],
                                        int (&cnt)[K1_VPW], const NdetGateMap& dgate, int lane) {
    constexpr int VPW = K1_VPW;
    const int c4 = C >> 2;
    for (int r0 = 0; r0 < n_views; r0 += 64) {
        // phase A: lanes over views, one camera matrix per lane, all voxels of the wave projected back to back
        const int v = r0 + lane;
        float P[12];
        {
            const float4* pm = reinterpret_cast<const float4*>(proj + (v < n_views ? v : 0) * 12);
            const float4 a = pm[0], b = pm[1], c = pm[2];
            P[0] = a.x; P[1] = a.y; P[2] = a.z; P[3] = a.w;
            P[4] = b.x; P[5] = b.y; P[6] = b.z; P[7] = b.w;
            P[8] = c.x; P[9] = c.y; P[10] = c.z; P[11] = c.w;
        }
        int off[VPW];
        unsigned long long mask[VPW];
#pragma unroll
        for (int j = 0; j < VPW; ++j) {
            int xi = 0, yi = 0;
            float z;
            bool ok = (v < n_views) && live[j] && ndet_project_z(P, px[j], py[j], pz[j], w, h, xi, yi, z);
            // depth gate: the lane's own view's depth value, before the ballot -- a gated-out view never costs a row gather
            if (DG) ok = ok && ndet_depth_band(dgate, v, xi, yi, z);
            off[j] = yi * row_pitch + xi * C;  // floats inside one view (< 2^31, checked on the host)
            mask[j] = __ballot(ok);
            cnt[j] += __popcll(mask[j]);
        }
        // phase B: walk the set bits; GATHER_BATCH independent row loads in flight
        const float* vbase = feat + (int64_t)r0 * view_pitch;
#pragma unroll
        for (int j = 0; j < VPW; ++j) {
            unsigned long long m = mask[j];
            int b = 0;
            while (m) {
                float4 t[GATHER_BATCH][NCHUNK];
                bool has[GATHER_BATCH];
#pragma unroll
                for (int k = 0; k < GATHER_BATCH; ++k) {
                    has[k] = (m != 0ull);
                    if (has[k]) {
                        b = __builtin_ctzll(m);
                        m &= (m - 1ull);
                    }  // else: re-read the previous row (L1 hit), discarded below
                    const int o = __builtin_amdgcn_readlane(off[j], b);
                    const float4* p = reinterpret_cast<const float4*>(vbase + (int64_t)b * view_pitch + o);
#pragma unroll
                    for (int q = 0; q < NCHUNK; ++q) {
                        const int ci = lane + q * 64;
                        t[k][q] = (ci < c4) ? p[ci] : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
#pragma unroll
                for (int k = 0; k < GATHER_BATCH; ++k) {
                    if (has[k]) {
#pragma unroll
                        for (int q = 0; q < NCHUNK; ++q) acc[j][q] = ndet_add4(acc[j][q], t[k][q]);
                    }
                }
            }
        }
    }
}

// The depth-gated instantiations (DG) hold the gate's map, pitches and band on top: at K1_MIN_WAVES they spill, one wave fewer per SIMD
// leaves them spill-free.
template <int NCHUNK, bool GATE, int LAYOUT, bool DG>
__global__ __launch_bounds__(256, DG ? K1_MIN_WAVES - 1 : K1_MIN_WAVES) void k_backproject_aggregate(
    const float* __restrict__ feat, int n_views, int C, int h, int w, int64_t view_pitch, int row_pitch,
    const float* __restrict__ points, int N, const float* __restrict__ proj, const float* __restrict__ alpha,
    float* __restrict__ out, int64_t* __restrict__ count, int n_tiles, NdetGateMap dgate) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // LAYOUT_CN only: [16][C + 4]
    constexpr int VPW = VOX_PER_TILE / 4;  // voxels per wave, processed together
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tile = ndet_xcd_remap(blockIdx.x, n_tiles);
    const int n0 = tile * VOX_PER_TILE;
    const int c4 = C >> 2;
    const int ldp = C + 4;

    // the wave's voxels: slots wave, wave+4, wave+8, wave+12 of the tile (the 4 waves of the workgroup work on
    // 4 neighbouring voxels at a time); coordinates of all of them are fetched up front
    float px[VPW], py[VPW], pz[VPW];
    bool live[VPW];
#pragma unroll
    for (int j = 0; j < VPW; ++j) {
        const int n = n0 + j * 4 + wave;
        live[j] = n < N;  // wave-uniform
        const int nn = live[j] ? n : 0;
        px[j] = points[nn];
        py[j] = points[N + nn];
        pz[j] = points[2 * N + nn];
    }
    float4 acc[VPW][NCHUNK];
    int cnt[VPW];
#pragma unroll
    for (int j = 0; j < VPW; ++j) {
        cnt[j] = 0;
#pragma unroll
        for (int q = 0; q < NCHUNK; ++q) acc[j][q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }

    for (int r0 = 0; r0 < n_views; r0 += 64) {
        // phase A: lanes over views, one camera matrix per lane, all voxels of the wave projected back to back
        const int v = r0 + lane;
        float P[12];
        {
            const float4* pm = reinterpret_cast<const float4*>(proj + (v < n_views ? v : 0) * 12);
            const float4 a = pm[0], b = pm[1], c = pm[2];
            P[0] = a.x; P[1] = a.y; P[2] = a.z; P[3] = a.w;
            P[4] = b.x; P[5] = b.y; P[6] = b.z; P[7] = b.w;
            P[8] = c.x; P[9] = c.y; P[10] = c.z; P[11] = c.w;
        }
        int off[VPW];
        unsigned long long mask[VPW];
#pragma unroll
        for (int j = 0; j < VPW; ++j) {
            int xi = 0, yi = 0;
            float z;
            bool ok = (v < n_views) && live[j] && ndet_project_z(P, px[j], py[j], pz[j], w, h, xi, yi, z);
            // depth gate: the lane's own view's depth value, before the ballot -- a gated-out view never costs a row gather
            if (DG) ok = ok && ndet_depth_band(dgate, v, xi, yi, z);
            off[j] = yi * row_pitch + xi * C;  // floats inside one view (< 2^31, checked on the host)
            mask[j] = __ballot(ok);
            cnt[j] += __popcll(mask[j]);
        }
        // phase B: walk the set bits; GATHER_BATCH independent row loads in flight
        const float* vbase = feat + (int64_t)r0 * view_pitch;
#pragma unroll
        for (int j = 0; j < VPW; ++j) {
            unsigned long long m = mask[j];
            int b = 0;
            while (m) {
                float4 t[GATHER_BATCH][NCHUNK];
                bool has[GATHER_BATCH];
#pragma unroll
                for (int k = 0; k < GATHER_BATCH; ++k) {
                    has[k] = (m != 0ull);
                    if (has[k]) {
                        b = __builtin_ctzll(m);
                        m &= (m - 1ull);
                    }  // else: re-read the previous row (L1 hit), discarded below
                    const int o = __builtin_amdgcn_readlane(off[j], b);
                    const float4* p = reinterpret_cast<const float4*>(vbase + (int64_t)b * view_pitch + o);
#pragma unroll
                    for (int q = 0; q < NCHUNK; ++q) {
                        const int ci = lane + q * 64;
                        t[k][q] = (ci < c4) ? p[ci] : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
#pragma unroll
                for (int k = 0; k < GATHER_BATCH; ++k) {
                    if (has[k]) {
#pragma unroll
                        for (int q = 0; q < NCHUNK; ++q) acc[j][q] = ndet_add4(acc[j][q], t[k][q]);
                    }
                }
            }
        }
    }

    // volume_sum / (valid + 1e-8); zero where no view sees the voxel (nerfdet.py:175-176);
    // optionally alpha * mean, again zeroed at count 0 (nerfdet.py:259-261).
#pragma unroll
    for (int j = 0; j < VPW; ++j) {
        if (!live[j]) continue;
        const int slot = j * 4 + wave;
        const int n = n0 + slot;
        const float denom = (float)cnt[j] + 1e-8f;
        float a = 1.0f;
        if (GATE) a = alpha[n];
#pragma unroll
        for (int q = 0; q < NCHUNK; ++q) {
            float4 mean;
            mean.x = acc[j][q].x / denom;
            mean.y = acc[j][q].y / denom;
            mean.z = acc[j][q].z / denom;
            mean.w = acc[j][q].w / denom;
            if (GATE) {
                mean.x = a * mean.x;
                mean.y = a * mean.y;
                mean.z = a * mean.z;
                mean.w = a * mean.w;
            }
            if (cnt[j] == 0) mean = make_float4(0.f, 0.f, 0.f, 0.f);
            const int ci = lane + q * 64;
            if (ci < c4) {
                if (LAYOUT == NDET_LAYOUT_NC)
                    *reinterpret_cast<float4*>(out + (int64_t)n * C + ci * 4) = mean;
                else
                    *reinterpret_cast<float4*>(smem + slot * ldp + ci * 4) = mean;
            }
        }
        if (lane == 0) count[n] = (int64_t)cnt[j];
    }

    if (LAYOUT == NDET_LAYOUT_CN) {
        // (16 voxels x C) tile -> C segments of 16 consecutive voxels (64 B) in the (C, N) tensor
        __syncthreads();
        for (int idx = threadIdx.x; idx < C * VOX_PER_TILE; idx += 256) {
            const int c = idx >> 4, jv = idx & 15;
            const int n = n0 + jv;
            if (n < N) out[(int64_t)c * N + n] = smem[jv * ldp + c];
        }
    }
}

template <int NCHUNK, bool DG>
static void launch_k1(bool gate, int layout, dim3 grid, size_t lds, hipStream_t st, const float* feat, int n_views, int C,
                      int h, int w, int64_t view_pitch, int row_pitch, const float* points, int N, const float* proj,
                      const float* alpha, float* out, int64_t* count, int n_tiles, const NdetGateMap& dgate) {
#define K1_LAUNCH(G, L)                                                                                                  \
    hipLaunchKernelGGL((k_backproject_aggregate<NCHUNK, G, L, DG>), grid, dim3(256), lds, st, feat, n_views, C, h, w,    \
                       view_pitch, row_pitch, points, N, proj, alpha, out, count, n_tiles, dgate)
    if (gate) {
        if (layout == NDET_LAYOUT_NC) K1_LAUNCH(true, NDET_LAYOUT_NC);
        else K1_LAUNCH(true, NDET_LAYOUT_CN);
    } else {
        if (layout == NDET_LAYOUT_NC) K1_LAUNCH(false, NDET_LAYOUT_NC);
        else K1_LAUNCH(false, NDET_LAYOUT_CN);
    }
#undef K1_LAUNCH
}

static int backproject_aggregate_impl(const char* fn, const float* features_nhwc, int n_views, int C, int h, int w,
                                      int64_t view_pitch, int64_t row_pitch, const float* points, int N,
                                      const float* projection, const float* alpha, float* out, int out_layout,
                                      int64_t* count, const NdetDepthGate* dgate, void* stream) {
    NDET_REQUIRE(features_nhwc && points && projection && out && count, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_views > 0 && C > 0 && h > 0 && w > 0 && N > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(out_layout == NDET_LAYOUT_CN || out_layout == NDET_LAYOUT_NC, NDET_E_INVALID, "%s: bad layout %d", fn, out_layout);
    NDET_REQUIRE(C % 4 == 0 && C <= 1024, NDET_E_UNSUPPORTED, "%s: C=%d must be a multiple of 4 and <= 1024", fn, C);
    NDET_REQUIRE(row_pitch >= (int64_t)w * C && view_pitch >= (int64_t)h * row_pitch, NDET_E_INVALID, "%s: pitches smaller than the image", fn);
    NDET_REQUIRE(row_pitch % 4 == 0 && view_pitch % 4 == 0 && ((uintptr_t)features_nhwc & 15) == 0, NDET_E_UNSUPPORTED,
                 "%s: feature rows must be 16-byte aligned", fn);
    NDET_REQUIRE((int64_t)h * row_pitch < (int64_t)1 << 31, NDET_E_UNSUPPORTED, "%s: one view exceeds 2^31 floats", fn);
    if (out_layout == NDET_LAYOUT_NC) NDET_REQUIRE(((uintptr_t)out & 15) == 0, NDET_E_UNSUPPORTED, "%s: out must be 16-byte aligned", fn);
    NdetGateMap gm = {};
    if (dgate) {
        const int rc = ndet_gate_prepare(dgate, fn, n_views, h, w, 0, 0, false, &gm, nullptr);
        if (rc != NDET_OK) return rc;
    }
    const int n_tiles = (N + VOX_PER_TILE - 1) / VOX_PER_TILE;
    const size_t lds = out_layout == NDET_LAYOUT_CN ? (size_t)VOX_PER_TILE * (C + 4) * sizeof(float) : 0;
    const dim3 grid(n_tiles);
    hipStream_t st = (hipStream_t)stream;
    const bool gate = alpha != nullptr;
#define K1_CHUNKS(DG)                                                                                                                                \
    if (C <= 256)                                                                                                                                    \
        launch_k1<1, DG>(gate, out_layout, grid, lds, st, features_nhwc, n_views, C, h, w, view_pitch, (int)row_pitch, points, N, projection, alpha, \
                         out, count, n_tiles, gm);                                                                                                   \
    else if (C <= 512)                                                                                                                               \
        launch_k1<2, DG>(gate, out_layout, grid, lds, st, features_nhwc, n_views, C, h, w, view_pitch, (int)row_pitch, points, N, projection, alpha, \
                         out, count, n_tiles, gm);                                                                                                   \
    else                                                                                                                                             \
        launch_k1<4, DG>(gate, out_layout, grid, lds, st, features_nhwc, n_views, C, h, w, view_pitch, (int)row_pitch, points, N, projection, alpha, \
                         out, count, n_tiles, gm)
    if (dgate) {
        K1_CHUNKS(true);
    } else {
        K1_CHUNKS(false);
    }
#undef K1_CHUNKS
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_backproject_aggregate(const float* features_nhwc, int n_views, int C, int h, int w,
                                          int64_t view_pitch, int64_t row_pitch, const float* points, int N,
                                          const float* projection, const float* alpha, float* out, int out_layout,
                                          int64_t* count, void* stream) {
    return backproject_aggregate_impl("ndet_backproject_aggregate", features_nhwc, n_views, C, h, w, view_pitch, row_pitch, points, N,
                                      projection, alpha, out, out_layout, count, nullptr, stream);
}

extern "C" int ndet_backproject_aggregate_gated(const float* features_nhwc, int n_views, int C, int h, int w,
                                                int64_t view_pitch, int64_t row_pitch, const float* points, int N,
                                                const float* projection, const float* alpha, float* out, int out_layout,
                                                int64_t* count, const NdetDepthGate* gate, void* stream) {
    NDET_REQUIRE(gate, NDET_E_INVALID, "ndet_backproject_aggregate_gated: null depth gate");
    return backproject_aggregate_impl("ndet_backproject_aggregate_gated", features_nhwc, n_views, C, h, w, view_pitch, row_pitch, points, N,
                                      projection, alpha, out, out_layout, count, gate, stream);
}

// ------------------------------------------------------------------------------------------
// Streaming scenes (include/nerfdet_hip.h): K1 split at its division, for one state (NdetSceneAccum), a ring of states
// (ndet_scene_*_finish_ring), the listed scenes of a group (NdetSceneGroup, grid.y = listed scene) and the listed scenes' rings
// (NdetGroupRingSel).
//
// K1-accumulate is k_backproject_aggregate's walk started from the scene's running sums (channels-last fp32) and count instead of zero,
// stored back without the division.  The walk adds rows in ascending view order, so a scene fed in chunks holds the very sums one launch
// over all its views forms.  K1-finish is K1's epilogue over the state; the state is only read.
//
// What the four families share is written once: the accumulate body (k1_accumulate_body around k1_walk), the sum over a ring's segments
// (k1_ring_sum) and the finish of one (voxel, channel quad) (k1_finish_quad).  The kernels are what differs: where the state, the points
// and the output row come from.  Not shared, on purpose: k_backproject_aggregate keeps its own walk and epilogue, because routed through
// an inlined helper its C = 512 instantiation spilled 114 VGPRs instead of 24 ("Streaming scenes").  That was measured for
// the one-shot kernel alone; the kernels below keep their LDS, scratch and occupancy with the helpers (DESIGN.md has the table).
// ------------------------------------------------------------------------------------------
// The accumulate kernels from the tile remap on: the tile's points, counts and running sums in, k1_walk over the n_views views at feat /
// proj / dgate, sums and counts out.
template <int NCHUNK, bool DG>
__device__ __forceinline__ void k1_accumulate_body(const float* __restrict__ feat, int n_views, int C, int h, int w, int64_t view_pitch,
                                                   int row_pitch, const float* __restrict__ points, int N, const float* __restrict__ proj,
                                                   float* __restrict__ sum, int pitch, int* __restrict__ count, int n_tiles,
                                                   const NdetGateMap& dgate) {
    constexpr int VPW = K1_VPW;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tile = ndet_xcd_remap(blockIdx.x, n_tiles);
    const int n0 = tile * VOX_PER_TILE;
    const int c4 = C >> 2;
    float px[VPW], py[VPW], pz[VPW];
    bool live[VPW];
    float4 acc[VPW][NCHUNK];
    int cnt[VPW];
#pragma unroll
    for (int j = 0; j < VPW; ++j) {
        const int n = n0 + j * 4 + wave;
        live[j] = n < N;  // wave-uniform
        const int nn = live[j] ? n : 0;
        px[j] = points[nn];
        py[j] = points[N + nn];
        pz[j] = points[2 * N + nn];
        cnt[j] = live[j] ? count[nn] : 0;
#pragma unroll
        for (int q = 0; q < NCHUNK; ++q) {
            const int ci = lane + q * 64;
            acc[j][q] = (live[j] && ci < c4) ? *reinterpret_cast<const float4*>(sum + (int64_t)nn * pitch + ci * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    k1_walk<NCHUNK, DG>(feat, n_views, C, h, w, view_pitch, row_pitch, proj, px, py, pz, live, acc, cnt, dgate, lane);
#pragma unroll
    for (int j = 0; j < VPW; ++j) {
        if (!live[j]) continue;
        const int n = n0 + j * 4 + wave;
#pragma unroll
        for (int q = 0; q < NCHUNK; ++q) {
            const int ci = lane + q * 64;
            if (ci < c4) *reinterpret_cast<float4*>(sum + (int64_t)n * pitch + ci * 4) = acc[j][q];
        }
        if (lane == 0) count[n] = cnt[j];
    }
}

// K1's epilogue for channel quad q of one voxel, expression for expression (k_backproject_aggregate above): s and cnt are the voxel's
// summed rows and view count, `row` its row of alpha, out and out_count.
__device__ __forceinline__ void k1_finish_quad(float4 s, int cnt, const float* __restrict__ alpha, int64_t row, int C, int q,
                                               float* __restrict__ out, int64_t* __restrict__ out_count) {
    const float denom = (float)cnt + 1e-8f;
    float4 mean;
    mean.x = s.x / denom;
    mean.y = s.y / denom;
    mean.z = s.z / denom;
    mean.w = s.w / denom;
    if (alpha) {
        const float a = alpha[row];
        mean.x = a * mean.x;
        mean.y = a * mean.y;
        mean.z = a * mean.z;
        mean.w = a * mean.w;
    }
    if (cnt == 0) mean = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(out + row * C + q * 4) = mean;
    if (q == 0) out_count[row] = (int64_t)cnt;
}

// Channel quad q of voxel n summed over a ring's segments (Segs: NdetRingArgSegs or NdetRingLdsSegs, ndet_common.hpp), and the voxel's
// view count.  The accumulator starts from the oldest segment's values, the others are added in array order, NDET_RING_BATCH segments at
// a time -- their counts are loaded first, then the rows of those that see the voxel (a segment that does not holds an all-zero row: adding
// +0 instead changes at most the sign of a zero), then the adds.  With one segment the loop does not run and s, cnt are the state's own.
template <class Segs>
__device__ __forceinline__ void k1_ring_sum(const Segs& g, int n_segs, int n, int q, float4& s, int& cnt) {
    constexpr int U = NDET_RING_BATCH;
    cnt = g.count(0)[n];
    s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cnt != 0) s = *reinterpret_cast<const float4*>(g.sum(0) + (int64_t)n * g.pitch(0) + q * 4);
    for (int s0 = 1; s0 < n_segs; s0 += U) {
        int cc[U];
        float4 vv[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int sj = min(s0 + j, n_segs - 1);     // past the end: the last segment's slot, not read (cc = 0)
            cc[j] = (s0 + j < n_segs) ? g.count(sj)[n] : 0;
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int sj = min(s0 + j, n_segs - 1);
            vv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cc[j] != 0) vv[j] = *reinterpret_cast<const float4*>(g.sum(sj) + (int64_t)n * g.pitch(sj) + q * 4);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            s.x = s.x + vv[j].x;
            s.y = s.y + vv[j].y;
            s.z = s.z + vv[j].z;
            s.w = s.w + vv[j].w;
            cnt += cc[j];
        }
    }
}

// The depth-gated instantiations run one wave fewer per SIMD, as k_backproject_aggregate's do.
template <int NCHUNK, bool DG>
__global__ __launch_bounds__(256, DG ? K1_MIN_WAVES - 1 : K1_MIN_WAVES) void k_backproject_accumulate(
    const float* __restrict__ feat, int n_views, int C, int h, int w, int64_t view_pitch, int row_pitch,
    const float* __restrict__ points, int N, const float* __restrict__ proj, float* __restrict__ sum, int pitch,
    int* __restrict__ count, int n_tiles, NdetGateMap dgate) {
    k1_accumulate_body<NCHUNK, DG>(feat, n_views, C, h, w, view_pitch, row_pitch, points, N, proj, sum, pitch, count, n_tiles, dgate);
}

// The listed scenes' chunks in one launch.  A block reads its scene's row of the device table, moves the view-indexed inputs on by y * k
// views -- as the host loop of ndet_scene_accumulate moves them on per 128-view launch -- and runs the body on that scene's state and
// points; no block reads or writes another scene's state.  The XCD remap stays on blockIdx.x: a scene's neighbouring tiles still share an
// L2, which XCD a slab lands on differs from row to row when the tile count is no multiple of 8 (locality only).
template <int NCHUNK, bool DG>
__global__ __launch_bounds__(256, DG ? K1_MIN_WAVES - 1 : K1_MIN_WAVES) void k_backproject_accumulate_group(
    const NdetSceneSlot* __restrict__ table, NdetGroupSel sel, int k, const float* __restrict__ feat_all, int C, int h, int w,
    int64_t view_pitch, int row_pitch, int N, const float* __restrict__ proj_all, int pitch, int n_tiles, NdetGateMap dgate_all) {
    const int y = blockIdx.y;                                  // listed scene: block-uniform, the row comes in through scalar loads
    const NdetSceneSlot& sl = table[sel.slot[y]];
    const int64_t v0 = (int64_t)y * k;                         // the scene's first view of the call
    k1_accumulate_body<NCHUNK, DG>(feat_all + v0 * view_pitch, k, C, h, w, view_pitch, row_pitch, sl.points, N, proj_all + v0 * 12, sl.k1_sum,
                                   pitch, sl.k1_count, n_tiles, DG ? ndet_gate_from_view(dgate_all, v0) : dgate_all);
}

// One thread per (voxel, channel quad) in all four finishes; the grouped ones write output row y N + n and index alpha the same way.
__global__ __launch_bounds__(256) void k_volume_finish(const float* __restrict__ sum, int pitch, const int* __restrict__ count,
                                                       const float* __restrict__ alpha, int C, int N, float* __restrict__ out,
                                                       int64_t* __restrict__ out_count) {
    const int c4 = C >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * c4) return;
    const int n = (int)(i / c4), q = (int)(i % c4);
    const int cnt = count[n];
    k1_finish_quad(*reinterpret_cast<const float4*>(sum + (int64_t)n * pitch + q * 4), cnt, alpha, n, C, q, out, out_count);
}

__global__ __launch_bounds__(256) void k_volume_finish_ring(NdetRingArgs r, int n_segs, const float* __restrict__ alpha, int C, int N,
                                                            float* __restrict__ out, int64_t* __restrict__ out_count) {
    const int c4 = C >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * c4) return;
    const int n = (int)(i / c4), q = (int)(i % c4);
    float4 s;
    int cnt;
    k1_ring_sum(NdetRingArgSegs{r}, n_segs, n, q, s, cnt);
    k1_finish_quad(s, cnt, alpha, n, C, q, out, out_count);
}

__global__ __launch_bounds__(256) void k_volume_finish_group(const NdetSceneSlot* __restrict__ table, NdetGroupSel sel, int pitch,
                                                             const float* __restrict__ alpha, int C, int N, float* __restrict__ out,
                                                             int64_t* __restrict__ out_count) {
    const int c4 = C >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * c4) return;
    const int y = blockIdx.y;
    const NdetSceneSlot& sl = table[sel.slot[y]];
    const int n = (int)(i / c4), q = (int)(i % c4);
    const int cnt = sl.k1_count[n];
    k1_finish_quad(*reinterpret_cast<const float4*>(sl.k1_sum + (int64_t)n * pitch + q * 4), cnt, alpha, (int64_t)y * N + n, C, q, out,
                   out_count);
}

// The segments are found through memory: segs[y][j] is a row of the pool table, the row holds the state's pointers.  That chain is
// block-uniform, so threads 0 .. n_segs - 1 resolve it once into LDS (64 x 16 bytes) and the walk reads its pointers from there after one
// barrier; the threads past N c4 stay for the barrier and do nothing after it.  The state pitch is the pool's.
__global__ __launch_bounds__(256) void k_volume_finish_group_ring(const NdetSceneSlot* __restrict__ table, NdetGroupRingSel sel,
                                                                  const int32_t* __restrict__ segs, int pitch,
                                                                  const float* __restrict__ alpha, int C, int N, float* __restrict__ out,
                                                                  int64_t* __restrict__ out_count) {
    __shared__ const float* s_sum[NDET_RING_MAX];
    __shared__ const int* s_count[NDET_RING_MAX];
    const int y = blockIdx.y;
    const int n_segs = sel.n_segs[y];
    if ((int)threadIdx.x < n_segs) {
        const NdetSceneSlot& sl = table[segs[y * NDET_RING_MAX + threadIdx.x]];
        s_sum[threadIdx.x] = sl.k1_sum;
        s_count[threadIdx.x] = sl.k1_count;
    }
    __syncthreads();
    const int c4 = C >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)N * c4) {
        const int n = (int)(i / c4), q = (int)(i % c4);
        float4 s;
        int cnt;
        k1_ring_sum(NdetRingLdsSegs{s_sum, s_count, pitch}, n_segs, n, q, s, cnt);
        k1_finish_quad(s, cnt, alpha, (int64_t)y * N + n, C, q, out, out_count);
    }
}

// ---- host checks, all before any launch ----
// A state's sizes and pitches: the same for a single state's block, a group's and a pool's.
static int state_dims_check(const char* fn, int N, int C, int cm, int64_t k1_pitch, int64_t k2_pitch) {
    NDET_REQUIRE(N > 0 && C > 0 && cm > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(C % 4 == 0 && C <= 1024, NDET_E_UNSUPPORTED, "%s: C=%d must be a multiple of 4 and <= 1024", fn, C);
    NDET_REQUIRE(cm % 4 == 0 && cm <= 128, NDET_E_UNSUPPORTED, "%s: cm=%d must be a multiple of 4 and <= 128", fn, cm);
    NDET_REQUIRE(k1_pitch >= C && k2_pitch >= 3 * (cm + 4), NDET_E_INVALID, "%s: state pitches smaller than a row", fn);
    NDET_REQUIRE(k1_pitch < ((int64_t)1 << 31) && k2_pitch < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: state pitches exceed int32", fn);
    NDET_REQUIRE(k1_pitch % 4 == 0 && k2_pitch % 4 == 0, NDET_E_UNSUPPORTED, "%s: state rows must be 16-byte aligned", fn);
    return NDET_OK;
}

// A single state's block (pointers, sizes, pitches, alignment).
static int scene_check(const NdetSceneAccum* s, const char* fn) {
    NDET_REQUIRE(s, NDET_E_INVALID, "%s: null scene state", fn);
    NDET_REQUIRE(s->size == (int32_t)sizeof(NdetSceneAccum), NDET_E_INVALID, "%s: NdetSceneAccum.size %d != %d (caller built against another layout)",
                 fn, s->size, (int)sizeof(NdetSceneAccum));
    NDET_REQUIRE(s->k1_sum && s->k1_count && s->k2_sum && s->k2_count, NDET_E_INVALID, "%s: null pointer in the scene state", fn);
    NDET_REQUIRE(s->n_views >= 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    const int rc = state_dims_check(fn, s->N, s->C, s->cm, s->k1_pitch, s->k2_pitch);
    if (rc != NDET_OK) return rc;
    NDET_REQUIRE((((uintptr_t)s->k1_sum | (uintptr_t)s->k2_sum) & 15) == 0 && (((uintptr_t)s->k1_count & 3) | ((uintptr_t)s->k2_count & 7)) == 0,
                 NDET_E_UNSUPPORTED, "%s: state rows must be 16-byte aligned", fn);
    return NDET_OK;
}

// The segment list of a ring finish: every block as scene_check checks it (the message names the segment), equal N / C / cm, a view
// total within int32.
static int ring_check(const NdetSceneAccum* segs, int n_segs, const char* fn, int* total_views) {
    NDET_REQUIRE(segs, NDET_E_INVALID, "%s: null segs", fn);
    NDET_REQUIRE(n_segs >= 1 && n_segs <= NDET_RING_MAX, NDET_E_INVALID, "%s: n_segs=%d must be 1 .. %d", fn, n_segs, NDET_RING_MAX);
    int64_t total = 0;
    for (int i = 0; i < n_segs; ++i) {
        const int rc = scene_check(&segs[i], fn);
        if (rc != NDET_OK) {
            char msg[400];
            snprintf(msg, sizeof(msg), "%s", g_err);
            ndet_set_error("%s (segs[%d])", msg, i);
            return rc;
        }
        NDET_REQUIRE(segs[i].N == segs[0].N, NDET_E_INVALID, "%s: segs[%d].N=%d differs from segs[0].N=%d", fn, i, segs[i].N, segs[0].N);
        NDET_REQUIRE(segs[i].C == segs[0].C, NDET_E_INVALID, "%s: segs[%d].C=%d differs from segs[0].C=%d", fn, i, segs[i].C, segs[0].C);
        NDET_REQUIRE(segs[i].cm == segs[0].cm, NDET_E_INVALID, "%s: segs[%d].cm=%d differs from segs[0].cm=%d", fn, i, segs[i].cm, segs[0].cm);
        total += segs[i].n_views;
        NDET_REQUIRE(total <= 0x7fffffff, NDET_E_UNSUPPORTED, "%s: n_views of segs[0..%d] add up to more than int32 holds", fn, i);
    }
    *total_views = (int)total;
    return NDET_OK;
}

// A table block (the table itself is device memory: its rows are the caller's): a `what` = "scene group" of up to NDET_GROUP_MAX rows,
// or a "state pool" of up to NDET_GROUP_POOL_MAX (NDET_RING_MAX + 1 states per scene).
static int table_check(const NdetSceneGroup* g, const char* fn, const char* what, const char* table, int max_slots) {
    NDET_REQUIRE(g, NDET_E_INVALID, "%s: null %s", fn, what);
    NDET_REQUIRE(g->size == (int32_t)sizeof(NdetSceneGroup), NDET_E_INVALID, "%s: NdetSceneGroup.size %d != %d (caller built against another layout)",
                 fn, g->size, (int)sizeof(NdetSceneGroup));
    NDET_REQUIRE(g->table, NDET_E_INVALID, "%s: null %s table", fn, table);
    NDET_REQUIRE(((uintptr_t)g->table & 15) == 0, NDET_E_UNSUPPORTED, "%s: the %s table must be 16-byte aligned", fn, table);
    NDET_REQUIRE(g->n_slots >= 1 && g->n_slots <= max_slots, NDET_E_INVALID, "%s: n_slots=%d must be 1 .. %d", fn, g->n_slots, max_slots);
    return state_dims_check(fn, g->N, g->C, g->cm, g->k1_pitch, g->k2_pitch);
}

// A group's block and a call's selection.
static int group_check(const NdetSceneGroup* g, const NdetGroupSel* sel, int k, const char* fn) {
    const int rc = table_check(g, fn, "scene group", "scene", NDET_GROUP_MAX);
    if (rc != NDET_OK) return rc;
    NDET_REQUIRE(sel, NDET_E_INVALID, "%s: null selection", fn);
    NDET_REQUIRE(sel->size == (int32_t)sizeof(NdetGroupSel), NDET_E_INVALID, "%s: NdetGroupSel.size %d != %d (caller built against another layout)",
                 fn, sel->size, (int)sizeof(NdetGroupSel));
    NDET_REQUIRE(sel->n >= 1 && sel->n <= NDET_GROUP_MAX, NDET_E_INVALID, "%s: %d listed scenes, must be 1 .. %d", fn, sel->n, NDET_GROUP_MAX);
    NDET_REQUIRE(k >= 0, NDET_E_INVALID, "%s: k=%d views", fn, k);
    unsigned long long used = 0ull;
    for (int i = 0; i < sel->n; ++i) {
        const int s = sel->slot[i];
        NDET_REQUIRE(s >= 0 && s < g->n_slots, NDET_E_INVALID, "%s: slot[%d]=%d outside the table's %d rows", fn, i, s, g->n_slots);
        NDET_REQUIRE(!((used >> s) & 1ull), NDET_E_INVALID, "%s: slot[%d]=%d is listed twice", fn, i, s);
        used |= 1ull << s;
        NDET_REQUIRE(sel->n_views[i] >= 0, NDET_E_INVALID, "%s: n_views[%d]=%d", fn, i, sel->n_views[i]);
        NDET_REQUIRE(sel->n_views[i] <= 0x7fffffff - k, NDET_E_UNSUPPORTED, "%s: view count of slot[%d] overflows int32", fn, i);
    }
    return NDET_OK;
}

// A pool's block, a call's selection and its segment lists (the HOST copy).
static int group_ring_check(const NdetSceneGroup* pool, const NdetGroupRingSel* sel, const int32_t* segs_host, const char* fn) {
    const int rc = table_check(pool, fn, "state pool", "pool", NDET_GROUP_POOL_MAX);
    if (rc != NDET_OK) return rc;
    NDET_REQUIRE(sel, NDET_E_INVALID, "%s: null selection", fn);
    NDET_REQUIRE(sel->size == (int32_t)sizeof(NdetGroupRingSel), NDET_E_INVALID,
                 "%s: NdetGroupRingSel.size %d != %d (caller built against another layout)", fn, sel->size, (int)sizeof(NdetGroupRingSel));
    NDET_REQUIRE(sel->n >= 1 && sel->n <= NDET_GROUP_MAX, NDET_E_INVALID, "%s: %d listed scenes, must be 1 .. %d", fn, sel->n, NDET_GROUP_MAX);
    NDET_REQUIRE(segs_host, NDET_E_INVALID, "%s: null segs_host", fn);
    uint64_t used[(NDET_GROUP_POOL_MAX + 63) / 64] = {};
    for (int i = 0; i < sel->n; ++i) {
        NDET_REQUIRE(sel->n_segs[i] >= 1 && sel->n_segs[i] <= NDET_RING_MAX, NDET_E_INVALID, "%s: n_segs[%d]=%d must be 1 .. %d", fn, i,
                     sel->n_segs[i], NDET_RING_MAX);
        NDET_REQUIRE(sel->n_views[i] >= 0, NDET_E_INVALID, "%s: n_views[%d]=%d", fn, i, sel->n_views[i]);
        for (int j = 0; j < sel->n_segs[i]; ++j) {
            const int s = segs_host[i * NDET_RING_MAX + j];
            NDET_REQUIRE(s >= 0 && s < pool->n_slots, NDET_E_INVALID, "%s: segs[%d][%d]=%d outside the pool's %d rows", fn, i, j, s, pool->n_slots);
            NDET_REQUIRE(!((used[s >> 6] >> (s & 63)) & 1ull), NDET_E_INVALID, "%s: segs[%d][%d]=%d is listed twice", fn, i, j, s);
            used[s >> 6] |= 1ull << (s & 63);
        }
    }
    return NDET_OK;
}

// The device copy of a grouped ring finish's segment lists.
static int segs_dev_check(const int32_t* segs_dev, const char* fn) {
    NDET_REQUIRE(segs_dev, NDET_E_INVALID, "%s: null segs_dev", fn);
    NDET_REQUIRE(((uintptr_t)segs_dev & 3) == 0, NDET_E_UNSUPPORTED, "%s: segs_dev must be 4-byte aligned", fn);
    return NDET_OK;
}

// A chunk's feature maps (K1's input, as backproject_aggregate_impl checks them), mapped maps and images (K2's, as
// density_features_packed_impl does); `per` = the most views one K2 launch covers.
static int accumulate_inputs_check(const char* fn, int C, int cm, int per, int h, int w, const float* features_nhwc, int64_t view_pitch,
                                   int64_t row_pitch, const float* mapped_nhwc, int64_t mview_pitch, int64_t mrow_pitch, const float* bias,
                                   int W, int64_t rsv, int64_t rsc, int64_t rsy) {
    NDET_REQUIRE(row_pitch >= (int64_t)w * C && view_pitch >= (int64_t)h * row_pitch, NDET_E_INVALID, "%s: feature pitches smaller than the map", fn);
    NDET_REQUIRE(row_pitch % 4 == 0 && view_pitch % 4 == 0 && ((uintptr_t)features_nhwc & 15) == 0, NDET_E_UNSUPPORTED,
                 "%s: feature rows must be 16-byte aligned", fn);
    NDET_REQUIRE((int64_t)h * row_pitch < (int64_t)1 << 31, NDET_E_UNSUPPORTED, "%s: one view exceeds 2^31 floats", fn);
    NDET_REQUIRE(mrow_pitch >= (int64_t)w * cm && mview_pitch >= (int64_t)h * mrow_pitch && rsy >= W && rsc >= 0 && rsv >= 0, NDET_E_INVALID,
                 "%s: mapped / image pitches smaller than the maps", fn);
    NDET_REQUIRE((int64_t)per * mview_pitch < ((int64_t)1 << 31) && (int64_t)per * rsv + 3 * rsc < ((int64_t)1 << 31), NDET_E_UNSUPPORTED,
                 "%s: a launch's source tensor exceeds 2^31 floats", fn);
    NDET_REQUIRE(mview_pitch % 4 == 0 && mrow_pitch % 4 == 0 && (((uintptr_t)mapped_nhwc | (uintptr_t)bias) & 15) == 0, NDET_E_UNSUPPORTED,
                 "%s: mapped features / bias must keep channel quads 16-byte aligned", fn);
    return NDET_OK;
}

// A finish's outputs: `name` = "global_feat" (8-byte rows, no count) or "out" (16-byte rows, and the int64 count); `threads` = the
// launch's threads per listed scene.
static int finish_out_check(const char* fn, const char* name, const void* out, int align, bool counted, const int64_t* count,
                            int64_t threads) {
    NDET_REQUIRE(out, NDET_E_INVALID, "%s: null %s", fn, name);
    if (counted) NDET_REQUIRE(count, NDET_E_INVALID, "%s: null count", fn);
    NDET_REQUIRE(((uintptr_t)out & (align - 1)) == 0, NDET_E_UNSUPPORTED, "%s: %s must be %d-byte aligned", fn, name, align);
    if (counted) NDET_REQUIRE(((uintptr_t)count & 7) == 0, NDET_E_UNSUPPORTED, "%s: count must be 8-byte aligned", fn);
    NDET_REQUIRE((threads + 255) / 256 < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: too many voxels", fn);
    return NDET_OK;
}

// launch(integral_constant NCHUNK, true_type / false_type DG) for the accumulate kernels' instantiation at C channels
template <class F>
static void k1_accumulate_dispatch(int C, bool gated, F&& launch) {
    ndet_by_flag(gated, [&](auto dg) {
        if (C <= 256) launch(std::integral_constant<int, 1>{}, dg);
        else if (C <= 512) launch(std::integral_constant<int, 2>{}, dg);
        else launch(std::integral_constant<int, 4>{}, dg);
    });
}

// ---- entry points: one state ----
extern "C" int ndet_scene_accumulate(const NdetSceneAccum* s, const float* features_nhwc, int n_views, int h, int w,
                                     int64_t view_pitch, int64_t row_pitch, const float* mapped_nhwc, int64_t mview_pitch,
                                     int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv, int64_t rsc,
                                     int64_t rsy, const float* points, const float* projection, const float* rgb_projection,
                                     const NdetDepthGate* gate, void* stream) {
    const char* fn = "ndet_scene_accumulate";
    NDET_TRY(scene_check(s, fn));
    const int N = s->N, C = s->C;
    NDET_REQUIRE(features_nhwc && mapped_nhwc && bias && rgb && points && projection && rgb_projection, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_views > 0 && h > 0 && w > 0 && H > 0 && W > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(s->n_views <= 0x7fffffff - n_views, NDET_E_UNSUPPORTED, "%s: view count overflows int32", fn);
    NDET_TRY(accumulate_inputs_check(fn, C, s->cm, n_views < 128 ? n_views : 128, h, w, features_nhwc, view_pitch, row_pitch, mapped_nhwc,
                                     mview_pitch, mrow_pitch, bias, W, rsv, rsc, rsy));
    NdetGateMap gf = {}, gr = {};
    if (gate) NDET_TRY(ndet_gate_prepare(gate, fn, n_views, h, w, H, W, true, &gf, &gr));
    hipStream_t st = (hipStream_t)stream;
    const int n_tiles = (N + VOX_PER_TILE - 1) / VOX_PER_TILE;
    k1_accumulate_dispatch(C, gate != nullptr, [&](auto nc, auto dg) {
        hipLaunchKernelGGL((k_backproject_accumulate<decltype(nc)::value, decltype(dg)::value>), dim3(n_tiles), dim3(256), 0, st, features_nhwc,
                           n_views, C, h, w, view_pitch, (int)row_pitch, points, N, projection, s->k1_sum, (int)s->k1_pitch, s->k1_count, n_tiles, gf);
    });
    NDET_CHECK_LAUNCH(fn);
    for (int v0 = 0; v0 < n_views; v0 += 128) {   // K2: launches of at most 128 views
        const int nv = n_views - v0 < 128 ? n_views - v0 : 128;
        ndet_scene_k2_accumulate_launch(s, mapped_nhwc + (int64_t)v0 * mview_pitch, nv, h, w, (int)mview_pitch, (int)mrow_pitch, bias,
                                        rgb + (int64_t)v0 * rsv, H, W, (int)rsv, (int)rsc, (int)rsy, points, projection + (int64_t)v0 * 12,
                                        rgb_projection + (int64_t)v0 * 12, gate != nullptr, gate ? ndet_gate_from_view(gf, v0) : gf,
                                        gate ? ndet_gate_from_view(gr, v0) : gr, st);
        NDET_CHECK_LAUNCH(fn);
    }
    return NDET_OK;
}

extern "C" int ndet_scene_density_finish(const NdetSceneAccum* s, const float* bias, float* global_feat, void* stream) {
    const char* fn = "ndet_scene_density_finish";
    NDET_TRY(scene_check(s, fn));
    NDET_REQUIRE(bias, NDET_E_INVALID, "%s: null bias", fn);
    NDET_TRY(finish_out_check(fn, "global_feat", global_feat, 8, false, nullptr, (int64_t)s->N * (s->cm + 3)));
    ndet_scene_k2_finish_launch(s, bias, global_feat, (hipStream_t)stream);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_scene_volume_finish(const NdetSceneAccum* s, const float* alpha, float* out, int64_t* count, void* stream) {
    const char* fn = "ndet_scene_volume_finish";
    NDET_TRY(scene_check(s, fn));
    const int64_t threads = (int64_t)s->N * (s->C / 4);
    NDET_TRY(finish_out_check(fn, "out", out, 16, true, count, threads));
    hipLaunchKernelGGL(k_volume_finish, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s->k1_sum, (int)s->k1_pitch,
                       s->k1_count, alpha, s->C, s->N, out, count);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ---- entry points: a ring of states ----
extern "C" int ndet_scene_density_finish_ring(const NdetSceneAccum* segs, int n_segs, const float* bias, float* global_feat, void* stream) {
    const char* fn = "ndet_scene_density_finish_ring";
    int n_views = 0;
    NDET_TRY(ring_check(segs, n_segs, fn, &n_views));
    NDET_REQUIRE(bias, NDET_E_INVALID, "%s: null bias", fn);
    NDET_TRY(finish_out_check(fn, "global_feat", global_feat, 8, false, nullptr, (int64_t)segs[0].N * (segs[0].cm / 4 + 1)));
    ndet_scene_k2_finish_ring_launch(segs, n_segs, n_views, bias, global_feat, (hipStream_t)stream);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_scene_volume_finish_ring(const NdetSceneAccum* segs, int n_segs, const float* alpha, float* out, int64_t* count,
                                             void* stream) {
    const char* fn = "ndet_scene_volume_finish_ring";
    int n_views = 0;
    NDET_TRY(ring_check(segs, n_segs, fn, &n_views));
    const int64_t threads = (int64_t)segs[0].N * (segs[0].C / 4);
    NDET_TRY(finish_out_check(fn, "out", out, 16, true, count, threads));
    NdetRingArgs r = {};
    for (int i = 0; i < n_segs; ++i) {
        r.sum[i] = segs[i].k1_sum;
        r.count[i] = segs[i].k1_count;
        r.pitch[i] = (int)segs[i].k1_pitch;
    }
    hipLaunchKernelGGL(k_volume_finish_ring, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r, n_segs, alpha,
                       segs[0].C, segs[0].N, out, count);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ---- entry points: scene groups ----
extern "C" int ndet_scene_group_check(const NdetSceneGroup* g, const NdetGroupSel* sel, int k) {
    return group_check(g, sel, k, "ndet_scene_group_check");
}

extern "C" int ndet_scene_accumulate_group(const NdetSceneGroup* g, const NdetGroupSel* sel, int k, const float* features_nhwc, int h, int w,
                                           int64_t view_pitch, int64_t row_pitch, const float* mapped_nhwc, int64_t mview_pitch,
                                           int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv, int64_t rsc,
                                           int64_t rsy, const float* projection, const float* rgb_projection, const NdetDepthGate* gate,
                                           void* stream) {
    const char* fn = "ndet_scene_accumulate_group";
    NDET_REQUIRE(k >= 1 && k <= 128, NDET_E_UNSUPPORTED, "%s: k=%d views per scene, must be 1 .. 128", fn, k);
    NDET_TRY(group_check(g, sel, k, fn));
    const int N = g->N, C = g->C, n = sel->n;
    NDET_REQUIRE(features_nhwc && mapped_nhwc && bias && rgb && projection && rgb_projection, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(h > 0 && w > 0 && H > 0 && W > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    // a scene's k views are one packed K2 launch's
    NDET_TRY(accumulate_inputs_check(fn, C, g->cm, k, h, w, features_nhwc, view_pitch, row_pitch, mapped_nhwc, mview_pitch, mrow_pitch, bias, W,
                                     rsv, rsc, rsy));
    NdetGateMap gf = {}, gr = {};
    if (gate) NDET_TRY(ndet_gate_prepare(gate, fn, n * k, h, w, H, W, true, &gf, &gr));
    hipStream_t st = (hipStream_t)stream;
    const int n_tiles = (N + VOX_PER_TILE - 1) / VOX_PER_TILE;
    k1_accumulate_dispatch(C, gate != nullptr, [&](auto nc, auto dg) {
        hipLaunchKernelGGL((k_backproject_accumulate_group<decltype(nc)::value, decltype(dg)::value>), dim3(n_tiles, n), dim3(256), 0, st, g->table,
                           *sel, k, features_nhwc, C, h, w, view_pitch, (int)row_pitch, N, projection, (int)g->k1_pitch, n_tiles, gf);
    });
    NDET_CHECK_LAUNCH(fn);
    ndet_scene_k2_accumulate_group_launch(g, sel, k, mapped_nhwc, h, w, (int)mview_pitch, (int)mrow_pitch, bias, rgb, H, W, (int)rsv, (int)rsc,
                                          (int)rsy, projection, rgb_projection, gate != nullptr, gf, gr, st);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_scene_density_finish_group(const NdetSceneGroup* g, const NdetGroupSel* sel, const float* bias, float* global_feat,
                                               void* stream) {
    const char* fn = "ndet_scene_density_finish_group";
    NDET_TRY(group_check(g, sel, 0, fn));
    NDET_REQUIRE(bias, NDET_E_INVALID, "%s: null bias", fn);
    NDET_TRY(finish_out_check(fn, "global_feat", global_feat, 8, false, nullptr, (int64_t)g->N * (g->cm + 3)));
    ndet_scene_k2_finish_group_launch(g, sel, bias, global_feat, (hipStream_t)stream);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_scene_volume_finish_group(const NdetSceneGroup* g, const NdetGroupSel* sel, const float* alpha, float* out, int64_t* count,
                                              void* stream) {
    const char* fn = "ndet_scene_volume_finish_group";
    NDET_TRY(group_check(g, sel, 0, fn));
    const int64_t threads = (int64_t)g->N * (g->C / 4);
    NDET_TRY(finish_out_check(fn, "out", out, 16, true, count, threads));
    hipLaunchKernelGGL(k_volume_finish_group, dim3((unsigned)((threads + 255) / 256), sel->n), dim3(256), 0, (hipStream_t)stream, g->table, *sel,
                       (int)g->k1_pitch, alpha, g->C, g->N, out, count);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ---- entry points: windowed groups ----
extern "C" int ndet_scene_group_ring_check(const NdetSceneGroup* pool, const NdetGroupRingSel* sel, const int32_t* segs_host) {
    return group_ring_check(pool, sel, segs_host, "ndet_scene_group_ring_check");
}

extern "C" int ndet_scene_density_finish_group_ring(const NdetSceneGroup* pool, const NdetGroupRingSel* sel, const int32_t* segs_host,
                                                    const int32_t* segs_dev, const float* bias, float* global_feat, void* stream) {
    const char* fn = "ndet_scene_density_finish_group_ring";
    NDET_TRY(group_ring_check(pool, sel, segs_host, fn));
    NDET_TRY(segs_dev_check(segs_dev, fn));
    NDET_REQUIRE(bias, NDET_E_INVALID, "%s: null bias", fn);
    NDET_TRY(finish_out_check(fn, "global_feat", global_feat, 8, false, nullptr, (int64_t)pool->N * (pool->cm / 4 + 1)));
    ndet_scene_k2_finish_group_ring_launch(pool, sel, segs_dev, bias, global_feat, (hipStream_t)stream);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_scene_volume_finish_group_ring(const NdetSceneGroup* pool, const NdetGroupRingSel* sel, const int32_t* segs_host,
                                                   const int32_t* segs_dev, const float* alpha, float* out, int64_t* count, void* stream) {
    const char* fn = "ndet_scene_volume_finish_group_ring";
    NDET_TRY(group_ring_check(pool, sel, segs_host, fn));
    NDET_TRY(segs_dev_check(segs_dev, fn));
    const int64_t threads = (int64_t)pool->N * (pool->C / 4);
    NDET_TRY(finish_out_check(fn, "out", out, 16, true, count, threads));
    hipLaunchKernelGGL(k_volume_finish_group_ring, dim3((unsigned)((threads + 255) / 256), sel->n), dim3(256), 0, (hipStream_t)stream, pool->table,
                       *sel, segs_dev, (int)pool->k1_pitch, alpha, pool->C, pool->N, out, count);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ------------------------------------------------------------------------------------------
// K2  density conditioning features   A5
//
// One wavefront per voxel, lanes over the 3 + cm channels (35 of 64 lanes at cm = 32): lanes 0-2
// read the three RGB planes at the stride-1 pixel, lanes 3.. read the cm-float row of the mapped
// feature map at the stride-4 pixel, all in one load instruction per view.  A view that does not see
// the voxel contributes the Linear's bias (mapped channels) or 0 (RGB) -- the "0 bias issue" of
// nerfdet.py:233.  Two passes over the views (mean, then squared deviations) as the reference does;
// the second pass re-reads the same few rows from L1/L2.  Views outside the union of the two
// validity masks all contribute the same constant and are folded in as n * const.
// ------------------------------------------------------------------------------------------
// Both validity masks and pixel offsets of one voxel for one 64-view round (lanes over views).
struct DensityRound {
    unsigned long long mf, mr;  // views seeing the voxel in the stride-4 map / in the full-resolution image
    int off_f, off_r;           // per-lane (= per-view) offsets into the mapped map / one RGB plane
    unsigned boff_f, boff_r;    // the same as byte offsets from the tensor base, view included (buffer-load path)
};

template <bool DG>
__device__ __forceinline__ DensityRound density_project(int v, int n_views, const float* __restrict__ proj, const float* __restrict__ rgb_proj,
                                                        float px, float py, float pz, int w, int h, int W, int H, int mrow_pitch, int cm,
                                                        int rsy, int64_t mview_pitch, int64_t rsv, const NdetGateMap& gf, const NdetGateMap& gr) {
    int xf = 0, yf = 0, xr = 0, yr = 0;
    bool okf = false, okr = false;
    if (v < n_views) {
        if (DG) {   // depth gate of both backproject() calls (nerfdet.py:164-169 / 204-210 -> 404-411)
            float zf, zr;
            okf = ndet_project_z(proj + v * 12, px, py, pz, w, h, xf, yf, zf) && ndet_depth_band(gf, v, xf, yf, zf);
            okr = ndet_project_z(rgb_proj + v * 12, px, py, pz, W, H, xr, yr, zr) && ndet_depth_band(gr, v, xr, yr, zr);
        } else {
            okf = ndet_project(proj + v * 12, px, py, pz, w, h, xf, yf);
            okr = ndet_project(rgb_proj + v * 12, px, py, pz, W, H, xr, yr);
        }
    }
    DensityRound r;
    r.off_f = yf * mrow_pitch + xf * cm;
    r.off_r = yr * rsy + xr;
    r.boff_f = (unsigned)((v * mview_pitch + r.off_f) * 4);
    r.boff_r = (unsigned)((v * rsv + r.off_r) * 4);
    r.mf = __ballot(okf);
    r.mr = __ballot(okr);
    return r;
}

// One pass over the union of valid views of a round: PASS 0 accumulates values, PASS 1 squared deviations from `mean`.
template <int PASS>
__device__ __forceinline__ float density_round_pass(const DensityRound& d, int r0, const float* __restrict__ mapped, int64_t mview_pitch,
                                                    const float* __restrict__ rgb, int64_t rsv, int64_t rsc, int lane, int cm, float fill,
                                                    float mean, float acc) {
    const int ch = lane;
    const bool is_rgb = ch < 3;
    const bool active = ch < 3 + cm;
    unsigned long long m = d.mf | d.mr;
    int b = 0;
    while (m) {
        float t[K2_BATCH];
        bool has[K2_BATCH], mine[K2_BATCH];
#pragma unroll
        for (int k = 0; k < K2_BATCH; ++k) {
            has[k] = (m != 0ull);
            if (has[k]) {
                b = __builtin_ctzll(m);
                m &= (m - 1ull);
            }
            const bool vf = (d.mf >> b) & 1ull, vr = (d.mr >> b) & 1ull;
            const int of = __builtin_amdgcn_readlane(d.off_f, b);
            const int orr = __builtin_amdgcn_readlane(d.off_r, b);
            mine[k] = active && (is_rgb ? vr : vf);
            const float* p = is_rgb ? (rgb + (int64_t)(r0 + b) * rsv + (int64_t)ch * rsc + orr)
                                    : (mapped + (int64_t)(r0 + b) * mview_pitch + of + (ch - 3));
            t[k] = mine[k] ? *p : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < K2_BATCH; ++k) {
            if (has[k]) {
                const float val = mine[k] ? t[k] : fill;
                if (PASS == 0) {
                    acc = acc + val;
                } else {
                    const float dd = val - mean;
                    acc = acc + dd * dd;
                }
            }
        }
    }
    return acc;
}

// The same pass with buffer loads: a view's offset (computed by the lane that projected it) becomes the instruction's scalar
// offset, the lane's channel its constant vector offset -- no per-view address arithmetic in the vector unit, which is what
// bounds this kernel (a 140-byte gather per voxel-view: ~30 instructions of pointer math against 2 loads).  Lanes of the other
// kind (and idle lanes) carry an out-of-range offset and read zeros.
#define K2_OOB 0x80000000u
template <int PASS>
__device__ __forceinline__ float density_round_pass_buf(const DensityRound& d, __amdgpu_buffer_rsrc_t mres, __amdgpu_buffer_rsrc_t rres,
                                                        unsigned fvoff, unsigned rvoff, bool is_rgb, float fill, float mean, float acc) {
    unsigned long long m = d.mf | d.mr;
    int b = 0;
    while (m) {
        float tf[K2_BATCH], tr[K2_BATCH];
        bool has[K2_BATCH], vf[K2_BATCH], vr[K2_BATCH];
#pragma unroll
        for (int k = 0; k < K2_BATCH; ++k) {
            has[k] = (m != 0ull);
            if (has[k]) {
                b = __builtin_ctzll(m);
                m &= (m - 1ull);
            }
            vf[k] = has[k] && ((d.mf >> b) & 1ull);
            vr[k] = has[k] && ((d.mr >> b) & 1ull);
            const unsigned of = (unsigned)__builtin_amdgcn_readlane((int)d.boff_f, b);
            const unsigned orr = (unsigned)__builtin_amdgcn_readlane((int)d.boff_r, b);
            tf[k] = vf[k] ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(mres, fvoff, of, 0)) : 0.0f;
            tr[k] = vr[k] ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rres, rvoff, orr, 0)) : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < K2_BATCH; ++k) {
            if (has[k]) {
                const float val = is_rgb ? (vr[k] ? tr[k] : fill) : (vf[k] ? tf[k] : fill);
                if (PASS == 0) {
                    acc = acc + val;
                } else {
                    const float dd = val - mean;
                    acc = acc + dd * dd;
                }
            }
        }
    }
    return acc;
}

template <bool BUF, bool DG>
__global__ __launch_bounds__(256) void k_density_features(const float* __restrict__ mapped, int n_views, int cm, int h, int w,
                                                          int64_t mview_pitch, int mrow_pitch, const float* __restrict__ bias,
                                                          const float* __restrict__ rgb, int H, int W, int64_t rsv, int64_t rsc,
                                                          int rsy, const float* __restrict__ points, int N,
                                                          const float* __restrict__ proj, const float* __restrict__ rgb_proj,
                                                          float* __restrict__ out, int n_tiles, NdetGateMap gf, NdetGateMap gr) {
    constexpr int VPW = VOX_PER_TILE / 4;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tile = ndet_xcd_remap(blockIdx.x, n_tiles);
    const int F = 2 * (3 + cm);
    const float fill = (lane >= 3 && lane < 3 + cm) ? bias[lane - 3] : 0.0f;
    const bool single_round = n_views <= 64;  // the common case: projections are computed once and reused by both passes
    const bool is_rgb = lane < 3;
    // buffer path: per-lane constant offsets (the lane's channel), out of range for lanes of the other kind
    const __amdgpu_buffer_rsrc_t mres = __builtin_amdgcn_make_buffer_rsrc((void*)mapped, 0, K2_OOB, 0x00020000);
    const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc((void*)rgb, 0, K2_OOB, 0x00020000);
    const unsigned fvoff = (lane >= 3 && lane < 3 + cm) ? (unsigned)((lane - 3) * 4) : K2_OOB;
    const unsigned rvoff = is_rgb ? (unsigned)(lane * rsc * 4) : K2_OOB;

    float px[VPW], py[VPW], pz[VPW];
    bool live[VPW];
#pragma unroll
    for (int j = 0; j < VPW; ++j) {
        const int n = tile * VOX_PER_TILE + j * 4 + wave;
        live[j] = n < N;
        const int nn = live[j] ? n : 0;
        px[j] = points[nn]; py[j] = points[N + nn]; pz[j] = points[2 * N + nn];
    }
    // the wave's 4 voxels are projected back to back (lanes over views) before any gather is issued
    DensityRound first[VPW];
#pragma unroll
    for (int j = 0; j < VPW; ++j) first[j] = density_project<DG>(lane, n_views, proj, rgb_proj, px[j], py[j], pz[j], w, h, W, H, mrow_pitch, cm, rsy, mview_pitch, rsv, gf, gr);

#pragma unroll
    for (int j = 0; j < VPW; ++j) {
        if (!live[j]) continue;
        const int n = tile * VOX_PER_TILE + j * 4 + wave;
        float sum = 0.0f;
        int cnt = 0, n_union = 0;
        for (int r0 = 0; r0 < n_views; r0 += 64) {
            const DensityRound d = (r0 == 0) ? first[j]
                                             : density_project<DG>(r0 + lane, n_views, proj, rgb_proj, px[j], py[j], pz[j], w, h, W, H, mrow_pitch, cm, rsy, mview_pitch, rsv, gf, gr);
            cnt += __popcll(d.mf);
            n_union += __popcll(d.mf | d.mr);
            sum = BUF ? density_round_pass_buf<0>(d, mres, rres, fvoff, rvoff, is_rgb, fill, 0.0f, sum)
                      : density_round_pass<0>(d, r0, mapped, mview_pitch, rgb, rsv, rsc, lane, cm, fill, 0.0f, sum);
        }
        const float rest = (float)(n_views - n_union);
        sum = sum + rest * fill;
        const float denom = (float)cnt + 1e-8f;
        const float mean = sum / denom;  // NOT zeroed at cnt == 0 (nerfdet.py:241)
        float ss = 0.0f;
        for (int r0 = 0; r0 < n_views; r0 += 64) {
            const DensityRound d = (r0 == 0 || single_round) ? first[j]
                                                             : density_project<DG>(r0 + lane, n_views, proj, rgb_proj, px[j], py[j], pz[j], w, h, W, H, mrow_pitch, cm, rsy, mview_pitch, rsv, gf, gr);
            ss = BUF ? density_round_pass_buf<1>(d, mres, rres, fvoff, rvoff, is_rgb, fill, mean, ss)
                     : density_round_pass<1>(d, r0, mapped, mview_pitch, rgb, rsv, rsc, lane, cm, fill, mean, ss);
        }
        const float dd = fill - mean;
        ss = ss + rest * (dd * dd);
        float var = ss / denom;
        if (cnt == 0) var = 1e6f;  // nerfdet.py:249
        const float cov = expf(-var);
        if (lane < 3 + cm) *reinterpret_cast<float2*>(out + (int64_t)n * F + 2 * lane) = make_float2(mean, cov);
    }
}

static int density_features_impl(const char* fn, const float* mapped_nhwc, int n_views, int cm, int h, int w, int64_t mview_pitch,
                                 int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv,
                                 int64_t rsc, int64_t rsy, const float* points, int N, const float* projection,
                                 const float* rgb_projection, float* global_feat, const NdetDepthGate* dgate, void* stream) {
    NDET_REQUIRE(mapped_nhwc && bias && rgb && points && projection && rgb_projection && global_feat, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_views > 0 && cm > 0 && h > 0 && w > 0 && H > 0 && W > 0 && N > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(cm <= 61, NDET_E_UNSUPPORTED, "%s: cm=%d mapped channels do not fit one wavefront (max 61)", fn, cm);
    NDET_REQUIRE((int64_t)h * mrow_pitch < (int64_t)1 << 31 && (int64_t)H * rsy < (int64_t)1 << 31, NDET_E_UNSUPPORTED,
                 "%s: one view exceeds 2^31 floats", fn);
    NDET_REQUIRE(((uintptr_t)global_feat & 7) == 0, NDET_E_UNSUPPORTED, "%s: global_feat must be 8-byte aligned", fn);
    NdetGateMap gf = {}, gr = {};
    if (dgate) {
        const int rc = ndet_gate_prepare(dgate, fn, n_views, h, w, H, W, true, &gf, &gr);
        if (rc != NDET_OK) return rc;
    }
    const int n_tiles = (N + VOX_PER_TILE - 1) / VOX_PER_TILE;
    // both tensors within 2 GB: gathers as buffer loads with the view offset in the scalar register
    const bool buf = (int64_t)n_views * mview_pitch * 4 < ((int64_t)1 << 31) && (int64_t)n_views * rsv * 4 < ((int64_t)1 << 31) &&
                     mview_pitch >= 0 && rsv >= 0 && rsc >= 0;
#define K2_LAUNCH(B, DG)                                                                                                                    \
    hipLaunchKernelGGL((k_density_features<B, DG>), dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, mapped_nhwc, n_views, cm, h, w,     \
                       mview_pitch, (int)mrow_pitch, bias, rgb, H, W, rsv, rsc, (int)rsy, points, N, projection, rgb_projection,            \
                       global_feat, n_tiles, gf, gr)
    if (dgate) {
        if (buf) K2_LAUNCH(true, true);
        else K2_LAUNCH(false, true);
    } else {
        if (buf) K2_LAUNCH(true, false);
        else K2_LAUNCH(false, false);
    }
#undef K2_LAUNCH
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_density_features(const float* mapped_nhwc, int n_views, int cm, int h, int w, int64_t mview_pitch,
                                     int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv,
                                     int64_t rsc, int64_t rsy, const float* points, int N, const float* projection,
                                     const float* rgb_projection, float* global_feat, void* stream) {
    return density_features_impl("ndet_density_features", mapped_nhwc, n_views, cm, h, w, mview_pitch, mrow_pitch, bias, rgb, H, W, rsv, rsc,
                                 rsy, points, N, projection, rgb_projection, global_feat, nullptr, stream);
}

extern "C" int ndet_density_features_gated(const float* mapped_nhwc, int n_views, int cm, int h, int w, int64_t mview_pitch,
                                           int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv,
                                           int64_t rsc, int64_t rsy, const float* points, int N, const float* projection,
                                           const float* rgb_projection, float* global_feat, const NdetDepthGate* gate, void* stream) {
    NDET_REQUIRE(gate, NDET_E_INVALID, "ndet_density_features_gated: null depth gate");
    return density_features_impl("ndet_density_features_gated", mapped_nhwc, n_views, cm, h, w, mview_pitch, mrow_pitch, bias, rgb, H, W, rsv,
                                 rsc, rsy, points, N, projection, rgb_projection, global_feat, gate, stream);
}

// ------------------------------------------------------------------------------------------
// A6 pieces: sigma -> alpha, gating (unfused form), MLP input rows
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sigma_to_alpha(const float* __restrict__ raw, float* __restrict__ alpha, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float s = ndet_relu(raw[n]);    // F.relu, nerf_mlp.py:227
    alpha[n] = 1.0f - expf(-s);            // nerfdet.py:257
}

extern "C" int ndet_sigma_to_alpha(const float* raw_sigma, float* alpha, int N, void* stream) {
    NDET_REQUIRE(raw_sigma && alpha, NDET_E_INVALID, "ndet_sigma_to_alpha: null pointer");
    NDET_REQUIRE(N > 0, NDET_E_INVALID, "ndet_sigma_to_alpha: N must be positive");
    hipLaunchKernelGGL(k_sigma_to_alpha, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, raw_sigma, alpha, N);
    NDET_CHECK_LAUNCH("ndet_sigma_to_alpha");
    return NDET_OK;
}

__global__ __launch_bounds__(256) void k_alpha_gate(const float* __restrict__ mean, const float* __restrict__ density,
                                                    const int64_t* __restrict__ count, float* __restrict__ out, int C, int N,
                                                    int layout) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)C * N) return;
    const int n = layout == NDET_LAYOUT_NC ? (int)(i / C) : (int)(i % N);
    const float a = 1.0f - expf(-density[n]);
    out[i] = count[n] == 0 ? 0.0f : a * mean[i];
}

extern "C" int ndet_alpha_gate(const float* mean, const float* density, const int64_t* count, float* out, int C, int N,
                               int layout, void* stream) {
    NDET_REQUIRE(mean && density && count && out, NDET_E_INVALID, "ndet_alpha_gate: null pointer");
    NDET_REQUIRE(C > 0 && N > 0, NDET_E_INVALID, "ndet_alpha_gate: sizes must be positive");
    NDET_REQUIRE(layout == NDET_LAYOUT_CN || layout == NDET_LAYOUT_NC, NDET_E_INVALID, "ndet_alpha_gate: bad layout");
    const int64_t total = (int64_t)C * N;
    hipLaunchKernelGGL(k_alpha_gate, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mean, density,
                       count, out, C, N, layout);
    NDET_CHECK_LAUNCH("ndet_alpha_gate");
    return NDET_OK;
}

__global__ __launch_bounds__(256) void k_posenc_concat(const float* __restrict__ points, const float* __restrict__ glob, int N,
                                                       int F, int K, float* __restrict__ out) {
    // K = row stride >= 63 + F; columns beyond 63 + F are zero (padding to the MFMA kernel's 32-channel K step)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * K) return;
    const int n = (int)(i / K), col = (int)(i % K);
    float r;
    if (col >= 63 + F) {
        r = 0.0f;
    } else if (col >= 63) {
        r = glob[(int64_t)n * F + (col - 63)];
    } else if (col < 3) {
        r = points[col * N + n];
    } else {
        // latent = sin(cat([xb, xb + pi/2])), xb degree-major / xyz-minor (nerf_mlp.py:190-194)
        const int t = col - 3;
        const int half = t >= 30 ? 1 : 0;
        const int k = (t - 30 * half) / 3, d = (t - 30 * half) % 3;
        float xb = points[d * N + n] * (float)(1 << k);
        if (half) xb = xb + 1.57079632679489661923f;
        r = sinf(xb);
    }
    out[i] = r;
}

extern "C" int ndet_posenc_concat(const float* points, const float* global_feat, int N, int F, int out_stride, float* out, void* stream) {
    NDET_REQUIRE(points && out && (global_feat || F == 0), NDET_E_INVALID, "ndet_posenc_concat: null pointer");
    NDET_REQUIRE(N > 0 && F >= 0 && out_stride >= 63 + F, NDET_E_INVALID, "ndet_posenc_concat: bad sizes");
    const int64_t total = (int64_t)N * out_stride;
    hipLaunchKernelGGL(k_posenc_concat, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points,
                       global_feat, N, F, out_stride, out);
    NDET_CHECK_LAUNCH("ndet_posenc_concat");
    return NDET_OK;
}


// ------------------------------------------------------------------------------------------------
// A6 tail: sigma = w . [h | x] + b over the re-joined trunk output (nerf_mlp.py:86,143: the skip concat after the last
// hidden layer feeds the 389 -> 1 sigma layer), then alpha = 1 - exp(-relu(sigma)) (nerf_mlp.py:227, nerfdet.py:257).
// One wavefront per row; the concat is never materialised.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sigma_head(const float* __restrict__ h, int Ch, const float* __restrict__ x, int Cx, int x_stride,
                                                    const float* __restrict__ w, const float* __restrict__ bias, int N,
                                                    float* __restrict__ raw_sigma, float* __restrict__ alpha) {
    const int lane = threadIdx.x & 63;
    const int n = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (n >= N) return;
    float acc = 0.0f;
    for (int c = lane; c < Ch; c += 64) acc = fmaf(h[(int64_t)n * Ch + c], w[c], acc);
    for (int c = lane; c < Cx; c += 64) acc = fmaf(x[(int64_t)n * x_stride + c], w[Ch + c], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        const float sg = acc + bias[0];
        if (raw_sigma) raw_sigma[n] = sg;
        alpha[n] = 1.0f - expf(-ndet_relu(sg));
    }
}

extern "C" int ndet_sigma_head(const float* h, int Ch, const float* x, int Cx, int x_stride, const float* w, const float* bias, int N,
                               float* raw_sigma, float* alpha, void* stream) {
    const char* fn = "ndet_sigma_head";
    NDET_REQUIRE(h && x && w && bias && alpha, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(N > 0 && Ch > 0 && Cx >= 0 && x_stride >= Cx, NDET_E_INVALID, "%s: bad sizes", fn);
    const int64_t blocks = ((int64_t)N + 3) / 4;
    hipLaunchKernelGGL(k_sigma_head, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, h, Ch, x, Cx, x_stride, w, bias, N, raw_sigma,
                       alpha);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
