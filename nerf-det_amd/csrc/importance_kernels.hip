// Hierarchical (importance) sampling of the NeRF ray branch on gfx950.
//   k_sample_pdf         sample_pdf() of mmdet3d/models/model_utils/render_ray.py:96-142, exact API form, `u` supplied by the caller
//   k_importance_merge   the fine-pass set-up of render_ray.py:343-356 fused: mid-point bins, inner weights, the draw, the sorted merge
//                        of coarse and fine depths and the points z * ray_d + ray_o
// Mapping: ONE WAVEFRONT PER RAY, four rays per 256-thread workgroup.  A ray's cdf and bins (M + 1 <= 255 floats each) and its merge
// buffer (<= 512 floats) live in the wave's own slice of LDS; the waves of a workgroup share nothing, so there is NO workgroup barrier
// anywhere in this file -- a wave whose ray index is past R (wave-uniform) simply returns.  A wave's LDS accesses complete in program
// order; wave_sync() only keeps the compiler from moving them across the phase boundaries.
//
// Order of the sums (fixed, so results repeat from run to run; torch's own orders differ, so agreement with it is a tolerance):
//   sum(w)   lane l adds w[l], w[l + 64], w[l + 128], w[l + 192] in that order (w = weights + 1e-5, skipping i >= M), then a butterfly
//            over the wave: partner lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 -- every lane ends with the same bits.
//   cumsum   C = ceil(M / 64); lane l owns the C consecutive bins l*C .. l*C + C - 1 and forms their running sum left to right from 0;
//            the lanes' totals are scanned serially in lane order, off[0] = 0, off[l + 1] = off[l] + total[l]; cdf[i + 1] =
//            off[l] + running[i].  A lane's last cdf value IS off[l + 1] (the same add), so the cdf is non-decreasing by construction
//            and the reference's count `above = #{i < M : u >= cdf[i]}` is a binary search.
// Every operation is rounded on its own (-ffp-contract=off); `/` is IEEE correctly rounded.
#include "ndet_common.hpp"

#define IMP_RAYS_PER_WG 4
#define IMP_MAX_BINS 256   // M + 1 <= 255
#define IMP_MAX_MERGE 512  // S + n_imp <= 512

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float lane_value(float v, int l) {  // l wave-uniform
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// render_ray.py:105-110: cdf (M + 1 floats, LDS) of one ray's weights w (M floats, global; NOT modified -- the reference adds 1e-5 in
// place, on a clone).  1 <= M <= 254.  Ends with a wave_sync.
__device__ __forceinline__ void imp_build_cdf(const float* __restrict__ w, int M, float* cdf, int lane) {
    float acc = 0.0f;
    for (int i = lane; i < M; i += 64) acc = acc + (w[i] + 1e-5f);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off);
    const float total = acc;
    const int C = (M + 63) >> 6;                             // 1 .. 4 bins per lane
    float run[4];
    float r = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane * C + k;
        if (k < C && i < M) r = r + (w[i] + 1e-5f) / total;  // pdf = weights / sum(weights)
        run[k] = r;
    }
    float off = 0.0f, s = 0.0f;
    const int used = (M + C - 1) / C;                        // lanes that own a bin
    for (int l = 0; l < used; ++l) {
        if (lane == l) off = s;
        s = s + lane_value(r, l);
    }
    if (lane == 0) cdf[0] = 0.0f;                            // cat([zeros, cdf])
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane * C + k;
        if (k < C && i < M) cdf[i + 1] = off + run[k];
    }
    wave_sync();
}

// render_ray.py:119-140 for one u against one ray's cdf and bins (M + 1 floats each, LDS).
__device__ __forceinline__ float imp_invert(const float* cdf, const float* bins, int M, float u) {
    int lo = 0, hi = M;                                      // above = #{i < M : u >= cdf[i]}, cdf non-decreasing
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u >= cdf[mid]) lo = mid + 1;
        else hi = mid;
    }
    const int above = lo;
    const int below = max(above - 1, 0);
    const float c0 = cdf[below];
    float denom = cdf[above] - c0;
    if (denom < 1e-5f) denom = 1.0f;
    const float t = (u - c0) / denom;
    const float b0 = bins[below];
    float s = b0 + t * (bins[above] - b0);
    // The one step the reference does not have: keep the sample inside the bins' span.  The rounded cdf may end a few ulps below 1, and
    // at u = 1.0 (the last entry of every det row) t then exceeds 1: the reference's own float32 result lands up to 2e-4 beyond bins[M]
    // where the last bin carries only the 1e-5 floor.  Nothing changes for u < cdf[M] beyond the last bit; a NaN stays a NaN.
    if (s > bins[M]) s = bins[M];
    if (s < bins[0]) s = bins[0];
    return s;
}

// The draw both entry points share: n_out samples of one ray, lanes striding over them; each goes to dst_lds[j] and / or dst_glob[j]
// (either may be null).  cdf must have been built (imp_build_cdf) and bins written and synchronised.
__device__ __forceinline__ void imp_draw(const float* cdf, const float* bins, int M, const float* __restrict__ u, int n_out,
                                         float* dst_lds, float* __restrict__ dst_glob, int lane) {
    for (int j = lane; j < n_out; j += 64) {
        const float s = imp_invert(cdf, bins, M, u[j]);
        if (dst_lds) dst_lds[j] = s;
        if (dst_glob) dst_glob[j] = s;
    }
}

__global__ __launch_bounds__(256) void k_sample_pdf(const float* __restrict__ bins, const float* __restrict__ weights, int R, int M,
                                                    const float* __restrict__ u, int u_row_stride, int n_out,
                                                    float* __restrict__ samples) {
    __shared__ float lds[IMP_RAYS_PER_WG][2 * IMP_MAX_BINS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * IMP_RAYS_PER_WG + wv;
    if (r >= R) return;                                      // wave-uniform; no workgroup barrier in this kernel
    float* cdf = lds[wv];
    float* b = lds[wv] + IMP_MAX_BINS;
    for (int i = lane; i <= M; i += 64) b[i] = bins[r * (M + 1) + i];
    imp_build_cdf(weights + r * M, M, cdf, lane);            // ends with wave_sync: b is visible too
    imp_draw(cdf, b, M, u + r * u_row_stride, n_out, nullptr, samples + r * n_out, lane);
}

__global__ __launch_bounds__(256) void k_importance_merge(const float* __restrict__ z_vals, const float* __restrict__ weights,
                                                          const float* __restrict__ ray_o, const float* __restrict__ ray_d, int R, int S,
                                                          const float* __restrict__ u, int u_row_stride, int n_imp,
                                                          float* __restrict__ z_out, float* __restrict__ pts_out,
                                                          float* __restrict__ z_samples_out) {
    __shared__ float lds[IMP_RAYS_PER_WG][2 * IMP_MAX_BINS + IMP_MAX_MERGE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * IMP_RAYS_PER_WG + wv;
    if (r >= R) return;                                      // wave-uniform; no workgroup barrier in this kernel
    float* cdf = lds[wv];
    float* b = lds[wv] + IMP_MAX_BINS;
    float* buf = lds[wv] + 2 * IMP_MAX_BINS;
    const int M = S - 2, S_tot = S + n_imp;
    int P = 4;                                               // bitonic size: the power of two >= S_tot (<= 512)
    while (P < S_tot) P <<= 1;
    for (int i = lane; i < S; i += 64) buf[i] = z_vals[r * S + i];
    for (int i = S_tot + lane; i < P; i += 64) buf[i] = __builtin_inff();
    wave_sync();
    for (int i = lane; i < S - 1; i += 64) b[i] = 0.5f * (buf[i + 1] + buf[i]);   // .5 * (z[1:] + z[:-1]), render_ray.py:343
    imp_build_cdf(weights + r * S + 1, M, cdf, lane);        // weights[:, 1:-1], render_ray.py:344
    imp_draw(cdf, b, M, u + r * u_row_stride, n_imp, buf + S, z_samples_out ? z_samples_out + r * n_imp : nullptr, lane);
    wave_sync();
    // torch.sort(cat(z_vals, z_samples)) as a bitonic network over the P slots (padding +inf sorts last); only values move, so equal
    // depths may land in either order
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const float a = buf[i], c = buf[p];
                const bool up = (i & k) == 0;
                if ((a > c) == up) {
                    buf[i] = c;
                    buf[p] = a;
                }
            }
            wave_sync();
        }
    }
    for (int i = lane; i < S_tot; i += 64) z_out[r * S_tot + i] = buf[i];
    const float ox = ray_o[r * 3], oy = ray_o[r * 3 + 1], oz = ray_o[r * 3 + 2];
    const float dx = ray_d[r * 3], dy = ray_d[r * 3 + 1], dz = ray_d[r * 3 + 2];
    float* __restrict__ p_out = pts_out + r * S_tot * 3;
    for (int e = lane; e < 3 * S_tot; e += 64) {             // z * ray_d + ray_o: a multiply, then an add (k_sample_rays, render_ray.py:356)
        const int s = e / 3, c = e - 3 * s;
        const float d = c == 0 ? dx : (c == 1 ? dy : dz), o = c == 0 ? ox : (c == 1 ? oy : oz);
        p_out[e] = buf[s] * d + o;
    }
}

extern "C" int ndet_sample_pdf(const float* bins, const float* weights, int R, int M, const float* u, int u_row_stride, int n_out,
                               float* samples, void* stream) {
    const char* fn = "ndet_sample_pdf";
    NDET_REQUIRE(bins && weights && u && samples, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(R >= 1 && M >= 1 && n_out >= 1, NDET_E_INVALID, "%s: need R >= 1, M >= 1 and n_out >= 1", fn);
    NDET_REQUIRE(u_row_stride == 0 || u_row_stride == n_out, NDET_E_INVALID, "%s: u_row_stride=%d is neither 0 nor n_out=%d", fn,
                 u_row_stride, n_out);
    NDET_REQUIRE(M <= IMP_MAX_BINS - 2, NDET_E_UNSUPPORTED, "%s: M=%d bins (max %d)", fn, M, IMP_MAX_BINS - 2);
    NDET_REQUIRE(n_out <= 256, NDET_E_UNSUPPORTED, "%s: n_out=%d samples a ray (max 256)", fn, n_out);
    NDET_REQUIRE((int64_t)R * (M + 1 + n_out) < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: R * (M + 1 + n_out) reaches 2^31", fn);
    const unsigned blocks = (unsigned)(((int64_t)R + IMP_RAYS_PER_WG - 1) / IMP_RAYS_PER_WG);
    hipLaunchKernelGGL(k_sample_pdf, dim3(blocks), dim3(64 * IMP_RAYS_PER_WG), 0, (hipStream_t)stream, bins, weights, R, M, u, u_row_stride,
                       n_out, samples);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_importance_merge(const float* z_vals, const float* weights, const float* ray_o, const float* ray_d, int R, int S,
                                     const float* u, int u_row_stride, int n_imp, float* z_out, float* pts_out, float* z_samples_out,
                                     void* stream) {
    const char* fn = "ndet_importance_merge";
    NDET_REQUIRE(z_vals && weights && ray_o && ray_d && u && z_out && pts_out, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(R >= 1 && S >= 3 && n_imp >= 1, NDET_E_INVALID, "%s: need R >= 1, S >= 3 and n_imp >= 1", fn);
    NDET_REQUIRE(u_row_stride == 0 || u_row_stride == n_imp, NDET_E_INVALID, "%s: u_row_stride=%d is neither 0 nor n_imp=%d", fn,
                 u_row_stride, n_imp);
    NDET_REQUIRE(S <= 256, NDET_E_UNSUPPORTED, "%s: S=%d coarse samples a ray (max 256)", fn, S);
    NDET_REQUIRE(n_imp <= 256, NDET_E_UNSUPPORTED, "%s: n_imp=%d fine samples a ray (max 256)", fn, n_imp);
    NDET_REQUIRE((int64_t)R * (S + n_imp) < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: R * (S + n_imp) reaches 2^31", fn);
    const unsigned blocks = (unsigned)(((int64_t)R + IMP_RAYS_PER_WG - 1) / IMP_RAYS_PER_WG);
    hipLaunchKernelGGL(k_importance_merge, dim3(blocks), dim3(64 * IMP_RAYS_PER_WG), 0, (hipStream_t)stream, z_vals, weights, ray_o, ray_d,
                       R, S, u, u_row_stride, n_imp, z_out, pts_out, z_samples_out);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
