// K2, packed form: per-voxel NeRF conditioning rows (mmdet3d/models/detectors/nerfdet.py:234-253) for gfx950.
//
// Same statement as k_density_features in volume_kernels.hip (kept for cm % 4 != 0 and for more than 128 views):
//   value of channel c in view v = mapped[v, y4, x4, c] where the stride-4 projection sees the voxel, else the Linear's bias
//                                = rgb[v, c, y1, x1]    where the stride-1 projection sees it, else 0
//   mean = sum over ALL views / (cnt + 1e-8) (cnt = views seeing it in the stride-4 map; not zeroed at cnt == 0),
//   cov  = exp(-sum over ALL views (value - mean)^2 / (cnt + 1e-8)), 0 where cnt == 0.
// What changed is the mapping onto the machine, the same scheme as the packed ray sampler (ray_stats_kernels.hip):
//   * a lane holds one channel QUAD (one 16-byte load per view instead of four 4-byte ones), one more lane the three colour planes;
//   * both projections of a (voxel, view) pair are evaluated once, lanes over views, and parked in LDS as element offsets;
//   * each lane walks only views that see the voxel in ITS map (set bits of its ballot), eight gathers per trip;
//   * one walk: the sum for the mean and the shifted sums for the variance (pivot = the fill value), see the kernel's comment.
// Compiled with -ffp-contract=off.
#include "ndet_common.hpp"

#define DK_ROUNDS 2  // view rounds of 64 kept in registers: n_views <= 128

// One voxel per wavefront.  The voxel's views are dealt round-robin to SPLIT = 64 / (cm/4 + 1) lane groups (7 at cm = 32), each group
// the cm/4 + 1 channel-quad lanes of the scheme above: a voxel seen by all 50 views is ONE trip of eight gathers per lane instead
// of a chain of seven, and the grid is 25 600 waves instead of 3 658 -- the launch used to last as long as its longest chain
// (3.6 waves per SIMD, all resident at once).  The groups share the pivot (the fill value: the Linear's bias / 0), so their partial
// sums add; they meet in LDS.  With pivot = fill the views that do not see the voxel drop out of the shifted sums:
//     sum_all (v - mean)^2 = sum_seen (v - fill)^2 - 2 (mean - fill) sum_seen (v - fill) + n_views (mean - fill)^2.
template <int DUMMY, bool DG>
__global__ __launch_bounds__(256) void k_density_features_packed(const float* __restrict__ mapped, int n_views, int cm, int h, int w,
                                                                 int mview_pitch, int mrow_pitch, const float* __restrict__ bias,
                                                                 const float* __restrict__ rgb, int H, int W, int rsv, int rsc, int rsy,
                                                                 const float* __restrict__ points, int N, const float* __restrict__ proj,
                                                                 const float* __restrict__ rgb_proj, float* __restrict__ out, int n_blocks,
                                                                 int nvp, NdetGateMap gf, NdetGateMap gr) {
    extern __shared__ int2 s_off[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lps = (cm >> 2) + 1;
    const int SPLIT = 64 / lps;
    const int grp = lane / lps, sub = lane - grp * lps;
    const int blk = ndet_xcd_remap(blockIdx.x, n_blocks);      // neighbouring voxel blocks hit the same pixels: keep them on one XCD's L2
    const int n = blk * 4 + wave;                              // this wave's voxel
    int2* rec = s_off + (size_t)wave * nvp;
    float4* part = reinterpret_cast<float4*>(s_off + (size_t)4 * nvp) + (size_t)wave * 64 * 3;   // [lane][acc, q, s1]
    const int rounds = (n_views + 63) >> 6;
    const bool live = n < N;

    // ---- phase 1: lanes over views, both projections of every (voxel, view) pair once ----
    unsigned long long mf[DK_ROUNDS], mr[DK_ROUNDS];
#pragma unroll
    for (int r = 0; r < DK_ROUNDS; ++r) { mf[r] = 0ull; mr[r] = 0ull; }
    if (live) {
        const float px = points[n], py = points[N + n], pz = points[2 * N + n];
#pragma unroll
        for (int r = 0; r < DK_ROUNDS; ++r) {
            if (r < rounds) {
                const int v = r * 64 + lane;
                bool okf = false, okr = false;
                if (v < n_views) {
                    int xf, yf, xr, yr;
                    float zf, zr;
                    okf = ndet_project_z(proj + v * 12, px, py, pz, w, h, xf, yf, zf);
                    okr = ndet_project_z(rgb_proj + v * 12, px, py, pz, W, H, xr, yr, zr);
                    if (DG) {   // depth gate of both backproject() calls (nerfdet.py:404-411)
                        okf = okf && ndet_depth_band(gf, v, xf, yf, zf);
                        okr = okr && ndet_depth_band(gr, v, xr, yr, zr);
                    }
                    rec[v] = make_int2(v * mview_pitch + yf * mrow_pitch + xf * cm, v * rsv + yr * rsy + xr);
                }
                mf[r] = __ballot(okf);
                mr[r] = __ballot(okr);
            }
        }
    }
    __syncthreads();

    // ---- phase 2: lanes over (view group, channel quad) ----
    const bool on = live && grp < SPLIT;
    const bool is_rgb = sub == 0;
    const int fq = sub - 1;
    float4 fill = make_float4(0.f, 0.f, 0.f, 0.f);            // what a view that does not see the voxel contributes (nerfdet.py:233)
    if (!is_rgb && on) fill = *reinterpret_cast<const float4*>(bias + 4 * fq);
    const float* fbase = mapped + 4 * max(fq, 0);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), q = acc, s1 = acc;
    auto fetch = [&](int idx) -> float4 {
        const int2 o = rec[idx];
        if (is_rgb) {
            const float* p = rgb + o.y;
            return make_float4(p[0], p[rsc], p[2 * rsc], 0.0f);
        }
        return *reinterpret_cast<const float4*>(fbase + o.x);
    };
    auto take = [&](const float4& v) {
        acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z; acc.w = acc.w + v.w;
        const float dx = v.x - fill.x, dy = v.y - fill.y, dz = v.z - fill.z, dw = v.w - fill.w;
        q.x = q.x + dx * dx; q.y = q.y + dy * dy; q.z = q.z + dz * dz; q.w = q.w + dw * dw;
        s1.x = s1.x + dx; s1.y = s1.y + dy; s1.z = s1.z + dz; s1.w = s1.w + dw;
    };
    // the views of group g: bits g, g + SPLIT, g + 2 SPLIT, ... of the round's mask
    unsigned long long stripe = 0ull;
    for (int b = grp; b < 64; b += SPLIT) stripe |= 1ull << b;
#pragma unroll
    for (int r = 0; r < DK_ROUNDS; ++r) {
        if (r >= rounds) break;
        unsigned long long m = on ? ((is_rgb ? mr[r] : mf[r]) & stripe) : 0ull;
        while (__ballot(m != 0ull) != 0ull) {
            bool hh[8];
            int bb[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                hh[k] = m != 0ull;
                bb[k] = hh[k] ? __builtin_ctzll(m) : 0;
                m = hh[k] ? (m & (m - 1ull)) : 0ull;
            }
            float4 vv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                vv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (hh[k]) vv[k] = fetch(r * 64 + bb[k]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (hh[k]) take(vv[k]);
        }
    }
    // ---- the groups' partial sums meet in LDS; group 0 finishes the voxel ----
    part[lane * 3 + 0] = acc;
    part[lane * 3 + 1] = q;
    part[lane * 3 + 2] = s1;
    __syncthreads();
    if (!(on && grp == 0)) return;
    for (int g2 = 1; g2 < SPLIT; ++g2) {
        const float4 a2 = part[(g2 * lps + sub) * 3 + 0], q2 = part[(g2 * lps + sub) * 3 + 1], s2 = part[(g2 * lps + sub) * 3 + 2];
        acc.x += a2.x; acc.y += a2.y; acc.z += a2.z; acc.w += a2.w;
        q.x += q2.x; q.y += q2.y; q.z += q2.z; q.w += q2.w;
        s1.x += s2.x; s1.y += s2.y; s1.z += s2.z; s1.w += s2.w;
    }
    int cnt = 0, n_mine = 0;
#pragma unroll
    for (int r = 0; r < DK_ROUNDS; ++r) {
        cnt += __popcll(mf[r]);
        n_mine += __popcll(is_rgb ? mr[r] : mf[r]);
    }
    const float denom = (float)cnt + 1e-8f;
    const float nu = (float)(n_views - n_mine), nv = (float)n_views;
    auto finish = [&](float a, float qq, float ss, float fl, float& mean, float& cov) {
        const float sum = a + nu * fl;
        mean = sum / denom;                                   // NOT zeroed at cnt == 0 (nerfdet.py:241)
        const float dm = mean - fl;
        float s = qq - 2.0f * dm * ss + nv * (dm * dm);
        s = ndet_max(s, 0.0f);                                // a sum of squares: rounding may leave -1 ulp (a NaN stays NaN)
        float var = s / denom;
        if (cnt == 0) var = 1e6f;                             // nerfdet.py:249
        cov = expf(-var);
    };
    float4 mean, cov;
    finish(acc.x, q.x, s1.x, fill.x, mean.x, cov.x);
    finish(acc.y, q.y, s1.y, fill.y, mean.y, cov.y);
    finish(acc.z, q.z, s1.z, fill.z, mean.z, cov.z);
    finish(acc.w, q.w, s1.w, fill.w, mean.w, cov.w);
    const int F = 2 * (3 + cm);
    float* row = out + (int64_t)n * F + (is_rgb ? 0 : 2 * (3 + 4 * fq));   // interleaved [mean_c, cov_c] (nerfdet.py:251-253)
    *reinterpret_cast<float2*>(row + 0) = make_float2(mean.x, cov.x);
    *reinterpret_cast<float2*>(row + 2) = make_float2(mean.y, cov.y);
    *reinterpret_cast<float2*>(row + 4) = make_float2(mean.z, cov.z);
    if (!is_rgb) *reinterpret_cast<float2*>(row + 6) = make_float2(mean.w, cov.w);
}

static int density_features_packed_impl(const char* fn, const float* mapped_nhwc, int n_views, int cm, int h, int w, int64_t mview_pitch,
                                        int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv,
                                        int64_t rsc, int64_t rsy, const float* points, int N, const float* projection,
                                        const float* rgb_projection, float* global_feat, const NdetDepthGate* dgate, void* stream) {
    NDET_REQUIRE(mapped_nhwc && bias && rgb && points && projection && rgb_projection && global_feat, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_views > 0 && cm > 0 && h > 0 && w > 0 && H > 0 && W > 0 && N > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(cm % 4 == 0 && cm <= 128, NDET_E_UNSUPPORTED, "%s: cm=%d must be a multiple of 4, at most 128 (use ndet_density_features)", fn, cm);
    NDET_REQUIRE(n_views <= 64 * DK_ROUNDS, NDET_E_UNSUPPORTED, "%s: %d views exceed %d (use ndet_density_features)", fn, n_views, 64 * DK_ROUNDS);
    NDET_REQUIRE(mrow_pitch >= (int64_t)w * cm && mview_pitch >= (int64_t)h * mrow_pitch && rsy >= W && rsc >= 0 && rsv >= 0, NDET_E_INVALID,
                 "%s: pitches smaller than the maps", fn);
    NDET_REQUIRE((int64_t)n_views * mview_pitch < ((int64_t)1 << 31) && (int64_t)n_views * rsv + 3 * rsc < ((int64_t)1 << 31), NDET_E_UNSUPPORTED,
                 "%s: a source tensor exceeds 2^31 floats", fn);
    NDET_REQUIRE(mview_pitch % 4 == 0 && mrow_pitch % 4 == 0 && (((uintptr_t)mapped_nhwc | (uintptr_t)bias) & 15) == 0, NDET_E_UNSUPPORTED,
                 "%s: mapped features / bias must keep channel quads 16-byte aligned", fn);
    NDET_REQUIRE(((uintptr_t)global_feat & 7) == 0, NDET_E_UNSUPPORTED, "%s: global_feat must be 8-byte aligned", fn);
    const int nvp = ((n_views + 63) / 64) * 64;
    const int lds = 4 * nvp * (int)sizeof(int2) + 4 * 64 * 3 * (int)sizeof(float4);
    const int64_t blocks = ((int64_t)N + 3) / 4;               // one voxel per wavefront
    NDET_REQUIRE(blocks < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: too many voxels", fn);
    NdetGateMap gf = {}, gr = {};
    if (dgate) {
        const int rc = ndet_gate_prepare(dgate, fn, n_views, h, w, H, W, true, &gf, &gr);
        if (rc != NDET_OK) return rc;
    }
    if (dgate)
        hipLaunchKernelGGL((k_density_features_packed<0, true>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, mapped_nhwc, n_views, cm,
                           h, w, (int)mview_pitch, (int)mrow_pitch, bias, rgb, H, W, (int)rsv, (int)rsc, (int)rsy, points, N, projection,
                           rgb_projection, global_feat, (int)blocks, nvp, gf, gr);
    else
        hipLaunchKernelGGL((k_density_features_packed<0, false>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, mapped_nhwc, n_views, cm,
                           h, w, (int)mview_pitch, (int)mrow_pitch, bias, rgb, H, W, (int)rsv, (int)rsc, (int)rsy, points, N, projection,
                           rgb_projection, global_feat, (int)blocks, nvp, gf, gr);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_density_features_packed(const float* mapped_nhwc, int n_views, int cm, int h, int w, int64_t mview_pitch,
                                            int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv,
                                            int64_t rsc, int64_t rsy, const float* points, int N, const float* projection,
                                            const float* rgb_projection, float* global_feat, void* stream) {
    return density_features_packed_impl("ndet_density_features_packed", mapped_nhwc, n_views, cm, h, w, mview_pitch, mrow_pitch, bias, rgb, H, W,
                                        rsv, rsc, rsy, points, N, projection, rgb_projection, global_feat, nullptr, stream);
}

extern "C" int ndet_density_features_packed_gated(const float* mapped_nhwc, int n_views, int cm, int h, int w, int64_t mview_pitch,
                                                  int64_t mrow_pitch, const float* bias, const float* rgb, int H, int W, int64_t rsv,
                                                  int64_t rsc, int64_t rsy, const float* points, int N, const float* projection,
                                                  const float* rgb_projection, float* global_feat, const NdetDepthGate* gate, void* stream) {
    NDET_REQUIRE(gate, NDET_E_INVALID, "ndet_density_features_packed_gated: null depth gate");
    return density_features_packed_impl("ndet_density_features_packed_gated", mapped_nhwc, n_views, cm, h, w, mview_pitch, mrow_pitch, bias, rgb,
                                        H, W, rsv, rsc, rsy, points, N, projection, rgb_projection, global_feat, gate, stream);
}

// ------------------------------------------------------------------------------------------
// Streaming scenes (include/nerfdet_hip.h, NdetSceneAccum): the packed kernel split at its finish.
//
// K2-accumulate adds a launch's (<= 128 views) group-reduced sums and counts to the scene's state: the walk's three sums per channel
// (sum_seen v for the mean, the shifted sums about the fill for the variance) and the two counts the finish needs.  Views that do not see a
// voxel add nothing; they enter only through n_views in the finish.  K2-finish is the packed kernel's finish over the state, expression for
// expression: a state filled by one launch gives its rows bit for bit (0 + x = x).  The state is only read.
//
// The kernels for one state, a ring of states, the listed scenes of a group and the listed scenes' rings share one text of everything
// but their set-up: the walk (k2_packed_sums), the add to the state (k2_state_add), the finish of one value (k2_finish_value), of one
// channel (k2_finish_channel) and of one quad (k2_finish_quad), and the sum over a ring's segments (k2_ring_sums).  Not shared, on
// purpose: k_density_features_packed above keeps its own walk and finish, as k_backproject_aggregate does, whose C = 512 instantiation
// spilled once routed through an inlined helper ("Streaming scenes"); neither one-shot kernel's code object may move.
// ------------------------------------------------------------------------------------------
// What a finishing lane (group 0) of a packed K2 wave holds after the walk over the launch's views and the groups' meeting in LDS.
struct K2Sums {
    float4 acc, q, s1, fill;   // sum_seen v, sum_seen (v - fill)^2, sum_seen (v - fill); the fill of the lane's channels
    int cnt, n_mine;           // views seeing the voxel in the stride-4 map / in the lane's own map
    bool is_rgb;
    int fq, n;                 // channel quad (-1: the colour lane), voxel
};

// Phases 1 and 2 of k_density_features_packed below, for its streaming form k_density_accumulate_packed.  Returns false on the lanes that
// do not finish a voxel (after the workgroup's last barrier).  The one-shot kernel keeps its own copy: inlined through this helper it
// compiles to another register allocation.
template <bool DG>
__device__ __forceinline__ bool k2_packed_sums(int2* s_off, const float* __restrict__ mapped, int n_views, int cm, int h, int w,
                                               int mview_pitch, int mrow_pitch, const float* __restrict__ bias,
                                               const float* __restrict__ rgb, int H, int W, int rsv, int rsc, int rsy,
                                               const float* __restrict__ points, int N, const float* __restrict__ proj,
                                               const float* __restrict__ rgb_proj, int n_blocks, int nvp, const NdetGateMap& gf,
                                               const NdetGateMap& gr, K2Sums& res) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lps = (cm >> 2) + 1;
    const int SPLIT = 64 / lps;
    const int grp = lane / lps, sub = lane - grp * lps;
    const int blk = ndet_xcd_remap(blockIdx.x, n_blocks);      // neighbouring voxel blocks hit the same pixels: keep them on one XCD's L2
    const int n = blk * 4 + wave;                              // this wave's voxel
    int2* rec = s_off + (size_t)wave * nvp;
    float4* part = reinterpret_cast<float4*>(s_off + (size_t)4 * nvp) + (size_t)wave * 64 * 3;   // [lane][acc, q, s1]
    const int rounds = (n_views + 63) >> 6;
    const bool live = n < N;

    // ---- phase 1: lanes over views, both projections of every (voxel, view) pair once ----
    unsigned long long mf[DK_ROUNDS], mr[DK_ROUNDS];
#pragma unroll
    for (int r = 0; r < DK_ROUNDS; ++r) { mf[r] = 0ull; mr[r] = 0ull; }
    if (live) {
        const float px = points[n], py = points[N + n], pz = points[2 * N + n];
#pragma unroll
        for (int r = 0; r < DK_ROUNDS; ++r) {
            if (r < rounds) {
                const int v = r * 64 + lane;
                bool okf = false, okr = false;
                if (v < n_views) {
                    int xf, yf, xr, yr;
                    float zf, zr;
                    okf = ndet_project_z(proj + v * 12, px, py, pz, w, h, xf, yf, zf);
                    okr = ndet_project_z(rgb_proj + v * 12, px, py, pz, W, H, xr, yr, zr);
                    if (DG) {   // depth gate of both backproject() calls (nerfdet.py:404-411)
                        okf = okf && ndet_depth_band(gf, v, xf, yf, zf);
                        okr = okr && ndet_depth_band(gr, v, xr, yr, zr);
                    }
                    rec[v] = make_int2(v * mview_pitch + yf * mrow_pitch + xf * cm, v * rsv + yr * rsy + xr);
                }
                mf[r] = __ballot(okf);
                mr[r] = __ballot(okr);
            }
        }
    }
    __syncthreads();

    // ---- phase 2: lanes over (view group, channel quad) ----
    const bool on = live && grp < SPLIT;
    const bool is_rgb = sub == 0;
    const int fq = sub - 1;
    float4 fill = make_float4(0.f, 0.f, 0.f, 0.f);            // what a view that does not see the voxel contributes (nerfdet.py:233)
    if (!is_rgb && on) fill = *reinterpret_cast<const float4*>(bias + 4 * fq);
    const float* fbase = mapped + 4 * max(fq, 0);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), q = acc, s1 = acc;
    auto fetch = [&](int idx) -> float4 {
        const int2 o = rec[idx];
        if (is_rgb) {
            const float* p = rgb + o.y;
            return make_float4(p[0], p[rsc], p[2 * rsc], 0.0f);
        }
        return *reinterpret_cast<const float4*>(fbase + o.x);
    };
    auto take = [&](const float4& v) {
        acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z; acc.w = acc.w + v.w;
        const float dx = v.x - fill.x, dy = v.y - fill.y, dz = v.z - fill.z, dw = v.w - fill.w;
        q.x = q.x + dx * dx; q.y = q.y + dy * dy; q.z = q.z + dz * dz; q.w = q.w + dw * dw;
        s1.x = s1.x + dx; s1.y = s1.y + dy; s1.z = s1.z + dz; s1.w = s1.w + dw;
    };
    // the views of group g: bits g, g + SPLIT, g + 2 SPLIT, ... of the round's mask
    unsigned long long stripe = 0ull;
    for (int b = grp; b < 64; b += SPLIT) stripe |= 1ull << b;
#pragma unroll
    for (int r = 0; r < DK_ROUNDS; ++r) {
        if (r >= rounds) break;
        unsigned long long m = on ? ((is_rgb ? mr[r] : mf[r]) & stripe) : 0ull;
        while (__ballot(m != 0ull) != 0ull) {
            bool hh[8];
            int bb[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                hh[k] = m != 0ull;
                bb[k] = hh[k] ? __builtin_ctzll(m) : 0;
                m = hh[k] ? (m & (m - 1ull)) : 0ull;
            }
            float4 vv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                vv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (hh[k]) vv[k] = fetch(r * 64 + bb[k]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (hh[k]) take(vv[k]);
        }
    }
    // ---- the groups' partial sums meet in LDS; group 0 finishes the voxel ----
    part[lane * 3 + 0] = acc;
    part[lane * 3 + 1] = q;
    part[lane * 3 + 2] = s1;
    __syncthreads();
    if (!(on && grp == 0)) return false;
    for (int g2 = 1; g2 < SPLIT; ++g2) {
        const float4 a2 = part[(g2 * lps + sub) * 3 + 0], q2 = part[(g2 * lps + sub) * 3 + 1], s2 = part[(g2 * lps + sub) * 3 + 2];
        acc.x += a2.x; acc.y += a2.y; acc.z += a2.z; acc.w += a2.w;
        q.x += q2.x; q.y += q2.y; q.z += q2.z; q.w += q2.w;
        s1.x += s2.x; s1.y += s2.y; s1.z += s2.z; s1.w += s2.w;
    }
    int cnt = 0, n_mine = 0;
#pragma unroll
    for (int r = 0; r < DK_ROUNDS; ++r) {
        cnt += __popcll(mf[r]);
        n_mine += __popcll(is_rgb ? mr[r] : mf[r]);
    }
    res.acc = acc; res.q = q; res.s1 = s1; res.fill = fill;
    res.cnt = cnt; res.n_mine = n_mine; res.is_rgb = is_rgb; res.fq = fq; res.n = n;
    return true;
}

// The accumulate kernels' epilogue: a finishing lane adds its three sums to its quad of the voxel's state row, the colour lane the two
// counts as well.
__device__ __forceinline__ void k2_state_add(const K2Sums& r, float* __restrict__ sum, int pitch, int* __restrict__ count, int cm) {
    const int seg = cm + 4;   // [r g b 0 | cm mapped channels] per sum
    float4* row = reinterpret_cast<float4*>(sum + (int64_t)r.n * pitch + (r.is_rgb ? 0 : 4 + 4 * r.fq));
    row[0] = ndet_add4(row[0], r.acc);
    row[seg / 4] = ndet_add4(row[seg / 4], r.q);
    row[2 * seg / 4] = ndet_add4(row[2 * seg / 4], r.s1);
    if (r.is_rgb) {
        int2* c = reinterpret_cast<int2*>(count) + r.n;
        const int2 c0 = *c;
        *c = make_int2(c0.x + r.cnt, c0.y + r.n_mine);
    }
}

// k_density_features_packed's finish of one channel, expression for expression: [mean, cov] from the channel's three sums a, q, s about
// its fill, the voxel's count in the stride-4 map (cnt) and in the channel's own map (n_mine), and the scene's view total.
__device__ __forceinline__ float2 k2_finish_value(float a, float q, float s, float fill, int cnt, int n_mine, int n_views) {
    const float denom = (float)cnt + 1e-8f;
    const float nu = (float)(n_views - n_mine), nv = (float)n_views;
    const float sm = a + nu * fill;
    const float mean = sm / denom;                        // NOT zeroed at cnt == 0 (nerfdet.py:241)
    const float dm = mean - fill;
    float sq = q - 2.0f * dm * s + nv * (dm * dm);
    sq = ndet_max(sq, 0.0f);                              // a sum of squares: rounding may leave -1 ulp (a NaN stays NaN)
    float var = sq / denom;
    if (cnt == 0) var = 1e6f;                             // nerfdet.py:249
    return make_float2(mean, expf(-var));
}

// Channel c (0 .. 2 colour, 3 .. the mapped ones) of voxel n, from a state to the voxel's output row.
__device__ __forceinline__ void k2_finish_channel(const float* __restrict__ sum, int pitch, const int* __restrict__ count,
                                                  const float* __restrict__ bias, int cm, int n, int c, int n_views,
                                                  float* __restrict__ out_row) {
    const bool is_rgb = c < 3;
    const int k = is_rgb ? c : c + 1;          // column inside a segment
    const int seg = cm + 4;
    const float* row = sum + (int64_t)n * pitch;
    const float a = row[k], qq = row[seg + k], ss = row[2 * seg + k];
    const float fl = is_rgb ? 0.0f : bias[c - 3];
    const int cnt = count[2 * n], n_mine = is_rgb ? count[2 * n + 1] : cnt;
    *reinterpret_cast<float2*>(out_row + 2 * c) = k2_finish_value(a, qq, ss, fl, cnt, n_mine, n_views);
}

// Quad qd of voxel n -- quad 0 the colour lane [r g b 0], quads 1 .. cm / 4 the mapped channels -- summed over a ring's segments (Segs:
// NdetRingArgSegs or NdetRingLdsSegs, ndet_common.hpp) with 16-byte loads of the three sums, and the voxel's two counts.  The sums and
// counts start from the oldest segment's values and take the others in array order, NDET_RING_BATCH segments at a time: counts first,
// then the rows of the segments that see the voxel in the quad's own map (the others hold zeros there), then the adds.
template <class Segs>
__device__ __forceinline__ void k2_ring_sums(const Segs& g, int n_segs, int cm, int n, int qd, float4& a, float4& qq, float4& ss, int& cnt,
                                             int& n_mine) {
    constexpr int U = NDET_RING_BATCH;
    const bool is_rgb = qd == 0;
    const int seg = cm + 4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    auto counts = [&](int sj, int& c_f, int& c_mine) {
        const int2 c = *reinterpret_cast<const int2*>(g.count(sj) + 2 * n);
        c_f = c.x;
        c_mine = is_rgb ? c.y : c.x;
    };
    counts(0, cnt, n_mine);
    a = zero; qq = zero; ss = zero;
    if (n_mine != 0) {
        const float* row = g.sum(0) + (int64_t)n * g.pitch(0) + 4 * qd;
        a = *reinterpret_cast<const float4*>(row);
        qq = *reinterpret_cast<const float4*>(row + seg);
        ss = *reinterpret_cast<const float4*>(row + 2 * seg);
    }
    for (int s0 = 1; s0 < n_segs; s0 += U) {
        int cc[U], mm[U];
        float4 va[U], vq[U], vs[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {      // unconditional loads (past the end: the last segment's counts again, dropped), so all U are in flight
            const bool in = s0 + j < n_segs;
            counts(min(s0 + j, n_segs - 1), cc[j], mm[j]);
            cc[j] = in ? cc[j] : 0;
            mm[j] = in ? mm[j] : 0;
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            va[j] = zero; vq[j] = zero; vs[j] = zero;
            if (mm[j] != 0) {      // implies s0 + j < n_segs
                const float* row = g.sum(s0 + j) + (int64_t)n * g.pitch(s0 + j) + 4 * qd;
                va[j] = *reinterpret_cast<const float4*>(row);
                vq[j] = *reinterpret_cast<const float4*>(row + seg);
                vs[j] = *reinterpret_cast<const float4*>(row + 2 * seg);
            }
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            a = ndet_add4(a, va[j]);
            qq = ndet_add4(qq, vq[j]);
            ss = ndet_add4(ss, vs[j]);
            cnt += cc[j];
            n_mine += mm[j];
        }
    }
}

// Every component of quad qd through k2_finish_value, to the voxel's output row: one segment gives k_density_finish's rows bit for bit.
// One sequence for both kinds of quad -- the colour quad's fill is 0 and it has no fourth value -- because written as a branch each the
// ring kernels came out up to 7 % longer than with the expressions in place ("One body per streaming kernel family").
__device__ __forceinline__ void k2_finish_quad(float4 a, float4 qq, float4 ss, int cnt, int n_mine, int n_views, const float* __restrict__ bias,
                                               int qd, float* __restrict__ out_row) {
    const bool is_rgb = qd == 0;
    const int c = 4 * (qd - 1);                               // first mapped channel of the quad
    float4 fl = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!is_rgb) fl = make_float4(bias[c], bias[c + 1], bias[c + 2], bias[c + 3]);
    float2* o = reinterpret_cast<float2*>(out_row) + (is_rgb ? 0 : 3 + c);
    o[0] = k2_finish_value(a.x, qq.x, ss.x, fl.x, cnt, n_mine, n_views);
    o[1] = k2_finish_value(a.y, qq.y, ss.y, fl.y, cnt, n_mine, n_views);
    o[2] = k2_finish_value(a.z, qq.z, ss.z, fl.z, cnt, n_mine, n_views);
    if (!is_rgb) o[3] = k2_finish_value(a.w, qq.w, ss.w, fl.w, cnt, n_mine, n_views);
}

template <bool DG>
__global__ __launch_bounds__(256) void k_density_accumulate_packed(const float* __restrict__ mapped, int n_views, int cm, int h, int w,
                                                                   int mview_pitch, int mrow_pitch, const float* __restrict__ bias,
                                                                   const float* __restrict__ rgb, int H, int W, int rsv, int rsc, int rsy,
                                                                   const float* __restrict__ points, int N, const float* __restrict__ proj,
                                                                   const float* __restrict__ rgb_proj, float* __restrict__ sum, int pitch,
                                                                   int* __restrict__ count, int n_blocks, int nvp, NdetGateMap gf, NdetGateMap gr) {
    extern __shared__ int2 s_off[];
    K2Sums r;
    if (!k2_packed_sums<DG>(s_off, mapped, n_views, cm, h, w, mview_pitch, mrow_pitch, bias, rgb, H, W, rsv, rsc, rsy, points, N, proj, rgb_proj,
                            n_blocks, nvp, gf, gr, r))
        return;
    k2_state_add(r, sum, pitch, count, cm);
}

// The listed scenes of a group (include/nerfdet_hip.h, ndet_scene_accumulate_group), grid.y = listed scene: the block takes its scene's
// state and points from the device table, moves the mapped maps, images, projections and gate maps on by y * k views and runs the packed
// walk over the scene's k views; the offsets the walk records stay inside those (k * mview_pitch and k * rsv below 2^31, checked on the
// host).
template <bool DG>
__global__ __launch_bounds__(256) void k_density_accumulate_group(const NdetSceneSlot* __restrict__ table, NdetGroupSel sel, int k,
                                                                  const float* __restrict__ mapped_all, int cm, int h, int w, int mview_pitch,
                                                                  int mrow_pitch, const float* __restrict__ bias, const float* __restrict__ rgb_all,
                                                                  int H, int W, int rsv, int rsc, int rsy, int N,
                                                                  const float* __restrict__ proj_all, const float* __restrict__ rgb_proj_all,
                                                                  int pitch, int n_blocks, int nvp, NdetGateMap gf_all, NdetGateMap gr_all) {
    extern __shared__ int2 s_off[];
    const int y = blockIdx.y;
    const NdetSceneSlot& sl = table[sel.slot[y]];
    const int64_t v0 = (int64_t)y * k;                         // the scene's first view of the call
    K2Sums r;
    if (!k2_packed_sums<DG>(s_off, mapped_all + v0 * mview_pitch, k, cm, h, w, mview_pitch, mrow_pitch, bias, rgb_all + v0 * rsv, H, W, rsv, rsc,
                            rsy, sl.points, N, proj_all + v0 * 12, rgb_proj_all + v0 * 12, n_blocks, nvp,
                            DG ? ndet_gate_from_view(gf_all, v0) : gf_all, DG ? ndet_gate_from_view(gr_all, v0) : gr_all, r))
        return;
    k2_state_add(r, sl.k2_sum, pitch, sl.k2_count, cm);
}

// One thread per (voxel, channel); the grouped kernel writes output row y N + n and finishes over the scene's own view total.
__global__ __launch_bounds__(256) void k_density_finish(const float* __restrict__ sum, int pitch, const int* __restrict__ count,
                                                        const float* __restrict__ bias, int cm, int N, int n_views, float* __restrict__ out) {
    const int nc = 3 + cm;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * nc) return;
    const int n = (int)(i / nc), c = (int)(i % nc);
    k2_finish_channel(sum, pitch, count, bias, cm, n, c, n_views, out + (int64_t)n * 2 * nc);
}

__global__ __launch_bounds__(256) void k_density_finish_group(const NdetSceneSlot* __restrict__ table, NdetGroupSel sel, int pitch,
                                                              const float* __restrict__ bias, int cm, int N, float* __restrict__ out) {
    const int nc = 3 + cm;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * nc) return;
    const int y = blockIdx.y;
    const NdetSceneSlot& sl = table[sel.slot[y]];
    const int n = (int)(i / nc), c = (int)(i % nc);
    k2_finish_channel(sl.k2_sum, pitch, sl.k2_count, bias, cm, n, c, sel.n_views[y], out + ((int64_t)y * N + n) * 2 * nc);
}

// One thread per (voxel, channel quad) over a ring of states (include/nerfdet_hip.h, ndet_scene_density_finish_ring).
__global__ __launch_bounds__(256) void k_density_finish_ring(NdetRingArgs r, int n_segs, const float* __restrict__ bias, int cm, int N,
                                                             int n_views, float* __restrict__ out) {
    const int nq = (cm >> 2) + 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * nq) return;
    const int n = (int)(i / nq), qd = (int)(i % nq);
    float4 a, qq, ss;
    int cnt, n_mine;
    k2_ring_sums(NdetRingArgSegs{r}, n_segs, cm, n, qd, a, qq, ss, cnt, n_mine);
    k2_finish_quad(a, qq, ss, cnt, n_mine, n_views, bias, qd, out + (int64_t)n * 2 * (3 + cm));
}

// The listed scenes of a windowed group (include/nerfdet_hip.h, ndet_scene_density_finish_group_ring), grid.y = listed scene: the scene's
// segments are rows segs[y][0 .. n_segs - 1] of the pool table.  Threads 0 .. n_segs - 1 resolve them into LDS once (block-uniform
// pointers, 64 x 16 bytes), one barrier, then the ring walk with the pool's pitch; threads past N nq stay for the barrier and do nothing
// after it.  Output row y N + n, finished over the scene's own view total.
__global__ __launch_bounds__(256) void k_density_finish_group_ring(const NdetSceneSlot* __restrict__ table, NdetGroupRingSel sel,
                                                                   const int32_t* __restrict__ segs, int pitch,
                                                                   const float* __restrict__ bias, int cm, int N, float* __restrict__ out) {
    __shared__ const float* s_sum[NDET_RING_MAX];
    __shared__ const int* s_count[NDET_RING_MAX];
    const int y = blockIdx.y;
    const int n_segs = sel.n_segs[y];
    const int n_views = sel.n_views[y];
    if ((int)threadIdx.x < n_segs) {
        const NdetSceneSlot& sl = table[segs[y * NDET_RING_MAX + threadIdx.x]];
        s_sum[threadIdx.x] = sl.k2_sum;
        s_count[threadIdx.x] = sl.k2_count;
    }
    __syncthreads();
    const int nq = (cm >> 2) + 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)N * nq) {
        const int n = (int)(i / nq), qd = (int)(i % nq);
        float4 a, qq, ss;
        int cnt, n_mine;
        k2_ring_sums(NdetRingLdsSegs{s_sum, s_count, pitch}, n_segs, cm, n, qd, a, qq, ss, cnt, n_mine);
        k2_finish_quad(a, qq, ss, cnt, n_mine, n_views, bias, qd, out + ((int64_t)y * N + n) * 2 * (3 + cm));
    }
}

// ---- launchers (ndet_common.hpp), called by the entry points in volume_kernels.hip once every argument has been checked ----
void ndet_scene_k2_accumulate_launch(const NdetSceneAccum* s, const float* mapped, int n_views, int h, int w, int mview_pitch, int mrow_pitch,
                                     const float* bias, const float* rgb, int H, int W, int rsv, int rsc, int rsy, const float* points,
                                     const float* proj, const float* rgb_proj, bool gated, const NdetGateMap& gf, const NdetGateMap& gr,
                                     hipStream_t stream) {
    const int nvp = ((n_views + 63) / 64) * 64;
    const int lds = 4 * nvp * (int)sizeof(int2) + 4 * 64 * 3 * (int)sizeof(float4);
    const int blocks = (s->N + 3) / 4;
    ndet_by_flag(gated, [&](auto dg) {
        hipLaunchKernelGGL((k_density_accumulate_packed<decltype(dg)::value>), dim3((unsigned)blocks), dim3(256), lds, stream, mapped, n_views,
                           s->cm, h, w, mview_pitch, mrow_pitch, bias, rgb, H, W, rsv, rsc, rsy, points, s->N, proj, rgb_proj, s->k2_sum,
                           (int)s->k2_pitch, s->k2_count, blocks, nvp, gf, gr);
    });
}

void ndet_scene_k2_accumulate_group_launch(const NdetSceneGroup* g, const NdetGroupSel* sel, int k, const float* mapped, int h, int w,
                                           int mview_pitch, int mrow_pitch, const float* bias, const float* rgb, int H, int W, int rsv, int rsc,
                                           int rsy, const float* proj, const float* rgb_proj, bool gated, const NdetGateMap& gf,
                                           const NdetGateMap& gr, hipStream_t stream) {
    const int nvp = ((k + 63) / 64) * 64;
    const int lds = 4 * nvp * (int)sizeof(int2) + 4 * 64 * 3 * (int)sizeof(float4);
    const int blocks = (g->N + 3) / 4;
    ndet_by_flag(gated, [&](auto dg) {
        hipLaunchKernelGGL((k_density_accumulate_group<decltype(dg)::value>), dim3((unsigned)blocks, sel->n), dim3(256), lds, stream, g->table,
                           *sel, k, mapped, g->cm, h, w, mview_pitch, mrow_pitch, bias, rgb, H, W, rsv, rsc, rsy, g->N, proj, rgb_proj,
                           (int)g->k2_pitch, blocks, nvp, gf, gr);
    });
}

void ndet_scene_k2_finish_launch(const NdetSceneAccum* s, const float* bias, float* global_feat, hipStream_t stream) {
    const int64_t total = (int64_t)s->N * (3 + s->cm);
    hipLaunchKernelGGL(k_density_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, s->k2_sum, (int)s->k2_pitch, s->k2_count,
                       bias, s->cm, s->N, s->n_views, global_feat);
}

void ndet_scene_k2_finish_group_launch(const NdetSceneGroup* g, const NdetGroupSel* sel, const float* bias, float* global_feat,
                                       hipStream_t stream) {
    const int64_t total = (int64_t)g->N * (3 + g->cm);
    hipLaunchKernelGGL(k_density_finish_group, dim3((unsigned)((total + 255) / 256), sel->n), dim3(256), 0, stream, g->table, *sel,
                       (int)g->k2_pitch, bias, g->cm, g->N, global_feat);
}

void ndet_scene_k2_finish_ring_launch(const NdetSceneAccum* segs, int n_segs, int n_views, const float* bias, float* global_feat,
                                      hipStream_t stream) {
    NdetRingArgs r = {};
    for (int i = 0; i < n_segs; ++i) {
        r.sum[i] = segs[i].k2_sum;
        r.count[i] = segs[i].k2_count;
        r.pitch[i] = (int)segs[i].k2_pitch;
    }
    const int64_t total = (int64_t)segs[0].N * (segs[0].cm / 4 + 1);
    hipLaunchKernelGGL(k_density_finish_ring, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, r, n_segs, bias, segs[0].cm,
                       segs[0].N, n_views, global_feat);
}

void ndet_scene_k2_finish_group_ring_launch(const NdetSceneGroup* pool, const NdetGroupRingSel* sel, const int32_t* segs_dev, const float* bias,
                                            float* global_feat, hipStream_t stream) {
    const int64_t total = (int64_t)pool->N * (pool->cm / 4 + 1);
    hipLaunchKernelGGL(k_density_finish_group_ring, dim3((unsigned)((total + 255) / 256), sel->n), dim3(256), 0, stream, pool->table, *sel,
                       segs_dev, (int)pool->k2_pitch, bias, pool->cm, pool->N, global_feat);
}
