// Empty-space skipping for renders from a streamed scene (nerf-det_amd/streaming.py, skip_empty=), for gfx950:
//   * ndet_occupancy_bits       the alpha a detect() computes at the voxel lattice (1 - exp(-relu(sigma)), nerfdet.py:255-257) -> a
//                               dilated bit grid (grid_common.hpp);
//   * ndet_cull_count / _write  ordered compaction of sample points against that grid: the kept flat indices ascending, and their
//                               points, the same bytes on every call (wave ballots and prefix popcounts, no atomics);
//   * ndet_ray_view_count_bank  the view-bank sampler's count pass alone (ray_stats_kernels.hip, rb_project_round<false>): the valid
//                               views of every sample through ndet_ray_project, lanes over views, no gathers.
// A sample whose raw row is zero is an exact no-op in k_composite (ray_kernels.hip: a = 1 - expf(-0) = 0, wgt = 0, T (1 - 0 + 1e-10f) =
// T), so "skipped" means "sigma = 0".  Plain vector stores only.  Compiled with -ffp-contract=off.
#include "grid_common.hpp"

// ------------------------------------------------------------------------------------------------
// alpha -> bits.  One thread per voxel; a wave's ballot is two whole words (64 consecutive voxels, 256 per workgroup).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool se_solid(const float* __restrict__ alpha, const int64_t* __restrict__ count, int n, float threshold) {
    return !(alpha[n] <= threshold) || count[n] == 0;       // NaN: solid; a voxel no view saw: solid (nothing is known about it)
}

__global__ __launch_bounds__(256) void k_occupancy_bits(const float* __restrict__ alpha, const int64_t* __restrict__ count, int nx, int ny, int nz,
                                                        int n_total, float threshold, int dilate, uint32_t* __restrict__ bits, int n_words) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool set = t < n_total && ndet_any_neighbour((int)t, nx, ny, nz, dilate,
                                                       [&](int, int, int, int m) { return se_solid(alpha, count, m, threshold); });
    ndet_ballot_store_words(set, t, bits, n_words);
}

extern "C" int ndet_occupancy_bits(const float* alpha, const int64_t* count, int nx, int ny, int nz, float threshold, int dilate,
                                   uint32_t* bits, void* stream) {
    const char* fn = "ndet_occupancy_bits";
    NDET_REQUIRE(alpha && count && bits, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(nx > 0 && ny > 0 && nz > 0, NDET_E_INVALID, "%s: bad sizes", fn);
    NDET_REQUIRE(dilate >= 0 && dilate <= 2, NDET_E_INVALID, "%s: dilate=%d must be 0, 1 or 2", fn, dilate);
    NDET_REQUIRE(std::isfinite(threshold), NDET_E_INVALID, "%s: threshold must be finite", fn);
    const int64_t total = (int64_t)nx * ny * nz;
    NDET_REQUIRE(total < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %lld voxels, must be fewer than 2^31", fn, (long long)total);
    NDET_REQUIRE(((uintptr_t)alpha & 3) == 0 && ((uintptr_t)count & 7) == 0 && ((uintptr_t)bits & 3) == 0, NDET_E_UNSUPPORTED,
                 "%s: misaligned pointer", fn);
    const int64_t blocks = (total + 255) / 256;
    NDET_REQUIRE(blocks <= ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: more than 2^24 workgroups", fn);
    hipLaunchKernelGGL(k_occupancy_bits, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, alpha, count, nx, ny, nz, (int)total,
                       threshold, dilate, bits, (int)((total + 31) / 32));
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ------------------------------------------------------------------------------------------------
// points against the bits.  A wave owns SE_WAVE_POINTS consecutive points (one "block of points": one kept count) and walks them 64 at
// a time in ascending order, so no wave needs another's counts: the 64 KiB of LDS are the bits' alone.
// ------------------------------------------------------------------------------------------------
#define SE_WAVE_POINTS 512
#define SE_LDS_BYTES (64 * 1024)

template <bool LDS, bool WRITE>
__global__ __launch_bounds__(256) void k_cull(const float* __restrict__ pts, int64_t n_points, const uint32_t* __restrict__ bits, int n_words,
                                              NdetLattice g, int keep_outside, int* __restrict__ block_count,
                                              const int* __restrict__ block_first, int* __restrict__ idx, float* __restrict__ pts_kept) {
    const uint32_t* b = ndet_stage_bits<LDS>(bits, n_words);
    const int lane = threadIdx.x & 63;
    const int64_t wb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // this wave's block of points
    const int64_t p0 = wb * SE_WAVE_POINTS;
    if (p0 >= n_points) return;                                           // wave-uniform, after the only barrier
    NdetCompact c = ndet_compact_begin<WRITE>(block_first, wb);
    for (int i = 0; i < SE_WAVE_POINTS; i += 64) {
        const int64_t p = p0 + i + lane;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        bool k = p < n_points;
        if (k) {
            x = pts[p * 3 + 0];
            y = pts[p * 3 + 1];
            z = pts[p * 3 + 2];
            k = ndet_grid_keep(x, y, z, g, b, keep_outside != 0);
        }
        const int64_t o = ndet_compact_step(c, k);
        if (WRITE && k) {
            idx[o] = (int)p;
            pts_kept[o * 3 + 0] = x;
            pts_kept[o * 3 + 1] = y;
            pts_kept[o * 3 + 2] = z;
        }
    }
    ndet_compact_end<WRITE>(c, block_count, wb);
}

static int se_cull_check(const char* fn, const float* pts, int64_t n_points, const uint32_t* bits, const int* n_voxels, const float* p0,
                         const float* vs, int outside, NdetLattice* g, int* n_words, int64_t* blocks) {
    NDET_REQUIRE(pts && bits && n_voxels && p0 && vs, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_points > 0, NDET_E_INVALID, "%s: bad sizes", fn);
    NDET_REQUIRE(outside == NDET_OUTSIDE_KEEP || outside == NDET_OUTSIDE_CULL, NDET_E_INVALID, "%s: outside=%d is neither keep nor cull", fn,
                 outside);
    int64_t total = 0;
    NDET_TRY(ndet_lattice_fill(fn, n_voxels[0], n_voxels[1], n_voxels[2], p0, vs, g, &total));
    NDET_REQUIRE(n_points < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %lld points, must be fewer than 2^31", fn, (long long)n_points);
    NDET_REQUIRE(((uintptr_t)pts & 3) == 0 && ((uintptr_t)bits & 3) == 0, NDET_E_UNSUPPORTED, "%s: misaligned pointer", fn);
    *n_words = (int)((total + 31) / 32);
    *blocks = (ndet_cull_blocks(n_points) + 3) / 4;
    NDET_REQUIRE(*blocks <= ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: more than 2^24 workgroups", fn);
    return NDET_OK;
}

template <bool WRITE>
static void se_cull_launch(int64_t blocks, int n_words, hipStream_t stream, const float* pts, int64_t n_points, const uint32_t* bits,
                           const NdetLattice& g, int outside, int* block_count, const int* block_first, int* idx, float* pts_kept) {
    const size_t lds = (size_t)n_words * sizeof(uint32_t);
    if (lds <= SE_LDS_BYTES)
        hipLaunchKernelGGL((k_cull<true, WRITE>), dim3((unsigned)blocks), dim3(256), lds, stream, pts, n_points, bits, n_words, g,
                           outside == NDET_OUTSIDE_KEEP, block_count, block_first, idx, pts_kept);
    else
        hipLaunchKernelGGL((k_cull<false, WRITE>), dim3((unsigned)blocks), dim3(256), 0, stream, pts, n_points, bits, n_words, g,
                           outside == NDET_OUTSIDE_KEEP, block_count, block_first, idx, pts_kept);
}

extern "C" int64_t ndet_cull_blocks(int64_t n_points) { return n_points > 0 ? (n_points + SE_WAVE_POINTS - 1) / SE_WAVE_POINTS : 0; }

extern "C" int ndet_cull_count(const float* pts, int64_t n_points, const uint32_t* bits, const int* n_voxels, const float* p0, const float* vs,
                               int outside, int* block_count, void* stream) {
    const char* fn = "ndet_cull_count";
    NdetLattice g;
    int n_words = 0;
    int64_t blocks = 0;
    NDET_TRY(se_cull_check(fn, pts, n_points, bits, n_voxels, p0, vs, outside, &g, &n_words, &blocks));
    NDET_REQUIRE(block_count, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(((uintptr_t)block_count & 3) == 0, NDET_E_UNSUPPORTED, "%s: misaligned pointer", fn);
    se_cull_launch<false>(blocks, n_words, (hipStream_t)stream, pts, n_points, bits, g, outside, block_count, nullptr, nullptr, nullptr);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_cull_write(const float* pts, int64_t n_points, const uint32_t* bits, const int* n_voxels, const float* p0, const float* vs,
                               int outside, const int* block_first, int* idx, float* pts_kept, void* stream) {
    const char* fn = "ndet_cull_write";
    NdetLattice g;
    int n_words = 0;
    int64_t blocks = 0;
    NDET_TRY(se_cull_check(fn, pts, n_points, bits, n_voxels, p0, vs, outside, &g, &n_words, &blocks));
    NDET_REQUIRE(block_first && idx && pts_kept, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(((uintptr_t)block_first & 3) == 0 && ((uintptr_t)idx & 3) == 0 && ((uintptr_t)pts_kept & 3) == 0, NDET_E_UNSUPPORTED,
                 "%s: misaligned pointer", fn);
    se_cull_launch<true>(blocks, n_words, (hipStream_t)stream, pts, n_points, bits, g, outside, nullptr, block_first, idx, pts_kept);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ------------------------------------------------------------------------------------------------
// the bank sampler's count pass alone.  Lanes over views in rounds of 64, the camera row in registers, as rb_project_round holds it
// (ray_stats_kernels.hip); a wave owns 64 consecutive samples, lane g keeps sample g's count and loads its point once (the sampler's
// wave-uniform loads read the same floats).  A sample's count is the popcount of the ballot of ndet_ray_project's mask over the views.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ray_count_bank(const float* __restrict__ pts, int64_t n_points, const NdetBankView* __restrict__ views,
                                                        int n_views, float img_h, float img_w, uint8_t* __restrict__ pixel_mask,
                                                        int* __restrict__ view_count) {
    const int lane = threadIdx.x & 63;
    const int64_t p_base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (p_base >= n_points) return;                            // wave-uniform
    const int64_t my_p = p_base + lane;
    const bool on = my_p < n_points;
    const float mx = on ? pts[my_p * 3 + 0] : 0.0f, my = on ? pts[my_p * 3 + 1] : 0.0f, mz = on ? pts[my_p * 3 + 2] : 0.0f;
    const int live = (int)min((int64_t)64, n_points - p_base);
    int cnt = 0;
    for (int v0 = 0; v0 < n_views; v0 += 64) {
        const int v = v0 + lane;
        float cam[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) cam[k] = v < n_views ? views[v].ke[k] : 0.0f;
        for (int gg = 0; gg < live; ++gg) {
            const float x = __shfl(mx, gg), y = __shfl(my, gg), z = __shfl(mz, gg);
            bool m = false;
            if (v < n_views) m = ndet_ray_project(cam, x, y, z, img_h, img_w).mask;
            const unsigned long long vb = __ballot(m);
            if (lane == gg) cnt += __popcll(vb);
        }
    }
    if (on) {
        pixel_mask[my_p] = cnt > 1 ? 1 : 0;                    // render_ray.py:301
        view_count[my_p] = cnt;
    }
}

extern "C" int ndet_ray_view_count_bank(const float* pts, int64_t n_points, const NdetBankView* views_dev, int n_views, float img_h, float img_w,
                                        uint8_t* pixel_mask, int* view_count, void* stream) {
    const char* fn = "ndet_ray_view_count_bank";
    NDET_REQUIRE(pts && views_dev && pixel_mask && view_count, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_points > 0 && n_views > 0, NDET_E_INVALID, "%s: bad sizes", fn);
    NDET_REQUIRE(n_points < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %lld points, must be fewer than 2^31", fn, (long long)n_points);
    NDET_REQUIRE(((uintptr_t)views_dev & 7) == 0, NDET_E_UNSUPPORTED, "%s: the view table must be 8-byte aligned", fn);
    NDET_REQUIRE(((uintptr_t)pts & 3) == 0 && ((uintptr_t)view_count & 3) == 0, NDET_E_UNSUPPORTED, "%s: misaligned pointer", fn);
    const int64_t blocks = (n_points + 255) / 256;
    NDET_REQUIRE(blocks <= ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: more than 2^24 workgroups", fn);
    hipLaunchKernelGGL(k_ray_count_bank, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pts, n_points, views_dev, n_views, img_h,
                       img_w, pixel_mask, view_count);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
