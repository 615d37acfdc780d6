// Early ray termination for renders from a streamed scene (nerf-det_amd/streaming.py, early_stop=), for gfx950: a ray's samples are
// walked front to back in segments of consecutive columns, and a ray whose transmittance has fallen below eps is left out from there on.
//   * ndet_ray_advance            the transmittance state: T[r] <- T[r] times the factors of columns [s0, s1), in k_composite's statements
//                                 (ray_kernels.hip), so that T[r] is k_composite's T_out[r, s1] bit for bit;
//   * ndet_front_count / _write   ordered compaction of the LIVE rays' samples of one segment, optionally through the occupancy grid of
//                                 skip_empty_kernels.hip in the same launch: the kept flat sample indices ascending, and their points, the
//                                 same bytes on every call (wave ballots and prefix popcounts, no atomics).
// A sample whose raw row stays zero is an exact no-op in k_composite (a = 0, wgt = 0, T (1 - 0 + 1e-10f) = T), so a stopped ray's T no
// longer moves and the ray stays stopped.  Plain vector stores only.  Compiled with -ffp-contract=off.
#include "grid_common.hpp"

// ------------------------------------------------------------------------------------------------
// T over one segment.  One lane per ray, the columns in ascending order, one store per ray.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ray_advance(const float* __restrict__ raw, float* __restrict__ T, int R, int S, int s0, int s1) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float t = T[r];
    for (int s = s0; s < s1; ++s) {
        const int64_t i = (int64_t)r * S + s;
        const float4 q = *reinterpret_cast<const float4*>(raw + i * 4);
        const float a = 1.0f - expf(-q.w);       // k_composite's two statements
        t = t * ((1.0f - a) + 1e-10f);
    }
    T[r] = t;
}

extern "C" int ndet_ray_advance(const float* raw, float* T, int R, int S, int s0, int s1, void* stream) {
    const char* fn = "ndet_ray_advance";
    NDET_REQUIRE(raw && T, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(R > 0 && S > 0, NDET_E_INVALID, "%s: bad sizes", fn);
    NDET_REQUIRE(s0 >= 0 && s1 <= S && s1 >= s0, NDET_E_INVALID, "%s: columns [%d, %d) of %d", fn, s0, s1, S);
    NDET_REQUIRE((int64_t)R * S < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %lld samples, must be fewer than 2^31", fn,
                 (long long)((int64_t)R * S));
    NDET_REQUIRE(((uintptr_t)raw & 15) == 0, NDET_E_UNSUPPORTED, "%s: raw must be 16-byte aligned (misaligned pointer)", fn);
    NDET_REQUIRE(((uintptr_t)T & 3) == 0, NDET_E_UNSUPPORTED, "%s: misaligned pointer", fn);
    const int64_t blocks = ((int64_t)R + 255) / 256;
    NDET_REQUIRE(blocks <= ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: more than 2^24 workgroups", fn);
    if (s0 == s1) return NDET_OK;
    hipLaunchKernelGGL(k_ray_advance, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, raw, T, R, S, s0, s1);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ------------------------------------------------------------------------------------------------
// the live rays' samples of one segment.  A segment of w columns has the nominal width wn = 4, 8, 16 or 32, the least of them that holds
// w; lane l of a wave step stands for column l % wn of ray l / wn of the step's 64 / wn consecutive rays (a lane whose column is w or
// more idles), so the lanes' order is the order of the flat sample indices.  A wave owns FS_WAVE_LANES / wn consecutive rays (one "block
// of rays": one kept count) and walks them in ascending order, so no wave needs another's counts: the LDS is the bits' alone.
// ------------------------------------------------------------------------------------------------
#define FS_WAVE_LANES 512
#define FS_LDS_BYTES (64 * 1024)
enum { FS_NO_GRID = 0, FS_GRID_LDS = 1, FS_GRID_GLOBAL = 2 };

static inline int fs_shift(int w) { return w <= 4 ? 2 : w <= 8 ? 3 : w <= 16 ? 4 : 5; }      // log2 of the nominal width, 1 <= w <= 32

template <int GRID, bool WRITE>
__global__ __launch_bounds__(256) void k_front(const float* __restrict__ pts, int R, int S, int s0, int w, int shift, const float* __restrict__ T,
                                               float eps, const uint32_t* __restrict__ bits, int n_words, NdetLattice g, int keep_outside,
                                               int* __restrict__ block_count, const int* __restrict__ block_first, int* __restrict__ idx,
                                               float* __restrict__ pts_kept) {
    const uint32_t* b = ndet_stage_bits<GRID == FS_GRID_LDS>(bits, n_words);
    const int lane = threadIdx.x & 63;
    const int64_t wb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // this wave's block of rays
    const int64_t r0 = wb * (FS_WAVE_LANES >> shift);
    if (r0 >= R) return;                                                  // wave-uniform, after the only barrier
    const int col = lane & ((1 << shift) - 1);
    NdetCompact c = ndet_compact_begin<WRITE>(block_first, wb);
    for (int i = 0; i < FS_WAVE_LANES; i += 64) {
        const int64_t r = r0 + ((i + lane) >> shift);
        const int64_t f = r * S + s0 + col;                               // below 2^31 wherever it is used (the host checks R S)
        bool k = r < R && col < w;
        if (k) k = !(T[r] < eps);                                         // fp32 compare; a NaN transmittance does not stop the ray
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (k && (WRITE || GRID != FS_NO_GRID)) {
            x = pts[f * 3 + 0];
            y = pts[f * 3 + 1];
            z = pts[f * 3 + 2];
        }
        if (GRID != FS_NO_GRID && k) k = ndet_grid_keep(x, y, z, g, b, keep_outside != 0);
        const int64_t o = ndet_compact_step(c, k);
        if (WRITE && k) {
            idx[o] = (int)f;
            pts_kept[o * 3 + 0] = x;
            pts_kept[o * 3 + 1] = y;
            pts_kept[o * 3 + 2] = z;
        }
    }
    ndet_compact_end<WRITE>(c, block_count, wb);
}

extern "C" int64_t ndet_front_blocks(int64_t R, int w) {
    if (R <= 0 || w < 1 || w > 32) return 0;
    const int64_t rays = FS_WAVE_LANES >> fs_shift(w);
    return (R + rays - 1) / rays;
}

static int fs_check(const char* fn, const float* pts, int R, int S, int s0, int s1, const float* T, float eps, const uint32_t* bits,
                    const int* n_voxels, const float* p0, const float* vs, int outside, NdetLattice* g, int* n_words, int64_t* blocks) {
    NDET_REQUIRE(pts && T, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(R > 0 && S > 0, NDET_E_INVALID, "%s: bad sizes", fn);
    NDET_REQUIRE(s0 >= 0 && s1 <= S && s1 > s0, NDET_E_INVALID, "%s: columns [%d, %d) of %d", fn, s0, s1, S);
    NDET_REQUIRE(eps >= 0.0f && eps < 1.0f, NDET_E_INVALID, "%s: eps must lie in [0, 1)", fn);      // a NaN fails both compares
    *n_words = 0;
    memset(g, 0, sizeof(*g));
    if (bits) {
        NDET_REQUIRE(n_voxels && p0 && vs, NDET_E_INVALID, "%s: null pointer", fn);
        NDET_REQUIRE(outside == NDET_OUTSIDE_KEEP || outside == NDET_OUTSIDE_CULL, NDET_E_INVALID, "%s: outside=%d is neither keep nor cull", fn,
                     outside);
        int64_t total = 0;
        NDET_TRY(ndet_lattice_fill(fn, n_voxels[0], n_voxels[1], n_voxels[2], p0, vs, g, &total));
        *n_words = (int)((total + 31) / 32);
    }
    NDET_REQUIRE(s1 - s0 <= 32, NDET_E_UNSUPPORTED, "%s: a segment of %d columns, at most 32", fn, s1 - s0);
    NDET_REQUIRE((int64_t)R * S < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %lld samples, must be fewer than 2^31", fn,
                 (long long)((int64_t)R * S));
    NDET_REQUIRE(((uintptr_t)pts & 3) == 0 && ((uintptr_t)T & 3) == 0 && ((uintptr_t)bits & 3) == 0, NDET_E_UNSUPPORTED, "%s: misaligned pointer",
                 fn);
    *blocks = (ndet_front_blocks(R, s1 - s0) + 3) / 4;
    NDET_REQUIRE(*blocks <= ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: more than 2^24 workgroups", fn);
    return NDET_OK;
}

template <bool WRITE>
static void fs_launch(int64_t blocks, int n_words, hipStream_t stream, const float* pts, int R, int S, int s0, int s1, const float* T, float eps,
                      const uint32_t* bits, const NdetLattice& g, int outside, int* block_count, const int* block_first, int* idx,
                      float* pts_kept) {
    const int w = s1 - s0, shift = fs_shift(w), keep = outside == NDET_OUTSIDE_KEEP;
    const size_t lds = (size_t)n_words * sizeof(uint32_t);
    const dim3 grid((unsigned)blocks), wg(256);
    if (!bits)
        hipLaunchKernelGGL((k_front<FS_NO_GRID, WRITE>), grid, wg, 0, stream, pts, R, S, s0, w, shift, T, eps, bits, 0, g, keep, block_count,
                           block_first, idx, pts_kept);
    else if (lds <= FS_LDS_BYTES)
        hipLaunchKernelGGL((k_front<FS_GRID_LDS, WRITE>), grid, wg, lds, stream, pts, R, S, s0, w, shift, T, eps, bits, n_words, g, keep,
                           block_count, block_first, idx, pts_kept);
    else
        hipLaunchKernelGGL((k_front<FS_GRID_GLOBAL, WRITE>), grid, wg, 0, stream, pts, R, S, s0, w, shift, T, eps, bits, n_words, g, keep,
                           block_count, block_first, idx, pts_kept);
}

extern "C" int ndet_front_count(const float* pts, int R, int S, int s0, int s1, const float* T, float eps, const uint32_t* bits,
                                const int* n_voxels, const float* p0, const float* vs, int outside, int* block_count, void* stream) {
    const char* fn = "ndet_front_count";
    NdetLattice g;
    int n_words = 0;
    int64_t blocks = 0;
    NDET_REQUIRE(block_count, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_TRY(fs_check(fn, pts, R, S, s0, s1, T, eps, bits, n_voxels, p0, vs, outside, &g, &n_words, &blocks));
    NDET_REQUIRE(((uintptr_t)block_count & 3) == 0, NDET_E_UNSUPPORTED, "%s: misaligned pointer", fn);
    fs_launch<false>(blocks, n_words, (hipStream_t)stream, pts, R, S, s0, s1, T, eps, bits, g, outside, block_count, nullptr, nullptr, nullptr);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

extern "C" int ndet_front_write(const float* pts, int R, int S, int s0, int s1, const float* T, float eps, const uint32_t* bits,
                                const int* n_voxels, const float* p0, const float* vs, int outside, const int* block_first, int* idx,
                                float* pts_kept, void* stream) {
    const char* fn = "ndet_front_write";
    NdetLattice g;
    int n_words = 0;
    int64_t blocks = 0;
    NDET_REQUIRE(block_first && idx && pts_kept, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_TRY(fs_check(fn, pts, R, S, s0, s1, T, eps, bits, n_voxels, p0, vs, outside, &g, &n_words, &blocks));
    NDET_REQUIRE(((uintptr_t)block_first & 3) == 0 && ((uintptr_t)idx & 3) == 0 && ((uintptr_t)pts_kept & 3) == 0, NDET_E_UNSUPPORTED,
                 "%s: misaligned pointer", fn);
    fs_launch<true>(blocks, n_words, (hipStream_t)stream, pts, R, S, s0, s1, T, eps, bits, g, outside, nullptr, block_first, idx, pts_kept);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
