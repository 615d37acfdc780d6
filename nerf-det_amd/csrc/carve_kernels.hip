// Space carving from depth frames for renders from a streamed scene (nerf-det_amd/streaming.py, begin_scene(carve=)), for gfx950:
//   * ndet_carve_accumulate  a chunk's k views -> per fine voxel a free count and a hit count, one 32-bit word (free in bits 0-15, hit in
//                            bits 16-31, each saturating at 65535), added into the caller's counter buffer;
//   * ndet_carve_bits        1 .. 64 counter segments -> the dilated bit grid ndet_cull_* / ndet_front_* read (the format of
//                            ndet_occupancy_bits), optionally ANDed with an undilated alpha grid on the parent (detection) lattice.
// The evidence of a view for a voxel is ndet_project_z (K2's stride-1 RGB projection) and the depth gate's own band test on the
// image-resolution map (ndet_depth_band): free | hit | behind partition the camera depths with no gap.  Integer counts: any chunking of
// the same views leaves the same bytes.  Plain vector stores, no atomics.  Compiled with -ffp-contract=off.
#include "grid_common.hpp"

#define CARVE_SAT 65535u

// ------------------------------------------------------------------------------------------------
// views -> counts.  One thread per fine voxel, z fastest: a wave reads 64 consecutive points and words, and the 64 voxels of a wave are
// one or a few z columns, which project onto short pixel runs of every view -- the gathers of a wave fall on neighbouring pixels.
// The view loop is inside the thread; v is wave-uniform, so a view's 12 floats are scalar loads from the device table.
// ------------------------------------------------------------------------------------------------
enum { CARVE_NONE = 0, CARVE_FREE = 1, CARVE_HIT = 2 };

// Evidence of view v at pixel (xi, yi) for camera depth z.  Call only where ndet_project_z accepted the pixel.  d = the map's value in
// its own dtype; !(d > 0): a hole, a negative or a NaN says nothing.  hit = ndet_depth_band; free = !(z > d - band), the same
// subtraction in the same dtype with the same rounding of band, so that free, hit and behind leave no gap.
__device__ __forceinline__ int carve_evidence(const NdetGateMap& g, int v, int xi, int yi, float z) {
    const int64_t o = (int64_t)v * g.view_pitch + (int64_t)yi * g.row_pitch + xi;
    bool free_;
    if (g.f64) {
        const double dv = static_cast<const double*>(g.map)[o];
        if (!(dv > 0.0)) return CARVE_NONE;
        free_ = !((double)z > dv - g.band);
    } else {
        const float dv = static_cast<const float*>(g.map)[o];
        if (!(dv > 0.0f)) return CARVE_NONE;
        free_ = !(z > dv - (float)g.band);
    }
    if (free_) return CARVE_FREE;
    return ndet_depth_band(g, v, xi, yi, z) ? CARVE_HIT : CARVE_NONE;
}

__device__ __forceinline__ uint32_t carve_add(uint32_t word, uint32_t free_, uint32_t hit) {
    const uint32_t f = min((word & 0xffffu) + min(free_, CARVE_SAT), CARVE_SAT);
    const uint32_t h = min((word >> 16) + min(hit, CARVE_SAT), CARVE_SAT);
    return f | (h << 16);
}

__global__ __launch_bounds__(256) void k_carve_accumulate(const float* __restrict__ pts, int N, const float* __restrict__ proj, int k,
                                                          NdetGateMap g, int H, int W, uint32_t* __restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const int n = (int)t;
    const float px = pts[n], py = pts[(int64_t)N + n], pz = pts[2 * (int64_t)N + n];
    uint32_t free_ = 0, hit = 0;
    for (int v = 0; v < k; ++v) {
        int xi, yi;
        float z;
        if (!ndet_project_z(proj + (int64_t)v * 12, px, py, pz, W, H, xi, yi, z)) continue;
        const int e = carve_evidence(g, v, xi, yi, z);
        free_ += e == CARVE_FREE;
        hit += e == CARVE_HIT;
    }
    counts[n] = carve_add(counts[n], free_, hit);      // the voxel's one read-modify-write of the launch
}

extern "C" int ndet_carve_accumulate(const float* points, int nx, int ny, int nz, const float* proj, int k, const void* depth, int dtype,
                                     int64_t view_pitch, int64_t row_pitch, int H, int W, double band, uint32_t* counts, void* stream) {
    const char* fn = "ndet_carve_accumulate";
    NDET_REQUIRE(points && proj && depth && counts, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(nx > 0 && ny > 0 && nz > 0 && k > 0 && H > 0 && W > 0, NDET_E_INVALID, "%s: bad sizes", fn);
    NDET_REQUIRE(dtype == 0 || dtype == 1, NDET_E_INVALID, "%s: depth dtype %d (0 = float32, 1 = float64)", fn, dtype);
    NDET_REQUIRE(band > 0.0 && band < 1e300, NDET_E_INVALID, "%s: band %g must be finite and > 0", fn, band);
    NDET_REQUIRE(row_pitch >= W && view_pitch >= (int64_t)H * row_pitch && row_pitch < ((int64_t)1 << 31), NDET_E_INVALID,
                 "%s: depth pitches smaller than the map", fn);
    const int64_t total = (int64_t)nx * ny * nz;
    NDET_REQUIRE(total < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %lld voxels, must be fewer than 2^31", fn, (long long)total);
    const int64_t blocks = (total + 255) / 256;
    NDET_REQUIRE(blocks <= ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: more than 2^24 workgroups", fn);
    NDET_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)proj & 3) == 0 && ((uintptr_t)counts & 3) == 0 &&
                     ((uintptr_t)depth % (dtype ? sizeof(double) : sizeof(float))) == 0,
                 NDET_E_UNSUPPORTED, "%s: misaligned pointer", fn);
    NdetGateMap g;
    g.map = depth;
    g.view_pitch = view_pitch;
    g.row_pitch = (int)row_pitch;
    g.f64 = dtype;
    g.band = band;
    hipLaunchKernelGGL(k_carve_accumulate, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, points, (int)total, proj, k, g, H, W,
                       counts);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ------------------------------------------------------------------------------------------------
// counts -> bits.  One thread per fine voxel; the bit grid and the segment table are grid_common.hpp's.
//   one pass    every thread sums the segments at each voxel of its (2 dilate + 1)^3 neighbourhood;
//   two passes  (scratch given, dilate > 0) the first launch writes the UNDILATED grid into scratch, the second dilates from those
//               bits: the segments are read once a voxel, the neighbourhood costs bit reads from a grid 1/32 the size of a segment.
// ------------------------------------------------------------------------------------------------
struct CarveGrid {
    int nx, ny, nz;
    int refine;                 // the parent lattice is (nx, ny, nz) / refine
    const uint32_t* coarse;     // undilated alpha bits on the parent lattice, or null
};

__device__ __forceinline__ bool carve_solid(const NdetSegs& s, int n_segs, uint32_t min_free, const CarveGrid& g, int x, int y, int z, int n) {
    uint32_t free_ = 0, hit = 0;
    for (int j = 0; j < n_segs; ++j) {
        const uint32_t w = s.seg[j][n];
        free_ += w & 0xffffu;
        hit += w >> 16;
    }
    bool solid = !(free_ >= min_free && hit == 0);       // unseen, behind a surface or on one
    if (g.coarse) {
        const int r = g.refine;
        const int p = ((x / r) * (g.ny / r) + y / r) * (g.nz / r) + z / r;
        solid = solid && ndet_bit(g.coarse, p);
    }
    return solid;
}

__global__ __launch_bounds__(256) void k_carve_bits(NdetSegs s, int n_segs, uint32_t min_free, int dilate, CarveGrid g, int n_total,
                                                    uint32_t* __restrict__ bits, int n_words) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool set = t < n_total && ndet_any_neighbour((int)t, g.nx, g.ny, g.nz, dilate, [&](int x, int y, int z, int m) {
                         return carve_solid(s, n_segs, min_free, g, x, y, z, m);
                     });
    ndet_ballot_store_words(set, t, bits, n_words);
}

__global__ __launch_bounds__(256) void k_carve_dilate(const uint32_t* __restrict__ solid, int nx, int ny, int nz, int n_total, int dilate,
                                                      uint32_t* __restrict__ bits, int n_words) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool set = t < n_total && ndet_any_neighbour((int)t, nx, ny, nz, dilate, [&](int, int, int, int m) { return ndet_bit(solid, m); });
    ndet_ballot_store_words(set, t, bits, n_words);
}

extern "C" int ndet_carve_bits(const uint32_t* const* segments, int n_segs, int min_free, int dilate, int nx, int ny, int nz,
                               const uint32_t* coarse_bits, int refine, uint32_t* scratch, uint32_t* bits, void* stream) {
    const char* fn = "ndet_carve_bits";
    NDET_REQUIRE(bits, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(nx > 0 && ny > 0 && nz > 0, NDET_E_INVALID, "%s: bad sizes", fn);
    NDET_REQUIRE(min_free >= 1, NDET_E_INVALID, "%s: min_free=%d must be at least 1", fn, min_free);
    NDET_REQUIRE(dilate >= 0 && dilate <= 2, NDET_E_INVALID, "%s: dilate=%d must be 0, 1 or 2", fn, dilate);
    NDET_REQUIRE(refine == 1 || refine == 2 || refine == 4, NDET_E_INVALID, "%s: refine=%d must be 1, 2 or 4", fn, refine);
    NDET_REQUIRE(!coarse_bits || (nx % refine == 0 && ny % refine == 0 && nz % refine == 0), NDET_E_INVALID,
                 "%s: the fine sizes (%d, %d, %d) must be multiples of refine=%d", fn, nx, ny, nz, refine);
    NdetSegs s;
    NDET_TRY(ndet_segs_fill(fn, segments, n_segs, &s));
    const int64_t total = (int64_t)nx * ny * nz;
    NDET_REQUIRE(total < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %lld voxels, must be fewer than 2^31", fn, (long long)total);
    const int64_t blocks = (total + 255) / 256;
    NDET_REQUIRE(blocks <= ((int64_t)1 << 24), NDET_E_UNSUPPORTED, "%s: more than 2^24 workgroups", fn);
    NDET_REQUIRE(((uintptr_t)bits & 3) == 0 && ((uintptr_t)coarse_bits & 3) == 0 && ((uintptr_t)scratch & 3) == 0, NDET_E_UNSUPPORTED,
                 "%s: misaligned pointer", fn);
    NDET_REQUIRE(scratch != bits, NDET_E_INVALID, "%s: scratch and bits must differ", fn);
    const CarveGrid g = {nx, ny, nz, refine, coarse_bits};
    const int n_words = (int)((total + 31) / 32);
    const bool two = scratch && dilate > 0;
    hipLaunchKernelGGL(k_carve_bits, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, s, n_segs, (uint32_t)min_free, two ? 0 : dilate,
                       g, (int)total, two ? scratch : bits, n_words);
    NDET_CHECK_LAUNCH(fn);
    if (two) {
        hipLaunchKernelGGL(k_carve_dilate, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, scratch, nx, ny, nz, (int)total, dilate,
                           bits, n_words);
        NDET_CHECK_LAUNCH(fn);
    }
    return NDET_OK;
}
