// The voxel lattice, the bit grid over it, ordered compaction and the segment table: what the occupancy, early-stop, carve and cloud
// kernels share (skip_empty_kernels.hip, early_stop_kernels.hip, carve_kernels.hip, cloud_kernels.hip).  Their features are contracts on
// bytes -- the live rays through a grid equal the cull, a cloud point's voxel is the cull's, a carved grid has ndet_occupancy_bits'
// format -- so each rule below is written once.  Compiled with -ffp-contract=off.
//
//   lattice   voxel n = (ix ny + iy) nz + iz of an (nx, ny, nz) lattice with first point p0 and spacing vs.  The nearest lattice point
//             of x is, per axis and in this fp32 statement order,   t = (x - p0) / vs + 0.5f;  i = (int)floorf(t).
//   bit grid  bit n & 31 of word n >> 5 for voxel n, (n_total + 31) / 32 words; one thread per voxel, so a wave's ballot is two whole
//             words (64 consecutive voxels).
#pragma once
#include "ndet_common.hpp"

#include <cmath>

struct NdetLattice {
    float p0[3], vs[3];
    int n[3];
};

// Axis j of the nearest lattice point: t (the cloud keeps t - fi, the offset within the cell), fi = floorf(t), and whether fi is on the
// lattice.  The range test runs on the floats (equal to the test on the ints wherever the cast is defined; NaN and +-inf fail it).
__device__ __forceinline__ bool ndet_lattice_cell(float x, const NdetLattice& g, int j, float& t, float& fi) {
    t = (x - g.p0[j]) / g.vs[j] + 0.5f;
    fi = floorf(t);
    return fi >= 0.0f && fi < (float)g.n[j];
}

// The flat index of the nearest lattice point of p, with every axis' t and fi; false (and n untouched) for a point that is not finite
// or off the lattice.
__device__ __forceinline__ bool ndet_lattice_index(const float (&p)[3], const NdetLattice& g, int* n, float (&t)[3], float (&fi)[3]) {
    bool inside = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) inside = ndet_lattice_cell(p[j], g, j, t[j], fi[j]) && isfinite(p[j]) && inside;
    if (inside) *n = ((int)fi[0] * g.n[1] + (int)fi[1]) * g.n[2] + (int)fi[2];
    return inside;
}

__device__ __forceinline__ bool ndet_lattice_index(float x, float y, float z, const NdetLattice& g, int* n) {
    const float p[3] = {x, y, z};
    float t[3], fi[3];
    return ndet_lattice_index(p, g, n, t, fi);
}

__device__ __forceinline__ bool ndet_bit(const uint32_t* bits, int n) { return (bits[n >> 5] >> (n & 31)) & 1u; }

// A point on the lattice is kept iff its voxel's bit is set, any other point iff keep_outside.
__device__ __forceinline__ bool ndet_grid_keep(float x, float y, float z, const NdetLattice& g, const uint32_t* bits, bool keep_outside) {
    int n;
    if (!ndet_lattice_index(x, y, z, g, &n)) return keep_outside;
    return ndet_bit(bits, n);
}

// Thread t of a one-thread-per-voxel launch holds voxel t's bit; every lane of the wave calls.
__device__ __forceinline__ void ndet_ballot_store_words(bool set, int64_t t, uint32_t* __restrict__ bits, int n_words) {
    const unsigned long long b = __ballot(set);
    const int64_t w = (t >> 6) * 2;                            // the wave's first word (t - lane is a multiple of 64)
    const int lane = threadIdx.x & 63;
    if (lane == 0 && w < n_words) bits[w] = (uint32_t)b;
    if (lane == 32 && w + 1 < n_words) bits[w + 1] = (uint32_t)(b >> 32);
}

// LDS: the workgroup (256 threads, all of them) copies the grid into its dynamic LDS, n_words * 4 bytes, and reads it there.
template <bool LDS>
__device__ __forceinline__ const uint32_t* ndet_stage_bits(const uint32_t* __restrict__ bits, int n_words) {
    extern __shared__ uint32_t s_bits[];
    if (!LDS) return bits;
    for (int i = threadIdx.x; i < n_words; i += 256) s_bits[i] = bits[i];
    __syncthreads();
    return s_bits;
}

// Whether pred(x, y, z, m) holds for any voxel m = (x ny + y) nz + z of voxel n's (2 dilate + 1)^3 neighbourhood, clamped to the
// lattice.  Stops at the first that does: pred has no side effects.
template <class Pred>
__device__ __forceinline__ bool ndet_any_neighbour(int n, int nx, int ny, int nz, int dilate, Pred pred) {
    const int iz = n % nz, iy = (n / nz) % ny, ix = n / (nz * ny);
    const int x0 = max(ix - dilate, 0), x1 = min(ix + dilate, nx - 1);
    const int y0 = max(iy - dilate, 0), y1 = min(iy + dilate, ny - 1);
    const int z0 = max(iz - dilate, 0), z1 = min(iz + dilate, nz - 1);
    bool any = false;
    for (int x = x0; x <= x1 && !any; ++x)
        for (int y = y0; y <= y1 && !any; ++y)
            for (int z = z0; z <= z1 && !any; ++z) any = pred(x, y, z, (x * ny + y) * nz + z);
    return any;
}

// Ordered compaction, two launches of one kernel around a prefix sum on the caller's side.  A wave owns block wb of consecutive elements
// (one kept count) and walks it 64 at a time in ascending order, so no wave needs another's counts: a step's ballot and a prefix
// popcount give a kept lane its output slot.  No atomics: the same bytes on every call.
//   count pass (WRITE = false)  block_count[wb] = how many of the block are kept;
//   write pass (WRITE = true)   block_first[wb] = the exclusive prefix sum of the counts; a kept lane writes at ndet_compact_step's slot.
struct NdetCompact {
    int64_t at;     // the slot of the step's first kept element
    int kept;
};

template <bool WRITE>
__device__ __forceinline__ NdetCompact ndet_compact_begin(const int* __restrict__ block_first, int64_t wb) {
    return NdetCompact{WRITE ? block_first[wb] : 0, 0};
}

// Every lane of the wave calls; the slot means something only to a lane whose k is true.
__device__ __forceinline__ int64_t ndet_compact_step(NdetCompact& c, bool k) {
    const unsigned long long m = __ballot(k);
    const int64_t o = c.at + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
    c.at += __popcll(m);
    c.kept += __popcll(m);
    return o;
}

template <bool WRITE>
__device__ __forceinline__ void ndet_compact_end(const NdetCompact& c, int* __restrict__ block_count, int64_t wb) {
    if (!WRITE && (threadIdx.x & 63) == 0) block_count[wb] = c.kept;
}

// Segment pointers riding in the kernel-argument block (512 bytes); entries beyond n_segs are null and never read.
struct NdetSegs {
    const uint32_t* seg[NDET_RING_MAX];
};

// ---- host side: NDET_OK, or the error code with the message set ----------------------------

// 1 .. NDET_RING_MAX segments, none null, each 4-byte aligned -> the table
static inline int ndet_segs_fill(const char* fn, const uint32_t* const* segments, int n_segs, NdetSegs* s) {
    NDET_REQUIRE(segments, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_segs >= 1 && n_segs <= NDET_RING_MAX, NDET_E_INVALID, "%s: %d segments, must be 1 .. %d", fn, n_segs, NDET_RING_MAX);
    *s = NdetSegs{};
    for (int j = 0; j < n_segs; ++j) {
        NDET_REQUIRE(segments[j], NDET_E_INVALID, "%s: null pointer (segment %d)", fn, j);
        NDET_REQUIRE(((uintptr_t)segments[j] & 3) == 0, NDET_E_UNSUPPORTED, "%s: misaligned pointer (segment %d)", fn, j);
        s->seg[j] = segments[j];
    }
    return NDET_OK;
}

// Three positive counts, fewer than 2^31 voxels in all, a finite origin and positive finite voxel sizes (p0, vs not null) -> the lattice
// and its voxel count
static inline int ndet_lattice_fill(const char* fn, int nx, int ny, int nz, const float* p0, const float* vs, NdetLattice* g, int64_t* total) {
    NDET_REQUIRE(nx > 0 && ny > 0 && nz > 0, NDET_E_INVALID, "%s: bad sizes", fn);
    const int n[3] = {nx, ny, nz};
    for (int k = 0; k < 3; ++k) {
        NDET_REQUIRE(std::isfinite(vs[k]) && vs[k] > 0.0f, NDET_E_INVALID, "%s: the voxel sizes must be positive and finite (axis %d)", fn, k);
        NDET_REQUIRE(std::isfinite(p0[k]), NDET_E_INVALID, "%s: the lattice origin must be finite (axis %d)", fn, k);
        g->p0[k] = p0[k];
        g->vs[k] = vs[k];
        g->n[k] = n[k];
    }
    *total = (int64_t)nx * ny * nz;
    NDET_REQUIRE(*total < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %lld voxels, must be fewer than 2^31", fn, (long long)*total);
    return NDET_OK;
}
