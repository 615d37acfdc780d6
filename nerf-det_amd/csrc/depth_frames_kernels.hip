// Depth frames on the device: the producer of the loader's `depth`, `gt_depths` and `depth_rays` (multi_view.py:98-105,156-166,
// render_ray.py:386-404) from the sensor's uint16 millimetre frames.
//
//   k_depth_frames       per selected frame and pixel of the crop [m, h - m) x [m, w - m) of the h x w resized map: the float64 branch of
//       datasets.imresize_linear(frame / 1000, (w, h)) bit for bit.  Each tap is double(u16) / 1000.0 (a correctly rounded division);
//       the positions are frame_tap.hpp's (float32(float64((d + 0.5) * (src / dst) - 0.5)), floor, both border clamps); the weight f is
//       that float32 widened, 1 - f is formed in float64; horizontal pass a * (1 - fx) + b * fx on the two source rows, vertical pass
//       h0 * (1 - fy) + h1 * fy.  The file is compiled with -ffp-contract=off: every product and every sum is rounded on its own.
//       Equal sizes give f = 0 on both axes and a * 1 + b * 0 = a: the copy the host function makes.
//
//   k_positive_indices   flatnonzero(x > 0) over a float64 array in ONE launch, ascending and reproducible: a single-pass scan over
//       tiles of 256 elements (one per thread).  A workgroup draws its tile from a ticket counter, so every tile before it belongs to a
//       workgroup that is already running; it counts its tile (ballot + popcount per wave), publishes the count, and sums the counts of
//       the tiles before it by looking back, a wave reading 64 status words at a time, until it meets a tile that has published its
//       inclusive prefix.  A status word is ONE aligned 8-byte granule {state, value}, written and read with relaxed agent-scope atomics
//       (the data is the flag: nothing else has to become visible).  No atomic decides where an index goes: the position of element i is
//       (positives before its tile) + (positives before it inside the tile), both sums of counts.  The ticket and the status words are
//       zeroed by a memset node in front of every launch.  Every wait is bounded: a workgroup that runs out of polls marks its tile
//       FAILED, the mark travels down the tiles after it, and the count comes out as -1 instead of a hang.
#include "ndet_common.hpp"
#include "frame_tap.hpp"

__global__ __launch_bounds__(256) void k_depth_frames(const uint16_t* __restrict__ frames, const int* __restrict__ ids, int n_sel, int Hd, int Wd,
                                                      int hc, int wc, int margin, double sy, double sx, double* __restrict__ out) {
    const int64_t hw = (int64_t)hc * wc;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sel * hw) return;
    const int v = (int)(i / hw);
    const int px = (int)(i - v * hw);                 // one crop holds fewer than 2^31 elements
    const int y = px / wc, x = px - y * wc;
    const FramePos ty = frame_pos(y + margin, sy, Hd), tx = frame_pos(x + margin, sx, Wd);
    const uint16_t* src = frames + (int64_t)(ids ? ids[v] : v) * Hd * Wd;   // one frame holds fewer than 2^31 elements
    const double a = (double)src[ty.s0 * Wd + tx.s0] / 1000.0, b = (double)src[ty.s0 * Wd + tx.s1] / 1000.0;
    const double c = (double)src[ty.s1 * Wd + tx.s0] / 1000.0, d = (double)src[ty.s1 * Wd + tx.s1] / 1000.0;
    const double fx = (double)tx.f, fy = (double)ty.f;
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    const double h0 = a * gx + b * fx;                // un-fused (see above)
    const double h1 = c * gx + d * fx;
    out[i] = h0 * gy + h1 * fy;
}

extern "C" int ndet_depth_frames(const uint16_t* frames_mm, const int* ids, int n_sel, int Hd, int Wd, int h, int w, int margin, double* out,
                                 void* stream) {
    const char* fn = "ndet_depth_frames";
    NDET_REQUIRE(frames_mm && out, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n_sel > 0 && Hd > 0 && Wd > 0 && h > 0 && w > 0, NDET_E_INVALID, "%s: sizes must be positive", fn);
    NDET_REQUIRE(margin >= 0 && 2 * (int64_t)margin < h && 2 * (int64_t)margin < w, NDET_E_INVALID, "%s: margin %d leaves no pixel of a %d x %d map", fn,
                 margin, h, w);
    const int hc = h - 2 * margin, wc = w - 2 * margin;
    NDET_REQUIRE((int64_t)Hd * Wd < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: a frame of %d x %d holds 2^31 elements or more", fn, Hd, Wd);
    NDET_REQUIRE((int64_t)hc * wc < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: a map of %d x %d holds 2^31 elements or more", fn, hc, wc);
    const int64_t blocks = ((int64_t)n_sel * hc * wc + 255) / 256;
    NDET_REQUIRE(blocks < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: %d maps of %d x %d need 2^31 workgroups or more", fn, n_sel, hc, wc);
    hipLaunchKernelGGL(k_depth_frames, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_mm, ids, n_sel, Hd, Wd, hc, wc, margin,
                       (double)Hd / (double)h, (double)Wd / (double)w, out);
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}

// ---- ordered compaction ----------------------------------------------------------------------------------------------------------
#define PI_TILE 256
// state of a tile's status word (bits 32-33; the value, a count below 2^31, is bits 0-31); 0 = nothing published yet
#define PI_COUNT 1ull    // value = positives of this tile
#define PI_PREFIX 2ull   // value = positives of this tile and of every tile before it
#define PI_FAILED 3ull   // a wait before this tile ran out of polls
#define PI_POLLS (1 << 22)   // per look-back window, each with an s_sleep: seconds, where a published word arrives within microseconds

__device__ __forceinline__ unsigned long long pi_word(unsigned long long state, int value) { return (state << 32) | (unsigned)value; }

__global__ __launch_bounds__(PI_TILE) void k_positive_indices(const double* __restrict__ x, int n, int64_t* __restrict__ idx, int64_t* __restrict__ count,
                                                              unsigned long long* ws /* [0] ticket, [1] unused, [2 + tile] status */) {
    __shared__ int s_tile, s_before, s_wave[PI_TILE / NDET_WAVE];
    const int tid = threadIdx.x, lane = tid & (NDET_WAVE - 1), wave = tid / NDET_WAVE;
    if (tid == 0) s_tile = (int)atomicAdd(reinterpret_cast<unsigned*>(ws), 1u);
    __syncthreads();
    const int tile = s_tile, n_tiles = (int)(((int64_t)n + PI_TILE - 1) / PI_TILE);
    const int64_t i = (int64_t)tile * PI_TILE + tid;
    const bool pos = i < n && x[i] > 0.0;
    const unsigned long long votes = __ballot(pos);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = 0, total = 0;            // positives of the tile in the waves before this one; in the whole tile
#pragma unroll
    for (int k = 0; k < PI_TILE / NDET_WAVE; ++k) {
        const int c = s_wave[k];
        before += k < wave ? c : 0;
        total += c;
    }
    unsigned long long* status = ws + 2;
    if (wave == 0) {
        if (lane == 0) __hip_atomic_store(status + tile, pi_word(tile == 0 ? PI_PREFIX : PI_COUNT, total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int sum = 0;                      // positives before this tile (lane-uniform)
        bool failed = false;
        for (int hi = tile - 1; hi >= 0 && !failed; hi -= NDET_WAVE) {   // window hi, hi - 1, .. hi - 63: the nearest tile on lane 0
            const int j = hi - lane;
            unsigned long long word = pi_word(PI_PREFIX, 0);             // in front of tile 0: an empty prefix
            for (int polls = 0;; ++polls) {
                if (j >= 0) word = __hip_atomic_load(status + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__all((word >> 32) != 0)) break;
                if (polls >= PI_POLLS) { failed = true; break; }         // lane-uniform
                __builtin_amdgcn_s_sleep(8);
            }
            if (failed || __any((word >> 32) == PI_FAILED)) { failed = true; break; }
            const unsigned long long closed = __ballot((word >> 32) == PI_PREFIX);
            const int last = closed ? __ffsll((long long)closed) - 1 : NDET_WAVE - 1;   // the nearest tile that knows its prefix
            int part = lane <= last ? (int)(unsigned)word : 0;
#pragma unroll
            for (int o = NDET_WAVE / 2; o > 0; o >>= 1) part += __shfl_xor(part, o);
            sum += part;
            if (closed) break;
        }
        if (lane == 0) {
            if (tile > 0)
                __hip_atomic_store(status + tile, failed ? pi_word(PI_FAILED, 0) : pi_word(PI_PREFIX, sum + total), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            if (tile == n_tiles - 1) count[0] = failed ? -1 : (int64_t)sum + total;
            s_before = failed ? -1 : sum;
        }
    }
    __syncthreads();
    const int base = s_before;
    if (pos && base >= 0) idx[base + before + __popcll(votes & ((1ull << lane) - 1))] = i;
}

extern "C" int64_t ndet_positive_indices_workspace_bytes(int64_t n) {
    if (n <= 0 || n >= ((int64_t)1 << 31)) return 0;
    const int64_t words = 2 + (n + PI_TILE - 1) / PI_TILE;    // the ticket's 16-byte block, then a word per tile
    return ((words + 1) / 2) * 16;                            // zeroed whole: a multiple of 16 bytes
}

extern "C" int ndet_positive_indices(const double* x, int64_t n, int64_t* indices, int64_t* count, void* workspace, void* stream) {
    const char* fn = "ndet_positive_indices";
    NDET_REQUIRE(x && indices && count && workspace, NDET_E_INVALID, "%s: null pointer", fn);
    NDET_REQUIRE(n > 0, NDET_E_INVALID, "%s: n must be positive", fn);
    NDET_REQUIRE(n < ((int64_t)1 << 31), NDET_E_UNSUPPORTED, "%s: n = %lld: 2^31 elements or more", fn, (long long)n);
    NDET_REQUIRE(((uintptr_t)workspace & 15) == 0, NDET_E_INVALID, "%s: workspace must be 16-byte aligned", fn);
    const int64_t tiles = (n + PI_TILE - 1) / PI_TILE;
    const hipError_t e = hipMemsetAsync(workspace, 0, (size_t)ndet_positive_indices_workspace_bytes(n), (hipStream_t)stream);
    NDET_REQUIRE(e == hipSuccess, NDET_E_LAUNCH, "%s: cannot clear the workspace: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(k_positive_indices, dim3((unsigned)tiles), dim3(PI_TILE), 0, (hipStream_t)stream, x, (int)n, indices, count,
                       static_cast<unsigned long long*>(workspace));
    NDET_CHECK_LAUNCH(fn);
    return NDET_OK;
}
